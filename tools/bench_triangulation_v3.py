"""ops.triangulation_magnitude_moments (csrc/triangulation_moments.hip, csrc/triangulation_bn_moments.hip) on one MI355X: forward +
backward of one stream of JuhanTestModelV3's pooling two ways in ONE process, alternating, device-event times after a warm-up, median of
--reps, peak allocated memory of each.

  fused         TriangulationMagnitudeNsCnnIndirectAttentionModule.fused_pool (ops.triangulation_magnitude_moments) + backward of the
                two pools (forward and backward also timed apart; the op's launches through ops.KERNEL_TIMELINE in a separate set of
                repetitions)
  materialised  TriangulationMagnitudeNsCnnIndirectAttentionModule.pool: the embedding, its normalised rolled differences, the Grams,
                the rectified convolutions and the moments in torch, autograd -- [(B*T), K*D] tensors
  shapes        (B, T, D, K, F) = (16, 200, 1024, 32, 64) and (16, 200, 128, 8, 16), the model's two streams at its defaults

No ratio is asked for; FLAGS.triangulation_v3_fused defaults to on only if the fused path is not slower at both shapes.  The FLOP count
set against the 157.3 TFLOP/s fp32 matrix peak is the pooling's own, not the kernels': two Grams and two M V products of 2 B T^2 K D each
and six convolution-sized products (two forward, two weight gradients, two input gradients) of 2 B T K F D each.  (The chain forms the
temporal M V and input-gradient products three times and the spatial ones twice: one sweep per dot product that must be complete.)

  python tools/bench_triangulation_v3.py [--reps 10] [--out profiles/bench_triangulation_v3.json]
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from learnablepoolingmethods_amd import ops, video_pooling_modules  # noqa: E402
from learnablepoolingmethods_amd import variables as vs  # noqa: E402

SHAPES = [(16, 200, 1024, 32, 64), (16, 200, 128, 8, 16)]      # B, T, D, K, F
GRADS = ("dx", "danchors", "dcnn_s", "dcnn_t")
PEAK_TFLOPS = 157.3                                             # fp32 matrix peak of one MI355X


def _inputs(B, T, D, K, F, dev):
    """L2-normalised frames, anchors 0.25 x orthonormal columns (the softmax away from one-hot), cnn weights at their initialiser's scale."""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B * T, D, generator=g)
    x = (x / x.norm(dim=1, keepdim=True)).to(dev).requires_grad_(True)
    qm, r = torch.linalg.qr(torch.randn(D, K, generator=g, dtype=torch.float64))
    anchors = (0.25 * qm * torch.sign(torch.diagonal(r))).float().to(dev).requires_grad_(True)
    cnn = [(torch.randn(K, F, D, generator=g) / math.sqrt(F * D)).to(dev).requires_grad_(True) for _ in range(2)]
    up = [torch.randn(B, 2 * (K * F + K), generator=g).to(dev) for _ in range(2)]
    return [x, anchors, *cnn], up


def _timed(fn):
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    z.record()
    return out, a, z


def _call(path, leaves, up, T):
    """-> (forward ms, backward ms, outputs)"""
    x, anchors, cnn_s, cnn_t = leaves
    D, K = anchors.shape
    store = vs.VariableStore(device=x.device)
    for name, v in (("anchor_weights", anchors), ("spatial_cnn_weights", cnn_s), ("temporal_cnn_weights", cnn_t)):
        store.vars[name], store.trainable[name] = v, True
    module = video_pooling_modules.TriangulationMagnitudeNsCnnIndirectAttentionModule(D, T, K, True, 1, cnn_s.shape[1], 1, False, True, True, True)

    def forward():
        with vs.use_store(store):
            return list(getattr(module, path)(x))
    for t in leaves:
        t.grad = None
    outs, a0, a1 = _timed(forward)
    _, b0, b1 = _timed(lambda: torch.autograd.backward(outs, up))
    torch.cuda.synchronize()
    return a0.elapsed_time(a1), b0.elapsed_time(b1), outs


def _stats(ts):
    return {"median_ms": round(statistics.median(ts), 4), "range_ms": [round(min(ts), 4), round(max(ts), 4)]}


def _breakdown(leaves, up, T, reps):
    per = {}
    for _ in range(reps):
        ops.KERNEL_TIMELINE = []
        try:
            _call("fused_pool", leaves, up, T)
            torch.cuda.synchronize()
            for name, _, t0, t1 in ops.KERNEL_TIMELINE:
                per.setdefault(name, []).append(t0.elapsed_time(t1))
        finally:
            ops.KERNEL_TIMELINE = None
    return {name: round(statistics.median(ts), 4) for name, ts in per.items()}


def _peak(path, leaves, up, T):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    for _ in range(2):                            # warm-up: code objects, allocator, library algorithm choices
        outs = _call(path, leaves, up, T)[2]
    grads = [t.grad.clone() for t in leaves]
    return round((torch.cuda.max_memory_allocated() - base) / 2**20, 1), [o.detach() for o in outs], grads


def bench(B, T, D, K, F, reps, dev):
    leaves, up = _inputs(B, T, D, K, F, dev)
    flop = 4 * 2 * B * T * T * K * D + 6 * 2 * B * T * K * F * D
    res = {"shape": {"B": B, "T": T, "D": D, "K": K, "F": F}, "reps": reps, "one_BT_KD_tensor_bytes": 4 * B * T * K * D, "flop": flop}
    res["fused_peak_allocated_MiB"], f_outs, f_grads = _peak("fused_pool", leaves, up, T)
    res["materialised_peak_allocated_MiB"], m_outs, m_grads = _peak("pool", leaves, up, T)
    res["fused_vs_materialised_max_abs_over_max_abs"] = {
        **{n: float((a - b).abs().max() / b.abs().max()) for n, a, b in zip(("spatial_pool", "temporal_pool"), f_outs, m_outs)},
        **{n: float((a - b).abs().max() / b.abs().max()) for n, a, b in zip(GRADS, f_grads, m_grads)}}
    del f_outs, f_grads, m_outs, m_grads
    times = {"fused": ([], []), "materialised": ([], [])}
    for _ in range(reps):
        for name, path in (("fused", "fused_pool"), ("materialised", "pool")):
            f, b, _ = _call(path, leaves, up, T)
            times[name][0].append(f)
            times[name][1].append(b)
    for name, (f, b) in times.items():
        res[name] = {"forward": _stats(f), "backward": _stats(b), "forward_backward": _stats([u + v for u, v in zip(f, b)])}
    res["fused_share_of_fp32_matrix_peak"] = round(flop / (res["fused"]["forward_backward"]["median_ms"] * 1e-3) / (PEAK_TFLOPS * 1e12), 4)
    res["materialised_over_fused"] = round(res["materialised"]["forward_backward"]["median_ms"] / res["fused"]["forward_backward"]["median_ms"], 2)
    res["fused_launches_ms"] = _breakdown(leaves, up, T, max(3, reps // 2))
    del leaves, up
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_triangulation_v3.py needs an MI355X: no GPU is visible")
    dev = torch.device("cuda:0")
    out = []
    for B, T, D, K, F in SHAPES:
        r = bench(B, T, D, K, F, a.reps, dev)
        print(json.dumps(r), flush=True)
        out.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        not_slower = all(r["materialised_over_fused"] >= 1.0 for r in out)
        with open(a.out, "w") as f:
            json.dump({"what": "tools/bench_triangulation_v3.py: forward + backward of one stream of JuhanTestModelV3's pooling, "
                               "TriangulationMagnitudeNsCnnIndirectAttentionModule.fused_pool (ops.triangulation_magnitude_moments) against .pool "
                               "(materialising), alternating in one process: time and peak allocated memory",
                       "measured": True, "device": torch.cuda.get_device_name(0), "fused_not_slower_at_both_model_default_shapes": not_slower,
                       "results": out}, f, indent=1)


if __name__ == "__main__":
    main()
