"""ops.triangulation_cnn_moments (csrc/triangulation_moments.hip) on one MI355X: forward + backward of one stream of JuhanTestModelV5's
pooling two ways in ONE process, alternating, device-event times, median of --reps.

  fused         ops.triangulation_cnn_moments(x, anchors, cnn_s, cnn_t, T) + backward of the two pools (forward and backward also timed
                apart; the op's two launches through ops.KERNEL_TIMELINE in a separate set of repetitions)
  materialised  TriangulationV5Module.pool: the embedding, its rolled differences, both convolutions and the moments in torch, autograd
                -- [B, T, K*D] tensors.  Run at --module-anchors (a reduced K, the result says which) where the full shape is not asked
                for with --module-full: the time per anchor is what is compared then
  shapes        (B, T, D, K, F) = (16, 30, 1024, 256, 512) and (16, 30, 128, 32, 64)

The fused video-stream time is set beside 3 x the forward FLOP count (2 products forward, 4 backward, each 2 B T K F D) over the fp32
matrix peak of 157.3 TFLOP/s.

  python tools/bench_triangulation_v5.py [--reps 10] [--module-anchors 64] [--module-full] [--out profiles/bench_triangulation_v5.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from learnablepoolingmethods_amd import ops, video_pooling_modules  # noqa: E402
from learnablepoolingmethods_amd import variables as vs  # noqa: E402

SHAPES = [(16, 30, 1024, 256, 512), (16, 30, 128, 32, 64)]      # B, T, D, K, F
FP32_MATRIX_PEAK = 157.3e12
GRADS = ("dx", "danchors", "dcnn_s", "dcnn_t")


def _inputs(B, T, D, K, F, dev):
    g = torch.Generator().manual_seed(1)
    init = vs.glorot_uniform_initializer()
    x = torch.randn(B * T, D, generator=g).to(dev).requires_grad_(True)
    anchors = init((D, K), torch.device("cpu"), g).to(dev).requires_grad_(True)
    cnn = [init((K, F, D), torch.device("cpu"), g).to(dev).requires_grad_(True) for _ in range(2)]
    up = [torch.randn(B, 2 * (K * F + K), generator=g).to(dev) for _ in range(2)]
    return [x, anchors, *cnn], up


def _timed(fn):
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    z.record()
    return out, a, z


def _call(forward, leaves, up):
    """-> (forward ms, backward ms, outputs)"""
    for t in leaves:
        t.grad = None
    outs, a0, a1 = _timed(forward)
    _, b0, b1 = _timed(lambda: torch.autograd.backward(outs, up))
    torch.cuda.synchronize()
    return a0.elapsed_time(a1), b0.elapsed_time(b1), outs


def fused_call(leaves, up, T):
    return _call(lambda: ops.triangulation_cnn_moments(*leaves, T), leaves, up)


def materialised_call(leaves, up, T):
    x, anchors, cnn_s, cnn_t = leaves
    D, K = anchors.shape
    F = cnn_s.shape[1]
    store = vs.VariableStore(device=x.device)
    for n, v in (("anchor_weights", anchors), ("spatial_cnn_weights", cnn_s), ("temporal_cnn_weights", cnn_t)):
        store.vars[n], store.trainable[n] = v, True

    def forward():
        with vs.use_store(store):
            return list(video_pooling_modules.TriangulationV5Module(D, T, K, False, 1, F, 1, True, True, True).pool(x))
    return _call(forward, leaves, up)


def _stats(ts):
    return {"median_ms": round(statistics.median(ts), 4), "range_ms": [round(min(ts), 4), round(max(ts), 4)]}


def _breakdown(leaves, up, T, reps):
    per = {}
    for _ in range(reps):
        ops.KERNEL_TIMELINE = []
        try:
            fused_call(leaves, up, T)
            torch.cuda.synchronize()
            for name, _, t0, t1 in ops.KERNEL_TIMELINE:
                per.setdefault(name, []).append(t0.elapsed_time(t1))
        finally:
            ops.KERNEL_TIMELINE = None
    return {name: round(statistics.median(ts), 4) for name, ts in per.items()}


def _peak(fn, leaves, up, T):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    for _ in range(2):                            # warm-up: code objects, allocator, library algorithm choices
        outs = fn(leaves, up, T)[2]
    grads = [t.grad.clone() for t in leaves]
    return round((torch.cuda.max_memory_allocated() - base) / 2**20, 1), [o.detach() for o in outs], grads


def bench(B, T, D, K, F, reps, dev, module_anchors, module_full):
    leaves, up = _inputs(B, T, D, K, F, dev)
    Km = K if module_full else min(K, module_anchors)
    flop = 2 * 2 * B * T * K * F * D
    res = {"shape": {"B": B, "T": T, "D": D, "K": K, "F": F}, "reps": reps, "one_B_T_KD_tensor_bytes": 4 * B * T * K * D,
           "forward_flop": flop, "module_anchors": Km}
    res["fused_peak_allocated_MiB"], f_outs, f_grads = _peak(fused_call, leaves, up, T)
    if Km == K:
        m_leaves, m_up = leaves, up
    else:                                          # the module path at a reduced K: the first Km anchors (its own inputs; times only)
        m_leaves, m_up = _inputs(B, T, D, Km, F, dev)
        res["materialised_note"] = (f"the module path runs at K = {Km} instead of {K}: one [B, T, K*D] tensor is {4 * B * T * K * D / 2**20:.0f} MiB at the "
                                    "full shape and autograd keeps several; its time is scaled by K / module_anchors for the ratio")
    res["materialised_peak_allocated_MiB"], m_outs, m_grads = _peak(materialised_call, m_leaves, m_up, T)
    if Km == K:
        res["fused_vs_materialised_max_abs_over_max_abs"] = {
            **{n: float((a - b).abs().max() / b.abs().max()) for n, a, b in zip(("spatial_pool", "temporal_pool"), f_outs, m_outs)},
            **{n: float((a - b).abs().max() / b.abs().max()) for n, a, b in zip(GRADS, f_grads, m_grads)}}
    del f_outs, f_grads, m_outs, m_grads
    times = {"fused": ([], []), "materialised": ([], [])}
    for _ in range(reps):
        for name, fn, lv, u in (("fused", fused_call, leaves, up), ("materialised", materialised_call, m_leaves, m_up)):
            f, b, _ = fn(lv, u, T)
            times[name][0].append(f)
            times[name][1].append(b)
    for name, (f, b) in times.items():
        res[name] = {"forward": _stats(f), "backward": _stats(b), "forward_backward": _stats([u + v for u, v in zip(f, b)])}
    fb = res["fused"]["forward_backward"]["median_ms"]
    res["materialised_scaled_to_K_ms"] = round(res["materialised"]["forward_backward"]["median_ms"] * K / Km, 4)
    res["materialised_over_fused"] = round(res["materialised_scaled_to_K_ms"] / fb, 2)
    res["fused_launches_ms"] = _breakdown(leaves, up, T, max(3, reps // 2))
    res["three_forward_flop_over_fp32_matrix_peak_ms"] = round(3 * flop / FP32_MATRIX_PEAK * 1e3, 4)
    res["fused_over_that_floor"] = round(fb / res["three_forward_flop_over_fp32_matrix_peak_ms"], 2)
    res["fused_TFLOP_per_s"] = round(3 * flop / (fb * 1e-3) * 1e-12, 2)
    del leaves, up, m_leaves, m_up
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--module-anchors", type=int, default=64)
    ap.add_argument("--module-full", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_triangulation_v5.py needs an MI355X: no GPU is visible")
    dev = torch.device("cuda:0")
    out = []
    for B, T, D, K, F in SHAPES:
        r = bench(B, T, D, K, F, a.reps, dev, a.module_anchors, a.module_full)
        print(json.dumps(r), flush=True)
        out.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"measured": True, "device": torch.cuda.get_device_name(0), "results": out}, f, indent=1)


if __name__ == "__main__":
    main()
