"""ops.triangulation_bn_moments (csrc/triangulation_bn_moments.hip) on one MI355X: forward + backward of one stream of JuhanTestModelV1's
pooling two ways in ONE process, alternating, device-event times, median of --reps, peak allocated memory of each.

  fused         TriangulationCnnIndirectAttentionModule.fused_pool (ops.triangulation_bn_moments and the moving-average update) +
                backward of the two pools (forward and backward also timed apart; the op's launches through ops.KERNEL_TIMELINE in a
                separate set of repetitions)
  materialised  TriangulationCnnIndirectAttentionModule.pool: the embedding, its rolled differences, both batch norms, the Grams and the
                moments in torch, autograd -- [(B*T), K*D] tensors
  shapes        (B, T, D, K) = (16, 30, 128, 16) and (16, 30, 1024, 64), the model's two streams at its defaults, and (80, 30, 1024, 64)

No ratio is asked for; FLAGS.triangulation_v1_fused defaults to on only if the fused path is not slower at both model-default shapes.

  python tools/bench_triangulation_v1.py [--reps 10] [--out profiles/bench_triangulation_v1.json]
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

SHAPES = [(16, 30, 128, 16), (16, 30, 1024, 64), (80, 30, 1024, 64)]      # B, T, D, K
GRADS = ("dx", "danchors", "dgamma_s", "dbeta_s", "dgamma_t", "dbeta_t")


def _inputs(B, T, D, K, dev):
    """L2-normalised frames, anchors N(0, 1/K), gamma = U(0.5, 1.5) / sqrt(J), beta = 0.1 N(0,1) / sqrt(J): the softmax away from one-hot."""
    g = torch.Generator().manual_seed(1)
    J = K * D
    x = torch.randn(B * T, D, generator=g)
    x = (x / x.norm(dim=1, keepdim=True)).to(dev).requires_grad_(True)
    anchors = (torch.randn(D, K, generator=g) / math.sqrt(K)).to(dev).requires_grad_(True)
    affine = []
    for _ in range(2):
        affine.append(((0.5 + torch.rand(J, generator=g)) / math.sqrt(J)).to(dev).requires_grad_(True))
        affine.append((0.1 * torch.randn(J, generator=g) / math.sqrt(J)).to(dev).requires_grad_(True))
    up = [torch.randn(B, 2 * J, generator=g).to(dev) for _ in range(2)]
    return [x, anchors, *affine], up


def _timed(fn):
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    z.record()
    return out, a, z


def _call(path, leaves, up, T):
    """-> (forward ms, backward ms, outputs)"""
    x, anchors, gamma_s, beta_s, gamma_t, beta_t = leaves
    D, K = anchors.shape
    J = K * D
    store = vs.VariableStore(device=x.device)
    store.vars["anchor_weights"], store.trainable["anchor_weights"] = anchors, True
    for scope, gamma, beta in (("spatial_bn", gamma_s, beta_s), ("temporal_bn", gamma_t, beta_t)):
        for name, v, tr in (("beta", beta, True), ("gamma", gamma, True), ("moving_mean", torch.zeros(J, device=x.device), False),
                            ("moving_variance", torch.ones(J, device=x.device), False)):
            store.vars[f"{scope}/{name}"], store.trainable[f"{scope}/{name}"] = v, tr
    module = video_pooling_modules.TriangulationCnnIndirectAttentionModule(D, T, K, True, 1, 1, True, True, True)

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


def bench(B, T, D, K, reps, dev):
    leaves, up = _inputs(B, T, D, K, dev)
    res = {"shape": {"B": B, "T": T, "D": D, "K": K}, "reps": reps, "one_BT_KD_tensor_bytes": 4 * B * T * K * D}
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
        raise SystemExit("bench_triangulation_v1.py needs an MI355X: no GPU is visible")
    dev = torch.device("cuda:0")
    out = []
    for B, T, D, K in SHAPES:
        r = bench(B, T, D, K, a.reps, dev)
        print(json.dumps(r), flush=True)
        out.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        not_slower = all(r["materialised_over_fused"] >= 1.0 for r in out[:2])
        with open(a.out, "w") as f:
            json.dump({"measured": True, "device": torch.cuda.get_device_name(0), "fused_not_slower_at_both_model_default_shapes": not_slower,
                       "results": out}, f, indent=1)


if __name__ == "__main__":
    main()
