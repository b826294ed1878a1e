"""ops.triangulation_attention_pool (csrc/triangulation_attention.hip) against the materialising module path on one MI355X: forward +
backward of one stream's soft-attention pooled triangulation embedding, both ways in ONE process, alternating, device-event times,
median of --reps.

  fused         ops.triangulation_attention_pool(x, l2_normalize(anchors, 0), T) + backward of the four pooled vectors (forward and
                backward also timed apart; the op's own launches through ops.KERNEL_TIMELINE in a separate set of repetitions)
  materialised  TriangulationEmbedding -> TriangulationTemporalEmbedding -> IndirectClusterMaxMeanPoolModule on both, torch autograd:
                [B, T, K*D] tensors
  shapes        (B, T, D, K) = (16, 64, 1024, 128) and (16, 64, 128, 16) both ways; (80, 64, 1024, 128) and (16, 300, 1024, 16) fused only:
                one [B, T, K*D] fp32 tensor is 2.7 GB / 315 MB there and autograd keeps about eight alive (the result says how many bytes)

  python tools/bench_soft_attention.py [--reps 20] [--out profiles/bench_soft_attention.json]
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

from learnablepoolingmethods_amd import aggregation_modules, layers, ops, video_pooling_modules  # noqa: E402
from learnablepoolingmethods_amd import variables as vs  # noqa: E402

SHAPES = [  # B, T, D, K, with the materialised side
    (16, 64, 1024, 128, True),
    (16, 64, 128, 16, True),
    (80, 64, 1024, 128, False),
    (16, 300, 1024, 16, False),
]
MATERIALISED_TENSORS_ALIVE = 8     # e, its residual, f, its difference, the two weighted products and autograd's copies: measured below where it runs
NAMES = ("mean_d", "max_d", "mean_t", "max_t")


def _inputs(B, T, D, K, dev):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B * T, D, generator=g).to(dev).requires_grad_(True)
    anchors = (torch.randn(D, K, generator=g) / K ** 0.5).to(dev).requires_grad_(True)
    up = [torch.randn(B, K * D, generator=g).to(dev) for _ in range(4)]
    return x, anchors, up


def _timed(fn):
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    z.record()
    return out, a, z


def fused_call(x, anchors, up, T):
    """-> (forward ms, backward ms, outputs)"""
    x.grad = anchors.grad = None
    outs, a0, a1 = _timed(lambda: ops.triangulation_attention_pool(x, layers.l2_normalize(anchors, 0), T))
    _, b0, b1 = _timed(lambda: torch.autograd.backward(outs, up))
    torch.cuda.synchronize()
    return a0.elapsed_time(a1), b0.elapsed_time(b1), outs


def materialised_call(x, anchors, up, T):
    D, K = anchors.shape
    x.grad = anchors.grad = None
    store = vs.VariableStore(device=x.device)
    store.vars["anchor_weights"], store.trainable["anchor_weights"] = anchors, True
    pool = aggregation_modules.IndirectClusterMaxMeanPoolModule(l2_normalize=False)

    def forward():
        with vs.use_store(store):
            emb = video_pooling_modules.TriangulationEmbedding(D, T, K, None, True).forward(x)
            tmp = video_pooling_modules.TriangulationTemporalEmbedding(D, T, K, None, True).forward(emb)
        agg_d, agg_t = pool.forward(emb.reshape(-1, T, K * D)), pool.forward(tmp)
        n = K * D
        return [agg_d[:, :n], agg_d[:, n:], agg_t[:, :n], agg_t[:, n:]]
    outs, a0, a1 = _timed(forward)
    _, b0, b1 = _timed(lambda: torch.autograd.backward(outs, up))
    torch.cuda.synchronize()
    return a0.elapsed_time(a1), b0.elapsed_time(b1), outs


def _stats(ts):
    return {"median_ms": round(statistics.median(ts), 4), "range_ms": [round(min(ts), 4), round(max(ts), 4)]}


def _breakdown(x, anchors, up, T, reps):
    """The op's own launches (ops._timed sites), median ms per site over ``reps`` forward + backward calls."""
    per = {}
    for _ in range(reps):
        ops.KERNEL_TIMELINE = []
        try:
            fused_call(x, anchors, up, T)
            torch.cuda.synchronize()
            for name, _, t0, t1 in ops.KERNEL_TIMELINE:
                per.setdefault(name, []).append(t0.elapsed_time(t1))
        finally:
            ops.KERNEL_TIMELINE = None
    return {name: round(statistics.median(ts), 4) for name, ts in per.items()}


def bench(B, T, D, K, reps, dev, with_materialised):
    x, anchors, up = _inputs(B, T, D, K, dev)
    ways = [("fused", fused_call)] + ([("materialised", materialised_call)] if with_materialised else [])
    one = 4 * B * T * K * D
    res = {"shape": {"B": B, "T": T, "D": D, "K": K}, "reps": reps, "one_B_T_KD_tensor_bytes": one,
           "gram_flop": 2 * 2 * B * T * T * K * D, "backward_product_flop": 5 * 2 * B * T * T * K * D}
    if not with_materialised:
        res["materialised"] = {"measured": False, "why": f"one [B, T, K*D] fp32 tensor is {one / 2**20:.0f} MiB here and the module path keeps about "
                               f"{MATERIALISED_TENSORS_ALIVE} alive through its backward: about {MATERIALISED_TENSORS_ALIVE * one / 2**30:.1f} GiB"}
    keep = {}
    for name, fn in ways:                       # warm-up: code objects, allocator, library algorithm choices
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        for _ in range(3):
            keep[name] = fn(x, anchors, up, T)[2]
        keep[name + "_dx"], keep[name + "_da"] = x.grad.clone(), anchors.grad.clone()
        res[name + "_peak_allocated_MiB"] = round((torch.cuda.max_memory_allocated() - base) / 2**20, 1)
    if with_materialised:                       # faster and different is not faster: the two sides on the same inputs
        res["max_abs_difference"] = {n: float((a.detach() - b.detach()).abs().max()) for n, a, b in zip(NAMES, keep["fused"], keep["materialised"])}
        for key in ("dx", "da"):
            ref = keep["materialised_" + key]
            res["max_abs_difference"][key + "_over_max_abs"] = float((keep["fused_" + key] - ref).abs().max() / ref.abs().max())
        # dx: a Gram entry within rounding of zero may fall on either side of the relu in two fp32 evaluations (its dl[t] then enters or
        # leaves every frame's gradient) -- counted here; a maximum whose two best frames are within rounding of each other may go to
        # different frames (tools/bench_triangulation.py separates those rows; this tool does not)
        with torch.no_grad():
            grams = ops.triangulation_attention_gram(x, layers.l2_normalize(anchors, 0), T)
        res["gram_entries"] = int(sum(g.numel() for g in grams))
        res["gram_entries_within_1e-5_of_zero"] = int(sum((g.abs() < 1e-5).sum() for g in grams))
        res["gram_entries_within_1e-6_of_zero"] = int(sum((g.abs() < 1e-6).sum() for g in grams))
    keep.clear()
    times = {name: ([], []) for name, _ in ways}
    for _ in range(reps):
        for name, fn in ways:
            f, b, _ = fn(x, anchors, up, T)
            times[name][0].append(f)
            times[name][1].append(b)
    for name, (f, b) in times.items():
        res[name] = {"forward": _stats(f), "backward": _stats(b), "forward_backward": _stats([u + v for u, v in zip(f, b)])}
    if with_materialised:
        res["materialised_over_fused"] = round(res["materialised"]["forward_backward"]["median_ms"] / res["fused"]["forward_backward"]["median_ms"], 2)
    res["fused_launches_ms"] = _breakdown(x, anchors, up, T, max(3, reps // 2))
    gram_s = res["fused_launches_ms"]["triangulation_attention_gram"] * 1e-3
    bwd_s = res["fused_launches_ms"]["triangulation_attention_bwd"] * 1e-3
    res["gram_TFLOP_per_s"] = round(res["gram_flop"] / gram_s * 1e-12, 2)
    res["backward_product_TFLOP_per_s"] = round(res["backward_product_flop"] / bwd_s * 1e-12, 2)
    del x, anchors, up
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_soft_attention.py needs an MI355X: no GPU is visible")
    dev = torch.device("cuda:0")
    out = []
    for B, T, D, K, mat in SHAPES:
        r = bench(B, T, D, K, a.reps, dev, mat)
        print(json.dumps(r), flush=True)
        out.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"measured": True, "device": torch.cuda.get_device_name(0), "results": out}, f, indent=1)


if __name__ == "__main__":
    main()
