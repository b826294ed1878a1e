"""ops.triangulation_pool (csrc/triangulation_pool.hip) against the materialising module path on one MI355X: forward + backward of one
stream's pooled triangulation embedding, both ways in ONE process, alternating, device-event times, median of --reps.

  fused         ops.triangulation_pool(x, anchors, T, 1/sqrt(K)) + backward of the four pooled vectors (forward and backward also timed apart)
  materialised  WeightedTriangulationEmbedding -> TriangulationTemporalEmbedding -> MaxMeanPoolingModule on both, torch autograd:
                [B, T, K*D] tensors, ~10 GB alive at the video shape -- which is why this side never runs at B = 80
  shapes        video (B, 300, 1024, 64), audio (B, 300, 128, 64) at --batch (default 16); the fused op alone also at --fused-batch (80)

The byte counts in the result are algorithmic (computed from the shapes): the fused path reads the frames once per direction and writes
the pooled vectors, 4 B (T D + 4 K D) bytes forward; the materialised path writes and reads [B, T, K*D] about eight times forward.

  python tools/bench_triangulation.py [--batch 16] [--fused-batch 80] [--reps 20] [--out profiles/bench_triangulation.json]
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

from learnablepoolingmethods_amd import aggregation_modules, ops, video_pooling_modules  # noqa: E402
from learnablepoolingmethods_amd import variables as vs  # noqa: E402

T_FRAMES, ANCHORS = 300, 64


def _inputs(B, T, D, K, dev):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B * T, D, generator=g).to(dev).requires_grad_(True)
    anchors = (torch.randn(D, K, generator=g) / math.sqrt(K)).to(dev).requires_grad_(True)
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
    outs, a0, a1 = _timed(lambda: ops.triangulation_pool(x, anchors, T, scale=1 / math.sqrt(anchors.shape[1])))
    _, b0, b1 = _timed(lambda: torch.autograd.backward(outs, up))
    torch.cuda.synchronize()
    return a0.elapsed_time(a1), b0.elapsed_time(b1), outs


def materialised_call(x, anchors, up, T):
    D, K = anchors.shape
    x.grad = anchors.grad = None
    store = vs.VariableStore(device=x.device)
    store.vars["anchor_weights"], store.trainable["anchor_weights"] = anchors, True
    pool = aggregation_modules.MaxMeanPoolingModule(l2_normalize=False)

    def forward():
        with vs.use_store(store):
            emb, _ = video_pooling_modules.WeightedTriangulationEmbedding(D, T, K, None, True).forward(x)
            tmp = video_pooling_modules.TriangulationTemporalEmbedding(D, T, K, None, True).forward(emb)
        agg_d, agg_t = pool.forward(emb), pool.forward(tmp)
        n = K * D
        return [agg_d[:, :n], agg_d[:, n:], agg_t[:, :n], agg_t[:, n:]]
    outs, a0, a1 = _timed(forward)
    _, b0, b1 = _timed(lambda: torch.autograd.backward(outs, up))
    torch.cuda.synchronize()
    return a0.elapsed_time(a1), b0.elapsed_time(b1), outs


def _stats(ts):
    return {"median_ms": round(statistics.median(ts), 4), "range_ms": [round(min(ts), 4), round(max(ts), 4)]}


def bench(B, T, D, K, reps, dev, with_materialised):
    x, anchors, up = _inputs(B, T, D, K, dev)
    ways = [("fused", fused_call)] + ([("materialised", materialised_call)] if with_materialised else [])
    res = {"shape": {"B": B, "T": T, "D": D, "K": K}, "reps": reps,
           "fused_algorithmic_bytes_fwd": 4 * B * (T * D + 4 * K * D),
           "fused_algorithmic_bytes_bwd": 4 * B * (2 * T * D + 5 * K * D) + 4 * D * K,
           "materialised_algorithmic_bytes_fwd_at_least": 8 * 4 * B * T * K * D,
           "useful_flop_fwd": 10 * B * T * K * D}
    torch.cuda.reset_peak_memory_stats()
    keep = {}
    for name, fn in ways:                       # warm-up: code objects, allocator, library algorithm choices
        for _ in range(3):
            keep[name] = fn(x, anchors, up, T)[2]
        keep[name + "_dx"] = x.grad.clone()
    if with_materialised:                       # faster and different is not faster: the two sides on the same inputs
        res["max_abs_difference"] = {n: float((a.detach() - b.detach()).abs().max()) for n, a, b in
                                     zip(("max_d", "mean_d", "max_t", "mean_t"), keep["fused"], keep["materialised"])}
        # dx: two fp32 evaluations may give a maximum to different frames where the two best frames are within rounding of each other
        # (the upstream gradient of that one element then lands in another row): counted apart from the rounding-level differences
        diff = (keep["fused_dx"] - keep["materialised_dx"]).abs()
        scale = float(keep["materialised_dx"].abs().max())
        rerouted = diff > 1e-4 * scale
        res["max_abs_dx"] = scale
        res["max_abs_difference"]["dx"] = float(diff.max())
        res["max_abs_difference"]["dx_outside_rerouted_rows"] = float(diff[~rerouted.any(dim=1)].max())
        res["dx_rows_with_a_rerouted_maximum"] = int(rerouted.any(dim=1).sum())
        res["dx_rows"] = int(diff.shape[0])
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
    res["peak_allocated_MiB"] = round(torch.cuda.max_memory_allocated() / 2**20, 1)
    fwd_s = res["fused"]["forward"]["median_ms"] * 1e-3
    res["fused_forward_GB_per_s_algorithmic"] = round(res["fused_algorithmic_bytes_fwd"] / fwd_s * 1e-9, 1)
    res["fused_forward_GFLOP_per_s_useful"] = round(res["useful_flop_fwd"] / fwd_s * 1e-9, 1)
    del x, anchors, up
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--fused-batch", type=int, default=80)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.batch > 16:
        raise SystemExit("bench_triangulation.py: the materialised side needs ~10 GB at --batch 16 and grows with it; use --fused-batch for larger batches")
    if not torch.cuda.is_available():
        raise SystemExit("bench_triangulation.py needs an MI355X: no GPU is visible")
    dev = torch.device("cuda:0")
    out = []
    for B, D, mat in ((a.batch, 1024, True), (a.batch, 128, True), (a.fused_batch, 1024, False), (a.fused_batch, 128, False)):
        r = bench(B, T_FRAMES, D, ANCHORS, a.reps, dev, mat)
        print(json.dumps(r), flush=True)
        out.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"measured": True, "device": torch.cuda.get_device_name(0), "results": out}, f, indent=1)


if __name__ == "__main__":
    main()
