"""ops.triangulation_cnn_pool (csrc/triangulation_mean.hip) on one MI355X: forward + backward of one stream of
TriangulationCnnClusterModel three ways in ONE process, alternating, device-event times, median of --reps.

  fused         ops.triangulation_cnn_pool(x, l2_normalize(anchors, 0), cnn_d, cnn_t, T) + backward of the two pooled vectors (forward and
                backward also timed apart; the op's own launches through ops.KERNEL_TIMELINE in a separate set of repetitions, among them
                the batched per-anchor projection)
  general       the same stream through ops.triangulation_attention_pool (both Grams, both maxima, the arg-max tensor, five M V products in
                the backward) with the same projection behind its two means: what the dedicated mean-only kernels save.  Its temporal
                mean carries softmax weights, so its numbers are not compared, only its time and memory
  materialised  TriangulationEmbedding -> TriangulationCnnModule -> IndirectClusterMeanPoolModule, TriangulationTemporalEmbedding ->
                TriangulationCnnModule -> MeanStdPoolModule, torch autograd: [B, T, K*D] and [B, T, K*F] tensors
  shapes        (B, T, D, K, F) = (16, 200, 1024, 128, 128) and (16, 200, 128, 32, 128) all ways; (80, 200, 1024, 128, 128) without the
                materialised side: one [B, T, K*D] fp32 tensor is 8.4 GB there (the result says how many bytes)

  python tools/bench_triangulation_cnn.py [--reps 20] [--out profiles/bench_triangulation_cnn.json]
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

SHAPES = [  # B, T, D, K, F, with the materialised side
    (16, 200, 1024, 128, 128, True),
    (16, 200, 128, 32, 128, True),
    (80, 200, 1024, 128, 128, False),
]
MATERIALISED_TENSORS_ALIVE = 8     # e, its residual, f, its difference, the transposed copies the convolutions read and autograd's copies
NAMES = ("agg_d", "agg_t")


def _inputs(B, T, D, K, F, dev):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B * T, D, generator=g).to(dev).requires_grad_(True)
    anchors = (torch.randn(D, K, generator=g) / K ** 0.5).to(dev).requires_grad_(True)
    cnn = [(torch.randn(K, F, D, generator=g) / (F * D) ** 0.5).to(dev).requires_grad_(True) for _ in range(2)]
    up = [torch.randn(B, K * F, generator=g).to(dev) for _ in range(2)]
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
    x, anchors, cnn_d, cnn_t = leaves
    return _call(lambda: ops.triangulation_cnn_pool(x, layers.l2_normalize(anchors, 0), cnn_d, cnn_t, T), leaves, up)


def _project(m, cnn):
    K, F, D = cnn.shape
    B = m.shape[0]
    return torch.bmm(m.view(B, K, D).transpose(0, 1), cnn.transpose(1, 2)).transpose(0, 1).reshape(B, K * F)


def general_call(leaves, up, T):
    x, anchors, cnn_d, cnn_t = leaves

    def forward():
        mean_d, _, mean_t, _ = ops.triangulation_attention_pool(x, layers.l2_normalize(anchors, 0), T)
        return [_project(mean_d, cnn_d), _project(mean_t, cnn_t)]
    return _call(forward, leaves, up)


def materialised_call(leaves, up, T):
    x, anchors, cnn_d, cnn_t = leaves
    D, K = anchors.shape
    F = cnn_d.shape[1]
    store = vs.VariableStore(device=x.device)
    for n, v in (("anchor_weights", anchors), ("d/cnn_weights", cnn_d), ("t/cnn_weights", cnn_t)):
        store.vars[n], store.trainable[n] = v, True

    def forward():
        with vs.use_store(store):
            emb = video_pooling_modules.TriangulationEmbedding(D, T, K, None, True).forward(x)
            with vs.variable_scope("d"):
                emb_cnn = video_pooling_modules.TriangulationCnnModule(D, T, F, K, None, True).forward(emb)
            agg_d = aggregation_modules.IndirectClusterMeanPoolModule(False).forward(emb.reshape(-1, T, K * D), emb_cnn)
            tmp = video_pooling_modules.TriangulationTemporalEmbedding(D, T, K, None, True).forward(emb)
            with vs.variable_scope("t"):
                tmp_cnn = video_pooling_modules.TriangulationCnnModule(D, T - 1, F, K, None, True).forward(tmp.reshape(-1, K * D))
        return [agg_d, aggregation_modules.MeanStdPoolModule(False).forward(tmp_cnn)]
    return _call(forward, leaves, up)


def _stats(ts):
    return {"median_ms": round(statistics.median(ts), 4), "range_ms": [round(min(ts), 4), round(max(ts), 4)]}


def _breakdown(fn, leaves, up, T, reps):
    """The ops' own launches (ops._timed sites), median ms per site over ``reps`` forward + backward calls."""
    per = {}
    for _ in range(reps):
        ops.KERNEL_TIMELINE = []
        try:
            fn(leaves, up, T)
            torch.cuda.synchronize()
            for name, _, t0, t1 in ops.KERNEL_TIMELINE:
                per.setdefault(name, []).append(t0.elapsed_time(t1))
        finally:
            ops.KERNEL_TIMELINE = None
    return {name: round(statistics.median(ts), 4) for name, ts in per.items()}


def bench(B, T, D, K, F, reps, dev, with_materialised):
    leaves, up = _inputs(B, T, D, K, F, dev)
    ways = [("fused", fused_call), ("general", general_call)] + ([("materialised", materialised_call)] if with_materialised else [])
    one = 4 * B * T * K * D
    res = {"shape": {"B": B, "T": T, "D": D, "K": K, "F": F}, "reps": reps, "one_B_T_KD_tensor_bytes": one,
           "gram_flop": 2 * B * T * T * K * D, "backward_product_flop": 2 * 2 * B * T * T * K * D, "projection_flop": 2 * 2 * B * K * D * F,
           "per_frame_convolution_flop": 2 * B * (2 * T - 1) * K * D * F}
    if not with_materialised:
        res["materialised"] = {"measured": False, "why": f"one [B, T, K*D] fp32 tensor is {one / 2**20:.0f} MiB here and the module path keeps about "
                               f"{MATERIALISED_TENSORS_ALIVE} alive through its backward: about {MATERIALISED_TENSORS_ALIVE * one / 2**30:.1f} GiB"}
    keep = {}
    for name, fn in ways:                       # warm-up: code objects, allocator, library algorithm choices
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        for _ in range(3):
            keep[name] = fn(leaves, up, T)[2]
        keep[name + "_grads"] = [t.grad.clone() for t in leaves]
        res[name + "_peak_allocated_MiB"] = round((torch.cuda.max_memory_allocated() - base) / 2**20, 1)
    if with_materialised:                       # faster and different is not faster: the two sides on the same inputs
        res["fused_vs_materialised_max_abs_over_max_abs"] = {
            n: float((a.detach() - b.detach()).abs().max() / b.detach().abs().max()) for n, a, b in zip(NAMES, keep["fused"], keep["materialised"])}
        for n, a, b in zip(("dx", "danchors", "dcnn_d", "dcnn_t"), keep["fused_grads"], keep["materialised_grads"]):
            res["fused_vs_materialised_max_abs_over_max_abs"][n] = float((a - b).abs().max() / b.abs().max())
        # dx: a Gram entry within rounding of zero may fall on either side of the relu in two fp32 evaluations (its dl[t] then enters or
        # leaves every frame's gradient) -- counted here
        with torch.no_grad():
            gram = ops.triangulation_mean_gram(leaves[0], layers.l2_normalize(leaves[1], 0), T)
        res["gram_entries"] = int(gram.numel())
        res["gram_entries_within_1e-5_of_zero"] = int((gram.abs() < 1e-5).sum())
        res["gram_entries_within_1e-6_of_zero"] = int((gram.abs() < 1e-6).sum())
        del gram
    keep.clear()
    times = {name: ([], []) for name, _ in ways}
    for _ in range(reps):
        for name, fn in ways:
            f, b, _ = fn(leaves, up, T)
            times[name][0].append(f)
            times[name][1].append(b)
    for name, (f, b) in times.items():
        res[name] = {"forward": _stats(f), "backward": _stats(b), "forward_backward": _stats([u + v for u, v in zip(f, b)])}
    fb = res["fused"]["forward_backward"]["median_ms"]
    res["general_over_fused"] = round(res["general"]["forward_backward"]["median_ms"] / fb, 2)
    if with_materialised:
        res["materialised_over_fused"] = round(res["materialised"]["forward_backward"]["median_ms"] / fb, 2)
    res["fused_launches_ms"] = _breakdown(fused_call, leaves, up, T, max(3, reps // 2))
    res["general_launches_ms"] = _breakdown(general_call, leaves, up, T, max(3, reps // 2))
    # the projection's forward only is a timed site; its backward is autograd's (three batched products): the rest of the fused time
    res["fused_projection_forward_share"] = round(res["fused_launches_ms"]["triangulation_cnn_projection"] / fb, 4)
    res["fused_time_outside_the_hip_launches_ms"] = round(fb - sum(v for k, v in res["fused_launches_ms"].items() if k != "triangulation_cnn_projection"), 4)
    res["gram_TFLOP_per_s"] = round(res["gram_flop"] / (res["fused_launches_ms"]["triangulation_mean_gram"] * 1e-3) * 1e-12, 2)
    res["backward_product_TFLOP_per_s"] = round(res["backward_product_flop"] / (res["fused_launches_ms"]["triangulation_mean_bwd"] * 1e-3) * 1e-12, 2)
    del leaves, up
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_triangulation_cnn.py needs an MI355X: no GPU is visible")
    dev = torch.device("cuda:0")
    out = []
    for B, T, D, K, F, mat in SHAPES:
        r = bench(B, T, D, K, F, a.reps, dev, mat)
        print(json.dumps(r), flush=True)
        out.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"measured": True, "device": torch.cuda.get_device_name(0), "results": out}, f, indent=1)


if __name__ == "__main__":
    main()
