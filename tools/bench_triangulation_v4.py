"""ops.triangulation_magnitude_frames (csrc/triangulation_moments.hip, csrc/triangulation_bn_moments.hip) on one MI355X: forward + backward
of one stream of JuhanTestModelV4 two ways in ONE process, alternating, device-event times after a warm-up, median of --reps, peak
allocated memory of each.

  features      the per-frame rows [relu(conv) | norm] of both NetVLADs and their backward from N(0,1) upstream gradients:
    fused         TriangulationMagnitudeNsCnnNetVladModule.fused_frames (ops.triangulation_magnitude_frames; forward and backward also timed
                  apart; the op's launches through ops.KERNEL_TIMELINE in a separate set of repetitions)
    materialised  TriangulationMagnitudeNsCnnNetVladModule.frames: the embedding, its normalised rolled differences and the rectified
                  convolutions in torch, autograd -- [(B*T), K*D] tensors
  module        the whole module either way: the features, both loupe_modules.NetVLAD (ops.netvlad + the projection) and the head, with
                256 clusters and the model's hidden / output widths, backward from an N(0,1) upstream gradient on its output
  shapes        (B, T, D, K, F) = (16, 200, 1024, 32, 64) and (16, 200, 128, 8, 16), the model's two streams at its defaults

No ratio is asked for; FLAGS.triangulation_v4_fused defaults to on only if the fused route is not slower at both shapes, features and
whole module alike.

  python tools/bench_triangulation_v4.py [--reps 10] [--out profiles/bench_triangulation_v4.json]
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

from learnablepoolingmethods_amd import loupe_modules, ops, video_pooling_modules  # noqa: E402
from learnablepoolingmethods_amd import variables as vs  # noqa: E402

SHAPES = [(16, 200, 1024, 32, 64, 2048, 2048), (16, 200, 128, 8, 16, 256, 256)]      # B, T, D, K, F, hidden, output
CLUSTERS = 256
GRADS = ("dx", "danchors", "dcnn_s", "dcnn_t")
CNN_NAMES = ("anchor_weights", "spatial_cnn_weights", "temporal_cnn_weights")


def _inputs(B, T, D, K, F, O, dev):
    """L2-normalised frames, anchors 0.25 x orthonormal columns, cnn weights at their initialiser's scale; upstream gradients for the
    (padded) feature matrices and for the module's output."""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B * T, D, generator=g)
    x = (x / x.norm(dim=1, keepdim=True)).to(dev).requires_grad_(True)
    qm, r = torch.linalg.qr(torch.randn(D, K, generator=g, dtype=torch.float64))
    anchors = (0.25 * qm * torch.sign(torch.diagonal(r))).float().to(dev).requires_grad_(True)
    cnn = [(torch.randn(K, F, D, generator=g) / math.sqrt(F * D)).to(dev).requires_grad_(True) for _ in range(2)]
    Wp = loupe_modules.padded_size(K * F + K, CLUSTERS)
    up = [torch.randn(B * Tz, Wp, generator=g).to(dev) for Tz in (T, T - 1)]
    return [x, anchors, *cnn], up, torch.randn(B, O, generator=g).to(dev)


def _timed(fn):
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    z.record()
    return out, a, z


class Stream:
    """One stream's module over a store that holds the benchmark's own leaves; the NetVLADs' and the head's variables are created by the
    first whole-module call and kept."""

    def __init__(self, leaves, T, F, H, O):
        x, anchors, cnn_s, cnn_t = leaves
        D, K = anchors.shape
        self.leaves, self.W = leaves, K * F + K
        self.store = vs.VariableStore(device=x.device, seed=2)
        for name, v in zip(CNN_NAMES, (anchors, cnn_s, cnn_t)):
            self.store.vars[name], self.store.trainable[name] = v, True
        self.module = video_pooling_modules.TriangulationMagnitudeNsCnnNetVladModule(D, T, K, True, H, F, O, False, True, True, True,
                                                                                      cluster_size=CLUSTERS)

    def call(self, path, up, whole):
        """-> (forward ms, backward ms, outputs); ``whole``: through the head, ``up`` the gradient of its output."""
        def forward():
            with vs.use_store(self.store):
                feats = getattr(self.module, path)(self.leaves[0])
                return [self.module.head(*feats)] if whole else list(feats)
        for t in list(self.leaves) + [v for v in self.store.vars.values() if v.requires_grad]:
            t.grad = None
        outs, a0, a1 = _timed(forward)
        ups = [up] if whole else [u[:, :o.shape[1]] for u, o in zip(up, outs)]
        _, b0, b1 = _timed(lambda: torch.autograd.backward(outs, ups))
        torch.cuda.synchronize()
        return a0.elapsed_time(a1), b0.elapsed_time(b1), outs

    def peak(self, path, up, whole):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        for _ in range(2):                            # warm-up: code objects, allocator, library algorithm choices
            outs = self.call(path, up, whole)[2]
        grads = [t.grad.clone() for t in self.leaves]
        return round((torch.cuda.max_memory_allocated() - base) / 2**20, 1), [o.detach() for o in outs], grads


def _stats(ts):
    return {"median_ms": round(statistics.median(ts), 4), "range_ms": [round(min(ts), 4), round(max(ts), 4)]}


def _breakdown(stream, up, reps):
    per = {}
    for _ in range(reps):
        ops.KERNEL_TIMELINE = []
        try:
            stream.call("fused_frames", up, False)
            torch.cuda.synchronize()
            for name, _, t0, t1 in ops.KERNEL_TIMELINE:
                per.setdefault(name, []).append(t0.elapsed_time(t1))
        finally:
            ops.KERNEL_TIMELINE = None
    return {name: round(statistics.median(ts), 4) for name, ts in per.items()}


def _compare(stream, up, whole, reps):
    res = {}
    res["fused_peak_allocated_MiB"], f_outs, f_grads = stream.peak("fused_frames", up, whole)
    res["materialised_peak_allocated_MiB"], m_outs, m_grads = stream.peak("frames", up, whole)
    W = stream.W
    names = ("output",) if whole else ("spatial_features", "temporal_features")
    res["fused_vs_materialised_max_abs_over_max_abs"] = {
        **{n: float((a[:, :b.shape[1]] - b).abs().max() / b.abs().max()) for n, a, b in zip(names, f_outs, m_outs)},
        **{n: float((a - b).abs().max() / b.abs().max()) for n, a, b in zip(GRADS, f_grads, m_grads)}}
    if not whole:
        res["padding_columns_max_abs"] = max(float(a[:, W:].abs().max()) if a.shape[1] > W else 0.0 for a in f_outs)
    del f_outs, f_grads, m_outs, m_grads
    times = {"fused": ([], []), "materialised": ([], [])}
    for _ in range(reps):
        for name, path in (("fused", "fused_frames"), ("materialised", "frames")):
            f, b, _ = stream.call(path, up, whole)
            times[name][0].append(f)
            times[name][1].append(b)
    for name, (f, b) in times.items():
        res[name] = {"forward": _stats(f), "backward": _stats(b), "forward_backward": _stats([u + v for u, v in zip(f, b)])}
    res["materialised_over_fused"] = round(res["materialised"]["forward_backward"]["median_ms"] / res["fused"]["forward_backward"]["median_ms"], 2)
    return res


def _against_torch(stream):
    """The module's output with both NetVLADs through ops.netvlad (padded widths) against the same with their torch formulation."""
    def output(pad_features):
        loupe_modules.NetVLAD.pad_features = pad_features
        try:
            with vs.use_store(stream.store), torch.no_grad():
                return stream.module.head(*stream.module.fused_frames(stream.leaves[0]))
        finally:
            loupe_modules.NetVLAD.pad_features = None
    a, b = output(None), output(False)
    return float((a - b).abs().max() / b.abs().max())


def bench(B, T, D, K, F, H, O, reps, dev):
    leaves, up, up_out = _inputs(B, T, D, K, F, O, dev)
    stream = Stream(leaves, T, F, H, O)
    res = {"shape": {"B": B, "T": T, "D": D, "K": K, "F": F, "clusters": CLUSTERS, "hidden": H, "output": O}, "reps": reps,
           "one_BT_KD_tensor_bytes": 4 * B * T * K * D, "feature_width": K * F + K, "netvlad_width": loupe_modules.padded_size(K * F + K, CLUSTERS),
           "netvlad_kernels": bool(loupe_modules.fused_ok(T, K * F + K, CLUSTERS) and loupe_modules.fused_ok(T - 1, K * F + K, CLUSTERS)),
           "hidden1_weights_bytes_each": 4 * CLUSTERS * (K * F + K) * H}
    res["features"] = _compare(stream, up, False, reps)
    res["features"]["fused_launches_ms"] = _breakdown(stream, up, max(3, reps // 2))
    stream.call("frames", up_out, True)               # creates the NetVLADs' and the head's variables: not part of either route's peak
    res["module"] = _compare(stream, up_out, True, reps)
    res["module"]["netvlad_kernels_vs_torch_formulation_max_abs_over_max_abs"] = _against_torch(stream)
    del stream, leaves, up
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_triangulation_v4.py needs an MI355X: no GPU is visible")
    dev = torch.device("cuda:0")
    out = []
    for B, T, D, K, F, H, O in SHAPES:
        r = bench(B, T, D, K, F, H, O, a.reps, dev)
        print(json.dumps(r), flush=True)
        out.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        not_slower = all(r[part]["materialised_over_fused"] >= 1.0 for r in out for part in ("features", "module"))
        with open(a.out, "w") as f:
            json.dump({"what": "tools/bench_triangulation_v4.py: forward + backward of one stream of JuhanTestModelV4, "
                               "TriangulationMagnitudeNsCnnNetVladModule.fused_frames (ops.triangulation_magnitude_frames) against .frames "
                               "(materialising), the features alone and the whole module (both NetVLADs and the head), alternating in one "
                               "process: time and peak allocated memory",
                       "measured": True, "device": torch.cuda.get_device_name(0), "fused_not_slower_at_both_model_default_shapes": not_slower,
                       "results": out}, f, indent=1)


if __name__ == "__main__":
    main()
