"""ops.triangulation_onefc_pool (csrc/triangulation_onefc.hip) on one MI355X: forward + backward of one stream of JuhanTestModelV6's pooling
two ways in ONE process, alternating, device-event times after a warm-up, median of --reps, peak allocated memory of each.

  fused         TriangulationV6Module.fused_pool (the op; forward and backward also timed apart; the op's launches through
                ops.KERNEL_TIMELINE in a separate set of repetitions)
  materialised  TriangulationV6Module.pool: the embedding, its two normalisations, the batch norm and the attention in torch, autograd --
                [(B*T), K*D] tensors
  shapes        (B, T, D, K, C) = (16, 30, 128, 32, 8) (the audio stream at the model's defaults), (16, 30, 1024, 16, 8) and
                (80, 30, 1024, 16, 8); the backward starts from an N(0,1) gradient of the pooled rows [B, C*K*D]

No ratio is asked for; FLAGS.triangulation_v6_fused defaults to on only if the fused path is not slower at all three shapes.

  python tools/bench_triangulation_v6.py [--reps 10] [--out profiles/bench_triangulation_v6.json]
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

SHAPES = [(16, 30, 128, 32, 8), (16, 30, 1024, 16, 8), (80, 30, 1024, 16, 8)]      # B, T, D, K, C
NAMES = ("x", "anchor_weights", "spatial_bn/gamma", "spatial_bn/beta", "one_fc_attention_weight", "alpha", "beta")


def _inputs(B, T, D, K, C, dev):
    """N(0,1) frames, anchors 0.5 N(0,1), gamma ~ U(0.5, 1.5), beta ~ 0.1 N(0,1), W ~ 2 N(0,1) (attention neither flat nor saturated)"""
    g = torch.Generator().manual_seed(1)
    J = K * D
    leaves = [torch.randn(B * T, D, generator=g), 0.5 * torch.randn(D, K, generator=g), 0.5 + torch.rand(J, generator=g),
              0.1 * torch.randn(J, generator=g), 2.0 * torch.randn(J, C, generator=g), torch.ones(1), torch.full((1,), 0.01)]
    return [t.to(dev).requires_grad_(True) for t in leaves], torch.randn(B, C * J, generator=g).to(dev)


def _timed(fn):
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    z.record()
    return out, a, z


class Stream:
    """One stream's module over a store that holds the benchmark's own leaves"""

    def __init__(self, leaves, T, C):
        D, K = leaves[1].shape
        self.leaves = leaves
        self.store = vs.VariableStore(device=leaves[0].device, seed=2)
        for name, v in zip(NAMES[1:], leaves[1:]):
            self.store.vars[name], self.store.trainable[name] = v, True
        self.module = video_pooling_modules.TriangulationV6Module(D, T, K, False, 0, 0, 1, C, True, True, True)

    def call(self, path, up):
        """-> (forward ms, backward ms, pooled)"""
        for t in self.leaves:
            t.grad = None

        def forward():
            with vs.use_store(self.store):
                return getattr(self.module, path)(self.leaves[0])
        out, a0, a1 = _timed(forward)
        _, b0, b1 = _timed(lambda: torch.autograd.backward([out], [up]))
        torch.cuda.synchronize()
        return a0.elapsed_time(a1), b0.elapsed_time(b1), out

    def peak(self, path, up):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        for _ in range(2):                            # warm-up: code objects, allocator, library algorithm choices
            out = self.call(path, up)[2]
        grads = [t.grad.clone() for t in self.leaves]
        return round((torch.cuda.max_memory_allocated() - base) / 2**20, 1), out.detach(), grads


def _stats(ts):
    return {"median_ms": round(statistics.median(ts), 4), "range_ms": [round(min(ts), 4), round(max(ts), 4)]}


def _breakdown(stream, up, reps):
    per = {}
    for _ in range(reps):
        ops.KERNEL_TIMELINE = []
        try:
            stream.call("fused_pool", up)
            torch.cuda.synchronize()
            for name, _, t0, t1 in ops.KERNEL_TIMELINE:
                per.setdefault(name, []).append(t0.elapsed_time(t1))
        finally:
            ops.KERNEL_TIMELINE = None
    return {name: round(statistics.median(ts), 4) for name, ts in per.items()}


def bench(B, T, D, K, C, reps, dev):
    leaves, up = _inputs(B, T, D, K, C, dev)
    stream = Stream(leaves, T, C)
    res = {"shape": {"B": B, "T": T, "D": D, "K": K, "C": C}, "reps": reps, "one_BT_KD_tensor_bytes": 4 * B * T * K * D,
           "pooled_bytes": 4 * B * C * K * D}
    res["fused_peak_allocated_MiB"], f_out, f_grads = stream.peak("fused_pool", up)
    res["materialised_peak_allocated_MiB"], m_out, m_grads = stream.peak("pool", up)
    res["fused_vs_materialised_max_abs_over_max_abs"] = {
        "pooled": float((f_out - m_out).abs().max() / m_out.abs().max()),
        **{"d " + n: float((a - b).abs().max() / b.abs().max()) for n, a, b in zip(NAMES, f_grads, m_grads)}}
    del f_out, f_grads, m_out, m_grads
    times = {"fused": ([], []), "materialised": ([], [])}
    for _ in range(reps):
        for name, path in (("fused", "fused_pool"), ("materialised", "pool")):
            f, b, _ = stream.call(path, up)
            times[name][0].append(f)
            times[name][1].append(b)
    for name, (f, b) in times.items():
        res[name] = {"forward": _stats(f), "backward": _stats(b), "forward_backward": _stats([u + v for u, v in zip(f, b)])}
    res["materialised_over_fused"] = round(res["materialised"]["forward_backward"]["median_ms"] / res["fused"]["forward_backward"]["median_ms"], 2)
    res["fused_launches_ms"] = _breakdown(stream, up, max(3, reps // 2))
    del stream, leaves, up
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_triangulation_v6.py needs an MI355X: no GPU is visible")
    dev = torch.device("cuda:0")
    out = []
    for B, T, D, K, C in SHAPES:
        r = bench(B, T, D, K, C, a.reps, dev)
        print(json.dumps(r), flush=True)
        out.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        not_slower = all(r["materialised_over_fused"] >= 1.0 for r in out)
        with open(a.out, "w") as f:
            json.dump({"what": "tools/bench_triangulation_v6.py: forward + backward of one stream of JuhanTestModelV6's pooling, "
                               "TriangulationV6Module.fused_pool (ops.triangulation_onefc_pool) against .pool (materialising), alternating "
                               "in one process: time and peak allocated memory",
                       "measured": True, "device": torch.cuda.get_device_name(0), "fused_not_slower_at_all_three_shapes": not_slower,
                       "results": out}, f, indent=1)


if __name__ == "__main__":
    main()
