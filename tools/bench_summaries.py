"""What the TensorBoard summaries cost on one MI355X (summaries.SummaryWriter, lpm_histogram_segments):

  variables  one histogram per variable of a built trainer at cfg-2 / cfg-5 sizes, three ways, alternating in one process, median of --reps:
               kernel      ops.histogram_segments over the parameter arena alone, in-stream time between two device events
               writer      SummaryWriter.add_variables + flush(): both launches, the one copy to pinned memory, encoding, the file write
               torch       the torch formulation per variable -- torch.bucketize on the fp64 limits (right=True) + torch.bincount + min /
                           max / fp64 sum / fp64 sum of squares -- and ONE copy of all results to the host
  run        training.run over --steps resident uint8 batches with a writer (log_every 10, --histogram-steps) against the same run without
             one, alternating, median of --run-reps; steps/s and the difference

  python tools/bench_summaries.py [--configs cfg2,cfg5] [--reps 10] [--steps 200] [--histogram-steps 50] [--run-reps 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from learnablepoolingmethods_amd import FLAGS, ops, registry, summaries, training  # noqa: E402
from learnablepoolingmethods_amd.train import Trainer  # noqa: E402

CONFIGS = {
    "cfg2": dict(model="NetVladV1", B=80, kw=dict(cluster_size=256, hidden_size=512)),
    "cfg5": dict(model="NetVladV1", B=128, kw=dict(cluster_size=512, hidden_size=1024, encoder=False), flags=dict(moe_num_mixtures=4,
                                                                                                              netvlad_storage="bf16")),
}
MAX_FRAMES, FEATURES, VOCAB, ROTATE = 300, 1152, 3862, 3


def _batches(B, dev, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for r in range(ROTATE):
        nf = torch.randint(MAX_FRAMES // 2, MAX_FRAMES + 1, (B,), generator=g, dtype=torch.int32)
        q = torch.randint(0, 256, (B, MAX_FRAMES, FEATURES), dtype=torch.uint8, generator=g)
        q[torch.arange(MAX_FRAMES).view(1, -1) >= nf.view(-1, 1)] = 0
        y = torch.rand(B, VOCAB, generator=g) < 3.0 / VOCAB
        out.append(([f"v{r}_{b}" for b in range(B)], q.to(dev), y.to(dev), nf.to(dev)))
    return out


def _trainer(c, dev):
    return Trainer(registry.get_model(c["model"]), vocab_size=VOCAB, batch_size=c["B"], device=dev, seed=3,
                   model_kwargs=dict(iterations=MAX_FRAMES, **c["kw"]))


def torch_histograms(tensors, limits):
    """The torch formulation: per variable bucketize + bincount + four reductions; everything to the host in one copy."""
    L = limits.numel()
    out = []
    for t in tensors:
        d = t.detach().reshape(-1).to(torch.float64)
        counts = torch.bincount(torch.bucketize(d, limits, right=True).clamp_max(L - 1), minlength=L)
        out.append(torch.cat([counts.to(torch.float64), torch.stack([d.min(), d.max(), d.sum(), (d * d).sum()])]))
    return torch.cat(out).cpu()


def variables(name, reps, dev, tmp):
    c = CONFIGS[name]
    try:
        for k, v in c.get("flags", {}).items():
            setattr(FLAGS, k, v)
        b = _batches(c["B"], dev, 99)[0]
        tr = _trainer(c, dev)
        tr.build(b[1], b[3], b[2].float())
        arena = tr.arena
        lens = [arena.views[n].numel() for n in arena.names]
        starts = arena.offsets_host[:len(lens)]
        tensors = list(tr.store.vars.values())
        limits = torch.tensor(summaries.default_bucket_limits(), dtype=torch.float64, device=dev)
        writer = summaries.SummaryWriter(tmp)

        def kernel():
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ops.histogram_segments(arena.param, starts, lens)
            z.record()
            torch.cuda.synchronize()
            return a.elapsed_time(z) * 1e-3

        def through_writer():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            writer.add_variables(tr, 1)
            writer.flush()
            return time.perf_counter() - t0

        def through_torch():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            torch_histograms(tensors, limits)
            return time.perf_counter() - t0
        ways = (("kernel", kernel), ("writer", through_writer), ("torch", through_torch))
        for _, fn in ways:
            fn()
            fn()
        times = {w: [] for w, _ in ways}
        for _ in range(reps):
            for w, fn in ways:
                times[w].append(fn())
        writer.close()
        res = {"what": "variables", "config": name, "variables": len(tensors), "parameters": int(sum(lens)), "arena_floats": int(arena.total),
               "largest": int(max(lens)), "reps": reps}
        for w, ts in times.items():
            res[w + "_ms"] = round(statistics.median(ts) * 1e3, 3)
            res[w + "_ms_range"] = [round(min(ts) * 1e3, 3), round(max(ts) * 1e3, 3)]
        res["kernel_GB_per_s"] = round(4.0 * sum(lens) / statistics.median(times["kernel"]) * 1e-9, 1)
        res["torch_over_writer"] = round(res["torch_ms"] / res["writer_ms"], 2)
        del tr
        return res
    finally:
        FLAGS.reset()
        torch.cuda.empty_cache()


def run_loop(name, steps, histogram_steps, reps, dev, tmp):
    c = CONFIGS[name]
    try:
        for k, v in c.get("flags", {}).items():
            setattr(FLAGS, k, v)
        batches = _batches(c["B"], dev, 7)

        def one(with_writer, n):
            tr = _trainer(c, dev)
            w = summaries.SummaryWriter(tmp) if with_writer else None
            training.run(tr, (batches[i % ROTATE] for i in range(10)), log=lambda s: None)           # warm-up, no writer
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            training.run(tr, (batches[i % ROTATE] for i in range(n)), log=lambda s: None, summary_writer=w, histogram_steps=histogram_steps)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if w is not None:
                w.close()
            del tr
            torch.cuda.empty_cache()
            return dt
        times = {False: [], True: []}
        for _ in range(reps):
            for with_writer in (False, True):
                times[with_writer].append(one(with_writer, steps))
        plain, summ = statistics.median(times[False]), statistics.median(times[True])
        return {"what": "run", "config": name, "batch": c["B"], "steps": steps, "log_every": 10, "histogram_steps": histogram_steps, "reps": reps,
                "plain_steps_per_s": round(steps / plain, 2), "with_writer_steps_per_s": round(steps / summ, 2),
                "plain_s_range": [round(min(times[False]), 3), round(max(times[False]), 3)],
                "with_writer_s_range": [round(min(times[True]), 3), round(max(times[True]), 3)],
                "overhead_pct": round((summ / plain - 1) * 100, 2)}
    finally:
        FLAGS.reset()
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--configs", default="cfg2,cfg5")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--histogram-steps", type=int, default=50)
    ap.add_argument("--run-reps", type=int, default=3)
    ap.add_argument("--run-configs", default="cfg2")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_summaries.py needs an MI355X: no GPU is visible")
    dev = torch.device("cuda:0")
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        for name in [n for n in a.configs.split(",") if n]:
            r = variables(name, a.reps, dev, tmp)
            print(json.dumps(r), flush=True)
            out.append(r)
        for name in [n for n in a.run_configs.split(",") if n]:
            r = run_loop(name, a.steps, a.histogram_steps, a.run_reps, dev, tmp)
            print(json.dumps(r), flush=True)
            out.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
