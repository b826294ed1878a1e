"""Evaluation-loop throughput (clips/s) at the shapes tools/bench_predict.py times, from synthetic uint8 reader batches with labels:

  predict    predictor.Predictor.predict alone, every batch
  evaluate   evaluation.evaluate(): predict + DeviceEvaluationMetrics.accumulate (lpm_eval_rows) every batch, get() at the end
  eval_util  predict + eval_util.EvaluationMetrics.accumulate (with evaluation.cross_entropy_rows as the loss) every batch, get() at the end

cfg-2 NetVladV1 B = 80, cfg-3 NetVladV2 B = 80, cfg-5 gated NetVladV1 B = 128 (bf16 storage); 300 frames of 1152 features per clip,
3862 classes, about 3 labels per clip.  Each loop runs --steps batches (rotating) between two device synchronisations and is timed on the
host clock; the three loops alternate --reps times after --warmup batches of each, and the median is printed.  The evaluate and
eval_util loops include their get() (get_ms: DeviceEvaluationMetrics.get alone over --steps batches).  The in-stream time of one
lpm_eval_rows launch at B = 80, V = 3862, k = 20 (device events around every launch; median of --kernel-reps) comes first.

  python tools/bench_eval.py [--configs cfg2,cfg3,cfg5] [--iterations 300] [--steps 20] [--warmup 5] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from learnablepoolingmethods_amd import FLAGS, eval_util, ops, registry  # noqa: E402
from learnablepoolingmethods_amd.evaluation import DeviceEvaluationMetrics, cross_entropy_rows, evaluate  # noqa: E402
from learnablepoolingmethods_amd.predictor import Predictor  # noqa: E402
from learnablepoolingmethods_amd.train import Trainer  # noqa: E402

CONFIGS = {
    "cfg2": dict(model="NetVladV1", B=80, kw=dict(cluster_size=256, hidden_size=512)),
    "cfg3": dict(model="NetVladV2", B=80, kw=dict(cluster_size=256, hidden_size=512)),
    "cfg5": dict(model="NetVladV1", B=128, kw=dict(cluster_size=512, hidden_size=1024, encoder=False), flags=dict(moe_num_mixtures=4,
                                                                                                              netvlad_storage="bf16")),
}
MAX_FRAMES, FEATURES, VOCAB, ROTATE = 300, 1152, 3862, 3


def _batches(B, dev, seed):
    """(ids, frames uint8, labels bool, num_frames) on the device, as evaluate() takes them from the reader."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for r in range(ROTATE):
        nf = torch.randint(MAX_FRAMES // 2, MAX_FRAMES + 1, (B,), generator=g, dtype=torch.int32)
        q = torch.randint(0, 256, (B, MAX_FRAMES, FEATURES), dtype=torch.uint8, generator=g)
        q[torch.arange(MAX_FRAMES).view(1, -1) >= nf.view(-1, 1)] = 0
        y = torch.rand(B, VOCAB, generator=g) < 3.0 / VOCAB
        out.append(([f"v{r}_{b}" for b in range(B)], q.to(dev), y.to(dev), nf.to(dev)))
    return out


def kernel_us(dev, reps):
    """In-stream time of one lpm_eval_rows launch at B = 80, V = 3862, k = 20 (with and without the loss), in microseconds."""
    g = torch.Generator().manual_seed(5)
    p = torch.rand(80, VOCAB, generator=g).to(dev)
    y = (torch.rand(80, VOCAB, generator=g) < 3.0 / VOCAB).to(dev)
    res = {}
    for with_loss in (True, False):
        for _ in range(10):
            ops.eval_rows(p, y, 20, with_loss)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for a, b in ev:
            a.record()
            ops.eval_rows(p, y, 20, with_loss)
            b.record()
        torch.cuda.synchronize()
        res["eval_rows_us" if with_loss else "eval_rows_no_loss_us"] = round(statistics.median(a.elapsed_time(b) for a, b in ev) * 1e3, 2)
    for _ in range(10):
        ops.topk_rows(p, 20)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        ops.topk_rows(p, 20)
        b.record()
    torch.cuda.synchronize()
    res["topk_rows_us"] = round(statistics.median(a.elapsed_time(b) for a, b in ev) * 1e3, 2)
    return res


def run(name, S, steps, warmup, reps, dev):
    c = CONFIGS[name]
    B = c["B"]
    try:
        for k, v in c.get("flags", {}).items():
            setattr(FLAGS, k, v)
        batches = _batches(B, dev, seed=4321 + S)
        tr = Trainer(registry.get_model(c["model"]), vocab_size=VOCAB, batch_size=B, device=dev, model_kwargs=dict(iterations=S, **c["kw"]))
        tr.build(batches[0][1], batches[0][3], batches[0][2].float())
        pr = Predictor.from_trainer(tr)
        del tr

        def stream(n):
            return (batches[i % ROTATE] for i in range(n))

        @torch.no_grad()
        def predict_loop(n):
            for _, q, _, nf in stream(n):
                pr.predict(q, nf)

        def evaluate_loop(n):
            evaluate(pr, stream(n), top_k=20)

        @torch.no_grad()
        def eval_util_loop(n):
            m = eval_util.EvaluationMetrics(VOCAB, 20)
            for _, q, y, nf in stream(n):
                p = pr.predict(q, nf)
                m.accumulate(p, y, cross_entropy_rows(p, y))
            m.get()

        loops = (("predict", predict_loop), ("evaluate", evaluate_loop), ("eval_util", eval_util_loop))
        for _, fn in loops:
            fn(warmup)
        torch.cuda.synchronize()
        times = {what: [] for what, _ in loops}
        for _ in range(reps):                                     # alternating: every rep runs all three loops on the same box
            for what, fn in loops:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(steps)
                torch.cuda.synchronize()
                times[what].append(time.perf_counter() - t0)
        res = {"config": name, "model": c["model"], "batch": B, "iterations": S, "steps": steps, "reps": reps}
        for what, ts in times.items():
            med = statistics.median(ts)
            res[what + "_ms_per_batch"] = round(med / steps * 1e3, 4)
            res[what + "_clips_per_s"] = round(B * steps / med, 1)
            res[what + "_clips_per_s_range"] = [round(B * steps / max(ts), 1), round(B * steps / min(ts), 1)]
        with torch.no_grad():                                     # the epoch reduction alone (get() over --steps batches)
            m = DeviceEvaluationMetrics(VOCAB, 20, dev)
            for _, q, y, nf in stream(steps):
                m.accumulate(pr.predict(q, nf), y)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.get()
            res["get_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        res["evaluate_overhead_pct"] = round((res["evaluate_ms_per_batch"] / res["predict_ms_per_batch"] - 1) * 100, 2)
        res["eval_util_overhead_pct"] = round((res["eval_util_ms_per_batch"] / res["predict_ms_per_batch"] - 1) * 100, 2)
        del pr
        return res
    finally:
        FLAGS.reset()
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--configs", default="cfg2,cfg3,cfg5")
    ap.add_argument("--iterations", default="300")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval.py needs an MI355X: no GPU is visible")
    dev = torch.device("cuda:0")
    k = {"kernel": "lpm_eval_rows", "batch": 80, "classes": VOCAB, "k": 20, **kernel_us(dev, a.kernel_reps)}
    print(json.dumps(k), flush=True)
    out = [k]
    for name in a.configs.split(","):
        for S in (int(s) for s in a.iterations.split(",")):
            r = run(name, S, a.steps, a.warmup, a.reps, dev)
            print(json.dumps(r), flush=True)
            out.append(r)
    print(f"{'config':6} {'S':>4} {'predict':>10} {'evaluate':>10} {'eval_util':>10}   (clips/s)")
    for r in out[1:]:
        print(f"{r['config']:6} {r['iterations']:4d} {r['predict_clips_per_s']:10.0f} {r['evaluate_clips_per_s']:10.0f} "
              f"{r['eval_util_clips_per_s']:10.0f}   evaluate {r['evaluate_overhead_pct']:+.2f} %, eval_util {r['eval_util_overhead_pct']:+.2f} %")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
