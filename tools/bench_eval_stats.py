"""What FLAGS.eval_stats_fused (lpm_eval_batch_stats behind lpm_eval_rows) and evaluate(on_batch=...) cost or save, by tools/bench_eval.py's
method: every loop runs between two device synchronisations on the host clock, the routes alternate in one process, every shape is warmed
up first, every timed window runs at least --window seconds (the batch count is sized from a first timed run), the median of --reps is
reported.  The reference point of every time is the flag-off route: the code as it was before the flag existed, run in the same process.

  accumulate   DeviceEvaluationMetrics.accumulate(predictions, labels) alone at (B, V) = (80, 3862), (128, 3862), (1024, 3862), flag on
               against off (about three positives per row; the row buffers are reused, so no window pays for their growth)
  evaluate     evaluation.evaluate() against Predictor.predict alone (DESIGN.md section 12's comparison), flag off and on: NetVladV1 cfg-2
               (B = 80), cfg-5 (B = 128, bf16 storage) and MoeModel on [1024, 1152] video-level features
  on_batch     evaluate(on_batch=..., summary_writer=..., global_step=...) against evaluate(), same flag

  python tools/bench_eval_stats.py [--parts accumulate,evaluate] [--configs cfg2,cfg5,moe] [--reps 5] [--window 0.5] [--out profiles/bench_eval_stats.json]

--out UPDATES the file's keys for the parts that ran.  "eval_stats_fused_default" follows the project's rule: true only if the fused
accumulate is not slower at all three shapes."""
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

from learnablepoolingmethods_amd import FLAGS, registry, summaries  # noqa: E402
from learnablepoolingmethods_amd.evaluation import DeviceEvaluationMetrics, evaluate  # noqa: E402
from learnablepoolingmethods_amd.predictor import Predictor  # noqa: E402
from learnablepoolingmethods_amd.train import Trainer  # noqa: E402

VOCAB, ROTATE = 3862, 3
ACCUMULATE_SHAPES = ((80, VOCAB), (128, VOCAB), (1024, VOCAB))
CONFIGS = {
    "cfg2": dict(model="NetVladV1", B=80, kw=dict(iterations=300, cluster_size=256, hidden_size=512)),
    "cfg5": dict(model="NetVladV1", B=128, kw=dict(iterations=300, cluster_size=512, hidden_size=1024, encoder=False),
                 flags=dict(moe_num_mixtures=4, netvlad_storage="bf16")),
    "moe": dict(model="MoeModel", B=1024, kw={}),
}


def _timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(n)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _alternate(routes, reps, window, first=16):
    """routes: name -> fn(n batches).  -> (n, name -> the seconds per batch of every rep)."""
    for fn in routes.values():
        fn(first)                                                   # warm-up
    fastest = min(_timed(fn, first) for fn in routes.values()) / first
    n = max(first, int(window / fastest * 1.1) + 1)                 # every route's window is at least `window` long
    times = {name: [] for name in routes}
    for _ in range(reps):
        for name, fn in routes.items():
            t = _timed(fn, n)
            if t < window:                                          # (sized from the fastest route: this cannot happen by much)
                n2 = int(n * window / t * 1.1) + 1
                t, n_used = _timed(fn, n2), n2
            else:
                n_used = n
            times[name].append(t / n_used)
    return n, times


def _us(ts):
    return {"median_us": round(statistics.median(ts) * 1e6, 2), "range_us": [round(min(ts) * 1e6, 2), round(max(ts) * 1e6, 2)]}


def accumulate_part(dev, reps, window):
    out = []
    for B, V in ACCUMULATE_SHAPES:
        g = torch.Generator().manual_seed(B)
        data = [(torch.rand(B, V, generator=g).to(dev), (torch.rand(B, V, generator=g) < 3.0 / V).to(dev)) for _ in range(ROTATE)]
        metrics = {flag: DeviceEvaluationMetrics(V, 20, dev) for flag in (False, True)}

        def route(flag):
            def loop(n):
                FLAGS.eval_stats_fused = flag
                m = metrics[flag]
                for i in range(n):
                    if i % 64 == 0:
                        m.num_examples = 0                          # the row buffers are written again from their start
                    p, y = data[i % ROTATE]
                    m.accumulate(p, y)
            return loop
        try:
            n, times = _alternate({"unfused": route(False), "fused": route(True)}, reps, window)
        finally:
            FLAGS.reset()
        r = {"batch": B, "classes": V, "batches_per_window": n, "unfused": _us(times["unfused"]), "fused": _us(times["fused"])}
        r["fused_over_unfused"] = round(r["fused"]["median_us"] / r["unfused"]["median_us"], 4)
        r["fused_not_slower"] = r["fused"]["median_us"] <= r["unfused"]["median_us"]
        print(json.dumps(r), flush=True)
        out.append(r)
    return out


def _predictor(name, dev):
    c = CONFIGS[name]
    B = c["B"]
    g = torch.Generator().manual_seed(4321)
    batches = []
    for r in range(ROTATE):
        y = (torch.rand(B, VOCAB, generator=g) < 3.0 / VOCAB).to(dev)
        if c["model"] == "MoeModel":
            x, nf = torch.randn(B, 1152, generator=g).to(dev), torch.ones(B, dtype=torch.int32, device=dev)
        else:
            nf = torch.randint(150, 301, (B,), generator=g, dtype=torch.int32)
            x = torch.randint(0, 256, (B, 300, 1152), dtype=torch.uint8, generator=g)
            x[torch.arange(300).view(1, -1) >= nf.view(-1, 1)] = 0
            x, nf = x.to(dev), nf.to(dev)
        batches.append(([f"v{r}_{b}" for b in range(B)], x, y, nf))
    tr = Trainer(registry.get_model(c["model"]), vocab_size=VOCAB, batch_size=B, device=dev, model_kwargs=c["kw"])
    tr.build(batches[0][1], batches[0][3], batches[0][2].float())
    pr = Predictor.from_trainer(tr)
    del tr
    return pr, B, batches


def evaluate_part(name, dev, reps, window):
    c = CONFIGS[name]
    try:
        for k, v in c.get("flags", {}).items():
            setattr(FLAGS, k, v)
        pr, B, batches = _predictor(name, dev)
        tmp = tempfile.mkdtemp(prefix="bench_eval_stats_")
        writer = summaries.SummaryWriter(tmp)
        seen = []

        def stream(n):
            return (batches[i % ROTATE] for i in range(n))

        @torch.no_grad()
        def predict_loop(n):
            for _, x, _, nf in stream(n):
                pr.predict(x, nf)

        def evaluate_loop(flag, reporting):
            def loop(n):
                FLAGS.eval_stats_fused = flag
                if reporting:
                    del seen[:]
                    evaluate(pr, stream(n), top_k=20, summary_writer=writer, global_step=1, on_batch=lambda done, info: seen.append(done))
                    assert len(seen) == n
                else:
                    evaluate(pr, stream(n), top_k=20)
            return loop
        routes = {"predict": predict_loop, "evaluate_unfused": evaluate_loop(False, False), "evaluate_fused": evaluate_loop(True, False),
                  "evaluate_unfused_on_batch": evaluate_loop(False, True), "evaluate_fused_on_batch": evaluate_loop(True, True)}
        n, times = _alternate(routes, reps, window, first=8)
        writer.close()
        for f in os.listdir(tmp):
            os.remove(os.path.join(tmp, f))
        os.rmdir(tmp)
        r = {"config": name, "model": c["model"], "batch": B, "batches_per_window": n}
        for what, ts in times.items():
            r[what] = _us(ts)
        base = r["predict"]["median_us"]
        for what in routes:
            if what != "predict":
                r[what + "_over_predict_us"] = round(r[what]["median_us"] - base, 2)
                r[what + "_overhead_pct"] = round((r[what]["median_us"] / base - 1) * 100, 2)
        r["on_batch_cost_us"] = {"unfused": round(r["evaluate_unfused_on_batch"]["median_us"] - r["evaluate_unfused"]["median_us"], 2),
                                 "fused": round(r["evaluate_fused_on_batch"]["median_us"] - r["evaluate_fused"]["median_us"], 2)}
        print(json.dumps(r), flush=True)
        del pr
        return r
    finally:
        FLAGS.reset()
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parts", default="accumulate,evaluate")
    ap.add_argument("--configs", default="cfg2,cfg5,moe")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval_stats.py needs an MI355X: no GPU is visible")
    dev = torch.device("cuda:0")
    data = {}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            data = json.load(f)
    data["method"] = (f"loops between two synchronisations on the host clock, routes alternating in one process, median of {a.reps} windows of "
                      f"at least {a.window} s after a warm-up; the unfused route is the code as it was before FLAGS.eval_stats_fused")
    data["device"] = torch.cuda.get_device_name(0)
    parts = a.parts.split(",")
    if "accumulate" in parts:
        data["accumulate"] = accumulate_part(dev, a.reps, a.window)
        ok = all(s["fused_not_slower"] for s in data["accumulate"])
        data["eval_stats_fused_default"] = bool(ok)
        data["eval_stats_fused_default_reason"] = ("the fused accumulate is not slower at all three shapes" if ok else
                                                   "the fused accumulate is slower at: " + ", ".join(
                                                       f"({s['batch']}, {s['classes']})" for s in data["accumulate"] if not s["fused_not_slower"]))
    if "evaluate" in parts:
        done = {r["config"]: r for r in data.get("evaluate", [])}
        for name in a.configs.split(","):
            done[name] = evaluate_part(name, dev, a.reps, a.window)
        data["evaluate"] = list(done.values())
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(data, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
