"""ops.class_filter (csrc/class_filter.hip) on one MI355X: the three glue stages of the class filter behind MoeModel2 / JuhanMoeModel,
forward + backward, two ways in ONE process, alternating, device-event times over --inner calls per window, median of --reps windows.

  fused   ops.class_filter: one launch forward, one backward per stage
  torch   video_level_models._filter_stage_torch on the GPU: the route FLAGS.class_filter_fused = False takes (autograd over ~25 small
          launches forward and more backward)
  stages  filter1  [B, 2V]: bias + leaky_relu + batch norm + keep mask
          residual [B, V]:  residual + leaky_relu + batch norm
          output   [B, V]:  bias + sigmoid
  shapes  (B, V) = (128, 3862) and (1024, 3862)
  step    one whole Trainer.step of MoeModel2 and of JuhanMoeModel on [B, 1152] video-level features, the flag on and off on the SAME
          trainer, alternating (host clock around a step that ends in a synchronise)

Beside the times: the bytes each stage must move (read a, the residual and the mask once, write y; backward: read dy, a, the residual
and the mask, write dpre) over the fused time.  No ratio is asked for; FLAGS.class_filter_fused defaults to on only if the fused route
is faster at both shapes.

  python tools/bench_class_filter.py [--reps 7] [--inner 20] [--out profiles/bench_class_filter.json]
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

from learnablepoolingmethods_amd import FLAGS, ops, registry, video_level_models  # noqa: E402
from learnablepoolingmethods_amd.train import Trainer  # noqa: E402

SHAPES = [(128, 3862), (1024, 3862)]          # B, V
FEATURES = 1152                               # mean_rgb + mean_audio
STAGES = {"filter1": dict(width=2, bias=True, residual=False, bn=True, keep=True, act="leaky_relu"),
          "residual": dict(width=1, bias=False, residual=True, bn=True, keep=False, act="leaky_relu"),
          "output": dict(width=1, bias=True, residual=False, bn=False, keep=False, act="sigmoid")}
KEEP_PROB = video_level_models.CLASS_FILTER_KEEP_PROB


def _stage_inputs(B, C, cfg, dev):
    g = torch.Generator(device=dev).manual_seed(1)
    t = dict(a=torch.randn(B, C, device=dev, generator=g).requires_grad_(True), bias=None, residual=None, bn=None, keep=None)
    if cfg["bias"]:
        t["bias"] = (0.1 * torch.randn(C, device=dev, generator=g)).requires_grad_(True)
    if cfg["residual"]:
        t["residual"] = torch.rand(B, C, device=dev, generator=g).requires_grad_(True)
    if cfg["bn"]:
        t["bn"] = ((1 + 0.1 * torch.randn(C, device=dev, generator=g)).requires_grad_(True),
                   (0.1 * torch.randn(C, device=dev, generator=g)).requires_grad_(True), torch.zeros(C, device=dev), torch.ones(C, device=dev))
    if cfg["keep"]:
        t["keep"] = (torch.rand(B, C, device=dev, generator=g) < KEEP_PROB).to(torch.uint8)
    return t, torch.randn(B, C, device=dev, generator=g)


def _stage_call(route, t, act):
    if route == "fused":
        return ops.class_filter(t["a"], t["bias"], t["residual"], act=act, bn=t["bn"], is_training=True, keep=t["keep"], keep_prob=KEEP_PROB)
    return video_level_models._filter_stage_torch(t["a"], t["bias"], t["residual"], act, t["bn"], True, t["keep"])


def _leaves(t):
    return [x for x in (t["a"], t["bias"], t["residual"]) + (t["bn"][:2] if t["bn"] else ()) if x is not None]


def _window(route, t, act, dy, inner):
    """-> (forward ms, backward ms) per call: `inner` forwards between two events, then `inner` backwards between two events"""
    leaves = _leaves(t)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    ev[0].record()
    ys = [_stage_call(route, t, act) for _ in range(inner)]
    ev[1].record()
    ev[2].record()
    for y in ys:
        torch.autograd.grad(y, leaves, dy)
    ev[3].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / inner, ev[2].elapsed_time(ev[3]) / inner


def _stats(ts):
    return {"median_ms": round(statistics.median(ts), 5), "range_ms": [round(min(ts), 5), round(max(ts), 5)]}


def bench_stage(name, B, V, reps, inner, dev):
    cfg = STAGES[name]
    C = V * cfg["width"]
    t, dy = _stage_inputs(B, C, cfg, dev)
    res = {"stage": name, "B": B, "C": C}
    outs = {}
    for route in ("fused", "torch"):                       # warm-up and the comparison of the two routes' results
        for _ in range(2):
            y = _stage_call(route, t, cfg["act"])
            grads = torch.autograd.grad(y, _leaves(t), dy)
        outs[route] = [y.detach()] + list(grads)
    res["fused_vs_torch_max_abs_over_max_abs"] = max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
                                                     for a, b in zip(outs["fused"], outs["torch"]))
    times = {"fused": ([], []), "torch": ([], [])}
    for _ in range(reps):
        for route in times:
            f, b = _window(route, t, cfg["act"], dy, inner)
            times[route][0].append(f)
            times[route][1].append(b)
    for route, (f, b) in times.items():
        res[route] = {"forward": _stats(f), "backward": _stats(b), "forward_backward": _stats([u + v for u, v in zip(f, b)])}
    res["torch_over_fused"] = round(res["torch"]["forward_backward"]["median_ms"] / res["fused"]["forward_backward"]["median_ms"], 3)
    n = B * C
    fwd_bytes = n * (4 + 4 + (4 if cfg["residual"] else 0) + (1 if cfg["keep"] else 0))
    bwd_bytes = n * (4 + 4 + 4 + (4 if cfg["residual"] else 0) + (1 if cfg["keep"] else 0))
    res["fused_forward_GBps_of_needed_bytes"] = round(fwd_bytes / res["fused"]["forward"]["median_ms"] / 1e6, 1)
    res["fused_backward_GBps_of_needed_bytes"] = round(bwd_bytes / res["fused"]["backward"]["median_ms"] / 1e6, 1)
    return res


def bench_step(model_name, B, V, reps, dev):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, FEATURES, generator=g).to(dev)
    nf = torch.ones(B, dtype=torch.int32, device=dev)
    y = (torch.rand(B, V, generator=g) < 0.001).to(dev)
    saved = FLAGS.class_filter_fused
    try:
        tr = Trainer(registry.get_model(model_name), vocab_size=V, batch_size=B, device=dev, seed=1)
        times = {True: [], False: []}
        for flag in (True, False) * 2:                     # warm-up of both routes
            FLAGS.class_filter_fused = flag
            tr.step(x, nf, y)
        torch.cuda.synchronize()
        for _ in range(reps):
            for flag in times:
                FLAGS.class_filter_fused = flag
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tr.step(x, nf, y)
                torch.cuda.synchronize()
                times[flag].append((time.perf_counter() - t0) * 1e3)
    finally:
        FLAGS.class_filter_fused = saved
    res = {"model": model_name, "B": B, "V": V, "features": FEATURES, "fused": _stats(times[True]), "torch": _stats(times[False])}
    res["torch_over_fused"] = round(res["torch"]["median_ms"] / res["fused"]["median_ms"], 3)
    del tr
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_class_filter.py needs an MI355X: no GPU is visible")
    dev = torch.device("cuda:0")
    stages, steps = [], []
    for B, V in SHAPES:
        for name in STAGES:
            stages.append(bench_stage(name, B, V, a.reps, a.inner, dev))
            print(json.dumps(stages[-1]), flush=True)
    for B, V in SHAPES:
        for model_name in ("MoeModel2", "JuhanMoeModel"):
            steps.append(bench_step(model_name, B, V, a.reps, dev))
            print(json.dumps(steps[-1]), flush=True)
    per_shape = {f"{B}x{V}": sum(s["fused"]["forward_backward"]["median_ms"] for s in stages if s["B"] == B)
                 < sum(s["torch"]["forward_backward"]["median_ms"] for s in stages if s["B"] == B) for B, V in SHAPES}
    summary = {"measured": True, "device": torch.cuda.get_device_name(0), "reps": a.reps, "inner": a.inner,
               "fused_faster_three_stages": per_shape, "fused_faster_at_both_shapes": all(per_shape.values()),
               "fused_step_not_slower": all(s["torch_over_fused"] >= 1.0 for s in steps), "stages": stages, "steps": steps}
    print(json.dumps({k: v for k, v in summary.items() if k not in ("stages", "steps")}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()
