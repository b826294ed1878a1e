"""ops.class_rows (csrc/class_rows.hip) on one MI355X: the two row stages of FishMoeModel3 and the two stages of the PN gate, forward +
backward, two ways in ONE process, alternating, device-event times over --inner calls per window, median of --reps windows.

  fused   ops.class_rows: one launch forward; backward one row-owned launch plus, with a bias or a layer norm, one column-owned launch
  torch   layers.class_rows_torch on the GPU: the route FLAGS.class_rows_fused = False takes (autograd over a dozen small launches)
  stages  layer_norm  [B, V]: bias + residual + LayerNorm          (FishMoeModel3, video_level_models.py:431-434)
          softmax     [B, V]: bias + softmax                       (:436)
          p_gate      [B, V]: relu6 + residual                     (PnGateModule, attention_modules.py:186-188)
          n_gate      [B, V]: -relu6(-t) + residual + softmax      (:191-196)
  shapes  (B, V) = (128, 3862) and (1024, 3862)
  step    one whole Trainer.step of FishMoeModel3 on [B, 1152] video-level features, the flag on and off on the SAME trainer,
          alternating (host clock around a step that ends in a synchronise)

Beside the times: the bytes each stage must move (forward: read a and the residual once, write y; backward: read dy, a, the residual,
y for a softmax, write da and, behind a gate, dresidual) over the fused time.  No ratio is asked for; FLAGS.class_rows_fused defaults to
on only if the fused route is faster at both shapes.

  python tools/bench_class_rows.py [--reps 7] [--inner 20] [--out profiles/bench_class_rows.json]
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

from learnablepoolingmethods_amd import FLAGS, layers, ops, registry  # noqa: E402
from learnablepoolingmethods_amd.train import Trainer  # noqa: E402

SHAPES = [(128, 3862), (1024, 3862)]          # B, V
FEATURES = 1152                               # mean_rgb + mean_audio
STAGES = {"layer_norm": dict(bias=True, residual=True, phi="identity", norm="layer_norm", model="FishMoeModel3"),
          "softmax": dict(bias=True, residual=False, phi="identity", norm="softmax", model="FishMoeModel3"),
          "p_gate": dict(bias=False, residual=True, phi="relu6", norm="none", model="PnGateModule"),
          "n_gate": dict(bias=False, residual=True, phi="neg_relu6", norm="softmax", model="PnGateModule")}


def _stage_inputs(B, C, cfg, dev):
    g = torch.Generator(device=dev).manual_seed(1)
    t = dict(a=(3 * torch.randn(B, C, device=dev, generator=g)).requires_grad_(True), bias=None, residual=None, ln=None)
    if cfg["bias"]:
        t["bias"] = (0.1 * torch.randn(C, device=dev, generator=g)).requires_grad_(True)
    if cfg["residual"]:
        t["residual"] = torch.rand(B, C, device=dev, generator=g).requires_grad_(True)
    if cfg["norm"] == "layer_norm":
        t["ln"] = ((1 + 0.1 * torch.randn(C, device=dev, generator=g)).requires_grad_(True),
                   (0.1 * torch.randn(C, device=dev, generator=g)).requires_grad_(True))
    return t, torch.randn(B, C, device=dev, generator=g)


def _stage_call(route, t, cfg):
    f = ops.class_rows if route == "fused" else layers.class_rows_torch
    return f(t["a"], t["bias"], t["residual"], cfg["phi"], cfg["norm"], t["ln"])


def _leaves(t):
    return [x for x in (t["a"], t["bias"], t["residual"]) + (t["ln"] or ()) if x is not None]


def _window(route, t, cfg, dy, inner):
    """-> (forward ms, backward ms) per call: `inner` forwards between two events, then `inner` backwards between two events"""
    leaves = _leaves(t)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    ev[0].record()
    ys = [_stage_call(route, t, cfg) for _ in range(inner)]
    ev[1].record()
    ev[2].record()
    for y in ys:
        torch.autograd.grad(y, leaves, dy)
    ev[3].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / inner, ev[2].elapsed_time(ev[3]) / inner


def _stats(ts):
    return {"median_ms": round(statistics.median(ts), 5), "range_ms": [round(min(ts), 5), round(max(ts), 5)]}


def bench_stage(name, B, C, reps, inner, dev):
    cfg = STAGES[name]
    t, dy = _stage_inputs(B, C, cfg, dev)
    res = {"stage": name, "model": cfg["model"], "B": B, "C": C}
    outs = {}
    for route in ("fused", "torch"):                       # warm-up and the comparison of the two routes' results
        for _ in range(2):
            y = _stage_call(route, t, cfg)
            grads = torch.autograd.grad(y, _leaves(t), dy)
        outs[route] = [y.detach()] + list(grads)
    res["fused_vs_torch_max_abs_over_max_abs"] = max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
                                                     for a, b in zip(outs["fused"], outs["torch"]))
    times = {"fused": ([], []), "torch": ([], [])}
    for _ in range(reps):
        for route in times:
            f, b = _window(route, t, cfg, dy, inner)
            times[route][0].append(f)
            times[route][1].append(b)
    for route, (f, b) in times.items():
        res[route] = {"forward": _stats(f), "backward": _stats(b), "forward_backward": _stats([u + v for u, v in zip(f, b)])}
    res["torch_over_fused"] = round(res["torch"]["forward_backward"]["median_ms"] / res["fused"]["forward_backward"]["median_ms"], 3)
    n = B * C
    gate = cfg["phi"] != "identity"
    fwd_bytes = n * 4 * (2 + (1 if cfg["residual"] else 0))
    bwd_bytes = n * 4 * (2 + (1 if gate or cfg["norm"] == "layer_norm" else 0) + (1 if cfg["norm"] == "layer_norm" else 0)
                         + (1 if cfg["norm"] == "softmax" else 0) + (1 if gate and cfg["residual"] else 0))
    res["fused_forward_GBps_of_needed_bytes"] = round(fwd_bytes / res["fused"]["forward"]["median_ms"] / 1e6, 1)
    res["fused_backward_GBps_of_needed_bytes"] = round(bwd_bytes / res["fused"]["backward"]["median_ms"] / 1e6, 1)
    return res


def bench_step(B, V, reps, dev):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, FEATURES, generator=g).to(dev)
    nf = torch.ones(B, dtype=torch.int32, device=dev)
    y = (torch.rand(B, V, generator=g) < 0.001).to(dev)
    saved = FLAGS.class_rows_fused
    try:
        tr = Trainer(registry.get_model("FishMoeModel3"), vocab_size=V, batch_size=B, device=dev, seed=1)
        times = {True: [], False: []}
        for flag in (True, False) * 2:                     # warm-up of both routes
            FLAGS.class_rows_fused = flag
            tr.step(x, nf, y)
        torch.cuda.synchronize()
        for _ in range(reps):
            for flag in times:
                FLAGS.class_rows_fused = flag
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tr.step(x, nf, y)
                torch.cuda.synchronize()
                times[flag].append((time.perf_counter() - t0) * 1e3)
    finally:
        FLAGS.class_rows_fused = saved
    res = {"model": "FishMoeModel3", "B": B, "V": V, "features": FEATURES, "fused": _stats(times[True]), "torch": _stats(times[False])}
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
        raise SystemExit("bench_class_rows.py needs an MI355X: no GPU is visible")
    dev = torch.device("cuda:0")
    stages, steps = [], []
    for B, V in SHAPES:
        for name in STAGES:
            stages.append(bench_stage(name, B, V, a.reps, a.inner, dev))
            print(json.dumps(stages[-1]), flush=True)
    for B, V in SHAPES:
        steps.append(bench_step(B, V, a.reps, dev))
        print(json.dumps(steps[-1]), flush=True)

    def total(route, B, model):
        return sum(s[route]["forward_backward"]["median_ms"] for s in stages if s["B"] == B and s["model"] == model)

    per_shape = {f"{model} {B}x{V}": total("fused", B, model) < total("torch", B, model)
                 for B, V in SHAPES for model in ("FishMoeModel3", "PnGateModule")}
    summary = {"measured": True, "device": torch.cuda.get_device_name(0), "reps": a.reps, "inner": a.inner,
               "fused_faster_stages_of": per_shape, "fused_faster_at_both_shapes": all(per_shape.values()),
               "fused_step_not_slower": all(s["torch_over_fused"] >= 1.0 for s in steps), "stages": stages, "steps": steps}
    print(json.dumps({k: v for k, v in summary.items() if k not in ("stages", "steps")}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()
