"""What the clip + update pass costs under each rule of --optimizer, on an arena of cfg-2's size and variable count (NetVladV1, K = 256,
hidden 512: the arena layout is read from a built Trainer, the arenas themselves are this tool's own).

For every rule of lpm_multi_tensor_clip_update (GradientDescent, Momentum, Adagrad, RMSProp, Adadelta) three routes alternate in one
process: the rule's three launches (ops.clip_update_step), Adam's three launches on the same arena (ops.clip_adam_step), and a plain
torch formulation of the same rule (per-variable norms and the update as torch._foreach_* passes over the variables' views).  Every
loop runs between two device synchronisations on the host clock, every route is warmed up first, every timed window runs at least
--window seconds, the median of --reps windows is reported.  Before the timing one step of the HIP route and of the torch route from
the same state are compared (the rules must agree, whatever the speed).

Bytes per parameter: the norm pass reads the gradient (4); the apply pass reads parameter and gradient, writes the parameter (12) and
reads + writes each slot the rule keeps (8 each): 16 (GradientDescent), 24 (one slot), 32 (Adadelta, and Adam).  Bandwidth = arena
floats x bytes per parameter / time: algorithmic bytes, not a counter.

  python tools/bench_optimizers.py [--reps 5] [--window 0.25] [--out profiles/bench_optimizers.json]
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

from learnablepoolingmethods_amd import FLAGS, ops, optimizers, registry  # noqa: E402
from learnablepoolingmethods_amd.train import Trainer  # noqa: E402

RULES = ("GradientDescentOptimizer", "MomentumOptimizer", "AdagradOptimizer", "RMSPropOptimizer", "AdadeltaOptimizer")
CFG2 = dict(B=80, kw=dict(iterations=300, cluster_size=256, hidden_size=512))
CLIP, LR, MOMENTUM = 1.0, 1e-4, 0.9


def bytes_per_parameter(slots: int) -> int:
    return 4 + 12 + 8 * slots


def arena_layout(dev):
    """-> (offsets [n + 1], numels [n]) of the cfg-2 model's parameter arena."""
    g = torch.Generator().manual_seed(1)
    B = CFG2["B"]
    nf = torch.randint(150, 301, (B,), generator=g, dtype=torch.int32)
    x = torch.randint(0, 256, (B, 300, 1152), dtype=torch.uint8, generator=g)
    y = torch.rand(B, 3862, generator=g) < 3.0 / 3862
    tr = Trainer(registry.get_model("NetVladV1"), vocab_size=3862, batch_size=B, device=dev, model_kwargs=CFG2["kw"])
    tr.build(x.to(dev), nf.to(dev), y.to(dev))
    offs = list(tr.arena.offsets_host)
    numels = [tr.arena.views[n].numel() for n in tr.arena.names]
    del tr
    torch.cuda.empty_cache() if dev.type == "cuda" else None
    return offs, numels


def torch_clip_update(spec, pv, gv, s0v, s1v, clip, lr):
    """The rule in plain torch over the lists of per-variable views: clip_by_norm, then the update, as multi-tensor passes."""
    norms = torch.stack(torch._foreach_norm(gv))
    factors = (clip / norms.clamp(min=clip)).unbind(0) if clip > 0 else None
    g = torch._foreach_mul(gv, list(factors)) if factors is not None else list(gv)
    k, h0, h1 = spec.kind, spec.h0, spec.h1
    if k == optimizers.GRADIENT_DESCENT:
        torch._foreach_add_(pv, g, alpha=-lr)
    elif k == optimizers.MOMENTUM:
        torch._foreach_mul_(s0v, h0)
        torch._foreach_add_(s0v, g)
        torch._foreach_add_(pv, s0v, alpha=-lr)
    elif k == optimizers.ADAGRAD:
        torch._foreach_addcmul_(s0v, g, g)
        torch._foreach_addcdiv_(pv, g, torch._foreach_sqrt(s0v), value=-lr)
    elif k == optimizers.RMSPROP:
        gg = torch._foreach_mul(g, g)
        torch._foreach_sub_(gg, s0v)
        torch._foreach_add_(s0v, gg, alpha=1.0 - h0)
        den = torch._foreach_add(s0v, h1)
        torch._foreach_sqrt_(den)
        torch._foreach_addcdiv_(pv, g, den, value=-lr)
    elif k == optimizers.ADADELTA:
        torch._foreach_mul_(s0v, h0)
        torch._foreach_addcmul_(s0v, g, g, value=1.0 - h0)
        u = torch._foreach_add(s1v, h1)
        torch._foreach_sqrt_(u)
        den = torch._foreach_add(s0v, h1)
        torch._foreach_sqrt_(den)
        torch._foreach_div_(u, den)
        torch._foreach_mul_(u, g)
        torch._foreach_mul_(s1v, h0)
        torch._foreach_addcmul_(s1v, u, u, value=1.0 - h0)
        torch._foreach_add_(pv, u, alpha=-lr)
    else:
        raise ValueError(spec.name)


def _views(arena, offs, numels):
    return [arena[o:o + k] for o, k in zip(offs, numels)]


def _timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _alternate(routes, reps, window, first=4):
    for fn in routes.values():
        _timed(fn, first)                                           # warm-up
    times = {name: [] for name in routes}
    calls = {name: max(first, int(window / (_timed(fn, first) / first) * 1.1) + 1) for name, fn in routes.items()}
    for _ in range(reps):
        for name, fn in routes.items():
            times[name].append(_timed(fn, calls[name]) / calls[name])
    return calls, times


def _ms(ts, total, bpp):
    med = statistics.median(ts)
    return {"median_ms": round(med * 1e3, 4), "range_ms": [round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)],
            "bytes_per_parameter": bpp, "algorithmic_TB_per_s": round(total * bpp / med / 1e12, 3)}


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def bench_rule(name, dev, offs, numels, P0, G, reps, window):
    spec = optimizers.by_name(name, momentum=MOMENTUM)
    total, n = offs[-1], len(numels)
    offsets = torch.tensor(offs, dtype=torch.int64, device=dev)

    def fresh():
        return P0.clone(), [torch.full((total,), init, device=dev) for init in spec.slot_init]
    # the two routes from the same state, one step: they must agree before their times mean anything
    P, slots = fresh()
    ops.clip_update_step(spec, P, G, slots, offsets, n, CLIP, LR)
    Pt, st = fresh()
    sv = [_views(s, offs, numels) for s in st] + [None, None]
    torch_clip_update(spec, _views(Pt, offs, numels), _views(G, offs, numels), sv[0], sv[1], CLIP, LR)
    # (over the variables' own elements: the kernel also walks the alignment padding -- RMSProp's slot decays there -- torch's views do not)
    def own(arena):
        return torch.cat(_views(arena, offs, numels))
    agree = {"parameters": _rel(own(P), own(Pt)), "slots": max([_rel(own(a), own(b)) for a, b in zip(slots, st)], default=0.0)}
    del Pt, st, sv
    # timing: every route on arenas of its own that it keeps updating
    Pa, M, V = P0.clone(), torch.zeros(total, device=dev), torch.zeros(total, device=dev)
    Pt, st = fresh()
    pv, gv = _views(Pt, offs, numels), _views(G, offs, numels)
    sv = [_views(s, offs, numels) for s in st] + [None, None]
    state = {"scratch": None, "adam_scratch": None, "step": 0}

    def hip():
        state["scratch"] = ops.clip_update_step(spec, P, G, slots, offsets, n, CLIP, LR, scratch=state["scratch"])

    def adam():
        state["step"] += 1
        state["adam_scratch"] = ops.clip_adam_step(Pa, G, M, V, offsets, n, CLIP, LR, state["step"], scratch=state["adam_scratch"])

    def plain():
        torch_clip_update(spec, pv, gv, sv[0], sv[1], CLIP, LR)
    calls, times = _alternate({"hip": hip, "adam_hip": adam, "torch": plain}, reps, window)
    finite = bool(torch.isfinite(P).all()) and all(bool(torch.isfinite(s).all()) for s in slots)
    r = {"optimizer": name, "slot_arenas": spec.slots, "calls_per_window": calls, "one_step_hip_against_torch_rel_err": agree,
         "finite_after_timing": finite,
         "hip": _ms(times["hip"], total, bytes_per_parameter(spec.slots)), "adam_hip": _ms(times["adam_hip"], total, bytes_per_parameter(2)),
         "torch": {"median_ms": round(statistics.median(times["torch"]) * 1e3, 4),
                   "range_ms": [round(min(times["torch"]) * 1e3, 4), round(max(times["torch"]) * 1e3, 4)]}}
    r["hip_over_adam"] = round(r["hip"]["median_ms"] / r["adam_hip"]["median_ms"], 4)
    r["bytes_over_adam_bytes"] = round(bytes_per_parameter(spec.slots) / bytes_per_parameter(2), 4)
    r["torch_over_hip"] = round(r["torch"]["median_ms"] / r["hip"]["median_ms"], 2)
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    what = ("tools/bench_optimizers.py: the three launches of lpm_multi_tensor_clip_update under each rule against lpm_multi_tensor_clip_adam and "
            "against a plain torch._foreach formulation of the same rule, on an arena of cfg-2's size and variable count")
    data = {"what": what}
    if not torch.cuda.is_available():
        data.update(measured=False, status="NOT MEASURED: no MI355X was visible to this run of the tool; there are no figures", results=[])
        if a.out:
            with open(a.out, "w") as f:
                json.dump(data, f, indent=1)
                f.write("\n")
        raise SystemExit("bench_optimizers.py needs an MI355X: no GPU is visible")
    dev = torch.device("cuda:0")
    try:
        offs, numels = arena_layout(dev)
    finally:
        FLAGS.reset()
    total = offs[-1]
    g = torch.Generator(device=dev).manual_seed(2)
    P0 = torch.randn(total, generator=g, device=dev) * 0.05
    G = torch.randn(total, generator=g, device=dev) * 1e-3
    for o, k, nxt in zip(offs, numels, offs[1:]):                 # alignment padding holds zeros, as in the trainer's arenas
        P0[o + k:nxt] = 0
        G[o + k:nxt] = 0
    data.update(measured=True, device=torch.cuda.get_device_name(0), arena_floats=total, variables=len(numels),
                parameters=int(sum(numels)), clip_norm=CLIP,
                method=(f"loops between two synchronisations on the host clock, the three routes alternating in one process, median of {a.reps} "
                        f"windows of at least {a.window} s after a warm-up; bandwidth from algorithmic bytes (norm pass 4 B per parameter + apply "
                        f"pass 12 B + 8 B per slot arena)"))
    data["results"] = [bench_rule(name, dev, offs, numels, P0, G, a.reps, a.window) for name in RULES]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(data, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
