"""The triangulation models' input stage from a uint8 [B, 300, 1152] batch on one MI355X, two ways in ONE process, alternating:
forward + backward of the stage alone, device-event times over windows of --inner calls, median of --reps windows.

  a_normalise_everything  ops.dequantize_l2_normalize over all 300 frames -> model_utils.SampleRandomFrames -> the batch norm(s)
                          (layers.batch_norm) -> contiguous stream slices: what the models do with fp32 input
  b_gather                frame_level_models._gather_and_normalise: model_utils.random_frame_index + ops.frame_gather_bn_split (the *_idx
                          frame-prep kernels): only the sampled uint8 rows are read
  bn                      "streams": video_bn [1024] + audio_bn [128] (four of the five models); "joint": input_bn [1152]
                          (RegularizedTriangulationModel)
  shapes                  (B, S) = (16, 30), (16, 64), (16, 200), (80, 300): the models' own; num_frames ~ U{120..300}

Bytes allocated are torch.cuda.max_memory_allocated over one call, above what was allocated before it.  b's rate is the algorithmic
bytes of forward + backward (the sampled uint8 rows read twice, the fp32 rows written once and their gradient read once) over its
whole-call time: a rate of the call, launches and allocations included, not of a kernel.
The last line is Trainer.step of JuhanTestModelV5 at its defaults, B = 16, FLAGS.gather_frames_fused on against off, alternating.

  python tools/bench_frame_gather.py [--reps 15] [--inner 20] [--out profiles/bench_frame_gather.json]
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

from learnablepoolingmethods_amd import FLAGS, frame_level_models, layers, model_utils, ops, registry  # noqa: E402
from learnablepoolingmethods_amd import variables as vs  # noqa: E402
from learnablepoolingmethods_amd.train import Trainer  # noqa: E402

SHAPES = [(16, 30), (16, 64), (16, 200), (80, 300)]
MF, F, DV = 300, 1152, 1024


def _batch(B, dev, seed=1):
    g = torch.Generator().manual_seed(seed)
    nf = torch.randint(120, MF + 1, (B,), generator=g, dtype=torch.int32)
    q = torch.randint(0, 256, (B, MF, F), generator=g, dtype=torch.uint8)
    q = torch.where(torch.arange(MF).view(1, -1, 1) < nf.view(-1, 1, 1), q, torch.zeros((), dtype=torch.uint8))
    return q.to(dev), nf.to(dev)


def path_a(q, nf, S, u, bn):
    x = ops.dequantize_l2_normalize(q, nf)
    x = model_utils.SampleRandomFrames(x, nf.reshape(-1, 1), S, uniform=u).reshape(-1, F)
    if bn == "joint":
        x = layers.batch_norm(x, True, "input_bn")
        return x[:, :DV].contiguous(), x[:, DV:].contiguous()
    return (layers.batch_norm(x[:, :DV], True, "video_bn").contiguous(), layers.batch_norm(x[:, DV:], True, "audio_bn").contiguous())


def path_b(q, nf, S, u, bn):
    scopes = ("input_bn",) if bn == "joint" else ("video_bn", "audio_bn")
    return frame_level_models._gather_and_normalise(q, nf, S, u, scopes, True, True)


def _call(path, store, q, nf, S, u, bn, ups):
    for n, v in store.vars.items():
        v.grad = None
    with vs.use_store(store):
        outs = path(q, nf, S, u, bn)
    torch.autograd.backward(list(outs), ups)
    return outs


def _window(fn, inner):
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    z.record()
    torch.cuda.synchronize()
    return a.elapsed_time(z) / inner


def _stats(ts):
    return {"median_ms": round(statistics.median(ts), 4), "range_ms": [round(min(ts), 4), round(max(ts), 4)]}


def bench(B, S, bn, reps, inner, dev):
    q, nf = _batch(B, dev)
    g = torch.Generator().manual_seed(2)
    u = torch.rand(B, S, generator=g).to(dev)
    ups = [torch.randn(B * S, DV, generator=g).to(dev), torch.randn(B * S, F - DV, generator=g).to(dev)]
    paths = {"a_normalise_everything": path_a, "b_gather": path_b}
    stores = {k: vs.VariableStore(device=dev) for k in paths}
    res = {"shape": {"B": B, "S": S, "max_frames": MF, "F": F}, "bn": bn, "reps": reps, "inner": inner}
    outs = {}
    for k, p in paths.items():
        for _ in range(3):                            # warm-up: code objects, allocator, the variables
            _call(p, stores[k], q, nf, S, u, bn, ups)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        o = _call(p, stores[k], q, nf, S, u, bn, ups)
        torch.cuda.synchronize()
        res[k] = {"allocated_bytes": int(torch.cuda.max_memory_allocated() - base)}
        outs[k] = [t.detach() for t in o]
        del o
    res["b_vs_a_outputs_max_abs_over_max_abs"] = [float((x - y).abs().max() / y.abs().max()) for x, y in zip(outs["b_gather"], outs["a_normalise_everything"])]
    del outs
    times = {k: [] for k in paths}
    for _ in range(reps):
        for k, p in paths.items():
            times[k].append(_window(lambda: _call(p, stores[k], q, nf, S, u, bn, ups), inner))
    for k in paths:
        res[k].update(_stats(times[k]))
    rows = B * S
    alg = rows * F * (1 + 4) + rows * F * (4 + 1)
    tb = res["b_gather"]["median_ms"]
    res["b_algorithmic_bytes"] = alg
    res["b_whole_call_GB_per_s"] = round(alg / (tb * 1e-3) * 1e-9, 1)
    res["a_over_b"] = round(res["a_normalise_everything"]["median_ms"] / tb, 2)
    res["b_not_slower"] = bool(tb <= res["a_normalise_everything"]["median_ms"])
    del q, ups
    torch.cuda.empty_cache()
    return res


def bench_step(reps, dev):
    """Trainer.step of JuhanTestModelV5 at its defaults, B = 16, on one resident uint8 batch: FLAGS.gather_frames_fused on against off."""
    B, V = 16, 3862
    q, nf = _batch(B, dev, seed=5)
    g = torch.Generator().manual_seed(6)
    lab = torch.zeros(B, V)
    lab[torch.arange(B).repeat_interleave(3), torch.randint(0, V, (3 * B,), generator=g)] = 1.0
    lab = lab.to(dev)
    trainers, times = {}, {"on": [], "off": []}
    try:
        for k in times:
            FLAGS.gather_frames_fused = k == "on"
            torch.manual_seed(0)
            trainers[k] = Trainer(registry.get_model("JuhanTestModelV5"), vocab_size=V, batch_size=B, base_learning_rate=1e-3, device=dev, seed=3)
            assert trainers[k]._quantised_frames(q) == (k == "on")
            for _ in range(3):
                trainers[k].step(q, nf, lab)
        for _ in range(reps):
            for k in times:
                FLAGS.gather_frames_fused = k == "on"
                times[k].append(_window(lambda: trainers[k].step(q, nf, lab), 5))
    finally:
        FLAGS.reset()
    return {"trainer_step": "JuhanTestModelV5 defaults, B = 16", "reps": reps, "steps_per_window": 5,
            "gather_frames_fused_on": _stats(times["on"]), "gather_frames_fused_off": _stats(times["off"])}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_frame_gather.py needs an MI355X: no GPU is visible")
    dev = torch.device("cuda:0")
    out = []
    for bn in ("streams", "joint"):
        for B, S in SHAPES:
            r = bench(B, S, bn, a.reps, a.inner, dev)
            print(json.dumps(r), flush=True)
            out.append(r)
    step = bench_step(a.reps, dev)
    print(json.dumps(step), flush=True)
    verdict = all(r["b_not_slower"] for r in out)
    print(json.dumps({"b_not_slower_at_every_shape": verdict}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"measured": True, "device": torch.cuda.get_device_name(0), "results": out, "end_to_end": step,
                       "b_not_slower_at_every_shape": verdict}, f, indent=1)


if __name__ == "__main__":
    main()
