"""ops.lstm_layer (csrc/lstm.hip) on one MI355X: forward + backward of ONE LSTM layer two ways in ONE process, alternating, device-event
times, median of --reps.

  fused     ops.lstm_layer: X Wx as one GEMM, a kernel per time step each way, dX / dkernel as GEMMs behind the loop (the time-step
            launches alone also timed through ops.KERNEL_TIMELINE in a separate set of repetitions)
  per_step  rnn_modules._lstm_layer_host on the GPU: the same layer as a per-step torch formulation, autograd
  shapes    (B, T, In, H) = (16, 30, 512, 512), the audio stream of TriangulationRelationalModel at its defaults, and
            (16, 30, 16384, 16384), its video stream (an 8.6 GB kernel); if the device refuses the allocations of the second, H = In = 4096
            takes its place and the result says so

Beside the times: the step's floor from the bytes of Wh over the HBM peak (8.0 TB/s) and the measured fraction of it.  No ratio is asked
for; FLAGS.lstm_fused defaults to on only if the fused route is not slower at both shapes.

  python tools/bench_lstm.py [--reps 5] [--out profiles/bench_lstm.json]
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

from learnablepoolingmethods_amd import ops, rnn_modules  # noqa: E402

SHAPES = [(16, 30, 512, 512), (16, 30, 16384, 16384)]      # B, T, In, H
FALLBACK = (16, 30, 4096, 4096)
HBM_PEAK = 8.0e12                                           # bytes / s
NAMES = ("outputs", "h_last", "c_last", "dx", "dkernel", "dbias")


def _inputs(B, T, In, H, dev):
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(B, T, In, device=dev, generator=g).requires_grad_(True)
    lim = math.sqrt(6.0 / (In + 5 * H))
    kernel = torch.rand(In + H, 4 * H, device=dev, generator=g).mul_(2).sub_(1).mul_(lim).requires_grad_(True)
    bias = (0.1 * torch.randn(4 * H, device=dev, generator=g)).requires_grad_(True)
    lengths = torch.randint(T // 2, T + 1, (B,), device=dev, generator=g)
    up = (torch.randn(B, T, H, device=dev, generator=g), torch.randn(B, H, device=dev, generator=g),
          torch.randn(B, H, device=dev, generator=g))
    return [x, kernel, bias], lengths, up


def _timed(fn):
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    z.record()
    return out, a, z


def _call(route, leaves, lengths, up):
    """-> (forward ms, backward ms, results, gradients)"""
    fn = ops.lstm_layer if route == "fused" else rnn_modules._lstm_layer_host
    for t in leaves:
        t.grad = None
    outs, a0, a1 = _timed(lambda: fn(*leaves, lengths))
    _, b0, b1 = _timed(lambda: torch.autograd.backward(outs, up))
    torch.cuda.synchronize()
    return a0.elapsed_time(a1), b0.elapsed_time(b1), outs


def _stats(ts):
    return {"median_ms": round(statistics.median(ts), 4), "range_ms": [round(min(ts), 4), round(max(ts), 4)]}


def _launches(leaves, lengths, up, reps):
    per = {}
    for _ in range(reps):
        ops.KERNEL_TIMELINE = []
        try:
            _call("fused", leaves, lengths, up)
            for name, _, t0, t1 in ops.KERNEL_TIMELINE:
                per.setdefault(name, []).append(t0.elapsed_time(t1))
        finally:
            ops.KERNEL_TIMELINE = None
    return {name: round(statistics.median(ts), 4) for name, ts in per.items()}


def bench(B, T, In, H, reps, dev):
    leaves, lengths, up = _inputs(B, T, In, H, dev)
    res = {"shape": {"B": B, "T": T, "In": In, "H": H}, "reps": reps, "kernel_bytes": 4 * (In + H) * 4 * H, "wh_bytes": 4 * H * 4 * H}
    results = {}
    for route in ("fused", "per_step"):                  # warm-up (code objects, allocator, library algorithm choices) and the comparison
        for _ in range(2):
            outs = _call(route, leaves, lengths, up)[2]
        results[route] = [o.detach().clone() for o in outs] + [t.grad.clone() for t in leaves[:1]] + [leaves[1].grad.clone(), leaves[2].grad.clone()]
    res["fused_vs_per_step_max_abs_over_max_abs"] = {n: float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
                                                     for n, a, b in zip(NAMES, results["fused"], results["per_step"])}
    del results, outs
    times = {"fused": ([], []), "per_step": ([], [])}
    for _ in range(reps):
        for route in times:
            f, b, _ = _call(route, leaves, lengths, up)
            times[route][0].append(f)
            times[route][1].append(b)
    for route, (f, b) in times.items():
        res[route] = {"forward": _stats(f), "backward": _stats(b), "forward_backward": _stats([u + v for u, v in zip(f, b)])}
    res["per_step_over_fused"] = round(res["per_step"]["forward_backward"]["median_ms"] / res["fused"]["forward_backward"]["median_ms"], 3)
    res["fused_time_loops_ms"] = _launches(leaves, lengths, up, max(3, reps // 2))
    floor = res["wh_bytes"] / HBM_PEAK * 1e3
    res["step_floor_ms_wh_bytes_over_hbm_peak"] = round(floor, 5)
    for key, name in (("forward", "lstm_layer_fwd"), ("backward", "lstm_layer_bwd")):
        step = res["fused_time_loops_ms"][name] / T
        res[f"{key}_step_ms"] = round(step, 5)
        res[f"{key}_step_fraction_of_hbm_floor"] = round(floor / step, 3)       # (only meaningful where Wh exceeds the caches)
    for t in leaves:
        t.grad = None
    del leaves, up
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", type=int, nargs=4, action="append", metavar=("B", "T", "IN", "H"), help="instead of the two default shapes")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lstm.py needs an MI355X: no GPU is visible")
    dev = torch.device("cuda:0")
    out, notes = [], []
    for shape in ([tuple(s) for s in a.shape] if a.shape else SHAPES):
        r = None
        try:
            r = bench(*shape, a.reps, dev)
        except torch.cuda.OutOfMemoryError as e:
            if a.shape or shape != SHAPES[1]:
                raise
            notes.append(f"{shape}: the device refused the allocations ({str(e).splitlines()[0]}); measured {FALLBACK} in its place")
        if r is None:                                    # (outside the handler: the failed attempt's tensors are released by now)
            torch.cuda.empty_cache()
            r = bench(*FALLBACK, a.reps, dev)
        print(json.dumps(r), flush=True)
        out.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"measured": True, "device": torch.cuda.get_device_name(0), "notes": notes,
                       "fused_not_slower_at_both_shapes": all(r["per_step_over_fused"] >= 1.0 for r in out), "results": out}, f, indent=1)


if __name__ == "__main__":
    main()
