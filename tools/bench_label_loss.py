"""ops.label_loss (csrc/label_loss.hip) on one MI355X: forward + backward of HingeLoss / SoftmaxLoss alone, two ways in ONE process.

  fused   ops.label_loss: one row-reduction launch and the batch mean forward, one element-wise launch backward; bool labels read as bytes
  torch   the classes' own torch formulation (losses.HingeLoss / SoftmaxLoss with FLAGS.label_loss_fused off), autograd: the yardstick
  shapes  (B, V) = (1024, 3862), the video-level route's batch, and (80, 3862), the frame-level batch; fp32 predictions in (0, 1), bool
          labels with about 3 positives per row

After a warm-up of both routes the two alternate in blocks: --blocks blocks of --iters calls (forward + backward) per route and shape,
device events around each block (blocks x iters >= 200 calls per route), the median block's time per call.  A second set of blocks
times the forward alone.  The launches per direction are counted with torch.profiler (device-side kernel records: they include the
library's own launches) in one extra call per route, after the timings.

FLAGS.label_loss_fused defaults to on only if the fused route is not slower than the torch route at both shapes for both kinds.

  python tools/bench_label_loss.py [--blocks 10] [--iters 20] [--out profiles/bench_label_loss.json]
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

from learnablepoolingmethods_amd import FLAGS, losses, ops  # noqa: E402

SHAPES = [(1024, 3862), (80, 3862)]      # B, V
KINDS = {"hinge": losses.HingeLoss, "softmax": losses.SoftmaxLoss}


def _inputs(B, V, dev):
    g = torch.Generator().manual_seed(1)
    p = torch.rand(B, V, generator=g).to(dev).requires_grad_(True)
    y = (torch.rand(B, V, generator=g) < 3.0 / V).to(dev)
    return p, y


def _routes(kind, p, y):
    fn = KINDS[kind]()

    def fused():
        return ops.label_loss(p, y, kind)

    def plain():
        return fn.calculate_loss(p, y)            # (FLAGS.label_loss_fused is off for the whole run: the torch formulation)
    return {"fused": fused, "torch": plain}


def _block(forward, p, iters, backward):
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        loss = forward()
        if backward:
            torch.autograd.grad(loss, p)
    z.record()
    torch.cuda.synchronize()
    return a.elapsed_time(z) / iters


def _stats(ts):
    return {"median_ms": round(statistics.median(ts), 5), "range_ms": [round(min(ts), 5), round(max(ts), 5)]}


def _launches(forward, p):
    """-> {"forward": n, "backward": n}: device kernel records of one call, or None where the profiler gives none."""
    from torch.profiler import ProfilerActivity, profile

    def kernels(fn):
        with profile(activities=[ProfilerActivity.CUDA]) as prof:          # (bench.py's count_dispatches: the same trace, the same filter)
            out = fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                 and not any(w in e.name for w in ("Memcpy", "Memset", "memcpy", "memset"))]
        return out, names
    try:
        loss, fwd = kernels(forward)
        _, bwd = kernels(lambda: torch.autograd.grad(loss, p))
    except Exception as e:                        # noqa: BLE001  (a profiler that does not work here is a gap in the report, not a failure)
        return {"error": f"{type(e).__name__}: {e}"}
    if not fwd and not bwd:
        return None
    return {"forward": len(fwd), "backward": len(bwd), "forward_kernels": fwd, "backward_kernels": bwd}


def bench(kind, B, V, blocks, iters, dev):
    p, y = _inputs(B, V, dev)
    routes = _routes(kind, p, y)
    res = {"kind": kind, "shape": {"B": B, "V": V}, "blocks": blocks, "iters_per_block": iters, "calls_per_route": blocks * iters}
    values = {}
    for name, fn in routes.items():               # warm-up: code objects, allocator; and the two routes' results side by side
        for _ in range(5):
            loss = fn()
            (g,) = torch.autograd.grad(loss, p)
        values[name] = (loss.detach().double(), g.double())
    torch.cuda.synchronize()
    res["fused_vs_torch"] = {"loss_rel": float((values["fused"][0] - values["torch"][0]).abs() / values["torch"][0].abs()),
                             "gradient_max_abs_over_max_abs": float((values["fused"][1] - values["torch"][1]).abs().max()
                                                                    / values["torch"][1].abs().max())}
    times = {name: {"forward_backward": [], "forward": []} for name in routes}
    for _ in range(blocks):
        for name, fn in routes.items():
            times[name]["forward_backward"].append(_block(fn, p, iters, True))
    for _ in range(blocks):
        for name, fn in routes.items():
            times[name]["forward"].append(_block(fn, p, iters, False))
    for name in routes:
        res[name] = {k: _stats(v) for k, v in times[name].items()}
    res["torch_over_fused"] = round(res["torch"]["forward_backward"]["median_ms"] / res["fused"]["forward_backward"]["median_ms"], 3)
    res["fused_not_slower"] = res["fused"]["forward_backward"]["median_ms"] <= res["torch"]["forward_backward"]["median_ms"]
    return res, routes, p


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.blocks * a.iters < 200:
        raise SystemExit("bench_label_loss.py: blocks x iters must be at least 200 calls per route")
    if not torch.cuda.is_available():
        raise SystemExit("bench_label_loss.py needs an MI355X: no GPU is visible")
    dev = torch.device("cuda:0")
    FLAGS.label_loss_fused = False                # the classes below are the torch route
    out, keep = [], []
    for kind in KINDS:
        for B, V in SHAPES:
            r, routes, p = bench(kind, B, V, a.blocks, a.iters, dev)
            out.append(r)
            keep.append((routes, p))

    def write():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump({"measured": True, "device": torch.cuda.get_device_name(0),
                           "fused_not_slower_at_both_shapes_for_both_kinds": all(r["fused_not_slower"] for r in out), "results": out}, f, indent=1)
    write()                                       # the timings are on disk before the profiler is touched
    for r, (routes, p) in zip(out, keep):
        r["launches"] = {name: _launches(fn, p) for name, fn in routes.items()}
        print(json.dumps(r), flush=True)
    write()


if __name__ == "__main__":
    main()
