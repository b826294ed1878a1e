"""The inference CSV end to end: inference.write_top_k (the rows formatted in Python) against inference.write_csv with
FLAGS.csv_rows_fused (ops.format_pairs on the device, lpm_csv_join_rows on the host, batch n's copy and join under batch n + 1's forward).

  default (needs an MI355X)   rows/s, wall clock from the first launch to the last byte written, over resident batches, the two routes
                              alternating in blocks in ONE process, at two shapes:
                                cfg2   NetVladV1 at the cfg-2 layer sizes (K 256, hidden 512, cluster encoders), B = 80, 300 uint8 frames
                                moe    MoeModel on [1024, 1152] video-level features
                              top_k = 20, 3862 classes, four-character ids, output to the null device; both routes' bytes are compared once
                              per shape.  And the kernel time of lpm_format_pairs alone at (B, k) = (1024, 20), device events around blocks.
  --host (no GPU)             the host side alone at (1024, 20): format_top_k_lines + write (the parent commit's formatter, unchanged)
                              against lpm_csv_join_rows + write on text / length already in host memory; lpm_format_pairs_host is timed
                              beside them.
  --exhaustive-line JSON      record the result line of tools/format_pairs_exhaustive.cc --all

Every mode UPDATES its own keys of --out (a JSON object) and leaves the others; "csv_rows_fused_default" follows from the GPU numbers: on
only if write_csv is not slower than write_top_k at both shapes.  On a shared GPU machine run it under a time limit of its own:

  timeout -k 10 600 python tools/bench_inference.py [--blocks 6] [--batches 30] [--out profiles/bench_inference.json]
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

from learnablepoolingmethods_amd import FLAGS, inference, ops, registry  # noqa: E402

VOCAB, TOP_K, ROTATE = 3862, 20, 3


def _ids(n, base=0):
    return ["%04x" % ((base + i) & 0xFFFF) for i in range(n)]


def _update(path, **keys):
    if not path:
        return
    data = {}
    if os.path.exists(path):
        with open(path) as f:
            data = json.load(f)
    data.update(keys)
    gpu = data.get("gpu")
    if isinstance(gpu, dict) and gpu.get("measured"):
        data["csv_rows_fused_default"] = bool(all(s["write_csv_not_slower"] for s in gpu["shapes"]))
        data["csv_rows_fused_default_reason"] = ("write_csv not slower than write_top_k at both shapes" if data["csv_rows_fused_default"]
                                                 else "write_csv slower than write_top_k at one shape or more: the flag stays off")
    else:
        data.setdefault("gpu", {"measured": False, "statement": "the end-to-end numbers on an MI355X were not taken"})
        data["csv_rows_fused_default"] = False
        data["csv_rows_fused_default_reason"] = "no GPU measurement: the flag stays off"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(data, f, indent=1)
        f.write("\n")


def _stats(ts):
    return {"median": round(statistics.median(ts), 1), "range": [round(min(ts), 1), round(max(ts), 1)]}


# ---- host side -----------------------------------------------------------------------------------------------------------------
def host(blocks, iters):
    B, k = 1024, TOP_K
    g = torch.Generator().manual_seed(1)
    scores = torch.sort(torch.rand(B, VOCAB, generator=g), dim=1, descending=True)[0][:, :k].contiguous()
    classes = torch.randint(0, VOCAB, (B, k), generator=g, dtype=torch.int32)
    ids = _ids(B)
    text, length = ops.format_pairs(classes, scores)
    want = "".join(inference.format_top_k_lines(ids, classes, scores)).encode("utf-8")
    same = bytes(ops.csv_join_rows(ids, text, length)) == want
    null_text, null_bytes = open(os.devnull, "w"), open(os.devnull, "wb")

    def python_route():
        for line in inference.format_top_k_lines(ids, classes, scores):
            null_text.write(line)

    def native_route():
        null_bytes.write(ops.csv_join_rows(ids, text, length))

    def host_format():
        ops.format_pairs(classes, scores)
    routes = {"format_top_k_lines_and_write": python_route, "csv_join_rows_and_write": native_route, "format_pairs_host": host_format}
    times = {n: [] for n in routes}
    for fn in routes.values():
        fn()
    for _ in range(blocks):
        for name, fn in routes.items():
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            times[name].append((time.perf_counter() - t0) / iters / B * 1e6)
    null_text.close()
    null_bytes.close()
    res = {"shape": {"B": B, "k": k}, "blocks": blocks, "iters_per_block": iters, "bytes_equal": same,
           "us_per_row": {n: {"median": round(statistics.median(t), 3), "range": [round(min(t), 3), round(max(t), 3)]} for n, t in times.items()}}
    old, new = (res["us_per_row"][n]["median"] for n in ("format_top_k_lines_and_write", "csv_join_rows_and_write"))
    res["python_over_native"] = round(old / new, 2)
    res["native_not_slower"] = new <= old
    res["note"] = ("format_top_k_lines is the parent commit's formatter, unchanged by this change; the native side is the join of ids and "
                   "device-formatted rows plus one write per batch; with a CPU predictor the rows cost format_pairs_host on top")
    return res


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
def _predictor(shape, dev):
    from learnablepoolingmethods_amd.predictor import Predictor
    from learnablepoolingmethods_amd.train import Trainer
    g = torch.Generator().manual_seed(3)
    if shape == "cfg2":
        B, model, kw = 80, "NetVladV1", dict(iterations=300, cluster_size=256, hidden_size=512)
        batches = []
        for _ in range(ROTATE):
            nf = torch.randint(150, 301, (B,), generator=g, dtype=torch.int32)
            q = torch.randint(0, 256, (B, 300, 1152), dtype=torch.uint8, generator=g)
            q[torch.arange(300).view(1, -1) >= nf.view(-1, 1)] = 0
            batches.append((q.to(dev), nf.to(dev)))
    else:
        B, model, kw = 1024, "MoeModel", {}
        batches = [(torch.randn(B, 1152, generator=g).to(dev), torch.ones(B, dtype=torch.int32, device=dev)) for _ in range(ROTATE)]
    tr = Trainer(registry.get_model(model), vocab_size=VOCAB, batch_size=B, device=dev, model_kwargs=kw)
    tr.build(batches[0][0], batches[0][1], torch.zeros(B, VOCAB, device=dev))
    pr = Predictor.from_trainer(tr)
    del tr
    return pr, B, model, [(_ids(B, i * B), x, None, nf) for i, (x, nf) in enumerate(batches)]


def _stream(resident, n):
    for i in range(n):
        yield resident[i % len(resident)]


def gpu_shape(shape, blocks, nbatches, dev):
    import io
    pr, B, model, resident = _predictor(shape, dev)
    ref, out = io.StringIO(), io.BytesIO()
    FLAGS.csv_rows_fused = False
    inference.write_top_k(ref, pr, _stream(resident, ROTATE + 1), TOP_K)
    FLAGS.csv_rows_fused = True
    inference.write_csv(out, pr, _stream(resident, ROTATE + 1), TOP_K)
    same = out.getvalue() == ref.getvalue().encode("utf-8")
    null_text, null_bytes = open(os.devnull, "w"), open(os.devnull, "wb")

    def top_k_route():
        FLAGS.csv_rows_fused = False
        return inference.write_top_k(null_text, pr, _stream(resident, nbatches), TOP_K)

    def csv_route():
        FLAGS.csv_rows_fused = True
        return inference.write_csv(null_bytes, pr, _stream(resident, nbatches), TOP_K)

    @torch.no_grad()
    def forward_only():
        for _, x, _, nf in _stream(resident, nbatches):
            pr.top_k(x, nf, TOP_K)
        return nbatches * B
    routes = {"write_top_k": top_k_route, "write_csv": csv_route, "top_k_only": forward_only}
    for fn in routes.values():
        fn()
    rates = {n: [] for n in routes}
    for _ in range(blocks):
        for name, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows = fn()
            torch.cuda.synchronize()
            rates[name].append(rows / (time.perf_counter() - t0))
    null_text.close()
    null_bytes.close()
    res = {"shape": shape, "model": model, "batch": B, "top_k": TOP_K, "blocks": blocks, "batches_per_block": nbatches, "bytes_equal": same,
           "rows_per_s": {n: _stats(r) for n, r in rates.items()}}
    res["write_csv_over_write_top_k"] = round(res["rows_per_s"]["write_csv"]["median"] / res["rows_per_s"]["write_top_k"]["median"], 3)
    res["write_csv_not_slower"] = res["rows_per_s"]["write_csv"]["median"] >= res["rows_per_s"]["write_top_k"]["median"]
    del pr
    torch.cuda.empty_cache()
    return res


def gpu_kernel(dev, blocks=10, iters=50):
    B, k = 1024, TOP_K
    g = torch.Generator().manual_seed(1)
    scores = torch.sort(torch.rand(B, VOCAB, generator=g), dim=1, descending=True)[0][:, :k].contiguous().to(dev)
    classes = torch.randint(0, VOCAB, (B, k), generator=g, dtype=torch.int32).to(dev)
    stride = ops.format_pairs_stride(k)
    text = torch.empty(B, stride, dtype=torch.uint8, device=dev)
    length = torch.empty(B, dtype=torch.int32, device=dev)
    for _ in range(5):
        ops.format_pairs_into(classes, scores, text, length)
    ts = []
    for _ in range(blocks):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            ops.format_pairs_into(classes, scores, text, length)
        z.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(z) / iters * 1e3)
    return {"shape": {"B": B, "k": k}, "blocks": blocks, "iters_per_block": iters,
            "us_per_call_back_to_back": {"median": round(statistics.median(ts), 2), "range": [round(min(ts), 2), round(max(ts), 2)]},
            "note": "device events around blocks of back-to-back calls: the kernel plus its launch gap"}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--exhaustive-line", default=None)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--batches", type=int, default=30, help="batches per block and route (GPU)")
    ap.add_argument("--iters", type=int, default=10, help="calls per block and route (--host)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.exhaustive_line is not None:
        r = {"command": "tools/format_pairs_exhaustive.cc --all --threads 16 (plain build)", "result": json.loads(a.exhaustive_line)}
        print(json.dumps(r), flush=True)
        _update(a.out, exhaustive=r)
        return
    if a.host:
        r = host(a.blocks, a.iters)
        print(json.dumps(r), flush=True)
        _update(a.out, host_side=r)
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_inference.py needs an MI355X: no GPU is visible (--host measures the host side alone)")
    dev = torch.device("cuda:0")
    try:
        shapes = []
        for shape in ("cfg2", "moe"):
            r = gpu_shape(shape, a.blocks, a.batches, dev)
            print(json.dumps(r), flush=True)
            shapes.append(r)
        kernel = gpu_kernel(dev)
        print(json.dumps(kernel), flush=True)
    finally:
        FLAGS.reset()
    _update(a.out, gpu={"measured": True, "device": torch.cuda.get_device_name(0), "shapes": shapes, "format_pairs_kernel": kernel})


if __name__ == "__main__":
    main()
