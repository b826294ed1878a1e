"""Video-level reader throughput (examples/s): readers.YT8MAggregatedFeatureReader.batches() (pure Python) against device_batches()
(pinned ring, lpm_yt8m_locate_examples, lpm_gather_examples / lpm_labels_dense), and against what it feeds: Trainer.step of MoeModel at
B = 1024 (FLAGS.batch_size's default), on resident batches and fed by training_batches().

Synthetic video-level files (mean_rgb 1024 + mean_audio 128 floats, about 3 labels per video, 3862 classes) are written once into a
temporary directory -- --unique different examples, framed once and repeated in a shuffled order up to --examples per pass, so that the
files are valid, CRCs included, without minutes of Python CRC -- and are then read from the page cache.  One JSON object:

  batches_examples_per_s                  the Python route over one batch
  device_examples_per_s[_t2][_unpacked]   device_batches() alone over all files: the consumer drops every batch at once and the device is
                                          synchronised before the clock is read; with reader_threads=2 (_t2); over files written unpacked,
                                          one tagged fixed32 per value (_unpacked: the indexer's stride-5 case)
  walk_ms, read_ms, index_ms, issue_ms    host clock per batch inside the pipeline threads (the 12-byte record headers; reading into the
                                          pinned slot; framing + locating + ids; enqueueing copies and kernels)
  copy_us, gather_us                      in-stream time per batch by device events: slot + tables to the device; the two kernels
  step_resident_examples_per_s            Trainer.step of MoeModel over eight resident batches, rotating
  step_fed_examples_per_s[_t2]            Trainer.step fed by training_batches() (shuffle pool on the device)
  reader_over_step                        device_examples_per_s / step_resident_examples_per_s: below 1 the reader is the slower side

Every loop is warmed up by one pass, timed --reps times between device synchronisations on the host clock, and the median is printed with
its range.

  python tools/bench_example_reader.py [--examples 16384] [--files 8] [--unique 256] [--reps 5] [--batch 1024] [--out FILE]
"""
import argparse
import json
import os
import statistics
import struct
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from learnablepoolingmethods_amd import readers, registry  # noqa: E402
from learnablepoolingmethods_amd.train import Trainer  # noqa: E402

VOCAB, SIZES = 3862, (1024, 128)


def write_files(directory, examples, files, unique, packed=True, seed=1):
    """-> (paths, examples written, bytes written)."""
    rng = np.random.default_rng(seed)
    framed = []
    for k in range(unique):
        labels = np.flatnonzero(rng.random(VOCAB) < 3.0 / VOCAB).tolist()
        rec = readers.make_example(f"vid{k:07d}", labels, {"mean_rgb": rng.standard_normal(SIZES[0]).astype(np.float32),
                                                           "mean_audio": rng.standard_normal(SIZES[1]).astype(np.float32)}, packed=packed)
        head = struct.pack("<Q", len(rec))
        framed.append(head + struct.pack("<I", readers.masked_crc32c(head)) + rec + struct.pack("<I", readers.masked_crc32c(rec)))
    per_file = examples // files
    paths, total = [], 0
    for i in range(files):
        path = os.path.join(directory, f"train{'' if packed else '_unpacked'}{i:04d}.tfrecord")
        with open(path, "wb") as f:
            for k in rng.integers(0, unique, size=per_file).tolist():
                f.write(framed[k])
                total += len(framed[k])
        paths.append(path)
    return paths, per_file * files, total


def timed(fn, reps):
    """Median and range of fn()'s seconds between device synchronisations, after one warm-up call."""
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def run(B, paths, unpacked, examples, nbytes, reps, dev):
    reader = readers.YT8MAggregatedFeatureReader(num_classes=VOCAB, feature_sizes=SIZES)
    res = {"tool": "bench_example_reader", "batch": B, "examples_per_pass": examples, "files": len(paths),
           "mean_record_bytes": round(nbytes / examples), "reps": reps}

    def rate(key, fn, n=examples):
        med, lo, hi = timed(fn, reps)
        res[key] = round(n / med, 1)
        res[key + "_range"] = [round(n / hi, 1), round(n / lo, 1)]

    t0 = time.perf_counter()
    it = reader.batches(paths, B)
    next(it)
    it.close()
    res["batches_examples_per_s"] = round(B / (time.perf_counter() - t0), 1)

    def drain(files, **kw):
        def fn():
            for _ in reader.device_batches(files, B, device=dev, **kw):
                pass                                            # dropped at once: the ring's back-pressure bounds the memory
        return fn
    rate("device_examples_per_s", drain(paths))
    rate("device_examples_per_s_t2", drain(paths, reader_threads=2))
    rate("device_examples_per_s_unpacked", drain(unpacked))
    # the split of one batch's time
    for suffix, kw in (("", {}), ("_t2", dict(reader_threads=2))):
        st = {"time_gather": True}
        for _ in reader.device_batches(paths, B, device=dev, stats=st, **kw):
            pass
        torch.cuda.synchronize()
        nb = st["batches"]
        for k in ("walk", "read", "index", "issue"):
            res[f"{k}_ms{suffix}"] = round(st[k + "_s"] / nb * 1e3, 3)
        res["copy_us" + suffix] = round(statistics.median(a.elapsed_time(b) for a, b, _ in st["gather_events"]) * 1e3, 1)
        res["gather_us" + suffix] = round(statistics.median(b.elapsed_time(c) for _, b, c in st["gather_events"]) * 1e3, 1)
        res["batch_bytes"] = round(st["bytes"] / nb)
    # what the reader feeds
    resident = []
    for item in reader.device_batches(paths, B, device=dev):
        resident.append(item)
        if len(resident) == 8:
            break
    tr = Trainer(registry.get_model("MoeModel"), vocab_size=VOCAB, batch_size=B, device=dev)
    nbatch = examples // B

    def step_resident():
        for i in range(nbatch):
            _, x, y, nf = resident[i % len(resident)]
            tr.step(x, nf, y)
    rate("step_resident_examples_per_s", step_resident, nbatch * B)

    def step_fed(**kw):
        def fn():
            it = reader.training_batches(paths, B, device=dev, num_epochs=1, seed=0, **kw)
            for k, (_, x, y, nf) in enumerate(it):
                if k == nbatch:
                    break
                tr.step(x, nf, y)
            it.close()
        return fn
    rate("step_fed_examples_per_s", step_fed(), nbatch * B)
    rate("step_fed_examples_per_s_t2", step_fed(reader_threads=2), nbatch * B)
    res["reader_over_step"] = round(res["device_examples_per_s"] / res["step_resident_examples_per_s"], 3)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--examples", type=int, default=16384)
    ap.add_argument("--files", type=int, default=8)
    ap.add_argument("--unique", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--dir", default=None, help="where the temporary files go (default: the system's temporary directory)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_example_reader.py needs an MI355X: no GPU is visible")
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        paths, examples, nbytes = write_files(d, a.examples, a.files, a.unique)
        unpacked, _, _ = write_files(d, a.examples, a.files, a.unique, packed=False)
        res = run(a.batch, paths, unpacked, examples, nbytes, a.reps, dev)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
