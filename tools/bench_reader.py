"""Reader throughput (clips/s): readers.YT8MFrameFeatureReader.batches() (pure Python) against device_batches() (pinned ring, native
indexer, lpm_gather_frames / lpm_labels_dense), alone and in front of evaluation.evaluate(Predictor) at cfg-2.

Synthetic YT8M-shaped TFRecord files (frame counts spread over 120-300, about 3 labels per clip, 3862 classes, 1024 + 128 bytes per frame)
are written once into a temporary directory -- --unique different clips, framed once and repeated in a shuffled order up to --clips per
pass, so that the files are valid, CRCs included, without hours of Python CRC -- and are then read from the page cache.  One JSON line per
batch size (80, 128):

  batches_clips_per_s                     the Python route over one batch's worth of clips
  device_clips_per_s[_crc][_t2]           device_batches() alone over all files: the consumer drops every batch at once and the device is
                                          synchronised before the clock is read; with verify_crc (_crc), with reader_threads=2 (_t2)
  read_ms, index_ms, issue_ms             host clock per batch inside the pipeline thread (reading into the pinned slot; framing + locating +
                                          ids; enqueueing copies and kernels)
  copy_us, gather_us                      in-stream time per batch by device events: slot + tables to the device; the two kernels
  evaluate_device_clips_per_s             evaluate(Predictor, device_batches(...)) at cfg-2 (batch 80 only)
  evaluate_resident_clips_per_s           evaluate over the same number of batches resident on the device (eight, rotating)
  predict_resident_clips_per_s            Predictor.predict alone over those

Every loop is warmed up by one pass, timed --reps times between device synchronisations on the host clock, and the median is printed with
its range.

  python tools/bench_reader.py [--clips 2560] [--files 16] [--unique 64] [--reps 5] [--batches 80,128] [--out FILE]
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
from learnablepoolingmethods_amd.evaluation import evaluate  # noqa: E402
from learnablepoolingmethods_amd.predictor import Predictor  # noqa: E402
from learnablepoolingmethods_amd.train import Trainer  # noqa: E402

MAX_FRAMES, VOCAB = 300, 3862
CFG2 = dict(model="NetVladV1", kw=dict(cluster_size=256, hidden_size=512))


def write_files(directory, clips, files, unique, seed=1):
    """-> (paths, clips written, bytes written)."""
    rng = np.random.default_rng(seed)
    framed = []
    for k in range(unique):
        n = int(rng.integers(120, 301))
        labels = np.flatnonzero(rng.random(VOCAB) < 3.0 / VOCAB).tolist()
        rec = readers.make_sequence_example(f"clip{k:06d}", labels, {"rgb": rng.integers(0, 256, (n, 1024), dtype=np.uint8),
                                                                    "audio": rng.integers(0, 256, (n, 128), dtype=np.uint8)})
        head = struct.pack("<Q", len(rec))
        framed.append(head + struct.pack("<I", readers.masked_crc32c(head)) + rec + struct.pack("<I", readers.masked_crc32c(rec)))
    per_file = clips // files
    paths, total = [], 0
    for i in range(files):
        path = os.path.join(directory, f"train{i:04d}.tfrecord")
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


def run(B, paths, clips, nbytes, reps, dev, with_model):
    reader = readers.YT8MFrameFeatureReader(num_classes=VOCAB, max_frames=MAX_FRAMES)
    res = {"tool": "bench_reader", "batch": B, "clips_per_pass": clips, "files": len(paths), "mean_record_bytes": round(nbytes / clips),
           "reps": reps}

    def rate(key, fn, n=clips):
        med, lo, hi = timed(fn, reps)
        res[key] = round(n / med, 1)
        res[key + "_range"] = [round(n / hi, 1), round(n / lo, 1)]

    # the Python route: one batch's worth of clips is enough at a few hundred clips per second
    t0 = time.perf_counter()
    it = reader.batches(paths, B)
    next(it)
    it.close()
    res["batches_clips_per_s"] = round(B / (time.perf_counter() - t0), 1)

    def drain(**kw):
        def fn():
            for _ in reader.device_batches(paths, B, device=dev, **kw):
                pass                                            # dropped at once: the ring's back-pressure bounds the memory
        return fn
    rate("device_clips_per_s", drain())
    rate("device_clips_per_s_t2", drain(reader_threads=2))
    rate("device_clips_per_s_crc", drain(verify_crc=True))
    rate("device_clips_per_s_crc_t2", drain(verify_crc=True, reader_threads=2))
    # the split of one batch's time
    st = {"time_gather": True}
    for _ in reader.device_batches(paths, B, device=dev, stats=st):
        pass
    torch.cuda.synchronize()
    nb = st["batches"]
    res["read_ms"] = round(st["read_s"] / nb * 1e3, 3)
    res["index_ms"] = round(st["index_s"] / nb * 1e3, 3)
    res["issue_ms"] = round(st["issue_s"] / nb * 1e3, 3)
    res["copy_us"] = round(statistics.median(a.elapsed_time(b) for a, b, _ in st["gather_events"]) * 1e3, 1)
    res["gather_us"] = round(statistics.median(b.elapsed_time(c) for _, b, c in st["gather_events"]) * 1e3, 1)
    res["batch_bytes"] = round(st["bytes"] / nb)
    if with_model:
        resident = []
        for item in reader.device_batches(paths, B, device=dev):
            resident.append(item)
            if len(resident) == 8:
                break
        tr = Trainer(registry.get_model(CFG2["model"]), vocab_size=VOCAB, batch_size=B, device=dev,
                     model_kwargs=dict(iterations=MAX_FRAMES, **CFG2["kw"]))
        tr.build(resident[0][1], resident[0][3], resident[0][2].float())
        pr = Predictor.from_trainer(tr)
        del tr
        nbatch = clips // B

        @torch.no_grad()
        def predict_resident():
            for i in range(nbatch):
                pr.predict(resident[i % 8][1], resident[i % 8][3])
        rate("predict_resident_clips_per_s", predict_resident, nbatch * B)
        rate("evaluate_resident_clips_per_s", lambda: evaluate(pr, (resident[i % 8] for i in range(nbatch)), top_k=20), nbatch * B)
        rate("evaluate_device_clips_per_s", lambda: evaluate(pr, reader.device_batches(paths, B, device=dev, drop_remainder=True), top_k=20),
             nbatch * B)
        rate("evaluate_device_clips_per_s_t2",
             lambda: evaluate(pr, reader.device_batches(paths, B, device=dev, drop_remainder=True, reader_threads=2), top_k=20), nbatch * B)
        res["reader_over_predict"] = round(res["device_clips_per_s"] / res["predict_resident_clips_per_s"], 3)
        del pr, resident
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--clips", type=int, default=2560)
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--unique", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", default="80,128")
    ap.add_argument("--dir", default=None, help="where the temporary files go (default: the system's temporary directory)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_reader.py needs an MI355X: no GPU is visible")
    dev = torch.device("cuda:0")
    out = []
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        paths, clips, nbytes = write_files(d, a.clips, a.files, a.unique)
        for B in (int(b) for b in a.batches.split(",")):
            r = run(B, paths, clips, nbytes, a.reps, dev, with_model=(B == 80))
            print(json.dumps(r), flush=True)
            out.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
