"""Training from the reader's quantised frames and from TFRecord files, in clips/s, at cfg-2 and cfg-5 on one MI355X.

Synthetic YT8M-shaped files as tools/bench_reader.py writes them, read from the page cache.  In ONE process per configuration,
alternating, --reps times each after a warm-up, the median and range of

  a_fp32_detour_clips_per_s       Trainer.step over eight resident rotating uint8 batches, FLAGS.train_quantised_frames off
                                  (ops.dequantize_l2_normalize writes the fp32 frames of all max_frames, the frame kernels re-read them)
  b_quantised_clips_per_s         the same with the flag on (lpm_frame_inv_norm_q8 + lpm_frame_stats_q8 + *_q8 apply + lpm_frame_bn_bwd*_q8)
  c_run_from_files_clips_per_s[_t2]
                                  training.run over YT8MFrameFeatureReader.training_batches(files) -- shuffle pool, log line every 10 steps --
                                  with reader_threads 1 and 2 (_t2), flag on
and the ratios b_over_a, c_over_b.  For (c) the pipeline's own host seconds per batch (device_batches' ``stats``) are reported too.
Every window is --steps steps between device synchronisations on the host clock.

The summed time of the frame-prep kernels per step comes from kernel traces taken in runs of their own:

  rocprofv3 --kernel-trace --stats -d DIR_A -o a -- python tools/bench_train_reader.py --steps-only cfg2 --quantised 0 --steps 60
  rocprofv3 --kernel-trace --stats -d DIR_B -o b -- python tools/bench_train_reader.py --steps-only cfg2 --quantised 1 --steps 60
  python tools/bench_train_reader.py --kernel-stats DIR_A DIR_B --steps 60 [--label cfg2] [--merge-into FILE]

  python tools/bench_train_reader.py [--configs cfg2,cfg5] [--steps 60] [--reps 3] [--clips 2560] [--files 16] [--out FILE]
"""
import argparse
import csv
import glob
import json
import os
import re
import sqlite3
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# kernels of the frame preparation (csrc/frame_prep.hip) a training step launches
FRAME_PREP = re.compile(r"dequantize_l2_normalize_kernel|frame_inv_norm_q8_kernel|frame_stats_kernel|frame_apply\w*_kernel|"
                        r"frame_bn_bwd_partial_kernel|frame_bn_bwd_reduce_kernel")


def _setup(cfg):
    import torch
    import bench
    from learnablepoolingmethods_amd import FLAGS, readers, registry
    from learnablepoolingmethods_amd.train import Trainer
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_reader.py needs an MI355X: no GPU is visible")
    wl = bench.WORKLOADS[cfg]
    FLAGS.reset()
    bench.set_flags(wl)
    dev = torch.device("cuda:0")

    def trainer():
        return Trainer(registry.get_model(wl.get("model", "NetVladV1")), vocab_size=bench.VOCAB, batch_size=wl["batch"], device=dev, seed=1234,
                       model_kwargs=wl["model_kwargs"], **bench.TRAIN)
    reader = readers.YT8MFrameFeatureReader(num_classes=bench.VOCAB, max_frames=bench.MAX_FRAMES)
    return torch, FLAGS, wl, dev, trainer, reader


def _resident(reader, paths, B, dev, n=8):
    out = []
    it = reader.device_batches(paths, B, device=dev)
    for _, q, y, nf in it:
        out.append((q, nf, y))
        if len(out) == n:
            break
    it.close()
    return out


def measure(cfg, paths, steps, reps, warmup):
    from learnablepoolingmethods_amd import training
    torch, FLAGS, wl, dev, trainer, reader = _setup(cfg)
    B = wl["batch"]
    resident = _resident(reader, paths, B, dev)
    tr = {"a": trainer(), "b": trainer()}
    count = {"a": 0, "b": 0}

    def block(which, n):
        FLAGS.train_quantised_frames = which == "b"
        t = tr[which]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            t.step(*resident[count[which] % len(resident)])
            count[which] += 1
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    for which in ("a", "b"):
        block(which, warmup)
    secs = {"a": [], "b": [], "c": [], "c_t2": []}
    for _ in range(reps):
        for which in ("a", "b"):
            secs[which].append(block(which, steps))
    # (c): the run loop over shuffled batches from files, on the trainer of (b)
    FLAGS.train_quantised_frames = True
    pipeline = {}
    for key, threads in (("c", 1), ("c_t2", 2)):
        st = {}
        it = reader.training_batches(paths, B, device=dev, num_epochs=None, seed=1, reader_threads=threads, stats=st)
        t = tr["b"]
        training.run(t, it, max_steps=t.global_step + warmup, log=lambda s: None)              # fills the pool, warms the route
        for _ in range(reps):
            torch.cuda.synchronize()
            out = training.run(t, it, max_steps=t.global_step + steps, log=lambda s: None)
            torch.cuda.synchronize()
            assert out["steps"] == steps
            secs[key].append(out["seconds"])
        it.close()
        nb = max(st.get("batches", 0), 1)
        pipeline[key] = {k[:-2] + "_ms_per_batch": round(st[k] / nb * 1e3, 3) for k in ("read_s", "index_s", "issue_s") if k in st}
    res = {"tool": "bench_train_reader", "config": cfg, "batch": B, "steps_per_window": steps, "reps": reps, "warmup_steps": warmup}
    names = {"a": "a_fp32_detour_clips_per_s", "b": "b_quantised_clips_per_s", "c": "c_run_from_files_clips_per_s",
             "c_t2": "c_run_from_files_clips_per_s_t2"}
    for key, name in names.items():
        med = statistics.median(secs[key])
        res[name] = round(steps * B / med, 1)
        res[name + "_range"] = [round(steps * B / max(secs[key]), 1), round(steps * B / min(secs[key]), 1)]
        res[name.replace("clips_per_s", "ms_per_step")] = round(med / steps * 1e3, 4)
    res["b_over_a"] = round(res[names["b"]] / res[names["a"]], 4)
    res["c_over_b"] = round(res[names["c"]] / res[names["b"]], 4)
    res["c_t2_over_b"] = round(res[names["c_t2"]] / res[names["b"]], 4)
    res["pipeline_host"] = pipeline
    return res


def steps_only(cfg, quantised, steps, paths):
    """The trainer of (a) or (b) for ``steps`` steps over resident batches: the program of a kernel-trace run."""
    torch, FLAGS, wl, dev, trainer, reader = _setup(cfg)
    resident = _resident(reader, paths, wl["batch"], dev)
    FLAGS.train_quantised_frames = bool(quantised)
    t = trainer()
    for i in range(steps):
        t.step(*resident[i % len(resident)])
    torch.cuda.synchronize()
    print(json.dumps({"config": cfg, "quantised": bool(quantised), "steps": steps}))


def kernel_stats(directory):
    """-> {kernel: (calls, total ns)} of a rocprofv3 --kernel-trace [--stats] output directory (kernel_stats.csv, else the rocpd database)."""
    rows = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            c, t = rows.get(r["Name"], (0, 0))
            rows[r["Name"]] = (c + int(r["Calls"]), t + int(float(r["TotalDurationNs"])))
    if rows:
        return rows
    for path in glob.glob(os.path.join(directory, "**", "*.db"), recursive=True):
        cur = sqlite3.connect(path).cursor()
        cols = [r[1] for r in cur.execute("pragma table_info(kernels)")]
        name = "name" if "name" in cols else cols[0]
        for n, c, t in cur.execute(f"select {name}, count(*), sum(end-start) from kernels group by {name}"):
            c0, t0 = rows.get(n, (0, 0))
            rows[n] = (c0 + c, t0 + t)
    if not rows:
        raise SystemExit(f"{directory}: no kernel_stats.csv and no rocpd database with kernels")
    return rows


def frame_prep_per_step(directory, steps):
    """steps: the training steps the trace covers (--steps of the --steps-only run; Trainer.build's dry-run forward adds one statistics
    and one apply dispatch to the first of them)."""
    rows = kernel_stats(directory)
    prep = {n: v for n, v in rows.items() if FRAME_PREP.search(n)}
    if not prep:
        raise SystemExit(f"{directory}: no frame-prep kernel in the trace")
    short = lambda n: re.sub(r"\(.*", "", n.replace("void ", "").replace("lpm::", ""))[:90]
    return {"steps_traced": steps, "frame_prep_us_per_step": round(sum(t for _, t in prep.values()) / steps / 1e3, 2),
            "all_kernels_us_per_step": round(sum(t for _, t in rows.values()) / steps / 1e3, 1),
            "kernels": {short(n): {"calls_per_step": round(c / steps, 2), "us_per_step": round(t / steps / 1e3, 2)}
                        for n, (c, t) in sorted(prep.items(), key=lambda kv: -kv[1][1])}}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--configs", default="cfg2,cfg5")
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--clips", type=int, default=2560)
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--unique", type=int, default=64)
    ap.add_argument("--dir", default=None, help="where the temporary files go (default: the system's temporary directory)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps-only", default=None, metavar="CFG", help="run --steps training steps of CFG and exit (for a kernel trace)")
    ap.add_argument("--quantised", type=int, default=1, help="--steps-only: FLAGS.train_quantised_frames")
    ap.add_argument("--kernel-stats", nargs=2, default=None, metavar=("DIR_A", "DIR_B"),
                    help="summarise the frame-prep kernels of two rocprofv3 output directories (flag off, flag on)")
    ap.add_argument("--label", default=None, help="--kernel-stats: the configuration the traces were taken at")
    ap.add_argument("--merge-into", default=None, help="--kernel-stats: a JSON file of this tool to add the summary to")
    a = ap.parse_args()
    if a.kernel_stats:
        summary = {"config": a.label, "a_fp32_detour": frame_prep_per_step(a.kernel_stats[0], a.steps),
                   "b_quantised": frame_prep_per_step(a.kernel_stats[1], a.steps)}
        print(json.dumps(summary, indent=1))
        if a.merge_into:
            doc = json.load(open(a.merge_into))
            doc.setdefault("frame_prep_kernels", []).append(summary)
            json.dump(doc, open(a.merge_into, "w"), indent=1)
        return
    from tools.bench_reader import write_files
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        if a.steps_only:
            paths, _, _ = write_files(d, 8 * 128, 4, a.unique)
            steps_only(a.steps_only, a.quantised, a.steps, paths)
            return
        paths, clips, nbytes = write_files(d, a.clips, a.files, a.unique)
        out = []
        for cfg in a.configs.split(","):
            r = measure(cfg, paths, a.steps, a.reps, a.warmup)
            r.update(clips_per_epoch=clips, files=len(paths), mean_record_bytes=round(nbytes / clips))
            print(json.dumps(r), flush=True)
            out.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"measurements": out}, f, indent=1)


if __name__ == "__main__":
    main()
