#!/usr/bin/env python3
"""bench.py -- clips/sec of one full NetVladV1 training step (BASELINE.json metric).

  python bench.py --gpus 1 --steps K --warmup W
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
         bench.py --gpus N --steps K --warmup W

A "step" = fwd + bwd + gradient SUM all-reduce (RCCL) + per-variable clip + TF-Adam on one synthetic batch
already resident in HBM (the reference's `Examples/sec`, train.py:450-451).  Workload = BASELINE configs[1]:
NetVladV1 K=256 hidden=512, rgb+audio 1152-d, 300 frames, bs 80 per GPU (weak scaling: cfg-4 at 8 GPUs).
Rank 0 prints ONE JSON line.

A plain run does only what the headline needs: set-up, a fixed number of spin-up and warm-up steps, the K timed
steps, the outputs (``--dump-outputs DIR``) and the line.  ``--full`` adds everything else, as before:
`other_configs` (cfg3 and cfg5 timed in child processes), `roofline` for the residual-aggregation kernel (K2,
video stream) timed with HIP events on the launch stream inside the timed region, `assign_gemm`, `clip_adam`,
`gradient_state`, `dispatches_per_step`, `cpu_baseline` = the CPU oracle (fp32 torch restatement, oracle/) timed
on the host cores on a bounded sample with the `parity` check against it (N=1 only), and with N > 1 the
`collectives` trace and the `replicas` check.

``--dump-outputs DIR`` writes what the last timed step handed its caller as float32 .npy files (see
dump_outputs); with the same arguments every run starts from the same seeded weights and batches and runs the
same steps, so two builds can be compared output for output.
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
# RCCL's cross-process buffer sharing needs dmabuf IPC on this pool's host driver (already exported by the image; kept
# here so that a bare environment still works).  Must be set before the HIP runtime initialises.
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

METRIC = "clips/sec training step, NetVladV1 K=256 300-frame 1152-d, bs=80, 1/2/4/8 GPU"
MAX_FRAMES, FEATURE, VOCAB = 300, 1152, 3862
TRAIN = dict(base_learning_rate=0.0002, learning_rate_decay=0.85, learning_rate_decay_examples=4000000)
HBM_PEAK_GBS = 8000.0                                                    # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
# The workloads bench.py can time.  cfg2 (the default, what the driver runs) is the configuration BASELINE.json's metric is quoted on;
# cfg5 is BASELINE configs[4] at its per-GPU share (bs 1024 over 8 GPUs), the HBM-bound residual-aggregation showcase.
WORKLOADS = {
    "cfg2": dict(metric=METRIC, model_kwargs=dict(iterations=300, cluster_size=256, hidden_size=512),   # README.md:12-18, 300 frames
                 oracle=dict(iterations=300, cluster_size=256, hidden_size=512), flags={}, batch=80, elt=4, dtype="f32", parity_tol=1e-3,
                 workload="NetVladV1 K=256 hidden=512 rgb+audio 1152-d 300 frames, bs 80 per GPU (BASELINE configs[1]; configs[3] at "
                          "8 GPUs), full training step",
                 dtype_detail="fp32 storage and accumulation everywhere; K1, K2, K3, K4 feed the bf16 MFMA pipe with split-bf16 (hi+lo) operands, "
                              "3 MFMAs per product (~5e-6 relative error); the encoder dense GEMMs run on fp16 (hi, lo) planes with delayed "
                              "per-tensor power-of-two scales (ops.OperandScales): forward products 3 MFMAs (~1e-6); input-gradient products 2 MFMAs, "
                              "the weight rounded once to fp16 (measured against fp64: 2.1e-4 relative L2 per GEMM); weight-gradient products "
                              "1 MFMA, BOTH operands rounded once to fp16 (2.9e-4 relative L2; tests/test_gpu_fp16x2.py; LPM_DW_TERMS=2: the "
                              "gradient operand exact); LPM_DENSE_ARITHMETIC=bf16x3 runs the dense GEMMs as in rounds 1-4 (LPM_MHA_BWD_TERMS=2, not the "
                              "default: K4's backward products behind dS on 2 fp16 MFMAs)"),
    "cfg3": dict(metric="clips/sec training step, NetVladV2 (attention-based cluster similarities) K=256 300-frame 1152-d, bs=80 (BASELINE configs[2])",
                 model="NetVladV2", model_kwargs=dict(iterations=300, cluster_size=256, hidden_size=512),     # hidden: README.md:17
                 oracle=dict(iterations=300, cluster_size=256, hidden_size=512), flags={}, batch=80, elt=4, dtype="f32", parity_tol=1e-3,
                 dropout=True,      # the reference trains the frame encoders with dropout rate 0.9 (transformer_utils.py:450)
                 workload="NetVladV2 K=256 hidden=512 rgb+audio 1152-d 300 frames, bs 80 on one GPU (BASELINE configs[2]), full training "
                          "step with the reference's dropout on",
                 dtype_detail="fp32 storage and accumulation everywhere; K2, K3, K4 and the encoder dense GEMMs feed the bf16 MFMA pipe with "
                              "split-bf16 (hi+lo) operands, 3 MFMAs per product (the logits_bn attention forward too at 300 keys; exact fp32 below 128)"),
    "cfg5": dict(metric="clips/sec training step, gated NetVLAD K=512 + MoE-4, 300-frame 1152-d bf16, bs=128 per GPU (BASELINE configs[4])",
                 model_kwargs=dict(iterations=300, cluster_size=512, hidden_size=1024, encoder=False),
                 oracle=dict(iterations=300, cluster_size=512, hidden_size=1024, encoder=False, moe_num_mixtures=4),
                 flags=dict(moe_num_mixtures=4, netvlad_storage="bf16"), batch=128, elt=2, dtype="bf16", parity_tol=2e-2,
                 workload="gated NetVLAD (NetVladV1 without the cluster encoders) K=512/128 hidden=1024 MoE-4, rgb+audio 1152-d 300 "
                          "frames, bs 128 per GPU (BASELINE configs[4] = bs 1024 over 8 GPUs), full training step",
                 dtype_detail="bf16 storage of the frames, logits / assignment and pooled descriptor of both NetVLAD streams, one bf16 MFMA "
                              "per product with fp32 accumulation; batch statistics, norms, projection, gating, MoE, gradients and the "
                              "optimiser in fp32"),
}
# ms per step measured on one MI355X at the final code of round 6 (README): converts --spinup-seconds into a fixed step count
SPINUP_STEP_MS = {"cfg2": 6.7, "cfg3": 8.5, "cfg5": 5.3}


def set_flags(wl):
    from learnablepoolingmethods_amd import FLAGS
    for k, v in wl["flags"].items():
        setattr(FLAGS, k, v)


def synthetic_batch(batch, device, seed):
    """Reader-faithful synthetic input generated on the device: uint8 -> Dequantize
    (utils.py:28-43) -> zero the frames past num_frames (readers.py:189-193); 1-5 positive labels."""
    g = torch.Generator(device=device).manual_seed(seed)
    q = torch.randint(0, 256, (batch, MAX_FRAMES, FEATURE), device=device, generator=g, dtype=torch.uint8)
    nf = torch.randint(120, MAX_FRAMES + 1, (batch,), device=device, generator=g, dtype=torch.int32)
    raw = q.float() * (4.0 / 255.0) + (4.0 / 512.0 - 2.0)
    raw = raw * (torch.arange(MAX_FRAMES, device=device)[None, :, None] < nf[:, None, None])
    labels = torch.zeros(batch, VOCAB, dtype=torch.bool, device=device)
    npos = torch.randint(1, 6, (batch,), device=device, generator=g)
    idx = torch.randint(0, VOCAB, (batch, 5), device=device, generator=g)
    labels.scatter_(1, idx, torch.arange(5, device=device)[None, :] < npos[:, None])
    return raw, nf, labels


def k2_algorithmic_bytes(B, T, D, K, elt=4):
    """read assignment logits + frames once, W2 (fp32) once per batch, write the descriptor once."""
    return elt * (B * T * K + B * T * D + B * D * K) + 4 * D * K


def cpu_baseline(budget_s, wl):
    """The oracle's train_step (fp32, torch CPU) on a bounded sample of the same workload."""
    from oracle import lpm_oracle as O
    cfg = O.OracleConfig(model=wl.get("model", "NetVladV1"), **wl["oracle"], **TRAIN)
    b = 4
    torch.set_flush_denormal(True)   # as TF's CPU kernels do; g*g underflows to denormals in Adam otherwise (100x slower)
    x, nf, lab = O.make_synthetic_batch(b, MAX_FRAMES, FEATURE, VOCAB, seed=0)
    p = O.init_params(cfg, FEATURE, seed=1000)
    masks = None
    if wl.get("dropout"):            # NetVladV2: keep masks (rate 0.9) drawn here and handed to both sides of the parity check
        g = torch.Generator().manual_seed(5)
        masks = {"video": (torch.rand(b, MAX_FRAMES, 1024, generator=g) >= 0.9).float(),
                 "audio": (torch.rand(b, MAX_FRAMES, FEATURE - 1024, generator=g) >= 0.9).float()}
    st = {"step": 0, "m": {}, "v": {}}
    t0 = time.perf_counter()
    p0 = p
    p, st, info0 = O.train_step(p, st, x, nf, lab, cfg, 1, dropout_masks=masks)   # warm-up (page-in, thread pools); also the parity sample
    warm = time.perf_counter() - t0
    first = {"x": x, "nf": nf, "lab": lab, "params": p0, "loss": info0["loss"], "predictions": info0["predictions"], "masks": masks}
    times = []
    while len(times) < 5 and (sum(times) + warm) < budget_s:
        t0 = time.perf_counter()
        p, st, _ = O.train_step(p, st, x, nf, lab, cfg, 1, dropout_masks=masks)
        times.append(time.perf_counter() - t0)
    if not times:
        times = [warm]
    med = sorted(times)[len(times) // 2]
    return {"value": round(b / med, 3), "unit": "clips/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"oracle/lpm_oracle.train_step fp32 torch-CPU, the workload's layer sizes, batch {b} "
                      f"(1 warm-up + {len(times)} timed steps, median {med:.2f} s/step); stand-in for the TF1 "
                      f"reference, which cannot run here (SURVEY F2)"}, first


def parity_check(first, device, wl):
    """output parity asserted in the same run, outside the timed region.  The CPU baseline's first step (the oracle
    from its seeded reference-style initialisation on its seeded 4-clip batch of the bench workload's layer sizes) is repeated by
    the HIP path from the same weights: loss and predictions must agree to the north-star's 1e-3."""
    from learnablepoolingmethods_amd import registry
    from learnablepoolingmethods_amd.train import Trainer
    b = first["x"].shape[0]
    tol = wl["parity_tol"]
    tr = Trainer(registry.get_model(wl.get("model", "NetVladV1")), vocab_size=VOCAB, batch_size=b, device=device, seed=1,
                 model_kwargs=wl["model_kwargs"], **TRAIN)
    tr.build(first["x"], first["nf"], first["lab"])
    tr.store.load({"tower/" + k: v for k, v in first["params"].items()})
    kw = {} if first.get("masks") is None else {"dropout_masks": {k: v.to(device) for k, v in first["masks"].items()}}
    out = tr.step(first["x"], first["nf"], first["lab"], **kw)
    torch.cuda.synchronize()
    pred, ref = out["predictions"].double().cpu(), first["predictions"].double()
    e_pred = float((pred - ref).abs().max() / ref.abs().max())
    e_loss = abs(float(out["loss"]) - float(first["loss"])) / abs(float(first["loss"]))
    res = {"against": "cpu_baseline's first step (fp32 oracle, same weights, its 4-clip sample of the workload)",
           "predictions_max_rel_err": float(f"{e_pred:.3e}"), "loss_rel_err": float(f"{e_loss:.3e}"), "tolerance": tol,
           "ok": bool(e_pred <= tol and e_loss <= tol)}
    del tr
    torch.cuda.empty_cache()
    return res


class Watchdog:
    """Multi-rank runs only: a daemon thread that ends THIS rank with a non-zero exit code, after saying where it stood,
    when the main thread has not reported progress for ``limit`` seconds -- a hang in a collective (a peer that died, a
    rendezvous that never completed) then shows up in the driver's log as a named phase and collective instead of as a
    silent time-out of the whole run."""

    def __init__(self, rank, limit):
        import threading
        self.rank, self.limit = rank, limit
        self.phase, self.t = "start", time.monotonic()
        self.stop = False
        if limit > 0:
            threading.Thread(target=self._run, daemon=True).start()

    def tick(self, phase):
        self.phase, self.t = phase, time.monotonic()

    def _run(self):
        while not self.stop:
            time.sleep(1.0)
            idle = time.monotonic() - self.t
            if idle > self.limit:
                try:
                    from learnablepoolingmethods_amd import train
                    last = train.LAST_COLLECTIVE
                except Exception:
                    last = "unknown"
                sys.stderr.write(f"[bench.py rank {self.rank}] WATCHDOG: no progress for {idle:.0f} s in phase '{self.phase}'; "
                                 f"last collective on this rank: {last}\n")
                sys.stderr.flush()
                os._exit(3)


def self_launch(n, argv):
    """`python bench.py --gpus N` without a launcher: start the N ranks as FRESH child processes (torch.distributed.run, one
    per GPU, rendezvous on 127.0.0.1) and return the worst exit code.  This parent never initialises the GPU -- it counts devices
    with torch.cuda.device_count() only, which does not create a HIP context on this image -- and never execs: a process that has
    touched the GPU must not be replaced.  Rank 0's JSON line reaches stdout through the inherited pipe."""
    import socket
    import subprocess
    phase = "self-launch: device count"
    share = os.environ.get("LPM_SHARE_GPU") == "1"
    have = torch.cuda.device_count()
    if have < n and not share:
        sys.stderr.write(f"[bench.py] phase '{phase}': --gpus {n} but this box exposes {have} GPU(s); one rank per GPU is "
                         f"the only measured configuration (LPM_SHARE_GPU=1 shares GPU 0 over gloo, debug only)\n")
        return 4
    with socket.socket() as s:                       # a free rendezvous port
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__), *argv]
    phase = "self-launch: torch.distributed.run"
    sys.stderr.write(f"[bench.py] {phase}: {' '.join(cmd)}\n")
    sys.stderr.flush()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    rc = subprocess.call(cmd, env=env)
    if rc != 0:
        sys.stderr.write(f"[bench.py] phase '{phase}': the launcher returned {rc} (the failing rank's own message, with its phase "
                         f"and last collective, is above)\n")
    return rc


def run_all(argv):
    """`--config all`: every single-GPU BASELINE configuration through this same script, each in a FRESH child process (this parent
    never touches the GPU), their JSON lines relayed in the order cfg3, cfg5, cfg2 -- the line of the configuration BASELINE.json's
    metric is quoted on comes last.  Returns the worst exit code."""
    import subprocess
    rest, skip = [], False
    for a in argv:                                   # drop "--config all" / "--config=all"
        if skip:
            skip = False
        elif a == "--config":
            skip = True
        elif not a.startswith("--config="):
            rest.append(a)
    worst = 0
    for cfg in ("cfg3", "cfg5", "cfg2"):
        sys.stderr.write(f"[bench.py] --config all: {cfg}\n")
        sys.stderr.flush()
        rc = subprocess.call([sys.executable, os.path.abspath(__file__), "--config", cfg, *rest])
        worst = max(worst, rc)
    return worst


def other_configs(args):
    """``--full`` run of cfg2 on one GPU: BASELINE configs[2] (cfg3) and configs[4] at its per-GPU share (cfg5) timed by this same script
    in FRESH child processes BEFORE this process touches the GPU, their headline figures embedded in the cfg-2 line as ``other_configs`` --
    so that the driver's one command puts all three single-GPU configurations under its clock.  Each child: the same steps / warm-up,
    rotating batches, no CPU baseline (that is this line's ``cpu_baseline``), at most ``limit`` seconds."""
    import subprocess
    out = {}
    limit = 110.0
    for cfg in ("cfg3", "cfg5"):
        cmd = [sys.executable, os.path.abspath(__file__), "--config", cfg, "--gpus", "1", "--steps", str(args.steps), "--warmup",
               str(args.warmup), "--spinup-seconds", str(min(args.spinup_seconds, 2.0)), "--batches", str(args.batches),
               "--full", "--no-cpu-baseline", "--no-other-configs"] + (["--single-batch"] if args.single_batch else [])
        t0 = time.perf_counter()
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
            line = None
            for ln in r.stdout.splitlines():
                if ln.startswith("{") and '"metric"' in ln:
                    line = json.loads(ln)
            if r.returncode != 0 or line is None:
                out[cfg] = {"error": f"exit code {r.returncode}", "stderr_tail": r.stderr[-400:]}
                continue
            roof = line.get("roofline") or {}
            out[cfg] = {"metric": line["metric"], "value": line["value"], "unit": line["unit"], "ms_per_step": line["ms_per_step"],
                        "steps": line["steps"], "warmup": line["warmup"], "dtype": line["dtype"], "final_loss": line.get("final_loss"),
                        "workload": line["config"]["workload"],
                        "roofline": {k: roof.get(k) for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "avg_kernel_ms", "algorithmic_bytes",
                                                              "traffic", "traffic_measured_by_this_run", "traffic_source", "a5_chain_traffic")},
                        "a5_function_frac": (roof.get("a5_function") or {}).get("frac"),
                        "assign_gemm": line.get("assign_gemm"), "dispatches_per_step": (line.get("dispatches_per_step") or {}).get("value"),
                        "wall_seconds": round(time.perf_counter() - t0, 1)}
        except subprocess.TimeoutExpired:
            out[cfg] = {"error": f"no line within {limit:.0f} s"}
        except Exception as ex:                       # never a reason to lose the headline line
            out[cfg] = {"error": f"{type(ex).__name__}: {ex}"}
    return out


def count_dispatches(step):
    """Kernel launches of ONE steady-state step, counted live (outside the timed region) with torch.profiler's device activity trace,
    which sees every kernel of the process -- the library's ctypes launches included.  -> dict or None (profiler unavailable)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        step()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        dur = []
        for e in prof.events():
            if e.device_type == torch.autograd.DeviceType.CUDA and not any(w in e.name for w in ("Memcpy", "Memset", "memcpy", "memset")):
                dur.append(float(getattr(e, "device_time", 0.0) or getattr(e, "cuda_time", 0.0) or 0.0))
        if not dur:
            return None
        small = [d for d in dur if d < 8.0]
        return {"value": len(dur), "measured": True, "launches_under_8us": len(small), "under_8us_total_us": round(sum(small), 1),
                "source": "torch.profiler device activity of one step after the timed region"}
    except Exception as ex:                          # the count is a diagnostic, never a reason to fail the bench
        sys.stderr.write(f"[bench.py] dispatch count unavailable: {type(ex).__name__}: {ex}\n")
        return None


def dump_outputs(path, out, trainer, per_variable=16384, seed=0):
    """``--dump-outputs``: what the last timed step handed its caller, as float32 .npy files in ``path``:
      predictions.npy  [batch, vocab]  the step's predictions (rank 0's shard)
      loss.npy         []              its label loss
      variables.npy    [n]             the model's variables after the step's update, every variable of the store in name order:
                                       all entries of one with at most ``per_variable`` of them, else ``per_variable`` entries at
                                       positions drawn (with replacement, sorted) from a CPU generator seeded with ``seed`` afresh
                                       for each variable -- the same positions in every run and every build.
    A few MB in all at the benched configurations."""
    import numpy as np
    if trainer.sharded is not None:
        trainer.sharded.wait_parameters()
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "predictions.npy"), out["predictions"].detach().float().cpu().numpy())
    np.save(os.path.join(path, "loss.npy"), out["loss"].detach().float().cpu().numpy())
    g = torch.Generator()
    parts = []
    for name in sorted(trainer.store.vars):
        v = trainer.store.vars[name].detach()
        if not v.is_floating_point():
            continue
        flat = v.reshape(-1)
        if flat.numel() > per_variable:
            g.manual_seed(seed)
            idx = torch.randint(0, flat.numel(), (per_variable,), generator=g).sort().values
            flat = flat[idx.to(flat.device)]
        parts.append(flat.float().cpu())
    np.save(os.path.join(path, "variables.npy"), torch.cat(parts).numpy())


def replica_check(trainer, world, group=None):
    """After the timed region: do all towers hold the same parameters?  Data-parallel replicas apply identical updates (train.py:266-336:
    shared variables in the reference) -- on the sharded route each rank updates its 1/N of hidden1_weights and the all-gather hands
    everyone the rest: a rank that missed a collective or read the variable before its gather landed shows up here.  A collective: every
    rank calls it.  (tests/test_dp_gloo.py runs it over gloo at world 8.)"""
    if trainer.sharded is not None:
        trainer.sharded.wait_parameters()
    pd = trainer.arena.param.double()
    cs = torch.stack([pd.sum(), (pd * pd).sum(), pd.abs().max()])
    del pd
    allcs = [torch.empty_like(cs) for _ in range(world)]
    dist.all_gather(allcs, cs, group=group)
    dev_ = max(float((c - allcs[0]).abs().max()) for c in allcs)
    route = "sharded (C)" if trainer.sharded is not None else ("factored (B)" if trainer.factored is not None else "all-reduce (A)")
    return {"consistent": dev_ == 0.0, "max_checksum_difference": dev_, "hidden1_weights_route": route,
            "checked": "sum, sum of squares and max |.| of the whole parameter arena, float64, every rank against rank 0"}


def dry_run_model(args):
    """--dry-run-model: the communication cost of one data-parallel step of ``--config`` over ``--gpus`` towers as FORMULAS with the bus
    bandwidth left as the variable (no GPU, no process group).  Per route of hidden1_weights (train.Trainer.build):
      A  bucket all-reduce of its gradient:            t = 2 (N - 1) / N * S_h1 / bw
      B  all-gather of the two gradient factors:       t = (N - 1) * (S_x + S_dy) / bw           (<= 4 towers)
      C  reduce-scatter + parameter all-gather:        t = (N - 1) / N * S_h1 / bw each          (the default beyond 4 towers)
    and for every other bucket t = 2 (N - 1) / N * S / bw.  ``bw`` is RCCL's bus bandwidth on this node -- what the first real run's
    ``collectives`` block measures; the table evaluates the formulas at 100 ... 400 GB/s (xGMI: 7 links x ~153 GB/s per GPU, point to
    point: a ring is per-link bound).  Windows: the N = 1 step's phases measured on one MI355X (profiles/r06_*)."""
    wl = WORKLOADS[args.config]
    N = max(2, args.gpus)
    mk = wl["model_kwargs"]
    K, H, B = mk["cluster_size"], mk["hidden_size"], wl["batch"]
    n1 = 1024 * K + 128 * (K // 4)
    s_h1 = 4 * n1 * H
    m = wl.get("flags", {}).get("moe_num_mixtures", 2)
    s_head = 4 * (H * VOCAB * (m + 1) + H * VOCAB * m + H * H + 4 * H)
    enc = mk.get("encoder", True) and wl.get("model", "NetVladV1") == "NetVladV1"
    s_enc = 4 * (12 * 1024 * 1024 + 12 * 128 * 128) if enc else (4 * (4 * 1024 * 1024 + 2 * 1024 * 4096 + 4096 * K) if wl.get("model") == "NetVladV2" else 0)
    s_pool = 4 * 2 * (1024 * K + 128 * (K // 4)) + 4 * 4 * 1152
    s_fact = 2 * 2 * (B * n1 + B * H)                 # split-bf16 tiles of X [B, n1] and DY [B, H] per tower
    rows = [("head bucket all-reduce", s_head, lambda bw: 2 * (N - 1) / N * s_head / bw),
            ("encoder bucket all-reduce", s_enc, lambda bw: 2 * (N - 1) / N * s_enc / bw),
            ("pooling bucket all-reduce", s_pool, lambda bw: 2 * (N - 1) / N * s_pool / bw),
            ("hidden1 route A: all-reduce", s_h1, lambda bw: 2 * (N - 1) / N * s_h1 / bw),
            ("hidden1 route B: all-gather of factors", s_fact, lambda bw: (N - 1) * s_fact / bw),
            ("hidden1 route C: reduce-scatter", s_h1, lambda bw: (N - 1) / N * s_h1 / bw),
            ("hidden1 route C: parameter all-gather", s_h1, lambda bw: (N - 1) / N * s_h1 / bw)]
    bws = [100, 200, 300, 400]
    out = {"config": args.config, "towers": N, "per_rank_batch": B, "formula": {
               "all_reduce": "2 (N - 1) / N * bytes / bw", "reduce_scatter / all_gather": "(N - 1) / N * bytes / bw",
               "all_gather of per-tower factors": "(N - 1) * bytes_per_tower / bw"},
           "ms_at_bus_GBps": {str(b): {} for b in bws}, "bytes": {}}
    for name, nbytes, f in rows:
        out["bytes"][name] = int(nbytes)
        for b in bws:
            out["ms_at_bus_GBps"][str(b)][name] = round(1e3 * f(b * 1e9), 3)
    out["default_route"] = "B (factored)" if N <= 4 else "C (sharded)"
    out["note"] = ("bw = RCCL bus bandwidth on the node, unmeasured (no multi-GPU node has been available in six rounds); the first real "
                   "run prints window_ms / exposed_ms per collective (train.CollectiveTrace) and replaces this table")
    print(json.dumps(out))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=20)   # a cold box needs ~0.2 s of load before clocks and caches settle
    ap.add_argument("--spinup-seconds", type=float, default=3.0,
                    help="untimed steps before the W warm-up steps, about this much wall time of them at the workload's measured "
                         "step time (SPINUP_STEP_MS; a fixed count, so that a run's steps depend on its arguments alone): a GPU that "
                         "has been idle needs a few seconds of load before its clocks settle (measured: 7.1-7.6k clips/s in the "
                         "first second, 8.4-8.7k afterwards)")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline: other_configs, roofline and kernel figures, gradient state, dispatch count, "
                         "cpu_baseline + parity, and with N > 1 the collective trace and the replica check")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed (predictions, loss, a fixed sample of the updated "
                         "variables) as float32 .npy files under DIR (rank 0)")
    ap.add_argument("--batches", type=int, default=8, help="distinct resident synthetic batches rotated through every step (seeds rank * N + i)")
    ap.add_argument("--single-batch", action="store_true", help="one batch for every step (the behaviour of rounds 1-4), for an A/B")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="--full run (cfg2, one GPU): do not time cfg3 and cfg5 in child processes first (see other_configs)")
    ap.add_argument("--cpu-baseline-seconds", type=float, default=25.0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-dispatch-count", action="store_true",
                    help="skip the live launch count (one more step under torch.profiler after the timed region): for runs that already "
                         "sit under rocprofv3")
    ap.add_argument("--config", choices=sorted(WORKLOADS) + ["all"], default="cfg2",
                    help="cfg2 (default): the configuration BASELINE.json's metric is quoted on; cfg3: BASELINE configs[2] (NetVladV2); "
                         "cfg5: BASELINE configs[4] per GPU; all: cfg3, cfg5, cfg2 one after the other, each in a fresh process -- three "
                         "JSON lines, the BASELINE metric's (cfg2) last")
    ap.add_argument("--watchdog-seconds", type=float, default=240.0,
                    help="N > 1 only: a rank that makes no progress for this long prints its phase and last collective and exits 3")
    ap.add_argument("--dry-run-model", action="store_true",
                    help="print the per-collective cost formulas of a data-parallel step over --gpus towers (no GPU needed) and exit")
    args = ap.parse_args()

    if args.dry_run_model:
        raise SystemExit(dry_run_model(args))
    if args.config == "all":
        raise SystemExit(run_all(sys.argv[1:]))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(self_launch(args.gpus, sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    others = None
    profiled = any(k.startswith(("ROCPROF", "ROCP_")) for k in os.environ) or "rocprof" in os.environ.get("LD_PRELOAD", "")
    if (args.full and args.config == "cfg2" and world == 1 and args.gpus == 1 and not args.no_other_configs and not profiled
            and not any(k.startswith("LPM_") for k in os.environ)):
        others = other_configs(args)                 # child processes, before this one initialises the GPU
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the hot path has no CPU fallback")
    # LPM_SHARE_GPU=1 (debug only): several ranks on ONE GPU over gloo, to exercise the data-parallel code path on a
    # single-GPU box; the measured configuration is always one rank per GPU over RCCL.
    share = os.environ.get("LPM_SHARE_GPU") == "1"
    if os.environ.get("LPM_SINGLE_STREAM") == "1":     # profiling only: per-kernel durations without a concurrent neighbour
        from learnablepoolingmethods_amd import FLAGS as _flags
        _flags.audio_side_stream = False
        _flags.hidden1_update_stream = False
    dev_index = 0 if share else local_rank
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    dog = Watchdog(rank, args.watchdog_seconds if world > 1 else 0)
    if world > 1:
        import datetime
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dog.tick("init_process_group (rendezvous)")
        to = datetime.timedelta(seconds=max(60.0, 2 * args.watchdog_seconds))   # RCCL's own watchdog, behind ours
        if share:
            dist.init_process_group("gloo", timeout=to)
        else:
            dist.init_process_group("nccl", device_id=device, timeout=to)       # nccl == RCCL on ROCm
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"

    from learnablepoolingmethods_amd import FLAGS, ops, registry
    from learnablepoolingmethods_amd.train import Trainer

    wl = WORKLOADS[args.config]
    set_flags(wl)
    # A/B on a real node (default: the route Trainer.build agrees on from the tower count): LPM_HIDDEN1_ROUTE=sharded | factored | allreduce
    route_env = os.environ.get("LPM_HIDDEN1_ROUTE")
    if route_env == "sharded":
        FLAGS.hidden1_sharded_update, FLAGS.hidden1_sharded_min_towers = True, 2
    elif route_env == "factored":
        FLAGS.hidden1_factored_update, FLAGS.hidden1_factored_max_towers, FLAGS.hidden1_sharded_update = True, 64, False
    elif route_env == "allreduce":
        FLAGS.hidden1_factored_update, FLAGS.hidden1_sharded_update = False, False
    elif route_env:
        raise SystemExit(f"LPM_HIDDEN1_ROUTE={route_env!r}: sharded | factored | allreduce")
    PER_GPU_BATCH = wl["batch"]
    model = registry.get_model(wl.get("model", "NetVladV1"))
    trainer = Trainer(model, vocab_size=VOCAB, batch_size=PER_GPU_BATCH, device=device, seed=1234, model_kwargs=wl["model_kwargs"], **TRAIN)
    # The reference's Examples/sec is quoted on FRESH batches (train.py:446-451): ``--batches`` (default 8) distinct synthetic batches,
    # all resident in HBM, rotate through spin-up, warm-up and the timed steps (seeds rank * NB + i), so that the timed steps do not run
    # on a model over-fitted to one batch (round 4: the loss of the single-batch run froze at 5.2861 with vanishing gradients, and kernel
    # time depends on operand data).  ``--single-batch`` keeps the old behaviour for an A/B.
    NB = 1 if args.single_batch else max(1, args.batches)
    batches = [synthetic_batch(PER_GPU_BATCH, device, seed=rank * NB + i) for i in range(NB)]
    raw, nf, labels = batches[0]
    counter = [0]

    def next_step():
        b = batches[counter[0] % NB]
        counter[0] += 1
        return trainer.step(*b)

    def barrier(what="barrier"):
        dog.tick(what)
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        dog.tick(what + " done")

    # device spin-up: every rank runs the SAME number of untimed steps (the step contains collectives), sized on rank 0
    spin = 0
    if args.spinup_seconds > 0:
        dog.tick("first steps (variable creation, arena broadcast, library set-up)")
        for _ in range(2):                                   # builds the variables / arenas, first-use library set-up
            next_step()
        torch.cuda.synchronize()
        dog.tick("spin-up steps")
        # a count fixed by the arguments (not by a clock): the timed steps then start from the same state in every run
        spin = 2 + math.ceil(1000.0 * args.spinup_seconds / SPINUP_STEP_MS[args.config])
        for i in range(spin - 2):
            next_step()
            if i % 32 == 0:
                torch.cuda.synchronize()
                dog.tick(f"spin-up step {i}")
        torch.cuda.synchronize()
    dog.tick("warm-up steps")
    for _ in range(args.warmup):
        next_step()
    from learnablepoolingmethods_amd import _capi
    lib = _capi.load()
    if args.full:
        ops.KERNEL_TIMELINE = []
        lib._lpm_kernel_timing_enable(1)   # K1 / K2 launches carry their own start/stop HIP events (kernel duration proper)
        if world > 1:
            from learnablepoolingmethods_amd import train as _train
            _train.TRACE.on = True         # three compute-stream events per collective: the overlap evidence printed below
    barrier("barrier before the timed steps")
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = next_step()
    barrier("barrier after the timed steps")
    elapsed = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, out, trainer)
    grad_state, timeline, dispatches = None, [], None
    k1_ms = k2_ms = at_ms = fin_ms = []
    if args.full:
        # the state the timed steps ran in: how much of the last timed step's gradient is exactly zero (a saturated, frozen model shows
        # up here).  hidden1_weights' slice is left out on the routes that never write its gradient (factored / sharded update).
        ga = trainer.arena
        g0 = ga.offsets_host[1] if (trainer.factored is not None or trainer.sharded is not None) else 0
        gsl = ga.grad[g0:]
        grad_state = {"zero_fraction": round(float((gsl == 0).float().mean()), 6) if gsl.numel() else None,
                      "max_abs": float(f"{float(gsl.abs().max()):.3e}") if gsl.numel() else None, "entries": int(gsl.numel()),
                      "of": "the gradient arena after the last timed step" + (" without hidden1_weights (its gradient is never written on this "
                                                                              "route)" if g0 else "")}
        timeline, ops.KERNEL_TIMELINE = ops.KERNEL_TIMELINE, None
        lib._lpm_kernel_timing_enable(0)
        dispatches = count_dispatches(next_step) if (world == 1 and not args.no_dispatch_count) else None

        def kernel_ms(tag):
            import ctypes
            buf = (ctypes.c_float * 4096)()
            n = lib._lpm_kernel_timing_read(tag, buf, 4096)
            return [float(buf[i]) for i in range(n)]
        k1_ms, k2_ms = kernel_ms(1), kernel_ms(2)
        at_ms, fin_ms = kernel_ms(3), kernel_ms(4)
    replicas = None
    collectives = None
    if world > 1:
        t = torch.tensor([elapsed], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        if args.full:
            _train.TRACE.on = False
            collectives = _train.TRACE.summary()   # rank 0's view: window = compute between a collective's launch and its wait, exposed = the stall
            # after the timed region: do all towers hold the same parameters?  (data-parallel replicas apply identical updates -- on the
            # sharded route each rank updates its 1/N of hidden1_weights and the all-gather hands everyone the rest: a rank that missed a
            # collective or read the variable before its gather landed shows up here, on the first real multi-GPU run as well)
            dog.tick("replica consistency check (all_gather of parameter checksums)")
            replicas = replica_check(trainer, world)
    loss = float(out["loss"])

    if rank == 0:
        global_batch = PER_GPU_BATCH * world
        ms = 1000.0 * elapsed / args.steps
        value = global_batch * args.steps / elapsed
        # dominant north-star kernel: K2 residual aggregation on the video stream (D=1024)
        k2 = [(d, a.elapsed_time(b)) for (n, d, a, b) in timeline if n == "vlad_aggregate_fwd" and d[2] == 1024]
        k1 = [(d, a.elapsed_time(b)) for (n, d, a, b) in timeline if n == "assign_gemm_fwd" and d[1] == 1024]
        roof = None
        if k2:
            B, T, D, K = k2[0][0]
            # duration of the kernel itself (start/stop events attached to the launch, on its stream, inside the timed
            # steps); the event pairs recorded AROUND the launch call also bracket cross-queue dispatch gaps now that the
            # audio branch runs on a second stream, and are kept only as a fallback
            avg_ms = sum(k2_ms) / len(k2_ms) if k2_ms else sum(t for _, t in k2) / len(k2)
            elt = wl["elt"]
            bytes_ = k2_algorithmic_bytes(B, T, D, K, elt)
            ach = bytes_ / (avg_ms * 1e-3) / 1e9
            prec = ops.VLAD_PRECISION
            if elt == 2 and ops.VLAD_CLIP16 and lib._lpm_vlad_clip16_slabs(D, K):
                kname = ("vlad_clip16_kernel (K2, video stream, plain bf16 tiles, one MFMA per product, LDS-DMA, clip-wide items: 256 clusters "
                         "x a third of a clip's columns per workgroup, 2 x 6 register tiles)")
            elif elt == 2:
                kname = "vlad_aggregate_tiles3_kernel<false,1> (K2, video stream, plain bf16 tiles, one MFMA per product, LDS-DMA)"
            elif prec == "bf16x3" and ops.VLAD_TILES3 and ops.VLAD_KMAJOR_SCALED and args.config == "cfg2":
                kname = ("vlad_kmajor_kernel (K2 + row scales, video stream, split-bf16 MFMA, LDS-DMA tiles, 256 x 128 and 128 x 128 "
                         "workgroup items)")
            elif (prec == "bf16x3" and ops.VLAD_TILES3 and ops.VLAD_CLIP and args.config in ("cfg2", "cfg3") and FLAGS.netvlad_lazy_descriptor
                  and lib._lpm_vlad_clip_slabs(D, K)):
                kname = ("vlad_clip_kernel (K2, video stream, split-bf16 MFMA, LDS-DMA tiles, clip-wide items: all 256 clusters x a "
                         "third of a clip's columns per workgroup" + ("; sums leave d-major)" if args.config == "cfg3" else ")"))
            elif prec == "bf16x3":
                kname = ("vlad_aggregate_tiles3_kernel (K2, video stream, split-bf16 MFMA, LDS-DMA tiles)" if ops.VLAD_TILES3
                         else "vlad_aggregate_tiles_kernel<8> (K2, video stream, split-bf16 MFMA, register streaming)")
            else:
                kname = "vlad_aggregate_kernel<8,4,true> (K2, video stream, exact-fp32 MFMA)"
            roof = {"kernel": kname, "bound": "hbm", "achieved": round(ach, 1),
                    "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 4), "traffic": None,
                    "algorithmic_bytes": bytes_, "avg_kernel_ms": round(avg_ms, 4), "launches": len(k2_ms) or len(k2),
                    "timing": "HIP events attached to the launch (hipExtLaunchKernelGGL) inside the timed steps" if k2_ms
                              else "HIP event pairs around the launch call",
                    "flops_per_launch": 2.0 * B * T * D * K,
                    "achieved_tflops": round(2.0 * B * T * D * K / (avg_ms * 1e-3) / 1e12, 2)}
            for nm in ("split_frames", "assign_tiles"):
                tt = [a.elapsed_time(b) for (n, d, a, b) in timeline if n == nm and d[2] in (1024, 256)]
                if tt:
                    roof[nm + "_avg_ms"] = round(sum(tt) / len(tt), 4)
            # HBM bytes per launch of this kernel from the PMC passes (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate runs,
            # tools/pmc_a5.sh -> tools/pmc_to_json.py, the guide's gfx950 corrections); the file names its commit
            # NOT measured by this run: a profiler cannot sit inside the timed region.  The figure is attached only when it describes the
            # kernel this run timed (same kernel name) and no A/B switch of the library is set in the environment.
            pmc = os.path.join(ROOT, "profiles", f"a5_hbm_traffic_{args.config}.json")
            ab = sorted(k for k in os.environ if k.startswith("LPM_") and k not in ("LPM_SHARE_GPU", "LPM_DP_BACKEND", "LPM_SINGLE_STREAM"))
            if os.path.exists(pmc) and not ab:
                try:
                    pj = json.load(open(pmc))
                    if str(pj.get("k2_kernel", "")).split("<")[0].split("::")[-1] == kname.split(" ")[0].split("<")[0]:
                        roof["traffic"] = pj.get("k2_bytes_per_launch")
                        roof["traffic_measured_by_this_run"] = False
                        roof["traffic_source"] = (f"profiles/a5_hbm_traffic_{args.config}.json, rocprofv3 --pmc passes taken at commit "
                                                  f"{pj.get('commit')}: {pj.get('k2_kernel')}")
                        roof["a5_chain_traffic"] = pj.get("chain_bytes_per_launch")
                except Exception:
                    pass
            # the WHOLE a5 function (frame_level_models.py:2798-2822: BN-affine + softmax -> residual aggregation -> both
            # normalisations) as the chain of launches that computes it for the video stream: assignment tiles + K2 + finalize.
            # Durations of the kernels themselves (start / stop events attached to each launch).
            if at_ms and k2_ms:
                chain = {"assign_tiles": sum(at_ms) / len(at_ms), "vlad_aggregate": avg_ms}
                launches = "lpm_assign_tiles + K2 with the row scales inside (lpm_vlad_aggregate_kmajor_scaled_fwd), video stream"
                if fin_ms:           # forms with a separate finalize / row-scale launch
                    chain["vlad_finalize"] = sum(fin_ms) / len(fin_ms)
                    launches = "lpm_assign_tiles + K2 + finalize / row scales (video stream)"
                tot = sum(chain.values())
                roof["a5_function"] = {"launches": launches,
                                       "kernel_ms": {k: round(v, 4) for k, v in chain.items()}, "total_ms": round(tot, 4),
                                       "algorithmic_bytes": bytes_, "achieved": round(bytes_ / (tot * 1e-3) / 1e9, 1), "unit": "GB/s",
                                       "frac": round(bytes_ / (tot * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                       "timing": "HIP events attached to each launch (kernel durations; gaps between the launches excluded)"}
        line = {"metric": wl["metric"], "value": round(value, 2), "unit": "clips/s", "n_gpus": world, "steps": args.steps,
                "warmup": args.warmup, "spinup_steps": spin, "ms_per_step": round(ms, 3), "higher_is_better": True, "scaling": "weak",
                "vs_baseline": None, "dtype": wl["dtype"], "data": "synthetic", "dtype_detail": wl["dtype_detail"],
                "config": {"workload": wl["workload"], "global_batch": global_batch, "seq_len": MAX_FRAMES, "parallelism": f"dp{world}"},
                "final_loss": round(loss, 4),
                "batches": {"distinct": NB, "seeds": f"rank * {NB} + i, i < {NB}", "rotation": "spin-up, warm-up and timed steps take them in turn; all resident in HBM"}}
        if grad_state is not None:
            line["gradient_state"] = grad_state
        # launches per step: counted live, on one more step AFTER the timed region (single GPU: the extra steps hold collectives otherwise)
        if world == 1 and dispatches is not None:
            line["dispatches_per_step"] = dispatches
        if replicas is not None:
            line["replicas"] = replicas
        if collectives:
            line["collectives"] = {"per_step_rank0": collectives,
                                   "what": "compute-stream events around every asynchronous collective of the timed steps: window_ms = compute "
                                           "between launch and wait (what it could hide under), exposed_ms = how long the compute stream stood "
                                           "still for it (train.CollectiveTrace)"}
        if others is not None:
            line["other_configs"] = others
        sc = getattr(trainer, "operand_scales", None)
        if sc is not None and sc.slots:
            rep = sc.report()
            line["operand_formats"] = {"encoder_gemm_steps_on_fp16_planes": sc.steps_fp16, "steps_run": sc.step + 1, "sites": len(rep),
                                       "log2_scale_range": [int(min(__import__("math").log2(v[1]) for v in rep.values())),
                                                            int(max(__import__("math").log2(v[1]) for v in rep.values()))],
                                       "what": "NetVladV1's encoder GEMMs: steps that ran on fp16 planes (the first steps of a run stay on split-bf16 "
                                               "until every operand's max |x| has been read back once), operand sites and their power-of-two scales"}
        if roof:
            line["roofline"] = roof
        if k1:
            M, D, K = k1[0][0]
            avg_ms = sum(k1_ms) / len(k1_ms) if k1_ms else sum(t for _, t in k1) / len(k1)
            fl = 2.0 * M * D * K
            if wl["elt"] == 2:
                line["assign_gemm"] = {"avg_kernel_ms": round(avg_ms, 4), "tflops": round(fl / (avg_ms * 1e-3) / 1e12, 2),
                                       "mfma": "v_mfma_f32_32x32x16_bf16 (plain bf16 operands, fp32 accumulate)",
                                       "mfma_util_vs_bf16_peak": round(fl / (avg_ms * 1e-3) / 2.5e15, 3)}
            elif ops.ASSIGN_PRECISION == "bf16x3":
                # split-bf16: 3 bf16 MFMAs per product -> matrix-pipe utilisation = 3 x useful flops / dense bf16 peak
                line["assign_gemm"] = {"avg_kernel_ms": round(avg_ms, 4), "tflops": round(fl / (avg_ms * 1e-3) / 1e12, 2),
                                       "mfma": "v_mfma_f32_32x32x16_bf16 x3 (split-bf16 operands, fp32 accumulate)",
                                       "executed_bf16_tflops": round(3 * fl / (avg_ms * 1e-3) / 1e12, 1),
                                       "mfma_util_vs_bf16_peak": round(3 * fl / (avg_ms * 1e-3) / 2.5e15, 3)}
            else:
                line["assign_gemm"] = {"avg_kernel_ms": round(avg_ms, 4), "tflops": round(fl / (avg_ms * 1e-3) / 1e12, 2),
                                       "mfma": "v_mfma_f32_32x32x2_f32 (exact fp32, peak 157.3 TFLOP/s)"}
        k5 = [(d, a.elapsed_time(b)) for (n, d, a, b) in timeline if n == "clip_adam"]
        k5f = [(d, a.elapsed_time(b)) for (n, d, a, b) in timeline if n == "factored_clip_adam"]
        if k5 or k5f:
            # generic part: p, m, v read + written (24 B), g read by the norm pass and by the update (8 B).  Factored part
            # (hidden1_weights, lpm_factored_clip_adam): p, m, v read + written (24 B per parameter) + the two factors' tiles read by
            # each of its two passes; its gradient (4 B written + 8 B read on the generic path) is never in memory.
            total = k5[0][0][0] if k5 else 0
            avg_ms = (sum(t for _, t in k5) / len(k5) if k5 else 0.0) + (sum(t for _, t in k5f) / len(k5f) if k5f else 0.0)
            byts = 32.0 * total
            kernels = "ca_chunk_sumsq + ca_tensor_factor + ca_apply (K5: per-variable clip + Adam over the arena)"
            if k5f:
                R, N1, N2 = k5f[0][0]
                byts += 24.0 * N1 * N2 + 2 * 4.0 * R * (N1 + N2)
                kernels = ("hidden1_weights: tile GEMM (norm pass) + fa_factor + tile GEMM (clip + Adam epilogue), gradient never written; "
                           "the other variables: " + kernels)
            line["clip_adam"] = {"kernels": kernels, "bound": "hbm", "avg_ms": round(avg_ms, 4), "algorithmic_bytes": int(byts),
                                 "achieved": round(byts / (avg_ms * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                 "frac": round(byts / (avg_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
            if k5f:
                line["clip_adam"]["factored_avg_ms"] = round(sum(t for _, t in k5f) / len(k5f), 4)
        if world == 1 and args.full and not args.no_cpu_baseline:
            line["cpu_baseline"], first = cpu_baseline(args.cpu_baseline_seconds, wl)
            line["parity"] = parity_check(first, device, wl)
        print(json.dumps(line), flush=True)
        if "parity" in line and not line["parity"]["ok"]:
            raise SystemExit(f"bench.py: parity check failed: {line['parity']}")
    if world > 1:
        barrier("final barrier")            # tear the process group down together (rank 0 was busy printing)
        dog.tick("destroy_process_group")
        dist.destroy_process_group()
    dog.stop = True


if __name__ == "__main__":
    main()
