"""Evaluation loop and command line (reference: eval.py, minus the TensorFlow plumbing: sessions and queue runners).

  eval.py:152-155            the loss of a model without a "loss" output: losses.py:41-51 CrossEntropyLoss on the predictions
                             -> lpm_eval_rows' loss_row (device) / ``cross_entropy_rows`` (host)
  eval.py:186-289            evaluation_loop: predictions of every labelled batch into EvaluationMetrics, then get()   -> ``evaluate``
  eval_util.py:138-221       EvaluationMetrics: accumulate / get / clear                                   -> ``DeviceEvaluationMetrics``
  eval_util.py:26-68         Hit@1, PERR: per-row terms from one HIP pass (ops.eval_rows / lpm_eval_rows), fp64 means on the device
  eval_util.py:71-135,
  (mean_)average_precision_calculator.py
                             GAP and per-class AP over the pooled top-k (class, value, label) triplets, once per epoch
  utils.py:99-142            AddEpochSummary's info line                                                   -> ``format_epoch_summary``
  utils.py:55-96             AddGlobalStepSummary: every batch's scalars and info line         -> ``evaluate(on_batch=...)``, ``format_batch_summary``
  eval.py:292-349            evaluate(): model_flags.json, the reader, the loss, the loop over checkpoints -> ``main``, ``run``, ``evaluate_latest``

``python -m learnablepoolingmethods_amd.evaluation --train_dir D --eval_data_pattern 'files*'`` watches D: every ``--poll_seconds`` it takes
the newest ``model.ckpt-<step>.pt`` (training.run renames a finished file into place), evaluates it over the files, logs every batch's
and the epoch's line and writes their scalars into an event file in ``--summary_dir`` (default: D, where eval.py writes them).

``DeviceEvaluationMetrics.accumulate`` launches lpm_eval_rows and appends its outputs to device buffers; it makes no host sync and
returns the batch's hit_at_one, perr and loss as 0-d device tensors.  With FLAGS.eval_stats_fused the batch means, the loss sum and the
per-class label counts behind it are ONE more launch (lpm_eval_batch_stats) instead of about ten small torch launches.  ``get`` reduces
everything in fp64 on the device with eval_util's definitions (PERR per row as hits_at_n / n; AP: pooled order, stable descending sort, the positives of a class as the
recall denominator) and copies the results to the host once.

The loss is the reference's CrossEntropyLoss of the predictions (eval.py takes it because MoeModel returns no "loss"), not the fused
head's cancellation-free loss that Trainer.step reports.

Tie rule: the device path ranks ties as a stable descending sort -- equal predictions by ascending class index inside a row (the arg-max
of Hit@1 is the lowest such index), pooled entries in pooled order.  eval_util's torch.topk leaves the order among ties unspecified and
the reference shuffles them (random.seed(0)), so the paths agree exactly whenever the ranked predictions are distinct.
"""
from __future__ import annotations

import argparse
import logging
import os
import time
from typing import Callable, Dict, List, Optional

import numpy as np
import torch

from . import FLAGS, eval_util, ops
from ._capi import LpmError

_CPU_HINT = "use eval_util.EvaluationMetrics for CPU tensors"


def cross_entropy_rows(predictions, labels) -> torch.Tensor:
    """-> fp64 [B]: sum over every row of -[y log(p + 1e-5) + (1 - y) log(1 - p + 1e-5)] (losses.py:41-51 before its batch mean), the
    terms in fp32, the sums in fp64: what lpm_eval_rows writes as loss_row, for any device."""
    p = torch.as_tensor(predictions, dtype=torch.float32)
    f = torch.as_tensor(labels).to(device=p.device, dtype=torch.float32)
    t = f * torch.log(p + 1e-5) + (1 - f) * torch.log(1 - p + 1e-5)
    return -(t.to(torch.float64).sum(dim=1))


def _average_precision(pred, lab, numpos):
    """eval_util._average_precision as a 0-d fp64 device tensor (numpos: a 0-d tensor)."""
    order = pred.argsort(descending=True, stable=True)
    pos = (lab[order] > 0).to(torch.float64)
    cum = pos.cumsum(0)
    ranks = torch.arange(1, pos.numel() + 1, device=pos.device, dtype=torch.float64)
    s = (pos * cum / ranks).sum()
    return torch.where(numpos > 0, s / numpos.clamp_min(1.0), torch.zeros_like(s))


def _per_class_ap(cls, pred, lab, class_pos):
    """eval_util.EvaluationMetrics._per_class_ap as an fp64 [V] device tensor.  The per-class sums are segment sums over the class-major
    order (torch.segment_reduce) instead of index_add_, whose device form adds in no fixed order."""
    V = class_pos.numel()
    order = pred.argsort(descending=True, stable=True)
    order = order[cls[order].argsort(stable=True)]                  # class-major, prediction-descending inside a class
    c, pos = cls[order], (lab[order] > 0).to(torch.float64)
    counts = torch.bincount(c, minlength=V)
    start = counts.cumsum(0) - counts
    idx = torch.arange(c.numel(), device=c.device)
    rank = (idx - start[c] + 1).to(torch.float64)
    cum = pos.cumsum(0)
    before = torch.cat([cum.new_zeros(1), cum])[start[c]]
    contrib = pos * (cum - before) / rank
    ap = torch.segment_reduce(contrib, "sum", lengths=counts, unsafe=True)
    return torch.where(class_pos > 0, ap / class_pos.clamp_min(1.0), torch.zeros_like(ap))


def batch_metrics(predictions, labels, top_k: int = 20) -> torch.Tensor:
    """-> fp64 [3] on the predictions' device: Hit@1, PERR and GAP of ONE batch (eval_util.calculate_hit_at_one,
    calculate_precision_at_equal_recall_rate, calculate_gap(top_k)) -- what train.py:461-465 computes for its log line.  On the GPU:
    one lpm_eval_rows pass (ops.eval_rows, no loss) and the average precision of the pooled top-k entries, all on the device with no
    host sync (the caller copies the three numbers when it wants them).  CPU tensors go through eval_util."""
    p = torch.as_tensor(predictions)
    y = torch.as_tensor(labels).to(p.device)
    if not p.is_cuda:
        return torch.tensor([eval_util.calculate_hit_at_one(p, y), eval_util.calculate_precision_at_equal_recall_rate(p, y),
                             eval_util.calculate_gap(p, y, top_k)], dtype=torch.float64)
    if y.dtype not in (torch.bool, torch.uint8):
        y = y != 0
    f64 = torch.float64
    r = ops.eval_rows(p.to(torch.float32), y, min(int(top_k), p.shape[1]), with_loss=False)
    n = r.num_labels.to(f64)
    perr = torch.where(n > 0, r.hits_at_n.to(f64) / n.clamp_min(1.0), torch.zeros_like(n)).mean()
    gap = _average_precision(r.top_value.reshape(-1).to(f64), r.top_label.reshape(-1).to(f64), n.sum())
    return torch.stack([r.hit1.to(f64).mean(), perr, gap])


class DeviceEvaluationMetrics:
    """eval_util.EvaluationMetrics on the GPU: accumulate(predictions, labels, loss=None), get(), clear()."""

    def __init__(self, num_class: int, top_k: int, device):
        if not isinstance(num_class, int) or num_class <= 1:
            raise ValueError("num_class must be a positive integer.")
        if not isinstance(top_k, int) or top_k <= 0:
            raise ValueError("k must be a positive integer.")
        device = torch.device(device)
        if device.type != "cuda":
            raise LpmError(f"DeviceEvaluationMetrics needs a GPU device, got {device}; {_CPU_HINT}")
        self.k = min(top_k, num_class)
        if self.k > ops.TOPK_MAX_K or num_class > ops.TOPK_MAX_V:
            raise LpmError(f"DeviceEvaluationMetrics: need min(top_k, num_class) <= {ops.TOPK_MAX_K} and num_class <= {ops.TOPK_MAX_V} "
                           f"(top_k={top_k}, num_class={num_class})")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.num_class, self.top_k, self.device = num_class, top_k, device
        self.clear()

    def clear(self):
        self.num_examples = 0
        self._cap = 0
        self._rows = None               # hit1 uint8, num_labels int32, hits_at_n int32 [cap]; top index / value / label [cap, k]
        self._sum_loss = torch.zeros((), dtype=torch.float64, device=self.device)      # sum over batches of mean loss * batch
        self._class_pos = torch.zeros(self.num_class, dtype=torch.int64, device=self.device)

    def _reserve(self, B):
        """Room for B more rows: the buffers double (the sizes are known on the host, so no sync); lpm_eval_rows writes into them."""
        need = self.num_examples + B
        if need <= self._cap:
            return
        cap = max(need, 2 * self._cap, 256)
        d, k = self.device, self.k
        rows = (torch.empty(cap, dtype=torch.uint8, device=d), torch.empty(cap, dtype=torch.int32, device=d),
                torch.empty(cap, dtype=torch.int32, device=d), torch.empty((cap, k), dtype=torch.int32, device=d),
                torch.empty((cap, k), dtype=torch.float32, device=d), torch.empty((cap, k), dtype=torch.uint8, device=d))
        if self._rows is not None:
            for new, old in zip(rows, self._rows):
                new[:self.num_examples].copy_(old[:self.num_examples])
        self._rows, self._cap = rows, cap

    def _check(self, t, what):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise LpmError(f"DeviceEvaluationMetrics.accumulate: {what} must be a tensor on {self.device}; {_CPU_HINT}")
        if t.device != self.device:
            raise LpmError(f"DeviceEvaluationMetrics.accumulate: {what} is on {t.device}, the metrics on {self.device}")

    def accumulate(self, predictions, labels, loss=None) -> Dict[str, torch.Tensor]:
        """One batch: predictions fp32 [B, num_class] and 0 / 1 labels [B, num_class] (bool or uint8; other dtypes count nonzero as a
        positive) on the metrics' device.  loss None: the kernel's cross-entropy of the predictions, averaged over the batch; a given
        loss (a device tensor) is averaged as eval_util averages it.  -> the batch's hit_at_one, perr, loss as 0-d fp64 device tensors."""
        self._check(predictions, "predictions")
        self._check(labels, "labels")
        if loss is not None:
            self._check(loss, "loss")
        if predictions.dim() != 2 or predictions.shape != labels.shape:
            raise ValueError("predictions and actuals must be [batch, num_classes] and agree in shape")
        if predictions.shape[1] != self.num_class:
            raise ValueError("the shape of predictions and actuals does not match num_class")
        if labels.dtype not in (torch.bool, torch.uint8):
            labels = labels != 0
        B = predictions.shape[0]
        self._reserve(B)
        s = slice(self.num_examples, self.num_examples + B)
        hit1, nl, hn, ti, tv, tl = (buf[s] for buf in self._rows)
        loss_row = torch.empty(B, dtype=torch.float64, device=self.device) if loss is None else None
        r = ops.eval_rows(predictions, labels, self.k, out=ops.EvalRows(hit1, nl, hn, loss_row, ti, tv, tl))   # straight into the buffers
        if FLAGS.eval_stats_fused:
            return self._accumulate_fused(r, labels, loss, B)
        f64 = torch.float64
        hit = r.hit1.to(f64).mean()
        n = r.num_labels.to(f64)
        perr = torch.where(n > 0, r.hits_at_n.to(f64) / n.clamp_min(1.0), torch.zeros_like(n)).mean()
        mean_loss = r.loss_row.mean() if loss is None else loss.to(f64).mean()
        self._sum_loss += mean_loss * B
        self._class_pos += labels.sum(dim=0)
        self.num_examples += B
        return {"hit_at_one": hit, "perr": perr, "loss": mean_loss}

    _SLOTS = 256                        # batch slots per allocation
    _slots, _slot_at, last_batch = None, 0, None

    def _accumulate_fused(self, r, labels, loss, B) -> Dict[str, torch.Tensor]:
        """accumulate's second launch with FLAGS.eval_stats_fused: lpm_eval_batch_stats writes (hit_at_one, perr, loss, B) into a slot
        of its own -- ``last_batch``, fp64 [4]; the returned tensors are views of it -- and adds to the loss sum and the class counts."""
        if loss is not None and (loss.numel() != 1 or loss.dtype not in (torch.float32, torch.float64)):
            loss = loss.to(torch.float64).mean()
        if self._slots is None or self._slot_at == self._SLOTS:          # (a new allocation: the slots handed out stay what they are)
            self._slots, self._slot_at = torch.empty((self._SLOTS, 4), dtype=torch.float64, device=self.device), 0
        slot = self._slots[self._slot_at]
        self._slot_at += 1
        ops.eval_batch_stats(r, labels if labels.is_contiguous() else labels.contiguous(), slot, self._sum_loss, self._class_pos, loss)
        self.num_examples += B
        self.last_batch = slot
        return {"hit_at_one": slot[0], "perr": slot[1], "loss": slot[2]}

    def get(self) -> Dict[str, object]:
        """eval_util.EvaluationMetrics.get's keys (avg_hit_at_one, avg_perr, avg_loss, aps, gap) plus num_examples."""
        if self.num_examples <= 0:
            raise ValueError("total_sample must be positive.")
        N, f64 = self.num_examples, torch.float64
        hit1, n, hits, idx, val, lab = (t[:N] for t in self._rows)
        n = n.to(f64)
        perr = torch.where(n > 0, hits.to(f64) / n.clamp_min(1.0), torch.zeros_like(n))
        cls, pred, labs = idx.reshape(-1).long(), val.reshape(-1).to(f64), lab.reshape(-1).to(f64)
        class_pos = self._class_pos.to(f64)
        gap = _average_precision(pred, labs, class_pos.sum())
        aps = _per_class_ap(cls, pred, labs, class_pos)
        head = torch.stack([hit1.to(f64).sum() / N, perr.sum() / N, self._sum_loss / N, gap])
        out = torch.cat([head, aps]).cpu().tolist()
        return {"avg_hit_at_one": out[0], "avg_perr": out[1], "avg_loss": out[2], "aps": out[4:], "gap": out[3], "num_examples": N}


class _BatchReports:
    """evaluate(on_batch=...)'s deliveries.  A GPU batch's numbers go to pinned host memory by an asynchronous copy with an event of its
    own behind it (a timing event: the interval to the previous batch's event is the batch's time) and are delivered once that event
    has completed -- looked at without waiting after every batch (``drain(False)``), waited for once the loop is over (``drain(True)``).  A pending batch is 32 bytes, so the pinned
    area grows by whole blocks instead of wrapping, and nothing in the loop blocks.  A CPU batch is delivered at once."""
    _BLOCK = 1024

    def __init__(self, on_batch, summary_writer, global_step):
        self.on_batch, self.writer, self.step = on_batch, summary_writer, global_step
        self.pending: List[tuple] = []
        self.host, self.at = None, 0
        self.last_event = None

    def start(self, device):
        """Before the first predict on a GPU: the event the first batch's time is measured from."""
        self.last_event = torch.cuda.Event(enable_timing=True)
        self.last_event.record(torch.cuda.current_stream(device))

    def deliver(self, examples, hit_at_one, perr, loss, examples_per_second):
        info = {"hit_at_one": float(hit_at_one), "perr": float(perr), "loss": float(loss), "examples_per_second": float(examples_per_second)}
        self.on_batch(examples, info)
        if self.writer is not None and self.step is not None:                                             # utils.py:76-89
            self.writer.add_scalars({"GlobalStep/Eval_Hit@1": info["hit_at_one"], "GlobalStep/Eval_Perr": info["perr"],
                                     "GlobalStep/Eval_Loss": info["loss"], "GlobalStep/Eval_Example_Second": info["examples_per_second"]},
                                    int(self.step))

    def device_batch(self, examples, rows, numbers):
        """numbers: the batch's (hit_at_one, perr, loss[, ...]) as one fp64 device tensor."""
        if self.last_event is None:                          # (a model that did not say where it computes: timed from here on)
            self.start(numbers.device)
        if self.host is None or self.at == self._BLOCK:
            self.host, self.at = torch.empty((self._BLOCK, 4), dtype=torch.float64, pin_memory=True), 0
        host = self.host[self.at, :numbers.numel()]
        self.at += 1
        host.copy_(numbers, non_blocking=True)
        event = torch.cuda.Event(enable_timing=True)
        event.record(torch.cuda.current_stream(numbers.device))
        self.pending.append((examples, rows, host, self.last_event, event))
        self.last_event = event
        self.drain(False)

    def drain(self, wait: bool):
        while self.pending:
            examples, rows, host, before, event = self.pending[0]
            if wait:
                event.synchronize()
            elif not event.query():
                return
            self.pending.pop(0)
            ms = before.elapsed_time(event)
            hit, perr, loss = host[:3].tolist()
            self.deliver(examples, hit, perr, loss, rows / (ms * 1e-3) if ms > 0 else float("inf"))


def evaluate(model, batches, top_k: int = 20, metrics=None, summary_writer=None, global_step=None,
             label_loss_fn=None, on_batch: Optional[Callable] = None) -> Dict[str, object]:
    """eval.py's evaluation_loop for anything with ``.predict(frames, num_frames)`` and ``.vocab_size`` (a Predictor or a Trainer) over
    (ids, frames, labels, num_frames) batches (readers.YT8MFrameFeatureReader.batches; uint8 frames go into predict as they are).
    Predictions on a GPU go into DeviceEvaluationMetrics, CPU predictions into eval_util.EvaluationMetrics with cross_entropy_rows as
    the loss.  ``metrics`` (cleared first) replaces the default.  -> get()'s dict plus map (the mean of aps), num_examples and
    examples_per_second.  With ``summary_writer`` (summaries.SummaryWriter) AND ``global_step`` the epoch's Epoch/Eval_Avg_Hit@1,
    Epoch/Eval_Avg_Perr, Epoch/Eval_Avg_Loss, Epoch/Eval_MAP and Epoch/Eval_GAP are written at that step (utils.py:123-137).
    ``label_loss_fn`` (a losses.BaseLoss: eval.py:316's ``find_class_by_name(FLAGS.label_loss, [losses])()``): its calculate_loss of every
    batch's predictions and labels is what both kinds of metrics accumulate, so avg_loss and Epoch/Eval_Avg_Loss are that loss weighted
    by examples; None keeps the cross entropy described above.
    ``on_batch(examples_processed, info)`` is called once per batch, in batch order, with the batch's hit_at_one, perr, loss and
    examples_per_second as Python floats (eval.py:247-262); with ``summary_writer`` and ``global_step`` every delivered batch also writes
    GlobalStep/Eval_Hit@1, _Perr, _Loss and _Example_Second at ``global_step`` (utils.py:55-96: every batch at the same step).  On a
    GPU the numbers reach the host by asynchronous copies and the calls may lag the loop -- no batch waits for the host; all of them
    are made before this returns -- and examples_per_second comes from device events at the batch boundaries (the first interval
    starts before the first predict).  On the CPU the call follows the batch at once and the rate is the wall clock of reading the batch
    and computing its predictions and loss."""
    t0 = time.perf_counter()
    if metrics is not None:
        metrics.clear()
    reports = _BatchReports(on_batch, summary_writer, global_step) if on_batch is not None else None
    examples = 0
    t_batch = t0
    for _, frames, labels, num_frames in batches:
        if reports is not None and examples == 0:
            where = getattr(model, "device", None)
            where = torch.device(where) if where is not None else frames.device
            if where.type == "cuda":
                reports.start(where)
        with torch.no_grad():
            p = model.predict(frames, num_frames)
        if metrics is None:
            metrics = (DeviceEvaluationMetrics(int(model.vocab_size), top_k, p.device) if p.is_cuda
                       else eval_util.EvaluationMetrics(int(model.vocab_size), top_k))
        y = labels.to(p.device)
        if label_loss_fn is not None:
            with torch.no_grad():
                loss = label_loss_fn.calculate_loss(p, y)
            seconds = time.perf_counter() - t_batch
            r = metrics.accumulate(p, y, loss)
        elif isinstance(metrics, DeviceEvaluationMetrics):
            seconds = time.perf_counter() - t_batch
            r = metrics.accumulate(p, y)
        else:
            loss = cross_entropy_rows(p, y)
            seconds = time.perf_counter() - t_batch
            r = metrics.accumulate(p, y, loss)
        if reports is not None:
            rows = int(p.shape[0])
            examples += rows
            if torch.is_tensor(r["hit_at_one"]) and r["hit_at_one"].is_cuda:
                slot = getattr(metrics, "last_batch", None)
                if slot is None or slot.data_ptr() != r["hit_at_one"].data_ptr():          # (the unfused route: three 0-d tensors)
                    slot = torch.stack([r["hit_at_one"], r["perr"], r["loss"]])
                reports.device_batch(examples, rows, slot)
            else:
                reports.deliver(examples, r["hit_at_one"], r["perr"], r["loss"], rows / seconds if seconds > 0 else float("inf"))
            t_batch = time.perf_counter()
    if metrics is None:
        raise ValueError("evaluate: no batches")
    info = metrics.get()                                   # (copies the device results to the host: the loop's one sync)
    if reports is not None:
        reports.drain(True)
    seconds = time.perf_counter() - t0
    info["map"] = float(np.mean(info["aps"]))
    info["num_examples"] = metrics.num_examples
    info["examples_per_second"] = metrics.num_examples / seconds if seconds > 0 else float("inf")
    if summary_writer is not None and global_step is not None:
        summary_writer.add_scalars({"Epoch/Eval_Avg_Hit@1": info["avg_hit_at_one"], "Epoch/Eval_Avg_Perr": info["avg_perr"],
                                    "Epoch/Eval_Avg_Loss": info["avg_loss"], "Epoch/Eval_MAP": info["map"],
                                    "Epoch/Eval_GAP": info["gap"]}, int(global_step))
    return info


def format_batch_summary(global_step, info: Dict[str, object]) -> str:
    """utils.py:92-95 (AddGlobalStepSummary): a batch's info string, byte for byte; examples_per_second -1 when ``info`` has none."""
    return ("global_step {0} | Batch Hit@1: {1:.3f} | Batch PERR: {2:.3f} | Batch Loss: {3:.3f} "
            "| Examples_per_sec: {4:.3f}").format(global_step, info["hit_at_one"], info["perr"], info["loss"],
                                                  info.get("examples_per_second", -1))


def format_epoch_summary(info: Dict[str, object], epoch_id) -> str:
    """utils.py:139-142 (AddEpochSummary): the epoch's info line, byte for byte -- MAP is numpy.mean(aps), and the loss keeps the
    reference's "{5:3f}" (width 3, six decimals)."""
    mean_ap = np.mean(info["aps"])
    return ("epoch/eval number {0} | Avg_Hit@1: {1:.3f} | Avg_PERR: {2:.3f} "
            "| MAP: {3:.3f} | GAP: {4:.3f} | Avg_Loss: {5:3f}").format(epoch_id, info["avg_hit_at_one"], info["avg_perr"], mean_ap,
                                                                       info["gap"], info["avg_loss"])


# ---- command line (python -m learnablepoolingmethods_amd.evaluation) -------------------------------------------------------------
class EvalState:
    """What the turns of ``run`` share: where the checkpoints are, what evaluates them, and the step of the last turn."""

    def __init__(self, train_dir, model, num_classes, reader, files, batch_size=1024, num_readers=1, device="cuda", top_k=20,
                 label_loss_fn=None, summary_writer=None, checkpoint=None, log: Callable[[str], None] = logging.info):
        self.train_dir, self.model, self.num_classes = train_dir, model, int(num_classes)
        self.reader, self.files, self.batch_size, self.num_readers = reader, list(files), int(batch_size), int(num_readers)
        self.device, self.top_k, self.label_loss_fn = torch.device(device), int(top_k), label_loss_fn
        self.summary_writer, self.checkpoint, self.log = summary_writer, checkpoint, log
        self.last_step = -1                 # eval.py:342's last_global_step_val
        self.last_info: Optional[Dict[str, object]] = None


def _checkpoint_step(path: str) -> int:
    """eval.py:216: the step is the number behind the file name's last "-" (model.ckpt-<step>.pt); 0 for a name without one."""
    digits = os.path.basename(path).split("-")[-1].split(".")[0]
    return int(digits) if digits.isdigit() else 0


def evaluate_latest(state: EvalState) -> int:
    """One turn of eval.py:186-289 -> the evaluated checkpoint's step.  No checkpoint: logs "No checkpoint file found." and returns -1.
    The step of the last turn again: logs the reference's skip line and returns the step.  Otherwise the checkpoint becomes a
    Predictor and ``evaluate`` runs over the files (device_batches on a GPU, batches() on the CPU) with every batch's line
    ("examples_processed: N | " + format_batch_summary) and the epoch's line (format_epoch_summary) logged and their scalars written;
    ``state.last_step`` and ``state.last_info`` (the epoch's dict plus global_step) then hold the result.  A checkpoint that cannot be
    loaded is logged and left for the next turn: ``state.last_step`` stays and is what this returns."""
    from . import training
    from .predictor import Predictor
    checkpoint = state.checkpoint or training.latest_checkpoint(state.train_dir)
    if not checkpoint:
        state.log("No checkpoint file found.")
        return -1
    step = _checkpoint_step(checkpoint)
    if step == state.last_step:
        state.log("skip this checkpoint global_step_val=%s (same as the previous one)." % step)
        return step
    state.log("Loading checkpoint for eval: " + checkpoint)
    try:
        predictor = Predictor.from_checkpoint(checkpoint, state.model, vocab_size=state.num_classes, device=state.device)
    except Exception as e:  # pylint: disable=broad-except  (whatever a half-written or foreign file raises in torch.load)
        state.log("Cannot load %s (%s: %s); trying again at the next turn." % (checkpoint, type(e).__name__, e))
        return state.last_step
    state.log("enter eval_once loop global_step_val = %s. " % step)
    if state.device.type == "cuda":
        batches = state.reader.device_batches(state.files, state.batch_size, device=state.device, reader_threads=state.num_readers)
    else:
        batches = state.reader.batches(state.files, state.batch_size)
    try:
        info = evaluate(predictor, batches, top_k=state.top_k, summary_writer=state.summary_writer, global_step=step,
                        label_loss_fn=state.label_loss_fn,
                        on_batch=lambda n, batch: state.log("examples_processed: %d | %s" % (n, format_batch_summary(step, batch))))
    finally:
        if hasattr(batches, "close"):
            batches.close()
    state.log(format_epoch_summary(info, step))
    if state.summary_writer is not None:
        state.summary_writer.flush()
    info["global_step"] = step
    state.last_step, state.last_info = step, info
    return step


def run(state: EvalState, run_once: bool = False, poll_seconds: float = 10.0, sleep: Callable[[float], None] = time.sleep) -> Dict[str, object]:
    """eval.py:342-349: ``evaluate_latest`` again and again until ``run_once`` (a ``state.checkpoint`` is evaluated once too), sleeping
    ``poll_seconds`` between the turns (the reference opens its next session at once).  -> the last epoch's dict plus global_step; None
    when no turn evaluated anything."""
    while True:
        evaluate_latest(state)
        if run_once or state.checkpoint:
            return state.last_info
        sleep(poll_seconds)


def _parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m learnablepoolingmethods_amd.evaluation",
                                 description="Evaluate the checkpoints of a training run over YT8M TFRecord files as they appear (the "
                                             "reference's eval.py flags).")
    ap.add_argument("--train_dir", default="/tmp/yt8m_model/", help="the directory of model_flags.json and the checkpoints (eval.py:38)")
    ap.add_argument("--eval_data_pattern", default="", help="comma-separated globs of TFRecord files (eval.py:41)")
    ap.add_argument("--batch_size", type=int, default=1024, help="eval.py:47")
    ap.add_argument("--num_readers", type=int, default=1, help="eval.py:49: device_batches' reader_threads (GPU route)")
    ap.add_argument("--run_once", action="store_true", help="eval.py:51: evaluate the newest checkpoint and return")
    ap.add_argument("--top_k", type=int, default=20, help="eval.py:53")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--checkpoint", default="", help="one model.ckpt-<step>.pt file, evaluated once (default: the newest one of --train_dir)")
    ap.add_argument("--poll_seconds", type=float, default=10.0, help="the sleep between two looks at --train_dir")
    ap.add_argument("--summary_dir", default=None, help="where the event file goes (default: --train_dir, as eval.py; empty: no summaries)")
    return ap


def main(argv=None) -> Dict[str, object]:
    """eval.py's ``evaluate``: model_flags.json + the newest checkpoint + files -> ``run``'s dict."""
    from . import losses, model_flags, registry, summaries
    args = _parser().parse_args(argv)
    flags_dict = model_flags.read(args.train_dir, "Cannot find file %s. Did you run train.py on the same --train_dir?")  # eval.py:296-299
    if not args.eval_data_pattern:
        raise IOError("'eval_data_pattern' was not specified. Nothing to evaluate.")                    # eval.py:318-320
    files = model_flags.matching_files(args.eval_data_pattern)
    if not files:
        raise IOError("Unable to find the evaluation files.")                                           # eval.py:96-97
    logging.info("number of evaluation files: " + str(len(files)))
    summary_dir = args.train_dir if args.summary_dir is None else args.summary_dir
    with model_flags.applied(flags_dict):
        writer = summaries.SummaryWriter(summary_dir) if summary_dir else None
        try:
            state = EvalState(args.train_dir, registry.get_model(flags_dict["model"]), flags_dict["num_classes"],
                              model_flags.build_reader(flags_dict), files, batch_size=args.batch_size, num_readers=args.num_readers,
                              device=args.device, top_k=args.top_k, label_loss_fn=losses.by_name(flags_dict["label_loss"]),
                              summary_writer=writer, checkpoint=args.checkpoint or None)
            return run(state, run_once=args.run_once, poll_seconds=args.poll_seconds)
        finally:
            if writer is not None:
                writer.close()


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    main()
