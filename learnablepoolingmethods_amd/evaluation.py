"""Evaluation loop (reference: eval.py, minus the TensorFlow plumbing: checkpoint watching, queue runners, summaries).

  eval.py:152-155            the loss of a model without a "loss" output: losses.py:41-51 CrossEntropyLoss on the predictions
                             -> lpm_eval_rows' loss_row (device) / ``cross_entropy_rows`` (host)
  eval.py:186-289            evaluation_loop: predictions of every labelled batch into EvaluationMetrics, then get()   -> ``evaluate``
  eval_util.py:138-221       EvaluationMetrics: accumulate / get / clear                                   -> ``DeviceEvaluationMetrics``
  eval_util.py:26-68         Hit@1, PERR: per-row terms from one HIP pass (ops.eval_rows / lpm_eval_rows), fp64 means on the device
  eval_util.py:71-135,
  (mean_)average_precision_calculator.py
                             GAP and per-class AP over the pooled top-k (class, value, label) triplets, once per epoch
  utils.py:99-142            AddEpochSummary's info line                                                   -> ``format_epoch_summary``

``DeviceEvaluationMetrics.accumulate`` launches lpm_eval_rows and appends its outputs to device buffers; it makes no host sync and
returns the batch's hit_at_one, perr and loss as 0-d device tensors.  ``get`` reduces everything in fp64 on the device with
eval_util's definitions (PERR per row as hits_at_n / n; AP: pooled order, stable descending sort, the positives of a class as the
recall denominator) and copies the results to the host once.

The loss is the reference's CrossEntropyLoss of the predictions (eval.py takes it because MoeModel returns no "loss"), not the fused
head's cancellation-free loss that Trainer.step reports.

Tie rule: the device path ranks ties as a stable descending sort -- equal predictions by ascending class index inside a row (the arg-max
of Hit@1 is the lowest such index), pooled entries in pooled order.  eval_util's torch.topk leaves the order among ties unspecified and
the reference shuffles them (random.seed(0)), so the paths agree exactly whenever the ranked predictions are distinct.
"""
from __future__ import annotations

import time
from typing import Dict, Optional

import numpy as np
import torch

from . import eval_util, ops
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
        f64 = torch.float64
        hit = r.hit1.to(f64).mean()
        n = r.num_labels.to(f64)
        perr = torch.where(n > 0, r.hits_at_n.to(f64) / n.clamp_min(1.0), torch.zeros_like(n)).mean()
        mean_loss = r.loss_row.mean() if loss is None else loss.to(f64).mean()
        self._sum_loss += mean_loss * B
        self._class_pos += labels.sum(dim=0)
        self.num_examples += B
        return {"hit_at_one": hit, "perr": perr, "loss": mean_loss}

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


def evaluate(model, batches, top_k: int = 20, metrics=None, summary_writer=None, global_step=None,
             label_loss_fn=None) -> Dict[str, object]:
    """eval.py's evaluation_loop for anything with ``.predict(frames, num_frames)`` and ``.vocab_size`` (a Predictor or a Trainer) over
    (ids, frames, labels, num_frames) batches (readers.YT8MFrameFeatureReader.batches; uint8 frames go into predict as they are).
    Predictions on a GPU go into DeviceEvaluationMetrics, CPU predictions into eval_util.EvaluationMetrics with cross_entropy_rows as
    the loss.  ``metrics`` (cleared first) replaces the default.  -> get()'s dict plus map (the mean of aps), num_examples and
    examples_per_second.  With ``summary_writer`` (summaries.SummaryWriter) AND ``global_step`` the epoch's Epoch/Eval_Avg_Hit@1,
    Epoch/Eval_Avg_Perr, Epoch/Eval_Avg_Loss, Epoch/Eval_MAP and Epoch/Eval_GAP are written at that step (utils.py:123-137).
    ``label_loss_fn`` (a losses.BaseLoss: eval.py:316's ``find_class_by_name(FLAGS.label_loss, [losses])()``): its calculate_loss of every
    batch's predictions and labels is what both kinds of metrics accumulate, so avg_loss and Epoch/Eval_Avg_Loss are that loss weighted
    by examples; None keeps the cross entropy described above."""
    t0 = time.perf_counter()
    if metrics is not None:
        metrics.clear()
    for _, frames, labels, num_frames in batches:
        with torch.no_grad():
            p = model.predict(frames, num_frames)
        if metrics is None:
            metrics = (DeviceEvaluationMetrics(int(model.vocab_size), top_k, p.device) if p.is_cuda
                       else eval_util.EvaluationMetrics(int(model.vocab_size), top_k))
        y = labels.to(p.device)
        if label_loss_fn is not None:
            with torch.no_grad():
                metrics.accumulate(p, y, label_loss_fn.calculate_loss(p, y))
        elif isinstance(metrics, DeviceEvaluationMetrics):
            metrics.accumulate(p, y)
        else:
            metrics.accumulate(p, y, cross_entropy_rows(p, y))
    if metrics is None:
        raise ValueError("evaluate: no batches")
    info = metrics.get()                                   # (copies the device results to the host: the loop's one sync)
    seconds = time.perf_counter() - t0
    info["map"] = float(np.mean(info["aps"]))
    info["num_examples"] = metrics.num_examples
    info["examples_per_second"] = metrics.num_examples / seconds if seconds > 0 else float("inf")
    if summary_writer is not None and global_step is not None:
        summary_writer.add_scalars({"Epoch/Eval_Avg_Hit@1": info["avg_hit_at_one"], "Epoch/Eval_Avg_Perr": info["avg_perr"],
                                    "Epoch/Eval_Avg_Loss": info["avg_loss"], "Epoch/Eval_MAP": info["map"],
                                    "Epoch/Eval_GAP": info["gap"]}, int(global_step))
    return info


def format_epoch_summary(info: Dict[str, object], epoch_id) -> str:
    """utils.py:139-142 (AddEpochSummary): the epoch's info line, byte for byte -- MAP is numpy.mean(aps), and the loss keeps the
    reference's "{5:3f}" (width 3, six decimals)."""
    mean_ap = np.mean(info["aps"])
    return ("epoch/eval number {0} | Avg_Hit@1: {1:.3f} | Avg_PERR: {2:.3f} "
            "| MAP: {3:.3f} | GAP: {4:.3f} | Avg_Loss: {5:3f}").format(epoch_id, info["avg_hit_at_one"], info["avg_perr"], mean_ap,
                                                                       info["gap"], info["avg_loss"])
