"""TensorBoard event files written by hand (reference: the ``tf.summary.scalar`` / ``tf.summary.histogram`` calls of train.py:250-326,
470-480, utils.py:55-143 and frame_level_models.py, and the Supervisor's summary writer).

    SummaryWriter(logdir) -> events.out.tfevents.<seconds>.<hostname>: TFRecord-framed ``Event`` messages, the first one
    Event{wall_time, file_version = "brain.Event:2"}, every other one Event{wall_time, step, summary{value{tag, simple_value | histo}}}.

The format is small and fixed, so it is encoded here as ``readers`` encodes ``SequenceExample``: TensorFlow and TensorBoard are not needed.
  Event          wall_time = 1 (double), step = 2 (varint), file_version = 3 (string), summary = 5 (message)
  Summary        value = 1 (repeated message)
  Summary.Value  tag = 1 (string), simple_value = 2 (float), histo = 5 (message)
  HistogramProto min, max, num, sum, sum_squares = 1..5 (double), bucket_limit = 6, bucket = 7 (packed doubles)
Scalar fields at their default (0) are left out, as proto3 serialisers do; the members of Value's oneof are always written.

Histograms follow tensorflow::histogram::Histogram: the 1551 bucket limits of ``default_bucket_limits`` (built by TensorFlow's own loop,
in which rounding accumulates: a limit is never recomputed), a value's bucket is the first limit strictly greater than it, and
``encode_histogram`` collapses runs of empty buckets as EncodeToProto(preserve_zero_buckets = false) does.  On the GPU the counting is one
HIP pass (ops.histogram_segments / lpm_histogram_segments; ops.histogram_frames_q8 for quantised frames); CPU tensors and arrays take a
numpy ``searchsorted`` path.  What a GPU histogram call produces stays on the device until the writer commits it: ONE non-blocking copy
into pinned memory behind an event for everything added at one step; the records are encoded and written, in the order of the calls, once
the event has completed -- polled at every later call, waited for at ``flush`` / ``close``.  A call that adds nothing reads nothing back.

Non-finite values (TensorFlow's histogram op fails on them): the histogram is written from the finite ones and one warning per tag names
their number; ``strict=True`` raises instead.
"""
from __future__ import annotations

import logging
import math
import os
import socket
import struct
import time
from typing import Callable, Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import readers, utils
from .readers import _enc_ld, _enc_varint, _fields, masked_crc32c

FILE_VERSION = "brain.Event:2"
DBL_MAX = 1.7976931348623157e308
_LIMITS: Optional[List[float]] = None
_LOG = logging.getLogger(__name__)


def default_bucket_limits() -> List[float]:
    """tensorflow/core/lib/histogram/histogram.cc InitDefaultBucketsInner: 1e-12 * 1.1^k below 1e20 by repeated multiplication, DBL_MAX,
    their negatives and 0 -- 1551 ascending limits."""
    global _LIMITS
    if _LIMITS is None:
        pos, v = [], 1e-12
        while v < 1e20:
            pos.append(v)
            v *= 1.1
        pos.append(DBL_MAX)
        _LIMITS = [-p for p in reversed(pos)] + [0.0] + pos
    return list(_LIMITS)


# ---- encoding --------------------------------------------------------------------------------------------------------------------
def _enc_double(num: int, v: float) -> bytes:
    v = float(v)
    if v == 0.0 and math.copysign(1.0, v) > 0:
        return b""
    return _enc_varint((num << 3) | 1) + struct.pack("<d", v)


def encode_histogram(stats: Sequence[float], counts: Sequence[float], limits: Optional[Sequence[float]] = None) -> bytes:
    """HistogramProto bytes of (min, max, num, sum, sum_squares) and per-bucket counts (one per limit): a run of empty buckets becomes ONE
    (limit of the run's last bucket, 0) pair, non-empty buckets go out as they are, and a histogram with nothing to emit gets (DBL_MAX, 0)."""
    limits = default_bucket_limits() if limits is None else limits
    counts = np.asarray(counts, dtype=np.float64).reshape(-1)
    lim = np.asarray(limits, dtype=np.float64).reshape(-1)
    if counts.shape != lim.shape:
        raise ValueError(f"encode_histogram: {counts.size} counts for {lim.size} bucket limits")
    nz = counts != 0
    # bucket i is emitted when it is non-empty, or when it ends a run of empty ones: the next bucket is non-empty, or it is the last
    keep = nz | np.append(nz[1:], True)
    if not keep.any():
        out_l, out_c = np.array([DBL_MAX]), np.array([0.0])
    else:
        out_l, out_c = lim[keep], counts[keep]
    body = b"".join(_enc_double(i + 1, s) for i, s in enumerate(stats))
    return body + _enc_ld(6, out_l.astype("<f8").tobytes()) + _enc_ld(7, out_c.astype("<f8").tobytes())


def encode_value(tag: str, simple_value: Optional[float] = None, histo: Optional[bytes] = None) -> bytes:
    """Summary.Value bytes."""
    body = _enc_ld(1, tag.encode("utf-8"))
    if histo is not None:
        return body + _enc_ld(5, histo)
    return body + b"\x15" + struct.pack("<f", float(simple_value))


def encode_event(wall_time: float, step: int = 0, file_version: Optional[str] = None, values: Optional[Sequence[bytes]] = None) -> bytes:
    """Event bytes; ``values``: encoded Summary.Value messages."""
    out = _enc_double(1, wall_time)
    if step:
        out += b"\x10" + _enc_varint(int(step))
    if file_version is not None:
        out += _enc_ld(3, file_version.encode("utf-8"))
    if values is not None:
        out += _enc_ld(5, b"".join(_enc_ld(1, v) for v in values))
    return out


def frame_record(data: bytes) -> bytes:
    """TFRecord framing of one payload."""
    head = struct.pack("<Q", len(data))
    return head + struct.pack("<I", masked_crc32c(head)) + data + struct.pack("<I", masked_crc32c(data))


# ---- histograms on the host ------------------------------------------------------------------------------------------------------
def histogram_numpy(values, limits: Optional[Sequence[float]] = None) -> Tuple[List[float], np.ndarray, int]:
    """-> (stats, counts, nonfinite) of an array, ops.histogram_segments' semantics in numpy (fp64)."""
    lim = np.asarray(default_bucket_limits() if limits is None else limits, dtype=np.float64)
    v = np.asarray(values).astype(np.float64).reshape(-1)
    finite = np.isfinite(v)
    bad = int(v.size - finite.sum())
    v = v[finite]
    counts = np.bincount(np.minimum(np.searchsorted(lim, v, side="right"), lim.size - 1), minlength=lim.size).astype(np.int64)
    if v.size == 0:
        return [DBL_MAX, -DBL_MAX, 0.0, 0.0, 0.0], counts, bad
    return [float(v.min()), float(v.max()), float(v.size), float(v.sum()), float((v * v).sum())], counts, bad


def histogram_of_counted_values(values, counts, limits: Optional[Sequence[float]] = None) -> Tuple[List[float], np.ndarray]:
    """-> (stats, bucket counts) of a multiset given as values and how often each occurs (the quantised input: 256 byte values + padding)."""
    lim = np.asarray(default_bucket_limits() if limits is None else limits, dtype=np.float64)
    v, c = np.asarray(values, dtype=np.float64).reshape(-1), np.asarray(counts, dtype=np.int64).reshape(-1)
    out = np.zeros(lim.size, dtype=np.int64)
    np.add.at(out, np.minimum(np.searchsorted(lim, v, side="right"), lim.size - 1), c)
    seen = c > 0
    if not seen.any():
        return [DBL_MAX, -DBL_MAX, 0.0, 0.0, 0.0], out
    cf = c.astype(np.float64)
    return [float(v[seen].min()), float(v[seen].max()), float(c.sum()), float((cf * v).sum()), float((cf * v * v).sum())], out


def dequantised_byte_values() -> np.ndarray:
    """utils.Dequantize of the 256 byte values in fp32 (ops.QUANT_MAX / QUANT_MIN), as the reference's reader computes them."""
    from . import ops
    return utils.Dequantize(torch.arange(256, dtype=torch.float32), ops.QUANT_MAX, ops.QUANT_MIN).numpy()


# ---- the writer ------------------------------------------------------------------------------------------------------------------
class _Staged:
    """What one GPU histogram call left on the device: a flat int64 tensor and how to turn its host copy into Summary.Value messages."""

    def __init__(self, wall_time, step, data, decode):
        self.wall_time, self.step, self.data, self.decode, self.size = wall_time, int(step), data, decode, data.numel()


class _Pending:
    """A committed copy: pinned host memory, the event behind the copy, and the staged calls whose data it holds (in call order)."""

    def __init__(self, host, event, items):
        self.host, self.event, self.items = host, event, items


class SummaryWriter:
    def __init__(self, logdir: str, filename_suffix: str = "", clock: Callable[[], float] = time.time, strict: bool = False,
                 limits: Optional[Sequence[float]] = None):
        os.makedirs(logdir, exist_ok=True)
        self.clock, self.strict = clock, bool(strict)
        self.limits = default_bucket_limits() if limits is None else [float(x) for x in limits]
        self._custom_limits = limits is not None
        now = clock()
        self.path = os.path.join(logdir, "events.out.tfevents.%010d.%s%s" % (int(now), socket.gethostname(), filename_suffix))
        self._file = open(self.path, "wb")
        self._queue: List[object] = []          # bytes (an encoded event) or a _Pending, in the order of the calls
        self._staged: List[_Staged] = []
        self._warned = set()
        self._file.write(frame_record(encode_event(now, file_version=FILE_VERSION)))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    # -- records -------------------------------------------------------------------------------------------------------------------
    def _check_open(self):
        if self._file is None:
            raise ValueError("SummaryWriter is closed")

    def _emit(self, wall_time, step, values: Sequence[bytes]):
        self._queue.append(frame_record(encode_event(wall_time, int(step), values=values)))

    def _drain(self, wait: bool):
        """Write the queue's head while it is ready (a pending copy: once its event has completed, or after waiting for it)."""
        while self._queue:
            head = self._queue[0]
            if isinstance(head, _Pending):
                if wait:
                    head.event.synchronize()
                elif not head.event.query():
                    return
                flat = head.host.numpy()
                at = 0
                for item in head.items:
                    values = item.decode(flat[at:at + item.size])
                    at += item.size
                    if values:
                        self._file.write(frame_record(encode_event(item.wall_time, item.step, values=values)))
            else:
                self._file.write(head)
            self._queue.pop(0)

    def _stage(self, step, data: torch.Tensor, decode):
        if self._staged and self._staged[0].step != int(step):
            self.commit()
        self._staged.append(_Staged(self.clock(), step, data, decode))

    def commit(self):
        """Start the host copy of what the GPU histogram calls since the last commit produced: one non-blocking copy into pinned memory
        and an event behind it.  Called by itself when a call for another step, a host-side add, ``flush`` or ``close`` follows."""
        if not self._staged:
            return
        items, self._staged = self._staged, []
        flat = items[0].data if len(items) == 1 else torch.cat([it.data for it in items])
        host = torch.empty(flat.numel(), dtype=torch.int64, pin_memory=True)
        host.copy_(flat, non_blocking=True)
        event = torch.cuda.Event()
        event.record(torch.cuda.current_stream(flat.device))
        for it in items:
            it.data = None
        self._queue.append(_Pending(host, event, items))

    def _nonfinite(self, tag: str, bad: int):
        if bad <= 0:
            return
        if self.strict:
            raise ValueError(f"summary {tag!r}: {bad} non-finite values")
        if tag not in self._warned:
            self._warned.add(tag)
            _LOG.warning("summary %r: %d non-finite values left out of the histogram", tag, bad)

    # -- the public adds -----------------------------------------------------------------------------------------------------------
    def add_scalar(self, tag: str, value, step: int):
        self._check_open()
        self.commit()
        self._emit(self.clock(), step, [encode_value(tag, simple_value=float(value))])
        self._drain(False)

    def add_scalars(self, scalars: Dict[str, float], step: int):
        """Several scalars of one step in one event."""
        self._check_open()
        self.commit()
        self._emit(self.clock(), step, [encode_value(t, simple_value=float(v)) for t, v in scalars.items()])
        self._drain(False)

    def add_histogram_raw(self, tag: str, stats: Sequence[float], counts: Sequence[float], step: int):
        """A histogram given as (min, max, num, sum, sum_squares) and one count per bucket limit of this writer."""
        self._check_open()
        self.commit()
        self._emit(self.clock(), step, [encode_value(tag, histo=encode_histogram(stats, counts, self.limits))])
        self._drain(False)

    def _device_limits(self):
        return self.limits if self._custom_limits else None

    def _decode_segments(self, tags: Sequence[str]):
        """The decoder of a packed ops.Histogram of len(tags) segments: counts [n, L] | stats [n, 5] (fp64 bits) | nonfinite [n]."""
        n, L = len(tags), len(self.limits)

        def decode(flat: np.ndarray) -> List[bytes]:
            counts = flat[:n * L].reshape(n, L)
            stats = flat[n * L:n * L + 5 * n].view(np.float64).reshape(n, 5)
            bad = flat[n * L + 5 * n:]
            out = []
            for i, tag in enumerate(tags):
                self._nonfinite(tag, int(bad[i]))
                out.append(encode_value(tag, histo=encode_histogram(stats[i].tolist(), counts[i], self.limits)))
            return out
        return decode

    @staticmethod
    def _pack(h) -> torch.Tensor:
        return torch.cat([h.counts.reshape(-1), h.stats.reshape(-1).view(torch.int64), h.nonfinite.reshape(-1)])

    def add_histogram(self, tag: str, values, step: int):
        """The histogram of every element of ``values``: a GPU tensor is counted on the device (ops.histogram_segments; other dtypes are
        converted to fp32 first), a CPU tensor or an array in numpy."""
        self._check_open()
        if isinstance(values, torch.Tensor) and values.is_cuda:
            from . import ops
            if values.numel() == 0:
                return self.add_histogram_raw(tag, [DBL_MAX, -DBL_MAX, 0.0, 0.0, 0.0], np.zeros(len(self.limits)), step)
            h = ops.histogram_segments(values.detach().to(torch.float32), limits=self._device_limits())
            self._stage(step, self._pack(h), self._decode_segments([tag]))
            self._drain(False)
            return
        if isinstance(values, torch.Tensor):
            values = values.detach().to(torch.float64 if values.dtype == torch.float64 else torch.float32).numpy()
        stats, counts, bad = histogram_numpy(values, self.limits)
        self._nonfinite(tag, bad)
        self.add_histogram_raw(tag, stats, counts, step)

    def add_variables(self, trainer, step: int):
        """One histogram per variable of the trainer's store, tagged with the variable's name (the reference: every
        ``slim.get_model_variables()``, train.py:285-286; here ALL variables, the non-trainable moving statistics included).  On the GPU:
        one lpm_histogram_segments launch over the parameter arena -- the fp32 master, after pending asynchronous writes into it have been
        waited for, with the arena's own offsets and every variable's numel(), so the arena's padding is not counted -- and one over the
        non-trainable variables laid end to end."""
        self._check_open()
        store, arena = getattr(trainer, "store", None), getattr(trainer, "arena", None)
        if store is None or not hasattr(arena, "param"):
            # a trainer without a variable store: the tensors of its state_dict()
            for name, t in trainer.state_dict().items():
                if isinstance(t, torch.Tensor) and t.dtype.is_floating_point:
                    self.add_histogram(name, t, step)
            return
        if hasattr(trainer, "wait_pending"):
            trainer.wait_pending()
        else:
            store.drain_pending()
        names = list(arena.names)
        lens = [arena.views[n].numel() for n in names]
        rest = [n for n in store.vars if n not in arena.views]
        if not arena.param.is_cuda:
            for n, a0, k in zip(names, arena.offsets_host, lens):
                self.add_histogram(n, arena.param[a0:a0 + k].detach(), step)
            for n in rest:
                self.add_histogram(n, store.vars[n].detach(), step)
            return
        from . import ops
        parts = [self._pack(ops.histogram_segments(arena.param, arena.offsets_host[:len(names)], lens, limits=self._device_limits()))]
        decoders = [self._decode_segments(names)]
        rest = [n for n in rest if store.vars[n].numel() > 0]
        if rest:
            flat = torch.cat([store.vars[n].detach().reshape(-1).to(torch.float32) for n in rest])
            rlens = [store.vars[n].numel() for n in rest]
            starts = np.concatenate([[0], np.cumsum(rlens)[:-1]]).tolist()
            parts.append(self._pack(ops.histogram_segments(flat, starts, rlens, limits=self._device_limits())))
            decoders.append(self._decode_segments(rest))
        sizes = [p.numel() for p in parts]

        def decode(flat: np.ndarray) -> List[bytes]:
            out, at = [], 0
            for size, d in zip(sizes, decoders):
                out.extend(d(flat[at:at + size]))
                at += size
            return out
        self._stage(step, parts[0] if len(parts) == 1 else torch.cat(parts), decode)
        self._drain(False)

    def add_input(self, frames, num_frames, step: int, tag: str = "model/input_raw"):
        """The reference's histogram of the raw input batch (train.py:260).  Quantised frames (uint8 [B, max_frames, F]) are counted by byte
        value over the frames below num_frames (ops.histogram_frames_q8 on the GPU) and the 256 dequantised values, with the padded
        elements at 0.0, are put into buckets on the host: exactly the histogram of the dequantised, zero-padded fp32 batch the reference
        sees, without ever forming it.  Other dtypes: the histogram of the tensor as it is."""
        self._check_open()
        if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8:
            return self.add_histogram(tag, frames, step)
        values = np.append(dequantised_byte_values().astype(np.float64), 0.0)

        def decode(flat: np.ndarray) -> List[bytes]:
            stats, counts = histogram_of_counted_values(values, flat, self.limits)
            return [encode_value(tag, histo=encode_histogram(stats, counts, self.limits))]
        if frames.is_cuda:
            from . import ops
            self._stage(step, ops.histogram_frames_q8(frames, num_frames.to(frames.device)), decode)
            self._drain(False)
            return
        q = frames.numpy()
        live = np.arange(q.shape[1])[None, :] < np.asarray(num_frames).reshape(-1, 1)
        counts = np.append(np.bincount(q[live].reshape(-1), minlength=256), (~live).sum() * q.shape[2])
        self.commit()
        self._emit(self.clock(), step, decode(counts))
        self._drain(False)

    def flush(self):
        """Everything added so far is in the file when this returns (waits for the pending device copies)."""
        self._check_open()
        self.commit()
        self._drain(True)
        self._file.flush()

    def close(self):
        if self._file is None:
            return
        try:
            self.flush()
        finally:
            self._file.close()
            self._file = None


# ---- reading back (tests, tools) ---------------------------------------------------------------------------------------------------
def _decode_histogram(buf) -> Dict[str, object]:
    h: Dict[str, object] = {"min": 0.0, "max": 0.0, "num": 0.0, "sum": 0.0, "sum_squares": 0.0, "bucket_limit": [], "bucket": []}
    keys = {1: "min", 2: "max", 3: "num", 4: "sum", 5: "sum_squares"}
    for num, wt, v in _fields(bytes(buf)):
        if num in keys and wt == 1:
            h[keys[num]] = struct.unpack("<d", bytes(v))[0]
        elif num in (6, 7):
            vals = np.frombuffer(bytes(v), dtype="<f8").tolist()
            h["bucket_limit" if num == 6 else "bucket"].extend(vals)
    return h


def decode_event(data: bytes) -> Dict[str, object]:
    """-> {wall_time, step, file_version, values}: values a list of (tag, float | histogram dict)."""
    ev: Dict[str, object] = {"wall_time": 0.0, "step": 0, "file_version": None, "values": []}
    for num, wt, v in _fields(data):
        if num == 1 and wt == 1:
            ev["wall_time"] = struct.unpack("<d", bytes(v))[0]
        elif num == 2 and wt == 0:
            ev["step"] = v - (1 << 64) if v >= (1 << 63) else v
        elif num == 3 and wt == 2:
            ev["file_version"] = bytes(v).decode("utf-8")
        elif num == 5 and wt == 2:
            for n2, _, value in _fields(bytes(v)):
                if n2 != 1:
                    continue
                tag, payload = "", None
                for n3, wt3, x in _fields(bytes(value)):
                    if n3 == 1:
                        tag = bytes(x).decode("utf-8")
                    elif n3 == 2 and wt3 == 5:
                        payload = struct.unpack("<f", bytes(x))[0]
                    elif n3 == 5 and wt3 == 2:
                        payload = _decode_histogram(x)
                ev["values"].append((tag, payload))
    return ev


def read_events(path: str) -> Iterator[Dict[str, object]]:
    """The decoded events of an event file, both CRCs of every record verified (IOError on a mismatch)."""
    for data in readers.read_tfrecord(path, verify_crc=True):
        yield decode_event(data)


def expand_histogram(h: Dict[str, object], limits: Optional[Sequence[float]] = None) -> np.ndarray:
    """A decoded histogram's counts per bucket of ``limits`` (the inverse of encode_histogram's run collapsing)."""
    lim = np.asarray(default_bucket_limits() if limits is None else limits, dtype=np.float64)
    out = np.zeros(lim.size, dtype=np.float64)
    at = np.searchsorted(lim, np.asarray(h["bucket_limit"], dtype=np.float64), side="left")
    out[at] = np.asarray(h["bucket"], dtype=np.float64)
    return out
