"""YT8M frame-level reader (reference: readers.py:134-271, utils.py:28-43): TFRecord files of tf.train.SequenceExample
protos -> quantised frame matrices, frame counts, dense labels.  TensorFlow is not needed: the TFRecord framing
(length, masked CRC-32C, payload, masked CRC-32C) and the four protobuf messages involved are decoded by hand from the
public wire formats.

Unlike the reference, the reader hands the frames on QUANTISED (uint8, 1 byte per feature): dequantisation
(``utils.Dequantize``), the zero padding past ``num_frames`` and the input L2 normalisation of the training step are one
HIP kernel on the device (``ops.dequantize_l2_normalize``), so the host->device copy and the first HBM read carry 4x fewer
bytes.  ``dequantize=True`` reproduces the reference's float32 ``[max_frames, sum(feature_sizes)]`` matrix on the host.

Two routes lead through the reader.  ``batches()`` is the pure-Python one, and the yardstick.  ``device_batches()`` yields the same
batches as tensors on the GPU: a thread reads the records into pinned memory, the native indexer (``frame_records`` /
``locate_records``: lpm_tfrecord_frame, lpm_yt8m_locate) looks at their header bytes only, the record bytes go to the device as they
are and ``ops.gather_frames`` / ``ops.labels_dense`` put frames and labels in place.

``YT8MAggregatedFeatureReader`` is the reference's other input mode, and its default (readers.py:68-131): video-level files of
tf.train.Example records whose features are float lists (``mean_rgb``, ``mean_audio``).  The same two routes: ``batches()`` in Python,
``device_batches()`` through ``locate_examples`` (lpm_yt8m_locate_examples) and ``ops.gather_examples``.

There are no TFRecord fixtures in the reference; ``write_tfrecord`` / ``make_sequence_example`` / ``make_example`` produce files in the same
format for the round-trip tests and for synthetic data."""
from __future__ import annotations

import ctypes as C
import os
import queue
import struct
import threading
import time
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, Iterable, Iterator, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _capi, utils

# ---- CRC-32C (Castagnoli), table driven, and the TFRecord mask ---------------------------------------------------------
_CRC_TABLE = None


def _crc_table():
    global _CRC_TABLE
    if _CRC_TABLE is None:
        poly, tab = 0x82F63B78, []
        for i in range(256):
            c = i
            for _ in range(8):
                c = (c >> 1) ^ poly if c & 1 else c >> 1
            tab.append(c)
        _CRC_TABLE = tab
    return _CRC_TABLE


def crc32c(data: bytes) -> int:
    tab, c = _crc_table(), 0xFFFFFFFF
    for b in data:
        c = tab[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def masked_crc32c(data: bytes) -> int:
    c = crc32c(data)
    return ((((c >> 15) | (c << 17)) & 0xFFFFFFFF) + 0xA282EAD8) & 0xFFFFFFFF


def read_tfrecord(path: str, verify_crc: bool = False) -> Iterator[bytes]:
    """Yields the payload of every record of a TFRecord file."""
    with open(path, "rb") as f:
        while True:
            head = f.read(12)
            if not head:
                return
            if len(head) < 12:
                raise IOError(f"{path}: truncated record header")
            (length,), (lcrc,) = struct.unpack("<Q", head[:8]), struct.unpack("<I", head[8:])
            if verify_crc and masked_crc32c(head[:8]) != lcrc:
                raise IOError(f"{path}: corrupt record length")
            data = f.read(length)
            tail = f.read(4)
            if len(data) < length or len(tail) < 4:
                raise IOError(f"{path}: truncated record")
            if verify_crc and masked_crc32c(data) != struct.unpack("<I", tail)[0]:
                raise IOError(f"{path}: corrupt record payload")
            yield data


def write_tfrecord(path: str, records: Iterable[bytes]) -> None:
    with open(path, "wb") as f:
        for data in records:
            head = struct.pack("<Q", len(data))
            f.write(head + struct.pack("<I", masked_crc32c(head)) + data + struct.pack("<I", masked_crc32c(data)))


# ---- protobuf wire format (only what tf.train.SequenceExample needs) ----------------------------------------------------
def _varint(buf: bytes, i: int) -> Tuple[int, int]:
    shift = val = 0
    while True:
        b = buf[i]
        i += 1
        val |= (b & 0x7F) << shift
        if not b & 0x80:
            return val, i
        shift += 7


def _fields(buf: bytes) -> Iterator[Tuple[int, int, object]]:
    """(field number, wire type, value) for every field of a message; length-delimited values come as memoryviews."""
    i, n = 0, len(buf)
    mv = memoryview(buf)
    while i < n:
        key, i = _varint(buf, i)
        num, wt = key >> 3, key & 7
        if wt == 0:
            v, i = _varint(buf, i)
        elif wt == 2:
            ln, i = _varint(buf, i)
            v = mv[i:i + ln]
            i += ln
        elif wt == 5:
            v = mv[i:i + 4]
            i += 4
        elif wt == 1:
            v = mv[i:i + 8]
            i += 8
        else:
            raise ValueError(f"unsupported protobuf wire type {wt}")
        yield num, wt, v


def _parse_feature(buf, float_array: bool = False) -> Tuple[str, list]:
    """tf.train.Feature: oneof bytes_list = 1 / float_list = 2 / int64_list = 3.  ``float_array``: a float list comes back as a float32
    array holding the file's bits (a Python float is a double: the round trip would quieten a signalling NaN)."""
    for num, _, v in _fields(bytes(buf)):
        if num == 1:
            return "bytes", [bytes(x) for n2, _, x in _fields(bytes(v)) if n2 == 1]
        if num == 3:
            vals = []
            for n2, wt, x in _fields(bytes(v)):
                if n2 != 1:
                    continue
                if wt == 0:                                   # unpacked
                    vals.append(x)
                else:                                         # packed varints
                    xb, j = bytes(x), 0
                    while j < len(xb):
                        val, j = _varint(xb, j)
                        vals.append(val)
            return "int64", [val - (1 << 64) if val >= (1 << 63) else val for val in vals]
        if num == 2:
            runs = [np.frombuffer(bytes(x), dtype="<f4") for n2, wt, x in _fields(bytes(v)) if n2 == 1]
            if float_array:
                return "float", np.concatenate(runs).astype(np.float32, copy=False) if runs else np.zeros(0, np.float32)
            return "float", [x for run in runs for x in run.tolist()]
    return "empty", []


def _parse_map(buf, parse_value) -> Dict[str, object]:
    out = {}
    for num, _, entry in _fields(bytes(buf)):
        if num != 1:
            continue
        key, val = None, None
        for n2, _, x in _fields(bytes(entry)):
            if n2 == 1:
                key = bytes(x).decode("utf-8")
            elif n2 == 2:
                val = parse_value(x)
        out[key] = val
    return out


def parse_sequence_example(serialized: bytes):
    """-> (context {name: (kind, values)}, feature_lists {name: [(kind, values), ...]})."""
    context, lists = {}, {}
    for num, _, v in _fields(serialized):
        if num == 1:
            context = _parse_map(v, _parse_feature)
        elif num == 2:
            lists = _parse_map(v, lambda fl: [_parse_feature(x) for n2, _, x in _fields(bytes(fl)) if n2 == 1])
    return context, lists


def parse_example(serialized: bytes) -> Dict[str, Tuple[str, object]]:
    """tf.train.Example -> {name: (kind, values)}; float lists as float32 arrays with the file's bits.  (Example.features = 1,
    Features.feature = 1, a map: a later ``features`` field replaces an earlier one, the last entry of a name counts.)"""
    features = {}
    for num, _, v in _fields(serialized):
        if num == 1:
            features = _parse_map(v, lambda x: _parse_feature(x, float_array=True))
    return features


# ---- encoder (tests, synthetic data) ----------------------------------------------------------------------------------
def _enc_varint(v: int) -> bytes:
    v &= (1 << 64) - 1
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        out.append(b | (0x80 if v else 0))
        if not v:
            return bytes(out)


def _enc_ld(num: int, payload: bytes) -> bytes:
    return _enc_varint((num << 3) | 2) + _enc_varint(len(payload)) + payload


def _enc_bytes_feature(values: Sequence[bytes]) -> bytes:
    return _enc_ld(1, b"".join(_enc_ld(1, v) for v in values))


def _enc_int64_feature(values: Sequence[int]) -> bytes:
    return _enc_ld(3, _enc_ld(1, b"".join(_enc_varint(int(v)) for v in values)))


def make_sequence_example(video_id: str, labels: Sequence[int], features: Dict[str, np.ndarray]) -> bytes:
    """features: {name: uint8 [num_frames, feature_size]} -> serialized tf.train.SequenceExample (one bytes value per frame)."""
    ctx = _enc_ld(1, _enc_ld(1, b"id") + _enc_ld(2, _enc_bytes_feature([video_id.encode("utf-8")])))
    ctx += _enc_ld(1, _enc_ld(1, b"labels") + _enc_ld(2, _enc_int64_feature(labels)))
    fl = b""
    for name, mat in features.items():
        mat = np.ascontiguousarray(mat, dtype=np.uint8)
        flist = b"".join(_enc_ld(1, _enc_bytes_feature([row.tobytes()])) for row in mat)
        fl += _enc_ld(1, _enc_ld(1, name.encode("utf-8")) + _enc_ld(2, flist))
    return _enc_ld(1, ctx) + _enc_ld(2, fl)


def make_example(video_id: str, labels: Sequence[int], features: Dict[str, np.ndarray], packed: bool = True) -> bytes:
    """features: {name: float32 [feature_size]} -> serialized tf.train.Example (the video-level files' records).  ``packed``: one
    length-delimited run per float list, as every writer emits it; ``packed=False``: one tagged fixed32 per value."""
    out = _enc_ld(1, _enc_ld(1, b"id") + _enc_ld(2, _enc_bytes_feature([video_id.encode("utf-8")])))
    out += _enc_ld(1, _enc_ld(1, b"labels") + _enc_ld(2, _enc_int64_feature(labels)))
    for name, vec in features.items():
        raw = np.ascontiguousarray(vec, dtype="<f4").reshape(-1).tobytes()
        flist = _enc_ld(1, raw) if packed else b"".join(b"\x0d" + raw[i:i + 4] for i in range(0, len(raw), 4))
        out += _enc_ld(1, _enc_ld(1, name.encode("utf-8")) + _enc_ld(2, _enc_ld(2, flist)))
    return _enc_ld(1, out)


# ---- the native indexer (liblpm_hip.so, host code: no GPU needed; ctypes releases the GIL during the calls) --------------------------
class RecordIndex(NamedTuple):
    """locate_records' per-clip tables (numpy; offsets are bytes from the start of the buffer the records lie in)."""
    num_frames: np.ndarray      # int32 [n], capped at max_frames
    frame_offset: np.ndarray    # int64 [n, features, max_frames], -1 at and beyond num_frames
    label_start: np.ndarray     # int32 [n + 1]: clip i's labels are label_index[label_start[i]:label_start[i + 1]]
    label_index: np.ndarray     # int32 [>= label_start[n]]: the labels in [0, num_classes), file order, duplicates kept
    id_offset: np.ndarray       # int64 [n]
    id_length: np.ndarray       # int32 [n] (0 without an id)


def _as_bytes_array(buf) -> np.ndarray:
    a = buf if isinstance(buf, np.ndarray) else np.frombuffer(buf, dtype=np.uint8)
    if a.dtype != np.uint8 or a.ndim != 1 or not a.flags.c_contiguous:
        raise ValueError("expected a contiguous one-dimensional uint8 buffer")
    return a


def _vp(a: Optional[np.ndarray]):
    return None if a is None or a.size == 0 else C.c_void_p(a.ctypes.data)


def _raise_native(lib, status: int, what: str, prefix: str = ""):
    """LPM_ERR_IO -> IOError, LPM_ERR_DATA -> ValueError (the types read_tfrecord / prepare_serialized_examples raise)."""
    text = lib.last_error()
    if prefix:                                              # the caller names file and record itself: "<entry point>: record i: why" -> why
        text = prefix + text.split(": ", 2)[-1]
    if status == _capi.LPM_ERR_IO:
        raise IOError(text)
    if status == _capi.LPM_ERR_DATA:
        raise ValueError(text)
    raise _capi.LpmError(f"{what} failed with status {status}: {text}")


def frame_records(buf, verify_crc: bool = False, max_records: Optional[int] = None, record_base: int = 0):
    """TFRecord framing of a byte buffer (lpm_tfrecord_frame) -> (payload offsets int64 [n], payload lengths int64 [n], bytes consumed).
    Only whole records count: a caller reading a file in pieces carries ``buf[consumed:]`` over.  ``verify_crc`` checks both masked
    CRC-32Cs of every record (IOError, naming record ``record_base + i``)."""
    a = _as_bytes_array(buf)
    lib = _capi.load()
    offs, lens, consumed = [], [], 0
    nrec, used = C.c_int(0), C.c_int64(0)
    while max_records is None or len(offs) < max_records:
        chunk = 1024 if max_records is None else min(1024, max_records - len(offs))
        o, ln = np.empty(chunk, np.int64), np.empty(chunk, np.int64)
        rest = a[consumed:]
        st = lib._lpm_tfrecord_frame(_vp(rest), rest.size, int(bool(verify_crc)), chunk, record_base + len(offs), _vp(o), _vp(ln),
                                     C.byref(nrec), C.byref(used))
        if st != 0:
            _raise_native(lib, st, "lpm_tfrecord_frame")
        offs.extend((o[:nrec.value] + consumed).tolist())
        lens.extend(ln[:nrec.value].tolist())
        consumed += used.value
        if nrec.value < chunk:
            break
    return np.asarray(offs, np.int64), np.asarray(lens, np.int64), consumed


def frame_file(path: str, verify_crc: bool = False):
    """A whole TFRecord file -> (its bytes uint8 [size], payload offsets, payload lengths); IOError, naming the record, for a CRC
    mismatch and for a file that ends inside a record (read_tfrecord's errors)."""
    buf = np.fromfile(path, dtype=np.uint8)
    lib = _capi.load()
    try:
        offs, lens, consumed = frame_records(buf, verify_crc=verify_crc)
    except IOError as e:
        raise IOError(f"{path}: {lib.last_error()}") from e
    if consumed != buf.size:
        raise IOError(f"{path}: record {len(offs)}: truncated record")
    return buf, offs, lens


def _locate_into(lib, a, rec_offset, rec_length, names_arr, sizes_arr, num_features, max_frames, num_classes, record_base, idx: RecordIndex):
    """One lpm_yt8m_locate call into caller-owned arrays -> (status, labels needed, failed record)."""
    needed, failed = C.c_int64(0), C.c_int(-1)
    st = lib._lpm_yt8m_locate(_vp(a), a.size, _vp(rec_offset), _vp(rec_length), len(rec_offset), record_base, C.cast(names_arr, C.c_void_p),
                              C.cast(sizes_arr, C.c_void_p), num_features, max_frames, num_classes, _vp(idx.num_frames),
                              _vp(idx.frame_offset), _vp(idx.label_start), _vp(idx.label_index), idx.label_index.size, C.byref(needed),
                              _vp(idx.id_offset), _vp(idx.id_length), C.byref(failed))
    return st, needed.value, failed.value


def _feature_arrays(feature_names, feature_sizes):
    names = (C.c_char_p * len(feature_names))(*[str(n).encode("utf-8") for n in feature_names])
    sizes = (C.c_int * len(feature_sizes))(*[int(s) for s in feature_sizes])
    return names, sizes


def locate_records(buf, rec_offset, rec_length, feature_names=("rgb", "audio"), feature_sizes=(1024, 128), max_frames=300,
                   num_classes=3862, record_base: int = 0) -> RecordIndex:
    """Where the frames, labels and ids of the tf.train.SequenceExample records of ``buf`` lie (lpm_yt8m_locate): the header bytes are
    walked with parse_sequence_example's semantics, the frame payloads are never touched.  ValueError for what
    prepare_serialized_examples refuses (and for a frame whose payload is not its feature's size), naming the record."""
    a = _as_bytes_array(buf)
    ro, rl = np.ascontiguousarray(rec_offset, np.int64), np.ascontiguousarray(rec_length, np.int64)
    n, nf = len(ro), len(feature_names)
    names, sizes = _feature_arrays(feature_names, feature_sizes)
    lib = _capi.load()
    cap = 8 * n + 16
    while True:
        idx = RecordIndex(np.zeros(n, np.int32), np.full((n, nf, max_frames), -1, np.int64), np.zeros(n + 1, np.int32), np.zeros(cap, np.int32),
                          np.zeros(n, np.int64), np.zeros(n, np.int32))
        st, needed, _ = _locate_into(lib, a, ro, rl, names, sizes, nf, int(max_frames), int(num_classes), record_base, idx)
        if st == _capi.LPM_ERR_WORKSPACE and needed > cap:
            cap = needed
            continue
        if st != 0:
            _raise_native(lib, st, "lpm_yt8m_locate")
        return idx


class ExampleIndex(NamedTuple):
    """locate_examples' per-record tables (numpy; offsets are bytes from the start of the buffer the records lie in)."""
    feature_offset: np.ndarray  # int64 [n, features]: the first value's four bytes; -1 where the stride is 0
    feature_stride: np.ndarray  # int32 [n, features]: 4 (one packed run), 5 (tagged fixed32 values back to back), 0 (anything else: repack)
    label_start: np.ndarray     # int32 [n + 1]
    label_index: np.ndarray     # int32 [>= label_start[n]]
    id_offset: np.ndarray       # int64 [n]
    id_length: np.ndarray       # int32 [n] (0 without an id)


def _locate_examples_into(lib, a, rec_offset, rec_length, names_arr, sizes_arr, num_features, num_classes, record_base, idx: ExampleIndex):
    """One lpm_yt8m_locate_examples call into caller-owned arrays -> (status, labels needed, failed record)."""
    needed, failed = C.c_int64(0), C.c_int(-1)
    st = lib._lpm_yt8m_locate_examples(_vp(a), a.size, _vp(rec_offset), _vp(rec_length), len(rec_offset), record_base,
                                       C.cast(names_arr, C.c_void_p), C.cast(sizes_arr, C.c_void_p), num_features, num_classes,
                                       _vp(idx.feature_offset), _vp(idx.feature_stride), _vp(idx.label_start), _vp(idx.label_index),
                                       idx.label_index.size, C.byref(needed), _vp(idx.id_offset), _vp(idx.id_length), C.byref(failed))
    return st, needed.value, failed.value


def locate_examples(buf, rec_offset, rec_length, feature_names=("mean_rgb", "mean_audio"), feature_sizes=(1024, 128), num_classes=3862,
                    record_base: int = 0) -> ExampleIndex:
    """Where the float lists, labels and ids of the tf.train.Example records of ``buf`` lie (lpm_yt8m_locate_examples): the header bytes
    are walked with parse_example's semantics, the values are never touched.  ValueError for what
    YT8MAggregatedFeatureReader.prepare_serialized_examples refuses, naming the record.  A list in an encoding that has no constant
    stride comes back with stride 0 and offset -1: valid, and for the caller to repack."""
    a = _as_bytes_array(buf)
    ro, rl = np.ascontiguousarray(rec_offset, np.int64), np.ascontiguousarray(rec_length, np.int64)
    n, nf = len(ro), len(feature_names)
    names, sizes = _feature_arrays(feature_names, feature_sizes)
    lib = _capi.load()
    cap = 8 * n + 16
    while True:
        idx = ExampleIndex(np.full((n, nf), -1, np.int64), np.zeros((n, nf), np.int32), np.zeros(n + 1, np.int32), np.zeros(cap, np.int32),
                           np.zeros(n, np.int64), np.zeros(n, np.int32))
        st, needed, _ = _locate_examples_into(lib, a, ro, rl, names, sizes, nf, int(num_classes), record_base, idx)
        if st == _capi.LPM_ERR_WORKSPACE and needed > cap:
            cap = needed
            continue
        if st != 0:
            _raise_native(lib, st, "lpm_yt8m_locate_examples")
        return idx


# ---- the reader ---------------------------------------------------------------------------------------------------------
class BaseReader(object):
    """readers.py:59-66."""

    def prepare_reader(self, unused_filename_queue):
        raise NotImplementedError()


class _RecordFileReader(BaseReader):
    """What the two YT8M readers share: ``batches()`` of a subclass, on the device and shuffled."""

    def device_batches(self, files: Sequence[str], batch_size: int, device="cuda", drop_remainder: bool = False, verify_crc: bool = False,
                       prefetch: int = 2, reader_threads: int = 1, stats: Optional[dict] = None):
        """What ``batches()`` yields, as tensors on the GPU: (ids, frames uint8 cuda [B, max_frames, F] -- the video-level reader: features
        float32 cuda [B, F] --, labels bool cuda [B, V], num_frames int32 cuda [B]), bit for bit.  A background thread reads the records of one batch back to back into a pinned host
        slot, runs the native indexer over their header bytes, copies slot and tables to the device on a side stream and launches
        ``ops.gather_frames`` (the video-level reader: ``ops.gather_examples``) / ``ops.labels_dense`` there; the consumer's current stream waits for that batch's event.  The tensors belong
        to the consumer.  ``prefetch``: finished batches that may wait for the consumer (the ring has prefetch + reader_threads pinned slots).
        ``reader_threads``: threads that read whole batches into their slots (1: the thread that walks the record headers itself).  ``stats``: a dict that receives the host
        seconds spent reading and indexing, bytes, batches, and (``stats["time_gather"] = True``) device events before the copies, between copies and kernels and after them.
        Errors (IOError: framing, CRC, truncation; ValueError: a malformed example) are raised at the batch they belong to; closing the
        generator stops and joins the thread.  Needs a GPU: there is no CPU fallback (use ``batches()``)."""
        dev = torch.device(device)
        if dev.type != "cuda" or not torch.cuda.is_available():
            raise _capi.LpmError("device_batches needs an MI355X (cuda/hip device); batches() is the host route")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self._check_device_features()
        if int(batch_size) < 1 or int(prefetch) < 1 or int(reader_threads) < 1:
            raise ValueError("device_batches: batch_size, prefetch and reader_threads must be at least 1")
        _capi.load()
        pipe = _DevicePipeline(self, list(files), int(batch_size), dev, bool(drop_remainder), bool(verify_crc), int(prefetch),
                               int(reader_threads), stats)
        try:
            while True:
                item = pipe.get()
                if item is None:
                    return
                if isinstance(item, BaseException):
                    raise item
                ids, frames, labels, nf, done = item
                cur = torch.cuda.current_stream(dev)
                cur.wait_event(done)
                for t in (frames, labels, nf):                  # allocated on the side stream, used (and freed) on the consumer's
                    t.record_stream(cur)
                yield ids, frames, labels, nf
        finally:
            pipe.close()

    def training_batches(self, files: Sequence[str], batch_size: int, device="cuda", num_epochs: Optional[int] = None, seed: int = 0,
                         shuffle_files: bool = True, capacity: Optional[int] = None, min_after_dequeue: Optional[int] = None,
                         **device_batches_kwargs):
        """The training input order (reference: train.py:172-184, ``string_input_producer(shuffle=True)`` feeding
        ``shuffle_batch_join(capacity=5*batch, min_after_dequeue=batch, allow_smaller_final_batch=True)``): yields what
        ``device_batches`` (on a CPU device: ``batches``) yields, with the clips shuffled through a ``ShufflePool`` on ``device``.
        The file list is permuted once at the start of every epoch (``shuffle_files``) with the pool's generator; epochs follow each
        other without draining the pool, as the reference's filename queue feeds its readers; ``num_epochs=None`` runs until the
        consumer stops.  Every batch has ``batch_size`` clips except the last one of a finite run.

        The same parameters and guarantees as the reference's queues -- NOT the same random stream: the order comes from
        ``numpy.random.Generator(PCG64(seed))`` and is reproducible for a seed, a file list and a batch size, on either device.
        Closing the generator closes the underlying ``device_batches`` generator (its threads are joined)."""
        files = list(files)
        dev = torch.device(device)
        rng = np.random.Generator(np.random.PCG64(seed))

        def source():
            epoch = 0
            while num_epochs is None or epoch < num_epochs:
                order = [files[i] for i in rng.permutation(len(files))] if shuffle_files else files
                if dev.type == "cuda":
                    yield from self.device_batches(order, batch_size, device=dev, **device_batches_kwargs)
                else:
                    yield from self.batches(order, batch_size, **device_batches_kwargs)
                epoch += 1
                if not files:
                    return
        src = source()
        try:
            yield from ShufflePool(src, batch_size, capacity=capacity, min_after_dequeue=min_after_dequeue, rng=rng)
        finally:
            src.close()


class YT8MFrameFeatureReader(_RecordFileReader):
    """readers.py:134-271.  Same constructor; records come from files instead of a TF filename queue."""

    def __init__(self, num_classes=3862, feature_sizes=(1024, 128), feature_names=("rgb", "audio"), max_frames=300):
        assert len(feature_names) == len(feature_sizes), \
            "length of feature_names (={}) != length of feature_sizes (={})".format(len(feature_names), len(feature_sizes))
        assert len(feature_names) > 0, "No feature selected: feature_names is empty!"
        self.num_classes = num_classes
        self.feature_sizes = list(feature_sizes)
        self.feature_names = list(feature_names)
        self.max_frames = max_frames

    def _check_device_features(self):
        if any(int(s) <= 0 or int(s) % 4 for s in self.feature_sizes) or len(self.feature_sizes) > 8:
            raise _capi.LpmError(f"device_batches: at most 8 features whose sizes are positive multiples of 4 (got {self.feature_sizes})")

    def prepare_serialized_examples(self, serialized_example: bytes, max_quantized_value=2, min_quantized_value=-2,
                                    dequantize=False):
        """-> (video_id, frames [max_frames, sum(feature_sizes)], labels bool [num_classes], num_frames).  frames is uint8
        (quantised, zero beyond num_frames) or, with dequantize=True, the reference's float32 matrix (readers.py:176-193)."""
        context, lists = parse_sequence_example(serialized_example)
        video_id = context["id"][1][0].decode("utf-8") if "id" in context else ""
        labels = np.zeros(self.num_classes, dtype=bool)
        for v in context.get("labels", ("int64", []))[1]:
            if 0 <= v < self.num_classes:                      # sparse_to_dense(validate_indices=False)
                labels[v] = True
        num_frames, mats = -1, []
        for name, size in zip(self.feature_names, self.feature_sizes):
            rows = [np.frombuffer(vals[0], dtype=np.uint8) for _, vals in lists[name]]
            mat = np.stack(rows).reshape(-1, size) if rows else np.zeros((0, size), dtype=np.uint8)
            n = min(mat.shape[0], self.max_frames)
            if num_frames == -1:
                num_frames = n
            elif n != num_frames:
                raise ValueError(f"{video_id}: feature '{name}' has {n} frames, expected {num_frames}")
            mats.append(mat[:n])
        q = np.zeros((self.max_frames, sum(self.feature_sizes)), dtype=np.uint8)
        q[:num_frames] = np.concatenate(mats, axis=1)
        if dequantize:
            f = np.zeros(q.shape, dtype=np.float32)
            f[:num_frames] = utils.Dequantize(q[:num_frames].astype(np.float32), max_quantized_value, min_quantized_value)
            return video_id, f, labels, num_frames
        return video_id, q, labels, num_frames

    def batches(self, files: Sequence[str], batch_size: int, drop_remainder: bool = False, verify_crc: bool = False):
        """Yields (ids, frames uint8 [B, max_frames, F], labels bool [B, V], num_frames int32 [B]) as torch tensors."""
        ids: List[str] = []
        q, y, nf = [], [], []

        def flush():
            out = (list(ids), torch.from_numpy(np.stack(q)), torch.from_numpy(np.stack(y)), torch.tensor(nf, dtype=torch.int32))
            ids.clear(); q.clear(); y.clear(); nf.clear()
            return out
        for path in files:
            for rec in read_tfrecord(path, verify_crc=verify_crc):
                vid, frames, labels, n = self.prepare_serialized_examples(rec)
                ids.append(vid); q.append(frames); y.append(labels); nf.append(n)
                if len(ids) == batch_size:
                    yield flush()
        if ids and not drop_remainder:
            yield flush()


class YT8MAggregatedFeatureReader(_RecordFileReader):
    """readers.py:68-131: the video-level files, one tf.train.Example of float lists per video.  Same constructor; records come from
    files instead of a TF filename queue."""

    def __init__(self, num_classes=3862, feature_sizes=(1024, 128), feature_names=("mean_rgb", "mean_audio")):
        assert len(feature_names) == len(feature_sizes), \
            "length of feature_names (={}) != length of feature_sizes (={})".format(len(feature_names), len(feature_sizes))
        assert len(feature_names) > 0, "No feature selected: feature_names is empty!"
        self.num_classes = num_classes
        self.feature_sizes = list(feature_sizes)
        self.feature_names = list(feature_names)

    def _check_device_features(self):
        if any(int(s) <= 0 for s in self.feature_sizes) or len(self.feature_sizes) > 8 or len(set(self.feature_names)) != len(self.feature_names):
            raise _capi.LpmError(f"device_batches: at most 8 distinct features of positive sizes (got {self.feature_names}, {self.feature_sizes})")

    def prepare_serialized_examples(self, serialized_example: bytes):
        """-> (video_id, features float32 [sum(feature_sizes)], labels bool [num_classes], 1): ``tf.parse_example`` as
        readers.py:104-131 configures it.  Every selected feature is a ``FixedLenFeature``: it has to be there, be a float list and hold
        exactly its size in values (ValueError, naming the id and the feature); ``labels`` is a ``VarLenFeature``: missing means none.
        As in YT8MFrameFeatureReader, and unlike a strict ``tf.sparse_to_dense``: label values outside [0, num_classes) are dropped,
        and a record without an ``id`` has the id "".  The features keep the file's bits."""
        feats = parse_example(serialized_example)
        video_id = feats["id"][1][0].decode("utf-8") if "id" in feats else ""
        labels = np.zeros(self.num_classes, dtype=bool)
        for v in feats.get("labels", ("int64", []))[1]:
            if 0 <= v < self.num_classes:
                labels[v] = True
        parts = []
        for name, size in zip(self.feature_names, self.feature_sizes):
            if feats.get(name) is None:
                raise ValueError(f"{video_id}: feature '{name}' is missing")
            kind, vals = feats[name]
            if kind != "float":
                raise ValueError(f"{video_id}: feature '{name}' is a {kind} list, not a float list")
            if len(vals) != size:
                raise ValueError(f"{video_id}: feature '{name}' has {len(vals)} values, expected {size}")
            parts.append(vals)
        return video_id, np.concatenate(parts), labels, 1

    def batches(self, files: Sequence[str], batch_size: int, drop_remainder: bool = False, verify_crc: bool = False):
        """Yields (ids, features float32 [B, F], labels bool [B, V], num_frames int32 [B] of ones -- the reference returns
        ``tf.ones([batch])`` in that slot) as torch tensors."""
        ids: List[str] = []
        x, y = [], []

        def flush():
            out = (list(ids), torch.from_numpy(np.stack(x)), torch.from_numpy(np.stack(y)), torch.ones(len(ids), dtype=torch.int32))
            ids.clear(); x.clear(); y.clear()
            return out
        for path in files:
            records, i = read_tfrecord(path, verify_crc=verify_crc), -1
            while True:
                i += 1
                try:                                            # (errors name the record, as device_batches' do)
                    rec = next(records, None)
                    if rec is None:
                        break
                    vid, features, labels, _ = self.prepare_serialized_examples(rec)
                except (IOError, ValueError) as e:
                    raise type(e)(f"{path}: record {i}: {str(e).replace(path + ': ', '', 1)}") from e
                ids.append(vid); x.append(features); y.append(labels)
                if len(ids) == batch_size:
                    yield flush()
        if ids and not drop_remainder:
            yield flush()


class ShufflePool:
    """``tf.train.shuffle_batch_join``'s policy over any iterator of (ids, frames, labels, num_frames) batches whose tensors live on
    one device (``batches()`` output on the CPU, ``device_batches()`` output on the GPU).

    The pool holds up to ``capacity`` clips in tensors preallocated on the input's device when the first batch arrives (the ids stay on
    the host).  Before each dequeue it pulls input batches while a whole one (the largest seen so far) still fits.  A dequeue draws
    ``batch_size`` distinct clips uniformly from the pool with a host generator (``numpy.random.Generator(PCG64(seed))``) and needs
    ``min_after_dequeue`` clips to stay behind until the input is exhausted; then the pool drains and the last batch may be smaller.
    Clips leave through ``index_select`` and arrive in the holes through ``index_copy_`` on the consumer's current stream; every count
    is known on the host from ``len(ids)``, so nothing waits for the device.  The yielded tensors are fresh and belong to the consumer.
    The same guarantees as the reference's queue, not its random stream."""

    def __init__(self, batches, batch_size: int, capacity: Optional[int] = None, min_after_dequeue: Optional[int] = None, seed: int = 0,
                 rng: Optional[np.random.Generator] = None):
        self.batch_size = int(batch_size)
        self.capacity = 5 * self.batch_size if capacity is None else int(capacity)
        self.min_after_dequeue = self.batch_size if min_after_dequeue is None else int(min_after_dequeue)
        if self.batch_size < 1 or self.min_after_dequeue < 0 or self.capacity < self.batch_size + self.min_after_dequeue:
            raise ValueError("ShufflePool: need batch_size >= 1, min_after_dequeue >= 0 and capacity >= batch_size + min_after_dequeue")
        self.rng = np.random.Generator(np.random.PCG64(seed)) if rng is None else rng
        self._it = iter(batches)
        self._exhausted = False
        self._pool = None                                   # (frames, labels, num_frames), each [capacity, ...]
        self._ids: List[object] = [None] * self.capacity
        self._filled = np.zeros(0, dtype=np.int64)          # slots that hold a clip
        self._free = list(range(self.capacity - 1, -1, -1))  # slots that do not (a stack: slot 0 first)
        self._in_batch = 0                                  # clips of the largest input batch seen

    def __len__(self):
        return len(self._filled)

    def _index(self, slots, dev):
        idx = torch.from_numpy(np.ascontiguousarray(slots, dtype=np.int64))
        if dev.type != "cuda":
            return idx
        pinned = torch.empty(idx.shape, dtype=torch.int64, pin_memory=True)      # (caching host allocator: reused only after the copy)
        pinned.copy_(idx)
        return pinned.to(dev, non_blocking=True)

    def _pull(self) -> bool:
        try:
            ids, frames, labels, nf = next(self._it)
        except StopIteration:
            self._exhausted = True
            return False
        n = len(ids)
        if n == 0:
            return True
        if not (frames.shape[0] == labels.shape[0] == nf.shape[0] == n):
            raise ValueError("ShufflePool: a batch's tensors and ids disagree on the number of clips")
        if self._pool is None:
            self._pool = tuple(torch.empty((self.capacity,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device) for t in (frames, labels, nf))
        if n > len(self._free):
            raise ValueError(f"ShufflePool: an input batch of {n} clips does not fit (capacity {self.capacity}, "
                             f"{len(self._filled)} clips held)")
        self._in_batch = max(self._in_batch, n)
        slots = np.array([self._free.pop() for _ in range(n)], dtype=np.int64)
        idx = self._index(slots, self._pool[0].device)
        for dst, t in zip(self._pool, (frames, labels, nf)):
            if t.device != dst.device or t.dtype != dst.dtype or t.shape[1:] != dst.shape[1:]:
                raise ValueError("ShufflePool: every batch must have the first one's device, dtypes and clip shapes")
            dst.index_copy_(0, idx, t)
        for s_, i in zip(slots, ids):
            self._ids[s_] = i
        self._filled = np.concatenate([self._filled, slots])
        return True

    def _dequeue(self, n: int):
        pos = self.rng.choice(len(self._filled), size=n, replace=False)
        slots = self._filled[pos]
        keep = np.ones(len(self._filled), dtype=bool)
        keep[pos] = False
        self._filled = self._filled[keep]
        idx = self._index(slots, self._pool[0].device)
        frames, labels, nf = (t.index_select(0, idx) for t in self._pool)
        ids = [self._ids[s_] for s_ in slots]
        for s_ in slots[::-1]:
            self._ids[s_] = None
            self._free.append(int(s_))
        return ids, frames, labels, nf

    def __iter__(self):
        while True:
            # room for a whole input batch (the first one: unknown size, the pool is empty): pull
            while not self._exhausted and len(self._free) >= max(self._in_batch, 1):
                self._pull()
            held = len(self._filled)
            if not self._exhausted:
                if held - self.batch_size < self.min_after_dequeue:
                    raise ValueError(f"ShufflePool: capacity {self.capacity} cannot hold batch_size + min_after_dequeue = "
                                     f"{self.batch_size + self.min_after_dequeue} clips next to a free input batch of {self._in_batch}")
                yield self._dequeue(self.batch_size)
            elif held:
                yield self._dequeue(min(self.batch_size, held))
            else:
                return


class _Slot:
    """One pinned host slot of the ring: the records of one batch back to back (framing included), and the tables that go to the device
    with them.  ``copied`` is recorded after the copies out of the slot; the slot is not refilled before it has completed."""

    def __init__(self, nbytes: int):
        self.copied: Optional[torch.cuda.Event] = None
        self.free = threading.Event()                           # set while the read thread may take the slot
        self.free.set()
        self._alloc(nbytes)
        self.meta = torch.empty(1 << 16, dtype=torch.uint8, pin_memory=True)

    def _alloc(self, nbytes: int):
        self.t = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        self.np = self.t.numpy()
        self.mv = memoryview(self.np)

    def reserve(self, nbytes: int, keep: int = 0):
        """Room for nbytes; the first ``keep`` bytes stay (0: the slot is empty)."""
        if nbytes > self.t.numel():
            old = self.np
            self._alloc(max(nbytes, 2 * self.t.numel()))
            self.np[:keep] = old[:keep]

    def reserve_meta(self, nbytes: int):
        if nbytes > self.meta.numel():
            self.meta = torch.empty(max(nbytes, 2 * self.meta.numel()), dtype=torch.uint8, pin_memory=True)


def _pread_exact(fd: int, mv, offset: int) -> int:
    """Fills mv from the file at ``offset``; returns the bytes read (short only at the end of the file)."""
    n = 0
    while n < len(mv):
        r = os.preadv(fd, [mv[n:]], offset + n)
        if r == 0:
            break
        n += r
    return n


class _DevicePipeline:
    """The two threads behind the readers' device_batches (DESIGN.md sections 13, 22): one reads the records of batch k + 1 into a
    pinned slot while the other indexes batch k, enqueues its copies and kernels and hands it to the consumer.  The read side does not
    know what a record holds; ``_emit`` indexes and gathers frames (SequenceExample) or float lists (Example, ``self.examples``)."""

    def __init__(self, reader, files, batch_size, dev, drop_remainder, verify_crc, prefetch, reader_threads, stats):
        self.reader, self.files, self.B, self.dev = reader, files, batch_size, dev
        self.drop_remainder, self.verify_crc, self.nthreads = drop_remainder, verify_crc, reader_threads
        self.examples = isinstance(reader, YT8MAggregatedFeatureReader)
        self.stats = stats if stats is not None else {}
        self.lock = threading.Lock()
        for k in ("walk_s", "read_s", "index_s", "issue_s", "bytes", "batches", "clips"):
            self.stats.setdefault(k, 0)
        self.time_gather = bool(self.stats.get("time_gather"))
        if self.time_gather:
            self.stats.setdefault("gather_events", [])
        self.nslots = prefetch + reader_threads
        self.slots: List[_Slot] = []
        self.mid = queue.Queue()                               # read thread -> index thread: (slot, bytes, records) | None | exception
        self.out = queue.Queue(maxsize=prefetch)               # index thread -> consumer: batches | None | exception
        self.stop = threading.Event()
        self.threads = [threading.Thread(target=self._run_read, name="lpm-device-batches-read", daemon=True),
                        threading.Thread(target=self._run_index, name="lpm-device-batches-index", daemon=True)]
        for t in self.threads:
            t.start()

    # ---- consumer side ------------------------------------------------------------------------------------------------------------
    def get(self):
        return self.out.get()

    def close(self):
        self.stop.set()
        while any(t.is_alive() for t in self.threads):
            try:
                self.out.get_nowait()                          # a producer blocked on a full queue sees the stop flag within its timeout
            except queue.Empty:
                pass
            for t in self.threads:
                t.join(timeout=0.02)
        while True:                                            # drop what is left (device tensors of batches nobody asked for)
            try:
                self.out.get_nowait()
            except queue.Empty:
                break
        for s in self.slots:                                   # nothing may still read a slot when its pinned memory goes
            if s.copied is not None:
                s.copied.synchronize()

    # ---- producer side: one thread reads records into the slots, one indexes them and drives the device ---------------------------------
    def _put(self, item) -> bool:
        while not self.stop.is_set():
            try:
                self.out.put(item, timeout=0.05)
                return True
            except queue.Full:
                continue
        return False

    def _run_read(self):
        pool = ThreadPoolExecutor(max_workers=self.nthreads, thread_name_prefix="lpm-record-read") if self.nthreads > 1 else None
        try:
            torch.cuda.set_device(self.dev)                     # (pinned allocations)
            self._fill(pool)
            self.mid.put(None)
        except BaseException as e:                              # handed on in order: raised in the consumer after the batches before it
            self.mid.put(e)
        finally:
            if pool is not None:
                pool.shutdown(wait=True)

    def _run_index(self):
        try:
            torch.cuda.set_device(self.dev)
            self.side = torch.cuda.Stream(device=self.dev)
            while not self.stop.is_set():
                try:
                    item = self.mid.get(timeout=0.05)
                except queue.Empty:
                    continue
                if item is None or isinstance(item, BaseException):
                    self._put(item)
                    return
                job, slot, nbytes, src = item
                try:
                    if job is not None:
                        job.result()                            # the read of this batch (a reader thread's IOError surfaces here, in order)
                    ok = self._emit(slot, nbytes, src)
                finally:
                    slot.free.set()
                if not ok:
                    return
        except BaseException as e:
            self._put(e)
            self.stop.set()                                     # the read thread has nobody to read for any more

    def _acquire(self, k: int, nbytes: int) -> Optional[_Slot]:
        """Slot k % nslots, once the index thread is done with it and the copy out of it has completed; None when stopping."""
        if len(self.slots) < self.nslots:
            self.slots.append(_Slot(nbytes if not self.slots else self.slots[0].t.numel()))
        slot = self.slots[k % self.nslots]
        while not slot.free.wait(timeout=0.05):
            if self.stop.is_set():
                return None
        if slot.copied is not None:
            slot.copied.synchronize()
            slot.copied = None
        slot.free.clear()
        return slot

    def _fill(self, pool):
        """Walks the record headers of the files (12 bytes each: the payload is not read here), cuts the stream into batches and has every
        batch read into its slot: one positioned read per run of records that lie back to back in one file, which is the layout of
        the slot as well."""
        k = 0                                                   # batch counter: slot k % nslots
        segs, src, total = [], [], 0                            # runs [path, file offset, bytes]; (path, index in its file) per record
        head = bytearray(12)
        hv = memoryview(head)
        for path in self.files:
            with open(path, "rb", buffering=0) as f:
                fd = f.fileno()
                size, fpos, idx = os.fstat(fd).st_size, 0, 0
                while not self.stop.is_set():
                    t0 = time.perf_counter()
                    got = _pread_exact(fd, hv, fpos)
                    if got == 0:
                        break
                    if got < 12:
                        raise IOError(f"{path}: record {idx}: truncated record header")
                    (length,) = struct.unpack_from("<Q", head)
                    if length + 4 > size - fpos - 12:           # (also a corrupt length: nothing that large is read or allocated)
                        raise IOError(f"{path}: record {idx}: truncated record")
                    n = 16 + length
                    if segs and segs[-1][0] == path and segs[-1][1] + segs[-1][2] == fpos:
                        segs[-1][2] += n
                    else:
                        segs.append([path, fpos, n])
                    src.append((path, idx))
                    total += n
                    fpos += n
                    idx += 1
                    self.stats["walk_s"] += time.perf_counter() - t0
                    if len(src) == self.B:
                        if not self._submit(pool, k, segs, src, total):
                            return
                        k += 1
                        segs, src, total = [], [], 0
            if self.stop.is_set():
                return
        if src and not self.drop_remainder:
            self._submit(pool, k, segs, src, total)

    def _submit(self, pool, k, segs, src, total) -> bool:
        slot = self._acquire(k, total + total // 4)
        if slot is None:
            return False
        slot.reserve(total)
        if pool is None:
            self._read_job(slot, segs)
            self.mid.put((None, slot, total, src))
        else:
            self.mid.put((pool.submit(self._read_job, slot, segs), slot, total, src))
        return True

    def _read_job(self, slot: _Slot, segs):
        t0 = time.perf_counter()
        pos = 0
        for path, off, n in segs:
            fd = os.open(path, os.O_RDONLY)
            try:
                got = _pread_exact(fd, slot.mv[pos:pos + n], off)
            finally:
                os.close(fd)
            if got < n:
                raise IOError(f"{path}: truncated record (the file ends before offset {off + n})")
            pos += n
        with self.lock:
            self.stats["read_s"] += time.perf_counter() - t0

    def _emit(self, slot: _Slot, nbytes: int, src) -> bool:
        """Index the slot's records, send slot and tables to the device, gather; False when the consumer has gone."""
        from . import ops
        r, lib = self.reader, _capi.load()
        n, nfeat = len(src), len(r.feature_names)
        T = 1 if self.examples else r.max_frames
        t0 = time.perf_counter()
        buf = slot.np[:nbytes]
        ro, rl = np.empty(n, np.int64), np.empty(n, np.int64)
        nrec, used = C.c_int(0), C.c_int64(0)
        st = lib._lpm_tfrecord_frame(_vp(buf), nbytes, int(self.verify_crc), n, 0, _vp(ro), _vp(rl), C.byref(nrec), C.byref(used))
        if st != 0:
            path, idx = src[min(nrec.value, n - 1)]
            _raise_native(lib, st, "lpm_tfrecord_frame", f"{path}: record {idx}: ")
        if nrec.value != n or used.value != nbytes:
            raise IOError(f"{src[0][0]}: the slot's framing does not match the records read ({nrec.value} of {n})")
        names, sizes = _feature_arrays(r.feature_names, r.feature_sizes)
        id_off, id_len = np.empty(n, np.int64), np.empty(n, np.int32)
        # the tables, in one pinned block: offsets (examples: offsets int64 | strides int32) | label_start | num_frames | labels
        n_off = 8 * n * nfeat * T
        n_tab = n_off + 4 * n * nfeat if self.examples else n_off
        n_fixed = n_tab + 4 * (n + 1) + 4 * n
        slot.reserve_meta(n_fixed + 4 * (8 * n + 64))
        what = "lpm_yt8m_locate_examples" if self.examples else "lpm_yt8m_locate"
        while True:
            m = slot.meta.numpy()
            label_start, num_frames = m[n_tab:n_tab + 4 * (n + 1)].view(np.int32), m[n_tab + 4 * (n + 1):n_fixed].view(np.int32)
            label_index = m[n_fixed:(m.size // 4) * 4].view(np.int32)
            if self.examples:
                idx = ExampleIndex(m[:n_off].view(np.int64).reshape(n, nfeat), m[n_off:n_tab].view(np.int32).reshape(n, nfeat), label_start,
                                   label_index, id_off, id_len)
                st, needed, failed = _locate_examples_into(lib, buf, ro, rl, names, sizes, nfeat, r.num_classes, 0, idx)
            else:
                idx = RecordIndex(num_frames, m[:n_off].view(np.int64), label_start, label_index, id_off, id_len)
                st, needed, failed = _locate_into(lib, buf, ro, rl, names, sizes, nfeat, T, r.num_classes, 0, idx)
            if st == _capi.LPM_ERR_WORKSPACE and n_fixed + 4 * needed > slot.meta.numel():
                slot.reserve_meta(n_fixed + 4 * needed)
                continue
            if st != 0:
                path, i = src[max(failed, 0)]
                _raise_native(lib, st, what, f"{path}: record {i}: ")
            break
        nlab = int(idx.label_start[n])
        ids = [bytes(buf[o:o + ln]).decode("utf-8") for o, ln in zip(id_off.tolist(), id_len.tolist())]
        if self.examples:
            num_frames[:] = 1
            nbytes = self._repack(slot, nbytes, ro, rl, idx)
        t1 = time.perf_counter()
        with torch.cuda.stream(self.side):
            ev = None
            if self.time_gather:                                # (before the copies, between copies and kernels, after the kernels)
                ev = tuple(torch.cuda.Event(enable_timing=True) for _ in range(3))
                ev[0].record(self.side)
            raw = torch.empty(((nbytes + 15) // 16) * 16 + 16, dtype=torch.uint8, device=self.dev)
            raw[:nbytes].copy_(slot.t[:nbytes], non_blocking=True)
            n_meta = n_fixed + 4 * nlab
            meta = torch.empty(n_meta, dtype=torch.uint8, device=self.dev)
            meta.copy_(slot.meta[:n_meta], non_blocking=True)
            slot.copied = torch.cuda.Event()
            slot.copied.record(self.side)
            nf = meta[n_tab + 4 * (n + 1):n_fixed].view(torch.int32).clone()      # (its own storage: it goes to the consumer)
            if ev is not None:
                ev[1].record(self.side)
            if self.examples:
                frames = ops.gather_examples(raw, nbytes, meta[:n_off].view(torch.int64).view(n, nfeat),
                                             meta[n_off:n_tab].view(torch.int32).view(n, nfeat), r.feature_sizes)
            else:
                frames = ops.gather_frames(raw, nbytes, meta[:n_off].view(torch.int64).view(n, nfeat, T), nf, r.feature_sizes, T)
            labels = ops.labels_dense(meta[n_tab:n_tab + 4 * (n + 1)].view(torch.int32), meta[n_fixed:n_meta].view(torch.int32),
                                      r.num_classes)
            if ev is not None:
                ev[2].record(self.side)
                self.stats["gather_events"].append(ev)
            done = torch.cuda.Event()
            done.record(self.side)
        t2 = time.perf_counter()
        st_ = self.stats
        st_["index_s"] += t1 - t0
        st_["issue_s"] += t2 - t1
        st_["bytes"] += nbytes
        st_["batches"] += 1
        st_["clips"] += n
        return self._put((ids, frames, labels, nf, done))

    def _repack(self, slot: _Slot, nbytes: int, ro, rl, idx: ExampleIndex) -> int:
        """Float lists without a constant stride (stride 0: several runs, a mix of packed and unpacked values, ...): the Python parser
        reads that record, its values go packed into the slot behind the records and the table points there.  -> the slot's bytes."""
        rows, cols = np.nonzero(idx.feature_stride == 0)
        if rows.size == 0:
            return nbytes
        sizes = [int(s) for s in self.reader.feature_sizes]
        pos = (nbytes + 3) & ~3
        slot.reserve(pos + 4 * sum(sizes[f] for f in cols.tolist()), keep=nbytes)
        parsed = {}
        for i, f in zip(rows.tolist(), cols.tolist()):
            if i not in parsed:
                parsed[i] = parse_example(bytes(slot.np[ro[i]:ro[i] + rl[i]]))
            vals = np.ascontiguousarray(parsed[i][self.reader.feature_names[f]][1], dtype="<f4")
            if vals.size != sizes[f]:
                raise ValueError(f"feature '{self.reader.feature_names[f]}' has {vals.size} values, expected {sizes[f]}")
            slot.np[pos:pos + 4 * sizes[f]] = vals.view(np.uint8)
            idx.feature_offset[i, f], idx.feature_stride[i, f] = pos, 4
            pos += 4 * sizes[f]
        return pos
