"""-m "not gpu": the TensorBoard writer's host side -- golden bytes of the Event / Summary / HistogramProto encoding (derived with the
protobuf runtime from the .proto layout, not with the writer), an independent decode with google.protobuf where it imports, TensorFlow's
bucket limits and its run-collapsing rule, the numpy histogram path, read_events' round trip and CRC check, training.run's scalars (with
a stand-in trainer, as tests/test_training_host.py: Trainer.step has no CPU path) and evaluate's Epoch/Eval_* tags."""
import ctypes
import logging
import os
import re
import struct
import threading

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lpm_hip.h")
DBL_MAX = 1.7976931348623157e308

GOLDEN_SCALAR = "09000000000000f83f100a2a0a0a080a0161150000003f"
GOLDEN_VERSION = "09000000000000f83f1a0d627261696e2e4576656e743a32"
GOLDEN_HISTO = ("09000000000000004010032a680a660a01682a6109000000000000f0bf11000000000000004019000000000000084021000000000000f83f29000000"
                "00000015403218000000000000f0bf000000000000e03f00000000000004403a18000000000000f03f000000000000f03f000000000000f03f")


def _frame(data: bytes) -> bytes:
    from learnablepoolingmethods_amd.readers import masked_crc32c
    head = struct.pack("<Q", len(data))
    return head + struct.pack("<I", masked_crc32c(head)) + data + struct.pack("<I", masked_crc32c(data))


# ---- golden bytes ------------------------------------------------------------------------------------------------------------------
def test_golden_bytes_of_events_and_of_a_written_file(tmp_path):
    from learnablepoolingmethods_amd import readers, summaries as S
    assert S.encode_event(1.5, 10, values=[S.encode_value("a", simple_value=0.5)]).hex() == GOLDEN_SCALAR
    assert S.encode_event(1.5, file_version="brain.Event:2").hex() == GOLDEN_VERSION
    histo = S.encode_histogram([-1.0, 2.0, 3.0, 1.5, 5.25], [1, 1, 1], [-1.0, 0.5, 2.5])
    assert S.encode_event(2.0, 3, values=[S.encode_value("h", histo=histo)]).hex() == GOLDEN_HISTO
    assert len(bytes.fromhex(GOLDEN_VERSION)) == 24
    assert readers.masked_crc32c(struct.pack("<Q", 24)) == 0x224B7FA3
    # a file written with a fixed clock: the framed records, byte for byte
    with S.SummaryWriter(str(tmp_path), clock=lambda: 1.5, limits=[-1.0, 0.5, 2.5]) as w:
        w.add_scalar("a", 0.5, 10)
        w.clock = lambda: 2.0
        w.add_histogram_raw("h", [-1.0, 2.0, 3.0, 1.5, 5.25], [1, 1, 1], 3)
        path = w.path
    import socket
    assert os.path.basename(path) == "events.out.tfevents.0000000001." + socket.gethostname()
    assert os.listdir(str(tmp_path)) == [os.path.basename(path)]
    want = b"".join(_frame(bytes.fromhex(h)) for h in (GOLDEN_VERSION, GOLDEN_SCALAR, GOLDEN_HISTO))
    assert open(path, "rb").read() == want
    assert open(path, "rb").read()[8:12] == struct.pack("<I", 0x224B7FA3)
    with S.SummaryWriter(str(tmp_path / "sfx"), filename_suffix=".x", clock=lambda: 12345678901.25) as w2:
        assert os.path.basename(w2.path) == "events.out.tfevents.12345678901." + socket.gethostname() + ".x"
    with pytest.raises(ValueError):
        w2.add_scalar("a", 1.0, 1)


# ---- an independent decoder --------------------------------------------------------------------------------------------------------
def _proto_classes():
    from google.protobuf import descriptor_pb2, descriptor_pool
    try:
        from google.protobuf import message_factory
        get_class = getattr(message_factory, "GetMessageClass", None)
    except ImportError:                                            # pragma: no cover
        get_class = None
    F = descriptor_pb2.FieldDescriptorProto
    fd = descriptor_pb2.FileDescriptorProto(name="lpm_test_event.proto", package="lpmtest", syntax="proto3")

    def message(name, fields, oneof=None):
        m = fd.message_type.add(name=name)
        if oneof:
            m.oneof_decl.add(name=oneof)
        for fname, num, typ, label, type_name, in_oneof in fields:
            f = m.field.add(name=fname, number=num, type=typ, label=label)
            if type_name:
                f.type_name = ".lpmtest." + type_name
            if in_oneof:
                f.oneof_index = 0
        return m
    OPT, REP = F.LABEL_OPTIONAL, F.LABEL_REPEATED
    message("HistogramProto", [("min", 1, F.TYPE_DOUBLE, OPT, None, False), ("max", 2, F.TYPE_DOUBLE, OPT, None, False),
                               ("num", 3, F.TYPE_DOUBLE, OPT, None, False), ("sum", 4, F.TYPE_DOUBLE, OPT, None, False),
                               ("sum_squares", 5, F.TYPE_DOUBLE, OPT, None, False), ("bucket_limit", 6, F.TYPE_DOUBLE, REP, None, False),
                               ("bucket", 7, F.TYPE_DOUBLE, REP, None, False)])
    message("Value", [("tag", 1, F.TYPE_STRING, OPT, None, False), ("simple_value", 2, F.TYPE_FLOAT, OPT, None, True),
                      ("histo", 5, F.TYPE_MESSAGE, OPT, "HistogramProto", True)], oneof="value")
    message("Summary", [("value", 1, F.TYPE_MESSAGE, REP, "Value", False)])
    message("Event", [("wall_time", 1, F.TYPE_DOUBLE, OPT, None, False), ("step", 2, F.TYPE_INT64, OPT, None, False),
                      ("file_version", 3, F.TYPE_STRING, OPT, None, True), ("summary", 5, F.TYPE_MESSAGE, OPT, "Summary", True)],
            oneof="what")
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fd)
    desc = pool.FindMessageTypeByName("lpmtest.Event")
    if get_class is not None:
        return get_class(desc)
    return message_factory.MessageFactory(pool).GetPrototype(desc)   # pragma: no cover  (older runtimes)


def test_protobuf_parses_what_the_writer_wrote(tmp_path):
    pytest.importorskip("google.protobuf")
    from learnablepoolingmethods_amd import readers, summaries as S
    Event = _proto_classes()
    # the golden bytes are what protobuf itself serialises
    e = Event(wall_time=1.5, step=10)
    v = e.summary.value.add(tag="a")
    v.simple_value = 0.5
    assert e.SerializeToString().hex() == GOLDEN_SCALAR
    assert Event(wall_time=1.5, file_version="brain.Event:2").SerializeToString().hex() == GOLDEN_VERSION

    rng = np.random.default_rng(0)
    data = (rng.standard_normal(1000) * 0.05).astype(np.float32)
    with S.SummaryWriter(str(tmp_path), clock=lambda: 7.25) as w:
        w.add_scalar("loss", 0.125, 4)
        w.add_scalars({"x": 1.0, "y": -2.5}, 5)
        w.add_histogram("weights", data, 6)
        w.add_scalar("zero", 0.0, 0)
        path = w.path
    events = [Event.FromString(r) for r in readers.read_tfrecord(path, verify_crc=True)]
    assert len(events) == 5
    assert events[0].file_version == "brain.Event:2" and events[0].wall_time == 7.25 and events[0].WhichOneof("what") == "file_version"
    assert events[1].step == 4 and [(x.tag, x.simple_value) for x in events[1].summary.value] == [("loss", 0.125)]
    assert events[2].step == 5 and [(x.tag, x.simple_value) for x in events[2].summary.value] == [("x", 1.0), ("y", -2.5)]
    h = events[3].summary.value[0]
    assert events[3].step == 6 and h.tag == "weights" and h.WhichOneof("value") == "histo"
    d = data.astype(np.float64)
    assert (h.histo.min, h.histo.max, h.histo.num) == (d.min(), d.max(), 1000.0)
    assert h.histo.sum == pytest.approx(d.sum(), rel=1e-12) and h.histo.sum_squares == pytest.approx((d * d).sum(), rel=1e-12)
    lim = np.asarray(S.default_bucket_limits())
    want = np.bincount(np.searchsorted(lim, d, side="right"), minlength=lim.size)
    got = np.zeros(lim.size)
    got[np.searchsorted(lim, list(h.histo.bucket_limit))] = list(h.histo.bucket)
    assert np.array_equal(got, want) and sum(h.histo.bucket) == 1000
    assert events[4].step == 0 and events[4].summary.value[0].WhichOneof("value") == "simple_value"


# ---- bucket limits and the run rule ------------------------------------------------------------------------------------------------
def test_default_bucket_limits_and_bucket_indices():
    from learnablepoolingmethods_amd import summaries as S
    lim = S.default_bucket_limits()
    assert len(lim) == 1551 and lim == sorted(lim) and len(set(lim)) == 1551
    assert lim[776] == 1e-12 and lim[777] == 1.1000000000000002e-12 and lim[775] == 0.0 and lim[774] == -1e-12
    assert lim[-1] == DBL_MAX and lim[0] == -DBL_MAX and lim[-2] == 9.920775621859783e+19
    assert [x for x in lim if abs(x) < 1e300 and float(np.float32(x)) == x] == [0.0], "only 0.0 is an fp32 value"
    for value, bucket in ((0.0, 776), (-0.0, 776), (1e-13, 776), (-1e-13, 775), (1.0, 1066), (-1.0, 485), (0.05, 1035), (3.4e38, 1550)):
        v = float(np.float32(value))
        assert int(np.searchsorted(lim, v, side="right")) == bucket, value
        stats, counts, bad = S.histogram_numpy(np.array([value], dtype=np.float32))
        assert bad == 0 and counts[bucket] == 1 and counts.sum() == 1, value


def _pairs(blob):
    from learnablepoolingmethods_amd import summaries as S
    h = S._decode_histogram(blob)
    return list(zip(h["bucket_limit"], h["bucket"]))


def test_encode_histogram_collapses_runs_of_empty_buckets():
    from learnablepoolingmethods_amd import summaries as S
    lim = [float(i) for i in range(1, 11)]
    stats = [0.0] * 5
    #                 leading run        inner run         trailing run
    counts = [0, 0, 0, 4, 5, 0, 0, 7, 0, 0]
    assert _pairs(S.encode_histogram(stats, counts, lim)) == [(3.0, 0.0), (4.0, 4.0), (5.0, 5.0), (7.0, 0.0), (8.0, 7.0), (10.0, 0.0)]
    assert _pairs(S.encode_histogram(stats, [1] + [0] * 8 + [2], lim)) == [(1.0, 1.0), (9.0, 0.0), (10.0, 2.0)]
    assert _pairs(S.encode_histogram(stats, [0, 1, 0, 1, 0, 1, 0, 1, 0, 1], lim)) == [(float(i), float(i % 2 == 0)) for i in range(1, 11)]
    # all empty: one pair, (DBL_MAX, 0) -- with the default limits the run's last limit IS DBL_MAX; with no buckets it is the fallback
    assert _pairs(S.encode_histogram(stats, np.zeros(1551))) == [(DBL_MAX, 0.0)]
    assert _pairs(S.encode_histogram(stats, [], [])) == [(DBL_MAX, 0.0)]
    with pytest.raises(ValueError):
        S.encode_histogram(stats, [1, 2], lim)


# ---- the numpy path, read_events -----------------------------------------------------------------------------------------------------
def test_cpu_histograms_round_trip_and_crc(tmp_path, caplog):
    from learnablepoolingmethods_amd import summaries as S
    rng = np.random.default_rng(1)
    a = np.concatenate([rng.standard_normal(777) * 0.05, [0.0, -0.0, 1e-45, 3.4028235e38, -3.4028235e38, 1.0, -1.0]]).astype(np.float32)
    t = torch.from_numpy(rng.standard_normal((5, 7)).astype(np.float32))
    bad = np.array([1.0, np.nan, np.inf, -np.inf, 2.0], dtype=np.float32)
    with S.SummaryWriter(str(tmp_path), clock=lambda: 3.0) as w:
        w.add_scalar("s", 0.25, 1)
        w.add_histogram("a", a, 2)
        w.add_histogram("t", t, 3)
        with caplog.at_level(logging.WARNING):
            w.add_histogram("bad", bad, 4)
            w.add_histogram("bad", bad, 5)
        path = w.path
    assert [r.getMessage() for r in caplog.records if "non-finite" in r.getMessage()] == \
        ["summary 'bad': 3 non-finite values left out of the histogram"], "one warning per tag, naming the count"
    ev = list(S.read_events(path))
    assert [e["step"] for e in ev] == [0, 1, 2, 3, 4, 5] and ev[0]["file_version"] == "brain.Event:2" and ev[0]["values"] == []
    assert all(e["wall_time"] == 3.0 for e in ev)
    assert ev[1]["values"] == [("s", 0.25)]
    lim = np.asarray(S.default_bucket_limits())
    for e, (tag, arr) in zip(ev[2:4], (("a", a), ("t", t.numpy()))):
        (got_tag, h), = e["values"]
        d = arr.astype(np.float64).reshape(-1)                                           # the test's own reference
        counts = np.bincount(np.searchsorted(lim, d, side="right"), minlength=lim.size)
        stats = [d.min(), d.max(), float(d.size), d.sum(), (d * d).sum()]
        assert got_tag == tag and np.array_equal(S.expand_histogram(h), counts)
        assert [h["min"], h["max"], h["num"]] == stats[:3]
        assert h["sum"] == pytest.approx(stats[3], rel=1e-12, abs=1e-300) and h["sum_squares"] == pytest.approx(stats[4], rel=1e-12)
    for e in ev[4:]:
        (_, h), = e["values"]
        assert (h["min"], h["max"], h["num"], h["sum"], h["sum_squares"]) == (1.0, 2.0, 2.0, 3.0, 5.0)
    with pytest.raises(ValueError, match="3 non-finite"), S.SummaryWriter(str(tmp_path / "strict"), strict=True) as ws:
        ws.add_histogram("bad", bad, 1)
    # a flipped payload byte
    raw = bytearray(open(path, "rb").read())
    raw[12 + 24 + 4 + 12 + 3] ^= 0x40                                                    # inside the second record's payload
    broken = str(tmp_path / "broken")
    open(broken, "wb").write(bytes(raw))
    with pytest.raises(IOError):
        list(S.read_events(broken))
    raw = bytearray(open(path, "rb").read())
    raw[1] ^= 1                                                                          # the first record's length
    open(broken, "wb").write(bytes(raw))
    with pytest.raises(IOError):
        list(S.read_events(broken))


def test_add_input_on_the_host_equals_the_histogram_of_the_dequantised_padded_batch(tmp_path):
    from learnablepoolingmethods_amd import ops, summaries as S, utils
    rng = np.random.default_rng(2)
    q = torch.from_numpy(rng.integers(0, 256, size=(3, 7, 12), dtype=np.uint8))
    nf = torch.tensor([0, 3, 7], dtype=torch.int32)
    with S.SummaryWriter(str(tmp_path)) as w:
        w.add_input(q, nf, 9)
        path = w.path
    (tag, h), = list(S.read_events(path))[1]["values"]
    x = utils.Dequantize(q.to(torch.float32), ops.QUANT_MAX, ops.QUANT_MIN)
    x = x * (torch.arange(7)[None, :, None] < nf[:, None, None])
    d = x.numpy().astype(np.float64).reshape(-1)
    lim = np.asarray(S.default_bucket_limits())
    assert tag == "model/input_raw" and h["num"] == d.size == 252 and h["min"] == d.min() and h["max"] == d.max()
    assert np.array_equal(S.expand_histogram(h), np.bincount(np.searchsorted(lim, d, side="right"), minlength=lim.size))
    assert h["sum"] == pytest.approx(d.sum(), rel=1e-12, abs=1e-12) and h["sum_squares"] == pytest.approx((d * d).sum(), rel=1e-12)


# ---- the C ABI and the refusals that need no GPU ---------------------------------------------------------------------------------------
def test_histogram_entry_points_are_declared_exported_and_bound():
    from learnablepoolingmethods_amd import _build, _capi
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    if not os.path.exists(_capi.LIB_PATH):
        _build.build(verbose=False)
    dll = ctypes.CDLL(_capi.LIB_PATH)
    for name in ("lpm_histogram_segments", "lpm_histogram_segments_workspace_bytes", "lpm_histogram_frames_q8"):
        assert re.search(r"\b" + name + r"\s*\(", txt), f"{name} not declared in lpm_hip.h"
        assert hasattr(dll, name), f"{name} not exported"
        assert name in _capi.SIGNATURES
    lib = _capi.load()
    assert lib._lpm_histogram_segments_workspace_bytes(0, 10) == 0
    small, big = lib._lpm_histogram_segments_workspace_bytes(3, 10), lib._lpm_histogram_segments_workspace_bytes(3, 10 ** 9)
    assert 0 < small < big


def test_histogram_ops_refuse_cpu_tensors(monkeypatch):
    from learnablepoolingmethods_amd import _capi, ops

    def refuse(*a, **k):
        raise AssertionError("the library was reached: the argument check came too late")
    monkeypatch.setattr(_capi, "load", refuse)
    with pytest.raises(_capi.LpmError):
        ops.histogram_segments(torch.zeros(10))
    with pytest.raises(_capi.LpmError):
        ops.histogram_frames_q8(torch.zeros(2, 3, 4, dtype=torch.uint8), torch.tensor([1, 2]))
    meta = torch.empty(100, device="meta")
    with pytest.raises(_capi.LpmError):
        ops.histogram_segments(meta.double())


# ---- the run loop ----------------------------------------------------------------------------------------------------------------------
V, MF = 12, 6
FULL = dict(num_classes=V, feature_sizes=(1024, 128), feature_names=("rgb", "audio"), max_frames=MF)
LOG_LINE = re.compile(r"^training step (\d+) \| Loss: (-?\d+\.\d\d) Examples/sec: (\d+\.\d\d) \| Hit@1: (\d\.\d\d) PERR: (\d\.\d\d) GAP: (\d\.\d\d)$")
SCALAR_TAGS = ["model/Training_Hit@1", "model/Training_Perr", "model/Training_GAP", "global_step/Examples/Second", "label_loss",
               "learning_rate"]


class ToyTrainer:
    """tests/test_training_host.py's stand-in (the interface training.run uses, around a logistic layer on the mean frame), with the
    learning-rate schedule of train.learning_rate in its step's dict."""
    num_towers = 1
    BASE_LR, DECAY, DECAY_EXAMPLES = 0.5, 0.5, 16

    def __init__(self, seed=3):
        self.device, self.seed = torch.device("cpu"), seed
        self.global_step, self.arena = 0, None

    def build(self, frames, num_frames, labels):
        if self.arena is None:
            g = torch.Generator().manual_seed(self.seed)
            self.w = 0.05 * torch.randn(frames.shape[2], labels.shape[1], generator=g)
            self.b = torch.zeros(labels.shape[1])
            self.arena = object()

    def step(self, frames, num_frames, labels):
        from learnablepoolingmethods_amd import losses
        from learnablepoolingmethods_amd.train import learning_rate, normalize_input
        self.build(frames, num_frames, labels)
        lr = learning_rate(self.BASE_LR, self.global_step, frames.shape[0], 1, self.DECAY_EXAMPLES, self.DECAY)
        w, b = self.w.clone().requires_grad_(), self.b.clone().requires_grad_()
        pooled = normalize_input(frames, num_frames).sum(1) / num_frames.clamp_min(1).view(-1, 1).float()
        p = torch.sigmoid(pooled.matmul(w) + b)
        loss = losses.CrossEntropyLoss().calculate_loss(p, labels.float())
        gw, gb = torch.autograd.grad(loss, [w, b])
        self.w, self.b = self.w - lr * gw, self.b - lr * gb
        self.global_step += 1
        return {"loss": loss.detach(), "predictions": p.detach(), "global_step": self.global_step, "learning_rate": lr}

    def state_dict(self):
        return {"w": self.w, "b": self.b, "global_step": self.global_step}

    def save(self, path):
        torch.save(self.state_dict(), path)

    def restore(self, path):
        state = torch.load(path, map_location="cpu")
        self.w, self.b, self.global_step = state["w"], state["b"], int(state["global_step"])


def _files(tmp_path, n_files=2, per_file=10):
    from learnablepoolingmethods_amd import readers
    rng = np.random.default_rng(7)
    files, k = [], 0
    for f in range(n_files):
        recs = []
        for _ in range(per_file):
            n = int(rng.integers(1, MF + 2))
            feats = {"rgb": rng.integers(0, 256, size=(n, 1024), dtype=np.uint8), "audio": rng.integers(0, 256, size=(n, 128), dtype=np.uint8)}
            recs.append(readers.make_sequence_example(f"clip{k}", sorted(set(rng.integers(0, V, size=2).tolist())), feats))
            k += 1
        path = str(tmp_path / f"train{f}.tfrecord")
        readers.write_tfrecord(path, recs)
        files.append(path)
    return files


def test_run_writes_the_scalars_of_the_logged_steps_and_histograms_on_the_cadence(tmp_path):
    from learnablepoolingmethods_amd import readers, summaries as S, training
    from learnablepoolingmethods_amd.train import learning_rate
    files = _files(tmp_path)
    reader = readers.YT8MFrameFeatureReader(**FULL)

    def batches():
        return reader.training_batches(files, 4, device="cpu", num_epochs=None, seed=11)
    lines = []
    sdir, tdir = str(tmp_path / "events"), str(tmp_path / "model")
    tr = ToyTrainer()
    w = S.SummaryWriter(sdir)
    it = batches()
    out = training.run(tr, it, max_steps=13, log_every=2, train_dir=tdir, log=lines.append, summary_writer=w, histogram_steps=4)
    it.close()
    w.close()
    assert out["global_step"] == 13
    ev = list(S.read_events(w.path))
    assert ev[0]["file_version"] == "brain.Event:2"
    scalars = [e for e in ev[1:] if all(isinstance(v, float) for _, v in e["values"])]
    histos = [e for e in ev[1:] if e not in scalars]
    assert [e["step"] for e in scalars] == [2, 4, 6, 8, 10, 12]
    logged = [LOG_LINE.match(l) for l in lines if l.startswith("training step")]
    assert len(logged) == 6 and all(logged)
    for e, m in zip(scalars, logged):
        got = dict(e["values"])
        assert list(got) == SCALAR_TAGS and int(m.group(1)) == e["step"]
        # the values the log line was formatted from
        assert "%.2f" % got["label_loss"] == m.group(2) and "%.2f" % got["global_step/Examples/Second"] == m.group(3)
        assert "%.2f" % got["model/Training_Hit@1"] == m.group(4) and "%.2f" % got["model/Training_Perr"] == m.group(5)
        assert "%.2f" % got["model/Training_GAP"] == m.group(6)
        want_lr = learning_rate(ToyTrainer.BASE_LR, e["step"] - 1, 4, 1, ToyTrainer.DECAY_EXAMPLES, ToyTrainer.DECAY)
        assert got["learning_rate"] == float(np.float32(want_lr))
    assert len({dict(e["values"])["learning_rate"] for e in scalars}) > 1, "the schedule decays within the run"
    # histograms: first logged step, then every logged step at which 4 steps have passed: 2, 6, 10
    steps = sorted({e["step"] for e in histos})
    assert steps == [2, 6, 10]
    for s in steps:
        tags = [t for e in histos if e["step"] == s for t, _ in e["values"]]
        assert tags == ["w", "b", "model/input_raw"]
    h = dict(v for e in histos if e["step"] == 2 for v in e["values"])
    assert h["w"]["num"] == 1152 * V and h["b"]["num"] == V and h["model/input_raw"]["num"] == 4 * MF * 1152
    assert not [t for t in threading.enumerate() if t.name.startswith("lpm-")]
    # the event file is the writer's business alone: train_dir holds checkpoints only
    assert sorted(os.listdir(tdir)) == ["model.ckpt-13.pt", "model.ckpt-2.pt"]
    assert len(os.listdir(sdir)) == 1 and os.listdir(sdir)[0].startswith("events.out.tfevents.")


def test_run_without_a_writer_leaves_what_it_left_before_and_the_same_state(tmp_path):
    from learnablepoolingmethods_amd import readers, summaries as S, training
    files = _files(tmp_path)
    reader = readers.YT8MFrameFeatureReader(**FULL)
    states = []
    for with_writer in (False, True):
        tdir = str(tmp_path / f"model{int(with_writer)}")
        tr = ToyTrainer()
        it = reader.training_batches(files, 4, device="cpu", num_epochs=None, seed=11)
        w = S.SummaryWriter(tdir) if with_writer else None               # (the summary directory may be train_dir)
        training.run(tr, it, max_steps=5, log_every=2, train_dir=tdir, log=lambda s: None, summary_writer=w, histogram_steps=2)
        it.close()
        names = sorted(os.listdir(tdir))
        if with_writer:
            w.close()
            assert [n for n in names if n.startswith("model.ckpt")] == ["model.ckpt-2.pt", "model.ckpt-5.pt"] and len(names) == 3
        else:
            assert names == ["model.ckpt-2.pt", "model.ckpt-5.pt"]
        states.append(tr.state_dict())
    assert torch.equal(states[0]["w"], states[1]["w"]) and torch.equal(states[0]["b"], states[1]["b"])
    with pytest.raises(ValueError):
        training.run(ToyTrainer(), iter(()), histogram_steps=0)


def test_command_line_has_the_summary_flags():
    from learnablepoolingmethods_amd import training
    args = training._parser().parse_args([])
    assert args.summary_dir == "" and args.histogram_steps == 1000
    args = training._parser().parse_args(["--summary_dir", "d", "--histogram_steps", "50"])
    assert args.summary_dir == "d" and args.histogram_steps == 50


# ---- evaluation ------------------------------------------------------------------------------------------------------------------------
def test_evaluate_writes_the_epoch_tags(tmp_path):
    from learnablepoolingmethods_amd import evaluation, summaries as S
    g = torch.Generator().manual_seed(0)

    class Model:
        vocab_size = 10

        def predict(self, frames, num_frames):
            return torch.sigmoid(frames.float().mean(1)[:, :10] / 64.0 - 2.0)
    batches = [(None, torch.randint(0, 256, (4, 5, 16), generator=g, dtype=torch.uint8), torch.rand(4, 10, generator=g) < 0.3,
                torch.full((4,), 5)) for _ in range(3)]
    with S.SummaryWriter(str(tmp_path / "a")) as w:
        info = evaluation.evaluate(Model(), batches, summary_writer=w, global_step=7)
        path = w.path
    ev = list(S.read_events(path))
    assert len(ev) == 2 and ev[1]["step"] == 7
    want = {"Epoch/Eval_Avg_Hit@1": info["avg_hit_at_one"], "Epoch/Eval_Avg_Perr": info["avg_perr"], "Epoch/Eval_Avg_Loss": info["avg_loss"],
            "Epoch/Eval_MAP": info["map"], "Epoch/Eval_GAP": info["gap"]}
    assert [t for t, _ in ev[1]["values"]] == list(want)
    assert {t: v for t, v in ev[1]["values"]} == {t: float(np.float32(v)) for t, v in want.items()}
    # both arguments are needed
    with S.SummaryWriter(str(tmp_path / "b")) as w:
        evaluation.evaluate(Model(), batches, summary_writer=w)
        path = w.path
    assert len(list(S.read_events(path))) == 1
