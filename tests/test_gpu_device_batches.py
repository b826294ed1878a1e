"""-m gpu: YT8MFrameFeatureReader.device_batches (pinned ring -> native indexer -> lpm_gather_frames / lpm_labels_dense) against
batches(), the pure-Python route, moved to the device.  Every comparison is torch.equal: the bytes are copied, not computed."""
import threading

import numpy as np
import pytest
import torch

from learnablepoolingmethods_amd import FLAGS, evaluation, ops, readers, registry
from learnablepoolingmethods_amd._capi import LpmError
from learnablepoolingmethods_amd.predictor import Predictor
from learnablepoolingmethods_amd.train import Trainer

from tests._util import cuda

pytestmark = pytest.mark.gpu


def _write(path, rng, frame_counts, num_classes, sizes=(1024, 128), names=("rgb", "audio"), first=0):
    recs = []
    for i, n in enumerate(frame_counts):
        labels = rng.integers(0, num_classes + 3, size=int(rng.integers(0, 6))).tolist()          # some at and above num_classes
        if i % 3 == 0 and labels:
            labels.append(labels[0])                                                               # a repeated label
        feats = {nm: rng.integers(0, 256, size=(n, s), dtype=np.uint8) for nm, s in zip(names, sizes)}
        recs.append(readers.make_sequence_example(f"clip{first + i}", labels, feats))
    readers.write_tfrecord(str(path), recs)
    return str(path)


def _same(dev_batches, host_batches, dev):
    dev_batches, host_batches = list(dev_batches), list(host_batches)
    assert len(dev_batches) == len(host_batches)
    for (ids, q, y, nf), (hids, hq, hy, hnf) in zip(dev_batches, host_batches):
        assert ids == hids
        assert q.is_cuda and q.dtype == torch.uint8 and y.dtype == torch.bool and nf.dtype == torch.int32
        assert q.is_contiguous() and y.is_contiguous()
        assert torch.equal(nf, hnf.to(dev))
        assert torch.equal(q, hq.to(dev)), "frames differ"
        assert torch.equal(y, hy.to(dev)), "labels differ"
    return len(dev_batches)


def _residues(reader, path):
    """The residues mod 16 of the rgb frame offsets of a file, from the indexer's table."""
    buf, offs, lens = readers.frame_file(path)
    idx = readers.locate_records(buf, offs, lens, reader.feature_names, reader.feature_sizes, reader.max_frames, reader.num_classes)
    o = idx.frame_offset[:, 0, :]
    return set((o[o >= 0] % 16).tolist())


@pytest.mark.parametrize("drop_remainder", [False, True])
def test_two_files_batch_across_the_boundary(tmp_path, drop_remainder):
    dev = cuda()
    rng = np.random.default_rng(21)
    reader = readers.YT8MFrameFeatureReader(num_classes=10, max_frames=9)
    files = [_write(tmp_path / "a.tfrecord", rng, [5, 9, 12, 1, 0], 10), _write(tmp_path / "b.tfrecord", rng, [12, 9, 5, 3, 9, 12, 7], 10, first=5)]
    n = _same(reader.device_batches(files, 4, device=dev, drop_remainder=drop_remainder, verify_crc=True),
              reader.batches(files, 4, drop_remainder=drop_remainder), dev)
    assert n == 3                                                 # 12 clips: three full batches, the second across the boundary
    files.append(_write(tmp_path / "c.tfrecord", rng, [4, 4], 10, first=12))
    n = _same(reader.device_batches(files, 4, device=dev, drop_remainder=drop_remainder), reader.batches(files, 4, drop_remainder=drop_remainder), dev)
    assert n == (3 if drop_remainder else 4)


def test_full_shape_and_all_source_alignments(tmp_path):
    dev = cuda()
    rng = np.random.default_rng(22)
    counts = [120, 300, 299] + rng.integers(120, 301, size=21).tolist()
    for V in (3862, 10):
        reader = readers.YT8MFrameFeatureReader(num_classes=V, max_frames=300)
        path = _write(tmp_path / f"full{V}.tfrecord", rng, counts if V == 3862 else counts[:5], V)
        assert _residues(reader, path) == set(range(16)), "the rgb sources must cover every residue mod 16"
        assert _same(reader.device_batches([path], 8, device=dev), reader.batches([path], 8), dev) == (3 if V == 3862 else 1)
        if V == 3862:
            rgb = readers.YT8MFrameFeatureReader(num_classes=V, feature_sizes=(1024,), feature_names=("rgb",), max_frames=300)
            _same(rgb.device_batches([path], 16, device=dev, reader_threads=2), rgb.batches([path], 16), dev)
            audio_first = readers.YT8MFrameFeatureReader(num_classes=V, feature_sizes=(128, 1024), feature_names=("audio", "rgb"), max_frames=40)
            _same(audio_first.device_batches([path], 5, device=dev), audio_first.batches([path], 5), dev)


def test_feature_sizes_that_are_multiples_of_4_only(tmp_path):
    """Rows of 20 + 12 bytes: the 16 destination bytes of a lane straddle features and rows (the dword route); 6 is refused."""
    dev = cuda()
    rng = np.random.default_rng(23)
    reader = readers.YT8MFrameFeatureReader(num_classes=7, feature_sizes=(20, 12), feature_names=("a", "b"), max_frames=11)
    path = _write(tmp_path / "odd.tfrecord", rng, [11, 3, 0, 14, 7], 7, sizes=(20, 12), names=("a", "b"))
    _same(reader.device_batches([path], 3, device=dev), reader.batches([path], 3), dev)
    one = readers.YT8MFrameFeatureReader(num_classes=7, feature_sizes=(20,), feature_names=("a",), max_frames=3)      # 60-byte clips, 180 in all
    _same(one.device_batches([path], 3, device=dev), one.batches([path], 3), dev)
    bad = readers.YT8MFrameFeatureReader(num_classes=7, feature_sizes=(6,), feature_names=("a",), max_frames=3)
    with pytest.raises(LpmError):
        next(bad.device_batches([path], 3, device=dev))
    with pytest.raises(LpmError):
        ops.gather_frames(torch.zeros(64, dtype=torch.uint8, device=dev), 40, torch.zeros((1, 1, 3), dtype=torch.int64, device=dev),
                          torch.ones(1, dtype=torch.int32, device=dev), (6,), 3)
    with pytest.raises(LpmError):
        ops.gather_frames(torch.zeros(64, dtype=torch.uint8), 40, torch.zeros((1, 1, 3), dtype=torch.int64), torch.ones(1, dtype=torch.int32), (8,), 3)


def test_gather_refuses_to_read_outside_the_records():
    """Offsets that do not lie inside the uploaded bytes give zeros (and no fault): the kernel checks every source range."""
    dev = cuda()
    raw = torch.arange(48, dtype=torch.uint8, device=dev)                       # 40 bytes of records in a 48-byte allocation
    off = torch.tensor([[[0, 33, 32, -1, 1 << 40]]], dtype=torch.int64, device=dev)
    out = ops.gather_frames(raw, 40, off, torch.tensor([5], dtype=torch.int32, device=dev), (8,), 5)
    want = torch.zeros((1, 5, 8), dtype=torch.uint8)
    want[0, 0] = torch.arange(0, 8)
    want[0, 2] = torch.arange(32, 40)                                           # 33 + 8 > 40: refused; 32 + 8 == 40: the last frame
    assert torch.equal(out.cpu(), want)
    y = ops.labels_dense(torch.tensor([0, 0, 3], dtype=torch.int32, device=dev), torch.tensor([4, 4, 0], dtype=torch.int32, device=dev), 5)
    assert y.dtype == torch.bool and y.cpu().tolist() == [[False] * 5, [True, False, False, False, True]]


def test_batches_stay_intact_while_later_ones_are_produced(tmp_path):
    """All batches collected first, compared afterwards, with the smallest ring: a slot or staging buffer reused too early shows."""
    dev = cuda()
    rng = np.random.default_rng(24)
    reader = readers.YT8MFrameFeatureReader(num_classes=12, max_frames=30)
    path = _write(tmp_path / "ring.tfrecord", rng, rng.integers(0, 40, size=27).tolist(), 12)
    got = list(reader.device_batches([path], 3, device=dev, prefetch=1))
    assert len(got) == 9                                                        # the ring has two slots
    torch.cuda.synchronize()
    _same(got, reader.batches([path], 3), dev)
    # a consumer on a stream of its own
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        got = [(ids, q.clone(), y.clone(), nf.clone()) for ids, q, y, nf in reader.device_batches([path], 4, device=dev, prefetch=1)]
    s.synchronize()
    _same(got, reader.batches([path], 4), dev)


def _small_trainer(dev, V, B):
    return Trainer(registry.get_model("NetVladV1"), vocab_size=V, batch_size=B, base_learning_rate=1e-3, device=dev, seed=3,
                   model_kwargs=dict(iterations=16, cluster_size=32, hidden_size=32))


def test_predictor_and_evaluate_over_both_routes(tmp_path):
    dev = cuda()
    rng = np.random.default_rng(25)
    V, B, MF = 30, 6, 40
    reader = readers.YT8MFrameFeatureReader(num_classes=V, max_frames=MF)
    path = _write(tmp_path / "p.tfrecord", rng, [int(rng.integers(1, 50)) for _ in range(15)], V)
    try:
        tr = _small_trainer(dev, V, B)
        (_, q, y, nf) = next(reader.batches([path], B))
        tr.step(q, nf, y.float())
        pr = Predictor.from_trainer(tr)
        for (ids, dq, dy, dnf), (hids, hq, hy, hnf) in zip(reader.device_batches([path], B, device=dev), reader.batches([path], B)):
            assert torch.equal(pr.predict(dq, dnf), pr.predict(hq.cuda(), hnf.cuda()))
        a = evaluation.evaluate(pr, reader.device_batches([path], B, device=dev), top_k=5)
        b = evaluation.evaluate(pr, reader.batches([path], B), top_k=5)
    finally:
        FLAGS.reset()
    a.pop("examples_per_second"), b.pop("examples_per_second")
    assert a["num_examples"] == 15 and sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64), equal_nan=True), k


def test_trainer_steps_from_both_routes_are_bit_identical(tmp_path):
    dev = cuda()
    rng = np.random.default_rng(26)
    V, B, MF = 30, 6, 40
    reader = readers.YT8MFrameFeatureReader(num_classes=V, max_frames=MF)
    path = _write(tmp_path / "t.tfrecord", rng, [int(rng.integers(1, 50)) for _ in range(12)], V)
    try:
        losses = []
        for route in ("device", "host"):
            tr = _small_trainer(dev, V, B)
            it = reader.device_batches([path], B, device=dev) if route == "device" else reader.batches([path], B)
            losses.append([tr.step(q, nf, y)["loss"].detach().clone() for _, q, y, nf in it])      # the bool labels as they are
    finally:
        FLAGS.reset()
    assert len(losses[0]) == 2
    for a, b in zip(*losses):
        assert torch.equal(a, b)


def _pipeline_threads():
    return [t for t in threading.enumerate() if t.name.startswith("lpm-")]


def test_errors_arrive_at_their_batch_and_the_thread_ends(tmp_path):
    dev = cuda()
    rng = np.random.default_rng(27)
    reader = readers.YT8MFrameFeatureReader(num_classes=10, max_frames=9)
    good = _write(tmp_path / "good.tfrecord", rng, [3, 9, 12, 5, 1, 2, 7, 8, 4], 10)
    data = bytearray(open(good, "rb").read())
    buf, offs, lens = readers.frame_file(good)
    idx = readers.locate_records(buf, offs, lens, max_frames=9, num_classes=10)
    # a corrupt record in the second of three batches: clip 4's audio loses a frame (ValueError) / a payload byte flips (IOError with CRC)
    rgb = rng.integers(0, 256, size=(4, 1024), dtype=np.uint8)
    uneven = readers.make_sequence_example("uneven", [1], {"rgb": rgb, "audio": rgb[:3, :128]})
    recs = list(readers.read_tfrecord(good))
    recs[4] = uneven
    bad_example = str(tmp_path / "bad_example.tfrecord")
    readers.write_tfrecord(bad_example, recs)
    data[int(idx.frame_offset[3, 0, 1]) + 17] ^= 0x40
    bad_crc = str(tmp_path / "bad_crc.tfrecord")
    open(bad_crc, "wb").write(bytes(data))
    truncated = str(tmp_path / "truncated.tfrecord")
    open(truncated, "wb").write(bytes(open(good, "rb").read()[:int(offs[5]) + 100]))
    first = next(reader.batches([good], 3))
    for path, kw, exc, name in ((bad_example, {}, ValueError, "record 4"), (bad_crc, dict(verify_crc=True), IOError, "record 3"),
                                (truncated, {}, IOError, "record 5")):
        it = reader.device_batches([path], 3, device=dev, **kw)
        _same([next(it)], [first], dev)
        with pytest.raises(exc, match=name):
            next(it)
        assert not _pipeline_threads(), "the reader thread must be gone after the error"
        with pytest.raises(exc):
            list(reader.batches([path], 3, **kw))                              # the Python route raises the same type
    # without verify_crc the flipped byte is data, on both routes
    _same(reader.device_batches([bad_crc], 3, device=dev), reader.batches([bad_crc], 3), dev)
    # closing early joins the thread; a new pipeline works in the same process
    it = reader.device_batches([good, good, good], 2, device=dev, prefetch=1)
    next(it)
    assert _pipeline_threads()
    it.close()
    assert not _pipeline_threads()
    _same(reader.device_batches([good], 3, device=dev), reader.batches([good], 3), dev)
    with pytest.raises(IOError):
        list(reader.device_batches([str(tmp_path / "missing.tfrecord")], 3, device=dev))
    with pytest.raises(LpmError):
        next(reader.device_batches([good], 3, device="cpu"))


def test_a_slot_grows_for_records_longer_than_max_frames(tmp_path):
    dev = cuda()
    rng = np.random.default_rng(28)
    reader = readers.YT8MFrameFeatureReader(num_classes=10, max_frames=4)       # slots sized for 4-frame clips
    path = _write(tmp_path / "long.tfrecord", rng, [60, 2, 75, 4, 90, 1], 10)
    _same(reader.device_batches([path], 2, device=dev, prefetch=1), reader.batches([path], 2), dev)
    st = {}
    _same(reader.device_batches([path], 4, device=dev, stats=st), reader.batches([path], 4), dev)
    assert st["clips"] == 6 and st["batches"] == 2 and st["bytes"] == len(open(path, "rb").read())
