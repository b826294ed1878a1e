"""-m gpu: the histogram kernels and the TensorBoard writer on the device.  The yardstick is numpy in fp64 -- searchsorted(side="right")
over summaries.default_bucket_limits(), min, max, math.fsum -- never the code under test:

  * lpm_histogram_segments: counts, min, max, num and nonfinite exact; sum and sum_squares within n * 2^-52 * sum |terms|, the first-order
    bound of ANY order of n fp64 additions; two calls give the same bits.  One buffer holds segments of 1, 63, 64, 65, 257 and 5 000
    elements at offsets of every alignment (odd ones first) with gaps of a value that must not be counted, 5 000 identical values, the fp32
    neighbours of 64 bucket limits, zeros of both signs, the smallest denormals, +-FLT_MAX, a segment with NaN / +-Inf sprinkled in, and
    one of 300 001 elements (74 workgroups and the final reduction);
  * lpm_histogram_frames_q8: all 257 counts, and add_input's decoded histogram against numpy on the dequantised, zero-padded batch;
  * add_variables on a tiny NetVladV1 trainer: one histogram per store variable, each equal to numpy on state_dict()'s tensor;
  * twelve steps through training.run with a writer and twelve without: state_dict() bit-identical, histograms at steps 2, 6 and 10;
  * the refusals, before any launch."""
import math
import threading

import numpy as np
import pytest
import torch

from learnablepoolingmethods_amd import FLAGS, _capi, ops, registry, summaries as S, training, utils
from learnablepoolingmethods_amd.train import Trainer

from tests._util import cuda

pytestmark = [pytest.mark.gpu]

LIM = np.asarray(S.default_bucket_limits(), dtype=np.float64)
GAP_VALUE = 1234.5                     # what lies between the segments: lands in no count
FLT_MAX = float(np.finfo(np.float32).max)
DENORM = float(np.float32(1e-45))      # the smallest fp32 denormal


def _reference(v32):
    """numpy / fsum on one segment -> counts, stats, nonfinite, and the bound's sum |terms| for sum and sum_squares."""
    d = v32.astype(np.float64)
    finite = np.isfinite(d)
    bad = int((~finite).sum())
    d = d[finite]
    counts = np.bincount(np.searchsorted(LIM, d, side="right"), minlength=LIM.size)
    if d.size == 0:
        return counts, [S.DBL_MAX, -S.DBL_MAX, 0.0, 0.0, 0.0], bad, (0.0, 0.0)
    sq = d * d
    return counts, [d.min(), d.max(), float(d.size), math.fsum(d), math.fsum(sq)], bad, (math.fsum(np.abs(d)), math.fsum(sq))


def _segments():
    rng = np.random.default_rng(0)
    segs = [(rng.standard_normal(n) * 0.05).astype(np.float32) for n in (1, 63, 64, 65, 257, 5000)]
    segs.append(np.full(5000, 0.0371, dtype=np.float32))
    # the fp32 neighbours of 64 limits, 32 of either sign: float32(limit), two floats below it and two above
    pos = np.flatnonzero((LIM > 0) & (LIM < 1e38))
    neg = np.flatnonzero((LIM < 0) & (LIM > -1e38))
    chosen = np.concatenate([rng.choice(pos, 32, replace=False), rng.choice(neg, 32, replace=False)])
    near = []
    for f in LIM[chosen].astype(np.float32):
        lo1 = np.nextafter(f, np.float32(-np.inf))
        hi1 = np.nextafter(f, np.float32(np.inf))
        near += [np.nextafter(lo1, np.float32(-np.inf)), lo1, f, hi1, np.nextafter(hi1, np.float32(np.inf))]
    segs.append(np.array(near, dtype=np.float32))
    segs.append(np.array([0.0, -0.0, DENORM, -DENORM, FLT_MAX, -FLT_MAX, 1e-13, -1e-13, 1.0, -1.0, 0.05, 3.4e38], dtype=np.float32))
    bad = (rng.standard_normal(1000) * 0.05).astype(np.float32)
    bad[[0, 17, 500, 999]] = np.nan
    bad[[3, 640]] = np.inf
    bad[[64, 65, 66]] = -np.inf
    segs.append(bad)
    segs.append((rng.standard_normal(300001) * 0.05).astype(np.float32))
    residues = [1, 3, 2, 1, 3, 0, 1, 3, 2, 1, 3]                                   # start % 4: every alignment, odd ones first
    starts, cur = [], 1
    for s, r in zip(segs, residues):
        while cur % 4 != r:
            cur += 1
        starts.append(cur)
        cur += len(s) + 3
    buf = np.full(cur + 5, GAP_VALUE, dtype=np.float32)
    for s, a in zip(segs, starts):
        buf[a:a + len(s)] = s
    return buf, starts, segs


@pytest.fixture(scope="module")
def segment_case():
    buf, starts, segs = _segments()
    return buf, starts, segs, [_reference(s) for s in segs]


def test_histogram_segments_against_numpy(segment_case):
    dev = cuda()
    buf, starts, segs, refs = segment_case
    x = torch.from_numpy(buf).to(dev)
    lens = [len(s) for s in segs]
    h = ops.histogram_segments(x, starts, lens)
    h2 = ops.histogram_segments(x, torch.tensor(starts), torch.tensor(lens))
    assert h.counts.shape == (len(segs), LIM.size) and h.counts.dtype == torch.int64 and h.stats.dtype == torch.float64
    counts, stats, nonfinite = h.counts.cpu().numpy(), h.stats.cpu().numpy(), h.nonfinite.cpu().numpy()
    for i, (want_counts, want_stats, want_bad, (abs_sum, abs_sq)) in enumerate(refs):
        n = lens[i]
        print(f"segment {i}: n {n} start {starts[i]}  sum err {abs(stats[i, 3] - want_stats[3]):.3e} (bound {n * 2.0 ** -52 * abs_sum:.3e})  "
              f"sum_squares err {abs(stats[i, 4] - want_stats[4]):.3e} (bound {n * 2.0 ** -52 * abs_sq:.3e})")
        assert np.array_equal(counts[i], want_counts), f"segment {i}: counts differ at buckets {np.flatnonzero(counts[i] != want_counts)[:8]}"
        assert stats[i, 0] == want_stats[0] and stats[i, 1] == want_stats[1] and stats[i, 2] == want_stats[2], f"segment {i}: min / max / num"
        assert nonfinite[i] == want_bad, f"segment {i}: nonfinite"
        assert counts[i].sum() + want_bad == n, f"segment {i}: the gaps were counted"
        assert abs(stats[i, 3] - want_stats[3]) <= n * 2.0 ** -52 * abs_sum, f"segment {i}: sum"
        assert abs(stats[i, 4] - want_stats[4]) <= n * 2.0 ** -52 * abs_sq, f"segment {i}: sum_squares"
    # the issue's table of buckets, on the device
    special = dict(zip(segs[8].tolist(), np.searchsorted(LIM, segs[8].astype(np.float64), side="right")))
    assert counts[8][776] == 4 and counts[8][775] == 2 and counts[8][1066] == 1 and counts[8][485] == 1 and counts[8][1035] == 1, special
    assert counts[8][1550] == 2 and counts[8][1] == 1 and counts[8][0] == 0      # (-FLT_MAX lies above limit 0 = -DBL_MAX)
    assert nonfinite[9] == 9
    # bit-identical from call to call
    assert torch.equal(h.stats.view(torch.int64), h2.stats.view(torch.int64)) and torch.equal(h.counts, h2.counts)
    assert torch.equal(h.nonfinite, h2.nonfinite)


def test_histogram_of_a_whole_tensor_and_custom_limits(segment_case):
    dev = cuda()
    _, _, segs, refs = segment_case
    x = torch.from_numpy(segs[5].reshape(50, 100)).to(dev)
    h = ops.histogram_segments(x)
    assert h.counts.shape == (1, LIM.size) and np.array_equal(h.counts[0].cpu().numpy(), refs[5][0])
    assert h.stats[0, :3].tolist() == refs[5][1][:3]
    lim = [-1.0, -0.01, 0.0, 0.01, 0.5, FLT_MAX]
    h = ops.histogram_segments(x, limits=lim)
    want = np.bincount(np.searchsorted(np.asarray(lim), segs[5].astype(np.float64), side="right"), minlength=len(lim))
    assert np.array_equal(h.counts[0].cpu().numpy(), want)
    # a view that does not start on a 16-byte boundary
    y = torch.from_numpy(segs[4]).to(dev)[3:]
    hv = ops.histogram_segments(y)
    assert np.array_equal(hv.counts[0].cpu().numpy(), _reference(segs[4][3:])[0])


Q8_CASES = [((3, 7, 12), [0, 3, 7]), ((2, 20, 1152), [1, 20])]


def _q8(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, size=shape, dtype=np.uint8)


@pytest.mark.parametrize("shape,frames", Q8_CASES)
def test_histogram_frames_q8_against_numpy(shape, frames, tmp_path):
    dev = cuda()
    q = _q8(shape, sum(shape))
    live = np.arange(shape[1])[None, :] < np.asarray(frames)[:, None]
    want = np.append(np.bincount(q[live].reshape(-1), minlength=256), (~live).sum() * shape[2])
    tq, nf = torch.from_numpy(q).to(dev), torch.tensor(frames, dtype=torch.int32, device=dev)
    got = ops.histogram_frames_q8(tq, nf)
    assert got.dtype == torch.int64 and got.shape == (257,) and np.array_equal(got.cpu().numpy(), want)
    assert int(got.sum()) == q.size
    assert np.array_equal(ops.histogram_frames_q8(tq, nf.long()).cpu().numpy(), want)
    # add_input: the histogram of the dequantised batch with the padded frames at 0.0
    with S.SummaryWriter(str(tmp_path)) as w:
        w.add_input(tq, nf, 5)
        path = w.path
    (tag, h), = list(S.read_events(path))[1]["values"]
    x = utils.Dequantize(torch.from_numpy(q).to(torch.float32), ops.QUANT_MAX, ops.QUANT_MIN).numpy()
    d = np.where(live[:, :, None], x, np.float32(0.0)).astype(np.float64).reshape(-1)
    assert tag == "model/input_raw" and h["num"] == d.size and h["min"] == d.min() and h["max"] == d.max()
    assert np.array_equal(S.expand_histogram(h), np.bincount(np.searchsorted(LIM, d, side="right"), minlength=LIM.size))
    assert abs(h["sum"] - math.fsum(d)) <= d.size * 2.0 ** -52 * math.fsum(np.abs(d))
    assert abs(h["sum_squares"] - math.fsum(d * d)) <= d.size * 2.0 ** -52 * math.fsum(d * d)


# ---- the trainer ---------------------------------------------------------------------------------------------------------------------
V, B, MF = 30, 6, 40


def _trainer(dev):
    return Trainer(registry.get_model("NetVladV1"), vocab_size=V, batch_size=B, base_learning_rate=1e-3, device=dev, seed=3,
                   model_kwargs=dict(iterations=16, cluster_size=32, hidden_size=32, encoder=False))


def _batches(dev, n):
    rng = np.random.default_rng(23)
    out = []
    for i in range(n):
        nf = torch.tensor(rng.integers(1, MF + 1, B), dtype=torch.int32)
        q = torch.from_numpy(rng.integers(0, 256, size=(B, MF, 1152), dtype=np.uint8))
        q = torch.where(torch.arange(MF).view(1, -1, 1) < nf.view(-1, 1, 1), q, torch.zeros((), dtype=torch.uint8))
        y = torch.zeros(B, V, dtype=torch.bool)
        y[torch.arange(B), torch.from_numpy(rng.integers(0, V, B))] = True
        out.append(([f"clip{i}_{j}" for j in range(B)], q.to(dev), y.to(dev), nf.to(dev)))
    return out


def test_add_variables_writes_one_histogram_per_store_variable(tmp_path):
    dev = cuda()
    try:
        tr = _trainer(dev)
        for _, q, y, nf in _batches(dev, 2):
            tr.step(q, nf, y)
        with S.SummaryWriter(str(tmp_path)) as w:
            w.add_variables(tr, 2)
            path = w.path
        state = tr.state_dict()
        ev = list(S.read_events(path))
        assert len(ev) == 2 and ev[1]["step"] == 2
        got = dict(ev[1]["values"])
        assert len(got) == len(ev[1]["values"]) and sorted(got) == sorted(tr.store.vars)
        assert any(not t for t in tr.store.trainable.values()) and any(tr.store.trainable.values())
        for name, v in tr.store.vars.items():
            want_counts, want_stats, bad, (abs_sum, abs_sq) = _reference(state[name].numpy().reshape(-1))
            h, n = got[name], v.numel()
            assert bad == 0 and h["num"] == n == want_stats[2], f"{name}: num (the arena's padding must not be counted)"
            assert np.array_equal(S.expand_histogram(h), want_counts), name
            assert h["min"] == want_stats[0] and h["max"] == want_stats[1], name
            assert abs(h["sum"] - want_stats[3]) <= n * 2.0 ** -52 * abs_sum and abs(h["sum_squares"] - want_stats[4]) <= n * 2.0 ** -52 * abs_sq, name
    finally:
        FLAGS.reset()


def test_summaries_do_not_change_a_bit_of_the_training_result(tmp_path):
    dev = cuda()
    batches = _batches(dev, 12)
    try:
        torch.manual_seed(0)
        plain = _trainer(dev)
        training.run(plain, iter(batches), log_every=2, log=lambda s: None)
        torch.manual_seed(0)
        tr = _trainer(dev)
        w = S.SummaryWriter(str(tmp_path))
        training.run(tr, iter(batches), log_every=2, log=lambda s: None, summary_writer=w, histogram_steps=4)
        w.close()
        assert not [t for t in threading.enumerate() if t.name.startswith("lpm-")]
        a, b = plain.state_dict(), tr.state_dict()
        assert sorted(a) == sorted(b) and a["global_step"] == b["global_step"] == 12
        for k in a:
            if torch.is_tensor(a[k]):
                assert torch.equal(a[k], b[k]), k
        ev = list(S.read_events(w.path))[1:]
        scalars = [e for e in ev if all(isinstance(v, float) for _, v in e["values"])]
        histos = [e for e in ev if e not in scalars]
        assert [e["step"] for e in scalars] == [2, 4, 6, 8, 10, 12]
        assert all([t for t, _ in e["values"]] == ["model/Training_Hit@1", "model/Training_Perr", "model/Training_GAP",
                                                   "global_step/Examples/Second", "label_loss", "learning_rate"] for e in scalars)
        assert sorted({e["step"] for e in histos}) == [2, 6, 10]
        for s in (2, 6, 10):
            tags = [t for e in histos if e["step"] == s for t, _ in e["values"]]
            assert sorted(tags) == sorted(list(tr.store.vars) + ["model/input_raw"])
        # the file keeps the order of the calls: a step's scalars, then its histograms
        assert [e["step"] for e in ev] == sorted(e["step"] for e in ev)
    finally:
        FLAGS.reset()


def test_activation_histograms_only_on_request(tmp_path):
    dev = cuda()
    batches = _batches(dev, 2)
    try:
        tr = _trainer(dev)
        with S.SummaryWriter(str(tmp_path)) as w:
            training.run(tr, iter(batches), log_every=1, log=lambda s: None, summary_writer=w, histogram_steps=2, summary_activations=True)
            path = w.path
        assert tr.store.summaries is None, "collection is switched off again after the histogram step"
        tags = [t for e in S.read_events(path) for t, v in e["values"] if isinstance(v, dict)]
        extra = [t for t in tags if t not in tr.store.vars and t != "model/input_raw"]
        assert extra, "no activation histogram was written"
        assert len(tags) == len(tr.store.vars) + 1 + len(extra), "histograms at step 1 only (histogram_steps = 2, two steps)"
    finally:
        FLAGS.reset()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["cpu", "dtype", "past_the_end", "negative_start", "zero_length", "unsorted", "count_mismatch", "last_limit"])
def test_histogram_segments_refuses_before_any_launch(case, monkeypatch):
    dev = cuda()
    x = torch.zeros(100, device=dev)
    kw = {}
    if case == "cpu":
        x = x.cpu()
    elif case == "dtype":
        x = x.double()
    elif case == "past_the_end":
        kw = dict(seg_start=[0, 90], seg_len=[10, 11])
    elif case == "negative_start":
        kw = dict(seg_start=[-1], seg_len=[10])
    elif case == "zero_length":
        kw = dict(seg_start=[0, 50], seg_len=[10, 0])
    elif case == "unsorted":
        kw = dict(limits=[-1.0, 1.0, 0.5, FLT_MAX])
    elif case == "count_mismatch":
        kw = dict(seg_start=[0, 50], seg_len=[10])
    elif case == "last_limit":
        kw = dict(limits=[-1.0, 1.0])

    def refuse(*a, **k):
        raise AssertionError("the library was reached: the argument check came too late")
    monkeypatch.setattr(_capi, "load", refuse)
    with pytest.raises(_capi.LpmError):
        ops.histogram_segments(x, **kw)


def test_histogram_frames_q8_refuses_before_any_launch(monkeypatch):
    dev = cuda()

    def refuse(*a, **k):
        raise AssertionError("the library was reached: the argument check came too late")
    monkeypatch.setattr(_capi, "load", refuse)
    nf = torch.tensor([1, 2], dtype=torch.int32, device=dev)
    for q, n in ((torch.zeros(2, 3, 6, dtype=torch.uint8, device=dev), nf), (torch.zeros(2, 3, 8, device=dev), nf),
                 (torch.zeros(2, 3, 8, dtype=torch.uint8, device=dev), nf[:1]), (torch.zeros(2, 3, 8, dtype=torch.uint8), nf.cpu())):
        with pytest.raises(_capi.LpmError):
            ops.histogram_frames_q8(q, n)
