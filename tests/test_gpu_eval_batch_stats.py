"""-m gpu: lpm_eval_batch_stats (ops.eval_batch_stats) behind lpm_eval_rows against exact host values, DeviceEvaluationMetrics with
FLAGS.eval_stats_fused against eval_util and against the flag off, evaluate(on_batch=...) without a synchronisation per batch, and the
eval command line on the device."""
import math

import numpy as np
import pytest
import torch

from learnablepoolingmethods_amd import FLAGS, eval_util, evaluation, losses, ops, readers, registry, summaries, training
from learnablepoolingmethods_amd.evaluation import DeviceEvaluationMetrics, cross_entropy_rows, evaluate
from learnablepoolingmethods_amd.predictor import Predictor

from tests import test_inference_cli_host as HC
from tests._util import cuda

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
# one row; V no multiple of 4 or 16; B above one workgroup's 256 threads; V above 4096 (no LDS image of the columns); many short rows
SHAPES = [(1, 2), (3, 5), (64, 500), (80, 3862), (257, 4097), (1024, 11)]
DENSITIES = [0.0, 0.02, 0.5, 1.0]
_CACHE = {}


def _batch(B, V, density):
    """Predictions, bool labels and lpm_eval_rows' outputs of one batch on the device, made once per (shape, density) and left as they are."""
    key = (B, V, density)
    if key not in _CACHE:
        dev = cuda()
        g = torch.Generator().manual_seed(1000 * B + V + int(100 * density))
        p = torch.rand(B, V, generator=g)
        if density == 0.0:
            y = torch.zeros(B, V, dtype=torch.bool)
        elif density == 1.0:
            y = torch.ones(B, V, dtype=torch.bool)
        else:
            y = torch.rand(B, V, generator=g) < density
            if density == 0.02:
                y[::9] = False                      # some videos without labels (test_eval_gpu's _tie_free)
        p, y = p.to(dev), y.to(dev)
        rows = ops.eval_rows(p, y, min(20, V))
        _CACHE[key] = (p, y, rows)
    return _CACHE[key]


def _bound(terms, B, value):
    """The worst case of ANY fixed-order fp64 sum of B terms against the exactly rounded one, divided by B: (B - 1) 2^-53 sum |x_i| / B,
    plus one ulp of the result for the division's and the reference's own rounding."""
    return (B - 1) * U * math.fsum(abs(x) for x in terms) / B + math.ulp(value)


def _stats(rows, labels, class_pos, sum_loss, loss=None):
    batch = torch.full((4,), -7.0, dtype=torch.float64, device=class_pos.device)
    out = ops.eval_batch_stats(rows, labels, batch, sum_loss, class_pos, loss)
    assert out is batch
    return batch


@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{b}x{v}" for b, v in SHAPES])
def test_batch_stats_against_exact_host_values(shape, density):
    B, V = shape
    dev = cuda()
    _, y, rows = _batch(B, V, density)
    hit1, nl, hn, lr = rows.hit1.cpu(), rows.num_labels.cpu().tolist(), rows.hits_at_n.cpu().tolist(), rows.loss_row.cpu().tolist()
    perr_terms = [h / n if n > 0 else 0.0 for h, n in zip(hn, nl)]
    want_pos = y.sum(0).cpu()
    big = torch.zeros(B + 1, V, dtype=torch.uint8, device=dev)
    big[1:] = y
    start = torch.arange(V, dtype=torch.int64, device=dev) * 3 + 5
    variants = {"bool": y, "uint8": y.to(torch.uint8), "row slice": big[1:]}
    if V % 2:
        assert variants["row slice"].data_ptr() % 2 == 1           # an odd start address
    results = []
    for name, labels in variants.items():
        class_pos = start.clone()                                   # from a non-zero class_pos
        sum_loss = torch.full((), 0.75, dtype=torch.float64, device=dev)
        batch = _stats(rows, labels, class_pos, sum_loss).cpu().tolist()
        print(f"{name} B={B} V={V} density={density}: batch={batch} sum_loss={float(sum_loss)!r}")
        assert torch.equal(class_pos.cpu() - start.cpu(), want_pos), name
        assert batch[0] == hit1.double().mean().item(), name        # (the host mean: an exact integer sum, one division)
        assert batch[3] == float(B)
        want_perr, want_loss = math.fsum(perr_terms) / B, math.fsum(lr) / B
        print(f"   perr {batch[1]!r} vs {want_perr!r} (bound {_bound(perr_terms, B, want_perr):.3e}); "
              f"loss {batch[2]!r} vs {want_loss!r} (bound {_bound(lr, B, want_loss):.3e})")
        assert abs(batch[1] - want_perr) <= _bound(perr_terms, B, want_perr), name
        assert abs(batch[2] - want_loss) <= _bound(lr, B, want_loss), name
        assert float(sum_loss) == 0.75 + batch[2] * B, name        # exactly: the product rounded, then the sum
        results.append((batch, class_pos.cpu()))
    # determinism: the same inputs, whatever the labels' dtype and address, give the same bits
    again = _stats(rows, y, start.clone(), torch.full((), 0.75, dtype=torch.float64, device=dev)).cpu().tolist()
    for batch, _ in results:
        assert np.array(batch).tobytes() == np.array(again).tobytes()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_given_loss_replaces_the_mean_bit_for_bit(dtype):
    dev = cuda()
    _, y, rows = _batch(64, 500, 0.02)
    given = torch.tensor(0.1234567891234, dtype=dtype, device=dev)
    class_pos = torch.zeros(500, dtype=torch.int64, device=dev)
    sum_loss = torch.zeros((), dtype=torch.float64, device=dev)
    no_loss = ops.EvalRows(rows.hit1, rows.num_labels, rows.hits_at_n, None, rows.top_index, rows.top_value, rows.top_label)
    batch = _stats(no_loss, y, class_pos, sum_loss, loss=given.reshape(1)).cpu().tolist()
    own = _stats(rows, y, torch.zeros_like(class_pos), torch.zeros_like(sum_loss)).cpu().tolist()
    assert batch[2] == float(given.double()) and float(sum_loss) == batch[2] * 64
    assert batch[:2] == own[:2] and batch[3] == 64.0 and torch.equal(class_pos, y.sum(0))


def test_nan_loss_row_gives_a_nan_mean_and_leaves_the_rest():
    dev = cuda()
    _, y, rows = _batch(80, 3862, 0.02)
    lr = rows.loss_row.clone()
    lr[41] = float("nan")
    bad = rows._replace(loss_row=lr)
    class_pos = torch.zeros(3862, dtype=torch.int64, device=dev)
    sum_loss = torch.zeros((), dtype=torch.float64, device=dev)
    batch = _stats(bad, y, class_pos, sum_loss).cpu().tolist()
    good = _stats(rows, y, torch.zeros_like(class_pos), torch.zeros_like(sum_loss)).cpu().tolist()
    assert math.isnan(batch[2]) and math.isnan(float(sum_loss))
    assert batch[:2] == good[:2] and batch[3] == 80.0 and torch.equal(class_pos, y.sum(0))


def test_bad_arguments_are_refused_before_the_launch():
    dev = cuda()
    from learnablepoolingmethods_amd._capi import LpmError
    _, y, rows = _batch(3, 5, 0.5)
    ok = dict(batch=torch.zeros(4, dtype=torch.float64, device=dev), sum_loss=torch.zeros((), dtype=torch.float64, device=dev),
              class_pos=torch.zeros(5, dtype=torch.int64, device=dev))
    with pytest.raises(LpmError, match="row-contiguous"):
        ops.eval_batch_stats(rows, torch.zeros(5, 3, dtype=torch.uint8, device=dev).t(), **ok)
    with pytest.raises(LpmError, match="class_pos"):
        ops.eval_batch_stats(rows, y, ok["batch"], ok["sum_loss"], torch.zeros(4, dtype=torch.int64, device=dev))
    with pytest.raises(LpmError, match="ONE float32 or float64"):
        ops.eval_batch_stats(rows, y, loss=torch.zeros(3, device=dev), **ok)
    with pytest.raises(LpmError, match="loss_row"):
        ops.eval_batch_stats(rows._replace(loss_row=None), y, **ok)
    with pytest.raises(LpmError):
        ops.eval_batch_stats(rows, y.cpu(), **ok)
    assert float(ok["batch"].abs().sum()) == 0.0 and int(ok["class_pos"].sum()) == 0


# ---- DeviceEvaluationMetrics with the flag ---------------------------------------------------------------------------------------------
def _tie_free(N, V, seed):
    g = torch.Generator().manual_seed(seed)
    p = ((torch.randperm(N * V, generator=g) + 1).double() / (N * V + 1)).float().view(N, V)
    y = torch.rand(N, V, generator=g) < 0.02
    y[::9] = False
    return p, y


def test_fused_device_metrics_match_eval_util_and_the_unfused_route():
    dev = cuda()
    V, splits = 500, (64, 64, 64, 64, 37)
    N = sum(splits)
    p, y = _tie_free(N, V, 11)
    loss = cross_entropy_rows(p, y)
    pd, yd = p.to(dev), y.to(dev)
    hm = eval_util.EvaluationMetrics(V, 20)
    try:
        FLAGS.eval_stats_fused = True
        given, own = DeviceEvaluationMetrics(V, 20, dev), DeviceEvaluationMetrics(V, 20, dev)
        o = 0
        for s in splits:
            sl = slice(o, o + s)
            a = given.accumulate(pd[sl], yd[sl], loss[sl].to(dev))
            own.accumulate(pd[sl], yd[sl])
            b = hm.accumulate(p[sl], y[sl], loss[sl])
            assert all(t.is_cuda and t.dim() == 0 and t.dtype == torch.float64 for t in a.values()) and set(a) == {"hit_at_one", "perr", "loss"}
            for key in ("hit_at_one", "perr", "loss"):
                print(key, float(a[key]), b[key])
                assert abs(float(a[key]) - b[key]) <= 1e-12, key
            o += s
        got, got_own, ref = given.get(), own.get(), hm.get()
        FLAGS.eval_stats_fused = False
        given_off, own_off = DeviceEvaluationMetrics(V, 20, dev), DeviceEvaluationMetrics(V, 20, dev)
        o, slack = 0, 0.0
        for s in splits:
            sl = slice(o, o + s)
            given_off.accumulate(pd[sl], yd[sl], loss[sl].to(dev))
            r = own_off.accumulate(pd[sl], yd[sl])
            # both routes sum the SAME s row losses (lpm_eval_rows' loss_row) in some fixed order: each is within (s - 1) 2^-53 sum |x| of
            # the exact sum, its mean (one division) and the mean * s (one product) within one more ulp each of a value near the sum
            rows_sum = float(r["loss"]) * s
            slack += 2 * ((s - 1) * U * abs(rows_sum) * (1 + 1e-9) + 2 * math.ulp(rows_sum))
            o += s
        off, off_own = given_off.get(), own_off.get()
    finally:
        FLAGS.reset()
    for key in ("avg_hit_at_one", "avg_perr", "avg_loss", "gap"):
        assert abs(got[key] - ref[key]) <= 1e-12, key
    np.testing.assert_allclose(np.array(got["aps"]), np.array(ref["aps"]), rtol=0, atol=1e-12)
    assert got["num_examples"] == N
    for on, was in ((got, off), (got_own, off_own)):
        assert on["aps"] == was["aps"] and on["gap"] == was["gap"] and on["avg_hit_at_one"] == was["avg_hit_at_one"]
        assert on["avg_perr"] == was["avg_perr"] and on["num_examples"] == was["num_examples"]        # (get() forms it from the rows)
    assert got["avg_loss"] == off["avg_loss"]              # a given loss of s elements is reduced by torch on both routes
    # the running sum of five products adds one rounding per batch and route on top
    bound = (slack + 2 * len(splits) * math.ulp(got_own["avg_loss"] * N)) / N
    print("avg_loss fused", got_own["avg_loss"], "unfused", off_own["avg_loss"], "bound", bound)
    assert abs(got_own["avg_loss"] - off_own["avg_loss"]) <= bound


# ---- evaluate(on_batch=...) -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """A video-level MoeModel trained for two steps on the CPU (the host test's files and flags): directory, train_dir, pattern, files."""
    tmp = tmp_path_factory.mktemp("evalcli")
    files = HC._video_files(tmp)
    train_dir, pattern = str(tmp / "model"), str(tmp / "video*.tfrecord")
    try:
        training.main(["--train_data_pattern", pattern, "--train_dir", train_dir] + HC.VIDEO_ARGS)
    finally:
        FLAGS.reset()
    return tmp, train_dir, pattern, files


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
def test_evaluate_reports_every_batch_without_a_sync_per_batch(trained, fused):
    dev = cuda()
    tmp, train_dir, _, _ = trained
    g = torch.Generator().manual_seed(3)
    sizes = (4, 4, 3, 4, 1, 4)
    resident = [([f"b{i}-{j}" for j in range(n)], torch.randn(n, 36, generator=g).to(dev), (torch.rand(n, HC.V, generator=g) < 0.3).to(dev),
                 torch.ones(n, dtype=torch.int32, device=dev)) for i, n in enumerate(sizes)]

    def guarded():
        """The mode is on from the first batch until the iterator is exhausted: everything evaluate() does between the batches."""
        try:
            for i, b in enumerate(resident):
                if i == 0:
                    torch.cuda.synchronize()
                    torch.cuda.set_sync_debug_mode("error")
                yield b
        finally:
            torch.cuda.set_sync_debug_mode("default")

    calls = []
    writer = summaries.SummaryWriter(str(tmp / f"events_{fused}"))
    try:
        FLAGS.moe_num_mixtures = 3
        FLAGS.eval_stats_fused = fused
        pr = Predictor.from_checkpoint(training.latest_checkpoint(train_dir), registry.get_model("MoeModel"), vocab_size=HC.V, device=dev)
        pr.predict(resident[0][1], resident[0][3])                 # (first-use work of the predictor happens outside the guarded loop)
        returned = []
        info = evaluate(pr, guarded(), top_k=5, summary_writer=writer, global_step=7, on_batch=lambda n, b: calls.append((n, dict(b))))
        returned.append(len(calls))
        plain = evaluate(pr, iter(resident), top_k=5)
        hm = eval_util.EvaluationMetrics(HC.V, 5)
        want = []
        for _, x, y, nf in resident:
            p = pr.predict(x, nf).cpu()
            want.append(hm.accumulate(p, y.cpu(), cross_entropy_rows(p, y.cpu())))
    finally:
        torch.cuda.set_sync_debug_mode("default")
        FLAGS.reset()
        writer.close()
    assert returned == [6]                                          # all six delivered before evaluate returned
    assert [n for n, _ in calls] == list(np.cumsum(sizes))
    for (_, b), w in zip(calls, want):
        assert set(b) == {"hit_at_one", "perr", "loss", "examples_per_second"} and all(type(v) is float for v in b.values())
        assert abs(b["hit_at_one"] - w["hit_at_one"]) <= 1e-12 and abs(b["perr"] - w["perr"]) <= 1e-12
        assert abs(b["loss"] - w["loss"]) <= 1e-6 * abs(w["loss"])                  # (logf on the device against the host's)
        assert b["examples_per_second"] > 0
    for key in ("avg_hit_at_one", "avg_perr", "avg_loss", "gap", "aps", "num_examples"):
        assert info[key] == plain[key], key                          # on_batch changes nothing of the epoch's result
    events = [e for e in summaries.read_events(writer.path) if e.get("values")]
    tags = [[tag for tag, _ in e["values"]] for e in events]
    per_batch = ["GlobalStep/Eval_Hit@1", "GlobalStep/Eval_Perr", "GlobalStep/Eval_Loss", "GlobalStep/Eval_Example_Second"]
    assert tags == [per_batch] * 6 + [["Epoch/Eval_Avg_Hit@1", "Epoch/Eval_Avg_Perr", "Epoch/Eval_Avg_Loss", "Epoch/Eval_MAP", "Epoch/Eval_GAP"]]
    assert all(e["step"] == 7 for e in events)
    for e, (_, b) in zip(events, calls):
        assert [value for _, value in e["values"][:3]] == [float(np.float32(b[k])) for k in ("hit_at_one", "perr", "loss")]


def test_eval_command_line_on_the_device(trained):
    dev = cuda()
    tmp, train_dir, pattern, files = trained
    reader = readers.YT8MAggregatedFeatureReader(num_classes=HC.V, feature_sizes=[24, 12])
    timing = ("examples_per_second",)
    try:
        for fused in (True, False):
            FLAGS.eval_stats_fused = fused
            got = evaluation.main(["--train_dir", train_dir, "--eval_data_pattern", pattern, "--run_once", "--device", "cuda", "--batch_size", "3",
                                   "--top_k", "5", "--summary_dir", str(tmp / f"cli_{fused}")])
            assert FLAGS.eval_stats_fused is fused
            FLAGS.moe_num_mixtures = 3
            pr = Predictor.from_checkpoint(training.latest_checkpoint(train_dir), registry.get_model("MoeModel"), vocab_size=HC.V, device=dev)
            batches = reader.device_batches(files, 3, device=dev)
            try:
                want = evaluate(pr, batches, top_k=5, label_loss_fn=losses.by_name("CrossEntropyLoss"))
            finally:
                batches.close()
            FLAGS.reset()
            assert got.pop("global_step") == 2 and got["num_examples"] == 7
            assert {k: v for k, v in got.items() if k not in timing} == {k: v for k, v in want.items() if k not in timing}
    finally:
        FLAGS.reset()
