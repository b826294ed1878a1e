"""-m gpu: ops.class_filter (csrc/class_filter.hip) and MoeModel2 / JuhanMoeModel on the fused route against the fp64 restatement on the
CPU (tests/_class_filter_ref.py) -- never against the op itself.

The bound is tests/test_gpu_triangulation_v6.py's rule: per output and per gradient the restatement evaluated in fp32 torch on the CPU
carries an error err32 against fp64 (maximum absolute error over the maximum absolute reference); the op's error must be
<= max(8 err32, 1e-6).  mean, rstd and both new moving statistics fall under the same bound.  A part whose fp64 reference is identically
zero must be exactly zero in the op.  Every figure is printed before any is asserted.  All inputs are drawn in fp32 and widened, so the op
and the reference read the same numbers; every pre-activation is sign(z) (|z| + 0.01), and that margin is asserted on the fp64
restatement before any launch.  One part is measured on another scale, in one test: dbias in the offset regime, a sum that cancels to
zero in exact arithmetic, relative to the fp64 sum_b |dpre| (test_offset_regime says why).

Measured on the MI355X: 107 tests in 4.4 s; worst error over bound 0.63, at (2, 1) filter1 leaky_relu in training."""
import functools
import math

import pytest
import torch

from tests import _class_filter_ref as R
from tests._util import REL_TOL, cuda, rel_err, rel_l2

pytestmark = pytest.mark.gpu

SHAPES = [(1, 5), (2, 1), (3, 37), (64, 64), (65, 130), (257, 33), (1024, 70), (4, 3862), (4, 7724)]
CONFIGS = [("filter1", "relu"), ("filter1", "leaky_relu"), ("residual", "relu"), ("residual", "leaky_relu"), ("output", "sigmoid")]
BN_NAMES = ("gamma", "beta", "moving_mean", "moving_variance")
WORST = {"ratio": 0.0, "what": ""}


def _err(a, ref, scale=None):
    ref = ref.double()
    s = float(ref.abs().max()) if scale is None else float(scale)
    return float((a.detach().double().cpu() - ref).abs().max()) / max(s, 1e-300)


@functools.lru_cache(maxsize=None)
def _case(B, C, kind, act, training, seed=0, offset=0.0, dead=False):
    """-> (fp32 inputs, dy, fp64 outputs and gradients, the fp32 CPU evaluation's); computed once and left unchanged"""
    inp32, dy32 = R.make_stage_inputs(B, C, kind, act, seed, offset=offset, dead=dead)
    o64, g64 = R.stage_gradients(R.widen(inp32), act, training, dy32.double())
    o32, g32 = R.stage_gradients(inp32, act, training, dy32)
    return inp32, dy32, (o64, g64), (o32, g32)


def _assert_margin(tag, inp32):
    pre = R.pre_activation(R.widen(inp32))
    m = float(pre.abs().min())
    print(f"[class_filter] {tag}: smallest |pre-activation| in fp64 {m:.4f}")
    assert m >= 0.009


def _run_op(inp32, dy32, act, training, dev):
    """-> (y, mean, rstd, new moving statistics, gradients): the autograd op for y, the gradients and the moving statistics; one more
    forward through the C entry for mean and rstd (on copies of the moving statistics), whose y must be the op's bit for bit."""
    from learnablepoolingmethods_amd import _capi, ops
    from learnablepoolingmethods_amd._capi import ptr, stream_ptr
    t = {k: v.to(dev) for k, v in inp32.items()}
    names = [n for n in R.GRAD_NAMES if n in t]
    for n in names:
        t[n].requires_grad_(True)
    has_bn = "gamma" in t
    bn = tuple(t[n] for n in BN_NAMES) if has_bn else None
    stats0 = (t["moving_mean"].clone(), t["moving_variance"].clone()) if has_bn else None
    keep = t.get("keep") if training else None
    y = ops.class_filter(t["a"], t.get("bias"), t.get("residual"), act=act, bn=bn, is_training=training, keep=keep,
                         keep_prob=R.KEEP_PROB, decay=R.DECAY, alpha=R.ALPHA)
    grads = dict(zip(names, torch.autograd.grad((y * dy32.to(dev)).sum(), [t[n] for n in names])))
    mean = rstd = None
    if has_bn:
        lib = _capi.load()
        B, C = t["a"].shape
        y2, mean, rstd = torch.empty_like(y), torch.empty(C, device=dev), torch.empty(C, device=dev)
        lib.check(lib._lpm_class_filter_fwd(ptr(t["a"].detach()), ptr(t["bias"].detach() if "bias" in t else None),
                                            ptr(t["residual"].detach() if "residual" in t else None), B, C, ops.CLASS_FILTER_ACTS[act], R.ALPHA,
                                            ptr(t["gamma"].detach()), ptr(t["beta"].detach()), ptr(stats0[0]), ptr(stats0[1]), int(training),
                                            R.EPS, R.DECAY, ptr(keep), R.KEEP_PROB, ptr(y2), ptr(mean), ptr(rstd), stream_ptr()), "fwd")
        assert torch.equal(y2, y.detach())
        assert torch.equal(stats0[0], t["moving_mean"]) and torch.equal(stats0[1], t["moving_variance"])
    stats = (t["moving_mean"], t["moving_variance"]) if has_bn else None
    return y.detach(), mean, rstd, stats, grads


def _check(tag, got, ref64, ref32, scales=None):
    """got / ref64 / ref32: {name: tensor}; scales: {name: the scale both errors of that part are taken relative to, instead of the
    largest |reference|}.  Every figure is printed before anything is asserted."""
    figures = []
    for n, op in got.items():
        r64, r32 = ref64[n], ref32[n]
        zero = float(r64.abs().max()) == 0.0
        scale = (scales or {}).get(n)
        if zero:
            e_op, e32 = float(op.detach().abs().max()), 0.0
            print(f"[class_filter] {tag} {n}: the fp64 reference is identically zero; largest |op| {e_op:.3e}")
        else:
            e_op, e32 = _err(op, r64, scale), _err(r32, r64, scale)
            print(f"[class_filter] {tag} {n}: op error {e_op:.3e}, fp32 evaluation error {e32:.3e}, bound {max(8 * e32, 1e-6):.3e}, "
                  f"ratio {e_op / max(8 * e32, 1e-6):.3f}")
        figures.append((n, zero, e_op, e32))
    worst = max([e_op / max(8 * e32, 1e-6) for _, zero, e_op, e32 in figures if not zero], default=0.0)
    if worst > WORST["ratio"]:
        WORST["ratio"], WORST["what"] = worst, tag
    print(f"[class_filter] {tag}: worst error over bound {worst:.3f} (so far over all cases: {WORST['ratio']:.3f} at {WORST['what']})")
    for n, zero, e_op, e32 in figures:
        if zero:
            assert e_op == 0.0, f"{tag} {n}: must be exactly zero, largest |op| {e_op:.3e}"
        else:
            assert math.isfinite(e_op) and e_op <= max(8 * e32, 1e-6), f"{tag} {n}: op error {e_op:.3e} > max(8 x {e32:.3e}, 1e-6)"


def _compare(tag, inp32, dy32, ref64, ref32, act, training, dev, scales=None):
    y, mean, rstd, stats, grads = _run_op(inp32, dy32, act, training, dev)
    (o64, g64), (o32, g32) = ref64, ref32
    got = {"y": y}
    r64, r32 = {"y": o64["y"]}, {"y": o32["y"]}
    if mean is not None:
        got.update(mean=mean, rstd=rstd, moving_mean=stats[0], moving_variance=stats[1])
        for n in ("mean", "rstd", "moving_mean", "moving_variance"):
            r64[n], r32[n] = o64[n], o32[n]
    for n, g in grads.items():
        got["d" + n], r64["d" + n], r32["d" + n] = g, g64[n], g32[n]
    _check(tag, got, r64, r32, scales)
    return y, mean, rstd, stats, grads


@pytest.mark.parametrize("training", [True, False], ids=["training", "eval"])
@pytest.mark.parametrize("kind,act", CONFIGS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_stage_matches_fp64(shape, kind, act, training):
    dev = cuda()
    B, C = shape
    inp32, dy32, ref64, ref32 = _case(B, C, kind, act, training)
    tag = f"{shape} {kind} {act} {'training' if training else 'eval'}"
    _assert_margin(tag, inp32)
    y, _, _, _, grads = _compare(tag, inp32, dy32, ref64, ref32, act, training, dev)
    assert y.shape == (B, C) and grads["a"].shape == (B, C)
    if "residual" in grads:
        assert torch.equal(grads["residual"], grads["a"])           # dpre once: the gradient of a and of the residual alike


@pytest.mark.parametrize("kind,act", CONFIGS[:4])
def test_offset_regime(kind, act):
    """|mean| = 1e3 std per column.  The two-pass restatement keeps err32 small; moments from raw sums (E[u^2] - mean^2 in fp32) do not:
    both are checked on the CPU here, before the op runs.  Every pre-activation of a column has the column's sign, so act' is constant
    per column and dbias = act' sum_b du is a sum that cancels to zero in exact arithmetic (the batch norm's backward removes the mean):
    the fp64 reference holds rounding noise only.  As tests/test_gpu_triangulation_v6.py does for its cancelling sums, the error of dbias
    and its err32 are taken relative to the fp64 sum_b |dpre| here (the largest over the columns)."""
    dev = cuda()
    B, C = 65, 130
    inp32, dy32, ref64, ref32 = _case(B, C, kind, act, True, seed=1, offset=1e3)
    tag = f"offset {kind} {act}"
    _assert_margin(tag, inp32)
    o64, o32 = ref64[0], ref32[0]
    std = 1 / o64["rstd"] ** 2 - R.EPS
    ratio = float((o64["mean"].abs() / std.sqrt()).min())
    e32 = _err(o32["y"], o64["y"])
    u32 = o32["u"]
    raw_var = (u32 * u32).mean(0) - u32.mean(0) ** 2                 # what a raw-moment kernel would hold, in fp32
    y_raw = (u32 - u32.mean(0)) / torch.sqrt(raw_var.clamp_min(0) + R.EPS) * inp32["gamma"] + inp32["beta"]
    if "keep" in inp32:
        y_raw = y_raw * inp32["keep"].float() / R.KEEP_PROB
    e_raw = _err(y_raw, o64["y"])
    print(f"[class_filter] {tag}: smallest |mean| / std {ratio:.1f}; y: fp32 two-pass error {e32:.3e}, fp32 raw-moment error {e_raw:.3e}")
    assert ratio >= 500 and e32 <= 1e-3 and e_raw > max(8 * e32, 1e-6)
    scales = {"dbias": float(ref64[1]["a"].abs().sum(0).max())} if "bias" in inp32 else None
    _compare(tag, inp32, dy32, ref64, ref32, act, True, dev, scales)


@pytest.mark.parametrize("kind", ["filter1", "residual"])
def test_dead_columns_under_relu(kind):
    """Every pre-activation negative: in training y is exactly beta (times mask / keep_prob), dgamma and dpre are exactly zero"""
    dev = cuda()
    B, C = 65, 130
    inp32, dy32, ref64, ref32 = _case(B, C, kind, "relu", True, seed=2, dead=True)
    assert float(R.pre_activation(R.widen(inp32)).max()) <= -0.009
    y, mean, rstd, stats, grads = _compare(f"dead {kind}", inp32, dy32, ref64, ref32, "relu", True, dev)
    want = inp32["beta"].expand(B, C)
    if "keep" in inp32:
        want = torch.where(inp32["keep"] != 0, want / torch.tensor(R.KEEP_PROB, dtype=torch.float32), torch.zeros(()))
    assert torch.equal(y.cpu(), want)
    assert torch.count_nonzero(grads["gamma"]) == 0 and torch.count_nonzero(grads["a"]) == 0
    assert torch.count_nonzero(mean) == 0


@pytest.mark.parametrize("act", ["relu", "leaky_relu"])
def test_one_row_in_training(act):
    """B = 1: the batch variance is zero, y is exactly beta, and the moving variance decays towards 0"""
    dev = cuda()
    C = 37
    inp32, dy32, ref64, ref32 = _case(1, C, "residual", act, True, seed=3)
    y, mean, rstd, stats, grads = _compare(f"one row {act}", inp32, dy32, ref64, ref32, act, True, dev)
    assert torch.equal(y.cpu(), inp32["beta"].view(1, C))
    assert torch.equal(mean.cpu(), ref32[0]["u"].view(C))
    assert torch.count_nonzero(grads["a"]) == 0 and torch.count_nonzero(grads["gamma"]) == 0
    assert torch.allclose(stats[1].cpu(), 0.99 * inp32["moving_variance"], rtol=1e-6, atol=0) and bool((stats[1].cpu() < inp32["moving_variance"]).all())


@pytest.mark.parametrize("training", [True, False], ids=["training", "eval"])
def test_two_runs_give_the_same_bits(training):
    dev = cuda()
    inp32, dy32, _, _ = _case(257, 33, "filter1", "leaky_relu", training)
    a = _run_op(inp32, dy32, "leaky_relu", training, dev)
    b = _run_op(inp32, dy32, "leaky_relu", training, dev)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert torch.equal(a[3][0], b[3][0]) and torch.equal(a[3][1], b[3][1])
    for n in a[4]:
        assert torch.equal(a[4][n], b[4][n]), n


def test_refusals_before_any_launch():
    from learnablepoolingmethods_amd import _capi, ops
    from learnablepoolingmethods_amd._capi import LpmError, ptr, stream_ptr
    dev = cuda()
    C = 6
    a = torch.randn(4, C, device=dev)
    bn = (torch.ones(C, device=dev), torch.zeros(C, device=dev), torch.full((C,), 0.25, device=dev), torch.full((C,), 2.0, device=dev))
    keep = torch.ones(4, C, dtype=torch.uint8, device=dev)
    bad = [dict(a=torch.randn(1025, C, device=dev), keep=None),                            # more rows than a workgroup walks
           dict(keep=keep.bool()), dict(keep=keep.float()), dict(keep=keep[:, :5].contiguous()), dict(keep=keep[:3]),
           dict(bias=torch.zeros(C + 1, device=dev)), dict(residual=torch.zeros(4, C + 1, device=dev)),
           dict(bn=(torch.ones(C + 2, device=dev),) + bn[1:]), dict(bn=bn[:3]),
           dict(a=a.cpu()), dict(bias=torch.zeros(C)), dict(keep=keep.cpu()),
           dict(a=a.double()), dict(a=a.t().contiguous().t()), dict(act="tanh"), dict(keep_prob=0.0), dict(keep_prob=1.5),
           dict(is_training=False)]                                                        # (a mask in eval mode)
    for kw in bad:
        args = dict(a=a, bias=None, residual=None, act="relu", bn=bn, is_training=True, keep=keep, keep_prob=0.8)
        args.update(kw)
        assert not ops.class_filter_ok(**args), kw
        with pytest.raises(LpmError, match="class_filter"):
            ops.class_filter(**args)
    assert torch.equal(bn[2], torch.full((C,), 0.25, device=dev)) and torch.equal(bn[3], torch.full((C,), 2.0, device=dev))
    assert ops.class_filter_ok(a, None, None, "relu", bn, True, keep, 0.8)
    # the C entries check for themselves
    lib = _capi.load()
    y, m, r = torch.empty_like(a), torch.empty(C, device=dev), torch.empty(C, device=dev)

    def fwd(B=4, Cc=C, act=1, gamma=bn[0], mean=m, training=1, keep_t=keep, keep_prob=0.8, decay=0.99):
        return lib._lpm_class_filter_fwd(ptr(a), None, None, B, Cc, act, 0.2, ptr(gamma), ptr(bn[1]), ptr(bn[2]), ptr(bn[3]), training, 1e-3,
                                         decay, ptr(keep_t), keep_prob, ptr(y), ptr(mean), ptr(r), stream_ptr())

    for call in (lambda: fwd(B=1025), lambda: fwd(B=0), lambda: fwd(Cc=0), lambda: fwd(act=0), lambda: fwd(act=4), lambda: fwd(gamma=None),
                 lambda: fwd(mean=None), lambda: fwd(training=0), lambda: fwd(keep_prob=0.0), lambda: fwd(decay=1.5)):
        assert call() != 0 and "lpm_class_filter_fwd" in lib.last_error()
    d = torch.empty_like(a)
    for B, act in ((1025, 1), (4, 7)):
        st = lib._lpm_class_filter_bwd(ptr(a), ptr(a), None, None, B, C, act, 0.2, ptr(bn[0]), ptr(m), ptr(r), 1, ptr(keep), 0.8, ptr(d), None,
                                       ptr(m), ptr(r), stream_ptr())
        assert st != 0 and "lpm_class_filter_bwd" in lib.last_error()
    st = lib._lpm_class_filter_bwd(ptr(a), ptr(a), ptr(bn[1]), None, 4, C, 1, 0.2, None, None, None, 1, None, 1.0, ptr(d), None, None, None,
                                   stream_ptr())
    assert st != 0 and "dbias" in lib.last_error()                   # (a bias without a place for its gradient)
    torch.cuda.synchronize()
    assert torch.equal(bn[2], torch.full((C,), 0.25, device=dev)) and torch.equal(bn[3], torch.full((C,), 2.0, device=dev))


# ---- the whole models on the fused route ---------------------------------------------------------------------------------------------
MB, MF, MV = 6, 36, 37


def _model_batch(seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(MB, MF, generator=g)
    x = x / x.norm(dim=1, keepdim=True)
    y = torch.rand(MB, MV, generator=g) < 0.2
    masks = {"probabilities": (torch.rand(MB, MV, generator=g) < 0.8).to(torch.uint8),
             "filter1": (torch.rand(MB, 2 * MV, generator=g) < 0.8).to(torch.uint8)}
    return x, y, masks


@functools.lru_cache(maxsize=None)
def _model_reference(name, training):
    """fp64 predictions, loss gradients of every trainable variable and new moving statistics, from R.make_variables(MF, MV, 5)"""
    x, y, masks = _model_batch()
    p = {k: v.double().requires_grad_(not k.endswith(("/moving_mean", "/moving_variance"))) for k, v in R.make_variables(MF, MV, 5).items()}
    pred, stats = R.model(name, x.double(), p, training, masks)
    names = [k for k, v in p.items() if v.requires_grad]
    grads = torch.autograd.grad(R.cross_entropy(pred, y), [p[k] for k in names])
    return pred.detach(), dict(zip(names, grads)), {k: v.detach() for k, v in stats.items()}


def _model_on_gpu(name, training, fused, dev):
    """The package's model on the GPU from the same variables -> (predictions, gradients, the store)"""
    from learnablepoolingmethods_amd import FLAGS, losses, registry
    from learnablepoolingmethods_amd import variables as vs
    x, y, masks = _model_batch()
    store = vs.VariableStore(device=dev)
    model = registry.get_model(name)
    saved = FLAGS.class_filter_fused
    FLAGS.class_filter_fused = fused
    try:
        with vs.use_store(store):
            with torch.no_grad(), vs.variable_scope("tower"):      # create the variables, then load the test's values
                model.create_model(x.to(dev), vocab_size=MV, is_training=False)
            store.pop_regularization_losses()
            store.load({"tower/" + k: v for k, v in R.make_variables(MF, MV, 5).items()}, strict=True)
            with vs.variable_scope("tower"):
                pred = model.create_model(x.to(dev), vocab_size=MV, is_training=training, dropout_masks=masks, labels=y.to(dev),
                                          fused_cross_entropy=True)["predictions"]
            store.pop_regularization_losses()
            names = [n for n in store.vars if store.trainable[n]]
            grads = torch.autograd.grad(losses.CrossEntropyLoss().calculate_loss(pred, y.to(dev)), [store.vars[n] for n in names])
    finally:
        FLAGS.class_filter_fused = saved
    return pred.detach(), {n[len("tower/"):]: g for n, g in zip(names, grads)}, store


@pytest.mark.parametrize("training", [True, False], ids=["training", "eval"])
@pytest.mark.parametrize("name", ["MoeModel2", "JuhanMoeModel"])
def test_models_match_fp64_and_the_torch_route(name, training, monkeypatch):
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    calls = []
    real = ops.class_filter
    monkeypatch.setattr(ops, "class_filter", lambda *a, **k: calls.append(k.get("act")) or real(*a, **k))
    pred64, g64, stats64 = _model_reference(name, training)
    pred_f, g_f, store_f = _model_on_gpu(name, training, True, dev)
    act = "relu" if name == "MoeModel2" else "leaky_relu"
    assert calls == [act, act, "sigmoid"] * 2                         # the three glue stages went through the op (twice: the forward
    pred_t, g_t, store_t = _model_on_gpu(name, training, False, dev)  # that creates the variables, then the one compared)
    assert len(calls) == 6                                            # ... and none of them with the flag off
    figures = [("predictions vs fp64", rel_err(pred_f, pred64)), ("predictions vs the torch route", rel_err(pred_f, pred_t))]
    for n in g64:
        figures.append((f"d{n} vs fp64", rel_l2(g_f[n], g64[n])))
        figures.append((f"d{n} vs the torch route", rel_l2(g_f[n], g_t[n])))
    for n, ref in stats64.items():
        figures.append((f"{n} vs fp64", rel_err(store_f.vars["tower/" + n], ref)))
        figures.append((f"{n} vs the torch route", rel_err(store_f.vars["tower/" + n], store_t.vars["tower/" + n])))
    for what, e in figures:
        print(f"[class_filter] {name} {'training' if training else 'eval'} {what}: {e:.3e}")
    assert set(g_f) == set(g64)
    for what, e in figures:
        assert math.isfinite(e) and e <= REL_TOL, f"{name} {what}: {e:.3e} > {REL_TOL:.1e}"


@pytest.mark.parametrize("name", ["MoeModel2", "JuhanMoeModel"])
def test_trainer_step_and_predictor_on_the_fused_route(name, monkeypatch):
    from learnablepoolingmethods_amd import FLAGS, ops, registry
    from learnablepoolingmethods_amd.predictor import Predictor
    from learnablepoolingmethods_amd.train import Trainer
    dev = cuda()
    calls = []
    real = ops.class_filter
    monkeypatch.setattr(ops, "class_filter", lambda *a, **k: calls.append(k.get("is_training")) or real(*a, **k))
    x, y, masks = _model_batch(1)
    nf = torch.ones(MB, dtype=torch.int32)
    saved = FLAGS.class_filter_fused
    FLAGS.class_filter_fused = True
    try:
        tr = Trainer(registry.get_model(name), vocab_size=MV, batch_size=MB, device=dev, seed=1)
        out = tr.step(x, nf, y)                                       # (the masks are drawn: ops.dropout_keep_mask)
        assert tr.global_step == 1 and torch.isfinite(out["loss"]) and torch.isfinite(out["predictions"]).all()
        assert calls[-3:] == [True, True, True]
        before = {n: v.clone() for n, v in tr.store.vars.items()}
        p = tr.predict(x, nf)
        assert calls[-3:] == [False, False, False]
        assert p.shape == (MB, MV) and torch.isfinite(p).all() and ((p >= 0) & (p <= 1)).all()
        assert all(torch.equal(v, before[n]) for n, v in tr.store.vars.items())      # eval mode writes no statistic
        pr = Predictor.from_trainer(tr)
        assert torch.equal(pr.predict(x, nf), p)
        mv = tr.store.vars["tower/batch_normalization/moving_variance"]
        assert bool((mv < 1).all()) and bool((mv > 0.98).all())       # one step of 0.99 old + 0.01 (a small batch variance)
    finally:
        FLAGS.class_filter_fused = saved
