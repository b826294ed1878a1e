"""-m gpu: ops.class_rows (csrc/class_rows.hip), FishMoeModel3 and the five class-gating modules on the fused route against the fp64
restatement on the CPU (tests/_class_rows_ref.py) -- never against the op itself.

The bound is tests/test_gpu_class_filter.py's rule: per output and per gradient the restatement evaluated in fp32 torch on the CPU
carries an error err32 against fp64 (maximum absolute error over the maximum absolute reference); the op's error must be
<= max(8 err32, 1e-6).  stats (mean, rstd) falls under the same bound.  A part whose fp64 reference is identically zero must be exactly
zero in the op.  Every figure is printed before any is asserted.  All inputs are drawn in fp32 and widened, so the op and the reference
read the same numbers; every gate argument is constructed at least 0.01 from 0 and from +-6, and that margin (and, from 8 columns on,
the presence of all three pieces of the gate) is asserted on the fp64 restatement before any launch.

Measured on the MI355X: 85 tests in 4.5 s; worst error over bound 0.21, at (2, 64) relu6 + residual + softmax.  (The softmax's backward
as first written, y (dy - sum_j y_j dy_j) with the fp32 y, stood at 5.06 times its bound at (1, 5); the kernel normalises y again in fp64.)"""
import functools
import math

import pytest
import torch

from tests import _class_rows_ref as R
from tests._util import REL_TOL, cuda, rel_err

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 5), (2, 64), (3, 37), (5, 255), (5, 256), (5, 257), (2, 1023), (2, 1025), (1024, 70), (4, 3862), (4, 7724), (2, 16384)]
WORST = {"ratio": 0.0, "what": ""}


def _err(a, ref):
    ref = ref.double()
    return float((a.detach().double().cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


@functools.lru_cache(maxsize=None)
def _case(B, C, form, seed=0, regime=None):
    """-> (fp32 inputs, dy, fp64 outputs and gradients, the fp32 CPU evaluation's); computed once and left unchanged"""
    cfg = R.FORMS[form]
    inp32, dy32 = R.make_rows_inputs(B, C, form, seed, regime)
    ref64 = R.rows_gradients(R.widen(inp32), cfg["phi"], cfg["norm"], dy32.double())
    ref32 = R.rows_gradients(inp32, cfg["phi"], cfg["norm"], dy32)
    return inp32, dy32, ref64, ref32


def _assert_margin(tag, inp32, form):
    t = R.gate_argument(R.widen(inp32))
    m = R.kink_distance(t)
    print(f"[class_rows] {tag}: smallest distance of a gate argument from 0 and +-6 in fp64 {m:.4f}")
    assert m >= 0.009
    phi = R.FORMS[form]["phi"]
    if t.shape[1] >= 8 and phi != "identity":
        s = t if phi == "relu6" else -t
        pieces = [int((s < 0).sum()), int(((s > 0) & (s < 6)).sum()), int((s > 6).sum())]
        print(f"[class_rows] {tag}: elements on the three pieces of {phi}: {pieces}")
        assert min(pieces) > 0


def _run_op(inp32, dy32, form, dev):
    """-> (y, stats, gradients): the autograd op for y and the gradients; for the layer norm one more forward through the C entry for
    stats, whose y must be the op's bit for bit."""
    from learnablepoolingmethods_amd import _capi, ops
    from learnablepoolingmethods_amd._capi import ptr, stream_ptr
    cfg = R.FORMS[form]
    t = {k: v.to(dev).requires_grad_(True) for k, v in inp32.items()}
    names = [n for n in R.GRAD_NAMES if n in t]
    ln = (t["gamma"], t["beta"]) if "gamma" in t else None
    y = ops.class_rows(t["a"], t.get("bias"), t.get("residual"), phi=cfg["phi"], norm=cfg["norm"], ln=ln, eps=R.LN_EPS)
    grads = dict(zip(names, torch.autograd.grad((y * dy32.to(dev)).sum(), [t[n] for n in names])))
    stats = None
    if ln is not None:
        lib = _capi.load()
        B, C = t["a"].shape
        y2, stats = torch.empty_like(y), torch.empty(B, 2, device=dev)
        lib.check(lib._lpm_class_rows_fwd(ptr(t["a"].detach()), ptr(t["bias"].detach() if "bias" in t else None),
                                          ptr(t["residual"].detach() if "residual" in t else None), B, C, ops.CLASS_ROWS_PHIS[cfg["phi"]],
                                          ops.CLASS_ROWS_NORMS[cfg["norm"]], ptr(ln[0].detach()), ptr(ln[1].detach()), R.LN_EPS, ptr(y2),
                                          ptr(stats), stream_ptr()), "fwd")
        assert torch.equal(y2, y.detach())
    return y.detach(), stats, grads


def _check(tag, got, ref64, ref32):
    """got / ref64 / ref32: {name: tensor}.  Every figure is printed before anything is asserted."""
    figures = []
    for n, op in got.items():
        r64, r32 = ref64[n], ref32[n]
        zero = float(r64.abs().max()) == 0.0
        if zero:
            e_op, e32 = float(op.detach().abs().max()), 0.0
            print(f"[class_rows] {tag} {n}: the fp64 reference is identically zero; largest |op| {e_op:.3e}")
        else:
            e_op, e32 = _err(op, r64), _err(r32, r64)
            print(f"[class_rows] {tag} {n}: op error {e_op:.3e}, fp32 evaluation error {e32:.3e}, bound {max(8 * e32, 1e-6):.3e}, "
                  f"ratio {e_op / max(8 * e32, 1e-6):.3f}")
        figures.append((n, zero, e_op, e32))
    worst = max([e_op / max(8 * e32, 1e-6) for _, zero, e_op, e32 in figures if not zero], default=0.0)
    if worst > WORST["ratio"]:
        WORST["ratio"], WORST["what"] = worst, tag
    print(f"[class_rows] {tag}: worst error over bound {worst:.3f} (so far over all cases: {WORST['ratio']:.3f} at {WORST['what']})")
    for n, zero, e_op, e32 in figures:
        if zero:
            assert e_op == 0.0, f"{tag} {n}: must be exactly zero, largest |op| {e_op:.3e}"
        else:
            assert math.isfinite(e_op) and e_op <= max(8 * e32, 1e-6), f"{tag} {n}: op error {e_op:.3e} > max(8 x {e32:.3e}, 1e-6)"


def _compare(tag, inp32, dy32, ref64, ref32, form, dev):
    y, stats, grads = _run_op(inp32, dy32, form, dev)
    (o64, g64), (o32, g32) = ref64, ref32
    got, r64, r32 = {"y": y}, {"y": o64["y"]}, {"y": o32["y"]}
    if stats is not None:
        got["stats"], r64["stats"], r32["stats"] = stats, o64["stats"], o32["stats"]
    for n, g in grads.items():
        got["d" + n], r64["d" + n], r32["d" + n] = g, g64[n], g32[n]
    _check(tag, got, r64, r32)
    return y, stats, grads


@pytest.mark.parametrize("form", list(R.FORMS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rows_match_fp64(shape, form):
    dev = cuda()
    B, C = shape
    inp32, dy32, ref64, ref32 = _case(B, C, form)
    tag = f"{shape} {form}"
    _assert_margin(tag, inp32, form)
    y, stats, grads = _compare(tag, inp32, dy32, ref64, ref32, form, dev)
    assert y.shape == (B, C) and grads["a"].shape == (B, C)
    if R.FORMS[form]["phi"] == "identity" and "residual" in grads:
        assert torch.equal(grads["residual"], grads["a"])               # dpre once: the gradient of a and of the residual alike
    if shape == (1, 1):                                                 # the exact cases: one class
        if R.FORMS[form]["norm"] == "softmax":
            assert float(y) == 1.0 and float(grads["a"]) == 0.0 and float(grads.get("residual", grads["a"])) == 0.0
        if R.FORMS[form]["norm"] == "layer_norm":
            assert torch.equal(y.cpu(), inp32["beta"].view(1, 1)) and float(grads["a"]) == 0.0 and float(grads["gamma"]) == 0.0


def test_layer_norm_offset_regime():
    """|mean| = 1e3 std per row.  The two-pass restatement keeps err32 small; moments from raw sums (E[x^2] - mean^2 in fp32) do not:
    both are checked on the CPU here, before the op runs."""
    dev = cuda()
    B, C = 6, 3862
    inp32, dy32, ref64, ref32 = _case(B, C, "ln", seed=1, regime="offset")
    _assert_margin("offset ln", inp32, "ln")
    o64, o32 = ref64[0], ref32[0]
    ratio = float((o64["stats"][:, 0].abs() * o64["stats"][:, 1]).min())
    e32 = _err(o32["y"], o64["y"])
    pre32 = o32["pre"]
    raw_var = (pre32 * pre32).mean(1, keepdim=True) - pre32.mean(1, keepdim=True) ** 2          # what a raw-moment kernel would hold
    y_raw = (pre32 - pre32.mean(1, keepdim=True)) / torch.sqrt(raw_var.clamp_min(0) + R.LN_EPS) * inp32["gamma"] + inp32["beta"]
    e_raw = _err(y_raw, o64["y"])
    print(f"[class_rows] offset ln: smallest |mean| / std {ratio:.1f}; y: fp32 two-pass error {e32:.3e}, fp32 raw-moment error {e_raw:.3e}")
    assert ratio >= 1000 and e32 <= 1e-3 and e_raw > max(8 * e32, 1e-6)
    _compare("offset ln", inp32, dy32, ref64, ref32, "ln", dev)


@pytest.mark.parametrize("form", ["softmax", "p_gate_softmax"])
@pytest.mark.parametrize("regime", ["shift", "spread"])
def test_softmax_regimes(form, regime):
    """shift: every score of a row + 1e3 (the row maximum is taken out before the exponential); spread: the scores of a row span 200,
    so that some probabilities underflow to exactly 0 in fp32 while fp64 still holds them."""
    dev = cuda()
    B, C = 6, 3862
    inp32, dy32, ref64, ref32 = _case(B, C, form, seed=2, regime=regime)
    tag = f"{regime} {form}"
    _assert_margin(tag, inp32, form)
    pre64 = ref64[0]["pre"]
    if regime == "shift":
        assert float(pre64.min()) >= 990
    else:
        span = float((pre64.max(1).values - pre64.min(1).values).min())
        zeros32, zeros64 = int((ref32[0]["y"] == 0).sum()), int((ref64[0]["y"] == 0).sum())
        print(f"[class_rows] {tag}: smallest span of a row {span:.1f}; probabilities that are exactly 0: {zeros32} in fp32, {zeros64} in fp64")
        assert span >= 150 and zeros32 > 0 and zeros64 == 0
    y, _, _ = _compare(tag, inp32, dy32, ref64, ref32, form, dev)
    assert torch.isfinite(y).all() and float((y.sum(1) - 1).abs().max()) < 1e-5


def test_two_runs_give_the_same_bits():
    dev = cuda()
    for form, shape in (("ln", (5, 257)), ("softmax", (4, 3862)), ("n_gate_softmax", (1024, 70)), ("p_gate", (2, 1025))):
        inp32, dy32, _, _ = _case(*shape, form)
        a = _run_op(inp32, dy32, form, dev)
        b = _run_op(inp32, dy32, form, dev)
        assert torch.equal(a[0], b[0]), form
        assert (a[1] is None and b[1] is None) or torch.equal(a[1], b[1]), form
        for n in a[2]:
            assert torch.equal(a[2][n], b[2][n]), (form, n)


def test_refusals_before_any_launch():
    from learnablepoolingmethods_amd import _capi, ops
    from learnablepoolingmethods_amd._capi import LpmError, ptr, stream_ptr
    dev = cuda()
    C = 6
    a = torch.randn(4, C, device=dev)
    ln = (torch.ones(C, device=dev), torch.zeros(C, device=dev))
    other = torch.device("cuda", 1) if torch.cuda.device_count() > 1 else None
    bad = [dict(a=a.cpu()), dict(bias=torch.zeros(C)), dict(residual=torch.zeros(4, C)), dict(ln=(ln[0].cpu(), ln[1])),
           dict(a=a.t().contiguous().t()), dict(residual=torch.zeros(C, 4, device=dev).t()),
           dict(a=a.double()), dict(bias=torch.zeros(C, device=dev, dtype=torch.float16)), dict(ln=(ln[0], ln[1].double())),
           dict(a=torch.randn(4, C, 1, device=dev)), dict(bias=torch.zeros(C + 1, device=dev)), dict(residual=torch.zeros(3, C, device=dev)),
           dict(ln=(torch.ones(C + 2, device=dev), ln[1])), dict(ln=(ln[0],)), dict(ln=None), dict(norm="softmax"),   # (gamma, beta given)
           dict(a=torch.randn(1025, C, device=dev), residual=None), dict(a=torch.randn(2, 16385, device=dev), residual=None, bias=None, ln=None,
                                                                        norm="softmax"),
           dict(phi="relu"), dict(phi=2), dict(norm="batch_norm"), dict(eps=0.0)]
    if other is not None:
        bad.append(dict(bias=torch.zeros(C, device=other)))
    for kw in bad:
        args = dict(a=a, bias=torch.zeros(C, device=dev), residual=torch.zeros(4, C, device=dev), phi="identity", norm="layer_norm", ln=ln,
                    eps=R.LN_EPS)
        args.update(kw)
        assert not ops.class_rows_ok(**args), kw
        with pytest.raises(LpmError, match="class_rows"):
            ops.class_rows(**args)
    assert ops.class_rows_ok(a, None, None, "identity", "layer_norm", ln)
    assert ops.class_rows_ok(torch.randn(1024, C, device=dev), norm="softmax") and ops.class_rows_ok(torch.randn(1, 16384, device=dev))
    # the C entries check for themselves; the output buffers stay as they were
    lib = _capi.load()
    y, st = torch.full_like(a, 7.0), torch.full((4, 2), 7.0, device=dev)

    def fwd(a_t=a, B=4, Cc=C, phi=1, norm=3, gamma=ln[0], beta=ln[1], eps=1e-12, y_t=y, stats=st):
        return lib._lpm_class_rows_fwd(ptr(a_t), None, None, B, Cc, phi, norm, ptr(gamma), ptr(beta), eps, ptr(y_t), ptr(stats), stream_ptr())

    for call in (lambda: fwd(a_t=None), lambda: fwd(y_t=None), lambda: fwd(phi=0), lambda: fwd(phi=4), lambda: fwd(norm=0), lambda: fwd(norm=4),
                 lambda: fwd(B=0), lambda: fwd(B=1025), lambda: fwd(Cc=0), lambda: fwd(Cc=16385), lambda: fwd(gamma=None),
                 lambda: fwd(beta=None), lambda: fwd(stats=None), lambda: fwd(norm=2), lambda: fwd(norm=1, beta=None), lambda: fwd(eps=0.0),
                 lambda: fwd(eps=-1.0)):
        assert call() != 0 and "lpm_class_rows_fwd" in lib.last_error()
    d, dg, db = torch.full_like(a, 7.0), torch.full((C,), 7.0, device=dev), torch.full((C,), 7.0, device=dev)

    def bwd(dy=a, B=4, Cc=C, phi=1, norm=3, bias=None, residual=None, y_t=None, gamma=ln[0], stats=st, da=d, dres=None, dbias=None,
            dgamma=dg, dbeta=db):
        return lib._lpm_class_rows_bwd(ptr(dy), ptr(a), ptr(bias), ptr(residual), ptr(y_t), B, Cc, phi, norm, ptr(gamma), ptr(stats), ptr(da),
                                       ptr(dres), ptr(dbias), ptr(dgamma), ptr(dbeta), stream_ptr())

    for call in (lambda: bwd(dy=None), lambda: bwd(da=None), lambda: bwd(phi=7), lambda: bwd(norm=0), lambda: bwd(B=1025), lambda: bwd(Cc=16385),
                 lambda: bwd(gamma=None), lambda: bwd(stats=None), lambda: bwd(dgamma=None), lambda: bwd(norm=2, y_t=a), lambda: bwd(norm=2,
                 gamma=None, dgamma=None, dbeta=None), lambda: bwd(bias=ln[1]), lambda: bwd(dbias=db), lambda: bwd(dres=d)):
        assert call() != 0 and "lpm_class_rows_bwd" in lib.last_error()
    assert bwd(bias=ln[1]) != 0 and "dbias" in lib.last_error()       # (a bias without a place for its gradient)
    torch.cuda.synchronize()
    for t in (y, st, d, dg, db):
        assert bool((t == 7.0).all())


# ---- the whole model and the modules on the fused route --------------------------------------------------------------------------------
MB, MF, MV = 6, 36, 37
SUBJECTS = ["FishMoeModel3"] + list(R.MODULES)


def _shapes(name):
    return R.fish_moe3_variables(MF, MV) if name == "FishMoeModel3" else {n: s(MV) for n, s in R.MODULES[name][1].items()}


def _restatement(name, x, p, training):
    return R.fish_moe3(x, p, training) if name == "FishMoeModel3" else R.MODULES[name][0](x, p, training)


def _batch(name, seed):
    g = torch.Generator().manual_seed(seed)
    if name == "FishMoeModel3":
        x = torch.randn(MB, MF, generator=g)
        x = x / x.norm(dim=1, keepdim=True)
    else:
        x = torch.rand(MB, MV, generator=g)                             # (probabilities)
    return x, torch.rand(MB, MV, generator=g) < 0.2


@functools.lru_cache(maxsize=None)
def _seed(name):
    """the first seed at which no relu / relu6 argument of the fp64 restatement is nearer than 1e-5 to a kink (chosen on the CPU)"""
    for seed in range(32):
        x, _ = _batch(name, seed)
        p = {k: v.double() for k, v in R.make_variables(_shapes(name), seed + 100).items()}
        if min(_restatement(name, x.double(), p, training)[2] for training in (True, False)) >= 1e-5:
            return seed
    raise AssertionError(f"{name}: no seed keeps the kinks at a distance")


@functools.lru_cache(maxsize=None)
def _reference(name, training):
    """fp64 output, loss gradients of every trainable variable and new moving statistics"""
    seed = _seed(name)
    x, y = _batch(name, seed)
    p = {k: v.double().requires_grad_(not R.is_statistic(k)) for k, v in R.make_variables(_shapes(name), seed + 100).items()}
    pred, stats, kink = _restatement(name, x.double(), p, training)
    print(f"[class_rows] {name} {'training' if training else 'eval'}: seed {seed}, smallest distance of a relu / relu6 argument from a "
          f"kink {kink:.3e}")
    assert kink >= 1e-5
    names = [k for k, v in p.items() if v.requires_grad]
    grads = torch.autograd.grad(R.cross_entropy(pred, y), [p[k] for k in names])
    return pred.detach(), dict(zip(names, grads)), stats


def _build(name, x, training):
    from learnablepoolingmethods_amd import attention_modules, registry
    if name == "FishMoeModel3":
        return registry.get_model(name).create_model(x, vocab_size=MV, is_training=training)["predictions"]
    return getattr(attention_modules, name)(MV, training).forward(x)


def _on_gpu(name, training, fused, dev):
    """The package's model / module on the GPU from the same variables -> (output, gradients, the store)"""
    from learnablepoolingmethods_amd import FLAGS, losses
    from learnablepoolingmethods_amd import variables as vs
    seed = _seed(name)
    x, y = _batch(name, seed)
    store = vs.VariableStore(device=dev)
    saved = FLAGS.class_rows_fused, FLAGS.class_filter_fused
    FLAGS.class_rows_fused = FLAGS.class_filter_fused = fused
    try:
        with vs.use_store(store):
            with torch.no_grad(), vs.variable_scope("tower"):          # create the variables, then load the test's values
                _build(name, x.to(dev), False)
            store.pop_regularization_losses()
            store.load({"tower/" + k: v for k, v in R.make_variables(_shapes(name), seed + 100).items()}, strict=True)
            with vs.variable_scope("tower"):
                pred = _build(name, x.to(dev), training)
            store.pop_regularization_losses()
            names = [n for n in store.vars if store.trainable[n]]
            grads = torch.autograd.grad(losses.CrossEntropyLoss().calculate_loss(pred, y.to(dev)), [store.vars[n] for n in names])
    finally:
        FLAGS.class_rows_fused, FLAGS.class_filter_fused = saved
    return pred.detach(), {n[len("tower/"):]: g for n, g in zip(names, grads)}, store


CALLS = {  # what one forward sends through the two ops with the flags on
    "FishMoeModel3": [("filter", "leaky_relu"), ("filter", "relu"), ("rows", "identity", "layer_norm"), ("filter", "leaky_relu"),
                      ("rows", "identity", "softmax")],
    "PnGateModule": [("rows", "relu6", "none"), ("rows", "neg_relu6", "softmax")],
    "NpGateModule": [("rows", "neg_relu6", "none"), ("rows", "relu6", "softmax")],
    "PGateModule": [("rows", "relu6", "softmax")],
    "CorNNGateModule": [("filter", "relu"), ("filter", "relu"), ("filter", "sigmoid")],
    "ContextGateV1": [],
}


def _record_calls(monkeypatch):
    from learnablepoolingmethods_amd import ops
    calls = []
    rows, filt = ops.class_rows, ops.class_filter
    monkeypatch.setattr(ops, "class_rows", lambda *a, **k: calls.append(("rows", k.get("phi"), k.get("norm"))) or rows(*a, **k))
    monkeypatch.setattr(ops, "class_filter", lambda *a, **k: calls.append(("filter", k.get("act"))) or filt(*a, **k))
    return calls


@pytest.mark.parametrize("training", [True, False], ids=["training", "eval"])
@pytest.mark.parametrize("name", SUBJECTS)
def test_model_and_modules_match_fp64_and_the_torch_route(name, training, monkeypatch):
    dev = cuda()
    calls = _record_calls(monkeypatch)
    pred64, g64, stats64 = _reference(name, training)
    pred_f, g_f, store_f = _on_gpu(name, training, True, dev)
    assert calls == CALLS[name] * 2                                    # (twice: the forward that creates the variables, then the one
    pred_t, g_t, store_t = _on_gpu(name, training, False, dev)         # compared) ... and nothing with the flags off
    assert len(calls) == 2 * len(CALLS[name])
    figures = [("output vs fp64", rel_err(pred_f, pred64)), ("output vs the torch route", rel_err(pred_f, pred_t))]
    for n in g64:
        figures.append((f"d{n} vs fp64", R.gradient_error(n, g_f[n], g64[n], g64, training)))       # (R.CANCELLING: dLayerNorm/beta)
        figures.append((f"d{n} vs the torch route", R.gradient_error(n, g_f[n], g_t[n], g64, training)))
    for n, ref in stats64.items():
        figures.append((f"{n} vs fp64", rel_err(store_f.vars["tower/" + n], ref)))
        figures.append((f"{n} vs the torch route", rel_err(store_f.vars["tower/" + n], store_t.vars["tower/" + n])))
    for what, e in figures:
        print(f"[class_rows] {name} {'training' if training else 'eval'} {what}: {e:.3e}")
    assert set(g_f) == set(g64)
    assert set(stats64) == ({n for n in _shapes(name) if R.is_statistic(n)} if training else set())
    for what, e in figures:
        assert math.isfinite(e) and e <= REL_TOL, f"{name} {what}: {e:.3e} > {REL_TOL:.1e}"


def test_trainer_step_and_predictor_on_the_fused_route(monkeypatch):
    from learnablepoolingmethods_amd import FLAGS, registry
    from learnablepoolingmethods_amd.predictor import Predictor
    from learnablepoolingmethods_amd.train import Trainer
    dev = cuda()
    calls = _record_calls(monkeypatch)
    x, y = _batch("FishMoeModel3", 1)
    nf = torch.ones(MB, dtype=torch.int32)
    saved = FLAGS.class_rows_fused, FLAGS.class_filter_fused
    FLAGS.class_rows_fused = FLAGS.class_filter_fused = True
    try:
        tr = Trainer(registry.get_model("FishMoeModel3"), vocab_size=MV, batch_size=MB, device=dev, seed=1)
        out = tr.step(x, nf, y)
        assert tr.global_step == 1 and torch.isfinite(out["loss"]) and torch.isfinite(out["predictions"]).all()
        assert calls[-5:] == CALLS["FishMoeModel3"]
        before = {n: v.clone() for n, v in tr.store.vars.items()}
        n_calls = len(calls)
        p = tr.predict(x, nf)
        assert calls[n_calls:] == CALLS["FishMoeModel3"]
        assert p.shape == (MB, MV) and torch.isfinite(p).all() and ((p >= 0) & (p <= 1)).all()
        assert float((p.sum(1) - 1).abs().max()) < 1e-5                # a softmax over the vocabulary
        assert all(torch.equal(v, before[n]) for n, v in tr.store.vars.items())      # eval mode writes no statistic
        pr = Predictor.from_trainer(tr)
        assert torch.equal(pr.predict(x, nf), p)
        mv = tr.store.vars["tower/batch_normalization/moving_variance"]
        assert bool((mv < 1).all()) and bool((mv > 0.98).all())        # one step of 0.99 old + 0.01 (a small batch variance)
    finally:
        FLAGS.class_rows_fused, FLAGS.class_filter_fused = saved
