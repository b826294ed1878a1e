"""-m gpu: ops.label_loss (csrc/label_loss.hip) against the fp64 restatement of the reference's lines (tests/_label_loss_ref.py).

Bound, per tensor: the op's error, relative to the reference tensor's largest magnitude, is at most
max(8 * err32, 1e-6), err32 being the error of the fp32 torch formulation (losses.HingeLoss / SoftmaxLoss on the CPU) against fp64.
The three figures are printed per case before anything is asserted.

Every input has class 0 set in row 0 and, where B > 1, row 1 without labels."""
import functools
import math

import pytest
import torch

from tests import _label_loss_ref as R
from tests._util import REL_TOL, assert_close, cuda

pytestmark = pytest.mark.gpu

SHAPES = [
    (1, 1),
    (4, 37),          # less than a wave
    (3, 257),         # odd rows start on 4-byte boundaries
    (5, 3862),        # the vocabulary: odd rows start on 8-byte boundaries
    (2, 4096),
    (1100, 16),       # more rows than any one round of workgroups
]
RANGES = {"hinge": [(0.0, 1.0)], "softmax": [(0.0, 1.0), (-30.0, 30.0), (90.0, 100.0)]}     # (90, 100): exp overflows unless the maximum is taken out
CASES = [(kind, lo, hi) for kind in ("hinge", "softmax") for lo, hi in RANGES[kind]]
CLASS_OF = {"hinge": "HingeLoss", "softmax": "SoftmaxLoss"}


def _inputs(B, V, seed, lo, hi):
    g = torch.Generator().manual_seed(seed * 7919 + B * 31 + V)
    p = lo + (hi - lo) * torch.rand(B, V, generator=g)
    y = torch.rand(B, V, generator=g) < min(3.0 / V, 0.5)
    y[0, 0] = True
    if B > 1:
        y[1] = False
    return p, y


def _reference(kind, p, y, b=1.0, upstream=1.0):
    """fp64 loss / gradient and the fp32 torch formulation's (CPU) loss / gradient."""
    from learnablepoolingmethods_amd import losses
    loss64, grad64 = R.BY_NAME[CLASS_OF[kind]](p, y, **({"b": b} if kind == "hinge" else {}), upstream=upstream)
    q = p.clone().requires_grad_(True)
    loss32 = getattr(losses, CLASS_OF[kind])().calculate_loss(q, y, b=b)
    (grad32,) = torch.autograd.grad(loss32, q, torch.tensor(upstream))
    return dict(loss64=loss64, grad64=grad64, loss32=loss32.detach(), grad32=grad32)


@functools.lru_cache(maxsize=None)
def _random_case(kind, B, V, seed, lo, hi, b=1.0, upstream=1.0):
    p, y = _inputs(B, V, seed, lo, hi)
    return p, y, _reference(kind, p, y, b, upstream)


def _run_op(kind, p, y, dev, b=1.0, upstream=1.0):
    from learnablepoolingmethods_amd import ops
    q = p.to(dev).requires_grad_(True)
    loss = ops.label_loss(q, y.to(dev), kind, b=b)
    (grad,) = torch.autograd.grad(loss, q, torch.tensor(upstream, device=dev))
    return loss.detach(), grad


def _err(a, ref):
    ref = ref.double()
    return float((a.detach().double().cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


def _check(tag, loss, grad, ref):
    rows = [("loss", _err(loss, ref["loss64"]), _err(ref["loss32"], ref["loss64"])),
            ("gradient", _err(grad, ref["grad64"]), _err(ref["grad32"], ref["grad64"]))]
    for n, e_op, e32 in rows:
        print(f"[label loss] {tag} {n}: op error {e_op:.3e}, fp32 evaluation error {e32:.3e}, bound {max(8 * e32, 1e-6):.3e}")
    for n, e_op, e32 in rows:
        assert math.isfinite(e_op) and e_op <= max(8 * e32, 1e-6), f"{tag} {n}: op error {e_op:.3e} > max(8 x {e32:.3e}, 1e-6)"


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("kind,lo,hi", CASES)
@pytest.mark.parametrize("B,V", SHAPES)
def test_op_matches_fp64(B, V, kind, lo, hi, seed):
    dev = cuda()
    p, y, ref = _random_case(kind, B, V, seed, lo, hi)
    loss, grad = _run_op(kind, p, y, dev)
    assert loss.shape == () and loss.dtype == torch.float32 and grad.shape == p.shape
    _check(f"{kind} ({B},{V}) in ({lo:g},{hi:g}) seed {seed}", loss, grad, ref)
    if kind == "softmax" and B > 1:                    # the row without labels
        assert torch.equal(grad[1].cpu(), torch.zeros(V))


@pytest.mark.parametrize("b", [1.0, 0.5])
def test_hinge_ties_are_exact(b):
    """p = b on a positive, p = -b on a negative: the margin is exactly 0, the element adds 0 to the loss and takes gradient exactly 0;
    the columns next to them sit a quarter inside the margin."""
    dev = cuda()
    V = 257
    y = torch.zeros(2, V, dtype=torch.bool)
    y[:, ::2] = True
    p = torch.where(y, torch.tensor(b), torch.tensor(-b))                     # every element a tie ...
    p[1, 4:8] = torch.tensor([b - 0.25, -b + 0.25, b + 0.25, -b - 0.25])      # ... but two inside and two outside the margin
    loss, grad = _run_op("hinge", p, y, dev, b=b)
    ref_loss, ref_grad = R.hinge(p, y, b=b)
    assert float(ref_loss) == 0.25 and float(loss) == 0.25
    assert torch.equal(grad.double().cpu(), ref_grad)
    assert int((grad != 0).sum()) == 2 and grad[1, 4] == -0.5 and grad[1, 5] == 0.5


def test_softmax_rows_without_labels_are_exact_zeros():
    dev = cuda()
    p, _ = _inputs(3, 3862, 5, -30.0, 30.0)
    y = torch.zeros(3, 3862, dtype=torch.bool)
    loss, grad = _run_op("softmax", p, y, dev)
    assert float(loss) == 0.0 and torch.equal(grad.cpu(), torch.zeros(3, 3862))


@pytest.mark.parametrize("B,V", [(3, 257), (5, 3862)])
def test_hinge_margin(B, V):
    dev = cuda()
    p, y, ref = _random_case("hinge", B, V, 3, 0.0, 1.0, 0.5)
    loss, grad = _run_op("hinge", p, y, dev, b=0.5)
    _check(f"hinge ({B},{V}) b = 0.5", loss, grad, ref)


@pytest.mark.parametrize("kind,lo,hi", CASES)
def test_upstream_gradient_scales_the_result(kind, lo, hi):
    dev = cuda()
    p, y, ref = _random_case(kind, 5, 3862, 4, lo, hi, 1.0, 0.37)
    loss, grad = _run_op(kind, p, y, dev, upstream=0.37)
    _check(f"{kind} (5,3862) in ({lo:g},{hi:g}) upstream 0.37", loss, grad, ref)


@pytest.mark.parametrize("kind", ["hinge", "softmax"])
def test_slices_of_a_wider_matrix(kind):
    """A column slice (rows not contiguous: the op packs it, and gives the bits of the same values in a tensor of their own) and a row
    slice whose first element is on no 16-byte boundary, the labels' on no 4-byte one (the element-by-element kernels: another walk,
    the same bound)."""
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    p, y, ref = _random_case(kind, 5, 3862, 6, 0.0, 1.0)
    own = _run_op(kind, p, y, dev)
    _check(f"{kind} (5,3862) own tensor", *own, ref)
    wide_p = torch.zeros(5, 3862 + 7, device=dev)
    wide_y = torch.ones(5, 3862 + 7, dtype=torch.bool, device=dev)
    wide_p[:, 3:3 + 3862], wide_y[:, 3:3 + 3862] = p.to(dev), y.to(dev)
    tall_p = torch.zeros(6, 3862, device=dev)
    tall_y = torch.ones(6, 3862, dtype=torch.bool, device=dev)
    tall_p[1:], tall_y[1:] = p.to(dev), y.to(dev)
    assert tall_p[1:].data_ptr() % 16 != 0 and tall_y[1:].data_ptr() % 4 != 0
    for what, (sp, sy) in (("columns", (wide_p[:, 3:3 + 3862], wide_y[:, 3:3 + 3862])), ("rows", (tall_p[1:], tall_y[1:]))):
        q = sp.detach().requires_grad_(True)
        loss = ops.label_loss(q, sy, kind)
        (grad,) = torch.autograd.grad(loss, q)
        _check(f"{kind} (5,3862) slice of {what}", loss, grad, ref)
        if what == "columns":
            assert torch.equal(loss, own[0]) and torch.equal(grad, own[1])


@pytest.mark.parametrize("kind,lo,hi", [("hinge", 0.0, 1.0), ("softmax", -30.0, 30.0)])
def test_two_calls_give_the_same_bits(kind, lo, hi):
    dev = cuda()
    p, y = _inputs(1100, 257, 8, lo, hi)
    a = _run_op(kind, p, y, dev)
    b = _run_op(kind, p, y, dev)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_refusals_come_before_any_launch(lib):
    from learnablepoolingmethods_amd import _capi, ops
    dev = cuda()
    p, y = torch.rand(4, 37, device=dev), torch.rand(4, 37, device=dev) < 0.1
    with pytest.raises(_capi.LpmError, match="CPU tensor"):
        ops.label_loss(p.cpu(), y.cpu(), "hinge")
    with pytest.raises(_capi.LpmError, match="CPU tensor"):
        ops.label_loss(p, y.cpu(), "softmax")
    for dtype in (torch.float64, torch.bfloat16):
        with pytest.raises(_capi.LpmError, match="float32"):
            ops.label_loss(p.to(dtype), y, "hinge")
    for dtype in (torch.float32, torch.int64, torch.int8):
        with pytest.raises(_capi.LpmError, match="bool or uint8"):
            ops.label_loss(p, y.to(dtype), "softmax")
    with pytest.raises(_capi.LpmError, match=r"same non-empty \[B, V\]"):
        ops.label_loss(p, y[:, :36], "hinge")
    with pytest.raises(_capi.LpmError, match=r"same non-empty \[B, V\]"):
        ops.label_loss(p.reshape(-1), y.reshape(-1), "softmax")
    for kind in ("cross_entropy", "Hinge", 3, None):
        with pytest.raises(_capi.LpmError, match="unknown kind"):
            ops.label_loss(p, y, kind)
    assert torch.equal(ops.label_loss(p, y.to(torch.uint8), "hinge"), ops.label_loss(p, y, "hinge"))     # uint8 labels are taken
    # the C entry points refuse as well, with their error codes
    ptr, s = _capi.ptr, _capi.stream_ptr
    state, rows, loss, dp = torch.ones(4, 3, device=dev), torch.empty(4, device=dev), torch.empty((), device=dev), torch.empty_like(p)

    def fwd(kind, B, V, st=state):
        return lib._lpm_label_loss_fwd(kind, ptr(p), ptr(y), B, V, 1.0, ptr(st), ptr(rows), ptr(loss), s())

    def bwd(kind, B, V, st=state):
        return lib._lpm_label_loss_bwd(kind, ptr(p), ptr(y), ptr(st), ptr(torch.ones((), device=dev)), B, V, 1.0, ptr(dp), s())
    for call in (fwd, bwd):
        assert call(3, 4, 37) == -1 and "kind" in lib.last_error()            # LPM_ERR_BADARG
        assert call(0, 4, 37) == -1
        assert call(2, 4, 37, None) == -1 and "row_state" in lib.last_error()
        assert call(1, 0, 37) == -2 and call(2, 4, 0) == -2                   # LPM_ERR_UNSUPPORTED_SHAPE
        assert call(1, 4, 37, None) == 0 and call(2, 4, 37) == 0
    torch.cuda.synchronize()


def _moe_batch():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(8, 40, generator=g)
    y = torch.rand(8, 37, generator=g) < 0.1
    y[:, 0] = True
    y[1] = False
    return x, torch.ones(8, dtype=torch.int32), y


@pytest.fixture
def fused_flag():
    """The classes hand GPU batches to the op whatever the flag's default is."""
    from learnablepoolingmethods_amd import FLAGS
    FLAGS.label_loss_fused = True
    try:
        yield
    finally:
        FLAGS.reset()


@pytest.mark.parametrize("name", ["HingeLoss", "SoftmaxLoss"])
def test_moe_trainer_matches_the_cpu_trainer(name, fused_flag, monkeypatch):
    """Trainer(MoeModel) on [8, 40] inputs, V = 37: three steps with each loss on the GPU (the classes -> ops.label_loss) against the
    same trainer on the CPU (the torch formulation) from the same variables: the losses and the parameters after step 3 at REL_TOL."""
    from learnablepoolingmethods_amd import losses, ops, registry
    from learnablepoolingmethods_amd.train import Trainer
    dev = cuda()
    x, nf, y = _moe_batch()
    kw = dict(vocab_size=37, batch_size=8, base_learning_rate=0.01, seed=1)
    host = Trainer(registry.get_model("MoeModel"), device="cpu", label_loss_fn=getattr(losses, name)(), **kw)
    host.build(x, nf, y)
    tr = Trainer(registry.get_model("MoeModel"), device=dev, label_loss_fn=getattr(losses, name)(), **kw)
    tr.build(x, nf, y)
    tr.load_state_dict(host.state_dict())
    calls = []
    real = ops.label_loss
    monkeypatch.setattr(ops, "label_loss", lambda *a, **k: (calls.append(a[2]), real(*a, **k))[1])
    for step in range(3):
        want, got = host.step(x, nf, y), tr.step(x, nf, y)
        e = assert_close(got["loss"], want["loss"], tol=REL_TOL, what=f"{name} loss at step {step + 1}")
        print(f"[label loss] MoeModel {name} step {step + 1}: loss {float(got['loss']):.6f} (CPU {float(want['loss']):.6f}), error {e:.3e}")
    assert calls == [{"HingeLoss": "hinge", "SoftmaxLoss": "softmax"}[name]] * 3          # the op ran, not the torch formulation
    a, b = tr.state_dict(), host.state_dict()
    for n in sorted(host.store.vars):
        e = assert_close(a[n], b[n], tol=REL_TOL, what=f"{name} {n} after step 3")
        print(f"[label loss] MoeModel {name} {n} after step 3: error {e:.3e}")


@pytest.mark.parametrize("name", ["HingeLoss", "SoftmaxLoss"])
def test_each_loss_behind_a_frame_level_model(name, fused_flag):
    """RegularizedTriangulationModel at the sizes of tests/test_gpu_triangulation.py's model test: one step with each loss gives a
    finite loss and finite gradients that reach the anchors."""
    from oracle import lpm_oracle as O
    from learnablepoolingmethods_amd import losses, registry
    from learnablepoolingmethods_amd.train import Trainer
    dev = cuda()
    V, KV, KA, S, B, MF = 40, 4, 2, 12, 6, 16
    x, nf, lab = O.make_synthetic_batch(B, MF, 1152, V, seed=21, min_frames=S)
    tr = Trainer(registry.get_model("RegularizedTriangulationModel"), vocab_size=V, batch_size=B, base_learning_rate=1e-3, device=dev, seed=3,
                 label_loss_fn=getattr(losses, name)(), model_kwargs=dict(iterations=S, video_anchor_size=KV, audio_anchor_size=KA))
    out = tr.step(x, nf, lab)
    assert math.isfinite(float(out["loss"])) and float(out["loss"]) > 0
    for n in ("tower/video_t_emb/anchor_weights", "tower/audio_t_emb/anchor_weights"):
        g = tr.gradient(n)
        print(f"[label loss] RegularizedTriangulationModel {name} {n}: loss {float(out['loss']):.4f}, max |gradient| {float(g.abs().max()):.3e}")
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0


@pytest.mark.parametrize("name", ["HingeLoss", "SoftmaxLoss"])
def test_evaluate_with_a_loss_over_device_batches(name, fused_flag):
    from learnablepoolingmethods_amd import evaluation, losses, registry
    from learnablepoolingmethods_amd.train import Trainer
    dev = cuda()
    x, nf, y = _moe_batch()
    tr = Trainer(registry.get_model("MoeModel"), vocab_size=37, batch_size=8, device=dev, seed=1)
    tr.build(x, nf, y)
    batches = [(None, x[:3].to(dev), y[:3].to(dev), nf[:3].to(dev)), (None, x[3:].to(dev), y[3:].to(dev), nf[3:].to(dev))]
    info = evaluation.evaluate(tr, batches, top_k=5, label_loss_fn=getattr(losses, name)())
    want = sum(float(R.BY_NAME[name](tr.predict(bx, bn), by)[0]) * bx.shape[0] for _, bx, by, bn in batches) / 8
    print(f"[label loss] evaluate {name}: avg_loss {info['avg_loss']:.8f}, example-weighted fp64 restatement {want:.8f}")
    assert info["num_examples"] == 8 and abs(info["avg_loss"] - want) <= 1e-6 * abs(want)
