"""-m gpu: ops.lstm_layer (csrc/lstm.hip), rnn_modules' two modules and TriangulationRelationalModel on the fused route against the fp64
restatement on the CPU (tests/_lstm_ref.py) -- never against the op itself or the package's torch route.

Tolerance of the op and the modules (the rule of tests/test_gpu_triangulation.py): the restatement evaluated in fp32 torch on the CPU
carries an error err32 against fp64 (maximum absolute error over the maximum absolute fp64 value, per tensor); the op's error must be
<= max(8 err32, 1e-6).  It is taken for outputs, h_last, c_last, dx, dkernel and dbias, with N(0, 1) upstream gradients on all three
results.  Every figure is printed before any is asserted.  The model's bound is the project's model-level 1e-3."""
import functools
import math

import pytest
import torch

from tests import _lstm_ref as R
from tests._util import cuda

pytestmark = pytest.mark.gpu

MIXED = (0, 1, 3, 7, 300)                    # a length of 0, of 1, inside, T itself and far above T in one batch
CASES = [(3, 1, 128, 128, None),
         (2, 5, 256, 128, None),             # In != H
         (5, 7, 128, 384, MIXED),
         (17, 4, 512, 512, None),            # the audio default; B is no multiple of the row tile
         (33, 3, 128, 128, None),            # a second (and a third) row tile
         (2, 30, 1024, 1024, None)]
SEEDS = (0, 1, 2)


def _err(a, ref):
    ref = ref.detach().double().cpu()
    return float((a.detach().double().cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


@functools.lru_cache(maxsize=None)
def _case(B, T, In, H, lengths, seed):
    """The inputs and the fp64 / fp32 CPU results of the restatement, computed once and shared."""
    inputs = R.make_inputs(B, T, In, H, seed, None if lengths is None else torch.tensor(lengths))
    x, kernel, bias, lens, up = inputs
    return inputs, R.layer_and_grads(x, kernel, bias, lens, up, torch.float64), R.layer_and_grads(x, kernel, bias, lens, up, torch.float32)


def _run_op(inputs, dev):
    from learnablepoolingmethods_amd import ops
    x, kernel, bias, lens, up = inputs
    leaves = [t.to(dev).clone().requires_grad_(True) for t in (x, kernel, bias)]
    outs = ops.lstm_layer(*leaves, lens.to(dev))
    grads = torch.autograd.grad(sum((o * u.to(dev)).sum() for o, u in zip(outs, up)), leaves)
    return dict(zip(R.NAMES, [o.detach() for o in outs] + list(grads)))


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("B,T,In,H,lengths", CASES)
def test_lstm_layer_against_fp64(B, T, In, H, lengths, seed):
    dev = cuda()
    inputs, r64, r32 = _case(B, T, In, H, lengths, seed)
    got = _run_op(inputs, dev)
    rows = [(n, _err(got[n], r64[n]), _err(r32[n], r64[n])) for n in R.NAMES]
    for n, e, e32 in rows:
        print(f"[lstm] ({B},{T},{In},{H}) seed {seed} {n}: error {e:.3e}, fp32 evaluation error {e32:.3e}, bound {max(8 * e32, 1e-6):.3e}, "
              f"ratio {e / max(8 * e32, 1e-6):.2f}")
    for n, e, e32 in rows:
        assert got[n].shape == r64[n].shape and bool(torch.isfinite(got[n]).all()), n
        assert e <= max(8 * e32, 1e-6), f"{n}: error {e:.3e} > max(8 x {e32:.3e}, 1e-6)"


@pytest.mark.parametrize("B,T,In,H,lengths", [CASES[2], CASES[3], CASES[5]])
def test_lstm_layer_gives_the_same_bits_twice(B, T, In, H, lengths):
    dev = cuda()
    inputs = _case(B, T, In, H, lengths, 0)[0]
    a, b = _run_op(inputs, dev), _run_op(inputs, dev)
    for n in R.NAMES:
        assert torch.equal(a[n], b[n]), n


def test_masked_steps_are_exactly_zero():
    dev = cuda()
    B, T, In, H, lengths = CASES[2]
    inputs = _case(B, T, In, H, lengths, 1)[0]
    got = _run_op(inputs, dev)
    for b, n in enumerate(lengths):
        n = min(n, T)
        assert float(got["outputs"][b, n:].abs().sum()) == 0.0, f"outputs of row {b} past its length {n}"
        assert float(got["dx"][b, n:].abs().sum()) == 0.0, f"dx of row {b} past its length {n}"
        if n:
            assert float(got["outputs"][b, :n].abs().min()) > 0.0 and float(got["dx"][b, :n].abs().max()) > 0.0
    assert float(got["h_last"][0].abs().max()) == 0.0 and float(got["c_last"][0].abs().max()) == 0.0, "a row of length 0"


def test_op_refuses_what_it_cannot_run():
    from learnablepoolingmethods_amd import _capi, ops
    dev = cuda()
    x, kernel, bias, lens, _ = R.make_inputs(2, 3, 128, 128, 0)
    with pytest.raises(_capi.LpmError):
        ops.lstm_layer(x.to(dev), kernel, bias.to(dev), lens)                                  # a CPU kernel
    with pytest.raises(_capi.LpmError):
        ops.lstm_layer(x.to(dev), kernel[:, :-4].to(dev), bias.to(dev), lens)                  # kernel and bias disagree
    x, kernel, bias, lens, _ = R.make_inputs(2, 3, 16, 64, 0)
    assert not ops.lstm_layer_ok(2, 3, 64)
    with pytest.raises(_capi.LpmError):
        ops.lstm_layer(x.to(dev), kernel.to(dev), bias.to(dev), lens)                          # H = 64: the torch route's


# ---- the modules ------------------------------------------------------------------------------------------------------------------
def _module_run(kind, x, nf, cells, dev, H, L):
    """The module on the GPU with FLAGS.lstm_fused from the given cells -> (its result, the gradients of the kernels and biases)."""
    from learnablepoolingmethods_amd import FLAGS, rnn_modules, variables as vs
    store = vs.VariableStore(device=dev)
    for l, (kernel, bias) in enumerate(cells):
        for n, v in (("kernel", kernel), ("bias", bias)):
            store.vars[R.CELL % l + n] = v.to(dev).clone().requires_grad_(True)
            store.trainable[R.CELL % l + n] = True
    FLAGS.lstm_fused = True
    try:
        with vs.use_store(store):
            module = (rnn_modules.LstmLastHiddenModule(H, L, nf.to(dev), H) if kind == "last"
                      else rnn_modules.LstmConcatAverageModule(H, L, nf.to(dev)))
            out = module.forward(x.to(dev))
    finally:
        FLAGS.reset()
    assert len(store.vars) == 2 * L, "the module read the given variables and created none"
    return out, store


@pytest.mark.parametrize("kind", ["last", "concat"])
def test_two_layer_modules_fused_against_fp64(kind):
    dev = cuda()
    B, T, F, H, L = 3, 5, 256, 128, 2
    g = torch.Generator().manual_seed(11)
    x, nf = torch.randn(B, T, F, generator=g), torch.tensor([5, 0, 3])
    cells = []
    for l in range(L):
        _, kernel, bias, _, _ = R.make_inputs(1, 1, F if l == 0 else H, H, 20 + l)
        cells.append((kernel, bias))
    ref_fn = R.last_hidden if kind == "last" else R.concat_average
    up = torch.randn(ref_fn(x, cells, nf).shape, generator=g)

    def reference(dt):
        leaves = [t.to(dt).clone().requires_grad_(True) for c in cells for t in c]
        out = ref_fn(x.to(dt), list(zip(leaves[0::2], leaves[1::2])), nf)
        return [out.detach()] + list(torch.autograd.grad((out * up.to(dt)).sum(), leaves))
    r64, r32 = reference(torch.float64), reference(torch.float32)
    out, store = _module_run(kind, x, nf, cells, dev, H, L)
    leaves = [store.vars[R.CELL % l + n] for l in range(L) for n in ("kernel", "bias")]
    got = [out.detach()] + list(torch.autograd.grad((out * up.to(dev)).sum(), leaves))
    names = ["result"] + [f"d cell_{l}/{n}" for l in range(L) for n in ("kernel", "bias")]
    rows = [(n, _err(a, b), _err(c, b)) for n, a, b, c in zip(names, got, r64, r32)]
    for n, e, e32 in rows:
        print(f"[lstm] module {kind} {n}: error {e:.3e}, fp32 evaluation error {e32:.3e}, bound {max(8 * e32, 1e-6):.3e}")
    for n, e, e32 in rows:
        assert e <= max(8 * e32, 1e-6), f"{kind} {n}: error {e:.3e} > max(8 x {e32:.3e}, 1e-6)"


# ---- the model --------------------------------------------------------------------------------------------------------------------
MODEL = dict(iterations=6, video_anchor_size=1, audio_anchor_size=2)
MODEL_BOUND = 1e-3


def _model_batch(seed, B=4, MF=8, Vn=20):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, MF, 1152, generator=g)
    xin = x * torch.rsqrt(torch.clamp((x * x).sum(2, keepdim=True), min=1e-12))          # train.normalize_input's formula
    nf = torch.tensor([8, 6, 7, 3])                                                     # (the last clip is shorter than the 6 sampled frames)
    lab = torch.rand(B, Vn, generator=g) < 0.3
    u = torch.rand(B, MODEL["iterations"], generator=g)
    masks = {k: torch.rand(B, R.HIDDEN, generator=g) < 0.5 for k in ("hidden_1", "hidden_2")}
    return x, xin, nf, lab, u, masks


def test_model_fused_against_the_fp64_restatement():
    """B = 4, 6 sampled frames, anchors 1 / 2 (hidden sizes 1024 / 256), vocab 20: predictions, loss and every variable's gradient."""
    from learnablepoolingmethods_amd import FLAGS, losses, registry, variables as vs
    dev = cuda()
    _, xin, nf, lab, u, masks = _model_batch(5)
    init = vs.VariableStore(device="cpu", seed=3)
    with vs.use_store(init), vs.variable_scope("tower"):
        registry.get_model("TriangulationRelationalModel").create_model(xin, num_frames=nf, vocab_size=lab.shape[1], is_training=False,
                                                                        frame_uniform=u, **MODEL)
    init.pop_regularization_losses()
    assert list(init.vars) == ["tower/" + n for n in R.model_variable_shapes(lab.shape[1], 1, 2)]
    g = torch.Generator().manual_seed(6)
    state = {n: v.detach().clone() for n, v in init.vars.items()}
    for n, v in state.items():                                     # the LSTM biases away from their zero start
        if n.endswith("basic_lstm_cell/bias"):
            v.copy_(0.1 * torch.randn(v.shape, generator=g))
    trainable = [n for n in state if init.trainable[n]]

    v64 = {n[len("tower/"):]: state[n].double().requires_grad_(True) for n in trainable}
    p64, loss64 = R.model(v64, xin.double(), nf, u, lab, masks, MODEL["iterations"])
    g64 = dict(zip(v64, torch.autograd.grad(loss64, list(v64.values()))))

    store = vs.VariableStore(device=dev)
    for n, v in state.items():
        store.vars[n] = v.to(dev).clone().requires_grad_(init.trainable[n])
        store.trainable[n] = init.trainable[n]
    FLAGS.lstm_fused = True
    try:
        with vs.use_store(store), vs.variable_scope("tower"):
            result = registry.get_model("TriangulationRelationalModel").create_model(
                xin.to(dev), num_frames=nf.to(dev), vocab_size=lab.shape[1], is_training=True, frame_uniform=u,
                dropout_masks={k: m.to(dev) for k, m in masks.items()}, **MODEL)
        reg = store.pop_regularization_losses()
    finally:
        FLAGS.reset()
    pred = result["predictions"]
    loss = losses.CrossEntropyLoss().calculate_loss(pred, lab.to(dev)) + torch.stack(reg).sum()
    grads = dict(zip(trainable, torch.autograd.grad(loss, [store.vars[n] for n in trainable])))
    rows = [("predictions", _err(pred, p64.detach())), ("loss", _err(loss.reshape(1), loss64.detach().reshape(1)))]
    rows += [("grad " + n, _err(grads[n], g64[n[len("tower/"):]])) for n in trainable]
    for n, e in rows:
        print(f"[lstm] model {n}: error {e:.3e}")
    assert pred.shape == (4, lab.shape[1])
    for n, e in rows:
        assert math.isfinite(e) and e <= MODEL_BOUND, f"model {n}: error {e:.3e} > {MODEL_BOUND:.0e}"


def test_three_trainer_steps_fused_and_not_agree():
    from learnablepoolingmethods_amd import FLAGS, registry
    from learnablepoolingmethods_amd.train import Trainer
    dev = cuda()
    batches = [_model_batch(30 + i) for i in range(3)]
    runs = {}
    for fused in (True, False):
        FLAGS.lstm_fused = fused
        try:
            tr = Trainer(registry.get_model("TriangulationRelationalModel"), vocab_size=20, batch_size=4, base_learning_rate=1e-3, device=dev,
                         seed=3, model_kwargs=MODEL)
            outs = []
            for x, _, nf, lab, u, masks in batches:
                out = tr.step(x.to(dev), nf.to(dev), lab.to(dev), frame_uniform=u, dropout_masks={k: m.to(dev) for k, m in masks.items()})
                outs.append((out["loss"].detach().reshape(1).clone(), out["predictions"].detach().clone()))
            runs[fused] = outs
        finally:
            FLAGS.reset()
    rows = []
    for i, ((la, pa), (lb, pb)) in enumerate(zip(runs[True], runs[False])):
        rows += [(f"step {i} loss", _err(la, lb)), (f"step {i} predictions", _err(pa, pb))]
    for n, e in rows:
        print(f"[lstm] trainer fused against per-step torch, {n}: difference {e:.3e}")
    for n, e in rows:
        assert math.isfinite(e) and e <= MODEL_BOUND, f"{n}: {e:.3e} > {MODEL_BOUND:.0e}"
