"""-m gpu: the indexed frame-prep forms (ops.frame_gather_bn_split, the *_idx kernels) and the five triangulation models on the
reader's uint8 frames.

  * the gather is exact (torch.equal against plain indexing, fp32 and uint8);
  * the q8 forms against the fp32 forms on ops.dequantize_l2_normalize's frames: outputs, moving statistics, dgamma / dbeta -- torch.equal;
  * against a float64 restatement (dequantise, pad, normalise, gather, batch norm) at tests._util.REL_TOL;
  * two runs give the same bits; autograd keeps no fp32 tensor of batch size;
  * model level: Predictor.predict and one Trainer.step on uint8 frames against the normalise-everything route at REL_TOL, with
    ops.dequantize_l2_normalize made to raise on the new route; training.run from TFRecord files.
The index table of every kernel-level case holds a frame drawn twice, an index equal to num_frames[b] (padding: a zero row) and one equal
to max_frames (clamped to the last frame); the clips have 0, 1 and max_frames frames."""
import math
import threading

import pytest
import torch

from learnablepoolingmethods_amd import FLAGS, ops, readers, registry, training
from learnablepoolingmethods_amd._capi import LpmError
from learnablepoolingmethods_amd.predictor import Predictor
from learnablepoolingmethods_amd.train import Trainer, normalize_input

from tests._util import REL_TOL, assert_close, cuda, rel_l2
from tests import test_training_host as H

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

# (B, max_frames, F, Dv, S): B S = 35 crosses a 32-row statistics block; whole blocks; F / 4 = 66 passes the 64-lane stride of the
# inverse-norm wave, with a narrow first stream
SHAPES = [(5, 20, 1152, 1024, 7), (3, 12, 1152, 1024, 32), (4, 9, 264, 8, 5)]
MODELS = ("RegularizedTriangulationModel", "SoftAttentionTriangulationModel", "TriangulationCnnClusterModel", "JuhanTestModelV5",
          "JuhanTestModelV1")


def _quantised(B, MF, F, seed):
    """A reader-like batch on the CPU: uint8 frames, zeros past num_frames; clips of 0, 1 and max_frames frames."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(0, 256, (B, MF, F), generator=g, dtype=torch.uint8)
    nf = torch.randint(0, MF + 1, (B,), generator=g, dtype=torch.int32)
    nf[:3] = torch.tensor([0, 1, MF], dtype=torch.int32)
    t = torch.arange(MF).view(1, -1, 1)
    return torch.where(t < nf.view(-1, 1, 1), q, torch.zeros((), dtype=torch.uint8)), nf


def _table(nf, MF, S, seed):
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, MF, (nf.shape[0], S), generator=g, dtype=torch.int32)
    idx[:, 1] = idx[:, 0]                       # a frame drawn twice
    idx[:, 2] = nf                              # an index equal to num_frames[b]: padding (and max_frames for the full clip)
    idx[:, 3] = MF                              # past the batch: clamped to max_frames - 1
    return idx


def _bn(F, dev, seed):
    g = torch.Generator().manual_seed(seed)
    gamma = (1.0 + 0.2 * torch.randn(F, generator=g)).to(dev).requires_grad_()
    beta = (0.1 * torch.randn(F, generator=g)).to(dev).requires_grad_()
    return gamma, beta, (0.05 * torch.randn(F, generator=g)).to(dev), (0.5 + torch.rand(F, generator=g)).to(dev)


_CASES = {}


def _case(shape):
    """Inputs and the float64 reference of one shape, computed once and shared (nothing below writes to them)."""
    if shape in _CASES:
        return _CASES[shape]
    B, MF, F, Dv, S = shape
    q, nf = _quantised(B, MF, F, seed=B * S + F)
    idx = _table(nf, MF, S, seed=F + S)
    g = torch.Generator().manual_seed(9)
    dys = [torch.randn(B * S, Dv, generator=g), torch.randn(B * S, F - Dv, generator=g)]
    # float64: utils.Dequantize, the reader's zero padding, l2_normalize, the gather, slim.batch_norm with batch statistics
    x = q.double() * (4.0 / 255.0) + (4.0 / 512.0 - 2.0)
    x = torch.where(torch.arange(MF).view(1, -1, 1) < nf.view(-1, 1, 1), x, torch.zeros((), dtype=torch.float64))
    x = x * torch.rsqrt(x.pow(2).sum(2, keepdim=True).clamp_min(1e-12))
    rows = x[torch.arange(B).unsqueeze(1), idx.long().clamp(0, MF - 1)].reshape(B * S, F)
    gamma, beta, mm, mv = (t.detach().double().cpu() for t in _bn(F, "cpu", 5))
    mean, var = rows.mean(0), rows.var(0, unbiased=False)
    xhat = (rows - mean) * torch.rsqrt(var + ops.BN_EPS)
    y = xhat * gamma + beta
    dy = torch.cat(dys, 1).double()
    n = B * S
    ref = dict(outputs=[y[:, :Dv], y[:, Dv:]], dgamma=(dy * xhat).sum(0), dbeta=dy.sum(0),
               moving_mean=mm * ops.BN_DECAY + mean * (1 - ops.BN_DECAY), moving_var=mv * ops.BN_DECAY + var * (n / (n - 1)) * (1 - ops.BN_DECAY),
               eval_outputs=list(((rows - mm) * torch.rsqrt(mv + ops.BN_EPS) * gamma + beta).split([Dv, F - Dv], 1)))
    _CASES[shape] = dict(q=q, nf=nf, idx=idx, dys=dys, ref=ref)
    return _CASES[shape]


def _run(frames, nf, idx, Dv, dys, dev, training=True):
    """One forward (+ backward in training mode) of the op with fresh batch-norm tensors -> everything it produces."""
    F = frames.shape[2]
    gamma, beta, mm, mv = _bn(F, dev, 5)
    kw = dict(quantised_training=True) if frames.dtype == torch.uint8 and training else {}
    assert ops.frame_gather_bn_split_ok(frames, Dv, training, **kw)
    outs = ops.frame_gather_bn_split(frames, nf, idx, gamma, beta, mm, mv, training, Dv, **kw)
    assert all(o.is_contiguous() for o in outs) and [tuple(o.shape) for o in outs] == [(idx.numel(), Dv), (idx.numel(), F - Dv)]
    res = dict(outputs=[o.detach().clone() for o in outs], moving_mean=mm.clone(), moving_var=mv.clone())
    if training:
        torch.autograd.backward(list(outs), [d.to(dev) for d in dys])
        res.update(dgamma=gamma.grad.clone(), dbeta=beta.grad.clone())
    return res


@pytest.mark.parametrize("shape", SHAPES)
def test_the_gather_is_exact(shape):
    dev = cuda()
    B, MF, F, Dv, S = shape
    c = _case(shape)
    q, nf, idx = c["q"].to(dev), c["nf"].to(dev), c["idx"].to(dev)
    assert int(nf.min()) == 0 and int(nf.max()) == MF and bool((idx == nf.view(-1, 1)).any()) and int(idx.max()) == MF
    batch = torch.arange(B, device=dev).unsqueeze(1)
    at = idx.long().clamp(0, MF - 1)
    frames = torch.randn(B, MF, F, generator=torch.Generator().manual_seed(4)).to(dev)
    yv, ya = ops.frame_gather_bn_split(frames, nf, idx, None, None, None, None, True, Dv)
    want = frames[batch, at].reshape(B * S, F)
    assert torch.equal(yv, want[:, :Dv]) and torch.equal(ya, want[:, Dv:])
    for training in (False, True):
        yv, ya = ops.frame_gather_bn_split(q, nf, idx, None, None, None, None, training, Dv, quantised_training=training)
        want = ops.dequantize_l2_normalize(q, nf)[batch, at].reshape(B * S, F)
        assert torch.equal(yv, want[:, :Dv]) and torch.equal(ya, want[:, Dv:])
        padding = (at >= nf.view(-1, 1)).reshape(-1)
        assert bool(padding.any()) and not bool(padding.all())
        assert float(yv[padding].abs().max()) == 0.0 and float(ya[padding].abs().max()) == 0.0
        assert bool((yv[~padding].abs().amax(1) > 0).all())


@pytest.mark.parametrize("shape", SHAPES)
def test_q8_forms_equal_the_fp32_forms_on_dequantised_frames(shape):
    dev = cuda()
    B, MF, F, Dv, S = shape
    c = _case(shape)
    q, nf, idx = c["q"].to(dev), c["nf"].to(dev), c["idx"].to(dev)
    fp32 = ops.dequantize_l2_normalize(q, nf)
    want, got = _run(fp32, nf, idx, Dv, c["dys"], dev), _run(q, nf, idx, Dv, c["dys"], dev)
    for i in range(2):
        assert torch.isfinite(got["outputs"][i]).all() and torch.equal(want["outputs"][i], got["outputs"][i]), f"output {i}"
    for k in ("moving_mean", "moving_var", "dgamma", "dbeta"):
        assert torch.isfinite(got[k]).all() and torch.equal(want[k], got[k]), k
    assert float(got["dgamma"].abs().max()) > 0 and float(got["dbeta"].abs().max()) > 0
    init = _bn(F, dev, 5)
    assert not torch.equal(got["moving_mean"], init[2]) and not torch.equal(got["moving_var"], init[3]), "updated in place"
    want, got = _run(fp32, nf, idx, Dv, None, dev, training=False), _run(q, nf, idx, Dv, None, dev, training=False)
    for i in range(2):
        assert torch.isfinite(got["outputs"][i]).all() and torch.equal(want["outputs"][i], got["outputs"][i]), f"eval output {i}"
    assert torch.equal(got["moving_mean"], init[2]) and torch.equal(got["moving_var"], init[3]), "eval mode leaves the statistics alone"


@pytest.mark.parametrize("shape", SHAPES)
def test_against_float64(shape):
    dev = cuda()
    B, MF, F, Dv, S = shape
    c = _case(shape)
    ref = c["ref"]
    got = _run(c["q"].to(dev), c["nf"].to(dev), c["idx"].to(dev), Dv, c["dys"], dev)
    for i in range(2):
        print(f"[frame gather] {shape} output {i}: {assert_close(got['outputs'][i], ref['outputs'][i], what=f'output {i}'):.3e}")
    for k in ("dgamma", "dbeta", "moving_mean", "moving_var"):
        print(f"[frame gather] {shape} {k}: {assert_close(got[k], ref[k], what=k):.3e}")
    ev = _run(c["q"].to(dev), c["nf"].to(dev), c["idx"].to(dev), Dv, None, dev, training=False)
    for i in range(2):
        print(f"[frame gather] {shape} eval output {i}: {assert_close(ev['outputs'][i], ref['eval_outputs'][i], what=f'eval output {i}'):.3e}")


@pytest.mark.parametrize("shape", SHAPES)
def test_two_runs_give_the_same_bits(shape):
    dev = cuda()
    c = _case(shape)
    args = (c["q"].to(dev), c["nf"].to(dev), c["idx"].to(dev), shape[3], c["dys"], dev)
    a, b = _run(*args), _run(*args)
    for k in ("moving_mean", "moving_var", "dgamma", "dbeta"):
        assert torch.equal(a[k], b[k]), k
    assert all(torch.equal(x, y) for x, y in zip(a["outputs"], b["outputs"]))


def test_autograd_keeps_no_fp32_frames_and_eval_has_no_gradient():
    dev = cuda()
    shape = SHAPES[0]
    B, MF, F, Dv, S = shape
    c = _case(shape)
    q, nf, idx = c["q"].to(dev), c["nf"].to(dev), c["idx"].to(dev)
    gamma, beta, mm, mv = _bn(F, dev, 5)
    with pytest.raises(LpmError, match="eval mode only"):
        ops.frame_gather_bn_split(q, nf, idx, gamma, beta, mm, mv, True, Dv)
    yv, ya = ops.frame_gather_bn_split(q, nf, idx, gamma, beta, mm, mv, True, Dv, quantised_training=True)
    saved = yv.grad_fn.saved_tensors
    assert yv.grad_fn is ya.grad_fn
    assert not any(t.dtype == torch.float32 and t.numel() >= B * MF * F for t in saved)
    assert sorted((str(t.dtype), tuple(t.shape)) for t in saved) == sorted(
        [("torch.uint8", (B, MF, F)), ("torch.int32", (B, S)), ("torch.float32", (B * S,)), ("torch.float32", (F,)), ("torch.float32", (F,))])
    yv, ya = ops.frame_gather_bn_split(q, nf, idx, gamma, beta, mm, mv, False, Dv)
    with pytest.raises(LpmError, match="eval-mode"):
        (yv.sum() + ya.sum()).backward()
    # what the kernels refuse reaches the caller as LpmError: a feature size that is no multiple of four, a table of another batch
    with pytest.raises(LpmError):
        ops.frame_gather_bn_split(torch.zeros(B, MF, 1026, dtype=torch.uint8, device=dev), nf, idx, None, None, None, None, False, 1024)
    with pytest.raises(LpmError, match="frame_index"):
        ops.frame_gather_bn_split(q, nf, idx[:-1], None, None, None, None, False, Dv)
    with pytest.raises(LpmError, match="frame_index"):
        ops.frame_gather_bn_split(q, nf, idx.long(), None, None, None, None, False, Dv)


# ---- model level -----------------------------------------------------------------------------------------------------------------
B_M, MF_M, S_M, V_M = 5, 12, 6, 30
KWARGS = {
    "RegularizedTriangulationModel": dict(video_anchor_size=4, audio_anchor_size=2),
    "SoftAttentionTriangulationModel": dict(video_anchor_size=4, audio_anchor_size=2, video_bottleneck=16, audio_bottleneck=8),
    "TriangulationCnnClusterModel": dict(video_anchor_size=4, audio_anchor_size=2, video_kernel_size=4, audio_kernel_size=2, video_hidden=16,
                                         audio_hidden=8),
    "JuhanTestModelV5": dict(video_anchor_size=3, audio_anchor_size=2, video_kernel_size=4, audio_kernel_size=2, video_hidden=16,
                             audio_hidden=8, video_output_dim=16, audio_output_dim=8),
    "JuhanTestModelV1": dict(video_anchor_size=4, audio_anchor_size=2, video_hidden=16, audio_hidden=8, video_output_dim=16, audio_output_dim=8),
}


def _model_batch(dev):
    """Clips of 6 to 12 frames and draws without repeats (a permutation of each clip's frames): the same frame twice in a row is the
    triangulation embedding's p = 0 case, which no fp32 evaluation holds to 1e-3 (tests/test_gpu_triangulation.py)."""
    g = torch.Generator().manual_seed(23)
    nf = torch.tensor([S_M, MF_M, 9, 7, 11], dtype=torch.int32)
    q = torch.randint(0, 256, (B_M, MF_M, 1152), generator=g, dtype=torch.uint8)
    q = torch.where(torch.arange(MF_M).view(1, -1, 1) < nf.view(-1, 1, 1), q, torch.zeros((), dtype=torch.uint8))
    u = torch.stack([(torch.randperm(int(n), generator=g)[:S_M].float() + 0.5) / float(n) for n in nf])
    lab = torch.zeros(B_M, V_M)
    lab[torch.arange(B_M), torch.randint(0, V_M, (B_M,), generator=g)] = 1.0
    masks = {"fc1": torch.rand(B_M, V_M, generator=g) < 0.5, "fc2": torch.rand(B_M, V_M, generator=g) < 0.5}
    return q.to(dev), nf.to(dev), lab.to(dev), u, masks


def _trainer(name, dev, u, masks):
    kw = dict(iterations=S_M, frame_uniform=u, **KWARGS[name])
    if name == "RegularizedTriangulationModel":
        kw["dropout_masks"] = masks
    torch.manual_seed(0)
    return Trainer(registry.get_model(name), vocab_size=V_M, batch_size=B_M, base_learning_rate=1e-3, device=dev, seed=3, model_kwargs=kw)


def _refuse(*a, **k):
    raise AssertionError("ops.dequantize_l2_normalize called on the route that gathers from the uint8 frames")


@pytest.mark.parametrize("name", MODELS)
def test_models_on_uint8_frames_against_the_normalised_route(name, monkeypatch):
    dev = cuda()
    q, nf, lab, u, masks = _model_batch(dev)
    try:
        # one step from the same seed: FLAGS.train_quantised_frames off (normalise everything, the fp32 route) and on
        off = _trainer(name, dev, u, masks)
        FLAGS.train_quantised_frames = False
        assert not off._quantised_frames(q)
        out_off = off.step(q, nf, lab)
        FLAGS.train_quantised_frames = True
        FLAGS.gather_frames_fused = True
        on = _trainer(name, dev, u, masks)
        assert on._quantised_frames(q) and not on._quantised_frames(q.cpu()) and not on._quantised_frames(q.float())
        assert not on._quantised_frames(torch.zeros(B_M, MF_M, 1026, dtype=torch.uint8, device=dev))
        with monkeypatch.context() as mp:
            mp.setattr(ops, "dequantize_l2_normalize", _refuse)
            out_on = on.step(q, nf, lab)
            # the frozen predictor on the uint8 batch (still no normalise-everything pass) ...
            p_on = Predictor.from_trainer(on)
            pred_q = p_on.predict(q, nf)
        # ... against itself on train.normalize_input's fp32 frames
        pred_f = p_on.predict(normalize_input(q, nf), nf)
        print(f"[frame gather] {name}: predictor uint8 vs fp32 {assert_close(pred_q, pred_f, what='Predictor.predict'):.3e}")
        assert torch.isfinite(pred_q).all() and pred_q.shape == (B_M, V_M)
        print(f"[frame gather] {name}: loss {assert_close(out_on['loss'], out_off['loss'], what='loss'):.3e}, predictions "
              f"{assert_close(out_on['predictions'], out_off['predictions'], what='predictions'):.3e}")
        names = list(on.arena.names)
        assert names == list(off.arena.names) and sorted(on.store.vars) == sorted(off.store.vars)
        # rel_l2 with the floor of the other model-level tests (tests/test_gpu_triangulation.py): the beta of a batch norm that feeds
        # another batch norm has a gradient that is mathematically zero -- fp32 noise over its own norm is no ratio -- so a variable's
        # error is taken relative to at least 1e-4 of the model's gradient scale per element
        gscale = max(float(off.gradient(n).abs().max()) for n in names)
        errs = {n: rel_l2(on.gradient(n), off.gradient(n), floor=1e-4 * gscale * off.gradient(n).numel() ** 0.5) for n in names}
        for n in names:
            print(f"[frame gather] {name}: gradient {n} {errs[n]:.3e}")
        for n in names:
            assert torch.isfinite(on.gradient(n)).all() and errs[n] <= REL_TOL, f"{n}: {errs[n]:.3e}"
        # the input batch norms' moving statistics were updated in place, scope by scope, by the same rule
        stats = [n for n in on.store.vars if n.endswith(("/moving_mean", "/moving_variance")) and n.split("/")[-2] in ("video_bn", "audio_bn", "input_bn")]
        assert len(stats) == {"RegularizedTriangulationModel": 2, "JuhanTestModelV1": 0}.get(name, 4), stats
        for n in stats:
            assert_close(on.store.vars[n], off.store.vars[n], what=n)
            init = 0.0 if n.endswith("moving_mean") else 1.0
            assert float((on.store.vars[n] - init).abs().max()) > 0, f"{n} not updated"
        # FLAGS.gather_frames_fused off: today's route
        FLAGS.gather_frames_fused = False
        plain = _trainer(name, dev, u, masks)
        assert not plain._quantised_frames(q)
        out_plain = plain.step(q, nf, lab)
        assert_close(out_plain["loss"], out_off["loss"], what="loss, flag off")
        assert_close(out_plain["predictions"], out_off["predictions"], what="predictions, flag off")
    finally:
        FLAGS.reset()


def test_willow_and_the_netvlad_models_keep_their_routes():
    dev = cuda()
    q = torch.zeros(6, 40, 1152, dtype=torch.uint8, device=dev)
    try:
        FLAGS.gather_frames_fused = True
        willow = Trainer(registry.get_model("WillowModelReg"), vocab_size=30, batch_size=6, device=dev, seed=3)
        assert not willow._quantised_frames(q)
        FLAGS.gather_frames_fused = False
        v1 = Trainer(registry.get_model("NetVladV1"), vocab_size=30, batch_size=6, device=dev, seed=3)
        assert v1._quantised_frames(q), "the flag is about the triangulation models only"
    finally:
        FLAGS.reset()


def test_training_from_files(tmp_path, monkeypatch):
    """training.run over training_batches(device=cuda) for a triangulation model: no normalise-everything pass, finite losses, no
    reader thread left behind."""
    dev = cuda()
    files = H._full_files(tmp_path, n_files=2, per_file=8)
    reader = readers.YT8MFrameFeatureReader(**H.FULL)
    losses = []
    try:
        monkeypatch.setattr(ops, "dequantize_l2_normalize", _refuse)
        FLAGS.gather_frames_fused = True
        tr = Trainer(registry.get_model("JuhanTestModelV5"), vocab_size=H.V, batch_size=4, base_learning_rate=1e-3, device=dev, seed=3,
                     model_kwargs=dict(iterations=4, **KWARGS["JuhanTestModelV5"]))
        it = reader.training_batches(files, 4, device=dev, num_epochs=None, seed=7)
        out = training.run(tr, it, max_steps=3, log=lambda s: None, on_step=lambda r, b: losses.append(float(r["loss"])))
        assert tr._quantised_frames(next(it)[1])
        it.close()
        assert out["global_step"] == out["steps"] == 3 and len(losses) == 3 and all(math.isfinite(v) for v in losses), losses
        assert not [t for t in threading.enumerate() if t.name.startswith("lpm-")]
    finally:
        FLAGS.reset()
