"""-m "not gpu": the triangulation-embedding modules against a numpy fp64 restatement, RegularizedTriangulationModel through the
registry on the CPU, and the C ABI of the fused op (symbols exported, CPU tensors refused).

Trainer.step has no CPU path (its clip + Adam update is a HIP kernel and the project keeps no eager fall-back: see
tests/test_training_host.py), so the CPU check of a training step goes as far as the CPU goes -- build, forward, loss, backward into
the gradient arena, nothing NaN; the update itself is checked on the GPU against fp64 (tests/test_gpu_triangulation.py)."""
import ctypes
import math

import numpy as np
import pytest
import torch


def _np_blocks(x, anchors):
    """[M, D], [D, K] -> [M, K, D]: unit vectors from each anchor to each row (tf.nn.l2_normalize: epsilon inside the max)."""
    r = x[:, None, :] - anchors.T[None, :, :]
    q = (r * r).sum(-1, keepdims=True)
    return r / np.sqrt(np.maximum(q, 1e-12))


def _np_temporal(e, T, K, D):
    """[B*T, K*D] -> [B, T-1, K*D]"""
    e = e.reshape(-1, T, K, D)
    u = e[:, 1:] - e[:, :-1]
    p = (u * u).sum(-1, keepdims=True)
    return (u / np.sqrt(np.maximum(p, 1e-12))).reshape(-1, T - 1, K * D)


def _store_with(anchors64, name="anchor_weights"):
    """A CPU variable store whose anchor variable already exists, in fp64."""
    from learnablepoolingmethods_amd import variables as vs
    store = vs.VariableStore(device="cpu")
    store.vars[name] = torch.from_numpy(anchors64).clone().requires_grad_(True)
    store.trainable[name] = True
    return store


@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(0)
    B, T, D, K = 2, 5, 16, 3
    return B, T, D, K, rng.standard_normal((B * T, D)), rng.standard_normal((D, K)) / math.sqrt(K)


def test_triangulation_embedding_matches_numpy(small):
    from learnablepoolingmethods_amd import variables as vs, video_pooling_modules as M
    B, T, D, K, x, a = small
    with vs.use_store(_store_with(a)):
        out = M.TriangulationEmbedding(D, T, K, True, True).forward(torch.from_numpy(x))
    assert out.shape == (B * T, D * K)
    an = a / np.sqrt(np.maximum((a * a).sum(0, keepdims=True), 1e-12))          # the anchor columns are L2-normalised first
    assert np.abs(out.detach().numpy() - _np_blocks(x, an).reshape(B * T, K * D)).max() < 1e-12


def test_weighted_embedding_is_the_scaled_block_embedding_and_det_reg_is_zero(small):
    from learnablepoolingmethods_amd import variables as vs, video_pooling_modules as M
    B, T, D, K, x, a = small
    with vs.use_store(_store_with(a)):
        out, det_reg = M.WeightedTriangulationEmbedding(D, T, K, True, True).forward(torch.from_numpy(x))
    assert out.shape == (B, T, D * K)
    assert float(det_reg) == 0.0
    blocks = _np_blocks(x, a).reshape(B * T, K * D)                             # anchors NOT normalised
    full = blocks / np.sqrt(np.maximum((blocks * blocks).sum(1, keepdims=True), 1e-12))
    assert np.abs(out.detach().numpy().reshape(B * T, K * D) - full).max() < 1e-12
    assert np.abs(full - blocks / math.sqrt(K)).max() < 1e-12, "the second l2_normalize is a division by sqrt(K)"


def test_embedding_is_k_major(small):
    """Zero frames and anchor k = c_k * onehot(d_k): block k of the row is -onehot(d_k), so element k * D + d comes from anchor k."""
    from learnablepoolingmethods_amd import variables as vs, video_pooling_modules as M
    _, T, D, K, _, _ = small
    a = np.zeros((D, K))
    hot = [3, 11, 6]
    for k, d in enumerate(hot):
        a[d, k] = 2.0 + k
    with vs.use_store(_store_with(a)):
        out = M.TriangulationEmbedding(D, T, K, True, True).forward(torch.zeros(T, D, dtype=torch.float64)).detach().numpy()
    expect = np.zeros((T, K * D))
    for k, d in enumerate(hot):
        expect[:, k * D + d] = -1.0
    assert np.array_equal(out, expect)


def test_temporal_embedding_drops_frame_zero(small):
    from learnablepoolingmethods_amd import video_pooling_modules as M
    B, T, D, K, x, a = small
    e = _np_blocks(x, a).reshape(B * T, K * D) / math.sqrt(K)
    out = M.TriangulationTemporalEmbedding(D, T, K, True, True).forward(torch.from_numpy(e).reshape(B, T, K * D))
    assert out.shape == (B, T - 1, D * K)
    assert np.abs(out.numpy() - _np_temporal(e, T, K, D)).max() < 1e-12
    flat = M.TriangulationTemporalEmbedding(D, T, K, True, True).forward(torch.from_numpy(e))      # [(B*T), K*D] is accepted too
    assert torch.equal(flat, out)


def test_aggregation_modules():
    from learnablepoolingmethods_amd import aggregation_modules as A
    rng = np.random.default_rng(1)
    x = rng.standard_normal((3, 7, 10))
    t = torch.from_numpy(x)
    mm = A.MaxMeanPoolingModule(l2_normalize=False).forward(t).numpy()
    assert mm.shape == (3, 20)
    assert np.array_equal(mm[:, :10], x.max(1)) and np.abs(mm[:, 10:] - x.mean(1)).max() < 1e-15, "[max | mean]"
    mn = A.MaxMeanPoolingModule(l2_normalize=True).forward(t).numpy()
    for half, ref in ((mn[:, :10], x.max(1)), (mn[:, 10:], x.mean(1))):
        assert np.abs(half - ref / np.sqrt((ref * ref).sum(1, keepdims=True))).max() < 1e-12
    assert np.array_equal(A.MaxPoolingModule().forward(t).numpy(), x.max(1))
    assert np.abs(A.MeanPooling().forward(t).numpy() - x.mean(1)).max() < 1e-15
    assert np.abs(A.MeanStdPoolModule(l2_normalize=False).forward(t).numpy() - x.mean(1)).max() < 1e-15      # the mean only, as written
    # the maximum's gradient goes to the first frame that attains it
    tie = torch.zeros(1, 3, 2, dtype=torch.float64, requires_grad=True)
    A.MaxPoolingModule().forward(tie).sum().backward()
    assert torch.equal(tie.grad[0], torch.tensor([[1.0, 1.0], [0.0, 0.0], [0.0, 0.0]], dtype=torch.float64))


# ---- the model through the registry ------------------------------------------------------------------------------------------------
VOCAB, KV, KA, ITER, B, MF = 10, 2, 1, 4, 3, 6
EXPECTED = {                      # name under "tower/" -> shape, as frame_level_models.py:1148-1307 + video_level_models.py:687-714 create them
    "input_bn/beta": (1152,), "input_bn/gamma": (1152,), "input_bn/moving_mean": (1152,), "input_bn/moving_variance": (1152,),
    "video_t_emb/anchor_weights": (1024, KV), "audio_t_emb/anchor_weights": (128, KA),
    "video_projection": (2 * KV * 1024, 1024),
    "video_projection_bn/beta": (1024,), "video_projection_bn/gamma": (1024,), "video_projection_bn/moving_mean": (1024,),
    "video_projection_bn/moving_variance": (1024,),
    "audio_projection": (2 * KA * 128, 128),
    "audio_projection_bn/beta": (128,), "audio_projection_bn/gamma": (128,), "audio_projection_bn/moving_mean": (128,),
    "audio_projection_bn/moving_variance": (128,),
    "temp_projection_1": (2 * KV * 1024 + 2 * KA * 128, 1152),
    "temp_projection_bn/beta": (1152,), "temp_projection_bn/gamma": (1152,), "temp_projection_bn/moving_mean": (1152,),
    "temp_projection_bn/moving_variance": (1152,),
    "dis_projection_2": (1152, 2048),
    "dis_activation_bn/beta": (2048,), "dis_activation_bn/gamma": (2048,), "dis_activation_bn/moving_mean": (2048,),
    "dis_activation_bn/moving_variance": (2048,),
    "temp_projection_2": (1152, 2048),
    "temp_activation_bn/beta": (2048,), "temp_activation_bn/gamma": (2048,), "temp_activation_bn/moving_mean": (2048,),
    "temp_activation_bn/moving_variance": (2048,),
    "fully_connected/weights": (4096, VOCAB), "LayerNorm/beta": (VOCAB,), "LayerNorm/gamma": (VOCAB,),
    "fully_connected_1/weights": (VOCAB, VOCAB), "LayerNorm_1/beta": (VOCAB,), "LayerNorm_1/gamma": (VOCAB,),
    "fully_connected_2/weights": (VOCAB, VOCAB), "fully_connected_2/biases": (VOCAB,),
}


def _batch(seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, MF, 1152, generator=g)
    nf = torch.tensor([6, 4, 5])
    lab = torch.rand(B, VOCAB, generator=g) < 0.3
    return x, nf, lab


def _trainer(seed=0):
    from learnablepoolingmethods_amd import registry
    from learnablepoolingmethods_amd.train import Trainer
    return Trainer(registry.get_model("RegularizedTriangulationModel"), vocab_size=VOCAB, batch_size=B, base_learning_rate=1e-3, device="cpu",
                   seed=seed, model_kwargs=dict(iterations=ITER, video_anchor_size=KV, audio_anchor_size=KA))


def test_flags_and_registry():
    from learnablepoolingmethods_amd import FLAGS, registry, video_level_models
    assert (FLAGS.wtm_video_anchor_size, FLAGS.wtm_audio_anchor_size, FLAGS.triangulation_fused) == (64, 64, True)
    assert (FLAGS.wtm_projection_l1, FLAGS.wtm_projection_l2) == (1e-5, 1.0)
    assert registry.validate_class_name("RegularizedTriangulationModel")
    assert registry.find_class_by_name("ClassLearningThreeNnModel") is video_level_models.ClassLearningThreeNnModel


def test_model_builds_on_the_cpu_with_the_reference_variables():
    x, nf, lab = _batch()
    tr = _trainer()
    tr.build(x, nf, lab)
    got = {n: tuple(v.shape) for n, v in tr.store.vars.items()}
    assert got == {"tower/" + n: s for n, s in EXPECTED.items()}
    assert list(got) == ["tower/" + n for n in EXPECTED], "creation order"
    assert sorted(n for n, t in tr.store.trainable.items() if not t) == sorted("tower/" + n for n in EXPECTED if "moving_" in n)
    a = tr.store.vars["tower/video_t_emb/anchor_weights"]
    assert abs(float(a.detach().std()) - 1 / math.sqrt(KV)) < 0.05, "anchor initialisation: stddev 1 / sqrt(K)"
    pred = tr.predict(x, nf)
    assert pred.shape == (B, VOCAB) and bool(((pred > 0) & (pred < 1)).all())


def test_training_forward_backward_on_the_cpu_is_finite():
    """One Trainer step as far as the CPU goes (the update is a HIP kernel): forward, loss, backward into the arena."""
    x, nf, lab = _batch(1)
    tr = _trainer()
    tr.build(x, nf, lab)
    tr.arena.zero_grad()
    u = torch.rand(B, ITER, generator=torch.Generator().manual_seed(2))
    result, reg_losses = tr._forward(tr._normalize_input(x, nf), nf, lab, frame_uniform=u)
    pred = result["predictions"]
    assert pred.shape == (B, VOCAB) and bool(((pred > 0) & (pred < 1)).all())
    assert float(result["regularization_loss"]) == 0.0, "det_reg is identically 0 as written"
    assert len(reg_losses) == 2 + 2 + 3, "L1 and L2 of the two *_projection_2 weights, L2 of the three classifier layers"
    loss = tr.loss_fn.calculate_loss(pred, lab) + tr.reg_penalty * (result["regularization_loss"] + torch.stack(reg_losses).sum())
    loss.backward()
    tr.arena.collect()
    assert math.isfinite(float(loss.detach()))
    for n in tr.arena.names:
        g = tr.arena.grad_views[n]
        assert bool(torch.isfinite(g).all()), n
        assert float(g.abs().max()) > 0 or n.endswith("/beta"), f"{n}: no gradient arrived"


def test_state_dict_round_trips():
    x, nf, lab = _batch()
    tr = _trainer(seed=0)
    tr.build(x, nf, lab)
    state = tr.state_dict()
    other = _trainer(seed=1)
    other.build(x, nf, lab)
    assert not torch.equal(other.store.vars["tower/video_projection"], tr.store.vars["tower/video_projection"])
    other.load_state_dict(state)
    for n, v in tr.store.vars.items():
        assert torch.equal(other.store.vars[n], v), n
    u = torch.full((B, ITER), 0.5)                      # (the model samples frames at random unless the draws are handed in)
    assert torch.equal(other.predict(x, nf, frame_uniform=u), tr.predict(x, nf, frame_uniform=u))


def test_module_path_equals_scaled_formula_in_the_model():
    """FLAGS.triangulation_fused = False and the CPU take the same (module) path: the flag changes nothing there."""
    from learnablepoolingmethods_amd import FLAGS
    x, nf, lab = _batch()
    tr = _trainer()
    tr.build(x, nf, lab)
    a = tr.predict(x, nf, frame_uniform=torch.full((B, ITER), 0.5))
    FLAGS.triangulation_fused = False
    try:
        b = tr.predict(x, nf, frame_uniform=torch.full((B, ITER), 0.5))
    finally:
        FLAGS.reset()
    assert torch.equal(a, b)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_triangulation_entry_points():
    from learnablepoolingmethods_amd import _build, _capi
    import os
    if not os.path.exists(_capi.LIB_PATH):
        _build.build(verbose=False)
    dll = ctypes.CDLL(_capi.LIB_PATH)
    for name in ("lpm_triangulation_pool_fwd", "lpm_triangulation_pool_bwd", "lpm_triangulation_pool_workspace_bytes"):
        assert hasattr(dll, name) and name in _capi.SIGNATURES
    lib = _capi.load()
    # the backward's workspace: per-(clip, anchor) anchor-gradient partials + at most 8 frame-sized dx partials per clip
    assert lib._lpm_triangulation_pool_workspace_bytes(4, 300, 1024, 64) == 4 * (4 * 64 * 1024 + 4 * 8 * 300 * 1024)
    assert lib._lpm_triangulation_pool_workspace_bytes(512, 300, 128, 64) == 4 * 512 * 64 * 128


def test_op_refuses_cpu_tensors():
    from learnablepoolingmethods_amd import _capi, ops
    with pytest.raises(_capi.LpmError):
        ops.triangulation_pool(torch.zeros(8, 128), torch.zeros(128, 4), 4)
