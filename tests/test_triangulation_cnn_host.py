"""-m "not gpu": TriangulationCnnModule and the pooling modules against the fp64 restatement (tests/_triangulation_cnn_ref.py), the
identity the fused op rests on (pool-then-project = project-then-pool), TriangulationCnnClusterModel through the registry on the CPU
(the module path), the flags and the C ABI of the fused op."""
import ctypes
import math
import os

import pytest
import torch

from tests import _soft_attention_ref as S
from tests import _triangulation_cnn_ref as C
from tests import _triangulation_ref as R

VOCAB, KV, KA, FV, FA, HV, HA, ITER, B, MF = 10, 2, 1, 3, 2, 5, 4, 4, 3, 6


def _case(seed=0, Bc=2, T=5, D=128, K=3, F=4):
    x, anchors, _ = S.make_inputs(Bc, T, D, K, seed)
    cnn_d, cnn_t, up, _ = C.make_weights(Bc, D, K, F, seed)
    return x.double(), anchors.double(), cnn_d.double(), cnn_t.double(), up


def test_cnn_module_shapes_and_variable():
    from learnablepoolingmethods_amd import variables as vs, video_pooling_modules as M
    Bc, T, D, K, F = 2, 5, 128, 3, 4
    x, anchors, cnn_d, _, _ = _case()
    e, f = R.embeddings(x, anchors, T, 1.0)
    store = vs.VariableStore(device="cpu")
    with vs.use_store(store), vs.variable_scope("video_d"):
        module = M.TriangulationCnnModule(D, T, F, K, None, True, "video_d")
        out = module.forward(e.reshape(Bc * T, K * D).float())
    assert list(store.vars) == ["video_d/cnn_weights"] and tuple(store.vars["video_d/cnn_weights"].shape) == (K, F, D)
    w = store.vars["video_d/cnn_weights"].detach()
    assert abs(float(w.std()) * math.sqrt(F * D) - 1) < 0.1, "initialisation: stddev 1 / sqrt(F D)"
    assert out.shape == (Bc, T, K * F)
    # element k * F + j of frame (b, t) is <cnn_weights[k, j], e[b, t, k, :]>
    ref = torch.einsum("btkd,kfd->btkf", e.reshape(Bc, T, K, D), w.double()).reshape(Bc, T, K * F)
    assert float((out.detach().double() - ref).abs().max()) < 1e-6
    assert float((C.conv(e, w.double()) - ref).abs().max()) < 1e-14
    # the temporal module is built with max_frames - 1 and takes the flattened differences
    store.vars["cnn_weights"] = cnn_d.clone()
    store.trainable["cnn_weights"] = True
    with vs.use_store(store):
        out_t = M.TriangulationCnnModule(D, T - 1, F, K, None, True, "video_t").forward(f.reshape(-1, K * D))
    assert out_t.shape == (Bc, T - 1, K * F) and float((out_t - C.conv(f, cnn_d)).abs().max()) < 1e-14


@pytest.mark.parametrize("shape", [(2, 5, 128, 3, 4), (3, 2, 128, 1, 1), (1, 9, 1024, 2, 3)])
def test_pool_then_project_equals_project_then_pool(shape):
    Bc, T, D, K, F = shape
    x, anchors, cnn_d, cnn_t, _ = _case(1, *shape)
    agg_d, agg_t = C.cnn_pool(x, anchors, cnn_d, cnn_t, T)
    m_d, m_t = C.mean_pool(x, anchors, T)
    assert agg_d.shape == agg_t.shape == (Bc, K * F) and m_d.shape == m_t.shape == (Bc, K * D)
    for a, m, cnn in ((agg_d, m_d, cnn_d), (agg_t, m_t, cnn_t)):
        err = float((C.project(m, cnn) - a).abs().max()) / float(a.abs().max())
        assert err <= 1e-12, f"pool-then-project differs from project-then-pool by {err:.3e}"


def test_modules_compose_the_restatement():
    """IndirectClusterMeanPoolModule takes its weights from the [B, T, K*D] embedding and pools the [B, T, K*F] convolution."""
    from learnablepoolingmethods_amd import aggregation_modules as A
    Bc, T, D, K, F = 2, 5, 128, 3, 4
    x, anchors, cnn_d, cnn_t, _ = _case(2)
    e, f = R.embeddings(x, anchors, T, 1.0)
    agg_d, agg_t = C.cnn_pool(x, anchors, cnn_d, cnn_t, T)
    got_d = A.IndirectClusterMeanPoolModule(False).forward(e, C.conv(e, cnn_d))
    got_t = A.MeanStdPoolModule(False).forward(C.conv(f, cnn_t))
    assert got_d.shape == (Bc, K * F) and float((got_d - agg_d).abs().max()) < 1e-14 and float((got_t - agg_t).abs().max()) < 1e-14


def test_flags_and_registry():
    from learnablepoolingmethods_amd import FLAGS, registry
    assert (FLAGS.tccm_iterations, FLAGS.tccm_add_batch_norm, FLAGS.tccm_video_anchor_size, FLAGS.tccm_audio_anchor_size,
            FLAGS.tccm_video_kernel_size, FLAGS.tccm_audio_kernel_size, FLAGS.tccm_video_hidden, FLAGS.tccm_audio_hidden,
            FLAGS.triangulation_cnn_fused) == (200, True, 128, 32, 128, 128, 2048, 256, True)
    assert registry.validate_class_name("TriangulationCnnClusterModel")
    assert not hasattr(FLAGS, "tccm_sample_random_frames")


def _batch(seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, MF, 1152, generator=g)
    nf = torch.tensor([6, 4, 5])
    lab = torch.rand(B, VOCAB, generator=g) < 0.3
    return x, nf, lab


def _trainer(seed=0, **kwargs):
    from learnablepoolingmethods_amd import registry
    from learnablepoolingmethods_amd.train import Trainer
    kw = dict(iterations=ITER, video_anchor_size=KV, audio_anchor_size=KA, video_kernel_size=FV, audio_kernel_size=FA, video_hidden=HV,
              audio_hidden=HA)
    kw.update(kwargs)
    return Trainer(registry.get_model("TriangulationCnnClusterModel"), vocab_size=VOCAB, batch_size=B, base_learning_rate=1e-3, device="cpu",
                   seed=seed, model_kwargs=kw)


def test_model_builds_on_the_cpu_with_the_reference_variables():
    x, nf, lab = _batch()
    tr = _trainer()
    tr.build(x, nf, lab)
    expected = C.model_variable_shapes(VOCAB, KV, KA, FV, FA, HV, HA)
    got = {n: tuple(v.shape) for n, v in tr.store.vars.items()}
    assert got == {"tower/" + n: s for n, s in expected.items()}
    assert list(got) == ["tower/" + n for n in expected], "creation order"
    assert sorted(n for n, t in tr.store.trainable.items() if not t) == sorted("tower/" + n for n in expected if "moving_" in n)
    w = tr.store.vars["tower/video_triangulation_embedding/video_d/cnn_weights"]
    assert abs(float(w.detach().std()) * math.sqrt(FV * 1024) - 1) < 0.1, "cnn_weights initialisation: stddev 1 / sqrt(F D)"


def test_training_step_on_the_cpu_equals_the_restatement():
    """One Trainer step as far as the CPU goes (the clip + Adam update is a HIP kernel without an eager fall-back: see
    tests/test_triangulation_host.py): the module path in training mode against tests/_triangulation_cnn_ref.model_loss in fp64, and a
    backward into the arena that reaches every new variable without NaN."""
    x, nf, lab = _batch(1)
    tr = _trainer()
    tr.build(x, nf, lab)
    tr.arena.zero_grad()
    u = torch.stack([(torch.randperm(int(n), generator=torch.Generator().manual_seed(3))[:ITER].float() + 0.5) / float(n) for n in nf])
    result, reg_losses = tr._forward(tr._normalize_input(x, nf), nf, lab, frame_uniform=u)
    pred = result["predictions"]
    assert result["regularization_loss"] == 0 and len(reg_losses) == 4, "L2 of the four classifier layers"
    p = {n[len("tower/"):]: v.detach().double() for n, v in tr.store.vars.items()}
    ref_pred, ref_label_loss, ref_final = C.model_loss(p, x.double(), nf, lab, u)
    loss = tr.loss_fn.calculate_loss(pred, lab)
    final = loss + tr.reg_penalty * (result["regularization_loss"] + torch.stack(reg_losses).sum())
    assert float((pred.detach().double() - ref_pred).abs().max()) < 1e-4, "fp32 module path against fp64"
    assert abs(float(loss.detach()) - float(ref_label_loss)) < 1e-4 * abs(float(ref_label_loss))
    assert abs(float(final.detach()) - float(ref_final)) < 1e-4 * abs(float(ref_final))
    final.backward()
    tr.arena.collect()
    for n in tr.arena.names:
        assert bool(torch.isfinite(tr.arena.grad_views[n]).all()), n
    g = tr.arena.grad_views
    for n in ("video_triangulation_embedding/anchor_weights", "video_triangulation_embedding/video_d/cnn_weights",
              "audio_triangulation_embedding/audio_t/cnn_weights", "video_hidden", "audio_hidden"):
        assert float(g["tower/" + n].abs().max()) > 0, f"{n} receives a gradient"


def test_eval_mode_and_the_fused_flag_on_the_cpu():
    from learnablepoolingmethods_amd import FLAGS
    x, nf, lab = _batch()
    tr = _trainer()
    tr.build(x, nf, lab)
    u = torch.full((B, ITER), 0.5)
    a = tr.predict(x, nf, frame_uniform=u)
    FLAGS.triangulation_cnn_fused = False
    try:
        b = tr.predict(x, nf, frame_uniform=u)
    finally:
        FLAGS.reset()
    assert a.shape == (B, VOCAB) and torch.equal(a, b) and bool(torch.isfinite(a).all())
    assert bool(((a >= 0) & (a <= 1)).all())


def test_flags_give_the_sizes_and_keywords_override_them():
    from learnablepoolingmethods_amd import FLAGS
    x, nf, lab = _batch()
    FLAGS.tccm_video_anchor_size, FLAGS.tccm_audio_anchor_size = 3, 2
    FLAGS.tccm_video_kernel_size, FLAGS.tccm_audio_kernel_size = 2, 1
    FLAGS.tccm_video_hidden, FLAGS.tccm_audio_hidden, FLAGS.tccm_iterations = 7, 6, 3
    try:
        tr = _trainer(iterations=None, video_anchor_size=None, audio_anchor_size=None, video_kernel_size=None, audio_kernel_size=None,
                      video_hidden=None, audio_hidden=None)
        tr.build(x, nf, lab)
        assert {n: tuple(v.shape) for n, v in tr.store.vars.items()} == {
            "tower/" + n: s for n, s in C.model_variable_shapes(VOCAB, 3, 2, 2, 1, 7, 6).items()}
        tr = _trainer(iterations=None, video_anchor_size=None, audio_anchor_size=None, video_kernel_size=None, audio_kernel_size=None,
                      video_hidden=None, audio_hidden=4)
        tr.build(x, nf, lab)
        assert tuple(tr.store.vars["tower/audio_hidden"].shape) == (2 * 2 * 1, 4)
    finally:
        FLAGS.reset()


def test_library_exports_the_mean_entry_points():
    from learnablepoolingmethods_amd import _build, _capi
    if not os.path.exists(_capi.LIB_PATH):
        _build.build(verbose=False)
    dll = ctypes.CDLL(_capi.LIB_PATH)
    for name in ("lpm_triangulation_mean_gram", "lpm_triangulation_mean_pool_fwd", "lpm_triangulation_mean_dw", "lpm_triangulation_mean_bwd",
                 "lpm_triangulation_mean_workspace_bytes"):
        assert hasattr(dll, name) and name in _capi.SIGNATURES
    lib = _capi.load()
    # bounded workspaces at the model's defaults, B = 16: at most 16 partial Grams per clip (one kind only), per-(clip, anchor) dot
    # products, anchor-gradient partials + at most 16 frame-sized dx partials per clip -- none grows with B * T * K * D
    assert lib._lpm_triangulation_mean_workspace_bytes(0, 16, 200, 1024, 128) == 4 * 16 * 4 * 200 * 200      # 10 tile pairs per clip: 4 slices
    assert lib._lpm_triangulation_mean_workspace_bytes(1, 16, 200, 1024, 128) == 4 * 16 * 128 * 200
    assert lib._lpm_triangulation_mean_workspace_bytes(2, 16, 200, 1024, 128) == 4 * (16 * 128 * 1024 + 16 * 16 * 200 * 1024)
    assert lib._lpm_triangulation_mean_workspace_bytes(0, 512, 64, 128, 16) == 0


def test_ops_refuse_cpu_tensors():
    from learnablepoolingmethods_amd import _capi, ops
    with pytest.raises(_capi.LpmError):
        ops.triangulation_mean_pool(torch.zeros(8, 128), torch.zeros(128, 4), 4)
    with pytest.raises(_capi.LpmError):
        ops.triangulation_cnn_pool(torch.zeros(8, 128), torch.zeros(128, 4), torch.zeros(4, 2, 128), torch.zeros(4, 2, 128), 4)
