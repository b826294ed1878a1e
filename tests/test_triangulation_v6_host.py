"""-m "not gpu": TriangulationV6Module and JuhanTestModelV6 on the CPU against the fp64 restatement (tests/_triangulation_v6_ref.py):
pool, head and their gradients, variable names, shapes, order and initialisers, the moving averages, inference mode, flags and registry,
the size check, the model through Trainer, fused_pool's plumbing with the restatement in the op's place, and the C ABI rows."""
import ctypes
import json
import math
import os
import re

import pytest
import torch

from tests import _triangulation_v6_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T, D, K, C, O = 3, 5, 128, 3, 2, 7
J = K * D
VOCAB, ITER, MF = 10, 4, 6
SIZES = dict(video_anchor_size=3, audio_anchor_size=2, video_cluster_size=2, audio_cluster_size=3, video_output_dim=7, audio_output_dim=4)
MODULE_NAMES = ["anchor_weights", "spatial_bn/beta", "spatial_bn/gamma", "spatial_bn/moving_mean", "spatial_bn/moving_variance",
                "one_fc_attention_weight", "alpha", "beta", "hidden_weight", "spatial_pool2_bn/beta", "spatial_pool2_bn/gamma",
                "spatial_pool2_bn/moving_mean", "spatial_pool2_bn/moving_variance"]


def _module(batch_norm=True, is_training=True):
    from learnablepoolingmethods_amd import video_pooling_modules as M
    return M.TriangulationV6Module(feature_size=D, max_frames=T, anchor_size=K, self_attention=False, hidden_layer_size=11, kernel_size=13,
                                   output_dim=O, cluster_size=C, add_relu=True, batch_norm=batch_norm, is_training=is_training)


def _store_from(inp, batch_norm=True, extra=()):
    """A float64 CPU store holding the restatement's inputs under the module's names (leaves that require a gradient)"""
    from learnablepoolingmethods_amd import variables as vs
    store = vs.VariableStore(device="cpu")
    rows = [("anchor_weights", inp["anchors"], True)]
    if batch_norm:
        rows += [("spatial_bn/beta", inp["beta"], True), ("spatial_bn/gamma", inp["gamma"], True),
                 ("spatial_bn/moving_mean", torch.zeros(J, dtype=torch.float64), False),
                 ("spatial_bn/moving_variance", torch.ones(J, dtype=torch.float64), False)]
    rows += [("one_fc_attention_weight", inp["w"], True), ("alpha", inp["alpha"], True), ("beta", inp["shift"], True)]
    for n, v, tr in list(rows) + list(extra):
        store.vars[n] = v.clone().requires_grad_(tr)
        store.trainable[n] = tr
    return store


REF_TO_VAR = {"anchors": "anchor_weights", "gamma": "spatial_bn/gamma", "beta": "spatial_bn/beta", "w": "one_fc_attention_weight",
              "alpha": "alpha", "shift": "beta"}


@pytest.mark.parametrize("batch_norm", [True, False])
def test_pool_and_its_gradients_against_the_restatement(batch_norm):
    from learnablepoolingmethods_amd import variables as vs
    inp = R.make_inputs(B, T, D, K, C, seed=0, w_scale=2.0)
    parts, grads = R.gradients(inp, T, batch_norm)
    store = _store_from(inp, batch_norm)
    x = inp["x"].clone().requires_grad_(True)
    with vs.use_store(store):
        y = _module(batch_norm).pool(x)
    assert y.shape == (B, C * J)
    assert float((y.detach() - parts["y"]).abs().max()) <= 1e-13 * float(parts["y"].abs().max())
    (y * inp["dy"]).sum().backward()
    assert float((x.grad - grads["x"]).abs().max()) <= 1e-12 * float(grads["x"].abs().max())
    for n, var in REF_TO_VAR.items():
        if grads[n] is None:
            assert not batch_norm and n in ("gamma", "beta")
            continue
        g = store.vars[var].grad
        assert float((g - grads[n]).abs().max()) <= 1e-12 * max(float(grads[n].abs().max()), float(grads["dalpha_abs"]) * (n == "alpha")), n
    rows = y.detach().reshape(B * C, J)                          # every cluster's row has norm 1 / sqrt(C)
    assert float((rows.norm(dim=1) - 1 / math.sqrt(C)).abs().max()) < 1e-12


@pytest.mark.parametrize("batch_norm", [True, False])
def test_head_and_its_gradients_against_the_restatement(batch_norm):
    from learnablepoolingmethods_amd import variables as vs
    g = torch.Generator().manual_seed(5)
    y = torch.randn(B, C * J, generator=g, dtype=torch.float64).requires_grad_(True)
    hw = torch.randn(C * J, O, generator=g, dtype=torch.float64)
    g2, b2 = 0.5 + torch.rand(O, generator=g, dtype=torch.float64), 0.1 * torch.randn(O, generator=g, dtype=torch.float64)
    up = torch.randn(B, O, generator=g, dtype=torch.float64)
    extra = [("hidden_weight", hw, True)]
    if batch_norm:
        extra += [("spatial_pool2_bn/beta", b2, True), ("spatial_pool2_bn/gamma", g2, True),
                  ("spatial_pool2_bn/moving_mean", torch.zeros(O, dtype=torch.float64), False),
                  ("spatial_pool2_bn/moving_variance", torch.ones(O, dtype=torch.float64), False)]
    from learnablepoolingmethods_amd import variables as vs2
    store = vs2.VariableStore(device="cpu")
    for n, v, tr in extra:
        store.vars[n], store.trainable[n] = v.clone().requires_grad_(tr), tr
    with vs.use_store(store):
        out = _module(batch_norm).head(y)
    leaves = {"y": y.detach().clone().requires_grad_(True), "hw": hw.clone().requires_grad_(True), "g2": g2.clone().requires_grad_(True),
              "b2": b2.clone().requires_grad_(True)}
    ref = R.head(leaves["y"], leaves["hw"], leaves["g2"], leaves["b2"], batch_norm)
    assert out.shape == (B, O) and float((out - ref).detach().abs().max()) <= 1e-13 * float(ref.detach().abs().max()) and float(out.detach().min()) >= 0
    (out * up).sum().backward()
    (ref * up).sum().backward()
    pairs = [(y.grad, leaves["y"].grad), (store.vars["hidden_weight"].grad, leaves["hw"].grad)]
    if batch_norm:
        pairs += [(store.vars["spatial_pool2_bn/gamma"].grad, leaves["g2"].grad), (store.vars["spatial_pool2_bn/beta"].grad, leaves["b2"].grad)]
    for a, b in pairs:
        assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())


def test_variable_names_shapes_order_and_initialisers():
    from learnablepoolingmethods_amd import variables as vs
    store = vs.VariableStore(device="cpu", seed=1)
    with vs.use_store(store):
        out = _module().forward(torch.randn(B * T, D))
    assert out.shape == (B, O)
    assert list(store.vars) == MODULE_NAMES
    shapes = {n: tuple(v.shape) for n, v in store.vars.items()}
    assert shapes["anchor_weights"] == (D, K) and shapes["one_fc_attention_weight"] == (J, C) and shapes["hidden_weight"] == (C * J, O)
    assert shapes["alpha"] == shapes["beta"] == (1,) and shapes["spatial_bn/gamma"] == (J,) and shapes["spatial_pool2_bn/gamma"] == (O,)
    assert float(store.vars["alpha"].detach()) == 1.0 and float(store.vars["beta"].detach()) == pytest.approx(0.01, rel=1e-6)
    for n in ("anchor_weights", "one_fc_attention_weight", "hidden_weight"):                  # xavier (uniform)
        w = store.vars[n].detach()
        lim = math.sqrt(6.0 / (w.shape[0] + w.shape[1]))
        assert float(w.abs().max()) <= lim and abs(float(w.std()) / (lim / math.sqrt(3)) - 1) < 0.1, n
    assert sorted(n for n, t in store.trainable.items() if not t) == sorted(n for n in MODULE_NAMES if "moving_" in n)
    store = vs.VariableStore(device="cpu", seed=1)
    with vs.use_store(store):
        _module(batch_norm=False).forward(torch.randn(B * T, D))
    assert list(store.vars) == [n for n in MODULE_NAMES if "_bn/" not in n]
    m = _module()
    assert (m.self_attention, m.hidden_layer_size, m.kernel_size, m.add_relu) == (False, 11, 13, True)      # stored, read nowhere


def test_moving_averages_after_one_training_forward_and_inference_on_them():
    from learnablepoolingmethods_amd import layers, variables as vs
    inp = R.make_inputs(B, T, D, K, C, seed=1, w_scale=2.0)
    parts = R.pool(*(inp[n] for n in R.NAMES), T, parts=True)
    store = _store_from(inp)
    with vs.use_store(store):
        _module().pool(inp["x"])
    n = B * T
    mm = (1 - layers.BN_DECAY) * parts["mean"]
    mv = layers.BN_DECAY + (1 - layers.BN_DECAY) * parts["var"] * n / (n - 1)
    assert float((store.vars["spatial_bn/moving_mean"] - mm).abs().max()) <= 1e-15
    assert float((store.vars["spatial_bn/moving_variance"] - mv).abs().max()) <= 1e-15
    stats = (store.vars["spatial_bn/moving_mean"].detach().clone(), store.vars["spatial_bn/moving_variance"].detach().clone())
    with vs.use_store(store):
        y = _module(is_training=False).pool(inp["x"])
    ref = R.pool(*(inp[n] for n in R.NAMES), T, stats=stats)
    assert float((y - ref).detach().abs().max()) <= 1e-13 * float(ref.detach().abs().max())
    assert torch.equal(store.vars["spatial_bn/moving_mean"], stats[0]), "inference leaves the moving averages alone"


def test_flags_and_registry():
    from learnablepoolingmethods_amd import FLAGS, ops, predictor, registry
    assert registry.validate_class_name("JuhanTestModelV6")
    assert registry.find_class_by_name("JuhanTestModelV6").__name__ == "JuhanTestModelV6"
    assert (FLAGS.jtmv6_iteration, FLAGS.jtmv6_add_batch_norm, FLAGS.jtmv6_sample_random_frames, FLAGS.jtmv6_video_anchor_size,
            FLAGS.jtmv6_audio_anchor_size, FLAGS.jtmv6_video_kernel_size, FLAGS.jtmv6_audio_kernel_size, FLAGS.jtmv6_video_hidden,
            FLAGS.jtmv6_video_output_dim, FLAGS.jtmv6_audio_hidden, FLAGS.jtmv6_audio_output_dim, FLAGS.jtmv6_video_cluster_size,
            FLAGS.jtmv6_audio_cluster_size) == (30, True, True, 256, 32, 512, 64, 2048, 4096, 256, 512, 64, 8)
    with open(os.path.join(ROOT, "profiles", "bench_triangulation_v6.json")) as f:
        bench = json.load(f)
    justified = bool(bench["measured"] and bench["fused_not_slower_at_all_three_shapes"])
    assert FLAGS.triangulation_v6_fused is justified, "on only if the benchmark has shown the fused path not slower at all three shapes"
    assert hasattr(ops, "triangulation_onefc_pool")
    assert "JuhanTestModelV6" in predictor.GATHER_Q8_LATER_MODELS


def test_size_check_both_ways_with_a_limit_passed_in():
    from learnablepoolingmethods_amd import frame_level_models as F
    assert F.weight_fits(10, 10) and not F.weight_fits(11, 10)
    nbytes = 4 * 1024 * 256 * 64 * 4096
    assert nbytes == 274877906944                                                         # the 275 GB of the video defaults
    with pytest.raises(ValueError) as e:
        F.check_v6_hidden_weight("video", 1024, 256, 64, 4096, limit=2**37)
    msg = str(e.value)
    assert "video" in msg and "274.9 GB" in msg
    assert all(f in msg for f in ("jtmv6_video_anchor_size", "jtmv6_video_cluster_size", "jtmv6_video_output_dim"))
    assert F.check_v6_hidden_weight("video", 1024, 256, 64, 4096, limit=nbytes) == nbytes
    with pytest.raises(ValueError, match="as much again for its gradient"):             # training holds the gradient beside the weight
        F.check_v6_hidden_weight("video", 1024, 256, 64, 4096, limit=2 * nbytes - 1, is_training=True)
    assert F.check_v6_hidden_weight("video", 1024, 256, 64, 4096, limit=2 * nbytes, is_training=True) == nbytes
    mi355x = 309220868096                                                                 # what the device reports: between the two
    assert F.check_v6_hidden_weight("video", 1024, 256, 64, 4096, limit=mi355x) == nbytes
    with pytest.raises(ValueError, match="video stream"):
        F.check_v6_hidden_weight("video", 1024, 256, 64, 4096, limit=mi355x, is_training=True)
    assert F.check_v6_hidden_weight("audio", 128, 32, 8, 512, limit=10**9) == 4 * 128 * 32 * 8 * 512      # 67 MB: the audio defaults fit


def _batch(seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, MF, 1152, generator=g)
    nf = torch.tensor([6, 4, 5])
    lab = torch.rand(B, VOCAB, generator=g) < 0.3
    return x, nf, lab


def _trainer(seed=0, **kwargs):
    from learnablepoolingmethods_amd import registry
    from learnablepoolingmethods_amd.train import Trainer
    kw = dict(iterations=ITER, **SIZES)
    kw.update(kwargs)
    return Trainer(registry.get_model("JuhanTestModelV6"), vocab_size=VOCAB, batch_size=B, base_learning_rate=1e-3, device="cpu", seed=seed,
                   model_kwargs=kw)


def test_the_video_defaults_raise_before_any_variable_and_the_audio_defaults_do_not():
    """At the flags' defaults the video stream's weight is 256 GiB: on a device of 128 GiB (the limit passed in) the video stream raises,
    and no variable has been created; with the video stream reduced the audio stream's defaults build.  With the host's own memory
    as the limit the same holds wherever the host has less than the weight."""
    x, nf, lab = _batch()
    tr = _trainer(video_anchor_size=None, video_cluster_size=None, video_output_dim=None, memory_limit=2**37)
    with pytest.raises(ValueError, match="video stream's hidden_weight"):
        tr.build(x, nf, lab)
    assert not tr.store.vars
    tr = _trainer(audio_anchor_size=None, audio_cluster_size=None, audio_output_dim=None, memory_limit=2**37)
    tr.build(x, nf, lab)
    assert tuple(tr.store.vars["tower/audio_triangulation_embedding/hidden_weight"].shape) == (32 * 128 * 8, 512)
    tr = _trainer(memory_limit=1000)
    with pytest.raises(ValueError, match="video stream's hidden_weight"):
        tr.build(x, nf, lab)
    from learnablepoolingmethods_amd import frame_level_models as F
    host = F.device_memory_bytes("cpu")
    assert host > 2**20
    if host < 2**38:
        with pytest.raises(ValueError, match="video stream's hidden_weight"):
            _trainer(video_anchor_size=None, video_cluster_size=None, video_output_dim=None).build(x, nf, lab)


def test_model_through_trainer_on_the_cpu():
    x, nf, lab = _batch(1)
    tr = _trainer()
    tr.build(x, nf, lab)
    names = list(tr.store.vars)
    streams = [f"tower/{s}_triangulation_embedding/{n}" for s in ("video", "audio") for n in MODULE_NAMES]
    bn = [f"tower/{s}_bn/{n}" for s in ("video", "audio") for n in ("beta", "gamma", "moving_mean", "moving_variance")]
    assert names[:len(bn) + len(streams)] == bn + streams, "creation order"
    assert tuple(tr.store.vars["tower/fc1_weights"].shape) == (7 + 4, VOCAB)
    tr.arena.zero_grad()
    u = torch.stack([(torch.randperm(int(n), generator=torch.Generator().manual_seed(3))[:ITER].float() + 0.5) / float(n) for n in nf])
    result, reg_losses = tr._forward(tr._normalize_input(x, nf), nf, lab, frame_uniform=u)
    pred = result["predictions"]
    assert pred.shape == (B, VOCAB) and bool(((pred > 0) & (pred < 1)).all()) and not reg_losses
    loss = tr.loss_fn.calculate_loss(pred, lab)
    assert math.isfinite(float(loss.detach()))
    loss.backward()
    tr.arena.collect()
    g = tr.arena.grad_views
    for n in tr.arena.names:
        assert bool(torch.isfinite(g[n]).all()), n
    for scope in ("video_triangulation_embedding", "audio_triangulation_embedding"):
        for n in ("anchor_weights", "one_fc_attention_weight", "alpha", "beta", "hidden_weight", "spatial_bn/gamma"):
            assert float(g[f"tower/{scope}/{n}"].abs().max()) > 0, f"{scope}/{n} receives a gradient"
    assert float(g["tower/video_bn/gamma"].abs().max()) > 0, "the input gradient reaches video_bn"


def test_flags_give_the_sizes_and_the_fused_flag_is_ignored_on_the_cpu():
    from learnablepoolingmethods_amd import FLAGS
    x, nf, lab = _batch()
    FLAGS.jtmv6_video_anchor_size, FLAGS.jtmv6_audio_anchor_size, FLAGS.jtmv6_iteration = 2, 1, 3
    FLAGS.jtmv6_video_cluster_size, FLAGS.jtmv6_audio_cluster_size = 3, 2
    FLAGS.jtmv6_video_output_dim, FLAGS.jtmv6_audio_output_dim = 5, 3
    FLAGS.triangulation_v6_fused = True
    try:
        tr = _trainer(iterations=None, **{k: None for k in SIZES})
        tr.build(x, nf, lab)
        got = {n: tuple(v.shape) for n, v in tr.store.vars.items()}
        assert got["tower/video_triangulation_embedding/hidden_weight"] == (3 * 2 * 1024, 5)
        assert got["tower/audio_triangulation_embedding/one_fc_attention_weight"] == (1 * 128, 2)
        assert got["tower/fc1_weights"] == (5 + 3, VOCAB)
        a = tr.predict(x, nf, frame_uniform=torch.full((B, 3), 0.5))
        assert a.shape == (B, VOCAB) and bool(torch.isfinite(a).all())
    finally:
        FLAGS.reset()


def test_fused_pool_plumbing_with_the_restatement_in_the_ops_place(monkeypatch):
    """fused_pool hands the op the module's variables in the op's order, feeds the moving averages from the statistics it returns by the
    rank-2 rule, and in inference mode passes the moving statistics: with the restatement patched in, it equals ``pool`` throughout."""
    from learnablepoolingmethods_amd import ops, variables as vs
    calls = []

    def fake(x, anchors, gamma, beta, attention_weight, alpha, shift, max_frames, batch_norm=True, stats=None):
        calls.append((batch_norm, stats is not None))
        P = R.pool(x, anchors, gamma, beta, attention_weight, alpha, shift, max_frames, batch_norm, stats, parts=True)
        return P["y"], ((P["mean"].detach(), P["var"].detach()) if batch_norm else None)
    monkeypatch.setattr(ops, "triangulation_onefc_pool", fake)
    inp = R.make_inputs(B, T, D, K, C, seed=2, w_scale=2.0)
    for batch_norm, is_training in ((True, True), (True, False), (False, True)):
        outs, stores = [], []
        for path in ("pool", "fused_pool"):
            store = _store_from(inp, batch_norm)
            if batch_norm and not is_training:
                with torch.no_grad():
                    store.vars["spatial_bn/moving_mean"].add_(0.01)
                    store.vars["spatial_bn/moving_variance"].mul_(1.0 / J)
            with vs.use_store(store):
                outs.append(getattr(_module(batch_norm, is_training), path)(inp["x"]))
            stores.append(store)
        assert float((outs[0] - outs[1]).detach().abs().max()) <= 1e-14, (batch_norm, is_training)
        assert list(stores[0].vars) == list(stores[1].vars), "the same variables in the same order"
        for n in stores[0].vars:
            assert float((stores[0].vars[n] - stores[1].vars[n]).detach().abs().max()) <= 1e-16, n
    assert calls == [(True, False), (True, True), (False, False)]


def test_the_op_refuses_cpu_tensors():
    from learnablepoolingmethods_amd import ops
    from learnablepoolingmethods_amd._capi import LpmError
    with pytest.raises(LpmError, match="no CPU"):
        ops.triangulation_onefc_pool(torch.zeros(4, 128), torch.zeros(128, 2), torch.ones(256), torch.zeros(256), torch.zeros(256, 3),
                                     torch.ones(1), torch.zeros(1), 2)


def test_header_and_ctypes_rows():
    from learnablepoolingmethods_amd import _build, _capi
    names = ["lpm_triangulation_onefc_" + n for n in ("max_clusters", "workspace_bytes", "norms", "stats", "project", "pool", "finish", "dz",
                                                       "bwd")]
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lpm_hip.h")).read(), flags=re.S)
    if not os.path.exists(_capi.LIB_PATH):
        _build.build(verbose=False)
    dll = ctypes.CDLL(_capi.LIB_PATH)
    for n in names:
        assert n in _capi.SIGNATURES and re.search(r"\b" + n + r"\s*\(", txt) and hasattr(dll, n), n
    lib = _capi.load()
    assert lib._lpm_triangulation_onefc_max_clusters() == 64
    assert lib._lpm_triangulation_onefc_workspace_bytes(0, 2, 7, 128, 5, 3) == 2 * 2 * 640 * 4
    assert lib._lpm_triangulation_onefc_workspace_bytes(3, 2, 7, 128, 5, 3) == (2 * 7 * 5 + 2 * 7 + 2 * 640) * 4
    assert lib._lpm_triangulation_onefc_workspace_bytes(0, 0, 7, 128, 5, 3) == 0
    # the shape refusals come before any launch: no device is needed to see them (null pointers are refused first, so hand over non-null ones)
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for B_, T_, D_, K_ in ((1, 0, 128, 1), (1, 321, 128, 1), (1, 2, 256, 1), (0, 2, 128, 1)):
        assert lib._lpm_triangulation_onefc_norms(p, p, B_, T_, D_, K_, p, None) != 0, (B_, T_, D_, K_)
    assert lib._lpm_triangulation_onefc_pool(p, p, p, p, 1, 2, 128, 1, 65, p, None, None) != 0
