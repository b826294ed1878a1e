"""-m "not gpu": FishMoeModel3 and the five class-gating modules of attention_modules on the CPU device (the torch formulation of the
row-wise glue) -- the registry, tf.layers' and slim's variable names, Trainer.step / predict / Predictor, the no-op dropout, the moving
statistics against the restatement (tests/_class_rows_ref.py), the C table, and
``python -m learnablepoolingmethods_amd.training --frame_features false --model FishMoeModel3`` from two tiny files, with a resume."""
import numpy as np
import pytest
import torch

from learnablepoolingmethods_amd import FLAGS, _capi, attention_modules, layers, ops, readers, registry, training, video_level_models
from learnablepoolingmethods_amd import variables as vs
from learnablepoolingmethods_amd._capi import LpmError
from learnablepoolingmethods_amd.predictor import Predictor
from learnablepoolingmethods_amd.train import Trainer, normalize_input
from tests import _class_rows_ref as R
from tests._util import REL_TOL, rel_err

B, F, V = 6, 36, 11


def _batch(seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, F, generator=g)
    y = torch.rand(B, V, generator=g) < 0.2
    return x, torch.ones(B, dtype=torch.int32), y


def _variables(tr):
    return {n[len("tower/"):]: v.detach().clone() for n, v in tr.store.vars.items()}


def test_registry_finds_the_model():
    assert registry.find_class_by_name("FishMoeModel3") is video_level_models.FishMoeModel3
    assert registry.validate_class_name("FishMoeModel3")
    assert type(registry.get_model("FishMoeModel3")).__name__ == "FishMoeModel3"


def test_both_entries_are_in_the_c_table():
    assert len(_capi.SIGNATURES["lpm_class_rows_fwd"][1]) == 13 and len(_capi.SIGNATURES["lpm_class_rows_bwd"][1]) == 17
    assert sorted(ops.CLASS_ROWS_PHIS) == ["identity", "neg_relu6", "relu6"] and sorted(ops.CLASS_ROWS_NORMS) == ["layer_norm", "none", "softmax"]
    lib = _capi.load()
    assert lib._lpm_class_rows_fwd(None, None, None, 1, 1, 1, 1, None, None, 1e-12, None, None, None) != 0
    assert "lpm_class_rows_fwd" in lib.last_error() and "null pointer" in lib.last_error()


def test_variable_names_shapes_order_and_trainability():
    x, nf, y = _batch()
    tr = Trainer(registry.get_model("FishMoeModel3"), vocab_size=V, batch_size=B, device="cpu", seed=1)
    tr.build(x, nf, y)
    want = R.fish_moe3_variables(F, V)
    assert [(n, tuple(v.shape)) for n, v in tr.store.vars.items()] == [("tower/" + n, s) for n, s in want.items()]
    for n in want:
        assert tr.store.trainable["tower/" + n] == (not R.is_statistic(n)), n
    for n in want:                                           # the dry run of build() leaves the statistics at their initial values
        if R.is_statistic(n):
            assert torch.equal(tr.store.vars["tower/" + n], (torch.ones if n.endswith("variance") else torch.zeros)(want[n]))
    tr.step(x, nf, y)
    assert list(tr.store.vars) == ["tower/" + n for n in want]         # a second forward meets the same names


@pytest.mark.parametrize("name", list(R.MODULES))
@pytest.mark.parametrize("scope_id", [None, 3])
def test_module_variable_names_shapes_order_and_trainability(name, scope_id):
    store = vs.VariableStore(device="cpu")
    cls = getattr(attention_modules, name)
    x = torch.rand(B, V)
    with vs.use_store(store):
        for _ in range(2):
            out = cls(V, True, scope_id=scope_id).forward(x)
    assert out.shape == (B, V)
    suffix = "" if scope_id is None or name.endswith("GateModule") and name != "CorNNGateModule" else str(scope_id)
    want = {n.replace("_v1", "_v1" + suffix): s(V) for n, s in R.MODULES[name][1].items()}
    assert [(n, tuple(v.shape)) for n, v in store.vars.items()] == list(want.items())
    for n in want:
        assert store.trainable[n] == (not R.is_statistic(n)), n
    if name in ("CorNNGateModule", "ContextGateV1"):                  # batch_norm is a constructor argument of these two alone
        store2 = vs.VariableStore(device="cpu")
        with vs.use_store(store2):
            cls(V, True, batch_norm=False, scope_id=scope_id).forward(x)
        assert list(store2.vars) == [n for n in want if "_bn_" not in n]


def test_gate_variables_are_random_normal_with_stddev_one_over_sqrt_v():
    store = vs.VariableStore(device="cpu")
    with vs.use_store(store):
        attention_modules.PnGateModule(400, True).forward(torch.rand(2, 400))
    for n in ("p_pn_gate", "n_pn_gate"):
        w = store.vars[n]
        assert abs(float(w.detach().std()) * 20 - 1) < 0.02 and abs(float(w.detach().mean())) < 1e-3


def _close(what, got, ref):
    e = rel_err(got, ref)
    print(f"[class_rows host] {what}: {e:.3e}")
    assert e <= REL_TOL, f"{what}: {e:.3e} > {REL_TOL:.1e}"


@pytest.mark.parametrize("training_mode", [True, False], ids=["training", "eval"])
def test_cpu_route_matches_the_fp64_restatement(training_mode):
    """FishMoeModel3: predictions, the gradient of the cross-entropy loss in every variable, the new moving statistics"""
    from learnablepoolingmethods_amd import losses
    x, nf, y = _batch(1)
    xn = normalize_input(x)
    p32 = R.make_variables(R.fish_moe3_variables(F, V), 5)
    store = vs.VariableStore(device="cpu")
    model = registry.get_model("FishMoeModel3")
    with vs.use_store(store):
        with torch.no_grad(), vs.variable_scope("tower"):
            model.create_model(xn, vocab_size=V, is_training=False)
        store.pop_regularization_losses()
        store.load({"tower/" + k: v for k, v in p32.items()}, strict=True)
        with vs.variable_scope("tower"):
            pred = model.create_model(xn, vocab_size=V, is_training=training_mode)["predictions"]
        store.pop_regularization_losses()
        names = [n for n in store.vars if store.trainable[n]]
        grads = dict(zip(names, torch.autograd.grad(losses.CrossEntropyLoss().calculate_loss(pred, y), [store.vars[n] for n in names])))
    p64 = {k: v.double().requires_grad_(not R.is_statistic(k)) for k, v in p32.items()}
    pred64, stats64, _ = R.fish_moe3(xn.double(), p64, training_mode)
    names64 = [k for k, v in p64.items() if v.requires_grad]
    g64 = dict(zip(names64, torch.autograd.grad(R.cross_entropy(pred64, y), [p64[k] for k in names64])))
    _close("predictions", pred, pred64)
    assert float((pred.sum(1) - 1).abs().max()) < 1e-5
    assert set(grads) == {"tower/" + n for n in g64}
    for n, g in g64.items():
        e = R.gradient_error(n, grads["tower/" + n], g, g64, training_mode)
        print(f"[class_rows host] d{n}: {e:.3e}")
        assert e <= REL_TOL, n
    assert set(stats64) == ({n for n in p32 if R.is_statistic(n)} if training_mode else set())
    for n, s in stats64.items():
        _close(n, store.vars["tower/" + n], s)


@pytest.mark.parametrize("training_mode", [True, False], ids=["training", "eval"])
@pytest.mark.parametrize("name", list(R.MODULES))
def test_modules_on_the_cpu_match_the_fp64_restatement(name, training_mode):
    g = torch.Generator().manual_seed(2)
    x = torch.rand(B, V, generator=g)
    p32 = R.make_variables({n: s(V) for n, s in R.MODULES[name][1].items()}, 6)
    store = vs.VariableStore(device="cpu")
    cls = getattr(attention_modules, name)
    with vs.use_store(store):
        with torch.no_grad():
            cls(V, False).forward(x)
        store.load(p32, strict=True)
        out = cls(V, training_mode).forward(x)
    out64, stats64, _ = R.MODULES[name][0](x.double(), {k: v.double() for k, v in p32.items()}, training_mode)
    _close(f"{name} output", out, out64)
    for n, s in stats64.items():
        _close(f"{name} {n}", store.vars[n], s)
    if name.endswith("GateModule") and name != "CorNNGateModule":
        assert float((out.sum(1) - 1).abs().max()) < 1e-5


def test_dropout_is_a_no_op_in_training():
    """tf.layers.dropout(r_activation0, 0.9) without training= (video_level_models.py:430): a dropout_masks argument changes nothing,
    and two training forwards from the same variables give the same bits (nothing is drawn)"""
    x, nf, y = _batch(2)
    outs = []
    for masks in (None, {"dense": torch.zeros(B, 2 * V, dtype=torch.uint8), "filter1": torch.zeros(B, 2 * V, dtype=torch.uint8)}, None):
        tr = Trainer(registry.get_model("FishMoeModel3"), vocab_size=V, batch_size=B, device="cpu", seed=1)
        out = tr.step(x, nf, y, dropout_masks=masks) if masks is not None else tr.step(x, nf, y)
        outs.append((out["predictions"], out["loss"], _variables(tr)))
    for o in outs[1:]:
        assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1])
        assert all(torch.equal(v, outs[0][2][n]) for n, v in o[2].items())


def test_moving_statistics_move_by_one_hundredth_towards_the_batch():
    x, nf, y = _batch(1)
    tr = Trainer(registry.get_model("FishMoeModel3"), vocab_size=V, batch_size=B, device="cpu", seed=2)
    tr.build(x, nf, y)
    stat_names = [n for n in R.fish_moe3_variables(F, V) if R.is_statistic(n)]
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():                                    # old values of the size of the batch's own, so that both terms count
        for n in stat_names:
            v = tr.store.vars["tower/" + n]
            v.copy_(0.5 + torch.rand(v.shape, generator=g) if n.endswith("variance") else 0.1 * torch.randn(v.shape, generator=g))
    before = _variables(tr)
    out = tr.step(x, nf, y)
    pred, stats, _ = R.fish_moe3(normalize_input(x), before, True)
    assert torch.allclose(out["predictions"], pred, rtol=1e-4, atol=1e-6)
    after = _variables(tr)
    assert len(stat_names) == 6
    for n in stat_names:
        assert torch.allclose(after[n], stats[n], rtol=1e-5, atol=1e-8), n
        assert not torch.equal(after[n], before[n]), n
    # spelled out for the first batch norm: 0.99 old + 0.01 (batch mean | BIASED batch variance) of the mixture's probabilities
    xn = normalize_input(x)
    gates = torch.softmax((xn @ before["gates/weights"]).reshape(-1, 3), dim=-1)
    experts = torch.sigmoid((xn @ before["experts/weights"] + before["experts/biases"]).reshape(-1, 2))
    p0 = (gates[:, :2] * experts).sum(1).reshape(-1, V)
    old_m, old_v = before["batch_normalization/moving_mean"], before["batch_normalization/moving_variance"]
    assert torch.allclose(after["batch_normalization/moving_mean"], 0.99 * old_m + 0.01 * p0.mean(0), rtol=1e-5, atol=1e-8)
    assert torch.allclose(after["batch_normalization/moving_variance"], 0.99 * old_v + 0.01 * p0.var(0, unbiased=False), rtol=1e-5, atol=1e-8)


def test_step_predict_and_predictor():
    x, nf, y = _batch()
    tr = Trainer(registry.get_model("FishMoeModel3"), vocab_size=V, batch_size=B, device="cpu", seed=1)
    out = tr.step(x, nf, y)
    assert tr.global_step == 1
    assert out["predictions"].shape == (B, V) and torch.isfinite(out["predictions"]).all() and torch.isfinite(out["loss"])
    p = tr.predict(x, nf)
    assert p.shape == (B, V) and torch.isfinite(p).all() and float((p.sum(1) - 1).abs().max()) < 1e-5
    pr = Predictor.from_trainer(tr)
    assert torch.equal(pr.predict(x, nf), p)


def test_num_mixtures_and_filter_size():
    """num_mixtures: the argument, or FLAGS.moe_num_mixtures; the penalty is FLAGS.moe_l2 whatever the argument says"""
    x = normalize_input(_batch()[0])
    store = vs.VariableStore(device="cpu")
    with vs.use_store(store), vs.variable_scope("tower"):
        registry.get_model("FishMoeModel3").create_model(x, vocab_size=V, is_training=True, num_mixtures=4, filter_size=3, l2_penalty=123.0)
    assert store.vars["tower/gates/weights"].shape == (F, 5 * V) and store.vars["tower/experts/weights"].shape == (F, 4 * V)
    assert store.vars["tower/dense/kernel"].shape == (V, 3 * V) and store.vars["tower/dense_1/kernel"].shape == (3 * V, V)
    reg = store.pop_regularization_losses()
    w = [store.vars["tower/gates/weights"], store.vars["tower/experts/weights"]]
    want = sum(FLAGS.moe_l2 * 0.5 * float((t.double() ** 2).sum()) for t in w)
    assert abs(float(sum(reg)) - want) <= 1e-6 * want


def test_the_fused_flags_change_nothing_on_the_cpu():
    assert isinstance(FLAGS.class_rows_fused, bool)
    x, nf, y = _batch()
    saved = FLAGS.class_rows_fused
    outs = []
    try:
        for fused in (False, True):
            FLAGS.class_rows_fused = fused
            tr = Trainer(registry.get_model("FishMoeModel3"), vocab_size=V, batch_size=B, device="cpu", seed=1)
            outs.append(tr.step(x, nf, y)["predictions"])
    finally:
        FLAGS.class_rows_fused = saved
    assert torch.equal(outs[0], outs[1])


def test_class_rows_op_refuses_cpu_tensors():
    a = torch.zeros(4, 6)
    assert not ops.class_rows_ok(a)
    with pytest.raises(LpmError, match="class_rows: a is a CPU tensor"):
        ops.class_rows(a, norm="softmax")
    with pytest.raises(LpmError, match="CPU tensor"):
        ops.class_rows(a, bias=torch.zeros(6), residual=a, norm="layer_norm", ln=(torch.ones(6), torch.zeros(6)))
    with pytest.raises(LpmError, match="unknown phi"):
        ops.class_rows(a, phi="relu")
    with pytest.raises(LpmError, match="unknown norm"):
        ops.class_rows(a, norm="batch_norm")


def test_torch_formulation_against_the_restatement():
    """layers.class_rows_torch, every form, in fp64: outputs and gradients"""
    for form, cfg in R.FORMS.items():
        inp32, dy32 = R.make_rows_inputs(5, 37, form, seed=0)
        inp, dy = R.widen(inp32), dy32.double()
        out, g = R.rows_gradients(inp, cfg["phi"], cfg["norm"], dy)
        leaves = {k: v.clone().requires_grad_(True) for k, v in inp.items()}
        ln = (leaves["gamma"], leaves["beta"]) if "gamma" in leaves else None
        y = layers.class_rows_torch(leaves["a"], leaves.get("bias"), leaves.get("residual"), cfg["phi"], cfg["norm"], ln)
        assert torch.allclose(y, out["y"], rtol=1e-10, atol=1e-12), form
        for n, got in zip(g, torch.autograd.grad((y * dy).sum(), [leaves[n] for n in g])):
            assert torch.allclose(got, g[n], rtol=1e-8, atol=1e-10), (form, n)


def test_restatement_matches_autograd_free_formulas():
    """The restatement's own backward against the closed forms of csrc/class_rows.hip, in fp64 (the GPU tests lean on it)"""
    inp32, dy32 = R.make_rows_inputs(7, 13, "ln", seed=0)
    inp, dy = R.widen(inp32), dy32.double()
    out, g = R.rows_gradients(inp, "identity", "layer_norm", dy)
    mean, rstd = out["stats"][:, :1], out["stats"][:, 1:]
    xhat = (out["pre"] - mean) * rstd
    gg = dy * inp["gamma"]
    dpre = rstd * (gg - gg.mean(1, keepdim=True) - xhat * (gg * xhat).mean(1, keepdim=True))
    assert torch.allclose(g["a"], dpre) and torch.allclose(g["residual"], dpre) and torch.allclose(g["bias"], dpre.sum(0))
    assert torch.allclose(g["gamma"], (dy * xhat).sum(0)) and torch.allclose(g["beta"], dy.sum(0))
    inp32, dy32 = R.make_rows_inputs(7, 13, "n_gate_softmax", seed=1)
    inp, dy = R.widen(inp32), dy32.double()
    out, g = R.rows_gradients(inp, "neg_relu6", "softmax", dy)
    assert R.kink_distance(inp["a"]) >= 0.009
    dpre = out["y"] * (dy - (out["y"] * dy).sum(1, keepdim=True))
    assert torch.allclose(g["residual"], dpre)
    assert torch.allclose(g["a"], dpre * ((inp["a"] > -6) & (inp["a"] < 0)).double())


def test_training_main_from_video_level_files(tmp_path):
    rng = np.random.default_rng(5)
    paths = []
    for k in range(2):
        recs = [readers.make_example(f"f{k}v{i}", rng.integers(0, V, size=2).tolist(),
                                     {"mean_rgb": rng.standard_normal(24).astype(np.float32),
                                      "mean_audio": rng.standard_normal(12).astype(np.float32)}) for i in range(9)]
        paths.append(str(tmp_path / f"train{k}.tfrecord"))
        readers.write_tfrecord(paths[-1], recs)
    train_dir = str(tmp_path / "model")
    argv = ["--train_data_pattern", str(tmp_path / "train*.tfrecord"), "--train_dir", train_dir, "--model", "FishMoeModel3",
            "--frame_features", "false", "--feature_sizes", "24,12", "--num_classes", str(V), "--device", "cpu", "--batch_size", "4",
            "--log_every", "1", "--num_epochs", "10"]
    saved = {n: getattr(FLAGS, n) for n in ("batch_size",)}
    try:
        out = training.main(argv + ["--max_steps", "3"])
        assert out["global_step"] == 3 and out["steps"] == 3 and np.isfinite(out["last_loss"])
        assert training.latest_checkpoint(train_dir) == training.checkpoint_path(train_dir, 3)
        state = torch.load(training.checkpoint_path(train_dir, 3), map_location="cpu")
        assert "tower/batch_normalization_2/moving_variance" in state and "tower/LayerNorm/gamma" in state and "tower/dense_2/kernel" in state
        again = training.main(argv + ["--max_steps", "5"])
        assert again["global_step"] == 5 and again["steps"] == 2
        assert training.latest_checkpoint(train_dir) == training.checkpoint_path(train_dir, 5)
    finally:
        for n, v in saved.items():
            setattr(FLAGS, n, v)
