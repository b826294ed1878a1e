"""-m "not gpu": ``--optimizer`` (train.py:106,252,577) on the CPU device -- optimizers.by_name against the table of tf.train's classes
built from the learning rate alone, a CPU Trainer under every rule against the table restated in fp64, checkpoints (TF's slot keys, a
bit-exact resume, the refusal of another rule's file, files from before the key existed, serving) and the training command line."""
import json
import os

import numpy as np
import pytest
import torch

from learnablepoolingmethods_amd import FLAGS, optimizers, readers, registry, training
from learnablepoolingmethods_amd._capi import LpmError
from learnablepoolingmethods_amd.predictor import Predictor
from learnablepoolingmethods_amd.train import Trainer

from tests._optimizer_ref import MU, RULES, TABLE, check_trainer_steps
from tests._util import rel_err

B, F, V = 8, 16 + 8, 40          # the shapes of test_moe_step_against_an_fp64_restatement


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, F, generator=g) * 3.0
    y = torch.rand(B, V, generator=g) < 0.15
    return x, torch.ones(B, dtype=torch.int32), y


def _trainer(name, seed=3):
    return Trainer(registry.get_model("MoeModel"), vocab_size=V, batch_size=B, base_learning_rate=1e-2, device="cpu", seed=seed,
                   model_kwargs=dict(num_mixtures=2), optimizer=name, optimizer_momentum=MU)


def test_by_name_returns_the_table():
    assert FLAGS.optimizer == "AdamOptimizer" and FLAGS.optimizer_momentum is None
    for name in RULES:
        spec = optimizers.by_name(name, momentum=MU)
        init, keys = TABLE[name]
        assert spec.name == name and spec.slots == len(init) and spec.slot_init == init and spec.slot_keys == keys
    kinds = [optimizers.by_name(n, momentum=MU).kind for n in RULES]
    assert kinds == [1, 2, 3, 4, 5]                                   # LPM_UPDATE_* of include/lpm_hip.h
    assert (optimizers.by_name("MomentumOptimizer", momentum=MU).h0, optimizers.by_name("MomentumOptimizer", momentum=0.5).h0) == (MU, 0.5)
    rms, ada = optimizers.by_name("RMSPropOptimizer"), optimizers.by_name("AdadeltaOptimizer")
    assert (rms.h0, rms.h1, ada.h0, ada.h1) == (0.9, 1e-10, 0.95, 1e-8)
    adam = optimizers.by_name("AdamOptimizer")
    assert adam.kind == 0 and adam.slot_keys == ("Adam", "Adam_1") and adam.slot_init == (0.0, 0.0)


@pytest.mark.parametrize("name", ["FtrlOptimizer", "ProximalGradientDescentOptimizer", "ProximalAdagradOptimizer", "AdagradDAOptimizer",
                                  "SomeOtherOptimizer", "adamoptimizer", ""])
def test_by_name_refuses_by_name_with_the_supported_list(name):
    with pytest.raises(LpmError) as e:
        optimizers.by_name(name)
    assert repr(name) in str(e.value)
    for ok in ("AdamOptimizer",) + RULES:
        assert ok in str(e.value)


def test_momentum_needs_its_flag():
    assert FLAGS.optimizer_momentum is None
    with pytest.raises(LpmError, match="optimizer_momentum"):
        optimizers.by_name("MomentumOptimizer")
    with pytest.raises(LpmError, match="optimizer_momentum"):
        Trainer(registry.get_model("MoeModel"), vocab_size=V, device="cpu", optimizer="MomentumOptimizer")
    try:
        FLAGS.optimizer_momentum = 0.8
        assert optimizers.by_name("MomentumOptimizer").h0 == 0.8
    finally:
        FLAGS.reset()


@pytest.mark.parametrize("name", RULES)
def test_cpu_trainer_steps_follow_the_table_in_fp64(name):
    tr = _trainer(name)
    check_trainer_steps(tr, name, [_batch(47), _batch(48)], rel_err)
    assert tr.global_step == 2 and tr.factored is None and tr.sharded is None
    assert tr.arena.m is None and tr.arena.v is None and len(tr.arena.slots) == len(TABLE[name][0])


def _state(tr):
    """Every variable and every slot of every variable (what a checkpoint holds: the arenas' alignment padding is nobody's state)."""
    return sorted((k, v) for k, v in tr.state_dict().items() if torch.is_tensor(v))


@pytest.mark.parametrize("name", RULES)
def test_checkpoint_keys_resume_and_refusal(name, tmp_path):
    batches = [_batch(50 + i) for i in range(4)]
    whole = _trainer(name)
    for b in batches[:2]:
        whole.step(*b)
    path = str(tmp_path / "two.pt")
    whole.save(path)
    state = torch.load(path, map_location="cpu")
    variables = ["tower/experts/biases", "tower/experts/weights", "tower/gates/weights"]
    want = set(variables) | {f"{v}/{k}" for v in variables for k in TABLE[name][1]} | {"global_step", "optimizer"}
    assert set(state) == want and state["optimizer"] == name and state["global_step"] == 2
    for b in batches[2:]:
        whole.step(*b)
    resumed = _trainer(name, seed=9)                          # (other initial values: everything must come from the file)
    resumed.build(*batches[2])
    resumed.restore(path)
    assert resumed.global_step == 2
    for b in batches[2:]:
        resumed.step(*b)
    got, want = _state(resumed), _state(whole)
    assert [k for k, _ in got] == [k for k, _ in want] and len(got) == 3 * (1 + len(TABLE[name][1]))
    for (k, a), (_, b) in zip(got, want):
        assert torch.equal(a, b), f"{name}: {k} of the resumed run differs from the uninterrupted one"
    other = _trainer("AdagradOptimizer" if name != "AdagradOptimizer" else "RMSPropOptimizer")
    other.build(*batches[0])
    for tr in (other, _adam_trainer(batches[0])):
        with pytest.raises(RuntimeError) as e:
            tr.restore(path)
        assert name in str(e.value) and tr.optimizer.name in str(e.value)


def _adam_trainer(batch, **kw):
    tr = Trainer(registry.get_model("MoeModel"), vocab_size=V, batch_size=B, base_learning_rate=1e-2, device="cpu", seed=3,
                 model_kwargs=dict(num_mixtures=2), **kw)
    tr.build(*batch)
    return tr


def test_a_state_without_the_key_is_adams():
    batch = _batch(60)
    tr = _adam_trainer(batch)
    assert tr.optimizer.name == "AdamOptimizer" and tr.arena.slots[0] is tr.arena.m and tr.arena.slots[1] is tr.arena.v
    tr.step(*batch)
    state = tr.state_dict()
    assert state.pop("optimizer") == "AdamOptimizer"           # what a checkpoint from before --optimizer holds
    fresh = _adam_trainer(batch, optimizer="AdamOptimizer")
    fresh.load_state_dict(state)
    assert fresh.global_step == 1 and bool(fresh.arena.m.abs().sum() > 0)
    for a, b in zip((tr.arena.param, tr.arena.m, tr.arena.v), (fresh.arena.param, fresh.arena.m, fresh.arena.v)):
        assert torch.equal(a, b)
    sgd = _trainer("GradientDescentOptimizer")
    sgd.build(*batch)
    with pytest.raises(RuntimeError, match="AdamOptimizer.*GradientDescentOptimizer"):
        sgd.load_state_dict(state)


def test_predictor_loads_an_adagrad_checkpoint(tmp_path):
    batch = _batch(61)
    tr = _trainer("AdagradOptimizer")
    tr.step(*batch)
    path = str(tmp_path / "adagrad.pt")
    tr.save(path)
    pr = Predictor.from_checkpoint(path, registry.get_model("MoeModel"), vocab_size=V, model_kwargs=dict(num_mixtures=2), device="cpu")
    assert sorted(pr.store.vars) == ["tower/experts/biases", "tower/experts/weights", "tower/gates/weights"]
    assert torch.equal(pr.predict(batch[0], batch[1]), tr.predict(batch[0], batch[1]))


def test_training_main_with_optimizer_trains_records_the_flag_and_resumes(tmp_path):
    rng = np.random.default_rng(5)
    for k in range(2):
        recs = [readers.make_example(f"f{k}v{i}", rng.integers(0, 11, size=2).tolist(),
                                     {"mean_rgb": rng.standard_normal(24).astype(np.float32),
                                      "mean_audio": rng.standard_normal(12).astype(np.float32)}) for i in range(9)]
        readers.write_tfrecord(str(tmp_path / f"train{k}.tfrecord"), recs)
    train_dir = str(tmp_path / "model")
    argv = ["--train_data_pattern", str(tmp_path / "train*.tfrecord"), "--train_dir", train_dir, "--model", "MoeModel",
            "--frame_features", "false", "--feature_sizes", "24,12", "--num_classes", "11", "--device", "cpu", "--batch_size", "4",
            "--moe_num_mixtures", "2", "--log_every", "1", "--num_epochs", "10", "--optimizer", "AdagradOptimizer"]
    try:
        out = training.main(argv + ["--max_steps", "3"])
        assert out["global_step"] == 3 and out["steps"] == 3 and np.isfinite(out["last_loss"])
        with open(os.path.join(train_dir, "model_flags.json")) as f:
            assert json.load(f)["flags"]["optimizer"] == "AdagradOptimizer"
        state = torch.load(training.checkpoint_path(train_dir, 3), map_location="cpu")
        assert state["optimizer"] == "AdagradOptimizer" and "tower/gates/weights/Adagrad" in state and "tower/gates/weights/Adam" not in state
        again = training.main(argv + ["--max_steps", "5"])
        assert again["global_step"] == 5 and again["steps"] == 2
        FLAGS.reset()
        with pytest.raises(RuntimeError, match="AdagradOptimizer.*AdamOptimizer"):          # the default rule refuses the directory's file
            training.main(argv[:-2] + ["--max_steps", "6"])
        FLAGS.reset()
        momentum = training.main(argv[:-2] + ["--optimizer", "MomentumOptimizer", "--optimizer_momentum", "0.9", "--max_steps", "2",
                                              "--train_dir", str(tmp_path / "momentum")])
        assert momentum["global_step"] == 2
        with open(os.path.join(str(tmp_path / "momentum"), "model_flags.json")) as f:
            assert json.load(f)["flags"] == {"batch_size": 4, "optimizer": "MomentumOptimizer", "optimizer_momentum": 0.9}
    finally:
        FLAGS.reset()
