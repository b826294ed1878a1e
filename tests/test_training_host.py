"""-m "not gpu": the host side of training from TFRecords -- the quantised training entry points are declared, exported and bound;
uint8 frames stay refused in training without the keyword; readers.ShufflePool's policy over CPU batches; the file order of
training_batches; training.run's log lines, checkpoints, resume and its equivalence to a hand-written loop (with a stand-in trainer:
see "the run loop" below); the command line's flags and its empty file set."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lpm_hip.h")
# name -> position of `raw` in the fp32 form's parameter list
NEW_SYMBOLS = {"lpm_frame_stats_q8": 0, "lpm_frame_bn_bwd_q8": 2, "lpm_frame_bn_bwd_split_q8": 5}


def test_quantised_training_entry_points_are_declared_exported_and_bound():
    from learnablepoolingmethods_amd import _build, _capi
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    if not os.path.exists(_capi.LIB_PATH):
        _build.build(verbose=False)
    dll = ctypes.CDLL(_capi.LIB_PATH)
    for name, at in NEW_SYMBOLS.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), f"{name} not declared in lpm_hip.h"
        assert hasattr(dll, name), f"{name} not exported"
        assert name in _capi.SIGNATURES, f"{name} missing from the ctypes table"
        # the fp32 form's parameters with (q, inv_norm, max, min) in place of raw
        fp32 = _capi.SIGNATURES[name[:-3]][1]
        assert _capi.SIGNATURES[name][1] == fp32[:at + 1] + [ctypes.c_void_p, ctypes.c_float, ctypes.c_float] + fp32[at + 1:], name
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", txt).group(1)
        params = [p.strip() for p in decl.split(",")]
        assert [p.split()[-1].lstrip("*") for p in params[at:at + 4]] == ["q", "inv_norm", "max_quantized_value", "min_quantized_value"]
        assert len(params) == len(fp32) + 3


def test_uint8_frames_stay_refused_in_training_without_the_keyword():
    from learnablepoolingmethods_amd import ops, registry
    from learnablepoolingmethods_amd import variables as vs
    from learnablepoolingmethods_amd._capi import LpmError
    q, nf = torch.zeros(2, 10, 1152, dtype=torch.uint8), torch.tensor([10, 4])
    with pytest.raises(LpmError, match="eval mode only"):
        ops.frame_sample_bn(q, nf, 5, is_training=True)
    with pytest.raises(LpmError, match="eval mode only"):
        ops.frame_sample_bn(q, nf, 5, is_training=True, quantised_training=False)
    with pytest.raises(LpmError, match="eval mode only"):
        ops.frame_sample_bn(q, nf, 5, is_training=True, quantised_training=True)           # CPU frames: the q8 path is the GPU's
    with pytest.raises(LpmError, match="eval mode only"):
        ops.frame_sample_bn_split(q, nf, 5, None, None, None, None, True, 1024, quantised_training=False)
    assert not ops.frame_sample_bn_split_ok(q, 1024, is_training=True)
    assert not ops.frame_sample_bn_split_ok(q, 1024, is_training=True, quantised_training=True)   # (not on the GPU)
    for model in ("NetVladV1", "NetVladV2"):
        store = vs.VariableStore(device="cpu")
        with vs.use_store(store), pytest.raises(LpmError, match="eval mode only"):
            registry.get_model(model).create_model(q, vocab_size=10, num_frames=nf, iterations=5, cluster_size=8, hidden_size=8,
                                                   is_training=True)


def test_the_flag_exists_and_defaults_to_on():
    from learnablepoolingmethods_amd import FLAGS
    assert FLAGS.train_quantised_frames is True


# ---- the shuffle pool ------------------------------------------------------------------------------------------------------------
V, MF, SIZES, NAMES = 12, 6, (8, 4), ("rgb", "audio")


def _reader():
    from learnablepoolingmethods_amd import readers
    return readers.YT8MFrameFeatureReader(num_classes=V, feature_sizes=SIZES, feature_names=NAMES, max_frames=MF)


def _write_files(tmp_path, n_files, per_file, seed=0):
    """n_files files of per_file DISTINCT clips (ids clip0, clip1, ... in file order)."""
    from learnablepoolingmethods_amd import readers
    rng = np.random.default_rng(seed)
    files, k = [], 0
    for f in range(n_files):
        recs = []
        for _ in range(per_file):
            n = int(rng.integers(0, MF + 3))
            feats = {nm: rng.integers(0, 256, size=(n, s), dtype=np.uint8) for nm, s in zip(NAMES, SIZES)}
            feats["rgb"][:, 0] = k % 256                                   # distinct content as well as a distinct id
            if n:
                feats["rgb"][0, 1] = k // 256
            recs.append(readers.make_sequence_example(f"clip{k}", sorted(set(rng.integers(0, V, size=3).tolist())), feats))
            k += 1
        path = str(tmp_path / f"part{f}.tfrecord")
        readers.write_tfrecord(path, recs)
        files.append(path)
    return files


def _by_id(reader, files, batch_size):
    out, order = {}, []
    for ids, q, y, nf in reader.batches(files, batch_size):
        for i, vid in enumerate(ids):
            out[vid] = (q[i].clone(), y[i].clone(), int(nf[i]))
            order.append(vid)
    return out, order


def _check_clips(batches, want):
    for ids, q, y, nf in batches:
        assert q.dtype == torch.uint8 and y.dtype == torch.bool and nf.dtype == torch.int32
        assert len(ids) == q.shape[0] == y.shape[0] == nf.shape[0]
        for i, vid in enumerate(ids):
            wq, wy, wn = want[vid]
            assert torch.equal(q[i], wq) and torch.equal(y[i], wy) and int(nf[i]) == wn, vid


def test_shuffle_pool_policy(tmp_path):
    from learnablepoolingmethods_amd import readers
    reader = _reader()
    files = _write_files(tmp_path, 4, 20)                                   # 80 clips: 10 input batches of 8
    B, CAP = 8, 40
    want, arrival = _by_id(reader, files, B)
    assert len(arrival) == 80 and len(set(arrival)) == 80
    pos = {vid: i for i, vid in enumerate(arrival)}

    def shuffled(seed):
        return list(readers.ShufflePool(reader.batches(files, B), B, capacity=CAP, min_after_dequeue=B, seed=seed))
    a = shuffled(1)
    _check_clips(a, want)
    order = [vid for ids, *_ in a for vid in ids]
    assert sorted(order) == sorted(arrival), "every clip exactly once"
    assert [len(b[0]) for b in a] == [B] * 10
    # the structural bound of the policy: when batch k is drawn at most k B + capacity clips have arrived
    for p, vid in enumerate(order):
        assert pos[vid] < (p // B) * B + CAP, (p, vid)
    assert [vid for ids, *_ in shuffled(1) for vid in ids] == order, "the same seed gives the same order"
    other = [vid for ids, *_ in shuffled(2) for vid in ids]
    assert other != order and other != arrival and order != arrival
    # a last batch that is smaller; defaults capacity = 5 B, min_after_dequeue = B; yielded tensors are fresh
    c = list(readers.ShufflePool(reader.batches(files, 7), 6, seed=3))
    _check_clips(c, want)
    assert [len(b[0]) for b in c] == [6] * 13 + [2]
    assert sorted(vid for ids, *_ in c for vid in ids) == sorted(arrival)
    assert len({b[1].data_ptr() for b in c}) == len(c)
    with pytest.raises(ValueError):
        readers.ShufflePool(iter(()), 8, capacity=10, min_after_dequeue=8)
    with pytest.raises(ValueError):                                        # 15 clips held, no room for 5 more, and 8 + 8 are needed
        list(readers.ShufflePool(reader.batches(files, 5), 8, capacity=16, min_after_dequeue=8))
    assert list(readers.ShufflePool(iter(()), 8)) == []


def test_training_batches_epochs_and_file_order(tmp_path, monkeypatch):
    reader = _reader()
    files = _write_files(tmp_path, 5, 6, seed=1)                            # 30 clips per epoch
    want, arrival = _by_id(reader, files, 4)
    seen_files = []
    real = reader.batches

    def spy(fs, *a, **k):
        seen_files.append(list(fs))
        return real(fs, *a, **k)
    monkeypatch.setattr(reader, "batches", spy)
    got = list(reader.training_batches(files, 4, device="cpu", num_epochs=2, seed=1, shuffle_files=True))
    _check_clips(got, want)
    order = [vid for ids, *_ in got for vid in ids]
    assert sorted(order) == sorted(arrival * 2), "every clip once per epoch"
    assert [len(b[0]) for b in got] == [4] * 15
    assert len(seen_files) == 2 and all(sorted(f) == sorted(files) for f in seen_files), "every file once per epoch"
    # (a seed for which it holds: two permutations of five files coincide once in 120 seeds, seed 0 among them)
    assert seen_files[0] != seen_files[1], "seed 1: the two epochs walk the files in different orders"
    seen_files.clear()
    again = [vid for ids, *_ in reader.training_batches(files, 4, device="cpu", num_epochs=2, seed=1) for vid in ids]
    assert again == order
    seen_files.clear()
    plain = list(reader.training_batches(files, 4, device="cpu", num_epochs=1, seed=0, shuffle_files=False, capacity=12, min_after_dequeue=4))
    assert seen_files == [files]
    assert sorted(vid for ids, *_ in plain for vid in ids) == sorted(arrival)
    # num_epochs=None runs until the consumer stops; closing it closes the source
    it = reader.training_batches(files, 4, device="cpu", seed=5)
    for _ in range(40):                                                     # more than five epochs' worth of batches
        ids, *_ = next(it)
        assert len(ids) == 4
    it.close()


# ---- the run loop ----------------------------------------------------------------------------------------------------------------
# Trainer.step has no CPU path (its clip + Adam update and every frame-level model's pooling are HIP kernels, and the project keeps no
# eager fall-back), so this tier drives training.run with ToyTrainer: the interface run() uses -- num_towers, device, global_step, arena,
# build, step, save, restore -- around a logistic layer on the mean frame in plain PyTorch.  tests/test_gpu_training.py runs the SAME
# checks (run_loop_checks) with the real Trainer and a tiny NetVladV1 on the GPU, and the command line's training run as well.
LOG_LINE = re.compile(r"^training step (\d+) \| Loss: (-?\d+\.\d\d) Examples/sec: (\d+\.\d\d) \| Hit@1: (\d\.\d\d) PERR: (\d\.\d\d) GAP: (\d\.\d\d)$")
FULL = dict(num_classes=V, feature_sizes=(1024, 128), feature_names=("rgb", "audio"), max_frames=MF)


class ToyTrainer:
    num_towers = 1

    def __init__(self, seed=3, lr=0.5):
        self.device, self.seed, self.lr = torch.device("cpu"), seed, lr
        self.global_step, self.arena = 0, None

    def build(self, frames, num_frames, labels):
        if self.arena is None:
            g = torch.Generator().manual_seed(self.seed)
            self.w = 0.05 * torch.randn(frames.shape[2], labels.shape[1], generator=g)
            self.b = torch.zeros(labels.shape[1])
            self.arena = object()

    def step(self, frames, num_frames, labels):
        from learnablepoolingmethods_amd import losses
        from learnablepoolingmethods_amd.train import normalize_input
        self.build(frames, num_frames, labels)
        w, b = self.w.clone().requires_grad_(), self.b.clone().requires_grad_()
        pooled = normalize_input(frames, num_frames).sum(1) / num_frames.clamp_min(1).view(-1, 1).float()
        p = torch.sigmoid(pooled.matmul(w) + b)
        loss = losses.CrossEntropyLoss().calculate_loss(p, labels.float())
        gw, gb = torch.autograd.grad(loss, [w, b])
        self.w, self.b = self.w - self.lr * gw, self.b - self.lr * gb
        self.global_step += 1
        return {"loss": loss.detach(), "predictions": p.detach(), "global_step": self.global_step}

    def state_dict(self):
        return {"w": self.w, "b": self.b, "global_step": self.global_step}

    def save(self, path):
        torch.save(self.state_dict(), path)

    def restore(self, path):
        state = torch.load(path, map_location="cpu")
        self.w, self.b, self.global_step = state["w"], state["b"], int(state["global_step"])


def _full_files(tmp_path, n_files=2, per_file=10):
    from learnablepoolingmethods_amd import readers
    rng = np.random.default_rng(7)
    files, k = [], 0
    for f in range(n_files):
        recs = []
        for _ in range(per_file):
            n = int(rng.integers(1, MF + 2))
            feats = {"rgb": rng.integers(0, 256, size=(n, 1024), dtype=np.uint8), "audio": rng.integers(0, 256, size=(n, 128), dtype=np.uint8)}
            recs.append(readers.make_sequence_example(f"clip{k}", sorted(set(rng.integers(0, V, size=2).tolist())), feats))
            k += 1
        path = str(tmp_path / f"train{f}.tfrecord")
        readers.write_tfrecord(path, recs)
        files.append(path)
    return files


def _same_state(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        if torch.is_tensor(a[k]) or torch.is_tensor(b[k]):
            assert torch.equal(torch.as_tensor(a[k]).cpu(), torch.as_tensor(b[k]).cpu()), k
        else:
            assert a[k] == b[k], k


def run_loop_checks(make_trainer, tmp_path, device):
    """training.run against its specification, for any trainer factory ``make_trainer(seed)`` (batch size 4, V classes) on ``device``."""
    from learnablepoolingmethods_amd import eval_util, readers, training
    files = _full_files(tmp_path)
    reader = readers.YT8MFrameFeatureReader(**FULL)

    def batches():
        return reader.training_batches(files, 4, device=device, num_epochs=None, seed=11)
    train_dir = str(tmp_path / "model")
    lines, captured = [], {}

    def on_step(result, batch):
        captured[result["global_step"]] = (result["predictions"].clone(), batch[2].clone(), float(result["loss"]))
    tr = make_trainer(3)
    it = batches()
    out = training.run(tr, it, max_steps=25, train_dir=train_dir, log=lines.append, on_step=on_step)
    it.close()
    assert out["global_step"] == 25 and out["steps"] == 25 and out["num_examples"] == 100 and tr.global_step == 25
    assert out["last_loss"] == captured[25][2] and out["seconds"] > 0 and out["examples_per_second"] > 0
    steps_logged = [l for l in lines if l.startswith("training step")]
    assert len(steps_logged) == 2
    for line, step in zip(steps_logged, (10, 20)):
        m = LOG_LINE.match(line)
        assert m, line
        p, y, loss = captured[step]
        p, y = p.cpu(), y.cpu()
        assert int(m.group(1)) == step and m.group(2) == "%.2f" % loss
        assert m.group(4) == "%.2f" % eval_util.calculate_hit_at_one(p, y)
        assert m.group(5) == "%.2f" % eval_util.calculate_precision_at_equal_recall_rate(p, y)
        assert m.group(6) == "%.2f" % eval_util.calculate_gap(p, y)
    # first logged step, (export_model_steps = 1000: none in between), exit
    assert sorted(os.listdir(train_dir)) == ["model.ckpt-10.pt", "model.ckpt-25.pt"]
    assert out["checkpoints"] == [os.path.join(train_dir, n) for n in ("model.ckpt-10.pt", "model.ckpt-25.pt")]

    # the same 25 steps by hand: bit-identical variables (and Adam slots)
    hand = make_trainer(3)
    it = batches()
    for _ in range(25):
        _, q, y, nf = next(it)
        hand.step(q, nf, y)
    it.close()
    _same_state(tr.state_dict(), hand.state_dict())

    # resume: a NEW trainer (another seed) continues at 25 from the newest checkpoint, with its variables
    seen = []
    tr2 = make_trainer(99)
    it = batches()
    out2 = training.run(tr2, it, max_steps=27, train_dir=train_dir, log=lines.append, export_model_steps=1,
                        on_step=lambda r, b: seen.append(r["global_step"]))
    it.close()
    assert seen == [26, 27] and out2["global_step"] == 27 and out2["steps"] == 2
    assert out2["checkpoints"] == [os.path.join(train_dir, "model.ckpt-27.pt")]
    it = batches()                                                           # the input stream restarts: step 26 sees the first batch
    for _ in range(2):
        _, q, y, nf = next(it)
        hand.step(q, nf, y)
    it.close()
    _same_state(tr2.state_dict(), hand.state_dict())
    # already at max_steps: nothing runs, nothing is written
    it = batches()
    out3 = training.run(make_trainer(3), it, max_steps=27, train_dir=train_dir, log=lines.append)
    it.close()
    assert out3["steps"] == 0 and out3["global_step"] == 27 and out3["checkpoints"] == [] and out3["last_loss"] is None

    # start_new_model: from step 0, the old checkpoints gone
    seen.clear()
    it = batches()
    out4 = training.run(make_trainer(3), it, max_steps=3, log_every=2, export_model_steps=1, train_dir=train_dir,
                        start_new_model=True, log=lines.append, on_step=lambda r, b: seen.append(r["global_step"]))
    it.close()
    assert seen == [1, 2, 3] and out4["global_step"] == 3
    assert sorted(os.listdir(train_dir)) == ["model.ckpt-2.pt", "model.ckpt-3.pt"]
    # export_model_steps between logged steps; the batches may simply end
    d2 = str(tmp_path / "model2")
    out5 = training.run(make_trainer(3), reader.training_batches(files, 4, device=device, num_epochs=2, seed=1), log_every=2,
                        export_model_steps=4, train_dir=d2, log=lines.append)
    assert out5["steps"] == 10 and out5["num_examples"] == 40
    assert sorted(os.listdir(d2), key=lambda n: int(n[11:-3])) == ["model.ckpt-2.pt", "model.ckpt-6.pt", "model.ckpt-10.pt"]


def test_run_logs_checkpoints_resumes_and_equals_a_hand_written_loop(tmp_path):
    run_loop_checks(lambda seed: ToyTrainer(seed=seed), tmp_path, "cpu")


def test_run_refuses_more_than_one_tower():
    from learnablepoolingmethods_amd import training

    class Two:
        num_towers = 2
    with pytest.raises(ValueError, match="num_towers"):
        training.run(Two(), iter(()))


CLI_TINY = ["--model", "NetVladV1", "--batch_size", "2", "--num_epochs", "1", "--max_steps", "2", "--base_learning_rate", "0.001",
            "--start_new_model", "--export_model_steps", "1", "--feature_names", "rgb,audio", "--feature_sizes", "1024,128",
            "--num_classes", str(V), "--max_frames", str(MF), "--iterations", "16", "--netvlad_cluster_size", "32",
            "--netvlad_hidden_size", "32", "--netvlad_encoder", "false"]


def test_command_line_flags_and_the_empty_file_set(tmp_path):
    """The flags parse onto FLAGS / run's arguments; a pattern that matches nothing raises train.py:168-170's IOError before any model is
    built.  (The two training steps of the command line need the GPU: tests/test_gpu_training.py.)"""
    from learnablepoolingmethods_amd import FLAGS, training
    args = training._parser().parse_args(["--train_data_pattern", "a*,b*", "--train_dir", "d"] + CLI_TINY)
    assert args.train_data_pattern == "a*,b*" and args.train_dir == "d" and args.model == "NetVladV1" and args.batch_size == 2
    assert args.num_epochs == 1 and args.max_steps == 2 and args.base_learning_rate == 0.001 and args.start_new_model is True
    assert args.export_model_steps == 1 and args.num_classes == V and args.netvlad_encoder is False and args.netvlad_cluster_size == 32
    assert training._parser().parse_args([]).start_new_model is False
    try:
        with pytest.raises(IOError, match="Unable to find training files"):
            training.main(["--train_data_pattern", str(tmp_path / "nothing*.tfrecord"), "--train_dir", str(tmp_path / "cli")] + CLI_TINY)
        with pytest.raises(IOError, match="Unable to find training files"):
            training.main(["--train_data_pattern", "", "--train_dir", str(tmp_path / "cli")])
    finally:
        FLAGS.reset()
