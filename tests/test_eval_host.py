"""-m "not gpu": the evaluation loop's host side -- lpm_eval_rows is declared, exported and bound; ops.eval_rows and
DeviceEvaluationMetrics refuse bad arguments before any GPU work; format_epoch_summary writes utils.AddEpochSummary's line; evaluate()
on a CPU model is the manual eval_util loop."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from learnablepoolingmethods_amd import _capi, eval_util, evaluation, ops
from learnablepoolingmethods_amd._capi import LpmError
from learnablepoolingmethods_amd.evaluation import DeviceEvaluationMetrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lpm_hip.h")


def test_eval_rows_is_declared_exported_and_bound():
    from learnablepoolingmethods_amd import _build
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    if not os.path.exists(_capi.LIB_PATH):
        _build.build(verbose=False)
    dll = ctypes.CDLL(_capi.LIB_PATH)
    assert re.search(r"\bint\s+lpm_eval_rows\s*\(", txt), "lpm_eval_rows not declared in lpm_hip.h"
    assert hasattr(dll, "lpm_eval_rows"), "lpm_eval_rows not exported"
    restype, args = _capi.SIGNATURES["lpm_eval_rows"]
    assert restype is ctypes.c_int and len(args) == 13
    decl = re.search(r"int\s+lpm_eval_rows\s*\(([^)]*)\)", txt).group(1)
    assert len(decl.split(",")) == len(args), "the ctypes row and the header disagree on the parameter count"


@pytest.fixture
def no_launch(monkeypatch):
    """Any attempt to load the library (the step before every launch) fails the test."""
    def refuse(*a, **k):
        raise AssertionError("the library was reached: the argument check came too late")
    monkeypatch.setattr(_capi, "load", refuse)


@pytest.mark.parametrize("case", ["dtype", "dim", "label_dtype", "label_shape", "k0", "k65", "k_above_v", "v_above_limit", "cpu"])
def test_eval_rows_refuses_bad_arguments_before_any_launch(no_launch, case):
    p, y, k = torch.rand(4, 100), torch.zeros(4, 100, dtype=torch.bool), 20
    if case == "dtype":
        p = p.double()
    elif case == "dim":
        p, y = p.reshape(-1), y.reshape(-1)
    elif case == "label_dtype":
        y = y.float()
    elif case == "label_shape":
        y = torch.zeros(4, 99, dtype=torch.bool)
    elif case == "k0":
        k = 0
    elif case == "k65":
        k = 65
    elif case == "k_above_v":
        p, y = torch.rand(4, 10), torch.zeros(4, 10, dtype=torch.bool)
    elif case == "v_above_limit":
        p, y = torch.empty(1, 65537, device="meta"), torch.empty(1, 65537, dtype=torch.uint8, device="meta")
    with pytest.raises(LpmError):
        ops.eval_rows(p, y, k)


def test_device_metrics_refuse_bad_arguments():
    with pytest.raises(LpmError, match="eval_util.EvaluationMetrics"):
        DeviceEvaluationMetrics(100, 20, "cpu")
    with pytest.raises(ValueError):
        DeviceEvaluationMetrics(1, 20, "cuda")
    with pytest.raises(ValueError):
        DeviceEvaluationMetrics(100, 0, "cuda")
    with pytest.raises(LpmError):
        DeviceEvaluationMetrics(100, 65, "cuda")
    with pytest.raises(LpmError):
        DeviceEvaluationMetrics(70000, 20, "cuda")


def _unbuilt_metrics(num_class=10, k=5):
    """A DeviceEvaluationMetrics that never touched a GPU (its constructor allocates device accumulators)."""
    m = DeviceEvaluationMetrics.__new__(DeviceEvaluationMetrics)
    m.num_class, m.top_k, m.k, m.device = num_class, k, k, torch.device("cuda", 0)
    m.num_examples, m._cap, m._rows = 0, 0, None
    return m


def test_device_metrics_refuse_cpu_tensors_and_an_empty_get(no_launch):
    m = _unbuilt_metrics()
    with pytest.raises(LpmError, match="eval_util.EvaluationMetrics"):
        m.accumulate(torch.rand(3, 10), torch.zeros(3, 10, dtype=torch.bool))
    with pytest.raises(ValueError):
        m.get()


def test_format_epoch_summary_is_the_reference_line():
    info = {"avg_hit_at_one": 0.8125, "avg_perr": 0.71875, "avg_loss": 12.3456789, "aps": [0.5, 0.25, 1.0], "gap": 0.6}
    assert evaluation.format_epoch_summary(info, 7) == ("epoch/eval number 7 | Avg_Hit@1: 0.812 | Avg_PERR: 0.719 | MAP: 0.583 | "
                                                        "GAP: 0.600 | Avg_Loss: 12.345679")
    assert evaluation.format_epoch_summary({**info, "avg_loss": 0.5}, "1000").endswith("| Avg_Loss: 0.500000")


def test_cross_entropy_rows_is_the_reference_loss():
    g = torch.Generator().manual_seed(3)
    p = torch.rand(6, 50, generator=g)
    y = torch.rand(6, 50, generator=g) < 0.2
    ref = -(y.double() * torch.log(p.double() + 1e-5) + (1 - y.double()) * torch.log(1 - p.double() + 1e-5)).sum(1)
    got = evaluation.cross_entropy_rows(p, y)
    assert got.dtype == torch.float64
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=1e-6)


class _CpuModel:
    """Anything with predict(frames, num_frames) and vocab_size: a fixed projection of the mean frame through a sigmoid."""
    vocab_size = 12

    def __init__(self):
        self.w = torch.randn(8, self.vocab_size, generator=torch.Generator().manual_seed(5))

    def predict(self, frames, num_frames):
        return torch.sigmoid((frames.float() / 255.0).mean(dim=1) @ self.w)


def _cpu_batches(sizes=(4, 4, 3), seed=9):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i, B in enumerate(sizes):
        q = torch.randint(0, 256, (B, 6, 8), dtype=torch.uint8, generator=g)
        y = torch.rand(B, _CpuModel.vocab_size, generator=g) < 0.3
        out.append(([f"v{i}_{b}" for b in range(B)], q, y, torch.full((B,), 6, dtype=torch.int32)))
    return out


def test_evaluate_on_a_cpu_model_is_the_eval_util_loop():
    model, batches = _CpuModel(), _cpu_batches()
    got = evaluation.evaluate(model, iter(batches), top_k=5)
    m = eval_util.EvaluationMetrics(model.vocab_size, 5)
    for _, q, y, nf in batches:
        p = model.predict(q, nf)
        m.accumulate(p, y, evaluation.cross_entropy_rows(p, y))
    ref = m.get()
    for key in ("avg_hit_at_one", "avg_perr", "avg_loss", "gap", "aps"):
        assert got[key] == ref[key], key
    assert got["map"] == float(np.mean(ref["aps"]))
    assert got["num_examples"] == 11 and got["examples_per_second"] > 0
    with pytest.raises(ValueError):
        evaluation.evaluate(model, iter([]))
