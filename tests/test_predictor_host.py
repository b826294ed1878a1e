"""-m "not gpu": the forward-only path's host side -- the new C-ABI entry points are declared, exported and bound; uint8 frames are
refused in training; Predictor / topk_rows argument checks fire before any GPU work; the top-k CSV lines are format_lines' lines."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lpm_hip.h")
NEW_SYMBOLS = ("lpm_frame_inv_norm_q8", "lpm_frame_apply_q8", "lpm_frame_apply_tiles_q8", "lpm_frame_apply_tiles_split_q8",
               "lpm_frame_apply_tiles2_q8", "lpm_frame_apply_tiles_bf16_q8", "lpm_topk_rows")


def test_forward_only_entry_points_are_declared_exported_and_bound():
    from learnablepoolingmethods_amd import _build, _capi
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    if not os.path.exists(_capi.LIB_PATH):
        _build.build(verbose=False)
    dll = ctypes.CDLL(_capi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), f"{name} not declared in lpm_hip.h"
        assert hasattr(dll, name), f"{name} not exported"
        assert name in _capi.SIGNATURES, f"{name} missing from the ctypes table"
    # each quantised apply form takes its fp32 form's parameters with (q, inv_norm, max, min) in place of raw
    for name in NEW_SYMBOLS[1:-1]:
        fp32 = _capi.SIGNATURES[name[:-3]][1]
        assert _capi.SIGNATURES[name][1] == fp32[:1] + [ctypes.c_void_p, ctypes.c_float, ctypes.c_float] + fp32[1:], name


@pytest.mark.parametrize("model", ["NetVladV1", "NetVladV2"])
def test_uint8_frames_are_refused_in_training(model):
    from learnablepoolingmethods_amd import registry
    from learnablepoolingmethods_amd import variables as vs
    from learnablepoolingmethods_amd._capi import LpmError
    store = vs.VariableStore(device="cpu")
    with vs.use_store(store), pytest.raises(LpmError, match="eval mode only"):
        registry.get_model(model).create_model(torch.zeros(2, 10, 1152, dtype=torch.uint8), vocab_size=10,
                                               num_frames=torch.tensor([10, 4]), iterations=5, cluster_size=8, hidden_size=8,
                                               is_training=True)


def test_frame_sample_bn_refuses_uint8_in_training():
    from learnablepoolingmethods_amd import ops
    from learnablepoolingmethods_amd._capi import LpmError
    q, nf = torch.zeros(2, 10, 1152, dtype=torch.uint8), torch.tensor([10, 4])
    with pytest.raises(LpmError, match="eval mode only"):
        ops.frame_sample_bn(q, nf, 5, is_training=True)
    with pytest.raises(LpmError, match="eval mode only"):
        ops.frame_sample_bn_split(q, nf, 5, None, None, None, None, True, 1024)
    assert not ops.frame_sample_bn_split_ok(q, 1024, is_training=True)


def _cpu_predictor(vocab=10):
    from learnablepoolingmethods_amd import registry
    from learnablepoolingmethods_amd.predictor import Predictor
    return Predictor(registry.get_model("NetVladV1"), vocab, {}, "cpu")


def test_predictor_argument_checks():
    from learnablepoolingmethods_amd._capi import LpmError
    pr = _cpu_predictor(vocab=10)
    nf = torch.tensor([3, 4])
    with pytest.raises(LpmError, match="frames"):
        pr.predict(torch.zeros(2, 5, 1152, dtype=torch.int32), nf)          # dtype
    with pytest.raises(LpmError, match="frames"):
        pr.predict(torch.zeros(2, 1152, dtype=torch.uint8), nf)             # rank
    with pytest.raises(LpmError, match="num_frames"):
        pr.predict(torch.zeros(2, 5, 1152, dtype=torch.uint8), torch.tensor([3, 4, 5]))
    with pytest.raises(LpmError, match="num_frames"):
        pr.predict(torch.zeros(2, 5, 1152, dtype=torch.uint8), torch.tensor([3.0, 4.0]))
    for k in (0, 11, 65):
        with pytest.raises(LpmError, match="top_k"):
            pr.top_k(torch.zeros(2, 5, 1152, dtype=torch.uint8), nf, k)


def test_topk_rows_argument_checks():
    from learnablepoolingmethods_amd import ops
    from learnablepoolingmethods_amd._capi import LpmError
    for p, k in ((torch.zeros(2, 10), 0), (torch.zeros(2, 10), 11), (torch.zeros(2, 100), 65), (torch.zeros(2, 70000), 5),
                 (torch.zeros(2, 10, dtype=torch.float64), 5), (torch.zeros(10), 5)):
        with pytest.raises(LpmError):
            ops.topk_rows(p, k)


def test_top_k_lines_are_format_lines():
    from learnablepoolingmethods_amd import inference
    g = torch.Generator().manual_seed(0)
    p = torch.rand(4, 50, generator=g)
    p[1, 7] = p[1, 3]                                                       # a tie: ascending class order
    ids = ["a", b"b", "c", "d"]
    sv, si = torch.sort(p, dim=1, descending=True, stable=True)
    assert list(inference.format_top_k_lines(ids, si[:, :20].int(), sv[:, :20])) == list(inference.format_lines(ids, p, 20))
