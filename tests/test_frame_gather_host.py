"""-m "not gpu": the host side of the indexed frame-prep forms -- the *_idx entry points are declared, exported and bound;
model_utils.random_frame_index names the frames SampleRandomFrames gathers; ops.frame_gather_bn_split and the five triangulation
models refuse CPU uint8 frames (no silent fall-back); the flag exists.  (Trainer._quantised_frames needs a tensor on the GPU: its
check is in tests/test_gpu_frame_gather.py.)"""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lpm_hip.h")
# fp32 form -> position of `raw` in its parameter list; its q8 form takes (q, inv_norm, max, min) there
IDX_FORMS = {"lpm_frame_stats_idx": 0, "lpm_frame_apply_split_idx": 0, "lpm_frame_bn_bwd_split_idx": 5}
MODELS = ("RegularizedTriangulationModel", "SoftAttentionTriangulationModel", "TriangulationCnnClusterModel", "JuhanTestModelV5",
          "JuhanTestModelV1")


def test_indexed_entry_points_are_declared_exported_and_bound():
    from learnablepoolingmethods_amd import _build, _capi
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    if not os.path.exists(_capi.LIB_PATH):
        _build.build(verbose=False)
    dll = ctypes.CDLL(_capi.LIB_PATH)

    def params(name):
        return [p.strip().split()[-1].lstrip("*") for p in re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", txt).group(1).split(",")]
    names = ["lpm_frame_inv_norm_q8_idx"] + [n + s for n in IDX_FORMS for s in ("", "_q8")]
    for name in names:
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), f"{name} not declared in lpm_hip.h"
        assert hasattr(dll, name), f"{name} not exported"
        assert name in _capi.SIGNATURES, f"{name} missing from the ctypes table"
        assert len(params(name)) == len(_capi.SIGNATURES[name][1]), name
        assert "frame_index" in params(name), name
    for name, at in IDX_FORMS.items():
        fp32 = _capi.SIGNATURES[name][1]
        assert _capi.SIGNATURES[name + "_q8"][1] == fp32[:at + 1] + [ctypes.c_void_p, ctypes.c_float, ctypes.c_float] + fp32[at + 1:], name
        assert params(name + "_q8")[at:at + 4] == ["q", "inv_norm", "max_quantized_value", "min_quantized_value"]
        # the table stands where the uniform form has num_frames
        uniform = name.replace("_idx", "").replace("apply_split", "apply_tiles_split")
        assert params(name).index("frame_index") == params(uniform).index("num_frames"), name
    # the inverse norms need both: the table names the frame, num_frames says whether it is padding
    p = params("lpm_frame_inv_norm_q8_idx")
    assert p[:3] == ["q", "num_frames", "frame_index"] and p[3:] == params("lpm_frame_inv_norm_q8")[2:]


def test_random_frame_index_names_the_frames_sample_random_frames_gathers():
    from learnablepoolingmethods_amd import model_utils
    g = torch.Generator().manual_seed(3)
    B, MF, F, S = 6, 300, 8, 9
    x = torch.randn(B, MF, F, generator=g)
    nf = torch.tensor([0, 1, 300, 299, 7, 120], dtype=torch.int32)
    u = torch.rand(B, S, generator=g)
    u[:, 0] = 1 - 2 ** -24                                      # the largest fp32 below 1
    u[:, 1] = 0.0
    idx = model_utils.random_frame_index(nf, S, uniform=u)
    assert idx.dtype == torch.int32 and idx.shape == (B, S)
    want = model_utils.SampleRandomFrames(x, nf.reshape(-1, 1), S, uniform=u)
    got = x[torch.arange(B).unsqueeze(1), idx.long().clamp(0, MF - 1)]
    assert torch.equal(got, want)
    # ... by the formula int32(fp32(u) * fp32(num_frames)): 0 for the clips of 0 and 1 frames (an empty clip's index EQUALS num_frames)
    assert torch.equal(idx, (u * nf.reshape(-1, 1).float()).to(torch.int32))
    assert torch.equal(idx[0], torch.zeros(S, dtype=torch.int32)) and int(idx[1].max()) <= 1
    assert int(idx[2, 0]) == 299 and int(idx[5, 0]) == 119, "fp32((1 - 2**-24) * n) stays below n for these n"
    assert int(idx.min()) == 0 and bool((idx[2:] < nf[2:].reshape(-1, 1)).all())
    # the draw itself: in range, on num_frames' device
    drawn = model_utils.random_frame_index(nf, 50)
    assert drawn.shape == (B, 50) and bool((drawn >= 0).all()) and bool((drawn <= nf.reshape(-1, 1)).all()) and int(drawn[4].max()) > 0


def test_the_op_refuses_cpu_tensors_and_training_without_the_keyword():
    from learnablepoolingmethods_amd import ops
    from learnablepoolingmethods_amd._capi import LpmError
    q, nf = torch.zeros(2, 10, 1152, dtype=torch.uint8), torch.tensor([10, 4], dtype=torch.int32)
    idx = torch.zeros(2, 5, dtype=torch.int32)
    bn = (torch.ones(1152), torch.zeros(1152), torch.zeros(1152), torch.ones(1152))
    with pytest.raises(LpmError, match="eval mode only"):
        ops.frame_gather_bn_split(q, nf, idx, *bn, True, 1024)
    with pytest.raises(LpmError, match="eval mode only"):
        ops.frame_gather_bn_split(q, nf, idx, None, None, None, None, True, 1024, quantised_training=False)
    with pytest.raises(LpmError):                               # CPU frames: the q8 path is the GPU's
        ops.frame_gather_bn_split(q, nf, idx, *bn, True, 1024, quantised_training=True)
    with pytest.raises(LpmError, match="on the GPU"):
        ops.frame_gather_bn_split(q, nf, idx, *bn, False, 1024)
    with pytest.raises(LpmError, match="on the GPU"):
        ops.frame_gather_bn_split(q.float(), nf, idx, *bn, True, 1024)
    for training in (False, True):
        for kw in (False, True):
            assert ops.frame_gather_bn_split_ok(q, 1024, training, kw) is False
            assert ops.frame_gather_bn_split_ok(q.float(), 1024, training, kw) is False


@pytest.mark.parametrize("model", MODELS)
def test_the_models_refuse_cpu_uint8_frames(model):
    from learnablepoolingmethods_amd import registry
    from learnablepoolingmethods_amd import variables as vs
    from learnablepoolingmethods_amd._capi import LpmError
    q, nf = torch.zeros(2, 10, 1152, dtype=torch.uint8), torch.tensor([10, 4])
    for training in (False, True):
        store = vs.VariableStore(device="cpu")
        with vs.use_store(store), vs.variable_scope("tower"), pytest.raises(LpmError, match="train.normalize_input"):
            registry.get_model(model).create_model(q, vocab_size=10, num_frames=nf, iterations=5, video_anchor_size=2, audio_anchor_size=2,
                                                   is_training=training, quantised_training=training)


def test_the_flag_exists_and_the_routing_names_the_five_models():
    from learnablepoolingmethods_amd import FLAGS, predictor
    assert isinstance(FLAGS.gather_frames_fused, bool)
    assert predictor.GATHER_Q8_MODELS == MODELS and "WillowModelReg" not in predictor.GATHER_Q8_MODELS + predictor.FUSED_Q8_MODELS
    # a CPU batch is never handed over unnormalised
    q = torch.zeros(2, 10, 1152, dtype=torch.uint8)
    from learnablepoolingmethods_amd import registry
    assert not any(predictor.takes_quantised_frames(registry.get_model(m), q) for m in MODELS)
