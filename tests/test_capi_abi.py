"""-m "not gpu": the C-ABI library loads on a CPU-only box and exports every symbol include/lpm_hip.h
declares, the ctypes table in _capi.py covers exactly those symbols, and the product path refuses CPU
tensors (no silent fallback).  No compute calls here."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lpm_hip.h")


def _declared():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(lpm_[a-z0-9_]+)\s*\(", txt)))


def test_header_declares_the_expected_entry_points():
    names = _declared()
    for must in ("lpm_assign_gemm_fwd", "lpm_vlad_aggregate_fwd", "lpm_vlad_aggregate_bwd", "lpm_mha_fwd", "lpm_mha_bwd",
                 "lpm_multi_tensor_clip_adam", "lpm_frame_apply", "lpm_version", "lpm_last_error"):
        assert must in names


def test_library_exports_every_declared_symbol():
    from learnablepoolingmethods_amd import _build, _capi
    if not os.path.exists(_capi.LIB_PATH):
        _build.build(verbose=False)
    dll = ctypes.CDLL(_capi.LIB_PATH)
    missing = [n for n in _declared() if not hasattr(dll, n)]
    assert not missing, f"declared in lpm_hip.h but not exported: {missing}"


def test_ctypes_table_matches_header():
    from learnablepoolingmethods_amd import _capi
    assert sorted(_capi.SIGNATURES) == _declared()
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, (_, args) in _capi.SIGNATURES.items():
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", txt, flags=re.S)
        assert m, name
        params = [a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]
        assert len(params) == len(args), f"{name}: header has {len(params)} parameters, ctypes table {len(args)}"


def test_frame_stats_partial_holds_the_raw_sums_the_shifted_sums_and_the_pivots():
    """lpm_frame_stats* fill, and lpm_frame_bn_fold reads, raw partials [nblk][2][F], shifted partials [nblk][2][F] and pivots [F];
    lpm_frame_bn_fold has lpm_bn_fold's parameters and `centre`; every lpm_frame_apply* form ends in (stream, centre)."""
    from learnablepoolingmethods_amd import _capi
    ret, args = _capi.SIGNATURES["lpm_bn_fold"]
    assert _capi.SIGNATURES["lpm_frame_bn_fold"] == (ret, args + [ctypes.c_void_p])              # ... and `centre` behind them
    header = open(HEADER).read()
    for name, (_, a) in _capi.SIGNATURES.items():
        if name.startswith("lpm_frame_apply"):
            assert a[-2:] == [ctypes.c_void_p, ctypes.c_void_p], name
            assert re.search(r"\b" + name + r"\s*\([^;]*lpm_stream_t stream, const float\* centre\);", header), name
    lib = _capi.load()
    for B, S, F in ((1, 3, 128), (2, 16, 1024), (5, 7, 128), (3, 33, 1152), (128, 300, 1152)):
        nblk = lib._lpm_frame_stats_nblk(B, S)
        assert nblk == (B * S + 31) // 32
        assert lib._lpm_frame_stats_workspace_bytes(B, S, F) == nblk * 2 * F * 4          # (the backward's workspace: unchanged)
        assert lib._lpm_frame_stats_partial_bytes(B, S, F) == (nblk * 4 * F + F) * 4


def test_frame_stats_refuse_a_partial_of_the_old_size():
    """The four lpm_frame_stats* forms take the size of `partial` and refuse, before any launch, a buffer of
    lpm_frame_stats_workspace_bytes -- what `partial` held before the shifted sums.  (The pointers are never dereferenced: the check fails.)"""
    from learnablepoolingmethods_amd import _capi
    lib = _capi.load()
    B, MF, F, S = 2, 40, 128, 7
    p = ctypes.c_void_p(4096)
    old, new = lib._lpm_frame_stats_workspace_bytes(B, S, F), lib._lpm_frame_stats_partial_bytes(B, S, F)
    assert new > 2 * old
    calls = {"lpm_frame_stats": lambda n: lib._lpm_frame_stats(p, p, B, MF, F, S, p, n, None),
             "lpm_frame_stats_idx": lambda n: lib._lpm_frame_stats_idx(p, p, B, MF, F, S, p, n, None),
             "lpm_frame_stats_q8": lambda n: lib._lpm_frame_stats_q8(p, p, 2.0, -2.0, p, B, MF, F, S, p, n, None),
             "lpm_frame_stats_idx_q8": lambda n: lib._lpm_frame_stats_idx_q8(p, p, 2.0, -2.0, p, B, MF, F, S, p, n, None)}
    for name, call in calls.items():
        assert _capi.SIGNATURES[name][1][-2] is ctypes.c_size_t, name
        for n in (old, new - 1):
            assert call(n) != 0 and name in lib.last_error() and "partial too small" in lib.last_error(), (name, n, lib.last_error())


def test_mha_logit_stats_shifted_refuses_a_partial_of_the_old_size():
    """lpm_mha_logit_stats_shifted fills partial [B*h][5][L] -- raw sums, sums about the pivots, pivots -- takes the size of the caller's
    buffer and refuses, before any launch, the [B*h][2][L] that lpm_mha_logit_stats(_moments) fill; lpm_mha_bn_fold has lpm_bn_fold's
    parameters.  (The pointers are never dereferenced: the check fails.)"""
    from learnablepoolingmethods_amd import _capi
    lib = _capi.load()
    assert _capi.SIGNATURES["lpm_mha_bn_fold"] == _capi.SIGNATURES["lpm_bn_fold"]
    moments = _capi.SIGNATURES["lpm_mha_logit_stats_moments"][1]
    assert _capi.SIGNATURES["lpm_mha_logit_stats_shifted"][1] == moments[:8] + [ctypes.c_size_t] + moments[8:]
    p = ctypes.c_void_p(4096)
    for B, L, h, d in ((2, 16, 1, 8), (3, 48, 2, 16), (80, 300, 64, 16)):
        new, old = lib._lpm_mha_logit_stats_partial_bytes(B, L, h), B * h * 2 * L * 4
        assert new == B * h * 5 * L * 4
        for n in (old, new - 1):
            assert lib._lpm_mha_logit_stats_shifted(p, p, h * d, B, L, h, d, p, n, p, None) != 0
            assert "lpm_mha_logit_stats_shifted" in lib.last_error() and "partial too small" in lib.last_error(), lib.last_error()
    assert lib._lpm_mha_logit_stats_partial_bytes(0, 16, 1) == 0


def test_version_and_error_string():
    from learnablepoolingmethods_amd import _capi
    lib = _capi.load()
    assert lib.version() == 100
    assert isinstance(lib.last_error(), str)


def test_product_path_refuses_cpu_tensors():
    from learnablepoolingmethods_amd import _capi, ops, registry
    from learnablepoolingmethods_amd import variables as vs
    with pytest.raises(_capi.LpmError):
        ops.netvlad(torch.zeros(8, 128), torch.zeros(128, 8), None, 4, bn=None, bias=torch.zeros(8))
    with pytest.raises(_capi.LpmError):
        ops.mha_core(torch.zeros(1, 16, 16), torch.zeros(1, 16, 16), torch.zeros(1, 16, 16), 1, 1.0)
    store = vs.VariableStore(device="cpu")
    with vs.use_store(store), pytest.raises(_capi.LpmError):
        registry.get_model("NetVladV1").create_model(torch.zeros(2, 10, 1152), vocab_size=10,
                                                     num_frames=torch.tensor([10, 10]), iterations=5,
                                                     cluster_size=8, hidden_size=8)


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "learnablepoolingmethods_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hip", ".h")):
                txt = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M), f"{f} imports the oracle"
