"""-m "not gpu": the exact "%i %g" formatter of the inference CSV (csrc/format_pairs.h through lpm_format_pairs_host) against Python's own
formatting, byte for byte; the stand-alone exhaustive checker over its stratified subset, plain and under the host sanitizers; and the
native join of ids and rows against format_top_k_lines."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from learnablepoolingmethods_amd import _capi, ops
from learnablepoolingmethods_amd.inference import format_top_k_lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INDEXES = [0, 65535, -1, 2147483647, -2147483648]


def oracle_scores():
    """The issue's list, as float32 bit patterns (uint32)."""
    rng = np.random.default_rng(20)
    bits = []
    for field in range(256):                                   # every exponent field: mantissas 0, 1, 0x7fffff and 256 random ones, both signs
        mant = np.concatenate([np.array([0, 1, 0x7FFFFF], dtype=np.uint32), rng.integers(0, 1 << 23, size=256, dtype=np.uint32)])
        for sign in (0, 1):
            bits.append((np.uint32(sign << 31) | np.uint32(field << 23) | mant).astype(np.uint32))
    # both zeros, both infinities, NaNs of both signs
    bits.append(np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], dtype=np.uint32))
    # the three floats on either side of 10^X, X in -45..38 (and the nearest float itself)
    near = []
    for X in range(-45, 39):
        centre = np.float32(float("1e%d" % X))
        b = int(centre.view(np.uint32)) if centre > 0 else 0
        near.extend(v for v in range(b - 3, b + 4) if 0 <= v < 0x7F800000)
    bits.append(np.array(near, dtype=np.uint32))
    # n + 0.5 for n in 100000..999999 step 37: the exact ties
    ties = (np.arange(100000, 1000000, 37, dtype=np.float64) + 0.5).astype(np.float32)
    assert np.all(ties.astype(np.float64) % 1.0 == 0.5)
    bits.append(ties.view(np.uint32))
    bits.append(np.array([2.0 ** -j for j in range(1, 31)], dtype=np.float32).view(np.uint32))
    return np.concatenate(bits)


def test_host_formatter_equals_python_on_the_oracle_list():
    bits = oracle_scores()
    k = 20
    rows = -(-bits.size // k)
    padded = np.zeros(rows * k, dtype=np.uint32)
    padded[:bits.size] = bits
    scores = torch.from_numpy(padded.view(np.float32).reshape(rows, k).copy())
    classes = torch.from_numpy(np.resize(np.array(INDEXES, dtype=np.int64), rows * k).astype(np.int32).reshape(rows, k))
    text, length = ops.format_pairs(classes, scores)
    stride = ops.format_pairs_stride(k)
    assert stride == 512 and text.shape == (rows, stride) and length.shape == (rows,) and length.dtype == torch.int32
    t, ln = text.numpy(), length.numpy()
    cl, sc = classes.numpy(), scores.numpy()
    bad = []
    for r in range(rows):
        want = (" ".join("%i %g" % (int(c), float(np.float32(s))) for c, s in zip(cl[r], sc[r])) + "\n").encode()
        got = t[r, :ln[r]].tobytes()
        if got != want or ln[r] != len(want):
            bad.append((r, got, want))
    assert not bad, bad[:3]
    # the named cases of the contract
    named = {100000.5: "100000", 100001.5: "100002", 2.0 ** -9: "0.00195312", 999999.5: "1e+06", 9.9999997e-05: "0.0001", -0.0: "-0",
             float("inf"): "inf", float("-inf"): "-inf", float("nan"): "nan", -1.17549435e-38: "-1.17549e-38", 1e-45: "1.4013e-45"}
    s1 = torch.tensor([list(named)], dtype=torch.float32)
    c1 = torch.arange(len(named), dtype=torch.int32).reshape(1, -1)
    t1, l1 = ops.format_pairs(c1, s1)
    assert t1[0, :int(l1[0])].numpy().tobytes().decode() == " ".join(f"{i} {v}" for i, v in enumerate(named.values())) + "\n"
    neg_nan = torch.from_numpy(np.array([[0xFFC00000]], dtype=np.uint32).view(np.float32))
    t2, l2 = ops.format_pairs(torch.tensor([[-2147483648]], dtype=torch.int32), neg_nan)
    assert t2[0, :int(l2[0])].numpy().tobytes() == b"-2147483648 nan\n"


def test_strides_limits_and_the_packed_buffer():
    assert [ops.format_pairs_stride(k) for k in (1, 7, 20, 64)] == [32, 176, 512, 1600]
    lib = _capi.load()
    assert lib._lpm_format_pairs_stride(0) == 0 and lib._lpm_format_pairs_stride(65) == 0
    for k in (0, 65):
        with pytest.raises(_capi.LpmError):
            ops.format_pairs(torch.zeros(1, k, dtype=torch.int32), torch.zeros(1, k))
    with pytest.raises(_capi.LpmError):
        ops.format_pairs(torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, 3))
    # the worst case fills a slot exactly as far as the stride allows, and nothing behind the packed buffer's two views is touched
    B, k = 3, 64
    stride = ops.format_pairs_stride(k)
    classes = torch.full((B, k), -2147483648, dtype=torch.int32)
    scores = torch.full((B, k), -1.17549435e-38)
    big = torch.full((16 + B * (stride + 4) + 16,), 0xAA, dtype=torch.uint8)
    text, length = ops.format_pairs(classes, scores, out=big[16:16 + B * (stride + 4)])
    assert length.tolist() == [25 * k] * B and text.data_ptr() == big.data_ptr() + 16
    assert text[1, :25 * k].numpy().tobytes() == b" ".join([b"-2147483648 -1.17549e-38"] * k) + b"\n"
    assert bool((big[:16] == 0xAA).all()) and bool((big[-16:] == 0xAA).all())


def _compile(cxx, flags, out):
    src = os.path.join(ROOT, "tools", "format_pairs_exhaustive.cc")
    subprocess.run([cxx, "-std=c++17", "-pthread", *flags, src, "-o", out], check=True, capture_output=True, text=True)


@pytest.fixture(scope="module")
def cxx():
    exe = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if exe is None:
        pytest.skip("no host C++ compiler")
    return exe


def test_exhaustive_checker_subset_plain_and_sanitized(tmp_path, cxx):
    """tools/format_pairs_exhaustive.cc (--all: the 2^32 patterns, run by hand; its result is in profiles/bench_inference.json) over its
    stratified subset: a plain build, and one with AddressSanitizer and UBSan -- a stand-alone host program, nothing loaded into Python."""
    plain, san = str(tmp_path / "fpe"), str(tmp_path / "fpe_san")
    _compile(cxx, ["-O2"], plain)
    _compile(cxx, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], san)
    for exe in (plain, san):
        r = subprocess.run([exe, "--subset"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert '"float_mismatches": 0' in r.stdout and '"int_mismatches": 0' in r.stdout, r.stdout


def test_join_equals_format_top_k_lines():
    rng = np.random.default_rng(3)
    B, k = 6, 5
    ids = ["first", "", "café-\U0001d11e", "with,comma", "x" * 40, "last"]
    classes = torch.from_numpy(rng.integers(0, 3862, size=(B, k)).astype(np.int32))
    scores = torch.from_numpy(rng.random((B, k), dtype=np.float32))
    text, length = ops.format_pairs(classes, scores)
    want = "".join(format_top_k_lines(ids, classes, scores)).encode("utf-8")
    assert bytes(ops.csv_join_rows(ids, text, length)) == want
    as_bytes = [v.encode("utf-8") for v in ids]
    assert bytes(ops.csv_join_rows(as_bytes, text, length)) == want
    nul = list(ids)
    nul[3] = "a\0b"                                            # an id that holds the blob's separator
    assert bytes(ops.csv_join_rows(nul, text, length)) == "".join(format_top_k_lines(nul, classes, scores)).encode("utf-8")
    with pytest.raises(_capi.LpmError):
        ops.csv_join_rows(ids[:-1], text, length)
    broken = length.clone()
    broken[2] = text.shape[1] + 1
    with pytest.raises(_capi.LpmError, match="row 2"):
        ops.csv_join_rows(ids, text, broken)
