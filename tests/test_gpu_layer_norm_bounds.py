"""-m gpu: the layer-norm family of csrc/layer_norm.hip (ops._ResidualLayerNorm, ops._ln_pair_forward, ops.residual_layer_norm) against the
fp64 restatement of tests/_layer_norm_ref.py -- never against the op itself -- per named part and per example.

Rule (tests/test_gpu_netvlad_bounds.py): the restatement evaluated in fp32 on the CPU (two-pass moments, as tf.nn.moments) carries an error
err32 against fp64; the op's error must be at most max(8 err32, 1e-6), per part.  The error figure of a part with an example axis (y, da, dr,
da1, dzy) is the maximum over the examples of (max |error| in the example / max |fp64 value| in the example), of dgamma / dbeta / dbias the
maximum over the tensor; example b's upstream gradient is N(0, 1) times 10^(6 b / (B - 1) - 3), so an error confined to the example with the
small gradient shows.  Every element of every part counts.  A part that is identically zero in fp64 must be exactly zero.  Every figure is
printed before anything is asserted.

The route is asserted: the entry names that pass through _capi._Lib.check are recorded, and the lpm_layer_norm_* ones must be exactly the
case's list, with multiplicity.  Every case is the minimal set of calls through ops._ResidualLayerNorm.forward / backward with ops._SubCtx, as
the block Functions make them.

case              (B, L, F)      form                                         why this shape / entries (lpm_layer_norm_ dropped)
one_row           (3, 1, 128)    residual                                     32 float4 per example: 15 of 16 chunks empty, row groups without rows
few_rows          (2, 7, 256)    bias + relu + residual                       fewer rows than row groups x chunks
ragged            (2, 33, 128)   residual                                     1056 float4: no multiple of 256; 33 rows over 8 x 16 row slots
two_rounds        (2, 130, 128)  bias + relu + residual                       rows past one round of LN_NB x RG = 128
wide              (3, 17, 1024)  bias, no relu, residual                      RG = 1: chunk 0 alone gets a second row
f512              (2, 20, 512)   plain (no r, no bias)                        the fourth width; z aliases a
many_examples     (33, 2, 128)   bias + relu + residual                       B LN_NB = 528 > 512: ln_colreduce_kernel's second round
single            (1, 64, 256)   residual                                     B = 1
row_scale         (2, 33, 128)   residual with r_scale [B L] in (0.5, 2)      act_fwd_rs
masked, _bool     (2, 33, 256)   bias + relu + keep mask (p 0.1, x 10) + res  act_mask_image_fwd, act_mask_bwd; mask as uint8 and as bool, da in fp32
image_bf16/_fp16  (2, 33, 128)   residual, image=True (fp16: an OperandSite)  act_image_fwd: y beside the image
pair, pair_wide   (2, 33, 128), (3, 17, 1024)  ops._ln_pair_forward, then backward(c2, dout), backward(c1, dz2, dr_extra=dz2) as
                                               ops._FFNBlockX3.backward chains them: pair_fwd + act_bwd x 2
pair_vs_separate  (2, 33, 128)   the pair as two _ResidualLayerNorm.forward   act_fwd x 2 + act_bwd x 2, under the same rule
slot, slot_pair   (3, 7, 256)    out= an ops.OutputSlot inside a wider buffer every byte outside the slot unchanged; a single norm and the pair
strided_dy        (3, 7, 256)    dy a column slice of a [B, total] buffer     read in place: the kernel is handed the view's pointer and stride
Regimes (tests/_layer_norm_ref.make_inputs): offset3 / offset10 / offset30 (r = R + N(0, 1): mean / std of z about R, three seeds each) and
scale_spread (rstd over four decades) on ragged, two_rounds, wide, pair and pair_wide.
Not cases: a constant example (fp64 variance 0, rstd = 1e6: any fp32 rounding of the mean is O(0.1) -- the extreme of the offset regime), and
the bitwise image identities, which tests/test_gpu_kernels.py holds.

Seeds: SEEDS below, the condition values of tests/_layer_norm_ref.conditions beside each.

Measured on the MI355X, worst error / bound over parts and seeds (the part that gives it in brackets).  "before": the moments from raw sums
alone, var = q/n - mu^2 from fp32 sums of z and z^2 (csrc/layer_norm.hip before this file existed); "after": today's fold, which takes those
raw sums where mean^2 <= var and sums shifted by the example's first z elsewhere (ln_moments) -- so every random and scale_spread row is the
same arithmetic before and after, bit for bit.  Nothing was modelled into the restatement: the plain two-pass fp32 evaluation bounds every
part of every case.
MEASURED-BEGIN
Before: every random and scale_spread case and offset3 within the bound (0.10 .. 0.32); offset10 and offset30 NOT -- 9 of the 41 tests
fail, each at its first seed, so the "before" figures of those rows are seed 0's alone:
case (regime)              before                after
one_row                    0.12 (y)              0.12 (y)
few_rows                   0.12 (dbias)          0.12 (dbias)
ragged                     0.10 (y)              0.10 (y)
two_rounds                 0.10 (y)              0.10 (y)
wide                       0.13 (da)             0.13 (da)
f512                       0.13 (da)             0.13 (da)
many_examples              0.13 (da)             0.13 (da)
single                     0.11 (y)              0.11 (y)
row_scale                  0.10 (dgamma)         0.10 (dgamma)
masked / masked_bool       0.14 (dgamma)         0.14 (dgamma)
image_bf16 / image_fp16    0.10 (y)              0.10 (y)
pair                       0.17 (dgamma1)        0.17 (dgamma1)
pair_wide                  0.15 (dzy)            0.15 (dzy)
pair_vs_separate           0.17 (dgamma1)        0.17 (dgamma1)
slot / slot_pair           0.10 (y) / 0.15 (dgamma2)   0.10 (y) / 0.15 (dgamma2)
strided_dy                 0.10 (y)              0.10 (y)
ragged (offset3)           0.29 (dgamma)         0.27 (dgamma)
ragged (offset10)          3.26 (da)   FAILS     0.17 (dgamma)
ragged (offset30)          3.44 (da)   FAILS     0.23 (da)
ragged (scale_spread)      0.12 (y)              0.12 (y)
two_rounds (offset3)       0.23 (dr)             0.11 (dr)
two_rounds (offset10)      1.64 (da)   FAILS     0.12 (dgamma)
two_rounds (offset30)      8.06 (dr)   FAILS     0.14 (dgamma)
two_rounds (scale_spread)  0.10 (y)              0.10 (y)
wide (offset3)             0.16 (da)             0.13 (da)
wide (offset10)            1.08 (da)   FAILS     0.13 (da)
wide (offset30)            8.80 (dbias) FAILS    0.16 (da)
wide (scale_spread)        0.13 (da)             0.13 (da)
pair (offset3)             0.32 (dbeta1)         0.18 (y)
pair (offset10)            1.15 (dbeta1) FAILS   0.19 (dgamma1)
pair (offset30)            11.20 (da1) FAILS     0.31 (da1)
pair (scale_spread)        0.11 (y)              0.11 (y)
pair_wide (offset3)        0.18 (da1)            0.16 (y)
pair_wide (offset10)       0.69 (da1)            0.20 (y)
pair_wide (offset30)       2.56 (dbias) FAILS    0.13 (dgamma2)
pair_wide (scale_spread)   0.14 (dzy)            0.14 (dzy)
Per part, error / bound, before -> after (offset10; offset30):
ragged      y 1.24 -> 0.14, da = dr 3.26 -> 0.15, dgamma 0.65 -> 0.17;        y 0.68 -> 0.12, da = dr 3.44 -> 0.23, dgamma 0.17 -> 0.13
two_rounds  y 0.66 -> 0.12, da 1.64 -> 0.11, dr 1.46 -> 0.11, dbias 0.39 -> 0.05;   y 1.40 -> 0.12, da 7.45 -> 0.11, dr 8.06 -> 0.12, dbias 1.27 -> 0.11
wide        y 0.41 -> 0.12, da = dr 1.08 -> 0.13, dbias 0.59 -> 0.09;          y 1.78 -> 0.11, da = dr 8.76 -> 0.16, dgamma 1.18 -> 0.13, dbias 8.80 -> 0.15
pair        y 0.47 -> 0.17, da1 0.72 -> 0.15, dbeta1 1.15 -> 0.12;             y 1.07 -> 0.09, da1 11.20 -> 0.31, dzy 5.83 -> 0.21, dgamma1 1.80 -> 0.14,
                                                                               dbeta1 5.39 -> 0.11, dbias 8.71 -> 0.22
pair_wide   y 0.33 -> 0.20, da1 0.69 -> 0.13, dzy 0.40 -> 0.14;                y 0.59 -> 0.09, da1 2.15 -> 0.12, dzy 2.14 -> 0.12, dbeta1 1.84 -> 0.06, dbias 2.56 -> 0.10
The op's error on y as a multiple of err32, before -> after: offset3 0.9 .. 1.8 -> 0.8 .. 1.5; offset10 2.6 .. 9.9 -> 0.9 .. 1.6; offset30
4.7 .. 14.2 -> 0.7 .. 1.0 -- the shifted sums are as good as the two-pass fp32 evaluation at every offset.  Before, the gradients (da, dr, dbias)
miss the bound by more than y does: it is they that show the defect first.
Shifted sums ALONE (the fold without the raw branch, measured on the way here) also met the rule everywhere, 0.10 .. 0.28 on the random rows:
there the pivot's distance from the mean costs more than the raw sums' cancellation (in the benched step, |mean|/std <= 0.23: the mean
4e-8 std off fp64 instead of 2e-9, rstd 1.9e-7 instead of 1.3e-7), which is why the fold keeps the raw sums for mean^2 <= var.
The whole file: 41 tests, 3 s (--durations: 0.3 s the first test, which loads the library; 0.17 s the slot case; 0.03 s or less each other).
MEASURED-END"""
import functools
import math

import pytest
import torch

from tests import _layer_norm_ref as R
from tests._util import cuda

pytestmark = pytest.mark.gpu

PREFIX = "lpm_layer_norm_"
SINGLE = ("act_fwd", "act_bwd")
PAIR = ("pair_fwd", "act_bwd", "act_bwd")


def _case(shape, form, route=SINGLE, **opts):
    return dict(shape=shape, form=form, route=tuple(route), opts=opts)


CASES = {
    "one_row": _case((3, 1, 128), "residual"),
    "few_rows": _case((2, 7, 256), "bias_relu_residual"),
    "ragged": _case((2, 33, 128), "residual"),
    "two_rounds": _case((2, 130, 128), "bias_relu_residual"),
    "wide": _case((3, 17, 1024), "bias_residual"),
    "f512": _case((2, 20, 512), "plain"),
    "many_examples": _case((33, 2, 128), "bias_relu_residual"),
    "single": _case((1, 64, 256), "residual"),
    "row_scale": _case((2, 33, 128), "row_scale", route=("act_fwd_rs", "act_bwd")),
    "masked": _case((2, 33, 256), "masked", route=("act_mask_image_fwd", "act_mask_bwd"), mask_dtype=torch.uint8),
    "masked_bool": _case((2, 33, 256), "masked", route=("act_mask_image_fwd", "act_mask_bwd"), mask_dtype=torch.bool),
    "image_bf16": _case((2, 33, 128), "residual", route=("act_image_fwd", "act_bwd"), image="bf16"),
    "image_fp16": _case((2, 33, 128), "residual", route=("act_image_fwd", "act_bwd"), image="fp16"),
    "pair": _case((2, 33, 128), "pair", route=PAIR),
    "pair_wide": _case((3, 17, 1024), "pair", route=PAIR),
    "pair_vs_separate": _case((2, 33, 128), "pair", route=SINGLE + SINGLE, separate=True),
    "slot": _case((3, 7, 256), "bias_relu_residual", slot=True),
    "slot_pair": _case((3, 7, 256), "pair", route=PAIR, slot=True),
    "strided_dy": _case((3, 7, 256), "bias_relu_residual", strided_dy=True),
}
REGIME_CASES = ("ragged", "two_rounds", "wide", "pair", "pair_wide")

# per case (or (case, regime)): the seeds, and beside them the condition values of tests/_layer_norm_ref.conditions per seed --
# min and max over the examples of |mean| / std of z, the least variance, the least maximum of a part (per example where it has that axis)
SEEDS = {
    # SEEDS-BEGIN
    "one_row": (0,),                                      # 3.9e-02, 1.2e-01, 1.7e+00, 2.2e-03
    "few_rows": (0,),                                     # 3.3e-01, 3.4e-01, 1.3e+00, 5.2e-03
    "ragged": (0,),                                       # 2.8e-03, 2.5e-02, 2.0e+00, 3.0e-03
    "two_rounds": (0,),                                   # 3.4e-01, 3.4e-01, 1.3e+00, 4.1e-03
    "wide": (0,),                                         # 3.9e-03, 7.0e-03, 2.1e+00, 3.4e-03
    "f512": (0,),                                         # 9.8e-03, 1.6e-02, 1.0e+00, 4.8e-03
    "many_examples": (0,),                                # 1.4e-01, 4.7e-01, 1.2e+00, 2.6e-03
    "single": (0,),                                       # 1.8e-02, 1.8e-02, 2.0e+00, 3.5e+00
    "row_scale": (0,),                                    # 7.4e-03, 1.1e-02, 2.9e+00, 2.4e-03
    "masked": (0,),                                       # 1.6e-01, 1.7e-01, 6.4e+00, 2.0e-03
    "masked_bool": (0,),                                  # 1.6e-01, 1.7e-01, 6.4e+00, 2.0e-03
    "image_bf16": (0,),                                   # 2.8e-03, 2.5e-02, 2.0e+00, 3.0e-03
    "image_fp16": (0,),                                   # 2.8e-03, 2.5e-02, 2.0e+00, 3.0e-03
    "pair": (0,),                                         # 4.3e-03, 3.7e-01, 1.4e+00, 2.0e-03
    "pair_wide": (0,),                                    # 2.6e-03, 3.6e-01, 1.4e+00, 2.5e-03
    "pair_vs_separate": (0,),                             # 4.3e-03, 3.7e-01, 1.4e+00, 2.0e-03
    "slot": (0,),                                         # 3.1e-01, 3.6e-01, 1.3e+00, 3.1e-03
    "slot_pair": (0,),                                    # 9.6e-03, 3.6e-01, 1.3e+00, 1.7e-03
    "strided_dy": (0,),                                   # 3.1e-01, 3.6e-01, 1.3e+00, 3.1e-03
    ("ragged", "offset3"): (0, 1, 2),                     # 2.1e+00, 2.1e+00, 2.0e+00, 3.0e-03; 2.1e+00, 2.1e+00, 2.0e+00, 3.5e-03; 2.1e+00, 2.1e+00, 2.0e+00, 2.8e-03
    ("ragged", "offset10"): (0, 1, 2),                    # 7.0e+00, 7.1e+00, 2.0e+00, 3.0e-03; 7.0e+00, 7.1e+00, 2.0e+00, 3.5e-03; 7.0e+00, 7.1e+00, 2.0e+00, 2.8e-03
    ("ragged", "offset30"): (0, 1, 2),                    # 2.1e+01, 2.1e+01, 2.0e+00, 3.0e-03; 2.1e+01, 2.1e+01, 2.0e+00, 3.5e-03; 2.1e+01, 2.1e+01, 2.0e+00, 2.8e-03
    ("ragged", "scale_spread"): (0,),                     # 2.8e-03, 2.5e-02, 2.0e-04, 3.0e-01
    ("two_rounds", "offset3"): (0, 1, 2),                 # 2.9e+00, 2.9e+00, 1.3e+00, 4.1e-03; 2.9e+00, 2.9e+00, 1.4e+00, 3.6e-03; 2.9e+00, 2.9e+00, 1.3e+00, 3.7e-03
    ("two_rounds", "offset10"): (0, 1, 2),                # 8.9e+00, 9.0e+00, 1.3e+00, 4.1e-03; 8.9e+00, 8.9e+00, 1.4e+00, 3.6e-03; 8.9e+00, 9.0e+00, 1.3e+00, 3.7e-03
    ("two_rounds", "offset30"): (0, 1, 2),                # 2.6e+01, 2.6e+01, 1.3e+00, 4.1e-03; 2.6e+01, 2.6e+01, 1.4e+00, 3.6e-03; 2.6e+01, 2.6e+01, 1.3e+00, 3.7e-03
    ("two_rounds", "scale_spread"): (0,),                 # 3.5e-01, 6.5e-01, 2.1e-02, 3.3e-02
    ("wide", "offset3"): (0, 1, 2),                       # 2.1e+00, 2.1e+00, 2.1e+00, 3.4e-03; 2.1e+00, 2.1e+00, 2.1e+00, 3.3e-03; 2.1e+00, 2.1e+00, 2.1e+00, 3.4e-03
    ("wide", "offset10"): (0, 1, 2),                      # 6.9e+00, 6.9e+00, 2.1e+00, 3.4e-03; 6.9e+00, 6.9e+00, 2.1e+00, 3.3e-03; 6.9e+00, 7.0e+00, 2.1e+00, 3.4e-03
    ("wide", "offset30"): (0, 1, 2),                      # 2.1e+01, 2.1e+01, 2.1e+00, 3.4e-03; 2.1e+01, 2.1e+01, 2.1e+00, 3.3e-03; 2.1e+01, 2.1e+01, 2.1e+00, 3.4e-03
    ("wide", "scale_spread"): (0,),                       # 1.8e-03, 2.7e-02, 9.2e-02, 1.6e-02
    ("pair", "offset3"): (0, 1, 2),                       # 1.6e+00, 2.9e+00, 1.4e+00, 2.0e-03; 1.5e+00, 2.9e+00, 1.3e+00, 2.4e-03; 1.5e+00, 3.0e+00, 1.3e+00, 2.0e-03
    ("pair", "offset10"): (0, 1, 2),                      # 5.2e+00, 8.9e+00, 1.4e+00, 2.0e-03; 5.1e+00, 9.0e+00, 1.3e+00, 2.4e-03; 5.1e+00, 9.0e+00, 1.3e+00, 2.0e-03
    ("pair", "offset30"): (0, 1, 2),                      # 1.6e+01, 2.6e+01, 1.4e+00, 2.0e-03; 1.5e+01, 2.6e+01, 1.3e+00, 2.4e-03; 1.5e+01, 2.6e+01, 1.3e+00, 2.0e-03
    ("pair", "scale_spread"): (0,),                       # 9.1e-03, 6.8e-01, 3.3e-02, 2.7e-02
    ("pair_wide", "offset3"): (0, 1, 2),                  # 1.5e+00, 2.9e+00, 1.4e+00, 2.5e-03; 1.5e+00, 2.9e+00, 1.4e+00, 2.4e-03; 1.6e+00, 2.9e+00, 1.3e+00, 2.4e-03
    ("pair_wide", "offset10"): (0, 1, 2),                 # 5.1e+00, 8.9e+00, 1.4e+00, 2.5e-03; 5.1e+00, 8.9e+00, 1.4e+00, 2.4e-03; 5.2e+00, 9.0e+00, 1.3e+00, 2.4e-03
    ("pair_wide", "offset30"): (0, 1, 2),                 # 1.5e+01, 2.6e+01, 1.4e+00, 2.5e-03; 1.5e+01, 2.6e+01, 1.4e+00, 2.4e-03; 1.6e+01, 2.6e+01, 1.3e+00, 2.4e-03
    ("pair_wide", "scale_spread"): (0,),                  # 2.0e-03, 6.8e-01, 3.3e-02, 3.0e-02
    # SEEDS-END
}


def seeds_of(name, regime="random"):
    return SEEDS[name if regime == "random" else (name, regime)]


@functools.lru_cache(maxsize=None)
def reference(name, seed, regime="random"):
    """-> (inputs, fp64 parts, fp32 parts, (ok, condition values)), computed once per (case, seed, regime) on the CPU."""
    case = CASES[name]
    inputs = R.make_inputs(*case["shape"], seed, regime)
    p64 = R.layer_norm_ref(inputs, torch.float64, case["form"])
    p32 = R.layer_norm_ref(inputs, torch.float32, case["form"])
    return inputs, p64, p32, R.conditions(inputs, case["form"], p64, regime)


def bounds(name, seed, regime="random"):
    """-> {part: (err32, bound)}"""
    _, p64, p32, _ = reference(name, seed, regime)
    B = CASES[name]["shape"][0]
    return {n: (e, max(8 * e, 1e-6)) for n, e in ((n, R.figure(p32[n], p64[n], n, B)) for n in p64)}


@pytest.fixture
def entries(monkeypatch):
    """The names that pass through _capi._Lib.check, in order."""
    from learnablepoolingmethods_amd import _capi
    seen = []
    original = _capi._Lib.check

    def check(self, status, what):
        seen.append(what)
        return original(self, status, what)
    monkeypatch.setattr(_capi._Lib, "check", check)
    return seen


SENTINEL = -12345.678
SLOT_PAD = 36            # floats either side of the slot: 144 bytes, the slot stays 16-byte aligned


def _slot(B, L, F, dev):
    from learnablepoolingmethods_amd import ops
    base = torch.full((B, L * F + 2 * SLOT_PAD), SENTINEL, device=dev)
    return base, ops.OutputSlot(base, SLOT_PAD, L, F)


def _assert_slot(base, y, L, F, tag):
    """y is the slot's view and every byte outside the slot still holds the sentinel."""
    n = L * F
    assert y.data_ptr() == base.data_ptr() + 4 * SLOT_PAD and y.stride(0) == base.shape[1], tag
    want = torch.full((1,), SENTINEL).view(torch.int32).item()
    bits = base.view(torch.int32)
    outside = torch.cat([bits[:, :SLOT_PAD], bits[:, SLOT_PAD + n:]], 1)
    assert bool((outside == want).all()), f"{tag}: bytes outside the output slot were written"
    assert bool(torch.isfinite(base[:, SLOT_PAD:SLOT_PAD + n]).all()) and not bool((bits[:, SLOT_PAD:SLOT_PAD + n] == want).any()), tag


def _upstream(inputs, case, dev):
    """-> (dy as the backward gets it, check to run afterwards or None).  strided_dy: a column slice of a wider NaN-filled buffer."""
    B, L, F = case["shape"]
    up = inputs["upstream"].to(dev)
    if not case["opts"].get("strided_dy"):
        return up
    total = L * F + 2 * SLOT_PAD
    buf = torch.full((B, total), float("nan"), device=dev)
    buf[:, SLOT_PAD:SLOT_PAD + L * F] = up.reshape(B, -1)
    dy = buf[:, SLOT_PAD:SLOT_PAD + L * F].unflatten(1, (L, F))
    assert dy.data_ptr() == buf.data_ptr() + 4 * SLOT_PAD and dy.stride() == (total, F, 1) and not dy.is_contiguous()
    return dy


def run_op(name, inputs, dev, monkeypatch):
    """The case's forward and backward calls -> {part: tensor} under the restatement's names."""
    from learnablepoolingmethods_amd import _capi, ops
    case = CASES[name]
    B, L, F = case["shape"]
    f, opts = R.FORMS[case["form"]], case["opts"]
    LN = ops._ResidualLayerNorm

    def g(key):
        return inputs[key].to(dev)
    a, gamma, beta = g("a"), g("gamma"), g("beta")
    r = g("r") if f.get("res") else None
    bias = g("bias") if f.get("bias") else None
    relu = bool(f.get("relu"))
    dy = _upstream(inputs, case, dev)
    base, out = _slot(B, L, F, dev) if opts.get("slot") else (None, None)
    if f.get("pair"):
        g2, be2 = g("gamma2"), g("beta2")
        c1, c2 = ops._SubCtx(), ops._SubCtx()
        if opts.get("separate"):
            n = LN.forward(c1, a, r, gamma, beta, bias, True)
            y = LN.forward(c2, n, r, g2, be2, None, False, out)
        else:
            y = ops._ln_pair_forward(c1, c2, a, r, gamma, beta, bias, g2, be2, out)
        dz2, _, dg2, dbe2 = LN.backward(c2, dy)[:4]                      # as ops._FFNBlockX3.backward chains them
        da1, dzy, dg1, dbe1, db2 = LN.backward(c1, dz2, dr_extra=dz2)[:5]
        parts = dict(y=y, da1=da1, dzy=dzy, dgamma1=dg1, dbeta1=dbe1, dgamma2=dg2, dbeta2=dbe2, dbias=db2)
    else:
        kw = {}
        if f.get("mask"):
            kw.update(mask=inputs["mask"].to(opts["mask_dtype"]).to(dev), mask_scale=R.MASK_SCALE)
        if opts.get("image"):
            kw["image"] = True
            if opts["image"] == "fp16":
                amax = torch.zeros(_capi.LPM_OPERAND_AMAX_SUB * _capi.LPM_OPERAND_AMAX_STRIDE, device=dev)
                kw["site"] = ops.OperandSite(True, 2.0 ** 7, amax.data_ptr(), role="a")
        ctx = ops._SubCtx()
        y = LN.forward(ctx, a, r, gamma, beta, bias, relu, out, g("r_scale") if f.get("row_scale") else None, **kw)
        if opts.get("image"):
            y3 = y._lpm_y3[0]
            assert y3.shape == (B * L, 3 * F) and y3.dtype == (torch.float16 if opts["image"] == "fp16" else torch.bfloat16)
        handed = []
        if opts.get("strided_dy"):            # what the library is handed: the view's own pointer and batch stride, no copy
            lib = _capi.load()
            entry = lib._lpm_layer_norm_act_bwd_fmt
            monkeypatch.setattr(lib, "_lpm_layer_norm_act_bwd_fmt", lambda *args: (handed.append((args[0].value, args[1])), entry(*args))[1])
        res = LN.backward(ctx, dy)
        if opts.get("strided_dy"):
            assert handed == [(dy.data_ptr(), dy.stride(0))], f"{name}: dy was not read in place: {handed}"
        parts = dict(y=y, da=res[0], dgamma=res[2], dbeta=res[3])
        if r is not None:
            parts["dr"] = res[1]
        if bias is not None:
            parts["dbias"] = res[4]
    torch.cuda.synchronize()
    if base is not None:
        _assert_slot(base, y, L, F, name)
    return parts


def check_parts(tag, got, name, seed, regime):
    """Figures, bounds and ratios of every part: printed, then asserted.  -> the worst ratio."""
    B = CASES[name]["shape"][0]
    _, p64, _, _ = reference(name, seed, regime)
    bnd = bounds(name, seed, regime)
    assert set(got) == set(p64), f"{tag}: parts {sorted(got)} against {sorted(p64)}"
    rows = []
    for n, (e32, bound) in bnd.items():
        e_op = R.figure(got[n], p64[n], n, B)
        zero = float(p64[n].abs().max()) == 0.0
        rows.append((n, e_op, e32, bound, zero))
        print(f"[layer_norm] {tag} {n}: op {e_op:.3e}, err32 {e32:.3e}, bound {bound:.3e}, ratio {e_op / bound:.3f}, op/err32 {e_op / e32:.2f}")
    for n, e_op, e32, bound, zero in rows:
        if zero:
            assert e_op == 0.0, f"{tag} {n}: identically zero in fp64, not exactly zero in the op"
        else:
            assert math.isfinite(e_op) and e_op <= bound, f"{tag} {n}: op error {e_op:.3e} > bound {bound:.3e} (err32 {e32:.3e})"
    worst = max((e_op / bound, n) for n, e_op, _, bound, zero in rows if not zero)
    print(f"[layer_norm] {tag} worst ratio {worst[0]:.3f} ({worst[1]})")
    return worst[0]


def check_case(name, seed, regime, dev, monkeypatch, entries):
    inputs, _, _, (ok, cond) = reference(name, seed, regime)
    tag = f"{name} {regime} seed {seed}"
    print(f"[layer_norm] {tag}: conditions {ok} " + ", ".join(f"{v:.2e}" for v in cond))
    assert ok, f"{tag}: the seed does not meet the conditions {cond}"
    del entries[:]
    got = run_op(name, inputs, dev, monkeypatch)
    reached = sorted(e for e in entries if e.startswith(PREFIX))
    print(f"[layer_norm] {tag} route: {reached}")
    worst = check_parts(tag, got, name, seed, regime)
    assert reached == sorted(PREFIX + n for n in CASES[name]["route"]), f"{tag}: reached {reached}"
    return worst


@pytest.mark.parametrize("name", list(CASES))
def test_op_meets_the_bound_on_every_route(name, monkeypatch, entries):
    from learnablepoolingmethods_amd import ops
    assert ops.LN_EPS == R.LN_EPS
    dev = cuda()
    for seed in seeds_of(name):
        check_case(name, seed, "random", dev, monkeypatch, entries)


@pytest.mark.parametrize("regime", R.REGIMES[1:])
@pytest.mark.parametrize("name", REGIME_CASES)
def test_op_meets_the_bound_in_every_regime(name, regime, monkeypatch, entries):
    dev = cuda()
    for seed in seeds_of(name, regime):
        check_case(name, seed, regime, dev, monkeypatch, entries)


def test_public_form_meets_the_bound_through_autograd(entries):
    """ops.residual_layer_norm, the autograd node around the same calls, at few_rows."""
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    name, seed = "few_rows", seeds_of("few_rows")[0]
    inputs = reference(name, seed)[0]
    a, r, gamma, beta, bias = (inputs[k].to(dev).requires_grad_(True) for k in ("a", "r", "gamma", "beta", "bias"))
    y = ops.residual_layer_norm(a, r, gamma, beta, bias=bias, relu=True)
    grads = torch.autograd.grad((y * inputs["upstream"].to(dev)).sum(), [a, r, gamma, beta, bias])
    torch.cuda.synchronize()
    got = dict(y=y.detach(), **dict(zip(("da", "dr", "dgamma", "dbeta", "dbias"), grads)))
    check_parts("few_rows through autograd", got, name, seed, "random")
    assert sorted(e for e in entries if e.startswith(PREFIX)) == sorted(PREFIX + n for n in SINGLE)


def test_backward_repeats_bit_for_bit_on_one_workspace():
    """Through the C ABI: two consecutive lpm_layer_norm_act_bwd calls with a bias on ONE workspace and stream at many_examples give the
    same bits in dgamma, dbeta and dbias -- the arrival counters of ln_colreduce_kernel live in the workspace and are re-armed by each
    call's first kernel (after the first call they stand at LN_RS).  A plain repeat, nothing else."""
    from learnablepoolingmethods_amd import _capi, ops
    dev = cuda()
    lib = _capi.load()
    name, seed = "many_examples", seeds_of("many_examples")[0]
    B, L, F = CASES[name]["shape"]
    inputs = reference(name, seed)[0]
    a, r, gamma, beta, bias, dy = (inputs[k].to(dev) for k in ("a", "r", "gamma", "beta", "bias", "upstream"))
    ctx = ops._SubCtx()
    ops._ResidualLayerNorm.forward(ctx, a, r, gamma, beta, bias, True)
    z, stats = ctx.saved_tensors[:2]
    wsb = lib._lpm_layer_norm_workspace_bytes(B, F)
    ws = torch.empty(wsb // 4, dtype=torch.float32, device=dev)
    runs = []
    for _ in range(2):
        dz, da = torch.empty_like(z), torch.empty_like(z)
        cols = [torch.full((F,), float("nan"), device=dev) for _ in range(3)]
        lib.check(lib._lpm_layer_norm_act_bwd(ops.ptr(dy), 0, ops.ptr(z), ops.ptr(stats), ops.ptr(gamma), ops.ptr(a), ops.ptr(bias), 1, B, L, F,
                                              ops.ptr(dz), ops.ptr(da), ops.ptr(cols[0]), ops.ptr(cols[1]), ops.ptr(cols[2]), None, None,
                                              ops.ptr(ws), wsb, ops.stream_ptr()), "lpm_layer_norm_act_bwd")
        runs.append([dz, da] + cols)
    torch.cuda.synchronize()
    for what, first, second in zip(("dz", "da", "dgamma", "dbeta", "dbias"), *runs):
        assert bool(torch.isfinite(first).all()), what
        assert torch.equal(first, second), f"{what} differs between two calls on one workspace"
    got = dict(da=runs[1][1], dr=runs[1][0], dgamma=runs[1][2], dbeta=runs[1][3], dbias=runs[1][4])
    p64 = reference(name, seed)[1]
    for n, (e32, bound) in bounds(name, seed).items():
        if n != "y":
            e_op = R.figure(got[n], p64[n], n, B)
            print(f"[layer_norm] many_examples, second call on the workspace {n}: op {e_op:.3e}, err32 {e32:.3e}, bound {bound:.3e}")
            assert e_op <= bound, n
