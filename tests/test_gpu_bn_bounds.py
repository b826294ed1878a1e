"""-m gpu: the batch-norm family of csrc/bn.hip (lpm_bn_rows_fwd / _act_fwd / _act_image_fwd_fmt, lpm_bn_bwd / _bwd_x16 / _act_bwd /
_act_bwd_image_fmt, lpm_bn_small_fwd / _bwd, lpm_bn_fold) against the fp64 restatement of tests/_bn_ref.py -- never against the op itself --
per named part, per example and per column.

Rule (tests/test_gpu_layer_norm_bounds.py, tests/test_gpu_netvlad_bounds.py): the restatement evaluated in fp32 on the CPU (two-pass moments)
carries an error err32 against fp64; the op's error must be at most max(8 err32, 1e-6), per part.  The figure of a part with a row axis (y,
dx, dmul) is the larger of the maximum over the examples of (max |error| in the example / max |fp64| in the example) and the maximum over the
columns of the same quotient per column -- a batch norm's defects are per column, and a figure over the tensor would hide a column with a
small gamma rstd; of dgamma, dbeta, dbias, batch_mean, batch_var and the moving statistics it is the maximum over the tensor.  Example b's
upstream gradient is N(0, 1) x 10^(6 b / (B - 1) - 3).  A part, a column of a row-axis part or a dead column's element of a column part that is
identically zero in fp64 must be exactly zero (the dead ReLU columns' dx, dgamma, dbias; their y must be beta, bit for bit).  Every figure
is printed before anything is asserted.  Nothing is modelled into the restatement beyond tests/_netvlad_ref.ONE_MINUS_DECAY.

The route is asserted: the names that pass through _capi._Lib.check are recorded, and the lpm_bn_* ones must be exactly the case's list,
with multiplicity.  The rows forms run ops._BatchNormRows / ops._BatchNormRowsAct forward and backward with an ops._SubCtx, the small ones
ops._BNSmall, the bf16 and image forms the C ABI.

case             (B, L, C)      form                              why this shape / entries (lpm_bn_ dropped)
few_rows         (1, 7, 128)    rows                              fewer rows than the 8 row groups at C/4 = 32
few_rows_act     (1, 7, 128)    rows_act, relu                    the same with the bias: dbias by the direct column sum (8 partial rows)
one_block_plus   (2, 33, 128)   rows_act, relu                    66 rows: a 2-row second block; the 8- and 4-row unroll tails
two_blocks       (2, 65, 128)   rows_act, relu                    130 rows; dbias through bn_colsum_stage1_kernel (136 partial rows > 64)
rg4, rg2         (2, 33, 256), (2, 20, 512)   rows                the other row-group counts
wide             (2, 65, 1024)  rows_act, no relu                 RG = 1, one column chunk; dbias is about 0: held on the absolute error
                                                                  against max |dbeta|, as tests/test_gpu_kernels.py holds it
chunks           (3, 17, 4096)  rows_act, relu                    four column chunks (gridDim.y)
odd_width        (3, 111, 100)  rows                              C/4 = 25 does not divide 256, C % 16 != 0 in the fold; 333 rows
odd_unfixed      (1, 7, 100)    rows                              bn_bwd_apply_kernel's per-element coefficients (stride no multiple of C/4)
unbiased         (2, 33, 128)   rows, biased_moving_variance=False   the other moving variance
bf16_logits      (2, 33, 128)   rows_fwd + bwd_x16 (C ABI)        x stored as bf16; the reference takes the bf16-rounded x in fp64
image_bf16/fp16  (2, 65, 128)   rows_act_image_fwd_fmt (relu) + act_bwd_image_fmt beside rows_act_fwd + act_bwd: the images are bit for bit
                                ops._split_rows of the fp32 entry points' results ([hi | lo | hi] / [hi | hi | lo]; fp16 through an
                                ops.OperandSite), mean, var, dgamma, dbeta, dbias and the recorded amax bitwise the plain form's
image_nobias     (2, 65, 128)   the bn_dense_x3 use: rows_act_image_fwd_fmt with a zero bias and no relu, then lpm_bn_bwd
small_MxC_actA   (2, 33), (7, 40), (250, 96), (256, 64), (80, 512) x act 0, 1, 2   ops._BNSmall: 8 row groups x 32 rows, C % 32 != 0, M at the
                                limit; parts y, dx, dgamma, dbeta, dmul, batch_mean, the moving statistics (unbiased)
fold_alone       nblk in {1, 63, 2047, 2048, 2100}, C = 12   ops.bn_fold on synthetic partials against the same partials folded in fp64
Regimes (tests/_bn_ref.make_inputs): offset3 / offset10 / offset30 (mean / std about R in every column), mixed_offset (every other column at
30), column_spread (std over four decades, variance down to 1e-4 << eps) on one_block_plus, two_blocks, wide, odd_width and small_250x96_act1;
dead_relu (dead and nearly dead ReLU columns) on one_block_plus and two_blocks.  Three seeds each.

Seeds: SEEDS below, the condition values of tests/_bn_ref.conditions beside each.

MEASURED-BEGIN
Measured on the MI355X, worst error / bound over parts and seeds (the part that gives it in brackets).  "before": csrc/bn.hip before this
file existed -- bn_fold_kernel formed var = q/n - mu^2 from the raw fp32 sums of x and x^2 alone, and the backward centred with the fp32
``mean`` as it is.  "after": today's kernels -- the rows statistics pass also sums (x - K) and (x - K)^2 with K the mean of the first eight
rows, the fold takes the raw sums where mean^2 <= var and the shifted ones elsewhere; the backward takes mean_r(x - mean), the part of the
mean that fp32 lost, off its centred values in the columns with mean^2 > var.  bn_small is two-pass and unchanged.
Before: 19 of the 63 tests fail -- every regime but dead_relu on the four rows cases, except odd_width column_spread (no bias: no column
with |mean| >> std there; in the bias forms the columns with std 0.01 sit at |mean|/std = 30 .. 70 behind the bias).  A failing test ends at
its first seed, so the "before" figures of those rows are that seed's alone.
case (regime)                     before                            after
few_rows                          0.16 (y)                          0.15 (dx)
few_rows_act                      0.30 (y)                          0.21 (dx)
one_block_plus                    0.23 (batch_var)                  0.23 (batch_var)
two_blocks                        0.21 (dbias)                      0.21 (dbias)
rg4                               0.13 (moving_var)                 0.14 (dx)
rg2                               0.12 (dx)                         0.12 (dx)
wide                              0.39 (y)                          0.24 (dgamma)
chunks                            0.50 (batch_var)                  0.33 (batch_var)
odd_width                         0.20 (dx)                         0.20 (dx)
odd_unfixed                       0.28 (y)                          0.26 (dx)
unbiased                          0.13 (batch_var)                  0.13 (batch_var)
bf16_logits                       0.13 (dx)                         0.13 (dx)
image_bf16                        0.21 (dbias)                      0.21 (dbias)
image_fp16                        0.21 (dbias)                      0.21 (dbias)
image_nobias                      0.14 (y)                          0.12 (moving_var)
small_2x33_act0                   0.16 (dgamma)                     0.16 (dgamma)
small_2x33_act1                   0.12 (dx)                         0.12 (dx)
small_2x33_act2                   0.16 (dgamma)                     0.16 (dgamma)
small_7x40_act0                   0.12 (moving_mean)                0.12 (moving_mean)
small_7x40_act1                   0.21 (dx)                         0.21 (dx)
small_7x40_act2                   0.16 (dmul)                       0.16 (dmul)
small_250x96_act0                 0.12 (moving_var)                 0.12 (moving_var)
small_250x96_act1                 0.12 (moving_var)                 0.12 (moving_var)
small_250x96_act2                 0.17 (dx)                         0.17 (dx)
small_256x64_act0                 0.12 (dx)                         0.12 (dx)
small_256x64_act1                 0.12 (moving_var)                 0.12 (moving_var)
small_256x64_act2                 0.15 (dgamma)                     0.15 (dgamma)
small_80x512_act0                 0.15 (dx)                         0.15 (dx)
small_80x512_act1                 0.14 (dgamma)                     0.14 (dgamma)
small_80x512_act2                 0.12 (moving_var)                 0.12 (moving_var)
one_block_plus (offset3)          1.64 (batch_var)  FAILS 0.16 (moving_var)
one_block_plus (offset10)         4.12 (batch_var)  FAILS 0.18 (dbias)
one_block_plus (offset30)         30.37 (moving_var)  FAILS 0.13 (dbias)
one_block_plus (mixed_offset)     31.36 (batch_var)  FAILS 0.26 (dbias)
one_block_plus (column_spread)    5.92 (dx)  FAILS     0.22 (batch_var)
one_block_plus (dead_relu)        0.29 (batch_var)                  0.29 (batch_var)
two_blocks (offset3)              1.02 (batch_var)  FAILS 0.25 (dx)
two_blocks (offset10)             3.75 (batch_var)  FAILS 0.15 (batch_var)
two_blocks (offset30)             25.18 (batch_var)  FAILS 0.13 (batch_var)
two_blocks (mixed_offset)         25.18 (batch_var)  FAILS 0.21 (dbias)
two_blocks (column_spread)        1.06 (dx)  FAILS                  0.27 (dbias)
two_blocks (dead_relu)            0.74 (dx)                         0.74 (dx)
wide (offset3)                    2.13 (batch_var)  FAILS 0.26 (dbeta)
wide (offset10)                   17.41 (batch_var)  FAILS 0.24 (dbeta)
wide (offset30)                   67.26 (moving_var)  FAILS 0.24 (dbeta)
wide (mixed_offset)               54.59 (moving_var)  FAILS 0.24 (dbeta)
wide (column_spread)              9.92 (dx)  FAILS     0.24 (dbeta)
odd_width (offset3)               1.49 (batch_var)  FAILS 0.23 (dgamma)
odd_width (offset10)              18.93 (moving_var)  FAILS 0.21 (moving_var)
odd_width (offset30)              219.80 (moving_var)  FAILS 0.16 (dbeta)
odd_width (mixed_offset)          82.21 (moving_var)  FAILS 0.16 (dbeta)
odd_width (column_spread)         0.22 (dx)                         0.22 (dx)
small_250x96_act1 (offset3)       0.21 (dx)                         0.21 (dx)
small_250x96_act1 (offset10)      0.16 (moving_mean)                0.16 (moving_mean)
small_250x96_act1 (offset30)      0.15 (moving_var)                 0.15 (moving_var)
small_250x96_act1 (mixed_offset)  0.15 (moving_var)                 0.15 (moving_var)
small_250x96_act1 (column_spread) 0.13 (moving_var)                 0.13 (moving_var)
The op's error as a multiple of err32 over the four rows cases and their seeds, before -> after:
y offset3 : 4.3 .. 6.4 -> after 0.6 .. 0.9
y offset10 : 11.8 .. 38.8 -> after 0.4 .. 0.8
y offset30 : 37.3 .. 125.9 -> after 0.4 .. 0.7
batch_var offset3 : 8.2 .. 17.1 -> after 0.7 .. 1.9
batch_var offset10 : 30.0 .. 139.2 -> after 0.6 .. 1.7
batch_var offset30 : 201.5 .. 2334.3 -> after 0.7 .. 1.3
dx offset3 : 4.6 .. 8.7 -> after 0.5 .. 2.0
dx offset10 : 16.2 .. 45.6 -> after 0.2 .. 0.6
dx offset30 : 46.6 .. 149.3 -> after 0.1 .. 0.9
Before, batch_var shows the defect first (1.02 .. 2.1 of its bound already at mean/std = 3), then dx, then y.  With the forward alone fixed
every part met its bound except dbias of the columns no ReLU clips at mean/std = 30 (one_block_plus, wide: 1.06 .. 1.09; two_blocks 0.77 ..
0.94): the fp32 rounding of the saved mean, eps32/2 |mean| = 1e-6 std, leaves the centred values with a non-zero column sum, which the
backward's correction removes (0.13 .. 0.26 after).  A first version with row 0 alone as the pivot, as the layer norms have it, was
emulated on the CPU before any GPU run: batch_var at 0.9 .. 1.3 of its bound at mean/std = 3 -- among 1024 columns some first rows lie 4 std
off the mean -- against 0.09 .. 0.43 with eight rows.
The whole file: 63 tests, 3.4 s (--durations: 0.39 s the first test, which loads the library; 0.12 s or less each other).
MEASURED-END"""
import functools
import math

import pytest
import torch

from tests import _bn_ref as R
from tests._netvlad_ref import DECAY, ONE_MINUS_DECAY
from tests._util import cuda

pytestmark = pytest.mark.gpu

PREFIX = "lpm_bn_"
ROWS = ("rows_fwd", "bwd")
ROWS_ACT = ("rows_act_fwd", "act_bwd")
SMALL = ("small_fwd", "small_bwd")
IMAGE = ROWS_ACT + ("rows_act_image_fwd", "act_bwd_image")


def _case(shape, form, route, **opts):
    return dict(shape=shape, form=form, route=tuple(route), opts=opts)


SMALL_SHAPES = {(2, 33): (2, 1), (7, 40): (7, 1), (250, 96): (5, 50), (256, 64): (4, 64), (80, 512): (4, 20)}      # (M, C) -> (B, L)

CASES = {
    "few_rows": _case((1, 7, 128), "rows", ROWS),
    "few_rows_act": _case((1, 7, 128), "rows_act", ROWS_ACT, relu=True),
    "one_block_plus": _case((2, 33, 128), "rows_act", ROWS_ACT, relu=True),
    "two_blocks": _case((2, 65, 128), "rows_act", ROWS_ACT, relu=True),
    "rg4": _case((2, 33, 256), "rows", ROWS),
    "rg2": _case((2, 20, 512), "rows", ROWS),
    "wide": _case((2, 65, 1024), "rows_act", ROWS_ACT, relu=False),
    "chunks": _case((3, 17, 4096), "rows_act", ROWS_ACT, relu=True),
    "odd_width": _case((3, 111, 100), "rows", ROWS),
    "odd_unfixed": _case((1, 7, 100), "rows", ROWS),
    "unbiased": _case((2, 33, 128), "rows", ROWS, biased=False),
    "bf16_logits": _case((2, 33, 128), "bf16_logits", ("rows_fwd", "bwd_x16")),
    "image_bf16": _case((2, 65, 128), "image", IMAGE, relu=True, f16=False),
    "image_fp16": _case((2, 65, 128), "image", IMAGE, relu=True, f16=True),
    "image_nobias": _case((2, 65, 128), "image_nobias", ("rows_act_fwd", "rows_act_image_fwd", "bwd")),
}
for (_M, _C), (_B, _L) in SMALL_SHAPES.items():
    for _act in (0, 1, 2):
        CASES[f"small_{_M}x{_C}_act{_act}"] = _case((_B, _L, _C), "small", SMALL, act=_act, biased=False)

REGIME_CASES = ("one_block_plus", "two_blocks", "wide", "odd_width", "small_250x96_act1")
RELU_CASES = ("one_block_plus", "two_blocks")
REGIME_PARAMS = [(n, r) for n in REGIME_CASES for r in R.REGIMES[1:] if r != "dead_relu" or n in RELU_CASES]

# per case (or (case, regime)): the seeds, and beside them the condition values of tests/_bn_ref.conditions per seed -- min and max over the
# columns of |mean| / std, the least column variance, the least maximum of a part (per example and per live column), and for act 1 the
# least distance of any fp64 z from 0 and 6 (tests/test_bn_ref_host.py proves every entry)
SEEDS = {
    # SEEDS-BEGIN
    "few_rows": (0,),                                     # 3.3e-04, 2.2e+00, 5.0e-02, 1.4e-03, inf
    "few_rows_act": (0,),                                 # 4.1e-01, 2.5e+00, 0.0e+00, 1.6e-03, inf
    "one_block_plus": (0,),                               # 2.5e-01, 1.7e+00, 1.6e-02, 1.5e-03, inf
    "two_blocks": (0,),                                   # 2.1e-01, 1.8e+00, 6.3e-03, 1.2e-03, inf
    "rg4": (0,),                                          # 3.9e-04, 1.4e+00, 2.2e-01, 9.6e-04, inf
    "rg2": (0,),                                          # 2.9e-03, 1.7e+00, 1.6e-01, 1.1e-03, inf
    "wide": (0,),                                         # 8.3e-04, 2.8e+00, 2.0e-01, 1.9e-11, inf
    "chunks": (0,),                                       # 1.4e-01, 2.8e+00, 0.0e+00, 2.1e-03, inf
    "odd_width": (0,),                                    # 2.3e-03, 1.3e+00, 2.3e-01, 8.3e-04, inf
    "odd_unfixed": (0,),                                  # 7.4e-03, 2.3e+00, 1.1e-01, 1.5e-03, inf
    "unbiased": (0,),                                     # 7.4e-03, 1.1e+00, 2.2e-01, 8.6e-04, inf
    "bf16_logits": (0,),                                  # 7.0e-03, 1.1e+00, 2.2e-01, 8.6e-04, inf
    "image_bf16": (0,),                                   # 2.1e-01, 1.8e+00, 6.3e-03, 1.2e-03, inf
    "image_fp16": (0,),                                   # 2.1e-01, 1.8e+00, 6.3e-03, 1.2e-03, inf
    "image_nobias": (0,),                                 # 1.5e-03, 1.1e+00, 2.5e-01, 8.9e-04, inf
    "small_2x33_act0": (0,),                              # 3.4e-02, 1.9e+01, 3.9e-04, 2.2e-03, inf
    "small_2x33_act1": (23,),                             # 2.6e-02, 1.4e+02, 7.9e-06, 6.8e-08, 9.0e-02
    "small_2x33_act2": (0,),                              # 3.4e-02, 1.9e+01, 3.9e-04, 1.3e-03, inf
    "small_7x40_act0": (0,),                              # 6.0e-02, 2.5e+00, 8.2e-02, 1.1e-03, inf
    "small_7x40_act1": (0,),                              # 6.0e-02, 2.5e+00, 8.2e-02, 1.1e-03, 2.0e-02
    "small_7x40_act2": (0,),                              # 6.0e-02, 2.5e+00, 8.2e-02, 1.1e-03, inf
    "small_250x96_act0": (0,),                            # 2.2e-03, 1.1e+00, 2.5e-01, 9.4e-04, inf
    "small_250x96_act1": (0,),                            # 2.2e-03, 1.1e+00, 2.5e-01, 9.4e-04, 5.2e-05
    "small_250x96_act2": (0,),                            # 2.2e-03, 1.1e+00, 2.5e-01, 9.4e-04, inf
    "small_256x64_act0": (0,),                            # 1.9e-03, 7.9e-01, 3.0e-01, 9.1e-04, inf
    "small_256x64_act1": (1,),                            # 8.7e-03, 1.3e+00, 2.7e-01, 9.2e-04, 4.0e-05
    "small_256x64_act2": (0,),                            # 1.9e-03, 7.9e-01, 3.0e-01, 9.1e-04, inf
    "small_80x512_act0": (0,),                            # 1.5e-03, 1.6e+00, 1.8e-01, 1.2e-03, inf
    "small_80x512_act1": (0,),                            # 1.5e-03, 1.6e+00, 1.8e-01, 1.2e-03, 4.0e-05
    "small_80x512_act2": (0,),                            # 1.5e-03, 1.6e+00, 1.8e-01, 1.2e-03, inf
    ("one_block_plus", "offset3"): (1, 2, 5),            # 2.0e+00, 4.4e+00, 2.0e-01, 2.9e-03, inf; 2.2e+00, 4.1e+00, 2.3e-01, 2.8e-03, inf; 1.8e+00, 4.3e+00, 2.1e-01, 2.9e-03, inf
    ("one_block_plus", "offset10"): (1, 2, 3),           # 7.6e+00, 1.3e+01, 2.0e-01, 4.5e-12, inf; 8.1e+00, 1.3e+01, 2.3e-01, 6.4e-12, inf; 7.6e+00, 1.3e+01, 2.6e-01, 8.2e-12, inf
    ("one_block_plus", "offset30"): (1, 2, 3),           # 2.4e+01, 4.0e+01, 2.0e-01, 5.5e-12, inf; 2.5e+01, 3.8e+01, 2.3e-01, 5.2e-12, inf; 2.4e+01, 3.9e+01, 2.6e-01, 6.4e-12, inf
    ("one_block_plus", "mixed_offset"): (1, 2, 3),       # 2.4e-01, 4.0e+01, 1.7e-02, 2.5e-03, inf; 3.6e-01, 3.8e+01, 4.3e-02, 2.8e-03, inf; 3.9e-01, 3.9e+01, 2.8e-02, 2.5e-03, inf
    ("one_block_plus", "column_spread"): (0, 1, 2),      # 1.5e-01, 4.8e+01, 0.0e+00, 1.7e-02, inf; 1.2e-01, 6.5e+01, 0.0e+00, 2.3e-04, inf; 1.2e-01, 4.9e+01, 0.0e+00, 6.4e-03, inf
    ("one_block_plus", "dead_relu"): (0, 1, 2),          # 1.2e-01, 1.7e+00, 0.0e+00, 1.3e-03, inf; 1.2e-01, 1.7e+00, 0.0e+00, 1.0e-03, inf; 1.2e-01, 1.5e+00, 0.0e+00, 1.3e-03, inf
    ("two_blocks", "offset3"): (0, 1, 3),                # 2.1e+00, 4.2e+00, 2.5e-01, 2.5e-03, inf; 2.1e+00, 4.1e+00, 2.3e-01, 2.6e-03, inf; 2.1e+00, 4.4e+00, 1.8e-01, 2.7e-03, inf
    ("two_blocks", "offset10"): (0, 1, 2),               # 8.3e+00, 1.3e+01, 2.5e-01, 9.1e-12, inf; 8.6e+00, 1.2e+01, 2.3e-01, 1.2e-11, inf; 7.7e+00, 1.2e+01, 2.8e-01, 1.2e-11, inf
    ("two_blocks", "offset30"): (0, 1, 2),               # 2.5e+01, 3.8e+01, 2.5e-01, 7.5e-12, inf; 2.6e+01, 3.4e+01, 2.3e-01, 7.7e-12, inf; 2.5e+01, 3.5e+01, 2.8e-01, 7.3e-12, inf
    ("two_blocks", "mixed_offset"): (0, 1, 2),           # 2.2e-01, 3.8e+01, 6.3e-03, 2.5e-03, inf; 2.7e-01, 3.4e+01, 1.9e-02, 2.6e-03, inf; 2.1e-01, 3.4e+01, 1.9e-02, 2.3e-03, inf
    ("two_blocks", "column_spread"): (0, 1, 2),          # 8.8e-02, 4.7e+01, 0.0e+00, 9.2e-03, inf; 9.3e-02, 1.4e+01, 0.0e+00, 3.6e-03, inf; 1.2e-01, 3.1e+01, 0.0e+00, 1.2e-02, inf
    ("two_blocks", "dead_relu"): (0, 1, 2),              # 8.8e-02, 1.3e+00, 0.0e+00, 1.2e-03, inf; 8.8e-02, 1.4e+00, 0.0e+00, 1.2e-03, inf; 8.8e-02, 1.9e+00, 0.0e+00, 1.0e-03, inf
    ("wide", "offset3"): (1, 15, 20),                    # 1.8e+00, 4.3e+00, 1.8e-01, 1.3e-11, inf; 1.9e+00, 4.4e+00, 1.9e-01, 1.1e-11, inf; 1.5e+00, 4.4e+00, 1.9e-01, 1.9e-11, inf
    ("wide", "offset10"): (0, 1, 2),                     # 7.9e+00, 1.3e+01, 2.0e-01, 1.2e-11, inf; 8.1e+00, 1.3e+01, 1.8e-01, 1.4e-11, inf; 7.8e+00, 1.2e+01, 2.0e-01, 1.0e-11, inf
    ("wide", "offset30"): (0, 1, 2),                     # 2.5e+01, 3.7e+01, 2.0e-01, 1.8e-11, inf; 2.5e+01, 3.7e+01, 1.8e-01, 1.2e-11, inf; 2.5e+01, 3.7e+01, 2.0e-01, 1.8e-11, inf
    ("wide", "mixed_offset"): (0, 1, 2),                 # 1.6e-03, 3.7e+01, 2.0e-01, 1.9e-11, inf; 3.0e-04, 3.6e+01, 1.8e-01, 1.3e-11, inf; 4.3e-04, 3.7e+01, 2.0e-01, 1.8e-11, inf
    ("wide", "column_spread"): (0, 1, 2),                # 4.6e-04, 5.7e+01, 8.9e-05, 2.3e-10, inf; 2.6e-04, 5.7e+01, 8.8e-05, 1.4e-10, inf; 1.4e-03, 6.9e+01, 8.9e-05, 1.7e-10, inf
    ("odd_width", "offset3"): (0, 1, 2),                 # 2.6e+00, 3.4e+00, 2.3e-01, 2.5e-03, inf; 2.6e+00, 3.4e+00, 2.4e-01, 2.6e-03, inf; 2.7e+00, 3.3e+00, 2.5e-01, 2.2e-03, inf
    ("odd_width", "offset10"): (0, 1, 2),                # 8.9e+00, 1.1e+01, 2.3e-01, 2.5e-03, inf; 8.9e+00, 1.1e+01, 2.4e-01, 2.6e-03, inf; 9.2e+00, 1.1e+01, 2.5e-01, 2.2e-03, inf
    ("odd_width", "offset30"): (0, 1, 2),                # 2.7e+01, 3.3e+01, 2.3e-01, 2.5e-03, inf; 2.7e+01, 3.3e+01, 2.4e-01, 2.6e-03, inf; 2.8e+01, 3.4e+01, 2.5e-01, 2.2e-03, inf
    ("odd_width", "mixed_offset"): (0, 1, 2),            # 2.3e-03, 3.2e+01, 2.3e-01, 2.5e-03, inf; 7.6e-03, 3.3e+01, 2.4e-01, 2.6e-03, inf; 2.7e-03, 3.4e+01, 2.5e-01, 2.2e-03, inf
    ("odd_width", "column_spread"): (0, 1, 2),           # 3.7e-04, 7.9e-01, 1.1e-04, 5.5e-02, inf; 1.2e-03, 8.4e-01, 1.1e-04, 3.8e-02, inf; 2.7e-03, 7.8e-01, 1.1e-04, 4.7e-02, inf
    ("small_250x96_act1", "offset3"): (0, 1, 3),         # 2.6e+00, 3.5e+00, 2.5e-01, 2.5e-03, 5.2e-05; 2.7e+00, 3.5e+00, 2.7e-01, 2.7e-03, 7.8e-05; 2.7e+00, 3.6e+00, 2.5e-01, 2.6e-03, 2.4e-05
    ("small_250x96_act1", "offset10"): (0, 1, 3),        # 8.8e+00, 1.2e+01, 2.5e-01, 2.5e-03, 5.2e-05; 8.9e+00, 1.2e+01, 2.7e-01, 2.7e-03, 7.8e-05; 9.0e+00, 1.2e+01, 2.5e-01, 2.6e-03, 2.3e-05
    ("small_250x96_act1", "offset30"): (0, 1, 3),        # 2.7e+01, 3.5e+01, 2.5e-01, 2.5e-03, 5.0e-05; 2.7e+01, 3.4e+01, 2.7e-01, 2.7e-03, 7.6e-05; 2.7e+01, 3.5e+01, 2.5e-01, 2.6e-03, 2.4e-05
    ("small_250x96_act1", "mixed_offset"): (0, 1, 3),    # 4.4e-03, 3.5e+01, 2.5e-01, 2.5e-03, 5.0e-05; 1.2e-03, 3.3e+01, 2.7e-01, 2.7e-03, 7.8e-05; 3.7e-03, 3.5e+01, 2.5e-01, 2.6e-03, 2.4e-05
    ("small_250x96_act1", "column_spread"): (0, 1, 2),   # 2.3e-03, 1.0e+00, 1.1e-04, 4.8e-02, 2.3e-05; 1.1e-02, 7.1e-01, 1.1e-04, 2.9e-02, 2.4e-05; 2.5e-03, 7.8e-01, 9.9e-05, 3.6e-02, 3.9e-05
    # SEEDS-END
}


def seeds_of(name, regime="random"):
    return SEEDS[name if regime == "random" else (name, regime)]


def ref_kwargs(name):
    """How tests/_bn_ref.bn_ref is asked for the case."""
    case = CASES[name]
    form, opts = case["form"], case["opts"]
    return dict(bias=form in ("rows_act", "image"), relu=bool(opts.get("relu")), act=opts.get("act", 0),
                biased_moving_variance=opts.get("biased", True))


@functools.lru_cache(maxsize=None)
def reference(name, seed, regime="random"):
    """-> (inputs, fp64 parts, fp32 parts, (ok, condition values)), computed once per (case, seed, regime) on the CPU."""
    case = CASES[name]
    inputs = R.make_inputs(*case["shape"], seed, regime)
    if case["form"] == "bf16_logits":
        inputs = dict(inputs, x=inputs["x"].bfloat16().float())          # what the kernel reads, exactly
    kw = ref_kwargs(name)
    p64, p32 = R.bn_ref(inputs, torch.float64, **kw), R.bn_ref(inputs, torch.float32, **kw)
    cond = R.conditions(inputs, p64, regime, bias=kw["bias"], relu=kw["relu"], act=kw["act"])
    return inputs, p64, p32, cond


def part_names(name):
    """The parts the case is held on."""
    kw = ref_kwargs(name)
    names = ["y", "dx", "dgamma", "dbeta", "batch_mean", "moving_mean", "moving_var"]
    if CASES[name]["form"] != "small":
        names.append("batch_var")
    if kw["bias"]:
        names.append("dbias")
    if kw["act"] == 2:
        names.append("dmul")
    return names


def floor_of(name, part, inputs, p64):
    """A bias whose ReLU clips nothing (wide: no ReLU; the ReLU forms in the offset regimes): the batch norm removes any per-column
    constant, dbias is zero but for rounding -- held on the absolute error against the scale of the gradients that are not, max |dbeta|."""
    kw = ref_kwargs(name)
    if part == "dbias" and kw["bias"] and (not kw["relu"] or bool((inputs["x"].double() + inputs["bias"].double() > 0).all())):
        return float(p64["dbeta"].abs().max())
    return None


def bounds(name, seed, regime="random"):
    """-> {part: (err32, bound)}"""
    inputs, p64, p32, _ = reference(name, seed, regime)
    B = CASES[name]["shape"][0]
    out = {}
    for n in part_names(name):
        e = R.figure(p32[n], p64[n], n, B, floor_of(name, n, inputs, p64))
        out[n] = (e, max(8 * e, 1e-6))
    return out


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


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b)), f"{what}: not bit for bit the plain form's"


def _amax(dev):
    from learnablepoolingmethods_amd import _capi
    return torch.zeros(_capi.LPM_OPERAND_AMAX_SUB * _capi.LPM_OPERAND_AMAX_STRIDE, device=dev)


def _moving(C, dev):
    return torch.zeros(C, device=dev), torch.zeros(C, device=dev)


def _run_rows(name, inputs, dev):
    from learnablepoolingmethods_amd import ops
    case = CASES[name]
    B, L, C = case["shape"]
    biased = case["opts"].get("biased", True)
    x, gamma, beta, dy = (inputs[k].to(dev) for k in ("x", "gamma", "beta", "upstream"))
    mm, mv = _moving(C, dev)
    ctx = ops._SubCtx()
    if case["form"] == "rows":
        y = ops._BatchNormRows.forward(ctx, x, gamma, beta, mm, mv, biased)
        mean, var = ctx.saved_tensors[1:3]
        dx, dgamma, dbeta = ops._BatchNormRows.backward(ctx, dy)[:3]
        extra = {}
    else:
        bias = inputs["bias"].to(dev)
        y = ops._BatchNormRowsAct.forward(ctx, x, bias, case["opts"]["relu"], gamma, beta, mm, mv, biased)
        mean, var = ctx.saved_tensors[2:4]
        res = ops._BatchNormRowsAct.backward(ctx, dy)
        dx, dgamma, dbeta, extra = res[0], res[3], res[4], dict(dbias=res[1])
    return dict(y=y, dx=dx, dgamma=dgamma, dbeta=dbeta, batch_mean=mean, batch_var=var, moving_mean=mm, moving_var=mv, **extra)


def _run_bf16_logits(name, inputs, dev):
    """The forward on the bf16-rounded x as fp32, the backward reading the SAME numbers stored as bf16 (lpm_bn_bwd_x16, as the bf16-storage
    configuration's attention hands its logits over)."""
    from learnablepoolingmethods_amd import _capi, ops
    lib = _capi.load()
    B, L, C = CASES[name]["shape"]
    M = B * L
    x, gamma, beta, dy = (inputs[k].to(dev) for k in ("x", "gamma", "beta", "upstream"))
    x16 = x.bfloat16().contiguous()
    assert torch.equal(x16.float(), x)
    mm, mv = _moving(C, dev)
    ctx = ops._SubCtx()
    y = ops._BatchNormRows.forward(ctx, x, gamma, beta, mm, mv, True)
    mean, var = ctx.saved_tensors[1:3]
    dx = torch.empty(M, C, device=dev)
    dgamma, dbeta = torch.empty(C, device=dev), torch.empty(C, device=dev)
    wsb = lib._lpm_bn_bwd_workspace_bytes(M, C)
    ws = torch.empty(wsb // 4, device=dev)
    lib.check(lib._lpm_bn_bwd_x16(ops.ptr(dy.contiguous()), ops.ptr(x16), ops.ptr(mean), ops.ptr(var), ops.ptr(gamma), R.BN_EPS, M, C, ops.ptr(dx),
                                  ops.ptr(dgamma), ops.ptr(dbeta), ops.ptr(ws), wsb, ops.stream_ptr()), "lpm_bn_bwd_x16")
    return dict(y=y, dx=dx, dgamma=dgamma, dbeta=dbeta, batch_mean=mean, batch_var=var, moving_mean=mm, moving_var=mv)


def _image_fwd(lib, ops, x2, bias, relu, gamma, beta, site, dev):
    """lpm_bn_rows_act_image_fwd_fmt -> (image, mean, var, moving_mean, moving_var)"""
    M, C = x2.shape
    img = torch.empty((M, 3 * C), dtype=site.dtype, device=dev)
    mean, var = torch.empty(C, device=dev), torch.empty(C, device=dev)
    mm, mv = _moving(C, dev)
    wsb = lib._lpm_bn_rows_workspace_bytes(M, C)
    ws = torch.empty(wsb // 4, device=dev)
    lib.check(lib._lpm_bn_rows_act_image_fwd_fmt(ops.ptr(x2), ops.ptr(bias), 1 if relu else 0, M, C, ops.ptr(gamma), ops.ptr(beta), R.BN_EPS, DECAY,
                                                 1, ops.ptr(img), ops.ptr(mean), ops.ptr(var), ops.ptr(mm), ops.ptr(mv), ops.ptr(ws), wsb, site.fmt,
                                                 ops.stream_ptr()), "lpm_bn_rows_act_image_fwd")
    return img, mean, var, mm, mv


def _assert_activation_image(ops, img, y2, site, amax, f16, dev, tag):
    """img is ops._split_rows(y2) in the site's format, the amax it recorded that pass's; bf16: the planes are [hi | lo | hi], hi = bf16(y)."""
    C = y2.shape[1]
    amax_ref = _amax(dev)
    want = ops._split_rows(y2, site=ops.OperandSite(f16, site.scale, amax_ref.data_ptr(), role="a"))
    _same_bits(img, want, f"{tag} activation image")
    assert float(amax.max()) == float(amax_ref.max()) == float(y2.abs().max()), f"{tag}: recorded amax {float(amax.max())}"
    if not f16:
        _same_bits(img[:, :C], y2.bfloat16(), f"{tag} hi plane")
        _same_bits(img[:, 2 * C:], img[:, :C], f"{tag} third plane")
        _same_bits(img[:, C:2 * C], (y2 - y2.bfloat16().float()).bfloat16(), f"{tag} lo plane")


def _run_image(name, inputs, dev):
    """The plain pair (parts under the rule) and the image pair on the same inputs: everything the image forms return is bitwise the plain
    form's, the images bit for bit ops._split_rows of the plain y and dx."""
    from learnablepoolingmethods_amd import _capi, ops
    lib = _capi.load()
    f16 = CASES[name]["opts"]["f16"]
    got = _run_rows(name, inputs, dev)
    B, L, C = CASES[name]["shape"]
    M = B * L
    x2, dy2 = inputs["x"].to(dev).reshape(M, C), inputs["upstream"].to(dev).reshape(M, C)
    bias, gamma, beta = (inputs[k].to(dev) for k in ("bias", "gamma", "beta"))
    amax_a, amax_g = _amax(dev), _amax(dev)
    site_a = ops.OperandSite(f16, 2.0 ** 7, amax_a.data_ptr(), role="a")
    site_g = ops.OperandSite(f16, 1.0, amax_g.data_ptr(), role="g")
    img, mean, var, mm, mv = _image_fwd(lib, ops, x2, bias, True, gamma, beta, site_a, dev)
    for n, t in (("batch_mean", mean), ("batch_var", var), ("moving_mean", mm), ("moving_var", mv)):
        _same_bits(t, got[n], f"{name} {n}")
    _assert_activation_image(ops, img, got["y"].reshape(M, C), site_a, amax_a, f16, dev, name)
    dimg = torch.empty((M, site_g.planes * C), dtype=site_g.dtype, device=dev)
    dgamma, dbeta, dbias = (torch.empty(C, device=dev) for _ in range(3))
    wsb = lib._lpm_bn_act_bwd_workspace_bytes(M, C)
    ws = torch.empty(wsb // 4, device=dev)
    lib.check(lib._lpm_bn_act_bwd_image_fmt(ops.ptr(dy2), ops.ptr(x2), ops.ptr(bias), 1, ops.ptr(mean), ops.ptr(var), ops.ptr(gamma), R.BN_EPS, M, C,
                                            ops.ptr(dimg), ops.ptr(dgamma), ops.ptr(dbeta), ops.ptr(dbias), ops.ptr(ws), wsb, site_g.fmt,
                                            ops.stream_ptr()), "lpm_bn_act_bwd_image")
    for n, t in (("dgamma", dgamma), ("dbeta", dbeta), ("dbias", dbias)):
        _same_bits(t, got[n], f"{name} {n}")
    dx2 = got["dx"].reshape(M, C)
    amax_ref = _amax(dev)
    want = ops._split_rows(dx2, grad=True, site=ops.OperandSite(f16, site_g.scale, amax_ref.data_ptr(), role="g"))
    _same_bits(dimg, want, f"{name} gradient image")
    assert float(amax_g.max()) == float(amax_ref.max()) == float(dx2.abs().max()), f"{name}: recorded gradient amax {float(amax_g.max())}"
    if not f16:
        _same_bits(dimg[:, :C], dx2.bfloat16(), f"{name} gradient hi plane")
        _same_bits(dimg[:, C:2 * C], dimg[:, :C], f"{name} gradient second plane")
        _same_bits(dimg[:, 2 * C:], (dx2 - dx2.bfloat16().float()).bfloat16(), f"{name} gradient lo plane")
    return got


def _run_image_nobias(name, inputs, dev):
    """ops._BNDenseX3's calls without its GEMMs: the image forward with a zero bias and no ReLU, lpm_bn_bwd behind it."""
    from learnablepoolingmethods_amd import _capi, ops
    lib = _capi.load()
    B, L, C = CASES[name]["shape"]
    M = B * L
    x2, dy2 = inputs["x"].to(dev).reshape(M, C), inputs["upstream"].to(dev).reshape(M, C)
    gamma, beta = inputs["gamma"].to(dev), inputs["beta"].to(dev)
    zero = torch.zeros(C, device=dev)
    y = torch.empty(M, C, device=dev)
    mean0, var0 = torch.empty(C, device=dev), torch.empty(C, device=dev)
    mm0, mv0 = _moving(C, dev)
    wsb = lib._lpm_bn_rows_workspace_bytes(M, C)
    ws = torch.empty(wsb // 4, device=dev)
    lib.check(lib._lpm_bn_rows_act_fwd(ops.ptr(x2), ops.ptr(zero), 0, M, C, ops.ptr(gamma), ops.ptr(beta), R.BN_EPS, DECAY, 1, ops.ptr(y),
                                       ops.ptr(mean0), ops.ptr(var0), ops.ptr(mm0), ops.ptr(mv0), ops.ptr(ws), wsb, ops.stream_ptr()),
              "lpm_bn_rows_act_fwd")
    amax = _amax(dev)
    site = ops.OperandSite(False, 1.0, amax.data_ptr(), role="a")
    img, mean, var, mm, mv = _image_fwd(lib, ops, x2, zero, False, gamma, beta, site, dev)
    for n, t, t0 in (("batch_mean", mean, mean0), ("batch_var", var, var0), ("moving_mean", mm, mm0), ("moving_var", mv, mv0)):
        _same_bits(t, t0, f"{name} {n}")
    _assert_activation_image(ops, img, y, site, amax, False, dev, name)
    dx = torch.empty(M, C, device=dev)
    dgamma, dbeta = torch.empty(C, device=dev), torch.empty(C, device=dev)
    wsb2 = lib._lpm_bn_bwd_workspace_bytes(M, C)
    ws2 = torch.empty(wsb2 // 4, device=dev)
    lib.check(lib._lpm_bn_bwd(ops.ptr(dy2), ops.ptr(x2), ops.ptr(mean), ops.ptr(var), ops.ptr(gamma), R.BN_EPS, M, C, ops.ptr(dx), ops.ptr(dgamma),
                              ops.ptr(dbeta), ops.ptr(ws2), wsb2, ops.stream_ptr()), "lpm_bn_bwd")
    return dict(y=y, dx=dx, dgamma=dgamma, dbeta=dbeta, batch_mean=mean, batch_var=var, moving_mean=mm, moving_var=mv)


def _run_small(name, inputs, dev):
    from learnablepoolingmethods_amd import ops
    case = CASES[name]
    B, L, C = case["shape"]
    act = case["opts"]["act"]
    x, dy, mul = (inputs[k].to(dev).reshape(B * L, C) for k in ("x", "upstream", "mul"))
    gamma, beta = inputs["gamma"].to(dev), inputs["beta"].to(dev)
    assert ops.bn_small_ok(x, mul if act == 2 else None)
    mm, mv = _moving(C, dev)
    ctx = ops._SubCtx()
    y = ops._BNSmall.forward(ctx, x, gamma, beta, mm, mv, act, mul if act == 2 else None)
    mean = ctx.saved_tensors[3]
    res = ops._BNSmall.backward(ctx, dy)
    got = dict(y=y, dx=res[0], dgamma=res[1], dbeta=res[2], batch_mean=mean, moving_mean=mm, moving_var=mv)
    if act == 2:
        got["dmul"] = res[6]
    return got


RUNNERS = {"rows": _run_rows, "rows_act": _run_rows, "bf16_logits": _run_bf16_logits, "image": _run_image, "image_nobias": _run_image_nobias,
           "small": _run_small}


def run_op(name, inputs, dev):
    """The case's calls -> {part: tensor} under the restatement's names."""
    got = RUNNERS[CASES[name]["form"]](name, inputs, dev)
    torch.cuda.synchronize()
    return got


def check_parts(tag, got, name, seed, regime):
    """Figures, bounds and ratios of every part: printed, then asserted.  -> the worst ratio."""
    B = CASES[name]["shape"][0]
    inputs, p64, _, _ = reference(name, seed, regime)
    bnd = bounds(name, seed, regime)
    assert set(got) == set(bnd), f"{tag}: parts {sorted(got)} against {sorted(bnd)}"
    rows = []
    for n, (e32, bound) in bnd.items():
        floor = floor_of(name, n, inputs, p64)
        e_op = R.figure(got[n], p64[n], n, B, floor)
        zero = floor is None and float(p64[n].abs().max()) == 0.0
        exact = floor is not None or R.exactly_zero(got[n], p64[n], n, p64["batch_var"] == 0)
        rows.append((n, e_op, e32, bound, zero, exact))
        print(f"[bn] {tag} {n}: op {e_op:.3e}, err32 {e32:.3e}, bound {bound:.3e}, ratio {e_op / bound:.3f}, op/err32 {e_op / max(e32, 1e-300):.2f}"
              + ("" if exact else "  NOT exactly zero where fp64 is"))
    for n, e_op, e32, bound, zero, exact in rows:
        assert exact, f"{tag} {n}: identically zero in fp64 somewhere, not exactly zero in the op there"
        if zero:
            assert e_op == 0.0, f"{tag} {n}: identically zero in fp64, not exactly zero in the op"
        else:
            assert math.isfinite(e_op) and e_op <= bound, f"{tag} {n}: op error {e_op:.3e} > bound {bound:.3e} (err32 {e32:.3e})"
    if regime == "dead_relu":                  # the dead columns' y is beta itself
        C = inputs["x"].shape[-1]
        dead = R.dead_columns(C)
        y = got["y"].detach().cpu().reshape(-1, C)[:, dead]
        assert torch.equal(y, inputs["beta"][dead].expand_as(y)), f"{tag}: y of a dead column is not beta"
    worst = max((e_op / bound, n) for n, e_op, _, bound, zero, _ in rows if not zero)
    print(f"[bn] {tag} worst ratio {worst[0]:.3f} ({worst[1]})")
    return worst[0]


def check_case(name, seed, regime, dev, entries):
    inputs, _, _, (ok, cond) = reference(name, seed, regime)
    tag = f"{name} {regime} seed {seed}"
    print(f"[bn] {tag}: conditions {ok} " + ", ".join(f"{v:.2e}" for v in cond))
    assert ok, f"{tag}: the seed does not meet the conditions {cond}"
    del entries[:]
    got = run_op(name, inputs, dev)
    reached = sorted(e for e in entries if e.startswith(PREFIX))
    print(f"[bn] {tag} route: {reached}")
    worst = check_parts(tag, got, name, seed, regime)
    assert reached == sorted(PREFIX + n for n in CASES[name]["route"]), f"{tag}: reached {reached}"
    return worst


@pytest.mark.parametrize("name", list(CASES))
def test_op_meets_the_bound_on_every_route(name, entries):
    from learnablepoolingmethods_amd import ops
    assert ops.BN_EPS == R.BN_EPS and ops.BN_DECAY == pytest.approx(DECAY)
    dev = cuda()
    for seed in seeds_of(name):
        check_case(name, seed, "random", dev, entries)


@pytest.mark.parametrize("name,regime", REGIME_PARAMS)
def test_op_meets_the_bound_in_every_regime(name, regime, entries):
    dev = cuda()
    for seed in seeds_of(name, regime):
        check_case(name, seed, regime, dev, entries)


def test_moving_statistics_blend_with_the_decay():
    """unbiased, a second call: from (0.1, 1) the moving statistics are 0.999 (0.1, 1) + (1 - 0.999) (batch mean, unbiased batch variance).
    One fp32 blend of numbers of magnitude 0.1 and 1: 4 eps32 of the largest value (the batch statistics themselves are held from zero)."""
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    name, seed = "unbiased", seeds_of("unbiased")[0]
    B, L, C = CASES[name]["shape"]
    inputs, p64, _, _ = reference(name, seed)
    x, gamma, beta = (inputs[k].to(dev) for k in ("x", "gamma", "beta"))
    mm, mv = torch.full((C,), 0.1, device=dev), torch.ones(C, device=dev)
    ops._BatchNormRows.forward(ops._SubCtx(), x, gamma, beta, mm, mv, False)
    torch.cuda.synchronize()
    want_m = DECAY * float(torch.tensor(0.1, dtype=torch.float32)) + p64["moving_mean"]
    want_v = DECAY * 1.0 + p64["moving_var"]
    e_mean, e_var = float((mm.double().cpu() - want_m).abs().max()), float((mv.double().cpu() - want_v).abs().max())
    tol_m, tol_v = (4 * 2.0 ** -24 * float(w.abs().max()) for w in (want_m, want_v))
    print(f"[bn] unbiased blend from (0.1, 1): moving_mean {e_mean:.3e} (<= {tol_m:.3e}), moving_variance {e_var:.3e} (<= {tol_v:.3e})")
    assert e_mean <= tol_m and e_var <= tol_v


FOLD_C = 12


@functools.lru_cache(maxsize=None)
def fold_partials(nblk):
    """Synthetic [nblk][2][C] partials: per 64-row block the fp32 column sums of x and x^2 of a random matrix (mean / std <= 0.5)."""
    g = torch.Generator().manual_seed(nblk)
    std, m = 0.5 + torch.rand(FOLD_C, generator=g), 0.25 * torch.randn(FOLD_C, generator=g).clamp(-1, 1)
    x = (std * torch.randn(nblk, 64, FOLD_C, generator=g) + m)
    gamma, beta = 1 + 0.2 * torch.randn(FOLD_C, generator=g), 0.1 * torch.randn(FOLD_C, generator=g)
    return torch.stack([x.sum(1), (x * x).sum(1)], 1).contiguous(), gamma, beta


@pytest.mark.parametrize("nblk", [1, 63, 2047, 2048, 2100])
def test_fold_alone(nblk, entries):
    """ops.bn_fold against the SAME fp32 partials folded in fp64 on the CPU: mean, var, scale, shift and the moving statistics (from zero,
    unbiased).  nblk >= 2048 takes partial_colsums<4>, below it <16>; C = 12 fills neither's last workgroup.  The kernel folds in fp64 and
    rounds once (mean, var) or through two or three fp32 operations (scale, shift, the moving statistics): the rule's floor, 1e-6."""
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    partial, gamma, beta = fold_partials(nblk)
    rows = nblk * 64
    p = partial.double()
    mu = p[:, 0].sum(0) / rows
    var = p[:, 1].sum(0) / rows - mu * mu
    scale = gamma.double() / torch.sqrt(var + R.BN_EPS)
    want = dict(mean=mu, var=var, scale=scale, shift=beta.double() - mu * scale, moving_mean=ONE_MINUS_DECAY * mu,
                moving_var=ONE_MINUS_DECAY * var * (rows / (rows - 1)))
    assert float(var.min()) > 0.1
    mm, mv = _moving(FOLD_C, dev)
    mean_g, var_g, scale_g, shift_g = ops.bn_fold(partial.to(dev), nblk, FOLD_C, rows, gamma.to(dev), beta.to(dev), mm, mv)
    torch.cuda.synchronize()
    got = dict(mean=mean_g, var=var_g, scale=scale_g, shift=shift_g, moving_mean=mm, moving_var=mv)
    figures = {n: R.figure(got[n], want[n], n, 1) for n in want}
    for n, e in figures.items():
        print(f"[bn] fold_alone nblk {nblk} {n}: {e:.3e}")
    assert [e for e in entries if e.startswith(PREFIX)] == ["lpm_bn_fold"]
    for n, e in figures.items():
        assert e <= 1e-6, (n, e)
