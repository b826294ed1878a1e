"""-m gpu: the frame-prep family (csrc/frame_prep.hip) -- ops.frame_sample_bn in its four apply forms, ops.frame_sample_bn_split,
ops.frame_gather_bn_split, each from fp32 frames and from the reader's uint8 frames (eval mode, and training mode with
quantised_training=True), and ops.dequantize_l2_normalize / ops.l2_normalize_rows on their own -- against the fp64 restatement
tests/_frame_prep_ref.py, never against the op itself, under the rule and layout of tests/test_gpu_netvlad_bounds.py: per named part the
op's error is at most max(8 err32, 1e-6), err32 the error of the same restatement evaluated in fp32 on the CPU.

Parts: y (the larger of the per-clip figure, max over clips of max |error| / max |fp64| in the clip, and the same quotient per column, as
tests/test_gpu_bn_bounds.py takes it); batch_mean and batch_var read back from moving statistics started at zero and divided by
tests/_netvlad_ref.ONE_MINUS_DECAY (the blend factor 1 - fp32(0.999) is fp32 arithmetic both sides share: it is in the model); dgamma and
dbeta with clip b's upstream gradient N(0, 1) x 10^(6 b / (B - 1) - 3).  A second call from (0, 1) keeps the decay covered
(test_moving_statistics_blend_with_the_decay, the tolerances of the NetVLAD file).  Eval mode normalises with given moving statistics,
the true moments of the sampled rows plus noise, and holds y, dgamma, dbeta (uint8 frames in eval mode: y alone -- that path has no
backward).  Every element counts; nothing is masked out.  Every figure is printed before anything is asserted.

Forms (FORMS): sample = frame_sample_bn (lpm_frame_apply at F = 128 / 2048, the tile-writing lpm_frame_apply_tiles at F = 1024 / 1152
under VLAD_PRECISION = "bf16x3"), row_tiles = the same with FRAME_ROW_TILES on (lpm_frame_apply_tiles2), bf16 = storage="bf16",
materialize=True (lpm_frame_apply_tiles_bf16), split = frame_sample_bn_split, gather = frame_gather_bn_split on a random index table
that repeats a row and names the last valid frame of every clip.  The tile images stay with the bitwise tests of
tests/test_gpu_kernels.py and the uint8 / fp32 identity with tests/test_gpu_frame_gather.py.

The route is asserted: the entry names that pass through _capi._Lib.check are recorded, and those that begin with lpm_frame_ (the fold,
lpm_frame_bn_fold, among them) or are lpm_bn_fold must be exactly the case's list (route()), with multiplicity.

Shapes (B, MF, F, S), each the smallest that reaches its edge:
(1, 3, 128, 3)        fewer gathered rows than the eight pivot rows; one clip
(2, 7, 128, 7)        14 rows in one partly filled 32-row statistics block; a clip of one frame, so all its samples are one row
(5, 40, 128, 7)       35 rows: the second block holds 3 rows; S < MF
(2, 40, 1024, 32)     exactly two blocks; the tile route
(3, 33, 1152, 33)     288 uchar4 columns, more than the 256 threads of the uint8 form; 4.5 passes of the fp32 form; Dv = 1024, Da = 128
(2, 5, 2048, 5)       the largest F the dequantising waves take: all eight unrolled slots
(2, 300, 1152, 300)   the whole frame walk
num_frames is ragged, with one full clip and one single-frame clip.  A single-row batch stays out: its fp64 variance is identically
zero, and any fp32 rounding of the mean is O(1) against rsqrt(eps) there.

Regimes (tests/_frame_prep_ref.make_inputs): every fp32 regime and both uint8 regimes on (5,40,128,7), (3,33,1152,33) and (2,40,1024,32),
three seeds each; random, offset30, q8_random and q8_narrow on the other shapes.  The seeds (SEEDS) were picked on the CPU from the
reference alone (tests/_frame_prep_ref.conditions, held by tests/test_frame_prep_ref_host.py); the condition values stand beside them.

Measured on the MI355X, worst error / bound over parts, forms and seeds (the part that gives it in brackets):
MEASURED-BEGIN
Worst error / bound over forms, parts and seeds (the part that gives it), as the kernels stood before the shifted sums and the centre
(the parent's library under this file) and after:
(B,MF,F,S)         regime         training: before         after                eval: before             after               
(5,40,128,7)       random         0.34 (y)                 0.22 (y)             0.12 (y)                 0.12 (y)            
(5,40,128,7)       offset3        4.04 (batch_var)         0.23 (batch_var)     0.37 (dgamma)            0.16 (y)            
(5,40,128,7)       offset10       35.46 (batch_var)        0.21 (batch_var)     1.58 (dgamma)            0.10 (y)            
(5,40,128,7)       offset30       358.90 (batch_var)       0.16 (batch_var)     3.86 (dgamma)            0.10 (y)            
(5,40,128,7)       mixed          358.90 (batch_var)       0.21 (batch_var)     3.86 (dgamma)            0.12 (y)            
(5,40,128,7)       column_spread  0.38 (y)                 0.23 (dgamma)        0.11 (y)                 0.11 (y)            
(5,40,128,7)       clip_offsets   0.79 (y)                 0.27 (batch_mean)    0.14 (y)                 0.12 (y)            
(5,40,128,7)       q8_random      0.21 (batch_var)         0.20 (batch_var)     0.12 (y)                 0.12 (y)            
(5,40,128,7)       q8_narrow      13.19 (batch_var)        0.10 (batch_mean)    0.10 (y)                 0.11 (y)            
(3,33,1152,33)     random         0.50 (y)                 0.37 (batch_var)     0.32 (dgamma)            0.32 (dgamma)       
(3,33,1152,33)     offset3        4.62 (batch_var)         0.30 (batch_var)     0.97 (dgamma)            0.15 (dgamma)       
(3,33,1152,33)     offset10       24.36 (batch_var)        0.32 (batch_var)     3.76 (dgamma)            0.18 (dgamma)       
(3,33,1152,33)     offset30       176.54 (batch_var)       0.23 (batch_var)     11.30 (dgamma)           0.20 (dgamma)       
(3,33,1152,33)     mixed          200.09 (batch_var)       0.37 (batch_var)     7.12 (dgamma)            0.32 (dgamma)       
(3,33,1152,33)     column_spread  0.60 (batch_var)         0.45 (dgamma)        0.42 (dgamma)            0.42 (dgamma)       
(3,33,1152,33)     clip_offsets   12.48 (y)                0.20 (batch_mean)    0.62 (dgamma)            0.18 (dgamma)       
(3,33,1152,33)     q8_random      0.33 (dgamma)            0.33 (dgamma)        0.10 (y)                 0.10 (y)            
(3,33,1152,33)     q8_narrow      11.21 (batch_var)        0.15 (dbeta)         0.11 (y)                 0.10 (y)            
(2,40,1024,32)     random         1.02 (batch_var)         0.28 (dgamma)        0.36 (dgamma)            0.26 (dgamma)       
(2,40,1024,32)     offset3        3.89 (batch_var)         0.22 (batch_var)     1.55 (dgamma)            0.20 (dgamma)       
(2,40,1024,32)     offset10       31.18 (batch_var)        0.24 (dbeta)         3.85 (dgamma)            0.24 (dbeta)        
(2,40,1024,32)     offset30       262.72 (batch_var)       0.27 (batch_var)     10.86 (dgamma)           0.24 (dbeta)        
(2,40,1024,32)     mixed          262.72 (batch_var)       0.26 (batch_var)     10.57 (dgamma)           0.25 (dgamma)       
(2,40,1024,32)     column_spread  1.05 (batch_var)         0.42 (batch_var)     0.37 (dgamma)            0.37 (dgamma)       
(2,40,1024,32)     clip_offsets   15.51 (y)                0.24 (dbeta)         2.40 (dgamma)            0.27 (dgamma)       
(2,40,1024,32)     q8_random      0.47 (batch_var)         0.41 (dgamma)        0.10 (y)                 0.10 (y)            
(2,40,1024,32)     q8_narrow      15.33 (batch_var)        0.24 (dbeta)         0.16 (y)                 0.17 (y)            
(1,3,128,3)        random         0.81 (y)                 0.11 (y)             23.30 (y)                0.09 (y)            
(1,3,128,3)        offset30       53.80 (batch_var)        0.13 (dgamma)        384.76 (y)               0.10 (y)            
(1,3,128,3)        q8_random      0.35 (dgamma)            0.18 (y)             0.13 (y)                 0.14 (y)            
(1,3,128,3)        q8_narrow      3.60 (batch_var)         0.13 (batch_mean)    0.17 (y)                 0.17 (y)            
(2,7,128,7)        random         0.52 (y)                 0.13 (batch_var)     0.12 (dgamma)            0.12 (dgamma)       
(2,7,128,7)        offset30       109.05 (batch_var)       0.12 (batch_var)     8.91 (dgamma)            0.10 (y)            
(2,7,128,7)        q8_random      0.28 (dgamma)            0.16 (batch_mean)    0.10 (y)                 0.10 (y)            
(2,7,128,7)        q8_narrow      18.50 (batch_var)        0.12 (batch_var)     0.12 (y)                 0.12 (y)            
(2,5,2048,5)       random         4.12 (y)                 0.15 (batch_var)     0.45 (y)                 0.10 (dgamma)       
(2,5,2048,5)       offset30       93.69 (batch_var)        0.14 (batch_var)     26.17 (y)                0.10 (y)            
(2,5,2048,5)       q8_random      0.18 (dgamma)            0.13 (dgamma)        0.23 (y)                 0.16 (y)            
(2,5,2048,5)       q8_narrow      5.10 (batch_var)         0.09 (batch_mean)    0.16 (y)                 0.13 (y)            
(2,300,1152,300)   random         1.08 (batch_var)         0.26 (batch_var)     0.23 (dgamma)            0.22 (dgamma)       
(2,300,1152,300)   offset30       218.87 (batch_var)       0.14 (batch_var)     6.01 (dgamma)            0.10 (dgamma)       
(2,300,1152,300)   q8_random      0.26 (batch_var)         0.19 (batch_var)     0.10 (y)                 0.10 (y)            
(2,300,1152,300)   q8_narrow      8.14 (batch_var)         0.10 (dbeta)         0.12 (y)                 0.10 (y)            
ops.dequantize_l2_normalize alone: 0.13 before, 0.13 after;  ops.l2_normalize_rows alone: 0.13 before, 0.13 after (neither kernel changed).
Failed before: 175 of the 344 cases of test_form_meets_the_bound (after: 0) -- by regime and mode, shapes x forms beyond the bound:
  offset3 training: (5,40,128,7) 3, (3,33,1152,33) 5, (2,40,1024,32) 5
  offset10 training: (5,40,128,7) 3, (3,33,1152,33) 5, (2,40,1024,32) 5
  offset10 eval: (5,40,128,7) 3, (3,33,1152,33) 5, (2,40,1024,32) 5
  offset30 training: (5,40,128,7) 3, (3,33,1152,33) 5, (2,40,1024,32) 5, (1,3,128,3) 3, (2,7,128,7) 3, (2,5,2048,5) 3, (2,300,1152,300) 5
  offset30 eval: (5,40,128,7) 3, (3,33,1152,33) 5, (2,40,1024,32) 5, (1,3,128,3) 3, (2,7,128,7) 3, (2,5,2048,5) 3, (2,300,1152,300) 5
  mixed training: (5,40,128,7) 3, (3,33,1152,33) 5, (2,40,1024,32) 5
  mixed eval: (5,40,128,7) 3, (3,33,1152,33) 5, (2,40,1024,32) 5
  q8_narrow training: (5,40,128,7) 3, (3,33,1152,33) 5, (2,40,1024,32) 5, (1,3,128,3) 3, (2,7,128,7) 3, (2,5,2048,5) 3, (2,300,1152,300) 5
  clip_offsets training: (3,33,1152,33) 5, (2,40,1024,32) 5
  random training: (2,40,1024,32) 5, (2,5,2048,5) 1, (2,300,1152,300) 1
  offset3 eval: (2,40,1024,32) 5
  column_spread training: (2,40,1024,32) 1
  clip_offsets eval: (2,40,1024,32) 5
  random eval: (1,3,128,3) 1
What the figures led to: frame_stats_kernel's shifted sums beside the raw ones and lpm_frame_bn_fold (the variance);
the per-column centre of the apply forms and of the backward's partial sums (eval mode, found by this file: y = x scale + (beta - mean scale)
and sum dy x lose eps32 (mean/std) where the restatement, given the mean, subtracts it exactly).  With the fold taking the shifted sums
from mean^2 > var, nine cases stayed at 1.02 (batch_var; random and mixed at (2,40,1024,32), seed 1, four forms each, and random at
(2,300,1152,300) through the table): half the batch there is ONE row, the single frame of the last clip, whose equal addends round the same
way every time, in columns at |mean|/std = 0.92 .. 0.96 -- the raw sums' path; the fold now takes the shifted sums from 4 mean^2 > var.
MEASURED-END"""
import functools
import math

import pytest
import torch

from tests import _frame_prep_ref as R
from tests._util import cuda

pytestmark = pytest.mark.gpu

REGIME_SHAPES = [(5, 40, 128, 7), (3, 33, 1152, 33), (2, 40, 1024, 32)]          # B, MF, F, S: every regime, three seeds
OTHER_SHAPES = [(1, 3, 128, 3), (2, 7, 128, 7), (2, 5, 2048, 5), (2, 300, 1152, 300)]
OTHER_REGIMES = ("random", "offset30", "q8_random", "q8_narrow")
FORMS = ("sample", "row_tiles", "bf16", "split", "gather")
TRACKED_PREFIX = "lpm_frame_"

# (shape, regime) -> seeds.  Beside every seed: tests/_frame_prep_ref.conditions' values for the uniform index / for the index table --
# least err32 of a part, least squared norm of a sampled row before the normalisation (inf: fp32 frames), median and maximum over the
# held columns of |mean| / std, least column variance.  Refused by the conditions: (2, 40, 1024, 32) offset3 seed 2 (one column's
# |mean| / std below 0.25 R).
SEEDS = {
    ((5, 40, 128, 7), "random"): (0, 1, 2),
    #   0: 7.2e-08 inf 0.32 1.2 0.13 / 7.5e-08 inf 0.36 1.5 0.17
    #   1: 6.5e-08 inf 0.22 1.2 0.21 / 6.5e-08 inf 0.24 1.1 0.22
    #   2: 5.7e-08 inf 0.27 1.5 0.13 / 5.7e-08 inf 0.32 1.5 0.18
    ((5, 40, 128, 7), "offset3"): (0, 1, 2),
    #   0: 7.7e-08 inf 3.1 5.1 0.13 / 7.7e-08 inf 3.2 5.9 0.17
    #   1: 6.5e-08 inf 3.2 4.3 0.21 / 6.5e-08 inf 3.2 5.1 0.22
    #   2: 5.7e-08 inf 3.2 4.8 0.13 / 5.7e-08 inf 3.3 5.2 0.18
    ((5, 40, 128, 7), "offset10"): (0, 1, 2),
    #   0: 7.7e-08 inf 10 17 0.13 / 7.7e-08 inf 10 18 0.17
    #   1: 6.5e-08 inf 11 15 0.21 / 6.5e-08 inf 11 17 0.22
    #   2: 5.7e-08 inf 11 16 0.13 / 5.7e-08 inf 11 17 0.18
    ((5, 40, 128, 7), "offset30"): (0, 1, 2),
    #   0: 7.7e-08 inf 31 52 0.13 / 7.7e-08 inf 31 54 0.17
    #   1: 6.5e-08 inf 32 46 0.21 / 6.5e-08 inf 32 51 0.22
    #   2: 5.7e-08 inf 32 47 0.13 / 5.7e-08 inf 32 49 0.18
    ((5, 40, 128, 7), "mixed"): (0, 1, 2),
    #   0: 7.7e-08 inf 32 52 0.13 / 7.7e-08 inf 34 54 0.17
    #   1: 6.5e-08 inf 31 44 0.21 / 6.5e-08 inf 33 49 0.22
    #   2: 5.7e-08 inf 31 46 0.13 / 5.7e-08 inf 32 48 0.18
    ((5, 40, 128, 7), "column_spread"): (0, 1, 2),
    #   0: 6.5e-08 inf 0.28 1.2 5.4e-09 / 5.2e-08 inf 0.33 1.3 6.8e-09
    #   1: 4.3e-08 inf 0.21 1.1 5.4e-09 / 3.7e-08 inf 0.23 1 5.8e-09
    #   2: 5.7e-08 inf 0.26 1.2 9.8e-09 / 5.7e-08 inf 0.29 1.5 7.7e-09
    ((5, 40, 128, 7), "clip_offsets"): (0, 1, 2),
    #   0: 7.7e-08 inf 0.36 2.2 0.065 / 6e-08 inf 0.36 2.2 0.072
    #   1: 6.5e-08 inf 0.3 3.1 0.065 / 6.5e-08 inf 0.3 3 0.06
    #   2: 5.7e-08 inf 0.42 2.6 0.026 / 5.7e-08 inf 0.42 2.3 0.029
    ((5, 40, 128, 7), "q8_random"): (0, 1, 2),
    #   0: 7.7e-08 1.4e+02 0.19 0.74 0.0036 / 7.7e-08 1.5e+02 0.2 1.1 0.0031
    #   1: 6.5e-08 1.5e+02 0.18 0.58 0.0043 / 6.5e-08 1.5e+02 0.21 1.2 0.0028
    #   2: 5.7e-08 1.6e+02 0.18 0.54 0.004 / 5.7e-08 1.5e+02 0.19 0.8 0.0038
    ((5, 40, 128, 7), "q8_narrow"): (0, 1, 2),
    #   0: 7.7e-08 83 16 36 9e-06 / 7.7e-08 83 16 43 8.3e-06
    #   1: 6.5e-08 73 13 41 1.4e-05 / 6.5e-08 73 14 38 1.1e-05
    #   2: 5.7e-08 80 15 45 1.1e-05 / 5.7e-08 80 15 39 9.8e-06
    ((3, 33, 1152, 33), "random"): (0, 1, 2),
    #   0: 1.1e-07 inf 0.34 2.2 0.13 / 1.1e-07 inf 0.36 2.6 0.11
    #   1: 1.1e-07 inf 0.34 2.3 0.13 / 8.4e-08 inf 0.37 2.3 0.11
    #   2: 1.1e-07 inf 0.38 2.2 0.11 / 1.1e-07 inf 0.39 2 0.1
    ((3, 33, 1152, 33), "offset3"): (0, 1, 2),
    #   0: 1.1e-07 inf 3.4 5.5 0.13 / 9.7e-08 inf 3.4 5.9 0.11
    #   1: 1.1e-07 inf 3.4 5.3 0.13 / 1.1e-07 inf 3.4 5.6 0.11
    #   2: 9.7e-08 inf 3.4 5.8 0.11 / 1.1e-07 inf 3.4 6.2 0.1
    ((3, 33, 1152, 33), "offset10"): (0, 1, 2),
    #   0: 1.1e-07 inf 11 18 0.13 / 1.1e-07 inf 11 20 0.11
    #   1: 1.1e-07 inf 11 17 0.13 / 1e-07 inf 11 19 0.11
    #   2: 1.1e-07 inf 11 19 0.11 / 1.1e-07 inf 11 20 0.1
    ((3, 33, 1152, 33), "offset30"): (0, 1, 2),
    #   0: 1.1e-07 inf 34 54 0.13 / 1.1e-07 inf 34 58 0.11
    #   1: 1.1e-07 inf 34 52 0.13 / 1.1e-07 inf 34 59 0.11
    #   2: 1.1e-07 inf 34 55 0.11 / 1.1e-07 inf 34 59 0.1
    ((3, 33, 1152, 33), "mixed"): (0, 1, 2),
    #   0: 1.1e-07 inf 34 46 0.13 / 1.1e-07 inf 34 53 0.11
    #   1: 1.1e-07 inf 33 48 0.13 / 9e-08 inf 34 50 0.11
    #   2: 1.1e-07 inf 34 55 0.11 / 1.1e-07 inf 34 59 0.1
    ((3, 33, 1152, 33), "column_spread"): (0, 1, 2),
    #   0: 5.2e-08 inf 0.33 1.5 5.7e-09 / 6.3e-08 inf 0.35 1.7 4.5e-09
    #   1: 9.8e-08 inf 0.34 1.6 5e-09 / 1.1e-07 inf 0.35 1.6 4.5e-09
    #   2: 1.1e-07 inf 0.36 1.8 5.2e-09 / 1.1e-07 inf 0.37 1.9 4e-09
    ((3, 33, 1152, 33), "clip_offsets"): (0, 1, 2),
    #   0: 1.1e-07 inf 0.55 11 0.0022 / 7.8e-08 inf 0.56 11 0.002
    #   1: 9.2e-08 inf 0.56 23 0.00068 / 8.3e-08 inf 0.56 23 0.00056
    #   2: 1.1e-07 inf 0.58 11 0.0029 / 1.1e-07 inf 0.58 11 0.0033
    ((3, 33, 1152, 33), "q8_random"): (0, 1, 2),
    #   0: 1.1e-07 1.5e+03 0.32 0.83 0.00037 / 1.1e-07 1.5e+03 0.31 0.98 0.00028
    #   1: 1.1e-07 1.5e+03 0.31 0.81 0.00032 / 1.1e-07 1.5e+03 0.32 0.99 0.00031
    #   2: 1.1e-07 1.4e+03 0.32 0.92 0.00037 / 1.1e-07 1.5e+03 0.32 0.97 0.00032
    ((3, 33, 1152, 33), "q8_narrow"): (0, 1, 2),
    #   0: 1.1e-07 7.3e+02 17 50 9.5e-07 / 1.1e-07 7.4e+02 17 53 8.4e-07
    #   1: 1.1e-07 7.5e+02 16 42 9.5e-07 / 1.1e-07 7.5e+02 16 45 6.7e-07
    #   2: 1.1e-07 7.5e+02 16 44 9.1e-07 / 1.1e-07 7.5e+02 16 47 7.7e-07
    ((2, 40, 1024, 32), "random"): (0, 1, 2),
    #   0: 1e-07 inf 0.48 2.3 0.091 / 1.2e-07 inf 0.51 2.9 0.056
    #   1: 1.1e-07 inf 0.51 2.4 0.098 / 1.3e-07 inf 0.5 2.5 0.057
    #   2: 1.3e-07 inf 0.52 2.4 0.075 / 8.9e-08 inf 0.55 2.5 0.06
    ((2, 40, 1024, 32), "offset3"): (0, 1, 3),
    #   0: 8e-08 inf 3.8 6.4 0.091 / 9.3e-08 inf 3.8 8.5 0.056
    #   1: 1e-07 inf 3.8 6.4 0.098 / 1.3e-07 inf 3.7 7.8 0.057
    #   3: 1.1e-07 inf 3.8 7.7 0.07 / 1.3e-07 inf 3.8 7 0.056
    ((2, 40, 1024, 32), "offset10"): (0, 1, 2),
    #   0: 1.4e-07 inf 12 21 0.091 / 1.2e-07 inf 13 27 0.056
    #   1: 1.2e-07 inf 12 21 0.098 / 9.7e-08 inf 12 24 0.057
    #   2: 1.3e-07 inf 13 22 0.075 / 1.3e-07 inf 13 26 0.06
    ((2, 40, 1024, 32), "offset30"): (0, 1, 2),
    #   0: 1.4e-07 inf 37 61 0.091 / 8.5e-08 inf 38 82 0.056
    #   1: 8.6e-08 inf 37 61 0.098 / 9.7e-08 inf 37 73 0.057
    #   2: 1.1e-07 inf 38 64 0.075 / 1.3e-07 inf 38 77 0.06
    ((2, 40, 1024, 32), "mixed"): (0, 1, 2),
    #   0: 1.4e-07 inf 37 61 0.091 / 8.5e-08 inf 38 68 0.056
    #   1: 1.1e-07 inf 38 61 0.098 / 1.3e-07 inf 38 73 0.057
    #   2: 1.3e-07 inf 38 58 0.075 / 1.3e-07 inf 38 77 0.06
    ((2, 40, 1024, 32), "column_spread"): (0, 1, 2),
    #   0: 1.2e-07 inf 0.48 2.1 3.6e-09 / 1.1e-07 inf 0.51 2.5 2.4e-09
    #   1: 1.3e-07 inf 0.49 1.9 2.9e-09 / 1.2e-07 inf 0.48 2.2 4e-09
    #   2: 9.9e-08 inf 0.51 2.4 4.4e-09 / 1.3e-07 inf 0.52 2 2.8e-09
    ((2, 40, 1024, 32), "clip_offsets"): (0, 1, 2),
    #   0: 1.4e-07 inf 1 35 0.00031 / 1.4e-07 inf 1 51 0.00036
    #   1: 1.1e-07 inf 0.98 57 0.00045 / 1.3e-07 inf 0.99 49 0.00036
    #   2: 1.3e-07 inf 0.93 39 0.00021 / 1.3e-07 inf 0.93 36 0.00017
    ((2, 40, 1024, 32), "q8_random"): (0, 1, 2),
    #   0: 1.4e-07 1.3e+03 0.52 1.2 0.0002 / 1.4e-07 1.3e+03 0.54 1.5 0.0002
    #   1: 1.3e-07 1.3e+03 0.51 1.1 0.00023 / 1.3e-07 1.3e+03 0.51 1.8 0.00022
    #   2: 1.3e-07 1.3e+03 0.52 1.2 0.00031 / 1.3e-07 1.3e+03 0.52 1.5 0.00022
    ((2, 40, 1024, 32), "q8_narrow"): (0, 1, 2),
    #   0: 1.4e-07 6.5e+02 17 56 8.1e-07 / 1.4e-07 6.5e+02 18 66 5e-07
    #   1: 1.3e-07 6.2e+02 17 54 8.2e-07 / 1.3e-07 6.2e+02 17 68 6.3e-07
    #   2: 1.3e-07 6.6e+02 18 50 7.1e-07 / 1.3e-07 6.6e+02 18 64 5.3e-07
    ((1, 3, 128, 3), "random"): (0,),
    #   0: 4.6e-08 inf 0.63 6.4 0.0096 / 5e-08 inf 1.2 1.1e+03 1.8e-07
    ((1, 3, 128, 3), "offset30"): (0,),
    #   0: 5e-08 inf 46 2.5e+02 0.0096 / 1.9e-08 inf 72 9.2e+04 1.8e-07
    ((1, 3, 128, 3), "q8_random"): (0,),
    #   0: 5.8e-08 1.5e+02 0.52 12 7.4e-05 / 5.8e-08 1.5e+02 1.3 8.8e+02 9.5e-09
    ((1, 3, 128, 3), "q8_narrow"): (0,),
    #   0: 5.8e-08 80 20 1.4e+02 6.2e-07 / 5.8e-08 80 32 2.1e+03 6.7e-13
    ((2, 7, 128, 7), "random"): (0,),
    #   0: 8.1e-08 inf 0.52 2.7 0.043 / 8.1e-08 inf 0.52 3.2 0.047
    ((2, 7, 128, 7), "offset30"): (0,),
    #   0: 8.1e-08 inf 38 1.3e+02 0.043 / 8.1e-08 inf 39 1.7e+02 0.047
    ((2, 7, 128, 7), "q8_random"): (0,),
    #   0: 8.1e-08 1.6e+02 0.55 2 0.0011 / 8.1e-08 1.6e+02 0.56 4.6 0.00054
    ((2, 7, 128, 7), "q8_narrow"): (0,),
    #   0: 8.1e-08 79 17 71 2.2e-06 / 8.1e-08 79 19 1.2e+02 7.9e-07
    ((2, 5, 2048, 5), "random"): (0,),
    #   0: 6.8e-08 inf 0.6 5.3 0.007 / 6.8e-08 inf 0.88 45 0.00013
    ((2, 5, 2048, 5), "offset30"): (0,),
    #   0: 6.8e-08 inf 40 2.3e+02 0.007 / 6.8e-08 inf 49 1.6e+03 0.00013
    ((2, 5, 2048, 5), "q8_random"): (0,),
    #   0: 6.8e-08 2.8e+03 0.51 7.8 1.2e-05 / 6.8e-08 2.8e+03 0.72 42 1.1e-07
    ((2, 5, 2048, 5), "q8_narrow"): (0,),
    #   0: 6.8e-08 1.3e+03 18 1.1e+02 3.7e-08 / 6.8e-08 1.3e+03 22 9e+02 1.9e-11
    ((2, 300, 1152, 300), "random"): (0,),
    #   0: 1.4e-07 inf 0.49 2 0.11 / 1.3e-07 inf 0.49 2 0.091
    ((2, 300, 1152, 300), "offset30"): (0,),
    #   0: 1.4e-07 inf 38 50 0.11 / 1.4e-07 inf 38 51 0.091
    ((2, 300, 1152, 300), "q8_random"): (0,),
    #   0: 1.4e-07 1.4e+03 0.52 0.89 0.00039 / 1.4e-07 1.4e+03 0.52 0.97 0.00036
    ((2, 300, 1152, 300), "q8_narrow"): (0,),
    #   0: 1.4e-07 7.3e+02 17 42 1.1e-06 / 1.4e-07 7.3e+02 17 43 1.1e-06
}


def seeds_of(shape, regime):
    return SEEDS[(tuple(shape), regime)]


def forms_of(F):
    """The tile-writing forms exist at the two input widths of the frame-level models."""
    return [f for f in FORMS if F in (1024, 1152) or f not in ("row_tiles", "bf16")]


def split_of(F):
    """Dv of the split and gather forms: the rgb block of a 1152-wide input, half the features elsewhere."""
    return 1024 if F == 1152 else F // 2


def _cases():
    """(shape, regime) pairs in the order of the docstring."""
    out = [(s, r) for s in REGIME_SHAPES for r in R.REGIMES]
    return out + [(s, r) for s in OTHER_SHAPES for r in OTHER_REGIMES]


def _params():
    for shape, regime in _cases():
        for form in forms_of(shape[2]):
            for training in (True, False):
                yield pytest.param(form, shape, regime, training,
                                   id=f"{form}-{'x'.join(map(str, shape))}-{regime}-{'training' if training else 'eval'}")


@functools.lru_cache(maxsize=None)
def reference(shape, seed, regime, uniform, training):
    """-> (inputs, fp64 parts, fp32 parts, err32 per part, eval-mode moving statistics or None, (ok, condition values)) of the rows the op
    samples.  Computed once per key and shared; nothing in it is changed afterwards."""
    B, MF, F, S = shape
    inputs = R.make_inputs(B, MF, F, S, seed, regime)
    moving = None if training else R.moving_for_eval(inputs, uniform, S)
    p64 = R.frame_prep_ref(inputs, torch.float64, S, uniform=uniform, training=training, moving=moving)
    p32 = R.frame_prep_ref(inputs, torch.float32, S, uniform=uniform, training=training, moving=moving)
    e32 = {n: R.part_figure(p32[n], p64[n], n, B) for n in p64}
    return inputs, p64, p32, e32, moving, R.conditions(inputs, S, p64, p32, uniform=uniform, regime=regime)


def route(form, F, q8, training):
    """The lpm_frame_* entries and the fold of one forward (+ backward) of the form, in order."""
    sfx = "_q8" if q8 else ""
    if form == "gather":
        names = ["lpm_frame_inv_norm_q8_idx"] if q8 else []
        if training:
            names += ["lpm_frame_stats_idx" + sfx, "lpm_frame_bn_fold"]
        names.append("lpm_frame_apply_split_idx" + sfx)
        bwd = "lpm_frame_bn_bwd_split_idx" + sfx
    else:
        names = ["lpm_frame_inv_norm_q8"] if q8 else []
        if training:
            names += ["lpm_frame_stats" + sfx, "lpm_frame_bn_fold"]
        apply = {"sample": "lpm_frame_apply_tiles" if F in (1024, 1152) else "lpm_frame_apply", "row_tiles": "lpm_frame_apply_tiles2",
                 "bf16": "lpm_frame_apply_tiles_bf16", "split": "lpm_frame_apply_tiles_split"}[form]
        names.append(apply + sfx)
        bwd = ("lpm_frame_bn_bwd_split" if form == "split" else "lpm_frame_bn_bwd") + sfx
    if training or not q8:                      # (uint8 frames in eval mode: no backward)
        names.append(bwd)
    return names


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


def tracked(entries):
    return [e for e in entries if e.startswith(TRACKED_PREFIX) or e == "lpm_bn_fold"]


def run_form(form, shape, inputs, dev, training, moving, monkeypatch, start=None):
    """One forward (+ backward, where the path has one) of the form -> {part: tensor}; the moving statistics start from zeros in training
    mode (``start``: from that pair instead) and are returned as the op left them under "moving"."""
    from learnablepoolingmethods_amd import ops
    B, MF, F, S = shape
    q8 = "q" in inputs
    monkeypatch.setattr(ops, "VLAD_PRECISION", "bf16x3")
    monkeypatch.setattr(ops, "FRAME_ROW_TILES", form == "row_tiles")
    frames = (inputs["q"] if q8 else inputs["frames"]).to(dev)
    nf = inputs["nf"].to(dev)
    grads = training or not q8
    gamma, beta = (inputs[k].detach().to(dev).requires_grad_(grads) for k in ("gamma", "beta"))
    if training:
        mm, mv = (torch.zeros(F, device=dev), torch.zeros(F, device=dev)) if start is None else (t.to(dev).clone() for t in start)
    else:
        mm, mv = (m.to(dev) for m in moving)
    Dv = split_of(F)
    if form == "gather":
        index = inputs["random_index"].to(torch.int32).to(dev)
        y = torch.cat(ops.frame_gather_bn_split(frames, nf, index, gamma, beta, mm, mv, training, Dv, quantised_training=q8 and training), 1)
    elif form == "split":
        y = torch.cat(ops.frame_sample_bn_split(frames, nf, S, gamma, beta, mm, mv, training, Dv, quantised_training=q8 and training), 1)
    else:
        y = ops.frame_sample_bn(frames, nf, S, gamma, beta, mm, mv, is_training=training, storage="bf16" if form == "bf16" else "f32",
                                materialize=True, quantised_training=q8 and training)
    got = dict(y=y.detach())
    if grads:
        got["dgamma"], got["dbeta"] = torch.autograd.grad((y * inputs["up"].to(dev)).sum(), [gamma, beta])
    torch.cuda.synchronize()
    if training:
        got["moving"] = (mm, mv)
        if start is None:                      # from zero moving statistics: (1 - fp32(0.999)) x the batch statistics
            got["batch_mean"], got["batch_var"] = (m.double().cpu() / R.ONE_MINUS_DECAY for m in (mm, mv))
    return got


@pytest.mark.parametrize("form,shape,regime,training", list(_params()))
def test_form_meets_the_bound(form, shape, regime, training, monkeypatch, entries):
    dev = cuda()
    B, MF, F, S = shape
    uniform = form != "gather"
    rows, routes = [], []
    for seed in seeds_of(shape, regime):
        inputs, p64, _, e32, moving, (ok, cond) = reference(shape, seed, regime, uniform, training)
        tag = f"{form} {shape} {regime} {'training' if training else 'eval'} seed {seed}"
        print(f"[frame_prep] {tag}: conditions {ok} " + ", ".join(f"{v:.2e}" for v in cond))
        assert ok, f"{tag}: the seed does not meet the conditions {cond}"
        del entries[:]
        got = run_form(form, shape, inputs, dev, training, moving, monkeypatch)
        routes.append((tag, tracked(entries), route(form, F, "q" in inputs, training)))
        parts = [n for n in p64 if n in got]
        assert parts == list(p64) or ("q" in inputs and not training and parts == ["y"]), tag
        for n in parts:
            e_op = R.part_figure(got[n], p64[n], n, B)
            bound = max(8 * e32[n], 1e-6)
            rows.append((tag, n, e_op, e32[n], bound))
            print(f"[frame_prep] {tag} {n}: op {e_op:.3e}, err32 {e32[n]:.3e}, bound {bound:.3e}, ratio {e_op / bound:.3f}")
    for tag, n, e_op, e, bound in rows:
        assert e > 0, f"{tag} {n}: err32 is zero"
        assert math.isfinite(e_op) and e_op <= bound, f"{tag} {n}: op error {e_op:.3e} > max(8 x {e:.3e}, 1e-6)"
    for tag, seen, want in routes:
        assert seen == want, f"{tag}: route {seen}"


BLEND_SHAPES = [(5, 40, 128, 7), (3, 33, 1152, 33)]


@pytest.mark.parametrize("regime", ["random", "q8_random"])
@pytest.mark.parametrize("shape", BLEND_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_moving_statistics_blend_with_the_decay(shape, regime, monkeypatch):
    """From (0, 1): moving = 0.999 (0, 1) + 0.001 (batch mean, unbiased batch variance), compared after the blend as
    tests/test_gpu_netvlad_bounds.py does; the batch statistics themselves are held to the rule above from zeros."""
    dev = cuda()
    B, MF, F, S = shape
    seed = seeds_of(shape, regime)[0]
    results = []
    for form in forms_of(F):
        inputs, p64, _, _, _, _ = reference(shape, seed, regime, form != "gather", True)
        got = run_form(form, shape, inputs, dev, True, None, monkeypatch, start=(torch.zeros(F), torch.ones(F)))
        mm, mv = (m.double().cpu() for m in got["moving"])
        e_mean = float((mm - R.ONE_MINUS_DECAY * p64["batch_mean"]).abs().max() / (R.ONE_MINUS_DECAY * p64["batch_mean"].abs().max()))
        e_var = float((mv - (R.DECAY + R.ONE_MINUS_DECAY * p64["batch_var"])).abs().max())
        print(f"[frame_prep] {form} {shape} {regime} blend from (0, 1): moving_mean {e_mean:.3e}, moving_variance {e_var:.3e}")
        results.append((form, e_mean, e_var))
    for form, e_mean, e_var in results:
        assert e_mean <= 1e-4 and e_var <= 1e-5, form


# ---- the two normalisation ops on their own ----
ALL_SHAPES = REGIME_SHAPES + OTHER_SHAPES


def _frames_figure(got, ref, B):
    """[B, MF, F]: the larger of the per-clip and the per-frame figure; a frame that is zero in fp64 (padding) must be exactly zero."""
    rows = ref.shape[0] * ref.shape[1]
    return max(R.figure(got, ref, "out", B), R.figure(got, ref, "out", rows))


def _check_frames(tag, got, ref64, ref32, B):
    e32 = _frames_figure(ref32, ref64, B)
    e_op = _frames_figure(got, ref64, B)
    bound = max(8 * e32, 1e-6)
    print(f"[frame_prep] {tag}: op {e_op:.3e}, err32 {e32:.3e}, bound {bound:.3e}, ratio {e_op / bound:.3f}")
    assert e32 > 0, f"{tag}: err32 is zero"
    assert math.isfinite(e_op) and e_op <= bound, f"{tag}: op error {e_op:.3e} > max(8 x {e32:.3e}, 1e-6)"


@pytest.mark.parametrize("regime", R.Q8_REGIMES)
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dequantize_l2_normalize_meets_the_bound(shape, regime, entries):
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    B, MF, F, S = shape
    inputs = reference(shape, seeds_of(shape, regime)[0], regime, True, True)[0]
    ref64, ref32 = (R.dequantize_l2_normalize(inputs["q"], inputs["nf"], dt) for dt in (torch.float64, torch.float32))
    got = ops.dequantize_l2_normalize(inputs["q"].to(dev), inputs["nf"].to(dev))
    torch.cuda.synchronize()
    _check_frames(f"dequantize_l2_normalize {shape} {regime}", got, ref64, ref32, B)
    assert entries == ["lpm_dequantize_l2_normalize"]


@pytest.mark.parametrize("regime", ["random", "offset30", "column_spread"])
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_l2_normalize_rows_meets_the_bound(shape, regime, entries):
    """... with one frame of zeros (it stays zero) and one frame far below the 1e-12 clamp of the squared norm (it leaves times 1e6)."""
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    B, MF, F, S = shape
    seed = seeds_of(shape, "random")[0]
    x = R.make_inputs(B, MF, F, S, seed, regime)["frames"].clone()
    x[0, 1] = 0
    x[0, 2] = x[0, 2] * 1e-12
    ref64, ref32 = (R.l2_normalize_rows(x.to(dt)) for dt in (torch.float64, torch.float32))
    assert float(ref64[0, 1].abs().max()) == 0 and float((x[0, 2].double() ** 2).sum()) < 1e-14 and float(ref64[0, 2].abs().max()) > 0
    got = ops.l2_normalize_rows(x.to(dev))
    torch.cuda.synchronize()
    _check_frames(f"l2_normalize_rows {shape} {regime}", got, ref64, ref32, B)
    assert entries == ["lpm_l2_normalize_rows"]
