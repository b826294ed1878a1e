"""-m gpu: ops.netvlad / ops.vlad_aggregate (K1 assignment GEMM + cluster_bn, K2 aggregation, K3 backward; storage="f32") against the fp64
restatement of tests/_netvlad_ref.py -- never against the op itself -- per named part and per clip.

Rule (tests/test_gpu_triangulation.py): the restatement evaluated in fp32 on the CPU carries an error err32 against fp64; in "bf16x3" mode
the fp64 restatement with the split-operand product mm3 (every matrix-product operand rounded to bf16 hi + bf16 lo, lo x lo dropped)
carries errx3.  The op's error must be at most max(8 err32, 1e-6) with VLAD_PRECISION = ASSIGN_PRECISION = "f32" and at most
max(8 (err32 + errx3), 1e-6) with "bf16x3".  The error figure of a part with a clip axis (out, dx, dsims) is the maximum over the clips of
(max |error| in the clip / max |fp64 value| in the clip), of the others the maximum over the tensor; clip b's upstream gradient is N(0, 1)
times 10^(6 b / (B - 1) - 3), so an error confined to the clip with the small gradient shows.  A part that is identically zero in fp64 must
be exactly zero.  The moving statistics start from zero: what the op leaves is 0.001 x (batch mean, unbiased batch variance) -- precisely
(1 - fp32(0.999)) x, see tests/_netvlad_ref.ONE_MINUS_DECAY -- and is held to the same rule; a second call from (0, 1) keeps the decay
covered.  Every figure is printed before anything is asserted.

The route is asserted: the entry names that pass through _capi._Lib.check are recorded, and the tracked ones (TRACKED) must be exactly
the case's list -- the operand splits (lpm_split_rows_tiles, lpm_split_weight_tiles, lpm_split_frames) and lpm_assign_tiles (batch-norm
affine + softmax -> assignment tiles) among them, so the fused-softmax route is the one WITHOUT an lpm_assign_tiles launch
(ops._assign_gemm_dx_operands has no entry of its own: its two splits behind K3's first half are looked for where the frames want a
gradient, and must be absent where they do not).  With "f32" every case takes F32_ROUTE (less what its form does not have).  Cases whose switches exist only on the
split-bf16 path (lazy, fused, clip-wide, ...) run in "bf16x3" alone.

case                 (B, T, D, K)        form / switches                           entries reached with "bf16x3" (lpm_ prefix dropped)
one_frame            (4, 1, 128, 32)     training, one frame per clip              assign_gemm_tiles_fwd, vlad_aggregate_tiles_fwd, vlad_finalize_fwd, K3 tiles
k16                  (3, 9, 128, 16)     training                                  assign_gemm_fwd (fp32 K1), vlad_aggregate_tiles_fwd, vlad_aggregate_bwd
k64                  (2, 37, 128, 64)    training                                  K1 tiles, vlad_aggregate_tiles_fwd (register streaming), K3 tiles
k64_kmajor           (2, 37, 128, 64)    kmajor                                    as k64, k-major store
k64_eval             (2, 37, 128, 64)    eval mode                                 as k64 without bn_fold / bn_bwd
k64_bias             (2, 37, 128, 64)    cluster_biases branch                     as k64 without bn_fold / bn_bwd
k64_light            (2, 37, 128, 64)    LightVLAD                                 as k64
k128                 (2, 33, 128, 128)   training                                  vlad_aggregate_tiles3_fwd (LDS shared) + vlad_finalize2_fwd (raw nrm), K3 tiles
k128_kmajor_eval     (2, 33, 128, 128)   kmajor, eval mode                         as k128, k-major store, no bn_fold / bn_bwd
k128_fused           (2, 33, 128, 128)   VLAD_FUSED                                vlad_aggregate_fused_fwd
k128_fused_fallback  (2, 33, 128, 128)   VLAD_FUSED + VLAD_FUSED_DEBUG_FALLBACK    vlad_aggregate_fused_fwd (every clip through the follow-up pass)
k128_lazy            (2, 33, 128, 128)   kmajor lazy input_affine                  vlad_aggregate_raw_kmajor_fwd, vlad_row_scales, input_bn_grads
k128_affine          (2, 33, 128, 128)   input_affine (d-major, not lazy)          vlad_aggregate_tiles3_fwd, vlad_finalize2_fwd, input_bn_grads
k128_lazy_scaled     (2, 33, 128, 128)   lazy + VLAD_KMAJOR_SCALED                 vlad_aggregate_kmajor_scaled_fwd
k128_lazy_smx        (2, 33, 128, 128)   lazy + VLAD_SOFTMAX_FUSED                 vlad_aggregate_raw_kmajor_smx_fwd, vlad_row_scales, no assign_tiles
k256_lazy_clip       (2, 33, 256, 256)   lazy, VLAD_CLIP on                        vlad_aggregate_clip_kmajor_fwd (clip-wide), vlad_row_scales
k256_lazy_noclip     (2, 33, 256, 256)   lazy, VLAD_CLIP off                       vlad_aggregate_raw_kmajor_fwd
k256_lazy_scaled     (2, 33, 256, 256)   lazy + VLAD_KMAJOR_SCALED                 vlad_aggregate_kmajor_scaled_fwd (wide workgroups)
k256                 (2, 33, 256, 256)   training                                  vlad_aggregate_tiles3_fwd at K = 256
straddle             (5, 129, 128, 256)  training                                  K1's 64-row tile form at K = 256 (D = 128 is below the flat form's depth), T past four row tiles
flat_straddle        (5, 129, 256, 256)  training                                  K1's flat 96-row workgroups (csrc/assign_flat.hip: K = 256, D = 256), seven of them over 645 rows,
                                                                                   straddling the clips; the k256* cases reach the same form with one workgroup (66 rows)
walk                 (2, 300, 128, 128)  training                                  the whole frame walk
video                (1, 16, 1024, 128)  training                                  the video width
agg_k64              (2, 37, 128, 64)    vlad_aggregate                            vlad_aggregate_tiles_fwd, K3 tiles, no K1
agg_k128_kmajor      (2, 33, 128, 128)   vlad_aggregate kmajor                     vlad_aggregate_tiles3_fwd + finalize2
agg_k16              (3, 9, 128, 16)     vlad_aggregate                            vlad_aggregate_tiles_fwd, vlad_aggregate_bwd
agg_lazy_clip        (2, 33, 256, 256)   vlad_aggregate lazy, VLAD_CLIP on         vlad_aggregate_clip_dmajor_fwd, vlad_row_scales
agg_lazy_noclip      (2, 33, 256, 256)   vlad_aggregate lazy, VLAD_CLIP off        vlad_aggregate_tiles3_fwd, vlad_row_scales
Which kernel an entry point launches (K1: flat / 64-row / 128-row workgroups) cannot be told from its name: the table says what the
selection code in csrc/tile_gemm.hip (lpm_assign_gemm_tiles_fwd) and csrc/assign_flat.hip (assign_flat_ok) gives for the shape.  K1's 128-row
tile form is not reached: wherever it qualifies (K = 256, D >= 256) the flat form goes first.
Not reachable with both precisions equal and storage "f32": lpm_assign_gemm_tiles_bwd_dx on its own (K1 tiles with the fp32 K3), and the
addmm_ of the reverse mix.
Seeds: SEEDS below, condition values beside each.  Regimes (random, saturated, near_centre, small_mass): k64 and k128, both precisions, three
seeds each.

Shapes and regimes as they had to be set:
* one frame: K2 and K3 take D in {128, 256, 512, 1024}, so the case is (4, 1, 128, 32) -- and with T = 1 the descriptor does not depend on the
  assignment, dW / dgamma / dbeta are zero up to rounding (fp64: 1e-12 or less beside dx at 3e2): they are held to the same rule on the
  ABSOLUTE error, max |op - fp64| <= 8 max |fp32 - fp64| (+ max |mm3 - fp64| with "bf16x3"), which anything leaking out of the padded rows
  of a tile into x^T dl or into the batch-norm backward would exceed.  A single-ROW batch (B = T = 1) is not
  a case: its fp64 batch variance is identically zero, the op forms sum x^2 / n - mean^2 from fp32 squares and leaves 0.001 x up to 9e-8 (l^2 up
  to 4.3; measured, in about half the columns) -- the extreme of the large-offset regime, which is left to the change of that form.
* small_mass: beta[k1] = -9, not -12 -- at -12 the column's squared norm is 1e-11 .. 2e-9 over these shapes and seeds, for most of them inside
  the band the conditions forbid; at -9 it is 4e-9 or more, and the column still holds less than 1e-5 of a clip's mass.
* saturated: no seed keeps every cluster column out of [1e-14, 1e-10] (gamma times 30 leaves most clusters of a clip without a frame, their
  squared norms spread over fifty decades); the band of that regime is a factor 2 either side of the clamp, see tests/_netvlad_ref.SATURATED_BAND.

Measured on the MI355X, worst error / bound over parts and seeds per case and precision (the part that gives it in brackets):
MEASURED-BEGIN
First run: every part of every case within its bound except batch_mean / batch_var, off by a constant 1.29e-5 in every case and both
precisions (ratio 4.6 .. 13 with "f32", 1.05 in one "bf16x3" case): the fp32 constant 1 - fp32(0.999) of the blend, now in the model
(tests/_netvlad_ref.ONE_MINUS_DECAY); no kernel changed.  With it:
case (regime)                  bf16x3 (part)          f32 (part)
one_frame                      0.13 (dgamma)          0.16 (dgamma)
k16                            0.17 (dgamma)          0.17 (dgamma)
k64                            0.12 (dW2)             0.17 (dbeta)
k64_kmajor                     0.12 (dbeta)           0.16 (batch_mean)
k64_eval                       0.13 (dW)              0.15 (dx)
k64_bias                       0.13 (out)             0.13 (out)
k64_light                      0.14 (dgamma)          0.16 (batch_mean)
k128                           0.13 (dx)              0.17 (dbeta)
k128_kmajor_eval               0.13 (dbeta)           0.12 (out)
k128_fused                     0.13 (dx)              -
k128_fused_fallback            0.13 (dx)              -
k128_lazy                      0.13 (d_in_gamma)      -
k128_affine                    0.14 (d_in_gamma)      -
k128_lazy_scaled               0.14 (d_in_gamma)      -
k128_lazy_smx                  0.13 (d_in_gamma)      -
k256_lazy_clip                 0.12 (dgamma)          -
k256_lazy_noclip               0.12 (dbeta)           -
k256_lazy_scaled               0.12 (dbeta)           -
k256                           0.14 (dbeta)           0.17 (dx)
straddle                       0.13 (dx)              0.13 (out)
flat_straddle                  0.12 (dbeta)           0.21 (dW)
walk                           0.14 (dbeta)           0.20 (dbeta)
video                          0.14 (dbeta)           0.55 (batch_var)
agg_k64                        0.22 (dcentres)        0.15 (dsims)
agg_k128_kmajor                0.21 (dcentres)        0.16 (dcentres)
agg_k16                        0.21 (dcentres)        0.12 (out)
agg_lazy_clip                  0.20 (dcentres)        -
agg_lazy_noclip                0.20 (dcentres)        -
k64 (saturated)                0.13 (dW2)             0.22 (dW2)
k64 (near_centre)              0.14 (dW)              0.16 (batch_mean)
k64 (small_mass)               0.14 (dgamma)          0.25 (out[:, :, 5])
k128 (saturated)               0.12 (out)             0.26 (dW2)
k128 (near_centre)             0.15 (dbeta)           0.23 (batch_var)
k128 (small_mass)              0.14 (out[:, :, 3])    0.25 (dgamma)
one_frame, the absolute rule (bf16x3 / f32): dW 0.11 / 0.10, dgamma 0.13 / 0.16, dbeta 0.12 / 0.10 -- max |op| 1.1e-2 / 1.5e-3, 2.7e-3 / 8e-5,
1.8e-3 / 6e-5 beside dx at 3e2: what the mm3 model and the fp32 evaluation give themselves
MEASURED-END"""
import functools
import math

import pytest
import torch

from tests import _netvlad_ref as R
from tests._util import cuda

pytestmark = pytest.mark.gpu

K1_TILES = ("split_rows_tiles", "split_weight_tiles", "assign_gemm_tiles_fwd")     # (the two splits again for dx's operands, see check_case)
K3_TILES = ("vlad_aggregate_bwd_tiles", "vlad_aggregate_bwd_tiles_dx")               # (the row tiles of x come from K1's forward)
K3_TILES_NO_DX = ("vlad_aggregate_bwd_tiles", "input_bn_grads")
K3_TILES_AGG = K3_TILES + ("split_rows_tiles",)                                      # (no K1 in front: K3 splits the rows of x itself)
BN = ("bn_fold", "bn_bwd")
DW = ("assign_gemm_tiles_bwd_dw",)                                                   # (its split_frames of dl is in every K2 route already)
X3 = ("split_frames", "assign_tiles")        # K2's split-bf16 operands: the frame tiles of x, batch-norm affine + softmax -> the assignment tiles
TILES = X3 + ("vlad_aggregate_tiles_fwd", "vlad_finalize_fwd")
TILES3 = X3 + ("vlad_aggregate_tiles3_fwd", "vlad_finalize2_fwd")
F32_ROUTE = ("assign_gemm_fwd", "vlad_aggregate_fwd", "vlad_finalize_fwd", "vlad_aggregate_bwd") + BN
TRACKED = {"lpm_" + n for n in (
    "split_rows_tiles", "split_weight_tiles", "split_frames", "assign_tiles",
    "assign_gemm_fwd", "assign_gemm_tiles_fwd", "bn_fold", "bn_bwd", "assign_gemm_tiles_bwd_dw", "assign_gemm_tiles_bwd_dx", "input_bn_grads",
    "vlad_aggregate_fwd", "vlad_aggregate_tiles_fwd", "vlad_aggregate_tiles3_fwd", "vlad_aggregate_fused_fwd", "vlad_aggregate_raw_kmajor_fwd",
    "vlad_aggregate_clip_kmajor_fwd", "vlad_aggregate_clip_dmajor_fwd", "vlad_aggregate_kmajor_scaled_fwd", "vlad_aggregate_raw_kmajor_smx_fwd",
    "vlad_finalize_fwd", "vlad_finalize2_fwd", "vlad_row_scales", "vlad_aggregate_bwd", "vlad_aggregate_bwd_tiles", "vlad_aggregate_bwd_tiles_dx")}

# every A/B switch of K2 is set for every case (a case's own ``switches`` on top): the routes do not depend on the environment
SWITCHES = dict(VLAD_TILES3=True, VLAD_FUSED=False, VLAD_FUSED_DEBUG_FALLBACK=False, VLAD_SOFTMAX_FUSED=False, VLAD_KMAJOR_SCALED=False,
                VLAD_CLIP=True)
BOTH = ("bf16x3", "f32")
ONLY_X3 = ("bf16x3",)
LAZY = dict(kmajor=True, lazy=True)


def _case(shape, form="netvlad", opts=None, switches=None, precisions=BOTH, route=(), rounding_only=()):
    """rounding_only: parts that are mathematically zero without being identically zero in fp64 (their fp64 value is rounding noise, a
    relative figure means nothing): held to the same rule on the ABSOLUTE error -- max |op - fp64| <= 8 max |fp32 - fp64| with "f32",
    <= 8 (max |fp32 - fp64| + max |mm3 - fp64|) with "bf16x3"."""
    return dict(shape=shape, form=form, opts=opts or {}, switches=switches or {}, precisions=precisions, route=tuple(route),
                rounding_only=tuple(rounding_only))


CASES = {
    # T = 1: V[b, :, k] = a_k (x - c_k), and the normalisation over d removes a_k -- the descriptor does not depend on the assignment, so the
    # gradients of W, gamma and beta are zero up to rounding (fp64: 1e-16 of the other parts)
    "one_frame": _case((4, 1, 128, 32), route=K1_TILES + TILES + K3_TILES + BN + DW, rounding_only=("dW", "dgamma", "dbeta")),
    "k16": _case((3, 9, 128, 16), route=("assign_gemm_fwd",) + TILES + ("vlad_aggregate_bwd",) + BN),
    "k64": _case((2, 37, 128, 64), route=K1_TILES + TILES + K3_TILES + BN + DW),
    "k64_kmajor": _case((2, 37, 128, 64), opts=dict(kmajor=True), route=K1_TILES + TILES + K3_TILES + BN + DW),
    "k64_eval": _case((2, 37, 128, 64), opts=dict(training=False), route=K1_TILES + TILES + K3_TILES + DW),
    "k64_bias": _case((2, 37, 128, 64), form="bias", route=K1_TILES + TILES + K3_TILES + DW),
    "k64_light": _case((2, 37, 128, 64), form="light", route=K1_TILES + TILES + K3_TILES + BN + DW),
    "k128": _case((2, 33, 128, 128), route=K1_TILES + TILES3 + K3_TILES + BN + DW),
    "k128_kmajor_eval": _case((2, 33, 128, 128), opts=dict(kmajor=True, training=False), route=K1_TILES + TILES3 + K3_TILES + DW),
    "k128_fused": _case((2, 33, 128, 128), switches=dict(VLAD_FUSED=True), precisions=ONLY_X3,
                        route=K1_TILES + X3 + ("vlad_aggregate_fused_fwd",) + K3_TILES + BN + DW),
    "k128_fused_fallback": _case((2, 33, 128, 128), switches=dict(VLAD_FUSED=True, VLAD_FUSED_DEBUG_FALLBACK=True), precisions=ONLY_X3,
                                 route=K1_TILES + X3 + ("vlad_aggregate_fused_fwd",) + K3_TILES + BN + DW),
    "k128_lazy": _case((2, 33, 128, 128), form="input_affine", opts=LAZY, precisions=ONLY_X3,
                       route=K1_TILES + X3 + ("vlad_aggregate_raw_kmajor_fwd", "vlad_row_scales") + K3_TILES_NO_DX + BN + DW),
    "k128_affine": _case((2, 33, 128, 128), form="input_affine", precisions=ONLY_X3, route=K1_TILES + TILES3 + K3_TILES_NO_DX + BN + DW),
    "k128_lazy_scaled": _case((2, 33, 128, 128), form="input_affine", opts=LAZY, switches=dict(VLAD_KMAJOR_SCALED=True), precisions=ONLY_X3,
                              route=K1_TILES + X3 + ("vlad_aggregate_kmajor_scaled_fwd",) + K3_TILES_NO_DX + BN + DW),
    "k128_lazy_smx": _case((2, 33, 128, 128), form="input_affine", opts=LAZY, switches=dict(VLAD_SOFTMAX_FUSED=True), precisions=ONLY_X3,
                           route=K1_TILES + ("split_frames", "vlad_aggregate_raw_kmajor_smx_fwd", "vlad_row_scales") + K3_TILES_NO_DX + BN + DW),
    "k256_lazy_clip": _case((2, 33, 256, 256), form="input_affine", opts=LAZY, switches=dict(VLAD_CLIP=True), precisions=ONLY_X3,
                            route=K1_TILES + X3 + ("vlad_aggregate_clip_kmajor_fwd", "vlad_row_scales") + K3_TILES_NO_DX + BN + DW),
    "k256_lazy_noclip": _case((2, 33, 256, 256), form="input_affine", opts=LAZY, switches=dict(VLAD_CLIP=False), precisions=ONLY_X3,
                              route=K1_TILES + X3 + ("vlad_aggregate_raw_kmajor_fwd", "vlad_row_scales") + K3_TILES_NO_DX + BN + DW),
    "k256_lazy_scaled": _case((2, 33, 256, 256), form="input_affine", opts=LAZY, switches=dict(VLAD_KMAJOR_SCALED=True), precisions=ONLY_X3,
                              route=K1_TILES + X3 + ("vlad_aggregate_kmajor_scaled_fwd",) + K3_TILES_NO_DX + BN + DW),
    "k256": _case((2, 33, 256, 256), route=K1_TILES + TILES3 + K3_TILES + BN + DW),
    "straddle": _case((5, 129, 128, 256), route=K1_TILES + TILES3 + K3_TILES + BN + DW),
    "flat_straddle": _case((5, 129, 256, 256), route=K1_TILES + TILES3 + K3_TILES + BN + DW),
    "walk": _case((2, 300, 128, 128), route=K1_TILES + TILES3 + K3_TILES + BN + DW),
    "video": _case((1, 16, 1024, 128), route=K1_TILES + TILES3 + K3_TILES + BN + DW),
    "agg_k64": _case((2, 37, 128, 64), form="aggregate", route=TILES + K3_TILES_AGG),
    "agg_k128_kmajor": _case((2, 33, 128, 128), form="aggregate", opts=dict(kmajor=True), route=TILES3 + K3_TILES_AGG),
    "agg_k16": _case((3, 9, 128, 16), form="aggregate", route=TILES + ("vlad_aggregate_bwd",)),
    "agg_lazy_clip": _case((2, 33, 256, 256), form="aggregate", opts=dict(lazy=True), switches=dict(VLAD_CLIP=True), precisions=ONLY_X3,
                           route=X3 + ("vlad_aggregate_clip_dmajor_fwd", "vlad_row_scales") + K3_TILES_AGG),
    "agg_lazy_noclip": _case((2, 33, 256, 256), form="aggregate", opts=dict(lazy=True), switches=dict(VLAD_CLIP=False), precisions=ONLY_X3,
                             route=X3 + ("vlad_aggregate_tiles3_fwd", "vlad_row_scales") + K3_TILES_AGG),
}
REGIME_CASES = ("k64", "k128")

# per case (or (case, regime)): the seeds, and beside them the condition values of tests/_netvlad_ref.conditions per seed --
# min squared column norm above the clamp band, max below it, min over clips of max |dx| (- without dx), min err32 over the parts
SEEDS = {
    # SEEDS-BEGIN
    "one_frame": (0,),                                        # 2.0e-04, 0.0e+00, 3.1e-04, 2.0e-07
    "k16": (0,),                                              # 1.3e+00, 0.0e+00, 5.2e+00, 1.1e-07
    "k64": (0, 1, 2),                                         # 5.2e-01, 0.0e+00, 2.8e+00, 1.9e-07; 3.0e-01, 0.0e+00, 5.1e+00, 1.7e-07; 4.4e-01, 0.0e+00, 4.5e+00, 2.1e-07
    "k64_kmajor": (0,),                                       # 5.2e-01, 0.0e+00, 2.8e+00, 1.9e-07
    "k64_eval": (0,),                                         # 3.8e-01, 0.0e+00, 6.0e-05, 2.5e-07
    "k64_bias": (0,),                                         # 5.2e-03, 0.0e+00, 7.4e-05, 2.7e-07
    "k64_light": (0,),                                        # 3.7e-01, 0.0e+00, 3.0e+00, 1.9e-07
    "k128": (0, 1, 2),                                        # 5.7e-02, 0.0e+00, 4.1e+00, 2.2e-07; 6.2e-02, 0.0e+00, 3.6e+00, 2.2e-07; 4.2e-02, 0.0e+00, 3.3e+00, 1.9e-07
    "k128_kmajor_eval": (0,),                                 # 6.1e-02, 0.0e+00, 6.5e-05, 2.7e-07
    "k128_fused": (0,),                                       # 5.7e-02, 0.0e+00, 4.1e+00, 2.2e-07
    "k128_fused_fallback": (0,),                              # 5.7e-02, 0.0e+00, 4.1e+00, 2.2e-07
    "k128_lazy": (0,),                                        # 8.6e-02, 0.0e+00, -, 1.5e-07
    "k128_affine": (0,),                                      # 8.6e-02, 0.0e+00, -, 1.5e-07
    "k128_lazy_scaled": (0,),                                 # 8.6e-02, 0.0e+00, -, 1.5e-07
    "k128_lazy_smx": (0,),                                    # 8.6e-02, 0.0e+00, -, 1.5e-07
    "k256_lazy_clip": (0,),                                   # 4.6e-02, 0.0e+00, -, 2.1e-07
    "k256_lazy_noclip": (0,),                                 # 4.6e-02, 0.0e+00, -, 2.1e-07
    "k256_lazy_scaled": (0,),                                 # 4.6e-02, 0.0e+00, -, 2.1e-07
    "k256": (0,),                                             # 2.2e-02, 0.0e+00, 3.0e+00, 2.7e-07
    "straddle": (0,),                                         # 6.0e-02, 0.0e+00, 3.4e-01, 2.1e-07
    "flat_straddle": (0,),                                    # 7.6e-02, 0.0e+00, 2.9e-01, 1.6e-07
    "walk": (0,),                                             # 1.1e+00, 0.0e+00, 4.4e-01, 1.7e-07
    "video": (0,),                                            # 2.1e-01, 0.0e+00, 4.0e-02, 3.3e-07
    "agg_k64": (0,),                                          # 2.4e+03, 0.0e+00, 6.3e-05, 2.7e-07
    "agg_k128_kmajor": (0,),                                  # 1.6e+03, 0.0e+00, 6.8e-05, 1.8e-07
    "agg_k16": (0,),                                          # 2.9e+02, 0.0e+00, 1.2e-04, 1.6e-07
    "agg_lazy_clip": (0,),                                    # 3.2e+03, 0.0e+00, 4.8e-05, 1.7e-07
    "agg_lazy_noclip": (0,),                                  # 3.2e+03, 0.0e+00, 4.8e-05, 1.7e-07
    ("k64", "saturated"): (0, 4, 6),                          # 3.4e-12, 3.2e-13, 5.4e+01, 1.9e-07; 3.9e-12, 1.0e-13, 5.6e+01, 1.4e-07; 2.9e-12, 1.0e-13, 6.0e+01, 1.8e-07
    ("k64", "near_centre"): (0, 1, 2),                        # 1.1e-01, 0.0e+00, 1.1e+01, 1.1e-07; 5.8e-02, 0.0e+00, 1.0e+01, 8.9e-08; 1.0e-01, 0.0e+00, 1.3e+01, 8.1e-08
    ("k64", "small_mass"): (0, 1, 2),                         # 2.0e-08, 6.5e-18, 2.7e+00, 1.9e-07; 3.6e-08, 3.6e-17, 5.0e+00, 1.9e-07; 3.6e-07, 6.6e-18, 4.4e+00, 2.2e-07
    ("k128", "saturated"): (0, 21, 27),                       # 2.1e-12, 1.9e-13, 3.8e+01, 2.2e-07; 5.8e-12, 4.6e-13, 1.4e+02, 2.0e-07; 4.4e-12, 2.9e-13, 1.0e+02, 2.3e-07
    ("k128", "near_centre"): (0, 1, 2),                       # 6.3e-03, 0.0e+00, 1.4e+01, 5.5e-08; 1.0e-02, 0.0e+00, 1.2e+01, 9.4e-08; 1.3e-02, 0.0e+00, 1.6e+01, 9.0e-08
    ("k128", "small_mass"): (0, 1, 2),                        # 8.0e-09, 8.1e-19, 4.0e+00, 2.2e-07; 2.9e-08, 1.6e-18, 3.6e+00, 2.2e-07; 3.8e-09, 3.2e-18, 3.3e+00, 1.9e-07
    # SEEDS-END
}


def route_of(name, precision):
    """The tracked entry names (with the lpm_ prefix) the case must reach, and no others."""
    case = CASES[name]
    if precision == "bf16x3":
        names = case["route"]
    elif case["form"] == "aggregate":
        names = ("vlad_aggregate_fwd", "vlad_finalize_fwd", "vlad_aggregate_bwd")
    elif case["form"] == "bias" or not case["opts"].get("training", True):
        names = tuple(n for n in F32_ROUTE if n not in BN)
    else:
        names = F32_ROUTE
    return {"lpm_" + n for n in names}


def seeds_of(name, regime="random"):
    return SEEDS[name if regime == "random" else (name, regime)]


@functools.lru_cache(maxsize=None)
def reference(name, seed, regime="random"):
    """-> (inputs, fp64 parts, fp32 parts, mm3 parts, (ok, condition values)), computed once per (case, seed, regime) on the CPU."""
    case = CASES[name]
    B, T, D, K = case["shape"]
    kw = dict(form=case["form"], training=case["opts"].get("training", True))
    inputs = R.make_inputs(B, T, D, K, seed, regime)
    p64 = R.values_and_grads(inputs, T, torch.float64, **kw)
    p32 = R.values_and_grads(inputs, T, torch.float32, **kw)
    px3 = R.values_and_grads(inputs, T, torch.float64, mm=R.mm3, **kw)
    return inputs, p64, p32, px3, R.conditions(inputs, T, p64, p32, regime=regime, **kw)


def bounds(name, seed, regime="random"):
    """-> {part: (err32, errx3, f32 bound, bf16x3 bound)}; for the small-mass regime also the two cluster columns of ``out``."""
    inputs, p64, p32, px3, _ = reference(name, seed, regime)
    B, _, _, K = CASES[name]["shape"]
    absolute = CASES[name]["rounding_only"]
    figs = {n: (R.figure(p32[n], p64[n], n, B), R.figure(px3[n], p64[n], n, B)) for n in p64 if n not in absolute}
    if regime == "small_mass":
        for k in (R.SMALL_MASS_K1, R.SMALL_MASS_K2):
            figs[f"out[:, :, {k}]"] = (R.column_figure(p32["out"], p64["out"], B, K, k), R.column_figure(px3["out"], p64["out"], B, K, k))
    bnd = {n: (e32, ex3, max(8 * e32, 1e-6), max(8 * (e32 + ex3), 1e-6)) for n, (e32, ex3) in figs.items()}
    for n in absolute:                                     # absolute errors, no relative floor
        e32, ex3 = absolute_error(p32[n], p64[n]), absolute_error(px3[n], p64[n])
        bnd[n] = (e32, ex3, 8 * e32, 8 * (e32 + ex3))
    return bnd


def absolute_error(got, ref):
    return float((got.detach().double().cpu().reshape(ref.shape) - ref.detach().double().cpu()).abs().max())


@pytest.fixture
def precision(request):
    """As tests/test_gpu_kernels.vlad_precision: the matrix-core arithmetic of K1 / K2 / K3, given by indirect parametrisation."""
    from learnablepoolingmethods_amd import ops
    old = ops.VLAD_PRECISION, ops.ASSIGN_PRECISION
    ops.VLAD_PRECISION = ops.ASSIGN_PRECISION = request.param
    yield request.param
    ops.VLAD_PRECISION, ops.ASSIGN_PRECISION = old


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


def run_op(name, inputs, dev, monkeypatch, moving=None):
    """One forward + backward of the op as the case describes it -> {part: tensor} in the restatement's layout (d-major), with
    moving_mean / moving_var as the op left them (training-mode batch norm; started from ``moving``, default zeros)."""
    from learnablepoolingmethods_amd import ops
    case = CASES[name]
    B, T, D, K = case["shape"]
    form, opts = case["form"], case["opts"]
    kmajor, lazy, training = opts.get("kmajor", False), opts.get("lazy", False), opts.get("training", True)
    for switch, value in {**SWITCHES, **case["switches"]}.items():
        assert hasattr(ops, switch)
        monkeypatch.setattr(ops, switch, value)            # (restored when the test ends)

    def g(key, grad=True):
        return inputs[key].to(dev).requires_grad_(grad)
    up = inputs["upstream"]
    up = (up.reshape(B, D, K).transpose(1, 2).contiguous() if kmajor else up).to(dev)
    parts = {}
    if form == "aggregate":
        leaves = dict(dsims=g("sims"), dx=g("x"), dcentres=g("W2"))
        out = ops.vlad_aggregate(leaves["dsims"], leaves["dx"], leaves["dcentres"][0], T, kmajor=kmajor, lazy=lazy)
    else:
        leaves = dict(dW=g("W"))
        affine = None
        if form == "input_affine":
            leaves.update(d_in_gamma=g("in_gamma"), d_in_beta=g("in_beta"))
            x64 = R.input_bn(inputs["frames"].double(), inputs["in_gamma"].double(), inputs["in_beta"].double(), training=True)[0]
            x = x64.float().to(dev)                       # input_bn's output: data for the op, which returns input_bn's gradients itself
            affine = (leaves["d_in_gamma"], leaves["d_in_beta"])
        else:
            x = leaves["dx"] = g("x")
        bn = bias = None
        if form == "bias":
            bias = leaves["dbias"] = g("bias")
        else:
            leaves.update(dgamma=g("gamma"), dbeta=g("beta"))
            if training:
                mm, mv = (torch.zeros(K), torch.zeros(K)) if moving is None else moving
            else:
                mm, mv = inputs["moving"]
            parts["moving"] = (mm.clone().to(dev), mv.clone().to(dev))
            bn = (leaves["dgamma"], leaves["dbeta"]) + parts["moving"]
        W2 = None if form == "light" else leaves.setdefault("dW2", g("W2"))
        out = ops.netvlad(x, leaves["dW"], W2, T, bn=bn, bias=bias, is_training=training, kmajor=kmajor, input_affine=affine, lazy=lazy)
    if lazy:
        assert ops.row_scale_of(out) is not None
        out = ops.materialise(out)
    assert out.shape == ((B, K, D) if kmajor else (B, D * K))
    names = list(leaves)
    grads = torch.autograd.grad((out * up).sum(), [leaves[n] for n in names])
    torch.cuda.synchronize()
    parts["out"] = out.detach().reshape(B, K, D).transpose(1, 2).reshape(B, D * K) if kmajor else out.detach()
    parts.update(zip(names, grads))
    return parts


def check_case(name, seed, regime, prec, dev, monkeypatch, entries):
    """Figures, bounds and ratios of every part: printed, then asserted.  -> the worst ratio."""
    B, _, _, K = CASES[name]["shape"]
    inputs, p64, _, _, (ok, cond) = reference(name, seed, regime)
    tag = f"{name} {regime} seed {seed} {prec}"
    print(f"[netvlad] {tag}: conditions {ok} " + ", ".join(f"{v:.2e}" for v in cond))
    assert ok, f"{tag}: the seed does not meet the conditions {cond}"
    bnd = bounds(name, seed, regime)
    del entries[:]
    got = run_op(name, inputs, dev, monkeypatch)
    reached = set(entries) & TRACKED
    if "batch_mean" in p64:                               # from zero moving statistics: (1 - fp32(0.999)) x the batch statistics
        got["batch_mean"], got["batch_var"] = (m / R.ONE_MINUS_DECAY for m in got["moving"])
    rows = []
    for n, (e32, ex3, b32, bx3) in bnd.items():
        if n.startswith("out["):
            e_op = R.column_figure(got["out"], p64["out"], B, K, int(n[len("out[:, :, "):-1]))
        elif n in CASES[name]["rounding_only"]:
            e_op = absolute_error(got[n], p64[n])
        else:
            e_op = R.figure(got[n], p64[n], n, B)
        bound = b32 if prec == "f32" else bx3
        zero = float(p64[n.split("[")[0]].abs().max()) == 0.0
        note = " (identically zero in fp64)" if zero else ""
        if n in CASES[name]["rounding_only"]:
            note = f" (absolute: zero up to rounding, max |op| {float(got[n].abs().max()):.3e}, max |fp64| {float(p64[n].abs().max()):.3e})"
        rows.append((n, e_op, e32, ex3, bound, zero))
        print(f"[netvlad] {tag} {n}: op {e_op:.3e}, err32 {e32:.3e}, errx3 {ex3:.3e}, bound {bound:.3e}, ratio {e_op / bound:.3f}"
              + note)
    print(f"[netvlad] {tag} route: {sorted(reached)}")
    assert reached == route_of(name, prec), f"{tag}: reached {sorted(reached)}, expected {sorted(route_of(name, prec))}"
    if "lpm_assign_gemm_tiles_fwd" in reached and "lpm_vlad_aggregate_bwd_tiles" in reached:
        # ops._assign_gemm_dx_operands (row tiles of dl, transposed weight tiles, split behind K3's first half) runs exactly when the frames
        # want a gradient
        behind_k3 = entries[entries.index("lpm_vlad_aggregate_bwd_tiles"):]
        for split in ("lpm_split_weight_tiles", "lpm_split_rows_tiles"):
            assert (split in behind_k3) == ("dx" in p64), f"{tag}: {behind_k3}"
    for n, e_op, e32, ex3, bound, zero in rows:
        if zero:
            assert e_op == 0.0, f"{tag} {n}: identically zero in fp64, not exactly zero in the op"
        else:
            assert math.isfinite(e_op) and e_op <= bound, f"{tag} {n}: op error {e_op:.3e} > bound {bound:.3e} (err32 {e32:.3e}, errx3 {ex3:.3e})"
    worst = max(e_op / bound for _, e_op, _, _, bound, zero in rows if not zero)
    print(f"[netvlad] {tag} worst ratio {worst:.3f}")
    return worst


def _params():
    return [pytest.param(name, prec, id=f"{name}-{prec}") for name, case in CASES.items() for prec in case["precisions"]]


@pytest.mark.parametrize("name,precision", _params(), indirect=["precision"])
def test_op_meets_the_bound_on_every_route(name, precision, monkeypatch, entries):
    dev = cuda()
    for seed in seeds_of(name):
        check_case(name, seed, "random", precision, dev, monkeypatch, entries)


@pytest.mark.parametrize("precision", BOTH, indirect=True)
@pytest.mark.parametrize("regime", R.REGIMES[1:])
@pytest.mark.parametrize("name", REGIME_CASES)
def test_op_meets_the_bound_in_every_regime(name, regime, precision, monkeypatch, entries):
    dev = cuda()
    for seed in seeds_of(name, regime):
        check_case(name, seed, regime, precision, dev, monkeypatch, entries)


@pytest.mark.parametrize("precision", BOTH, indirect=True)
@pytest.mark.parametrize("name", REGIME_CASES)
def test_moving_statistics_blend_with_the_decay(name, precision, monkeypatch):
    """From (0, 1): moving = 0.999 (0, 1) + 0.001 (batch mean, unbiased batch variance), compared after the blend as
    tests/test_gpu_kernels.test_netvlad_fwd_bwd does; the batch statistics themselves are held to the rule above from zeros."""
    dev = cuda()
    B, T, D, K = CASES[name]["shape"]
    seed = seeds_of(name)[0]
    inputs, p64, _, _, _ = reference(name, seed)
    got = run_op(name, inputs, dev, monkeypatch, moving=(torch.zeros(K), torch.ones(K)))
    mm, mv = (m.double().cpu() for m in got["moving"])
    e_mean = float((mm - R.ONE_MINUS_DECAY * p64["batch_mean"]).abs().max() / (R.ONE_MINUS_DECAY * p64["batch_mean"].abs().max()))
    e_var = float((mv - (R.DECAY + R.ONE_MINUS_DECAY * p64["batch_var"])).abs().max())
    print(f"[netvlad] {name} {precision} blend from (0, 1): moving_mean {e_mean:.3e}, moving_variance {e_var:.3e}")
    assert e_mean <= 1e-4 and e_var <= 1e-5
