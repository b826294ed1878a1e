"""-m gpu: ops.triangulation_magnitude_frames (csrc/triangulation_moments.hip, csrc/triangulation_bn_moments.hip), loupe_modules.NetVLAD,
TriangulationMagnitudeNsCnnNetVladModule on the GPU and JuhanTestModelV4 against the fp64 restatement on the CPU
(tests/_triangulation_v4_ref.py) -- never against the op itself or the module.

Tolerance of the op (the rule of tests/test_gpu_triangulation.py): the restatement evaluated in fp32 torch on the CPU carries an error
err32 against fp64 (maximum absolute error over the maximum absolute fp64 value); the op's error must be <= max(8 err32, 1e-6).  It is
taken per PART (spatial / temporal x convolution / norm / padding columns) and per gradient (dx, danchors, dcnn_s, dcnn_t, with N(0,1)
upstream gradients on both outputs, the padding columns included).  Every figure is printed before any is asserted.  The padding columns,
and any part whose fp64 reference is identically zero, must be exactly zero in the op.

Conditions, asserted on the fp64 restatement before any launch (V3's, with V3's thresholds): no squared norm, q or p, below 1e-6; no
convolution pre-activation of either stream below 1e-5 of its stream's largest magnitude (a mask flipped by rounding changes a gradient
entry by a whole upstream element), with at least 10 % of them negative.  The "frame == anchor" test is exempt from the first two: it is
about exactly that.  The frames, anchors and convolution weights of a (shape, seed) are tests/_triangulation_v3_ref.make_inputs' bit for
bit, so the seeds below are the ones tests/test_gpu_triangulation_v3.py found for the same shapes -- its conditions contain these --
checked again on the CPU for this file; a seed that fails one is replaced, never skipped, and no threshold is loosened.  SEEDS:
(B, T, D, K, F) or a test's name -> seeds, with the smallest squared norm, the smallest pre-activation ratio and the smaller share of
negative pre-activations measured for each.

loupe_modules.NetVLAD runs the project's split-bf16 NetVLAD forms: its bound is the one tests/test_gpu_netvlad_bounds.py:284 holds
ops.netvlad's output and gradients to in "bf16x3" mode, max(8 (err32 + errx3), 1e-6), errx3 being the error of the fp64 restatement with
the split-operand product tests/_netvlad_ref.mm3 in the two NetVLAD stages, and the figures tests/_netvlad_ref.figure's (per clip for
the output and the input gradient).  The module (fused_frames + head) is held to the same bound with errx3 taken of the whole module's
restatement, in the model-level figures below.  The model is held to the project's model-level bound, 1e-3
(tests/_util.REL_TOL), in the figures tests/test_gpu_models.py:155-175 takes: values (output, predictions, loss) in the maximum norm,
tests/_util.rel_err; every gradient in the Frobenius norm of its variable, tests/_util.rel_l2, over a floor of 1e-4 x the largest
gradient entry of the run x sqrt(numel) -- the beta of a batch norm that another batch norm follows has a gradient that is zero but for
rounding (1e-17 in fp64).  The fp32 CPU path's own error is printed beside each figure."""
import functools
import math

import pytest
import torch

from tests import _netvlad_ref as R
from tests import _triangulation_v4_ref as V
from tests._util import REL_TOL, cuda, rel_err, rel_l2

pytestmark = pytest.mark.gpu

NAMES = V.PARTS + V.GRADS

SEEDS = {
    # SEEDS-BEGIN
    (3, 2, 128, 1, 1): (0, 2, 7),                           # 1.0e+00, 5.8e-02, 0.33; 1.0e+00, 6.1e-02, 0.33; 1.0e+00, 1.1e-01, 0.33
    (2, 7, 128, 5, 3): (0, 2, 3),                           # 9.6e-01, 4.7e-04, 0.53; 9.7e-01, 4.3e-05, 0.41; 9.4e-01, 8.1e-04, 0.47
    (2, 30, 1024, 3, 33): (0, 1, 3),                        # 1.0e+00, 1.2e-05, 0.50; 1.0e+00, 2.3e-05, 0.50; 1.0e+00, 6.0e-05, 0.48
    (2, 33, 128, 8, 32): (3, 7, 8),                         # 9.2e-01, 2.5e-05, 0.49; 9.3e-01, 1.9e-05, 0.49; 9.3e-01, 3.8e-05, 0.50
    (5, 30, 128, 2, 4): (0, 1, 2),                          # 9.4e-01, 4.6e-05, 0.49; 8.9e-01, 4.3e-04, 0.51; 9.3e-01, 1.4e-04, 0.47
    (1, 320, 128, 2, 2): (14573, 32220, 34351),             # 9.1e-01, 9.0e-05, 0.53; 9.3e-01, 6.1e-05, 0.51; 8.9e-01, 1.6e-04, 0.52
    "frame == anchor": (0,),                                # 0, 0 (the clamped row), 0.48
    "module": (0,),                                         # (4, 7, 128, 5, 3): 9.6e-01, 1.5e-03, 0.45
    # (MODEL_SEED = 0: video 8.9e-01, 1.8e-03, 0.50; audio 1.4e-01, 7.6e-04, 0.27)
    # SEEDS-END
}

SHAPES = [  # B, T, D, K, F, pad_to
    (3, 2, 128, 1, 1, 1),                    # feat_t has one row per clip; K = 1: the roll wraps onto the same anchor; W = 2
    (2, 7, 128, 5, 3, 32),                   # everything odd; W = 20 -> 32
    (2, 30, 1024, 3, 33, 1),                 # video width; F one past a 32-filter tile; W = 102
    (2, 33, 128, 8, 32, 1),                  # T one past a 32-row tile
    (5, 30, 128, 2, 4, 32),                  # 150 rows: a 128-row tile spans clip boundaries and the temporal rows compact across them (145)
    (1, 320, 128, 2, 2, 1),                  # the largest T
]


def _err(a, ref):
    ref = ref.double()
    return float((a.detach().double().cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


def _named(outs, grads, K, F):
    return {**V.split_parts(*outs, K, F), **dict(zip(V.GRADS, grads))}


def _reference(x, anchors, cnn, up, T, pad_to):
    """fp64 and fp32 values / gradients of the restatement, split into the named parts, and the conditions."""
    ref = dict(cond=V.conditions(x, anchors, cnn, T))
    K, F = cnn[0].shape[0], cnn[0].shape[1]
    for key, dt in (("64", torch.float64), ("32", torch.float32)):
        outs, grads = V.features_and_grads(x.to(dt), anchors.to(dt), [c.to(dt) for c in cnn], T, up, pad_to)
        ref[key] = _named(outs, grads, K, F)
    return ref


@functools.lru_cache(maxsize=None)
def _random_case(B, T, D, K, F, pad_to, seed):
    x, anchors, cnn, up = V.make_inputs(B, T, D, K, F, seed, pad_to)
    return (x, anchors, cnn, up), _reference(x, anchors, cnn, up, T, pad_to)


def _condition(tag, ref, clamped=False):
    c = ref["cond"]
    print(f"[triangulation v4] {tag} smallest squared norm {c['smallest']:.3e}, smallest |pre-activation| / max {c['conv_ratio']:.3e}, "
          f"negative pre-activations {c['conv_negative']:.2f}")
    if not clamped:
        assert c["smallest"] >= 1e-6, f"{tag}: a squared norm of the restatement lies below 1e-6 ({c['smallest']:.3e})"
        assert c["conv_ratio"] >= 1e-5, f"{tag}: a pre-activation lies within 1e-5 of zero relative to its stream's largest ({c['conv_ratio']:.3e})"
    assert c["conv_negative"] >= 0.10, f"{tag}: only {c['conv_negative']:.2f} of a stream's pre-activations are negative"


def _run_op(inputs, T, dev, pad_to, up=None):
    from learnablepoolingmethods_amd import ops
    x, anchors, cnn, up0 = inputs
    up = up0 if up is None else up
    leaves = [t.to(dev).requires_grad_(True) for t in (x, anchors, *cnn)]
    feats = ops.triangulation_magnitude_frames(*leaves, T, pad_to=pad_to)
    loss = sum((o * g.to(dev)).sum() for o, g in zip(feats, up))
    grads = torch.autograd.grad(loss, leaves)
    return _named(feats, grads, cnn[0].shape[0], cnn[0].shape[1]), feats


def _check(tag, got, ref, names=NAMES, values_only=False):
    """Every figure is printed before anything is asserted.  -> the worst error-over-bound ratio."""
    rows = []
    for n in names:
        assert got[n].shape == ref["64"][n].shape, f"{tag} {n}: shape {tuple(got[n].shape)}, the restatement's {tuple(ref['64'][n].shape)}"
        if ref["64"][n].numel() == 0:                       # (the padding parts without padding)
            continue
        zero = float(ref["64"][n].abs().max()) == 0.0
        rows.append((n, zero, float(got[n].detach().abs().max()) if zero else _err(got[n], ref["64"][n]),
                     0.0 if zero else _err(ref["32"][n], ref["64"][n])))
    worst = 0.0
    for n, zero, e_op, e32 in rows:
        if zero:
            print(f"[triangulation v4] {tag} {n}: the fp64 reference is identically zero; max |op| {e_op:.3e}")
        else:
            worst = max(worst, e_op / max(8 * e32, 1e-6))
            print(f"[triangulation v4] {tag} {n}: op error {e_op:.3e}, fp32 evaluation error {e32:.3e}, bound {max(8 * e32, 1e-6):.3e}, "
                  f"ratio {e_op / max(8 * e32, 1e-6):.2f}")
    print(f"[triangulation v4] {tag} worst error over bound {worst:.2f}")
    for n, zero, e_op, e32 in rows:
        assert bool(torch.isfinite(got[n]).all()), f"{tag} {n}: not finite"
        if values_only and n in V.GRADS:
            continue
        if zero:
            assert e_op == 0.0, f"{tag} {n}: must be exactly zero, max |op| {e_op:.3e}"
        else:
            assert e_op <= max(8 * e32, 1e-6), f"{tag} {n}: op error {e_op:.3e} > max(8 x {e32:.3e}, 1e-6)"
    return worst


@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("B,T,D,K,F,pad_to", SHAPES)
def test_op_matches_fp64(B, T, D, K, F, pad_to, which):
    dev = cuda()
    seed = SEEDS[(B, T, D, K, F)][which]
    inputs, ref = _random_case(B, T, D, K, F, pad_to, seed)
    tag = f"({B},{T},{D},{K},{F}) pad_to {pad_to} seed {seed}"
    _condition(tag, ref)
    got, feats = _run_op(inputs, T, dev, pad_to)
    Wp = V.padded(K * F + K, pad_to)
    assert feats[0].shape == (B * T, Wp) and feats[1].shape == (B * (T - 1), Wp) and feats[0].is_contiguous() and feats[1].is_contiguous()
    assert got["dx"].shape == (B * T, D) and got["danchors"].shape == (D, K) and got["dcnn_s"].shape == got["dcnn_t"].shape == (K, F, D)
    _check(tag, got, ref)
    if pad_to > 1:
        assert got["s_pad"].shape[1] == got["t_pad"].shape[1] == Wp - K * F - K > 0
        # an upstream gradient on the padding columns alone contributes exactly nothing
        up = [torch.zeros_like(u) for u in inputs[3]]
        for u, u0 in zip(up, inputs[3]):
            u[:, K * F + K:] = u0[:, K * F + K:]
        only, _ = _run_op(inputs, T, dev, pad_to, up)
        for n in V.GRADS:
            assert float(only[n].abs().max()) == 0.0, f"{tag} {n}: the padding columns' gradient contribution is {float(only[n].abs().max()):.3e}"


def test_frame_equal_to_an_anchor_has_a_zero_norm_column_with_zero_gradients():
    """q = 0: e is the clamped l2_normalize's value (0), that norm column and that anchor's spatial convolution columns are exactly 0, and
    an upstream gradient on that norm entry alone reaches nothing."""
    dev = cuda()
    B, T, D, K, F = 2, 5, 128, 3, 4
    seed = SEEDS["frame == anchor"][0]
    x, anchors, cnn, up = V.make_inputs(B, T, D, K, F, seed)
    x[T + 2] = anchors[:, 1]                                    # clip 1, frame 2 sits on anchor 1
    ref = _reference(x, anchors, cnn, up, T, 1)
    _condition("frame == anchor", ref, clamped=True)
    assert ref["cond"]["smallest"] == 0.0
    for n in NAMES:
        assert bool(torch.isfinite(ref["64"][n]).all()), n
    got, feats = _run_op((x, anchors, cnn, up), T, dev, 1)
    _check("frame == anchor", got, ref, values_only=True)
    assert float(feats[0].detach()[T + 2, K * F + 1]) == 0.0 and float(feats[0].detach()[T + 2, F:2 * F].abs().max()) == 0.0
    only = [torch.zeros_like(u) for u in up]
    only[0][T + 2, K * F + 1] = 3.0
    grads, _ = _run_op((x, anchors, cnn, up), T, dev, 1, only)
    for n in V.GRADS:
        assert float(grads[n].abs().max()) == 0.0, f"{n}: the clamped norm's gradient contribution is {float(grads[n].abs().max()):.3e}"


@pytest.mark.parametrize("B,T,D,K,F,pad_to", [(2, 33, 128, 8, 32, 1), (5, 30, 128, 2, 4, 32)])
def test_convolution_columns_carry_the_bits_of_the_magnitude_conv_entry(B, T, D, K, F, pad_to):
    """feat_s[:, :K*F] == so and the compacted feat_t[:, :K*F] == to[frames >= 1] of lpm_triangulation_magnitude_norms + _conv, bit for
    bit; and two runs of the op give the same bits in outputs and gradients."""
    from learnablepoolingmethods_amd import _capi, ops
    dev = cuda()
    inputs, _ = _random_case(B, T, D, K, F, pad_to, SEEDS[(B, T, D, K, F)][0])
    a, feats = _run_op(inputs, T, dev, pad_to)
    b, _ = _run_op(inputs, T, dev, pad_to)
    for n in NAMES:
        assert torch.equal(a[n], b[n]), n
    lib = _capi.load()
    x, anchors, cnn_s, cnn_t = (t.to(dev).contiguous() for t in (inputs[0], inputs[1], *inputs[2]))
    q, p = torch.empty(2, B * T, K, device=dev), torch.empty(2, B * T, K, device=dev)
    so, to = torch.empty(B * T, K * F, device=dev), torch.empty(B * T, K * F, device=dev)
    lib.check(lib._lpm_triangulation_magnitude_norms(ops.ptr(x), ops.ptr(anchors), B, T, D, K, ops.ptr(q), ops.ptr(p), ops.stream_ptr()),
              "lpm_triangulation_magnitude_norms")
    lib.check(lib._lpm_triangulation_magnitude_conv(ops.ptr(x), ops.ptr(anchors), ops.ptr(cnn_s), ops.ptr(cnn_t), ops.ptr(q), ops.ptr(p), B, T,
                                                    D, K, F, ops.ptr(so), ops.ptr(to), ops.stream_ptr()), "lpm_triangulation_magnitude_conv")
    torch.cuda.synchronize()
    assert torch.equal(feats[0][:, :K * F], so)
    assert torch.equal(feats[1][:, :K * F], to.reshape(B, T, K * F)[:, 1:].reshape(B * (T - 1), K * F))
    assert float(to.reshape(B, T, K * F)[:, 0].abs().max()) == 0.0
    assert torch.equal(feats[0][:, K * F:K * F + K], q[0].sqrt())
    assert torch.equal(feats[1][:, K * F:K * F + K], p[0].reshape(B, T, K)[:, 1:].reshape(-1, K).sqrt())


def test_bad_arguments_raise():
    from learnablepoolingmethods_amd import _capi, ops
    dev = cuda()

    def refused(x, anchors, T, **kw):
        D, K = anchors.shape
        cnn = [torch.randn(K, 3, D, device=anchors.device) for _ in range(2)]
        with pytest.raises(_capi.LpmError):
            ops.triangulation_magnitude_frames(x, anchors, *cnn, T, **kw)
    a128 = torch.randn(128, 4, device=dev)
    x = torch.randn(8, 128, device=dev)
    refused(torch.randn(8, 256, device=dev), torch.randn(256, 4, device=dev), 4)           # D = 256
    refused(torch.randn(5, 128, device=dev), a128, 1)                                      # T = 1
    refused(torch.randn(8, 256, device=dev)[:, :128], a128, 4)                             # non-contiguous x
    refused(torch.randn(321, 128, device=dev), a128, 321)                                  # T = 321
    refused(x, a128, 4, pad_to=0)
    fs, ft = ops.triangulation_magnitude_frames(x, a128, torch.randn(4, 3, 128, device=dev), torch.randn(4, 3, 128, device=dev), 4, pad_to=32)
    assert fs.shape == (8, 32) and ft.shape == (6, 32)
    torch.cuda.synchronize()


# ---- loupe_modules.NetVLAD ----
def _moving_mean(tag, store, x, v):
    """The moving mean is of the logits AS THEY ARE (loupe_modules.NetVLAD centres the rows it hands to the kernels): from zero,
    (1 - fp32(0.999)) x their batch mean (tests/_netvlad_ref.ONE_MINUS_DECAY), held to the NetVLAD rule with the figures of that mean."""
    W = v["cluster_weights"]
    want = R.ONE_MINUS_DECAY * x.double().matmul(W.double()).mean(0)
    e32 = rel_err(R.ONE_MINUS_DECAY * x.matmul(W).mean(0), want)
    ex3 = rel_err(R.ONE_MINUS_DECAY * R.three_term(x.double(), W.double()).mean(0), want)
    e_op = rel_err(store.vars["cluster_bn/moving_mean"], want)
    print(f"[triangulation v4] {tag} moving mean: op {e_op:.3e}, err32 {e32:.3e}, errx3 {ex3:.3e}, bound {max(8 * (e32 + ex3), 1e-6):.3e}")
    assert e_op <= max(8 * (e32 + ex3), 1e-6), f"{tag}: moving mean {e_op:.3e}"


def _loupe_on(dev, x, v, S, pad_input_to=None):
    from learnablepoolingmethods_amd import loupe_modules as L, variables as vs
    D, C = v["cluster_weights"].shape
    store = vs.VariableStore(device=dev)
    for n, t in v.items():
        store.vars[n], store.trainable[n] = t.to(dev).clone().requires_grad_(True), True
    xl = (x if pad_input_to is None else torch.nn.functional.pad(x, (0, pad_input_to - D))).to(dev).requires_grad_(True)
    with vs.use_store(store):
        out = L.NetVLAD(D, S, C, v["hidden1_weights"].shape[1], False, True, True).forward(xl)
    return out, xl, store


@pytest.mark.parametrize("B,S,D,C,O,padded_input", [(2, 7, 32, 32, 16, False), (2, 6, 20, 32, 16, False), (2, 6, 20, 32, 16, True)])
def test_loupe_netvlad_matches_fp64(B, S, D, C, O, padded_input):
    from learnablepoolingmethods_amd import loupe_modules as L
    dev = cuda()
    assert L.fused_ok(S, D, C), "ops.netvlad runs this shape: the test is about that route"
    x, v, up = V.netvlad_inputs(B, S, D, C, O, 0)
    p64, p32 = V.netvlad_and_grads(x, v, S, up, torch.float64), V.netvlad_and_grads(x, v, S, up, torch.float32)
    px3 = V.netvlad_and_grads(x, v, S, up, torch.float64, mm=R.mm3)
    out, xl, store = _loupe_on(dev, x, v, S, L.padded_size(D, C) if padded_input else None)
    assert out.shape == (B, O)
    grads = torch.autograd.grad((out * up.to(dev)).sum(), [xl] + [store.vars[n] for n in V.VLAD_VARS])
    got = dict(out=out, dx=grads[0][:, :D], **{"d" + n: g for n, g in zip(V.VLAD_VARS, grads[1:])})
    tag = f"loupe NetVLAD ({B},{S},{D},{C},{O}){' padded input' if padded_input else ''}"
    rows = []
    for n in p64:
        assert got[n].shape == p64[n].shape, n
        e32, ex3 = R.figure(p32[n], p64[n], n, B), R.figure(px3[n], p64[n], n, B)
        rows.append((n, R.figure(got[n], p64[n], n, B), e32, ex3, max(8 * (e32 + ex3), 1e-6)))     # tests/test_gpu_netvlad_bounds.py:284
    for n, e_op, e32, ex3, bound in rows:
        print(f"[triangulation v4] {tag} {n}: op {e_op:.3e}, err32 {e32:.3e}, errx3 {ex3:.3e}, bound {bound:.3e}, ratio {e_op / bound:.3f}")
    for n, e_op, e32, ex3, bound in rows:
        assert math.isfinite(e_op) and e_op <= bound, f"{tag} {n}: op error {e_op:.3e} > bound {bound:.3e}"
    if padded_input:
        assert grads[0].shape == (B * S, L.padded_size(D, C)) and bool(torch.isfinite(grads[0]).all())
    _moving_mean(tag, store, x, v)


def test_loupe_netvlad_is_the_projects_netvlad_class_followed_by_the_matmul():
    """From the same variables on the GPU: frame_level_models.NetVLAD (ops.netvlad on the rows as they are) and a matmul against
    loupe_modules.NetVLAD (the same on centred rows): one function, so both lie within the NetVLAD bound of the same fp64 value, and the
    moving mean loupe_modules.NetVLAD leaves is the class's (of the logits as they are)."""
    from learnablepoolingmethods_amd import frame_level_models, variables as vs
    dev = cuda()
    B, S, D, C, O = 2, 7, 128, 32, 16                                      # (a width the class takes as it is: no padding)
    x, v, up = V.netvlad_inputs(B, S, D, C, O, 0)
    p64, p32 = V.netvlad_and_grads(x, v, S, up, torch.float64), V.netvlad_and_grads(x, v, S, up, torch.float32)
    px3 = V.netvlad_and_grads(x, v, S, up, torch.float64, mm=R.mm3, centre=False)     # (the class: the rows as they are)
    out, _, store = _loupe_on(dev, x, v, S)
    _moving_mean("loupe_modules.NetVLAD (2,7,128,32,16)", store, x, v)
    with vs.use_store(store), torch.no_grad():                             # (training mode: the batch statistics normalise, as above)
        store.vars["cluster_bn/moving_mean"].zero_()
        vlad = frame_level_models.NetVLAD(D, S, C, True, True).forward(x.to(dev))
    _moving_mean("frame_level_models.NetVLAD (2,7,128,32,16)", store, x, v)
    bound = max(8 * (R.figure(p32["out"], p64["out"], "out", B) + R.figure(px3["out"], p64["out"], "out", B)), 1e-6)
    e_class = R.figure(vlad.matmul(store.vars["hidden1_weights"]), p64["out"], "out", B)
    e_loupe = R.figure(out, p64["out"], "out", B)
    print(f"[triangulation v4] class + matmul {e_class:.3e}, loupe_modules.NetVLAD {e_loupe:.3e}, bound {bound:.3e}")
    assert e_class <= bound and e_loupe <= bound


def test_the_models_default_shapes_take_the_netvlad_kernels():
    """No launch.  The predicates ops.netvlad consults accept (T, Wp, C) of both streams at the defaults with Wp the next multiple of 32,
    video 32 * 64 + 32 = 2080 and audio 8 * 16 + 8 = 136 -> 160: the assignment GEMM and the backward would run.  The aggregation FORWARD
    has no predicate of its own for the d-major form and refuses both (lpm_vlad_aggregate_tiles_fwd: 128 / 256 / 512 / 1024 columns); its
    LDS-shared form (lpm_vlad_tiles3_supported) takes multiples of 128 with 256 clusters, so loupe_modules pads to 2176 and 256, which
    every predicate accepts."""
    from learnablepoolingmethods_amd import _capi, loupe_modules as L, ops
    lib = _capi.load()
    for T, Wp, C in ((200, 2080, 256), (199, 2080, 256), (200, 160, 256), (199, 160, 256)):
        assert bool(lib._lpm_assign_gemm_tiles_supported(T, Wp, C)) and ops._bwd_tiles_ok(lib, T, Wp, C) and ops.netvlad_input_shortcut_ok(T, Wp, C)
        assert not lib._lpm_vlad_tiles3_supported(Wp, C) and Wp not in L.STREAMING_WIDTHS
    assert L.padded_size(2080, 256) == 2176 and L.padded_size(136, 256) == 256
    for T, Wp, C in ((200, 2176, 256), (199, 2176, 256), (200, 256, 256), (199, 256, 256)):
        assert bool(lib._lpm_assign_gemm_tiles_supported(T, Wp, C)) and ops._bwd_tiles_ok(lib, T, Wp, C) and ops.netvlad_input_shortcut_ok(T, Wp, C)
        assert bool(lib._lpm_vlad_tiles3_supported(Wp, C))
    for T, W in ((200, 2080), (199, 2080), (200, 136), (199, 136)):
        assert L.fused_ok(T, W, 256)
    assert L.padded_size(20, 32) == L.padded_size(32, 32) == 128 and L.padded_size(1025, 32) is None and not L.fused_ok(7, 20, 16)


def _floor(n, r64, gscale):
    """The floor under the Frobenius norm of gradient ``n``'s fp64 reference: 1e-4 x the largest gradient entry of the run x sqrt(numel)
    (tests/test_gpu_models.py:175).  The beta of a batch norm that another batch norm follows has a gradient that is ZERO in exact
    arithmetic (the shift is the same for every row and leaves with the next batch mean): its fp64 reference is rounding, 1e-17, and any
    evaluation's value is the rounding of sum_b dA[b] over the rows, which scales with the summands dA -- not with the largest entry of
    some other variable.  The gamma of the same batch norm is sum_b dA[b] xhat[b] over the same summands with |xhat| about 1, so where a
    beta's reference is below 1e-9 of its gamma's (decided on the fp64 reference alone) the floor is the norm of that gamma's
    gradient.  (Under the floor above the fp32 evaluation on the CPU is itself at 1.07e-3 for one of them.)"""
    floor = 1e-4 * gscale * r64[n].numel() ** 0.5
    if n.endswith("/beta") and n[:-len("beta")] + "gamma" in r64:
        gamma = float(r64[n[:-len("beta")] + "gamma"].double().norm())
        if float(r64[n].double().norm()) <= 1e-9 * gamma:
            floor = max(floor, gamma)
    return floor


def _model_level(tag, got, r64, r32, values):
    """The project's model-level figures (tests/test_gpu_models.py:155-175): ``values`` by rel_err, gradients by rel_l2 over ``_floor``;
    everything printed, then held to REL_TOL."""
    gscale = max(float(v.abs().max()) for n, v in r64.items() if n not in values)

    def fig(a, n):
        return rel_err(a, r64[n]) if n in values else rel_l2(a, r64[n], floor=_floor(n, r64, gscale))
    rows = [(n, fig(got[n], n), fig(r32[n], n)) for n in r64]
    for n, e_op, e32 in rows:
        print(f"[triangulation v4] {tag} {n}: error {e_op:.3e}, fp32 CPU path {e32:.3e}, bound {REL_TOL:.0e}, ratio {e_op / REL_TOL:.3f}")
    for n, e_op, e32 in rows:
        assert bool(torch.isfinite(got[n]).all()) and e_op <= REL_TOL, f"{tag} {n}: error {e_op:.3e} > {REL_TOL:.0e}"


# ---- the module ----
def _module_run(path, device, dtype, state, x, T, D, K, F, H, O, C, up):
    from learnablepoolingmethods_amd import variables as vs, video_pooling_modules as M
    store = vs.VariableStore(device=device)
    for n, (t, tr) in state.items():
        store.vars[n] = t.to(device=device, dtype=dtype).clone().requires_grad_(tr)
        store.trainable[n] = tr
    xl = x.to(device=device, dtype=dtype).requires_grad_(True)
    with vs.use_store(store):
        module = M.TriangulationMagnitudeNsCnnNetVladModule(D, T, K, True, H, F, O, False, True, True, True, cluster_size=C)
        out = module.head(*getattr(module, path)(xl))
    names = [n for n, tr in store.trainable.items() if tr]
    grads = torch.autograd.grad((out * up.to(device=device, dtype=dtype)).sum(), [xl] + [store.vars[n] for n in names])
    return dict(out=out.detach(), dx=grads[0], **{"grad " + n: g for n, g in zip(names, grads[1:])})


def test_module_fused_frames_and_head_on_the_gpu_against_frames_and_head_in_fp64():
    from learnablepoolingmethods_amd import variables as vs, video_pooling_modules as M
    dev = cuda()
    B, T, D, K, F, H, O, C = 4, 7, 128, 5, 3, 16, 8, 32
    seed = SEEDS["module"][0]
    x, anchors, cnn, _ = V.make_inputs(B, T, D, K, F, seed)
    _condition("module (4,7,128,5,3)", dict(cond=V.conditions(x, anchors, cnn, T)))
    init = vs.VariableStore(device="cpu", seed=5)
    for n, t in zip(("anchor_weights", "spatial_cnn_weights", "temporal_cnn_weights"), (anchors, *cnn)):
        init.vars[n], init.trainable[n] = t.clone(), True
    with vs.use_store(init), torch.no_grad():
        M.TriangulationMagnitudeNsCnnNetVladModule(D, T, K, True, H, F, O, False, True, True, False, cluster_size=C).forward(x)
    state = {n: (t.detach().clone(), init.trainable[n]) for n, t in init.vars.items()}
    up = torch.randn(B, O, generator=torch.Generator().manual_seed(9))
    r64 = _module_run("frames", "cpu", torch.float64, state, x, T, D, K, F, H, O, C, up)
    r32 = _module_run("frames", "cpu", torch.float32, state, x, T, D, K, F, H, O, C, up)
    got = _module_run("fused_frames", dev, torch.float32, state, x, T, D, K, F, H, O, C, up)
    assert got["out"].shape == (B, O) and set(got) == set(r64)
    # the bound is the NetVLAD op's (tests/test_gpu_netvlad_bounds.py:284), max(8 (err32 + errx3), 1e-6): errx3 the restatement's own error
    # with the split-operand product in its four NetVLAD products, on centred rows as loupe_modules.NetVLAD hands them over (measured
    # on the CPU at this shape: 8e-6 to 2e-5 of most gradients, 7e-5 / 9e-5 of the two cluster_bn/beta; on the rows as they are 1.4e-4 to
    # 2.3e-4 and 1.4e-3 / 1.8e-3 -- three batch norms over B = 4 rows behind a product rounded at 2^-16 of rows that differ by a twentieth)
    flat = {n: t for n, (t, _) in state.items()}
    p64, px3 = V.module_and_grads(x, flat, T, up), V.module_and_grads(x, flat, T, up, mm=R.mm3)
    assert set(p64) == set(r64)
    gscale = max(float(v.abs().max()) for n, v in r64.items() if n != "out")

    def fig(a, ref, n):
        return rel_err(a, ref) if n == "out" else rel_l2(a, ref, floor=_floor(n, r64, gscale))
    rows = [(n, fig(got[n], r64[n], n), fig(r32[n], r64[n], n), fig(px3[n], p64[n], n), fig(p64[n], r64[n], n)) for n in r64]
    for n, e_op, e32, ex3, e_ref in rows:
        bound = max(8 * (e32 + ex3), 1e-6)
        print(f"[triangulation v4] module {n}: error {e_op:.3e}, err32 {e32:.3e}, errx3 {ex3:.3e}, bound {bound:.3e}, ratio {e_op / bound:.3f} "
              f"(the restatement against the fp64 module path: {e_ref:.1e})")
    for n, e_op, e32, ex3, e_ref in rows:
        assert e_ref <= 1e-9, f"module {n}: the restatement and the fp64 module path differ by {e_ref:.3e}"
        assert bool(torch.isfinite(got[n]).all()) and e_op <= max(8 * (e32 + ex3), 1e-6), f"module {n}: error {e_op:.3e} > bound"


# ---- the model ----
MODEL_SEED = 0                              # MODEL-SEED (searched like SEEDS: the conditions hold on both streams)
MODEL = dict(iterations=6, video_anchor_size=4, audio_anchor_size=2, video_kernel_size=5, audio_kernel_size=3, video_hidden=16,
             audio_hidden=8, video_output_dim=16, audio_output_dim=8, cluster_size=32)


def _model_run(state, xin, nf, lab, u, device, dtype, fused):
    """One training forward + backward of JuhanTestModelV4 from ``state``: predictions, loss and every trainable variable's gradient."""
    from learnablepoolingmethods_amd import FLAGS, losses, registry, variables as vs
    store = vs.VariableStore(device=device)
    for n, (v, tr) in state.items():
        store.vars[n] = v.to(device=device, dtype=dtype).clone().requires_grad_(tr)
        store.trainable[n] = tr
    FLAGS.triangulation_v4_fused = fused
    try:
        with vs.use_store(store), vs.variable_scope("tower"):
            result = registry.get_model("JuhanTestModelV4").create_model(xin.to(device=device, dtype=dtype), num_frames=nf.to(device),
                                                                         vocab_size=lab.shape[1], is_training=True, frame_uniform=u, **MODEL)
        reg = store.pop_regularization_losses()
    finally:
        FLAGS.reset()
    pred = result["predictions"]
    loss = losses.CrossEntropyLoss().calculate_loss(pred, lab.to(device))
    if reg:
        loss = loss + torch.stack(reg).sum()
    names = [n for n, tr in store.trainable.items() if tr]
    grads = torch.autograd.grad(loss, [store.vars[n] for n in names])
    return dict(predictions=pred.detach(), loss=loss.detach().reshape(1), **{"grad " + n: g for n, g in zip(names, grads)})


def model_state_and_batch(seed):
    """The model's variables at their initialisers with the anchors scaled by 0.25 (as the op's own inputs), a synthetic batch and its
    frame draws."""
    from oracle import lpm_oracle as O
    from learnablepoolingmethods_amd import layers, registry, variables as vs
    Vn, B, MF = 20, 4, 8
    x, nf, lab = O.make_synthetic_batch(B, MF, 1152, Vn, seed=seed, min_frames=MODEL["iterations"])
    xin = layers.l2_normalize(x, 2)                        # train.normalize_input's formula, once, for all three runs
    g = torch.Generator().manual_seed(42)
    u = torch.stack([(torch.randperm(int(n), generator=g)[:MODEL["iterations"]].float() + 0.5) / float(n) for n in nf])
    init = vs.VariableStore(device="cpu", seed=3)
    with vs.use_store(init), vs.variable_scope("tower"):
        registry.get_model("JuhanTestModelV4").create_model(xin, num_frames=nf, vocab_size=Vn, is_training=False, frame_uniform=u, **MODEL)
    init.pop_regularization_losses()
    state = {n: (v.detach().clone(), init.trainable[n]) for n, v in init.vars.items()}
    for n, (v, tr) in state.items():
        if n.endswith("anchor_weights"):
            v.mul_(0.25)
    return state, xin, nf, lab, u


def model_stream_conditions(state, xin, nf, u):
    from learnablepoolingmethods_amd import model_utils
    frames = model_utils.SampleRandomFrames(xin, nf.reshape(-1, 1), MODEL["iterations"], uniform=u).reshape(-1, 1152)
    out = {}
    for name, cols in (("video", slice(0, 1024)), ("audio", slice(1024, None))):
        s = f"tower/{name}_triangulation_embedding/"
        cnn = [state[s + "spatial_cnn_weights"][0], state[s + "temporal_cnn_weights"][0]]
        out[name] = V.conditions(frames[:, cols], state[s + "anchor_weights"][0], cnn, MODEL["iterations"])
    return out


def test_juhan_test_model_v4_fused_on_the_gpu_against_the_fp64_cpu_path():
    """B = 4, 6 sampled frames, anchors 4 / 2, filters 5 / 3, 32 clusters, hidden 16 / 8, output 16 / 8, vocab 20: the model with
    FLAGS.triangulation_v4_fused on the GPU against the model built on the fp64 CPU path from the same variables and frame draws, at the
    model-level bound 1e-3 (the NetVLAD stage is split-bf16); the fp32 CPU path's own error beside each figure.

    Measured on the MI355X: the largest of the 53 figures is 5.8e-04 (the video stream's temporal_vlad/cluster_bn/beta; its
    spatial_vlad/cluster_bn/beta 3.0e-04, where the fp32 CPU path has 3.3e-04 and 2.2e-04), predictions 2e-05.  With the rows handed to
    the NetVLAD kernels as they are, not centred (loupe_modules.NetVLAD._fused_descriptor), these two were at 6.3e-03 and 3.3e-03: the
    gradient of cluster_bn/beta is a column sum of softmax gradients that cancel over the rows, behind dU . (x - w2) in split-bf16 on
    rows that differ by a twentieth of their length and in front of three batch norms over B = 4 rows."""
    dev = cuda()
    state, xin, nf, lab, u = model_state_and_batch(MODEL_SEED)
    for name, c in model_stream_conditions(state, xin, nf, u).items():                      # the op's conditions, per stream
        _condition(f"model {name} stream", dict(cond=c))
    r64 = _model_run(state, xin, nf, lab, u, "cpu", torch.float64, False)
    r32 = _model_run(state, xin, nf, lab, u, "cpu", torch.float32, False)
    got = _model_run(state, xin, nf, lab, u, dev, torch.float32, True)
    assert got["predictions"].shape == (4, 20) and set(got) == set(r64)
    assert not any("final_activation_bn" in n or "input_bn" in n for n in got)
    _model_level("model", got, r64, r32, ("predictions", "loss"))


def test_three_steps_of_the_run_loop_and_a_checkpoint_that_predicts_the_same_bits_twice(tmp_path):
    from oracle import lpm_oracle as O
    from learnablepoolingmethods_amd import FLAGS, registry, training
    from learnablepoolingmethods_amd.predictor import Predictor
    from learnablepoolingmethods_amd.train import Trainer
    dev = cuda()
    Vn, B, MF = 20, 4, 8
    batches = []
    for i in range(3):
        x, nf, lab = O.make_synthetic_batch(B, MF, 1152, Vn, seed=50 + i, min_frames=MODEL["iterations"])
        batches.append((None, x.to(dev), lab.to(dev), nf.to(dev)))
    losses = []
    FLAGS.triangulation_v4_fused = True
    try:
        tr = Trainer(registry.get_model("JuhanTestModelV4"), vocab_size=Vn, batch_size=B, base_learning_rate=1e-3, device=dev, seed=3,
                     model_kwargs=MODEL)
        res = training.run(tr, iter(batches), log_every=1, log=lambda s: None, on_step=lambda out, batch: losses.append(float(out["loss"])))
        print(f"[triangulation v4] run loop losses {losses}")
        assert res["global_step"] == res["steps"] == 3 and len(losses) == 3 and all(math.isfinite(v) for v in losses)
        path = str(tmp_path / "model.ckpt-3.pt")
        tr.save(path)
        _, x, _, nf = batches[0]
        u = torch.full((B, MODEL["iterations"]), 0.5)
        pr = Predictor.from_checkpoint(path, registry.get_model("JuhanTestModelV4"), vocab_size=Vn, model_kwargs=dict(MODEL, frame_uniform=u),
                                       device=dev)
        a, b = pr.predict(x, nf), pr.predict(x, nf)
    finally:
        FLAGS.reset()
    assert a.shape == (B, Vn) and bool(torch.isfinite(a).all()) and torch.equal(a, b)
