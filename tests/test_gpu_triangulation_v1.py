"""-m gpu: ops.triangulation_bn_moments (csrc/triangulation_bn_moments.hip), TriangulationCnnIndirectAttentionModule on the GPU and
JuhanTestModelV1 against the fp64 restatement on the CPU (tests/_triangulation_v1_ref.py) -- never against the op itself or the module.

Tolerance (the rule of tests/test_gpu_triangulation.py): the restatement evaluated in fp32 torch on the CPU carries an error err32
against fp64 (maximum absolute error over the maximum absolute fp64 value); the op's error must be <= max(8 err32, 1e-6).  It is taken
per PART (spatial mean, spatial variance, temporal mean, temporal variance) and per gradient (dx, danchors and the four affine ones,
with N(0,1) upstream gradients on all parts).  Every figure is printed before any is asserted.  A part whose fp64 reference is
identically zero (the temporal variance at T = 2) must be exactly zero in the op.

Conditions, asserted on the fp64 restatement before any launch: no spatial squared norm below 1e-6 (the clamped test is exempt: it is
about exactly that); in every clip no |G[t,u]| of either Gram below 1e-5 max |G| of that clip (a relu mask flipped by rounding changes
a gradient row by about 1/T: not a rounding error); except in the saturated test the largest softmax weight of every clip with at
least three rows is <= 0.9.  The seeds below were searched on the CPU for these conditions; a seed that fails one is replaced, never
skipped, and no threshold is loosened.  SEEDS: (B, T, D, K) or a test's name -> seeds, with the smallest Gram ratio and the largest
weight measured for each."""
import functools
import math

import pytest
import torch

from tests import _triangulation_v1_ref as V
from tests._util import cuda

pytestmark = pytest.mark.gpu

NAMES = V.PARTS + V.GRADS
STAT_NAMES = ("mean_s", "var_s", "mean_t", "var_t")

SEEDS = {
    # SEEDS-BEGIN
    (3, 2, 128, 1): (0, 1, 2),                              # 2.6e-02, 0.00; 6.4e-02, 0.00; 5.8e-02, 0.00
    (2, 7, 128, 5): (0, 1, 2),                              # 5.1e-04, 0.18; 1.1e-03, 0.18; 5.2e-04, 0.18
    (2, 30, 1024, 3): (0, 1, 2),                            # 5.3e-01, 0.03; 5.3e-01, 0.03; 5.6e-01, 0.03
    (2, 33, 128, 16): (2, 16, 21),                          # 1.5e-04, 0.05; 1.0e-04, 0.05; 1.1e-04, 0.05
    (1, 70, 128, 4): (10, 12, 16),                          # 1.2e-04, 0.02; 1.2e-04, 0.02; 1.1e-04, 0.02
    (1, 320, 128, 2): (8797, 54239, 5317),                  # 1.3e-05, 0.03; 1.3e-05, 0.02; 1.2e-05, 0.04 (about one seed in 7000 passes)
    ("combinations", 2, 7, 128, 5, True): (0,),             # 5.1e-04, 0.18
    ("combinations", 2, 7, 128, 5, False): (0,),            # 9.3e-01, 0.25
    ("combinations", 2, 33, 128, 16, True): (2,),           # 1.5e-04, 0.05
    ("combinations", 2, 33, 128, 16, False): (4,),          # 8.4e-01, 0.88
    "given statistics": (0,),                               # 9.3e-01, 0.18
    "saturated": (1,),                                      # 1.3e-04, 1.00
    "nearly constant": (0, 1, 2),                           # 1.0e+00, 0.03; 1.0e+00, 0.03; 1.0e+00, 0.03
    "frame == anchor": (0,),                                # 2.8e-03, 0.78
    # SEEDS-END
}


def _err(a, ref):
    ref = ref.double()
    return float((a.detach().double().cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


def _names(use_bn):
    return NAMES if use_bn else V.PARTS + V.GRADS[:2]


def _reference(x, anchors, affine, up, T, att=True, use_bn=True, stats=None):
    """fp64 and fp32 values / gradients of the restatement, split into the named parts, the batch statistics and the conditions."""
    ref = dict(cond=V.conditions(x, anchors, affine, T, use_bn, stats))
    for key, dt in (("64", torch.float64), ("32", torch.float32)):
        st = None if stats is None else [s.to(dt) for s in stats]
        outs, grads = V.pools_and_grads(x.to(dt), anchors.to(dt), [a.to(dt) for a in affine], T, up, att, use_bn, st)
        ref[key] = {**V.split_parts(*outs), **dict(zip(V.GRADS, grads)), **dict(zip(STAT_NAMES, V.batch_statistics(x.to(dt), anchors.to(dt), T)))}
    return ref


@functools.lru_cache(maxsize=None)
def _random_case(B, T, D, K, seed, att=True, use_bn=True):
    x, anchors, affine, up = V.make_inputs(B, T, D, K, seed)
    return (x, anchors, affine, up), _reference(x, anchors, affine, up, T, att, use_bn)


def _given_statistics(J, seed):
    """Moving statistics of the embeddings' own scale (entries ~ 1/sqrt(D), variances ~ 1/D), unrelated to the batch."""
    g = torch.Generator().manual_seed(1000 + seed)
    return [0.02 * torch.randn(J, generator=g), (0.5 + torch.rand(J, generator=g)) * 1e-2,
            0.02 * torch.randn(J, generator=g), (0.5 + torch.rand(J, generator=g)) * 1e-2]


def _nearly_constant(B, T, D, K, seed):
    x, anchors, affine, up = V.make_inputs(B, T, D, K, seed)
    g = torch.Generator().manual_seed(100 + seed)
    base = torch.randn(B, 1, D, generator=g)
    base = base / base.norm(dim=2, keepdim=True)
    x = (base + 1e-3 * torch.randn(B, T, D, generator=g) / math.sqrt(D)).reshape(B * T, D)
    return x, anchors, affine, up


def _saturated(B, T, D, K, seed):
    x, anchors, affine, up = V.make_inputs(B, T, D, K, seed)
    J = K * D
    return x, anchors, [torch.ones(J), torch.zeros(J), torch.ones(J), torch.zeros(J)], up


def _condition(tag, ref, saturated=False, clamped=False):
    c = ref["cond"]
    print(f"[triangulation v1] {tag} smallest squared norm {c['smallest']:.3e}, smallest |G| / max |G| {c['gram_ratio']:.3e}, "
          f"largest softmax weight {c['weight']:.3f}")
    if not clamped:
        assert c["smallest"] >= 1e-6, f"{tag}: a squared norm of the restatement lies below 1e-6 ({c['smallest']:.3e})"
    assert c["gram_ratio"] >= 1e-5, f"{tag}: a Gram entry lies within 1e-5 of zero relative to its clip's largest ({c['gram_ratio']:.3e})"
    if not saturated:
        assert c["weight"] <= 0.9, f"{tag}: a softmax weight of {c['weight']:.3f}"


def _run_op(inputs, T, dev, up=None, att=True, use_bn=True, stats=None):
    from learnablepoolingmethods_amd import ops
    x, anchors, affine, up0 = inputs
    up = up0 if up is None else up
    leaves = [t.to(dev).requires_grad_(True) for t in (x, anchors, *(affine if use_bn else ()))]
    aff = leaves[2:] if use_bn else [None] * 4
    st = None if stats is None else tuple(s.to(dev) for s in stats)
    pool_s, pool_t, bstats = ops.triangulation_bn_moments(leaves[0], leaves[1], *aff, T, self_attention=att, batch_norm=use_bn, stats=st)
    loss = sum((o * g.to(dev)).sum() for o, g in zip((pool_s, pool_t), up))
    grads = torch.autograd.grad(loss, leaves)
    got = {**V.split_parts(pool_s, pool_t), **dict(zip(V.GRADS, grads))}
    if use_bn:
        assert all(not s.requires_grad for s in bstats)
        got.update(zip(STAT_NAMES, bstats))
    else:
        assert bstats is None
    return got, (pool_s, pool_t)


def _check(tag, got, ref, names, values_only=False):
    """Every figure is printed before anything is asserted.  -> the worst error-over-bound ratio."""
    rows = []
    for n in names:
        zero = float(ref["64"][n].abs().max()) == 0.0
        rows.append((n, zero, float(got[n].detach().abs().max()) if zero else _err(got[n], ref["64"][n]), 0.0 if zero else _err(ref["32"][n], ref["64"][n])))
    worst = 0.0
    for n, zero, e_op, e32 in rows:
        if zero:
            print(f"[triangulation v1] {tag} {n}: the fp64 reference is identically zero; max |op| {e_op:.3e}")
        else:
            worst = max(worst, e_op / max(8 * e32, 1e-6))
            print(f"[triangulation v1] {tag} {n}: op error {e_op:.3e}, fp32 evaluation error {e32:.3e}, bound {max(8 * e32, 1e-6):.3e}, "
                  f"ratio {e_op / max(8 * e32, 1e-6):.2f}")
    print(f"[triangulation v1] {tag} worst error over bound {worst:.2f}")
    for n, zero, e_op, e32 in rows:
        assert bool(torch.isfinite(got[n]).all()), f"{tag} {n}: not finite"
        if values_only and n in V.GRADS:
            continue
        if zero:
            assert e_op == 0.0, f"{tag} {n}: must be exactly zero, max |op| {e_op:.3e}"
        else:
            assert e_op <= max(8 * e32, 1e-6), f"{tag} {n}: op error {e_op:.3e} > max(8 x {e32:.3e}, 1e-6)"
    return worst


SHAPES = [  # B, T, D, K
    (3, 2, 128, 1),                          # one temporal row; K = 1: the roll wraps onto the same anchor
    (2, 7, 128, 5),                          # everything odd
    (2, 30, 1024, 3),                        # video width at the model's own T
    (2, 33, 128, 16),                        # T one past a 32-row tile
    (1, 70, 128, 4),                         # T past 64 with a remainder: two Gram tiles
    (1, 320, 128, 2),                        # the largest T
]


@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("B,T,D,K", SHAPES)
def test_op_matches_fp64(B, T, D, K, which):
    dev = cuda()
    seed = SEEDS[(B, T, D, K)][which]
    inputs, ref = _random_case(B, T, D, K, seed)
    tag = f"({B},{T},{D},{K}) seed {seed}"
    _condition(tag, ref)
    got, outs = _run_op(inputs, T, dev)
    J = K * D
    assert outs[0].shape == outs[1].shape == (B, 2 * J)
    assert got["dx"].shape == (B * T, D) and got["danchors"].shape == (D, K) and all(got[n].shape == (J,) for n in V.GRADS[2:] + STAT_NAMES)
    _check(tag, got, ref, NAMES + STAT_NAMES)
    if T == 2:
        # one temporal row: its weight is exactly 1, so the temporal mean is V itself, and an upstream gradient on the (identically
        # zero) temporal variance alone contributes exactly nothing
        up = [torch.zeros(B, 2 * J), torch.zeros(B, 2 * J)]
        up[1][:, J:] = inputs[3][1][:, J:]
        only, _ = _run_op(inputs, T, dev, up)
        for n in V.GRADS:
            assert float(only[n].abs().max()) == 0.0, f"{tag} {n}: the zero variance's gradient contribution is {float(only[n].abs().max()):.3e}"


@pytest.mark.parametrize("use_bn,att", [(True, False), (False, True), (False, False)])
@pytest.mark.parametrize("B,T,D,K", [(2, 7, 128, 5), (2, 33, 128, 16)])
def test_the_other_combinations_of_batch_norm_and_attention(B, T, D, K, use_bn, att):
    dev = cuda()
    seed = SEEDS[("combinations", B, T, D, K, use_bn)][0]
    inputs, ref = _random_case(B, T, D, K, seed, att, use_bn)
    tag = f"({B},{T},{D},{K}) batch_norm={use_bn} self_attention={att} seed {seed}"
    _condition(tag, ref)
    got, _ = _run_op(inputs, T, dev, att=att, use_bn=use_bn)
    _check(tag, got, ref, _names(use_bn) + (STAT_NAMES if use_bn else ()))


def test_given_statistics_are_constants_and_the_batch_statistics_are_still_the_batchs_own():
    dev = cuda()
    B, T, D, K = 2, 7, 128, 5
    seed = SEEDS["given statistics"][0]
    x, anchors, affine, up = V.make_inputs(B, T, D, K, seed)
    stats = _given_statistics(K * D, seed)
    ref = _reference(x, anchors, affine, up, T, stats=stats)
    tag = f"given statistics seed {seed}"
    _condition(tag, ref)
    got, _ = _run_op((x, anchors, affine, up), T, dev, stats=stats)
    _check(tag, got, ref, NAMES + STAT_NAMES)            # (the fp64 gradients carry no statistics term: the restatement's stats are constants)


def test_saturated_softmax_stays_finite_and_within_the_rule():
    dev = cuda()
    B, T, D, K = 2, 30, 128, 3
    seed = SEEDS["saturated"][0]
    inputs = _saturated(B, T, D, K, seed)
    ref = _reference(*inputs, T)
    tag = f"saturated softmax seed {seed}"
    _condition(tag, ref, saturated=True)
    got, _ = _run_op(inputs, T, dev)
    _check(tag, got, ref, NAMES)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_nearly_constant_clips_keep_their_variances(which):
    """Every clip's frames = one unit frame + 1e-3 noise: the per-clip variances are ~1e-6 of the squared means."""
    dev = cuda()
    B, T, D, K = 2, 30, 128, 4
    seed = SEEDS["nearly constant"][which]
    inputs = _nearly_constant(B, T, D, K, seed)
    ref = _reference(*inputs, T)
    tag = f"nearly constant clips seed {seed}"
    _condition(tag, ref)
    got, _ = _run_op(inputs, T, dev)
    _check(tag, got, ref, NAMES)


def test_frame_equal_to_an_anchor_takes_the_clamped_value():
    """q = 0: e is the clamped l2_normalize's value (0); the values are the restatement's, the gradients finite."""
    dev = cuda()
    B, T, D, K = 2, 5, 128, 3
    seed = SEEDS["frame == anchor"][0]
    x, anchors, affine, up = V.make_inputs(B, T, D, K, seed)
    x[T + 2] = anchors[:, 1]                                    # clip 1, frame 2 sits on anchor 1
    ref = _reference(x, anchors, affine, up, T)
    _condition("frame == anchor", ref, clamped=True)
    assert ref["cond"]["smallest"] == 0.0
    for n in NAMES:
        assert bool(torch.isfinite(ref["64"][n]).all()), n
    got, _ = _run_op((x, anchors, affine, up), T, dev)
    _check("frame == anchor", got, ref, NAMES, values_only=True)


def test_two_runs_give_the_same_bits():
    dev = cuda()
    B, T, D, K = 2, 33, 128, 16
    inputs, _ = _random_case(B, T, D, K, SEEDS[(B, T, D, K)][0])
    a, _ = _run_op(inputs, T, dev)
    b, _ = _run_op(inputs, T, dev)
    for n in NAMES + STAT_NAMES:
        assert torch.equal(a[n], b[n]), n


def test_bad_arguments_raise():
    from learnablepoolingmethods_amd import _capi, ops
    dev = cuda()

    def refused(x, anchors, T, affine=None, **kw):
        J = anchors.shape[0] * anchors.shape[1]
        affine = [torch.ones(J, device=anchors.device) for _ in range(4)] if affine is None else affine
        with pytest.raises(_capi.LpmError):
            ops.triangulation_bn_moments(x, anchors, *affine, T, **kw)
    a128 = torch.randn(128, 4, device=dev)
    x = torch.randn(8, 128, device=dev)
    refused(torch.randn(8, 256, device=dev), torch.randn(256, 4, device=dev), 4)           # D = 256
    refused(torch.randn(5, 128, device=dev), a128, 1)                                      # T = 1
    refused(torch.randn(321, 128, device=dev), a128, 321)                                  # T = 321
    refused(torch.randn(9, 128, device=dev), a128, 4)                                      # rows no multiple of T
    refused(x, a128, 4, [torch.ones(511, device=dev)] + [torch.ones(512, device=dev)] * 3)  # wrong affine length
    refused(x, a128, 4, [torch.ones(512, device=dev)] * 3 + [None])                        # a missing affine tensor with batch norm
    refused(x, a128, 4, stats=[torch.ones(512, device=dev)] * 3 + [torch.ones(4, device=dev)])
    refused(torch.randn(8, 256, device=dev)[:, :128], a128, 4)                             # non-contiguous x
    refused(x.double(), a128, 4)                                                           # not fp32
    refused(x, a128, 4, [torch.ones(512, device=dev).double()] + [torch.ones(512, device=dev)] * 3)
    # without batch norm the affine tensors may be None
    ps, pt, st = ops.triangulation_bn_moments(x, a128, None, None, None, None, 4, batch_norm=False)
    assert st is None and ps.shape == pt.shape == (2, 1024)
    torch.cuda.synchronize()


def _moving(ref_stats, B, T):
    """layers.batch_norm's rank-2 rule from (mean_s, var_s, mean_t, var_t): moving mean, then moving variance (unbiased), per stream."""
    from learnablepoolingmethods_amd import layers
    out = []
    for z, n in enumerate((B * T, B * (T - 1))):
        out += [(1 - layers.BN_DECAY) * ref_stats[2 * z], layers.BN_DECAY + (1 - layers.BN_DECAY) * ref_stats[2 * z + 1] * n / (n - 1)]
    return out


def test_module_on_the_gpu_fused_against_pool():
    """fused_pool and pool with the same variables on the GPU: pools, gradients and moving averages, each held to the rule against the
    same fp64 yardstick."""
    from learnablepoolingmethods_amd import variables as vs, video_pooling_modules as M
    dev = cuda()
    B, T, D, K = 2, 7, 128, 5
    J = K * D
    inputs, ref = _random_case(B, T, D, K, SEEDS[(B, T, D, K)][0])
    _condition("module (2,7,128,5)", ref)
    x, anchors, affine, up = inputs
    moving_names = ("spatial_bn/moving_mean", "spatial_bn/moving_variance", "temporal_bn/moving_mean", "temporal_bn/moving_variance")
    mv64 = _moving([ref["64"][n] for n in STAT_NAMES], B, T)
    mv32 = _moving([ref["32"][n] for n in STAT_NAMES], B, T)
    for path in ("pool", "fused_pool"):
        leaves = [t.to(dev).requires_grad_(True) for t in (x, anchors, *affine)]
        store = vs.VariableStore(device=dev)
        store.vars["anchor_weights"], store.trainable["anchor_weights"] = leaves[1], True
        for z, scope in enumerate(("spatial_bn", "temporal_bn")):
            for name, v, tr in (("beta", leaves[3 + 2 * z], True), ("gamma", leaves[2 + 2 * z], True),
                                ("moving_mean", torch.zeros(J, device=dev), False), ("moving_variance", torch.ones(J, device=dev), False)):
                store.vars[f"{scope}/{name}"], store.trainable[f"{scope}/{name}"] = v, tr
        with vs.use_store(store):
            module = M.TriangulationCnnIndirectAttentionModule(D, T, K, True, 6, 5, True, True, True)
            outs = getattr(module, path)(leaves[0])
        assert len(store.vars) == 9
        grads = torch.autograd.grad(sum((o * g.to(dev)).sum() for o, g in zip(outs, up)), leaves)
        _check(f"module.{path} (2,7,128,5)", {**V.split_parts(*outs), **dict(zip(V.GRADS, grads))}, ref, NAMES)
        for n, r64, r32 in zip(moving_names, mv64, mv32):
            e_op, e32 = _err(store.vars[n], r64), _err(r32, r64)
            print(f"[triangulation v1] module.{path} {n}: error {e_op:.3e}, fp32 evaluation error {e32:.3e}")
            assert e_op <= max(8 * e32, 1e-6), f"module.{path} {n}"


MODEL_SEED = 41                             # (searched like SEEDS: the conditions hold on both streams)
MODEL = dict(iterations=6, video_anchor_size=4, audio_anchor_size=2, video_hidden=16, audio_hidden=8, video_output_dim=16, audio_output_dim=8)


def _model_run(state, xin, nf, lab, u, device, dtype, fused):
    """One training forward + backward of JuhanTestModelV1 from ``state``: predictions, loss and every trainable variable's gradient."""
    from learnablepoolingmethods_amd import FLAGS, losses, registry, variables as vs
    store = vs.VariableStore(device=device)
    for n, (v, tr) in state.items():
        store.vars[n] = v.to(device=device, dtype=dtype).clone().requires_grad_(tr)
        store.trainable[n] = tr
    FLAGS.triangulation_v1_fused = fused
    try:
        with vs.use_store(store), vs.variable_scope("tower"):
            result = registry.get_model("JuhanTestModelV1").create_model(xin.to(device=device, dtype=dtype), num_frames=nf.to(device), vocab_size=lab.shape[1], is_training=True,
                                                                         frame_uniform=u, **MODEL)
        reg = store.pop_regularization_losses()
    finally:
        FLAGS.reset()
    pred = result["predictions"]
    loss = losses.CrossEntropyLoss().calculate_loss(pred, lab.to(device)) + torch.stack(reg).sum()
    names = [n for n, tr in store.trainable.items() if tr]
    grads = torch.autograd.grad(loss, [store.vars[n] for n in names])
    return dict(predictions=pred.detach(), loss=loss.detach().reshape(1), **{"grad " + n: g for n, g in zip(names, grads)})


def test_juhan_test_model_v1_fused_on_the_gpu_against_the_fp64_cpu_path():
    """B = 4, 6 sampled frames, anchors 4 / 2, hidden 16 / 8, output 16 / 8, vocab 20: the model with FLAGS.triangulation_v1_fused on the
    GPU against the model built on the fp64 CPU path from the same variables and frame draws; err32 is the fp32 CPU path's."""
    from oracle import lpm_oracle as O
    from learnablepoolingmethods_amd import layers, model_utils, registry, variables as vs
    dev = cuda()
    Vn, B, MF = 20, 4, 8
    x, nf, lab = O.make_synthetic_batch(B, MF, 1152, Vn, seed=MODEL_SEED, min_frames=MODEL["iterations"])
    xin = layers.l2_normalize(x, 2)                        # train.normalize_input's formula, once, for all three runs
    g = torch.Generator().manual_seed(42)
    u = torch.stack([(torch.randperm(int(n), generator=g)[:MODEL["iterations"]].float() + 0.5) / float(n) for n in nf])
    init = vs.VariableStore(device="cpu", seed=3)
    with vs.use_store(init), vs.variable_scope("tower"):
        registry.get_model("JuhanTestModelV1").create_model(xin, num_frames=nf, vocab_size=Vn, is_training=False,
                                                            frame_uniform=u, **MODEL)
    init.pop_regularization_losses()
    state = {n: (v.detach().clone(), init.trainable[n]) for n, v in init.vars.items()}
    g2 = torch.Generator().manual_seed(43)
    for n, (v, tr) in state.items():                      # the softmax away from saturation, as the op's own inputs (make_inputs)
        if n.endswith(("spatial_bn/gamma", "temporal_bn/gamma")):
            v.copy_((0.5 + torch.rand(v.shape, generator=g2)) / math.sqrt(v.numel()))
        elif n.endswith(("spatial_bn/beta", "temporal_bn/beta")):
            v.copy_(0.1 * torch.randn(v.shape, generator=g2) / math.sqrt(v.numel()))
    frames = model_utils.SampleRandomFrames(xin, nf.reshape(-1, 1), MODEL["iterations"], uniform=u).reshape(-1, 1152)
    for name, cols in (("video", slice(0, 1024)), ("audio", slice(1024, None))):          # the op's conditions, per stream
        s = f"tower/{name}_triangulation_embedding/"
        affine = [state[s + n][0] for n in ("spatial_bn/gamma", "spatial_bn/beta", "temporal_bn/gamma", "temporal_bn/beta")]
        _condition(f"model {name} stream", dict(cond=V.conditions(frames[:, cols], state[s + "anchor_weights"][0], affine, MODEL["iterations"])))
    r64 = _model_run(state, xin, nf, lab, u, "cpu", torch.float64, False)
    r32 = _model_run(state, xin, nf, lab, u, "cpu", torch.float32, False)
    got = _model_run(state, xin, nf, lab, u, dev, torch.float32, True)
    assert got["predictions"].shape == (B, Vn) and set(got) == set(r64)
    rows = [(n, _err(got[n], r64[n]), _err(r32[n], r64[n])) for n in r64]
    for n, e_op, e32 in rows:
        print(f"[triangulation v1] model {n}: error {e_op:.3e}, fp32 evaluation error {e32:.3e}, bound {max(8 * e32, 1e-6):.3e}, "
              f"ratio {e_op / max(8 * e32, 1e-6):.2f}")
    for n, e_op, e32 in rows:
        assert bool(torch.isfinite(got[n]).all()) and e_op <= max(8 * e32, 1e-6), f"model {n}: error {e_op:.3e} > max(8 x {e32:.3e}, 1e-6)"


def test_three_steps_of_the_run_loop_give_finite_losses():
    from oracle import lpm_oracle as O
    from learnablepoolingmethods_amd import FLAGS, registry, training
    from learnablepoolingmethods_amd.train import Trainer
    dev = cuda()
    Vn, B, MF = 20, 4, 8
    batches = []
    for i in range(3):
        x, nf, lab = O.make_synthetic_batch(B, MF, 1152, Vn, seed=50 + i, min_frames=MODEL["iterations"])
        batches.append((None, x.to(dev), lab.to(dev), nf.to(dev)))
    losses = []
    FLAGS.triangulation_v1_fused = True
    try:
        tr = Trainer(registry.get_model("JuhanTestModelV1"), vocab_size=Vn, batch_size=B, base_learning_rate=1e-3, device=dev, seed=3,
                     model_kwargs=MODEL)
        res = training.run(tr, iter(batches), log_every=1, log=lambda s: None, on_step=lambda out, batch: losses.append(float(out["loss"])))
    finally:
        FLAGS.reset()
    print(f"[triangulation v1] run loop losses {losses}")
    assert res["global_step"] == res["steps"] == 3 and len(losses) == 3 and all(math.isfinite(v) for v in losses)
