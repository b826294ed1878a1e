"""-m gpu: ops.triangulation_attention_pool (csrc/triangulation_attention.hip) and SoftAttentionTriangulationModel against fp64
restatements on the CPU (tests/_soft_attention_ref.py) -- never against the op itself.

Tolerance of the op (the rule of tests/test_gpu_triangulation.py): the materialised formulas evaluated in fp32 torch on the CPU carry an
error err32 against fp64 (maximum absolute error over the maximum absolute reference, per tensor); the op's error must be
<= max(8 err32, 1e-6).  Two conditions keep that comparison meaningful; every test asserts them on its own inputs before any launch:
(a) a maximum whose fp64 runner-up lies within 1e-5 may route its gradient to another frame in fp32: the upstream g_max_* is zeroed
    there for every side (at most 1 % of positions); the forward maxima are compared everywhere;
(b) no Gram entry of the fp64 restatement, either kind, lies within 1e-5 of zero: a relu mask that flips between fp32 and fp64 moves
    dx by far more than the tolerance and says nothing about the kernel."""
import functools
import math

import pytest
import torch

from tests import _soft_attention_ref as S
from tests import _triangulation_ref as R
from tests._util import cuda

pytestmark = pytest.mark.gpu

REACH = 1e-5


def _err(a, ref, scale=None):
    ref = ref.double()
    s = float(ref.abs().max()) if scale is None else scale
    return float((a.detach().double().cpu() - ref).abs().max()) / max(s, 1e-300)


def _reference(x, anchors, T, upstream, no_gram_gradient=False, nonzero_only=False):
    """fp64 values / gradients, the fp32 CPU evaluation's errors against them, the upstream gradients with near-ties zeroed (and, with
    ``no_gram_gradient``, the two mean gradients zeroed), the near-tie share and the smallest |G|."""
    ties = R.near_ties(x.double(), anchors.double(), T, 1.0, reach=REACH)
    up = [g.clone() for g in upstream]                      # order: mean_d, max_d, mean_t, max_t
    up[1][ties[0]] = 0.0
    up[3][ties[1]] = 0.0
    if no_gram_gradient:
        up[0].zero_()
        up[2].zero_()
    share = max(float(t.float().mean()) for t in ties)
    smallest = S.near_zero_gram(x.double(), anchors.double(), T, REACH, nonzero_only=nonzero_only)
    o64, dx64, da64 = S.pool_and_grads(x.double(), anchors.double(), T, [g.double() for g in up])
    o32, dx32, da32 = S.pool_and_grads(x, anchors, T, up)
    return dict(up=up, share=share, smallest=smallest, o64=o64, dx64=dx64, da64=da64, o32=o32, dx32=dx32, da32=da32)


@functools.lru_cache(maxsize=None)
def _random_case(B, T, D, K, seed, no_gram_gradient=False):
    x, anchors, upstream = S.make_inputs(B, T, D, K, seed)
    return x, anchors, _reference(x, anchors, T, upstream, no_gram_gradient)


def _conditions(tag, ref, gram_condition=True):
    print(f"[soft attention] {tag} near-tie share {ref['share']:.4%}, smallest |G| {ref['smallest']:.3e}")
    assert ref["share"] <= 0.01, f"{tag}: {ref['share']:.3%} of the maxima are near-ties"
    if gram_condition:
        assert ref["smallest"] >= REACH, f"{tag}: a Gram entry lies within {REACH} of zero ({ref['smallest']:.3e})"


def _run_op(x, anchors, T, upstream, dev):
    from learnablepoolingmethods_amd import ops
    xg = x.to(dev).requires_grad_(True)
    ag = anchors.to(dev).requires_grad_(True)
    outs = ops.triangulation_attention_pool(xg, ag, T)
    loss = sum((o * g.to(dev)).sum() for o, g in zip(outs, upstream))
    dx, da = torch.autograd.grad(loss, [xg, ag])
    return outs, dx, da


def _check(tag, outs, dx, da, ref, grad_scale=None):
    """Every figure is printed before anything is asserted."""
    rows = []
    for n, o, o64, o32 in zip(S.NAMES, outs, ref["o64"], ref["o32"]):
        rows.append((n, _err(o, o64), _err(o32, o64)))
    rows.append(("dx", _err(dx, ref["dx64"], grad_scale), _err(ref["dx32"], ref["dx64"], grad_scale)))
    rows.append(("danchors", _err(da, ref["da64"], grad_scale), _err(ref["da32"], ref["da64"], grad_scale)))
    for n, e_op, e32 in rows:
        print(f"[soft attention] {tag} {n}: op error {e_op:.3e}, fp32 evaluation error {e32:.3e}, bound {max(8 * e32, 1e-6):.3e}")
    for n, e_op, e32 in rows:
        assert math.isfinite(e_op) and e_op <= max(8 * e32, 1e-6), f"{tag} {n}: op error {e_op:.3e} > max(8 x {e32:.3e}, 1e-6)"


SHAPES = [  # B, T, D, K
    (3, 2, 128, 1),                          # one difference: the temporal Gram is 1x1
    (3, 7, 128, 5),                          # odd everything
    (2, 33, 1024, 3),                        # video width
    (2, 64, 128, 16),                        # the audio stream's defaults, a full 64 tile
    (1, 70, 128, 4),                         # T crosses a 64 tile with a remainder of 6; the temporal kind has 69
]


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("B,T,D,K", SHAPES)
def test_op_matches_fp64(B, T, D, K, seed):
    dev = cuda()
    x, anchors, ref = _random_case(B, T, D, K, seed)
    tag = f"({B},{T},{D},{K}) seed {seed}"
    _conditions(tag, ref)
    outs, dx, da = _run_op(x, anchors, T, ref["up"], dev)
    assert all(o.shape == (B, K * D) for o in outs) and dx.shape == x.shape and da.shape == anchors.shape
    _check(tag, outs, dx, da, ref)


@pytest.mark.parametrize("seed", [3, 5, 7])                 # (seeds 0 to 2 fail condition (b) at this shape)
def test_op_matches_fp64_over_three_tiles_with_a_remainder(seed):
    dev = cuda()
    B, T, D, K = 1, 130, 128, 2
    x, anchors, ref = _random_case(B, T, D, K, seed)
    tag = f"({B},{T},{D},{K}) seed {seed}"
    _conditions(tag, ref)
    outs, dx, da = _run_op(x, anchors, T, ref["up"], dev)
    _check(tag, outs, dx, da, ref)


def test_op_matches_fp64_on_the_full_frame_walk():
    """T = 300: no seed of twelve keeps every Gram entry 1e-5 away from zero at this size, so the four forward outputs are compared
    everywhere and the gradients with g_mean_d = g_mean_t = 0: the Gram then carries no gradient, and the max route walks all 300
    frames (M = 0 goes through the same matrix products)."""
    dev = cuda()
    B, T, D, K = 1, 300, 128, 2
    x, anchors, ref = _random_case(B, T, D, K, 0, True)
    tag = f"({B},{T},{D},{K}) seed 0, no mean gradient"
    _conditions(tag, ref, gram_condition=False)
    outs, dx, da = _run_op(x, anchors, T, ref["up"], dev)
    _check(tag, outs, dx, da, ref)


# The backward's other paths (csrc/triangulation_attention.hip): G = min(K, clamp(floor(512 / B), 1, 16)) workgroups per clip take the
# anchors g, g + G, ... in turn, each adding onto the [T, D] block it wrote itself; with G > 1 a second pass adds the groups' blocks.
# The Gram's anchor slices: S = min(K, clamp(ceil(512 / (B tiles^2)), 1, 16)), added by a second pass when S > 1.
# Conditions (a) and (b) were checked on the CPU for each of these first (seed 4: smallest |G| 1.5e-3 for the two wide batches, 0.18 and
# 0.37 for the others; near-tie share at most 0.03 %).
PARTITION_PATHS = [  # B, T, D, K
    (1, 5, 128, 70),                         # 16 groups and 16 Gram slices with 5 or 4 anchors each
    (2, 4, 1024, 20),                        # 16 groups with 2 anchors or 1 at the video width
    (256, 2, 128, 9),                        # 2 groups with 5 and 4 anchors, 2 Gram slices
    (600, 2, 128, 3),                        # one group and one Gram slice per clip: straight into dx and G, no second pass
]


@pytest.mark.parametrize("B,T,D,K", PARTITION_PATHS)
def test_op_matches_fp64_on_every_anchor_partition_path(B, T, D, K):
    dev = cuda()
    x, anchors, ref = _random_case(B, T, D, K, 4)
    tag = f"({B},{T},{D},{K}) seed 4"
    _conditions(tag, ref)
    outs, dx, da = _run_op(x, anchors, T, ref["up"], dev)
    _check(tag, outs, dx, da, ref)


def test_frame_equal_to_an_anchor():
    """q = 0: the clamped first normalisation gives e = 0 for that (frame, anchor); the gradient carries the reference's own 1e6."""
    dev = cuda()
    B, T, D, K = 2, 6, 128, 3
    x, anchors, upstream = S.make_inputs(B, T, D, K, 5)
    x[T + 2] = anchors[:, 1]                                    # clip 1, frame 2 sits on anchor 1
    ref = _reference(x, anchors, T, upstream)
    e64, _ = R.embeddings(x.double(), anchors.double(), T, 1.0)
    assert float(e64[1, 2, D:2 * D].abs().max()) == 0.0
    _conditions("frame == anchor", ref)
    outs, dx, da = _run_op(x, anchors, T, ref["up"], dev)
    _check("frame == anchor", outs, dx, da, ref, grad_scale=float(ref["dx64"].abs().max()))


def test_identical_consecutive_frames():
    """p = 0: f = 0 for that frame pair -- a row and a column of exact zeros in G_t, relu'(0) = 0 on every side (condition (b) is
    asserted over the non-zero entries) -- and e ties exactly between the two frames: the first index wins on every side."""
    dev = cuda()
    B, T, D, K = 2, 6, 128, 3
    x, anchors, upstream = S.make_inputs(B, T, D, K, 6)
    x[3] = x[2]                                                 # clip 0: frames 2 and 3 identical
    ref = _reference(x, anchors, T, upstream, nonzero_only=True)
    e64, f64 = R.embeddings(x.double(), anchors.double(), T, 1.0)
    assert float(f64[0, 2].abs().max()) == 0.0 and torch.equal(e64[0, 2], e64[0, 3])
    assert float(S.gram(f64)[0, 2].abs().max()) == 0.0
    assert bool((R.first_max(e64)[1][0] == 2).any()), "the case must contain an exact tie of the maximum"
    _conditions("identical frames", ref)
    outs, dx, da = _run_op(x, anchors, T, ref["up"], dev)
    print(f"[soft attention] identical frames: max |dx| {float(ref['dx64'].abs().max()):.3e}, median |dx| {float(ref['dx64'].abs().median()):.3e}")
    _check("identical frames", outs, dx, da, ref, grad_scale=float(ref["dx64"].abs().max()))


@pytest.mark.parametrize("B,T,D,K,seed", [(2, 33, 1024, 3, 0), (1, 130, 128, 2, 3), (1, 300, 128, 2, 0)])
def test_gram_matches_fp64(B, T, D, K, seed):
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    x, anchors, _ = S.make_inputs(B, T, D, K, seed)
    g64 = S.grams(x.double(), anchors.double(), T)
    g32 = S.grams(x, anchors, T)
    got = ops.triangulation_attention_gram(x.to(dev), anchors.to(dev), T)
    rows = [(n, _err(g, r64), _err(r32, r64)) for n, g, r64, r32 in zip(("G_d", "G_t"), got, g64, g32)]
    for n, e_op, e32 in rows:
        print(f"[soft attention] ({B},{T},{D},{K}) {n}: op error {e_op:.3e}, fp32 evaluation error {e32:.3e}, bound {max(8 * e32, 1e-6):.3e}")
    assert got[0].shape == (B, T, T) and got[1].shape == (B, T - 1, T - 1)
    for n, e_op, e32 in rows:
        assert e_op <= max(8 * e32, 1e-6), f"{n}: op error {e_op:.3e} > max(8 x {e32:.3e}, 1e-6)"


def test_two_calls_give_the_same_bits():
    dev = cuda()
    x, anchors, upstream = S.make_inputs(3, 20, 1024, 20, 11)
    a = _run_op(x, anchors, 20, upstream, dev)
    b = _run_op(x, anchors, 20, upstream, dev)
    for u, v in zip([*a[0], a[1], a[2]], [*b[0], b[1], b[2]]):
        assert torch.equal(u, v)


def test_nothing_of_size_T_K_D_is_allocated():
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    B, T, D, K = 16, 64, 1024, 128
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B * T, D, generator=g).to(dev).requires_grad_(True)
    anchors = R.l2n(torch.randn(D, K, generator=g), 0).to(dev).requires_grad_(True)
    up = [torch.randn(B, K * D, generator=g).to(dev) for _ in range(4)]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    outs = ops.triangulation_attention_pool(x, anchors, T)
    torch.autograd.backward(outs, up)
    torch.cuda.synchronize()
    delta = torch.cuda.max_memory_allocated() - base
    one = 4 * B * T * K * D
    print(f"[soft attention] peak allocation over forward + backward {delta / 2**20:.1f} MiB; one [B,T,K*D] tensor {one / 2**20:.1f} MiB")
    assert delta < one // 4
    assert bool(torch.isfinite(x.grad).all()) and bool(torch.isfinite(anchors.grad).all())


def test_refusals_come_before_any_launch(lib):
    from learnablepoolingmethods_amd import _capi, ops
    dev = cuda()
    most = lib._lpm_triangulation_attention_max_frames()
    assert most >= 300
    a128 = torch.randn(128, 4, device=dev)
    with pytest.raises(_capi.LpmError):
        ops.triangulation_attention_pool(torch.randn(5, 128, device=dev), a128, 1)                       # T = 1
    with pytest.raises(_capi.LpmError):
        ops.triangulation_attention_pool(torch.randn(8, 96, device=dev), torch.randn(96, 4, device=dev), 4)   # D = 96
    with pytest.raises(_capi.LpmError):
        ops.triangulation_attention_pool(torch.randn(8, 256, device=dev)[:, :128], a128, 4)               # non-contiguous x
    with pytest.raises(_capi.LpmError):
        ops.triangulation_attention_pool(torch.randn(0, 128, device=dev), a128, 4)                        # B = 0
    with pytest.raises(_capi.LpmError):
        ops.triangulation_attention_pool(torch.randn(most + 1, 128, device=dev), a128, most + 1)          # T above the supported maximum
    # the C entry points themselves refuse as well, with their error codes
    x = torch.randn(8, 128, device=dev)
    outs = [torch.empty(8, 4 * 128, device=dev) for _ in range(4)]
    idx = torch.empty(8, 4 * 128, dtype=torch.int32, device=dev)
    small = [torch.empty(64, device=dev) for _ in range(4)]
    ws = torch.empty(1 << 16, device=dev)
    p, st = _capi.ptr, _capi.stream_ptr

    def gram(B, T, D, K):
        return lib._lpm_triangulation_attention_gram(p(x), p(a128), B, T, D, K, 1.0, p(small[0]), p(small[1]), p(ws), ws.numel() * 4, st())

    def fwd(B, T, D, K):
        return lib._lpm_triangulation_attention_pool_fwd(p(x), p(a128), p(small[0]), p(small[1]), B, T, D, K, 1.0, *(p(o) for o in outs), p(idx), st())

    def dw(B, T, D, K):
        return lib._lpm_triangulation_attention_dw(p(x), p(a128), p(outs[0]), p(outs[2]), B, T, D, K, 1.0, p(small[0]), p(small[1]), p(ws),
                                                   ws.numel() * 4, st())

    def bwd(B, T, D, K):
        return lib._lpm_triangulation_attention_bwd(p(x), p(a128), p(idx), p(small[0]), p(small[1]), p(small[2]), p(small[3]),
                                                    *(p(o) for o in outs), B, T, D, K, 1.0, p(torch.empty_like(x)), p(torch.empty_like(a128)),
                                                    p(ws), ws.numel() * 4, st())
    for call in (gram, fwd, dw, bwd):
        assert call(8, 1, 128, 4) == -2 and "frames" in lib.last_error()         # LPM_ERR_UNSUPPORTED_SHAPE
        assert call(2, 4, 96, 4) == -2
        assert call(0, 4, 128, 4) == -1                                          # LPM_ERR_BADARG
        assert call(1, most + 1, 128, 4) == -2 and "frames" in lib.last_error()
    torch.cuda.synchronize()


def test_module_path_on_the_gpu_meets_the_same_bound():
    """The materialising modules (the path FLAGS.soft_attention_fused = False takes) on the GPU, held to the op's bound against the
    same fp64 yardstick: the two paths then agree with each other within twice the op tolerance."""
    from learnablepoolingmethods_amd import aggregation_modules, variables as vs, video_pooling_modules as M
    dev = cuda()
    B, T, D, K = 3, 7, 128, 5
    x, raw, upstream = R.make_inputs(B, T, D, K, 0)             # raw: the variable as initialised; the module normalises it itself
    ref = _reference(x, R.l2n(raw, 0), T, upstream)
    _conditions("module path (3,7,128,5)", ref)
    # danchors is taken with respect to the variable here: through l2_normalize(anchor_weights, 0) on every side
    for dt, key in ((torch.float64, "64"), (torch.float32, "32")):
        x_, a_ = x.to(dt).requires_grad_(True), raw.to(dt).requires_grad_(True)
        outs = S.pool(x_, R.l2n(a_, 0), T)
        ref["dx" + key], ref["da" + key] = torch.autograd.grad(sum((o * g.to(dt)).sum() for o, g in zip(outs, ref["up"])), [x_, a_])
    xg = x.to(dev).requires_grad_(True)
    store = vs.VariableStore(device=dev)
    ag = store.vars["anchor_weights"] = raw.to(dev).requires_grad_(True)          # the variable exists already, with the case's values
    store.trainable["anchor_weights"] = True
    with vs.use_store(store):
        emb = M.TriangulationEmbedding(D, T, K, None, True).forward(xg)
        tmp = M.TriangulationTemporalEmbedding(D, T, K, None, True).forward(emb)
    pool = aggregation_modules.IndirectClusterMaxMeanPoolModule(l2_normalize=False)
    agg_d, agg_t = pool.forward(emb.reshape(-1, T, K * D)), pool.forward(tmp)
    n = K * D
    outs = [agg_d[:, :n], agg_d[:, n:], agg_t[:, :n], agg_t[:, n:]]
    loss = sum((o * g.to(dev)).sum() for o, g in zip(outs, ref["up"]))
    dx, da = torch.autograd.grad(loss, [xg, ag])
    _check("module path (3,7,128,5)", outs, dx, da, ref)
    # ... and the op with the same variable
    xg2, ag2 = x.to(dev).requires_grad_(True), raw.to(dev).requires_grad_(True)
    from learnablepoolingmethods_amd import layers, ops
    outs2 = ops.triangulation_attention_pool(xg2, layers.l2_normalize(ag2, 0), T)
    dx2, da2 = torch.autograd.grad(sum((o * g.to(dev)).sum() for o, g in zip(outs2, ref["up"])), [xg2, ag2])
    _check("fused path, gradient of the variable (3,7,128,5)", outs2, dx2, da2, ref)


MODEL_BATCH_SEED = 29


def test_soft_attention_triangulation_model_step_matches_fp64():
    """SoftAttentionTriangulationModel at tiny sizes (vocab 40, anchors 4 / 2, bottlenecks 6 / 3, 12 sampled frames, B = 6), frame
    draws handed in WITHOUT repeats (the same frame twice in a row is the p = 0 case, see
    test_regularized_triangulation_model_step_matches_fp64): predictions, loss, raw and clipped gradients and the variables after one
    Trainer step against the fp64 restatement (tests/_soft_attention_ref.model_loss), at the project's model-level 1e-3 (1e-4 for the
    loss) with the floors of that test.  The variables come from a CPU build (seed 3), so that they do not depend on the device's
    generator; batch seed 29 (draws seed 30) was picked on the CPU among 21, 23, ..., 31: the fp64 restatement's smallest |G| over both streams and
    kinds is 2.01e-4 there (3.8e-5 to 8.3e-5 for the other five), and the test asserts that it is at least 1e-4."""
    from oracle import lpm_oracle as O
    from learnablepoolingmethods_amd import FLAGS, registry
    from learnablepoolingmethods_amd.train import Trainer
    from tests._util import assert_close, rel_l2
    dev = cuda()
    V, KV, KA, BV, BA, Sf, B, MF, lr = 40, 4, 2, 6, 3, 12, 6, 16, 1e-3
    x, nf, lab = O.make_synthetic_batch(B, MF, 1152, V, seed=MODEL_BATCH_SEED, min_frames=Sf)
    g = torch.Generator().manual_seed(MODEL_BATCH_SEED + 1)
    u = torch.stack([(torch.randperm(int(n), generator=g)[:Sf].float() + 0.5) / float(n) for n in nf])
    kwargs = dict(iterations=Sf, video_anchor_size=KV, audio_anchor_size=KA, video_bottleneck=BV, audio_bottleneck=BA, frame_uniform=u)
    host = Trainer(registry.get_model("SoftAttentionTriangulationModel"), vocab_size=V, batch_size=B, base_learning_rate=lr, device="cpu",
                   seed=3, model_kwargs=kwargs)
    host.build(x, nf, lab)
    tr = Trainer(registry.get_model("SoftAttentionTriangulationModel"), vocab_size=V, batch_size=B, base_learning_rate=lr, device=dev, seed=3,
                 model_kwargs=kwargs)
    tr.build(x, nf, lab)
    tr.load_state_dict(host.state_dict())
    shapes = S.model_variable_shapes(V, KV, KA, BV, BA)
    assert {n: tuple(v.shape) for n, v in tr.store.vars.items()} == {"tower/" + n: s for n, s in shapes.items()}
    p = {n[len("tower/"):]: v.detach().double().cpu() for n, v in tr.store.vars.items()}
    smallest = S.model_smallest_gram(p, x.double(), nf, u)
    print(f"[soft attention] model: smallest |G| over both streams and kinds {smallest:.3e}")
    assert smallest >= 1e-4
    names = [n for n in p if R.is_trainable(n)]
    for n in names:
        p[n].requires_grad_(True)
    pred, label_loss, final = S.model_loss(p, x.double(), nf, lab, u)
    grads = dict(zip(names, torch.autograd.grad(final, [p[n] for n in names])))
    gscale = max(float(v.abs().max()) for v in grads.values())
    clipped = O.clip_gradient_norms(grads, 1.0)

    # the module path predicts what the fused path predicts (inference mode: same variables, moving statistics)
    fused_pred = tr.predict(x, nf, frame_uniform=u)
    FLAGS.soft_attention_fused = False
    try:
        module_pred = tr.predict(x, nf, frame_uniform=u)
    finally:
        FLAGS.reset()
    print(f"[soft attention] model: fused vs module predictions {float((fused_pred - module_pred).abs().max()):.3e}")
    assert_close(fused_pred, module_pred.double().cpu(), tol=1e-5, what="fused vs module path predictions")

    out = tr.step(x, nf, lab)
    e_loss = assert_close(out["loss"], label_loss.detach(), tol=1e-4, what="loss")
    e_pred = assert_close(out["predictions"], pred.detach(), what="predictions")
    print(f"[soft attention] model: loss error {e_loss:.3e}, predictions error {e_pred:.3e}")
    for n in names:
        raw = tr.gradient("tower/" + n).detach().double().cpu()
        floor = 1e-4 * gscale * grads[n].numel() ** 0.5
        e_raw = rel_l2(raw, grads[n], floor=floor)
        e_clip = rel_l2(O.clip_gradient_norms({n: raw}, 1.0)[n], clipped[n], floor=floor)
        ref_new, _, _ = O.adam_tf_update(p[n].detach(), clipped[n], torch.zeros_like(clipped[n]), torch.zeros_like(clipped[n]), lr, 1)
        got = tr.store.vars["tower/" + n].detach().double().cpu()
        mask = grads[n].abs() > max(1e-3 * float(grads[n].abs().max()), 1e-4 * gscale)
        e_upd = rel_l2((got - p[n].detach())[mask], (ref_new - p[n].detach())[mask]) if bool(mask.any()) else 0.0
        print(f"[soft attention] model {n}: gradient {e_raw:.3e}, clipped {e_clip:.3e}, update {e_upd:.3e} on {int(mask.sum())} of {mask.numel()}")
        assert e_raw <= 1e-3 and e_clip <= 1e-3, f"gradient {n}: relative L2 error {e_raw:.3e} (clipped {e_clip:.3e})"
        assert e_upd <= 1e-3, f"variable {n} after one step: relative L2 error of the update {e_upd:.3e}"
