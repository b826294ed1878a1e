"""-m gpu: ops.triangulation_pool (csrc/triangulation_pool.hip) and RegularizedTriangulationModel against fp64 restatements on the CPU
(tests/_triangulation_ref.py) -- never against the op itself.

Tolerance of the op: the materialised formulas evaluated in fp32 torch on the CPU carry an error err32 against fp64 (maximum absolute
error over the maximum absolute reference, per tensor); the op's error must be <= max(8 err32, 1e-6) -- the 8 covers another summation
order over D and t and the hardware rsqrt.  A maximum whose fp64 runner-up lies within 1e-5 may route its gradient to another frame in
fp32: the upstream g_max_* is zeroed there for every side (at most 1 % of positions); the forward maxima are compared everywhere."""
import functools
import math

import pytest
import torch

from tests import _triangulation_ref as R
from tests._util import cuda

pytestmark = pytest.mark.gpu

SHAPES = [  # B, T, D, K, scale
    (3, 2, 128, 1, 1.0),                     # one temporal difference, one anchor
    (3, 7, 128, 5, 1 / math.sqrt(5)),        # odd T, odd K
    (2, 33, 1024, 3, 1.0),                   # video width
    (2, 40, 128, 64, 1 / 8),                 # the default anchor count
    (1, 300, 1024, 4, 1.0),                  # the full frame walk
]
NAMES = ("max_d", "mean_d", "max_t", "mean_t")


def _err(a, ref, scale=None):
    ref = ref.double()
    s = float(ref.abs().max()) if scale is None else scale
    return float((a.detach().double().cpu() - ref).abs().max()) / max(s, 1e-300)


def _reference(x, anchors, T, s, upstream):
    """fp64 values / gradients, the fp32 CPU evaluation's errors against them, and the upstream gradients with near-ties zeroed."""
    ties = R.near_ties(x.double(), anchors.double(), T, s)
    up = [g.clone() for g in upstream]
    up[0][ties[0]] = 0.0
    up[2][ties[1]] = 0.0
    share = max(float(t.float().mean()) for t in ties)
    o64, dx64, da64 = R.pool_and_grads(x.double(), anchors.double(), T, s, [g.double() for g in up])
    o32, dx32, da32 = R.pool_and_grads(x, anchors, T, s, up)
    return dict(up=up, share=share, o64=o64, dx64=dx64, da64=da64, o32=o32, dx32=dx32, da32=da32)


@functools.lru_cache(maxsize=None)
def _random_case(B, T, D, K, s, seed):
    x, anchors, upstream = R.make_inputs(B, T, D, K, seed)
    return x, anchors, _reference(x, anchors, T, s, upstream)


def _run_op(x, anchors, T, s, upstream, dev):
    from learnablepoolingmethods_amd import ops
    xg = x.to(dev).requires_grad_(True)
    ag = anchors.to(dev).requires_grad_(True)
    outs = ops.triangulation_pool(xg, ag, T, scale=s)
    loss = sum((o * g.to(dev)).sum() for o, g in zip(outs, upstream))
    dx, da = torch.autograd.grad(loss, [xg, ag])
    return outs, dx, da


def _check(tag, outs, dx, da, ref, grad_scale=None):
    """Every figure is printed before anything is asserted."""
    rows = []
    for n, o, o64, o32 in zip(NAMES, outs, ref["o64"], ref["o32"]):
        rows.append((n, _err(o, o64), _err(o32, o64)))
    rows.append(("dx", _err(dx, ref["dx64"], grad_scale), _err(ref["dx32"], ref["dx64"], grad_scale)))
    rows.append(("danchors", _err(da, ref["da64"], grad_scale), _err(ref["da32"], ref["da64"], grad_scale)))
    for n, e_op, e32 in rows:
        print(f"[triangulation] {tag} {n}: op error {e_op:.3e}, fp32 evaluation error {e32:.3e}, bound {max(8 * e32, 1e-6):.3e}")
    print(f"[triangulation] {tag} near-tie share {ref['share']:.4%}")
    assert ref["share"] <= 0.01, f"{tag}: {ref['share']:.3%} of the maxima are near-ties"
    for n, e_op, e32 in rows:
        assert math.isfinite(e_op) and e_op <= max(8 * e32, 1e-6), f"{tag} {n}: op error {e_op:.3e} > max(8 x {e32:.3e}, 1e-6)"


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("B,T,D,K,s", SHAPES)
def test_op_matches_fp64(B, T, D, K, s, seed):
    dev = cuda()
    x, anchors, ref = _random_case(B, T, D, K, s, seed)
    outs, dx, da = _run_op(x, anchors, T, s, ref["up"], dev)
    assert all(o.shape == (B, K * D) for o in outs) and dx.shape == x.shape and da.shape == anchors.shape
    _check(f"({B},{T},{D},{K}) seed {seed}", outs, dx, da, ref)


# The backward's other paths (csrc/triangulation_pool.hip): a workgroup takes eight anchors per round; G = min(rounds, clamp(ceil(256 / B), 1, 8))
# groups per clip write dx partials that a second pass adds; a group with more than one round adds onto what it wrote itself.
BACKWARD_PATHS = [  # B, T, D, K, scale
    (1, 5, 128, 70, 1.0),                    # 9 rounds in 8 groups: group 0 takes two rounds, the second with six anchors
    (2, 4, 1024, 20, 0.5),                   # three groups, the last with four anchors; the partial sum pass at the video width
    (1, 3, 1024, 70, 1.0),                   # two rounds in one group at the video width
    (256, 2, 128, 9, 1 / 3),                 # one group per clip, two rounds: straight into dx, no second pass
]


@pytest.mark.parametrize("B,T,D,K,s", BACKWARD_PATHS)
def test_op_matches_fp64_on_every_backward_path(B, T, D, K, s):
    dev = cuda()
    x, anchors, ref = _random_case(B, T, D, K, s, 4)
    outs, dx, da = _run_op(x, anchors, T, s, ref["up"], dev)
    _check(f"({B},{T},{D},{K}) seed 4", outs, dx, da, ref)


def test_frame_equal_to_an_anchor():
    """q = 0: the clamped first normalisation gives e = 0 for that (frame, anchor); the gradient carries the reference's own 1e6."""
    dev = cuda()
    B, T, D, K, s = 2, 6, 128, 3, 1.0
    x, anchors, upstream = R.make_inputs(B, T, D, K, 5)
    x[T + 2] = anchors[:, 1]                                    # clip 1, frame 2 sits on anchor 1
    ref = _reference(x, anchors, T, s, upstream)
    e64, _ = R.embeddings(x.double(), anchors.double(), T, s)
    assert float(e64[1, 2, D:2 * D].abs().max()) == 0.0
    outs, dx, da = _run_op(x, anchors, T, s, ref["up"], dev)
    _check("frame == anchor", outs, dx, da, ref, grad_scale=float(ref["dx64"].abs().max()))


# s = 1/3: a scale that is no power of two -- s eh must be rounded before the difference is taken (no product fused into it), or u is
# the rounding error of s eh instead of zero and f, behind the clamped 1e6, something of the order of 1e-3
@pytest.mark.parametrize("B,T,D,K,s", [(2, 6, 128, 3, 1.0), (2, 6, 128, 3, 1 / 3), (1, 4, 1024, 2, 1 / 3)])
def test_identical_consecutive_frames(B, T, D, K, s):
    """p = 0: f = 0 for that frame pair, and e ties exactly between the two frames -- the first index wins on every side."""
    dev = cuda()
    x, anchors, upstream = R.make_inputs(B, T, D, K, 6)
    x[3] = x[2]                                                 # clip 0: frames 2 and 3 identical
    ref = _reference(x, anchors, T, s, upstream)
    e64, f64 = R.embeddings(x.double(), anchors.double(), T, s)
    assert float(f64[0, 2].abs().max()) == 0.0 and torch.equal(e64[0, 2], e64[0, 3])
    tied = (R.first_max(e64)[1][0] == 2)
    assert bool(tied.any()), "the case must contain an exact tie of the maximum"
    outs, dx, da = _run_op(x, anchors, T, s, ref["up"], dev)
    print(f"[triangulation] identical frames: max |dx| {float(ref['dx64'].abs().max()):.3e}, median |dx| {float(ref['dx64'].abs().median()):.3e}")
    _check("identical frames", outs, dx, da, ref, grad_scale=float(ref["dx64"].abs().max()))


def test_two_calls_give_the_same_bits():
    dev = cuda()
    x, anchors, upstream = R.make_inputs(3, 20, 1024, 20, 11)
    a = _run_op(x, anchors, 20, 0.5, upstream, dev)
    b = _run_op(x, anchors, 20, 0.5, upstream, dev)
    for u, v in zip([*a[0], a[1], a[2]], [*b[0], b[1], b[2]]):
        assert torch.equal(u, v)


def test_nothing_of_size_T_K_D_is_allocated():
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    B, T, D, K = 4, 300, 1024, 64
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B * T, D, generator=g).to(dev).requires_grad_(True)
    anchors = (torch.randn(D, K, generator=g) / 8).to(dev).requires_grad_(True)
    up = [torch.randn(B, K * D, generator=g).to(dev) for _ in range(4)]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    outs = ops.triangulation_pool(x, anchors, T, scale=1 / 8)
    torch.autograd.backward(outs, up)
    torch.cuda.synchronize()
    delta = torch.cuda.max_memory_allocated() - base
    one = 4 * B * T * K * D
    print(f"[triangulation] peak allocation over forward + backward {delta / 2**20:.1f} MiB; one [B,T,K*D] tensor {one / 2**20:.1f} MiB")
    assert delta < one // 4
    assert bool(torch.isfinite(x.grad).all()) and bool(torch.isfinite(anchors.grad).all())


def test_refusals_come_before_any_launch(lib):
    from learnablepoolingmethods_amd import _capi, ops
    dev = cuda()
    a128 = torch.randn(128, 4, device=dev)
    with pytest.raises(_capi.LpmError):
        ops.triangulation_pool(torch.randn(5, 128, device=dev), a128, 1)                       # T = 1
    with pytest.raises(_capi.LpmError):
        ops.triangulation_pool(torch.randn(8, 96, device=dev), torch.randn(96, 4, device=dev), 4)   # D = 96
    with pytest.raises(_capi.LpmError):
        ops.triangulation_pool(torch.randn(8, 256, device=dev)[:, :128], a128, 4)               # non-contiguous x
    # the C entry point itself refuses as well, with its error codes
    x = torch.randn(8, 128, device=dev)
    outs = [torch.empty(8, 4 * 128, device=dev) for _ in range(4)]
    idx = torch.empty(8, 4 * 128, dtype=torch.int32, device=dev)
    p = _capi.ptr

    def fwd(B, T, D, K):
        return lib._lpm_triangulation_pool_fwd(p(x), p(a128), B, T, D, K, 1.0, *(p(o) for o in outs), p(idx), _capi.stream_ptr())
    assert fwd(8, 1, 128, 4) == -2 and "frames" in lib.last_error()         # LPM_ERR_UNSUPPORTED_SHAPE
    assert fwd(2, 4, 96, 4) == -2
    assert fwd(0, 4, 128, 4) == -1                                          # LPM_ERR_BADARG
    assert fwd(2, 4, 128, 4) == 0
    torch.cuda.synchronize()


def test_module_path_on_the_gpu_meets_the_same_bound():
    """The materialising modules (the path FLAGS.triangulation_fused = False takes) on the GPU, held to the op's bound against the same
    fp64 yardstick: the two paths then agree with each other within twice the op tolerance."""
    from learnablepoolingmethods_amd import aggregation_modules, variables as vs, video_pooling_modules as M
    dev = cuda()
    B, T, D, K = 3, 7, 128, 5
    s = 1 / math.sqrt(K)
    x, anchors, ref = _random_case(B, T, D, K, s, 0)
    xg = x.to(dev).requires_grad_(True)
    store = vs.VariableStore(device=dev)
    ag = store.vars["anchor_weights"] = anchors.to(dev).requires_grad_(True)      # the variable exists already, with the case's values
    store.trainable["anchor_weights"] = True
    with vs.use_store(store):
        emb, det_reg = M.WeightedTriangulationEmbedding(D, T, K, None, True).forward(xg)
        tmp = M.TriangulationTemporalEmbedding(D, T, K, None, True).forward(emb)
    pool = aggregation_modules.MaxMeanPoolingModule(l2_normalize=False)
    agg_d, agg_t = pool.forward(emb), pool.forward(tmp)
    n = K * D
    outs = [agg_d[:, :n], agg_d[:, n:], agg_t[:, :n], agg_t[:, n:]]
    loss = sum((o * g.to(dev)).sum() for o, g in zip(outs, ref["up"]))
    dx, da = torch.autograd.grad(loss, [xg, ag])
    assert float(det_reg) == 0.0
    _check("module path (3,7,128,5)", outs, dx, da, ref)


def test_regularized_triangulation_model_step_matches_fp64():
    """RegularizedTriangulationModel at tiny sizes (vocab 40, anchors 4 / 2, 12 sampled frames, B = 6), frame draws and dropout masks
    handed in: predictions, loss, raw and clipped gradients and the variables after one Trainer step against the fp64 restatement
    (tests/_triangulation_ref.model_loss), at the project's model-level 1e-3 as for WillowModelReg (tests/test_gpu_models.py).
    Gradients: Frobenius norm per variable with the floor used there -- the betas of the three *_projection_bn feed a second batch norm
    that removes them, their gradient is mathematically zero.  Variables after the step: Adam's first step moves an element by
    lr * sign(g), so, as in tests/test_gpu_models._train_compare, the update is compared where the sign is well defined."""
    from oracle import lpm_oracle as O
    from learnablepoolingmethods_amd import FLAGS, registry
    from learnablepoolingmethods_amd.train import Trainer
    from tests._util import assert_close, rel_l2
    dev = cuda()
    V, KV, KA, S, B, MF, lr = 40, 4, 2, 12, 6, 16, 1e-3
    x, nf, lab = O.make_synthetic_batch(B, MF, 1152, V, seed=21, min_frames=S)
    g = torch.Generator().manual_seed(22)
    # draws WITHOUT repeats (a random permutation of each clip's frames): SampleRandomFrames draws with replacement, and the same frame
    # twice in a row is the p = 0 case -- the reference's own 1e6 amplification, +-1e4 terms that cancel in danchors, 1e-1 off in ANY fp32
    # evaluation (the op-level case test_identical_consecutive_frames holds the kernel to fp64 there, relative to max |dx|)
    u = torch.stack([(torch.randperm(int(n), generator=g)[:S].float() + 0.5) / float(n) for n in nf])
    masks = {"fc1": torch.rand(B, V, generator=g) < 0.5, "fc2": torch.rand(B, V, generator=g) < 0.5}
    tr = Trainer(registry.get_model("RegularizedTriangulationModel"), vocab_size=V, batch_size=B, base_learning_rate=lr, device=dev, seed=3,
                 model_kwargs=dict(iterations=S, video_anchor_size=KV, audio_anchor_size=KA, frame_uniform=u, dropout_masks=masks))
    tr.build(x, nf, lab)
    shapes = R.model_variable_shapes(V, KV, KA)
    assert {n: tuple(v.shape) for n, v in tr.store.vars.items()} == {"tower/" + n: s for n, s in shapes.items()}
    p = {n[len("tower/"):]: v.detach().double().cpu() for n, v in tr.store.vars.items()}
    names = [n for n in p if R.is_trainable(n)]
    for n in names:
        p[n].requires_grad_(True)
    pred, label_loss, final = R.model_loss(p, x.double(), nf, lab, u, masks, S, l1=FLAGS.wtm_projection_l1, l2=FLAGS.wtm_projection_l2)
    grads = dict(zip(names, torch.autograd.grad(final, [p[n] for n in names])))
    gscale = max(float(v.abs().max()) for v in grads.values())
    clipped = O.clip_gradient_norms(grads, 1.0)

    # the module path predicts what the fused path predicts (inference mode: same variables, moving statistics)
    fused_pred = tr.predict(x, nf, frame_uniform=u)
    FLAGS.triangulation_fused = False
    try:
        module_pred = tr.predict(x, nf, frame_uniform=u)
    finally:
        FLAGS.reset()
    print(f"[triangulation] model: fused vs module predictions {float((fused_pred - module_pred).abs().max()):.3e}")
    assert_close(fused_pred, module_pred.double().cpu(), tol=1e-5, what="fused vs module path predictions")

    out = tr.step(x, nf, lab)
    e_loss = assert_close(out["loss"], label_loss.detach(), tol=1e-4, what="loss")
    e_pred = assert_close(out["predictions"], pred.detach(), what="predictions")
    print(f"[triangulation] model: loss error {e_loss:.3e}, predictions error {e_pred:.3e}")
    for n in names:
        raw = tr.gradient("tower/" + n).detach().double().cpu()
        floor = 1e-4 * gscale * grads[n].numel() ** 0.5
        e_raw = rel_l2(raw, grads[n], floor=floor)
        e_clip = rel_l2(O.clip_gradient_norms({n: raw}, 1.0)[n], clipped[n], floor=floor)
        ref_new, _, _ = O.adam_tf_update(p[n].detach(), clipped[n], torch.zeros_like(clipped[n]), torch.zeros_like(clipped[n]), lr, 1)
        got = tr.store.vars["tower/" + n].detach().double().cpu()
        mask = grads[n].abs() > max(1e-3 * float(grads[n].abs().max()), 1e-4 * gscale)
        e_upd = rel_l2((got - p[n].detach())[mask], (ref_new - p[n].detach())[mask]) if bool(mask.any()) else 0.0
        print(f"[triangulation] model {n}: gradient {e_raw:.3e}, clipped {e_clip:.3e}, update {e_upd:.3e} on {int(mask.sum())} of {mask.numel()}")
        assert e_raw <= 1e-3 and e_clip <= 1e-3, f"gradient {n}: relative L2 error {e_raw:.3e} (clipped {e_clip:.3e})"
        assert e_upd <= 1e-3, f"variable {n} after one step: relative L2 error of the update {e_upd:.3e}"
