"""-m gpu: ops.triangulation_cnn_pool / ops.triangulation_mean_pool (csrc/triangulation_mean.hip) and TriangulationCnnClusterModel
against fp64 restatements on the CPU (tests/_triangulation_cnn_ref.py: project every frame, then pool) -- never against the op itself.

Tolerance of the op (the rule of tests/test_gpu_triangulation.py): the materialised formulas evaluated in fp32 torch on the CPU carry an
error err32 against fp64 (maximum absolute error over the maximum absolute reference, per tensor); the op's error must be
<= max(8 err32, 1e-6).  There are no maxima here, so one condition keeps that comparison meaningful; every test asserts it on its own
inputs before any launch: no G_d entry of the fp64 restatement lies within 1e-5 of zero (a relu mask that flips between fp32 and fp64
moves dx by far more than the tolerance and says nothing about the kernel)."""
import functools
import math

import pytest
import torch

from tests import _soft_attention_ref as S
from tests import _triangulation_cnn_ref as C
from tests import _triangulation_ref as R
from tests._util import cuda

pytestmark = pytest.mark.gpu

REACH = 1e-5
TENSORS = ("agg_d", "agg_t", "dx", "danchors", "dcnn_d", "dcnn_t", "m_d", "m_t")


def _err(a, ref, scale=None):
    ref = ref.double()
    s = float(ref.abs().max()) if scale is None else scale
    return float((a.detach().double().cpu() - ref).abs().max()) / max(s, 1e-300)


def _reference(x, anchors, T, F, seed):
    """fp64 values / gradients of the projected pooling and the inner op's two means, the same in fp32 on the CPU, the smallest |G_d|."""
    D, K = anchors.shape
    B = x.shape[0] // T
    cnn_d, cnn_t, up, _ = C.make_weights(B, D, K, F, seed)
    ref = dict(cnn_d=cnn_d, cnn_t=cnn_t, up=up, smallest=C.smallest_gram_d(x.double(), anchors.double(), T))
    for key, dt in (("64", torch.float64), ("32", torch.float32)):
        outs, grads = C.cnn_pool_and_grads(x.to(dt), anchors.to(dt), cnn_d.to(dt), cnn_t.to(dt), T, up)
        with torch.no_grad():
            means = C.mean_pool(x.to(dt), anchors.to(dt), T)
        ref[key] = dict(zip(TENSORS, [*outs, *grads, *means]))
    return ref


@functools.lru_cache(maxsize=None)
def _random_case(B, T, D, K, F, seed):
    x, anchors, _ = S.make_inputs(B, T, D, K, seed)
    return x, anchors, _reference(x, anchors, T, F, seed)


def _condition(tag, ref):
    print(f"[triangulation cnn] {tag} smallest |G_d| {ref['smallest']:.3e}")
    assert ref["smallest"] >= REACH, f"{tag}: a G_d entry lies within {REACH} of zero ({ref['smallest']:.3e})"


def _run_op(x, anchors, T, ref, dev):
    from learnablepoolingmethods_amd import ops
    leaves = [t.to(dev).requires_grad_(True) for t in (x, anchors, ref["cnn_d"], ref["cnn_t"])]
    outs = ops.triangulation_cnn_pool(*leaves, T)
    loss = sum((o * g.to(dev)).sum() for o, g in zip(outs, ref["up"]))
    grads = torch.autograd.grad(loss, leaves)
    with torch.no_grad():
        means = ops.triangulation_mean_pool(leaves[0].detach(), leaves[1].detach(), T)
    return dict(zip(TENSORS, [*outs, *grads, *means]))


def _check(tag, got, ref, grad_scale=None):
    """Every figure is printed before anything is asserted."""
    rows = []
    for n in TENSORS:
        scale = grad_scale if n == "dx" else None
        rows.append((n, _err(got[n], ref["64"][n], scale), _err(ref["32"][n], ref["64"][n], scale)))
    for n, e_op, e32 in rows:
        print(f"[triangulation cnn] {tag} {n}: op error {e_op:.3e}, fp32 evaluation error {e32:.3e}, bound {max(8 * e32, 1e-6):.3e}")
    for n, e_op, e32 in rows:
        assert math.isfinite(e_op) and e_op <= max(8 * e32, 1e-6), f"{tag} {n}: op error {e_op:.3e} > max(8 x {e32:.3e}, 1e-6)"


def _case_test(B, T, D, K, F, seed):
    dev = cuda()
    x, anchors, ref = _random_case(B, T, D, K, F, seed)
    tag = f"({B},{T},{D},{K}) F={F} seed {seed}"
    _condition(tag, ref)
    got = _run_op(x, anchors, T, ref, dev)
    assert got["agg_d"].shape == got["agg_t"].shape == (B, K * F) and got["m_d"].shape == got["m_t"].shape == (B, K * D)
    assert got["dx"].shape == x.shape and got["danchors"].shape == anchors.shape and got["dcnn_d"].shape == got["dcnn_t"].shape == (K, F, D)
    _check(tag, got, ref)


SHAPES = [  # B, T, D, K, F
    (3, 2, 128, 1, 1),                       # one difference
    (3, 7, 128, 5, 3),                       # odd everything
    (2, 33, 1024, 3, 8),                     # video width
    (2, 64, 128, 16, 16),                    # a full 64 tile (the last frame count of the backward's LDS-resident form)
    (1, 70, 128, 4, 5),                      # T crosses a 64 tile with a remainder of 6: three tile pairs, one of them off the diagonal
]


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("B,T,D,K,F", SHAPES)
def test_op_matches_fp64(B, T, D, K, F, seed):
    _case_test(B, T, D, K, F, seed)


@pytest.mark.parametrize("seed", [0, 2, 3])
def test_op_matches_fp64_over_three_tiles_with_a_remainder(seed):
    _case_test(1, 130, 128, 2, 4, seed)


@pytest.mark.parametrize("seed", [0, 3, 4])
def test_op_matches_fp64_at_the_models_default_frame_count(seed):
    _case_test(1, 200, 128, 2, 4, seed)


@pytest.mark.parametrize("seed", [5, 6])
def test_op_matches_fp64_on_the_full_frame_walk_with_all_gradients(seed):
    _case_test(1, 300, 128, 2, 3, seed)


# The anchor partitions (csrc/triangulation_mean.hip): the backward's G = min(K, clamp(floor(512 / B), 1, 16)) workgroups per clip take
# the anchors g, g + G, ... in turn, each adding onto the [T, D] block it wrote itself; with G > 1 a second pass adds the groups' blocks.
# The Gram's anchor slices: S = min(K, clamp(ceil(512 / (B pairs)), 1, 16)) with pairs = tiles (tiles + 1) / 2 (1 at these frame
# counts, as in triangulation_attention.hip), added by a second pass when S > 1.  Condition (b) was checked on the CPU for each of
# these first (seed 4: smallest |G_d| 3.7e-1, 1.8e-1, 1.5e-3, 1.6e-3).
PARTITION_PATHS = [  # B, T, D, K
    (1, 5, 128, 70),                         # 16 groups and 16 Gram slices with 5 or 4 anchors each (a partial last round)
    (2, 4, 1024, 20),                        # 16 groups and slices with 2 anchors or 1 at the video width
    (256, 2, 128, 9),                        # 2 groups with 5 and 4 anchors, 2 Gram slices
    (600, 2, 128, 3),                        # one group and one Gram slice per clip: straight into dx and G_d, no second pass
]


@pytest.mark.parametrize("B,T,D,K", PARTITION_PATHS)
def test_op_matches_fp64_on_every_anchor_partition_path(B, T, D, K):
    _case_test(B, T, D, K, 2, 4)


def test_frame_equal_to_an_anchor():
    """q = 0: the clamped first normalisation gives e = 0 for that (frame, anchor); the gradient carries the reference's own 1e6."""
    dev = cuda()
    B, T, D, K, F = 2, 6, 128, 3, 2
    x, anchors, _ = S.make_inputs(B, T, D, K, 5)
    x[T + 2] = anchors[:, 1]                                    # clip 1, frame 2 sits on anchor 1
    ref = _reference(x, anchors, T, F, 5)
    e64, _ = R.embeddings(x.double(), anchors.double(), T, 1.0)
    assert float(e64[1, 2, D:2 * D].abs().max()) == 0.0
    _condition("frame == anchor", ref)
    got = _run_op(x, anchors, T, ref, dev)
    _check("frame == anchor", got, ref, grad_scale=float(ref["64"]["dx"].abs().max()))


def test_identical_consecutive_frames():
    """p = 0: f = 0 for that frame pair, which adds nothing to m_t; dx stays finite and within the bound relative to max |dx|."""
    dev = cuda()
    B, T, D, K, F = 2, 6, 128, 3, 2
    x, anchors, _ = S.make_inputs(B, T, D, K, 6)
    x[3] = x[2]                                                 # clip 0: frames 2 and 3 identical
    ref = _reference(x, anchors, T, F, 6)
    e64, f64 = R.embeddings(x.double(), anchors.double(), T, 1.0)
    assert float(f64[0, 2].abs().max()) == 0.0 and torch.equal(e64[0, 2], e64[0, 3])
    rest = torch.cat([f64[0, :2], f64[0, 3:]]).sum(dim=0) / (T - 1)
    assert float((ref["64"]["m_t"][0] - rest).abs().max()) < 1e-15, "the zero difference contributes nothing to m_t"
    _condition("identical frames", ref)
    got = _run_op(x, anchors, T, ref, dev)
    print(f"[triangulation cnn] identical frames: max |dx| {float(ref['64']['dx'].abs().max()):.3e}, median |dx| {float(ref['64']['dx'].abs().median()):.3e}")
    assert bool(torch.isfinite(got["dx"]).all())
    _check("identical frames", got, ref, grad_scale=float(ref["64"]["dx"].abs().max()))


@pytest.mark.parametrize("B,T,D,K,seed", [(2, 33, 1024, 3, 0), (1, 130, 128, 2, 0), (1, 300, 128, 2, 5)])
def test_gram_matches_fp64(B, T, D, K, seed):
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    x, anchors, _ = S.make_inputs(B, T, D, K, seed)
    g64 = C.gram_d(x.double(), anchors.double(), T)
    g32 = C.gram_d(x, anchors, T)
    got = ops.triangulation_mean_gram(x.to(dev), anchors.to(dev), T)
    e_op, e32 = _err(got, g64), _err(g32, g64)
    print(f"[triangulation cnn] ({B},{T},{D},{K}) G_d: op error {e_op:.3e}, fp32 evaluation error {e32:.3e}, bound {max(8 * e32, 1e-6):.3e}")
    assert got.shape == (B, T, T)
    assert e_op <= max(8 * e32, 1e-6), f"G_d: op error {e_op:.3e} > max(8 x {e32:.3e}, 1e-6)"
    assert torch.equal(got, got.transpose(1, 2)), "a tile pair is written to both places"


def test_two_calls_give_the_same_bits():
    dev = cuda()
    B, T, D, K, F = 3, 20, 1024, 20, 4
    x, anchors, _ = S.make_inputs(B, T, D, K, 11)
    cnn_d, cnn_t, up, _ = C.make_weights(B, D, K, F, 11)
    ref = dict(cnn_d=cnn_d, cnn_t=cnn_t, up=up)
    a = _run_op(x, anchors, T, ref, dev)
    b = _run_op(x, anchors, T, ref, dev)
    for n in TENSORS:
        assert torch.equal(a[n], b[n]), n


def test_nothing_of_size_T_K_D_is_allocated():
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    B, T, D, K, F = 16, 64, 1024, 128, 16
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B * T, D, generator=g).to(dev).requires_grad_(True)
    anchors = R.l2n(torch.randn(D, K, generator=g), 0).to(dev).requires_grad_(True)
    cnn = [(torch.randn(K, F, D, generator=g) / math.sqrt(F * D)).to(dev).requires_grad_(True) for _ in range(2)]
    up = [torch.randn(B, K * F, generator=g).to(dev) for _ in range(2)]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    outs = ops.triangulation_cnn_pool(x, anchors, cnn[0], cnn[1], T)
    torch.autograd.backward(outs, up)
    torch.cuda.synchronize()
    delta = torch.cuda.max_memory_allocated() - base
    one = 4 * B * T * K * D
    print(f"[triangulation cnn] peak allocation over forward + backward {delta / 2**20:.1f} MiB; one [B,T,K*D] tensor {one / 2**20:.1f} MiB")
    assert delta < one // 4
    for t in (x, anchors, *cnn):
        assert bool(torch.isfinite(t.grad).all())


def test_refusals_come_before_any_launch(lib):
    from learnablepoolingmethods_amd import _capi, ops
    dev = cuda()
    most = lib._lpm_triangulation_attention_max_frames()
    a128 = torch.randn(128, 4, device=dev)
    c128 = torch.randn(4, 2, 128, device=dev)

    def both(x, anchors, T):
        with pytest.raises(_capi.LpmError):
            ops.triangulation_mean_pool(x, anchors, T)
        with pytest.raises(_capi.LpmError):
            ops.triangulation_cnn_pool(x, anchors, torch.randn(anchors.shape[1], 2, anchors.shape[0], device=dev),
                                       torch.randn(anchors.shape[1], 2, anchors.shape[0], device=dev), T)
    both(torch.randn(5, 128, device=dev), a128, 1)                                        # T = 1
    both(torch.randn(8, 96, device=dev), torch.randn(96, 4, device=dev), 4)               # D = 96
    both(torch.randn(8, 256, device=dev)[:, :128], a128, 4)                               # non-contiguous x
    both(torch.randn(0, 128, device=dev), a128, 4)                                        # B = 0
    both(torch.randn(most + 1, 128, device=dev), a128, most + 1)                          # T above the supported maximum
    x = torch.randn(8, 128, device=dev)
    for bad in (torch.randn(3, 2, 128, device=dev), torch.randn(4, 2, 64, device=dev), torch.randn(4, 128, device=dev),
                torch.randn(4, 128, 2, device=dev)):                                      # wrong cnn_* shape: K, D, rank, [K, D, F]
        with pytest.raises(_capi.LpmError):
            ops.triangulation_cnn_pool(x, a128, bad, c128, 4)
        with pytest.raises(_capi.LpmError):
            ops.triangulation_cnn_pool(x, a128, c128, bad, 4)
    # the C entry points themselves refuse as well, with their error codes
    outs = [torch.empty(8, 4 * 128, device=dev) for _ in range(2)]
    small = [torch.empty(64, device=dev) for _ in range(2)]
    ws = torch.empty(1 << 16, device=dev)
    p, st = _capi.ptr, _capi.stream_ptr

    def gram(B, T, D, K):
        return lib._lpm_triangulation_mean_gram(p(x), p(a128), B, T, D, K, 1.0, p(small[0]), p(ws), ws.numel() * 4, st())

    def fwd(B, T, D, K):
        return lib._lpm_triangulation_mean_pool_fwd(p(x), p(a128), p(small[0]), B, T, D, K, 1.0, p(outs[0]), p(outs[1]), st())

    def dw(B, T, D, K):
        return lib._lpm_triangulation_mean_dw(p(x), p(a128), p(outs[0]), B, T, D, K, 1.0, p(small[0]), p(ws), ws.numel() * 4, st())

    def bwd(B, T, D, K):
        return lib._lpm_triangulation_mean_bwd(p(x), p(a128), p(small[0]), p(small[1]), p(outs[0]), p(outs[1]), B, T, D, K, 1.0,
                                               p(torch.empty_like(x)), p(torch.empty_like(a128)), p(ws), ws.numel() * 4, st())
    for call in (gram, fwd, dw, bwd):
        assert call(8, 1, 128, 4) == -2 and "frames" in lib.last_error()         # LPM_ERR_UNSUPPORTED_SHAPE
        assert call(2, 4, 96, 4) == -2
        assert call(0, 4, 128, 4) == -1                                          # LPM_ERR_BADARG
        assert call(1, most + 1, 128, 4) == -2 and "frames" in lib.last_error()
    torch.cuda.synchronize()


def test_module_path_on_the_gpu_meets_the_same_bound():
    """The materialising modules (the path FLAGS.triangulation_cnn_fused = False takes) on the GPU, held to the op's bound against the
    same fp64 yardstick; danchors is taken with respect to the variable here (through l2_normalize(anchor_weights, 0)) on every side."""
    from learnablepoolingmethods_amd import aggregation_modules, layers, ops, variables as vs, video_pooling_modules as M
    dev = cuda()
    B, T, D, K, F = 3, 7, 128, 5, 3
    x, raw, _ = R.make_inputs(B, T, D, K, 0)                    # raw: the variable as initialised; the module normalises it itself
    ref = _reference(x, R.l2n(raw, 0), T, F, 0)
    _condition("module path (3,7,128,5)", ref)
    for dt, key in ((torch.float64, "64"), (torch.float32, "32")):
        leaves = [t.to(dt).requires_grad_(True) for t in (x, raw, ref["cnn_d"], ref["cnn_t"])]
        outs = C.cnn_pool(leaves[0], R.l2n(leaves[1], 0), leaves[2], leaves[3], T)
        grads = torch.autograd.grad(sum((o * g.to(dt)).sum() for o, g in zip(outs, ref["up"])), leaves)
        ref[key].update(zip(TENSORS[2:6], grads))
    leaves = [t.to(dev).requires_grad_(True) for t in (x, raw, ref["cnn_d"], ref["cnn_t"])]
    store = vs.VariableStore(device=dev)
    for n, v in zip(("anchor_weights", "d/cnn_weights", "t/cnn_weights"), leaves[1:]):     # the variables exist already, with the case's values
        store.vars[n], store.trainable[n] = v, True
    with vs.use_store(store):
        emb = M.TriangulationEmbedding(D, T, K, None, True).forward(leaves[0])
        with vs.variable_scope("d"):
            emb_cnn = M.TriangulationCnnModule(D, T, F, K, None, True, "d").forward(emb)
        tmp = M.TriangulationTemporalEmbedding(D, T, K, None, True).forward(emb)
        with vs.variable_scope("t"):
            tmp_cnn = M.TriangulationCnnModule(D, T - 1, F, K, None, True, "t").forward(tmp.reshape(-1, K * D))
    assert len(store.vars) == 3
    agg_d = aggregation_modules.IndirectClusterMeanPoolModule(l2_normalize=False).forward(emb.reshape(-1, T, K * D), emb_cnn)
    agg_t = aggregation_modules.MeanStdPoolModule(l2_normalize=False).forward(tmp_cnn)
    grads = torch.autograd.grad(sum((o * g.to(dev)).sum() for o, g in zip((agg_d, agg_t), ref["up"])), leaves)
    got = dict(zip(TENSORS[:6], [agg_d, agg_t, *grads]))
    got["m_d"], got["m_t"] = aggregation_modules.IndirectClusterMeanPoolModule(False).forward(emb.reshape(-1, T, K * D), emb.reshape(-1, T, K * D)), tmp.mean(dim=1)
    _check("module path (3,7,128,5)", got, ref)
    # ... and the op with the same variable
    leaves = [t.to(dev).requires_grad_(True) for t in (x, raw, ref["cnn_d"], ref["cnn_t"])]
    outs = ops.triangulation_cnn_pool(leaves[0], layers.l2_normalize(leaves[1], 0), leaves[2], leaves[3], T)
    grads = torch.autograd.grad(sum((o * g.to(dev)).sum() for o, g in zip(outs, ref["up"])), leaves)
    with torch.no_grad():
        means = ops.triangulation_mean_pool(leaves[0].detach(), layers.l2_normalize(leaves[1].detach(), 0), T)
    _check("fused path, gradient of the variable (3,7,128,5)", dict(zip(TENSORS, [*outs, *grads, *means])), ref)


MODEL_BATCH_SEED = 31


def test_triangulation_cnn_cluster_model_step_matches_fp64():
    """TriangulationCnnClusterModel at tiny sizes (vocab 40, anchors 4 / 2, filters 3 / 2, hidden 16 / 8, 12 sampled frames, B = 6), frame
    draws handed in WITHOUT repeats: predictions, loss, raw and clipped gradients and the variables after one Trainer step against the
    fp64 restatement (tests/_triangulation_cnn_ref.model_loss), exactly as test_soft_attention_triangulation_model_step_matches_fp64
    checks its model: the project's model-level 1e-3 (1e-4 for the loss) with the floors of that test.  The variables come from a CPU
    build (seed 3).  Batch seed 31 (draws seed 32) was picked on the CPU among 21, 23, ..., 31: the fp64 restatement's smallest |G_d|
    over both streams is 1.53e-4 there (1.35e-4 and 1.31e-4 at 21 and 29, 5.0e-5 to 9.1e-5 for the other three), and the test asserts
    that it is at least 1e-4."""
    from oracle import lpm_oracle as O
    from learnablepoolingmethods_amd import FLAGS, registry
    from learnablepoolingmethods_amd.train import Trainer
    from tests._util import assert_close, rel_l2
    dev = cuda()
    V, KV, KA, FV, FA, HV, HA, Sf, B, MF, lr = 40, 4, 2, 3, 2, 16, 8, 12, 6, 16, 1e-3
    x, nf, lab = O.make_synthetic_batch(B, MF, 1152, V, seed=MODEL_BATCH_SEED, min_frames=Sf)
    g = torch.Generator().manual_seed(MODEL_BATCH_SEED + 1)
    u = torch.stack([(torch.randperm(int(n), generator=g)[:Sf].float() + 0.5) / float(n) for n in nf])
    kwargs = dict(iterations=Sf, video_anchor_size=KV, audio_anchor_size=KA, video_kernel_size=FV, audio_kernel_size=FA, video_hidden=HV,
                  audio_hidden=HA, frame_uniform=u)
    name = "TriangulationCnnClusterModel"
    host = Trainer(registry.get_model(name), vocab_size=V, batch_size=B, base_learning_rate=lr, device="cpu", seed=3, model_kwargs=kwargs)
    host.build(x, nf, lab)
    tr = Trainer(registry.get_model(name), vocab_size=V, batch_size=B, base_learning_rate=lr, device=dev, seed=3, model_kwargs=kwargs)
    tr.build(x, nf, lab)
    tr.load_state_dict(host.state_dict())
    shapes = C.model_variable_shapes(V, KV, KA, FV, FA, HV, HA)
    assert {n: tuple(v.shape) for n, v in tr.store.vars.items()} == {"tower/" + n: s for n, s in shapes.items()}
    p = {n[len("tower/"):]: v.detach().double().cpu() for n, v in tr.store.vars.items()}
    smallest = C.model_smallest_gram(p, x.double(), nf, u)
    print(f"[triangulation cnn] model: smallest |G_d| over both streams {smallest:.3e}")
    assert smallest >= 1e-4
    names = [n for n in p if R.is_trainable(n)]
    for n in names:
        p[n].requires_grad_(True)
    pred, label_loss, final = C.model_loss(p, x.double(), nf, lab, u)
    grads = dict(zip(names, torch.autograd.grad(final, [p[n] for n in names])))
    gscale = max(float(v.abs().max()) for v in grads.values())
    clipped = O.clip_gradient_norms(grads, 1.0)

    # the module path predicts what the fused path predicts (inference mode: same variables, moving statistics)
    fused_pred = tr.predict(x, nf, frame_uniform=u)
    FLAGS.triangulation_cnn_fused = False
    try:
        module_pred = tr.predict(x, nf, frame_uniform=u)
    finally:
        FLAGS.reset()
    print(f"[triangulation cnn] model: fused vs module predictions {float((fused_pred - module_pred).abs().max()):.3e}")
    assert_close(fused_pred, module_pred.double().cpu(), tol=1e-5, what="fused vs module path predictions")

    out = tr.step(x, nf, lab)
    e_loss = assert_close(out["loss"], label_loss.detach(), tol=1e-4, what="loss")
    e_pred = assert_close(out["predictions"], pred.detach(), what="predictions")
    print(f"[triangulation cnn] model: loss error {e_loss:.3e}, predictions error {e_pred:.3e}")
    for n in names:
        raw = tr.gradient("tower/" + n).detach().double().cpu()
        floor = 1e-4 * gscale * grads[n].numel() ** 0.5
        e_raw = rel_l2(raw, grads[n], floor=floor)
        e_clip = rel_l2(O.clip_gradient_norms({n: raw}, 1.0)[n], clipped[n], floor=floor)
        ref_new, _, _ = O.adam_tf_update(p[n].detach(), clipped[n], torch.zeros_like(clipped[n]), torch.zeros_like(clipped[n]), lr, 1)
        got = tr.store.vars["tower/" + n].detach().double().cpu()
        mask = grads[n].abs() > max(1e-3 * float(grads[n].abs().max()), 1e-4 * gscale)
        e_upd = rel_l2((got - p[n].detach())[mask], (ref_new - p[n].detach())[mask]) if bool(mask.any()) else 0.0
        print(f"[triangulation cnn] model {n}: gradient {e_raw:.3e}, clipped {e_clip:.3e}, update {e_upd:.3e} on {int(mask.sum())} of {mask.numel()}")
        assert e_raw <= 1e-3 and e_clip <= 1e-3, f"gradient {n}: relative L2 error {e_raw:.3e} (clipped {e_clip:.3e})"
        assert e_upd <= 1e-3, f"variable {n} after one step: relative L2 error of the update {e_upd:.3e}"
