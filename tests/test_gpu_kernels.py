"""-m gpu: each HIP kernel through the C ABI vs the fp64 oracle on the same seeded inputs.
Tolerance: 1e-3 relative (north_star); the exact-fp32 MFMA kernels land around 1e-6."""
import numpy as np
import pytest
import torch

from oracle import lpm_oracle as O
from oracle import numpy_ref as R
from tests._util import assert_close, cuda, rel_err, rel_l2

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["bf16x3", "f32"])
def vlad_precision(request):
    """Both matrix-core arithmetics of K1 / K2: split-bf16 (default) and exact fp32."""
    from learnablepoolingmethods_amd import ops
    old = ops.VLAD_PRECISION, ops.ASSIGN_PRECISION
    ops.VLAD_PRECISION = ops.ASSIGN_PRECISION = request.param
    yield request.param
    ops.VLAD_PRECISION, ops.ASSIGN_PRECISION = old


@pytest.fixture(params=["bf16x3", "bf16x3/2", "f32"])
def mha_precision(request):
    """The matrix-core arithmetics of the attention core K4: split-bf16 (three-term products throughout, the default), split-bf16 with
    the backward's products behind dS on two fp16 terms ("bf16x3/2": lpm_mha_bwd_set_terms(2), round 6), and exact fp32."""
    from learnablepoolingmethods_amd import _capi, ops
    lib = _capi.load()
    old = ops.MHA_PRECISION, ops.MHA_BN_PRECISION
    prec, _, terms = request.param.partition("/")
    ops.MHA_PRECISION = ops.MHA_BN_PRECISION = prec
    prev = lib._lpm_mha_bwd_set_terms(int(terms or 3))
    yield request.param
    lib._lpm_mha_bwd_set_terms(prev)
    ops.MHA_PRECISION, ops.MHA_BN_PRECISION = old


def _netvlad_inputs(B, T, D, K, ld=None, seed=0, dev=None):
    g = torch.Generator().manual_seed(seed)
    ld = ld or D
    full = torch.randn(B * T, ld, generator=g)
    W = torch.randn(D, K, generator=g) / D ** 0.5
    gamma = 1 + 0.3 * torch.randn(K, generator=g)
    beta = 0.2 * torch.randn(K, generator=g)
    W2 = torch.randn(1, D, K, generator=g) / D ** 0.5
    dout = torch.randn(B, D * K, generator=g)
    return full, W, gamma, beta, W2, dout


def _oracle_netvlad(x, W, gamma, beta, W2, T, dout, residual=True):
    p = {"s/cluster_weights": W.double().requires_grad_(True), "s/cluster_bn/gamma": gamma.double().requires_grad_(True),
         "s/cluster_bn/beta": beta.double().requires_grad_(True), "s/cluster_weights2": W2.double().requires_grad_(True)}
    xd = x.double().requires_grad_(True)
    upd = {}
    fn = O.netvlad_forward if residual else O.lightvlad_forward
    out = fn(xd, p, "s", T, True, True, upd)
    out.backward(dout.double())
    return out.detach(), xd.grad, p, upd


@pytest.mark.parametrize("B,T,D,K,off", [(3, 30, 1024, 16, 0), (2, 37, 128, 64, 1024), (4, 300, 1024, 256, 0),
                                          (2, 300, 128, 64, 1024), (2, 16, 256, 96, 0), (1, 9, 512, 40, 0)])
def test_netvlad_fwd_bwd(B, T, D, K, off, vlad_precision):
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    ld = 1152 if off or D == 1024 else D
    full, W, gamma, beta, W2, dout = _netvlad_inputs(B, T, D, K, ld, seed=B * 1000 + T)
    xs = full[:, off:off + D]
    ref, dx_ref, p, upd = _oracle_netvlad(xs, W, gamma, beta, W2, T, dout)
    fg = full.to(dev).requires_grad_(True)
    xg = fg[:, off:off + D]
    Wg, gg, bg, W2g = (t.to(dev).requires_grad_(True) for t in (W, gamma, beta, W2))
    mm, mv = torch.zeros(K, device=dev), torch.ones(K, device=dev)
    out = ops.netvlad(xg, Wg, W2g, T, bn=(gg, bg, mm, mv), is_training=True)
    assert out.shape == (B, D * K)
    assert_close(out, ref, what="netvlad fwd")
    out.backward(dout.to(dev))
    assert_close(fg.grad[:, off:off + D], dx_ref, what="dx")
    assert_close(Wg.grad, p["s/cluster_weights"].grad, what="dW")
    assert_close(gg.grad, p["s/cluster_bn/gamma"].grad, what="dgamma")
    assert_close(bg.grad, p["s/cluster_bn/beta"].grad, what="dbeta")
    assert_close(W2g.grad, p["s/cluster_weights2"].grad, what="dW2")
    # moving statistics (decay 0.999, unbiased variance on the fused path)
    assert_close(mm, upd["s/cluster_bn/moving_mean"] * 0.001, tol=1e-4, what="moving_mean")
    assert_close(mv, 0.999 + upd["s/cluster_bn/moving_variance"] * 0.001, tol=1e-5, what="moving_var")
    # norm invariant: unit global norm, every cluster column 1/sqrt(K)
    o = out.detach().reshape(B, D, K)
    assert torch.allclose(o.norm(dim=(1, 2)), torch.ones(B, device=dev), atol=1e-5)
    assert torch.allclose(o.norm(dim=1), torch.full((B, K), K ** -0.5, device=dev), atol=1e-5)


@pytest.mark.parametrize("B,T,D,K,kmajor", [(4, 300, 1024, 256, True), (4, 300, 1024, 256, False), (3, 50, 256, 512, True),
                                            (5, 37, 128, 128, False), (2, 300, 1024, 512, False)])
def test_fused_aggregation_matches_the_two_pass_form(B, T, D, K, kmajor):
    """K2 with the finalize pass fused in (lpm_vlad_aggregate_fused_fwd, the default where the shape allows) against the two-launch
    form and against the oracle: forward in both layouts, backward (K3 reads the un-normalised sums the fused kernel stores only when
    a gradient is wanted), inference (nothing but the descriptor is written), a degenerate (all-zero) cluster column, and the
    kernel's time-out path driven on purpose -- every clip finished by the follow-up pass instead."""
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    full, W, gamma, beta, W2, dout = _netvlad_inputs(B, T, D, K, seed=B * 77 + K)
    ref, dx_ref, p, _ = _oracle_netvlad(full, W, gamma, beta, W2, T, dout)
    refo = ref.reshape(B, D, K).transpose(1, 2) if kmajor else ref
    dog = (dout.reshape(B, D, K).transpose(1, 2).contiguous() if kmajor else dout).to(dev)

    def run(fused, fallback=False, grad=True):
        old = ops.VLAD_FUSED, ops.VLAD_FUSED_DEBUG_FALLBACK
        ops.VLAD_FUSED, ops.VLAD_FUSED_DEBUG_FALLBACK = fused, fallback
        try:
            xg = full.to(dev).requires_grad_(grad)
            Wg, gg, bg, W2g = (t.to(dev).requires_grad_(grad) for t in (W, gamma, beta, W2))
            out = ops.netvlad(xg, Wg, W2g, T, bn=(gg, bg, torch.zeros(K, device=dev), torch.ones(K, device=dev)), is_training=True,
                              kmajor=kmajor)
            if grad:
                out.backward(dog)
                return out.detach(), xg.grad, Wg.grad, W2g.grad
            return out.detach(), None, None, None
        finally:
            ops.VLAD_FUSED, ops.VLAD_FUSED_DEBUG_FALLBACK = old
    two = run(False)
    fus = run(True)
    assert fus[0].shape == refo.shape
    assert_close(fus[0], refo, what="fused fwd vs oracle")
    assert_close(fus[0], two[0], tol=1e-6, what="fused fwd vs two-pass")
    assert_close(fus[1], dx_ref, what="fused dx")
    assert_close(fus[2], p["s/cluster_weights"].grad, what="fused dW")
    assert_close(fus[3], p["s/cluster_weights2"].grad, what="fused dW2")
    for a, b, nm in zip(fus[1:], two[1:], ("dx", "dW", "dW2")):
        assert_close(a, b, tol=1e-5, what=f"fused vs two-pass {nm}")
    inf = run(True, grad=False)
    assert torch.equal(inf[0], fus[0]), "inference (no U stored) and training forward agree bit for bit"
    fb = run(True, fallback=True)
    assert_close(fb[0], fus[0], tol=1e-6, what="time-out path fwd")
    for a, b, nm in zip(fb[1:], fus[1:], ("dx", "dW", "dW2")):
        assert_close(a, b, tol=1e-5, what=f"time-out path {nm}")
    fbi = run(True, fallback=True, grad=False)
    assert_close(fbi[0], fus[0], tol=1e-6, what="time-out path fwd (inference: U written by the fallback itself)")
    # a degenerate cluster: similarities that are zero for one cluster give an all-zero column (l2_normalize's epsilon clamp)
    g = torch.Generator().manual_seed(3)
    sims = torch.rand(B, T, K, generator=g)
    sims[:, :, 5] = 0.0
    cen = torch.randn(D, K, generator=g) / D ** 0.5
    refd = O.vlad_aggregate(sims.double(), full.double().reshape(B, T, D), cen.double())
    refd = refd.reshape(B, D, K).transpose(1, 2) if kmajor else refd
    for fused in (True, False):
        old = ops.VLAD_FUSED
        ops.VLAD_FUSED = fused
        try:
            got = ops.vlad_aggregate(sims.to(dev), full.to(dev), cen.to(dev), T, kmajor=kmajor)
        finally:
            ops.VLAD_FUSED = old
        assert_close(got, refd, what=f"degenerate column (fused={fused})")
        assert float(got.reshape(B, K, D)[:, 5].abs().max() if kmajor else got.reshape(B, D, K)[:, :, 5].abs().max()) == 0.0


def test_netvlad_kmajor_layout_and_eval_mode(vlad_precision):
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    B, T, D, K = 3, 20, 128, 32
    full, W, gamma, beta, W2, dout = _netvlad_inputs(B, T, D, K, seed=5)
    gmv = torch.Generator().manual_seed(6)
    mm, mv = 0.1 * torch.randn(K, generator=gmv), 1 + 0.2 * torch.rand(K, generator=gmv)
    p = {"s/cluster_weights": W.double(), "s/cluster_bn/gamma": gamma.double(), "s/cluster_bn/beta": beta.double(),
         "s/cluster_weights2": W2.double(), "s/cluster_bn/moving_mean": mm.double(), "s/cluster_bn/moving_variance": mv.double()}
    for k in ("s/cluster_weights", "s/cluster_weights2", "s/cluster_bn/gamma", "s/cluster_bn/beta"):
        p[k].requires_grad_(True)
    xd = full.double().requires_grad_(True)
    ref = O.netvlad_forward(xd, p, "s", T, True, False)
    refk = ref.reshape(B, D, K).transpose(1, 2)
    dk = torch.randn(B, K, D, generator=torch.Generator().manual_seed(9))
    (refk * dk.double()).sum().backward()
    xg = full.to(dev).requires_grad_(True)
    Wg, gg, bg, W2g = (t.to(dev).requires_grad_(True) for t in (W, gamma, beta, W2))
    out = ops.netvlad(xg, Wg, W2g, T, bn=(gg, bg, mm.to(dev), mv.to(dev)), is_training=False, kmajor=True)
    assert out.shape == (B, K, D)
    assert_close(out, refk, what="kmajor eval fwd")
    out.backward(dk.to(dev))
    assert_close(xg.grad, xd.grad, what="dx")
    assert_close(Wg.grad, p["s/cluster_weights"].grad, what="dW")
    assert_close(gg.grad, p["s/cluster_bn/gamma"].grad, what="dgamma (eval)")
    assert_close(W2g.grad, p["s/cluster_weights2"].grad, what="dW2")


def test_lightvlad_and_bias_mode(vlad_precision):
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    B, T, D, K = 2, 12, 128, 8
    full, W, gamma, beta, W2, dout = _netvlad_inputs(B, T, D, K, seed=11)
    ref, dx_ref, p, _ = _oracle_netvlad(full, W, gamma, beta, W2, T, dout, residual=False)
    xg = full.to(dev).requires_grad_(True)
    Wg, gg, bg = (t.to(dev).requires_grad_(True) for t in (W, gamma, beta))
    out = ops.netvlad(xg, Wg, None, T, bn=(gg, bg, torch.zeros(K, device=dev), torch.ones(K, device=dev)))
    assert_close(out, ref, what="lightvlad fwd")
    out.backward(dout.to(dev))
    assert_close(xg.grad, dx_ref, what="lightvlad dx")
    # no-BN branch: logits + cluster_biases (frame_level_models.py:2790-2796)
    bias = torch.randn(K, generator=torch.Generator().manual_seed(3))
    pb = {"s/cluster_weights": W.double(), "s/cluster_biases": bias.double().requires_grad_(True), "s/cluster_weights2": W2.double()}
    xd = full.double().requires_grad_(True)
    refb = O.netvlad_forward(xd, pb, "s", T, False, True)
    refb.backward(dout.double())
    xg2 = full.to(dev).requires_grad_(True)
    bgp = bias.to(dev).requires_grad_(True)
    outb = ops.netvlad(xg2, W.to(dev), W2.to(dev), T, bn=None, bias=bgp)
    assert_close(outb, refb, what="bias-mode fwd")
    outb.backward(dout.to(dev))
    assert_close(xg2.grad, xd.grad, what="bias-mode dx")
    assert_close(bgp.grad, pb["s/cluster_biases"].grad, what="dbias")


@pytest.mark.parametrize("B,T,D,K,ld,off", [(3, 30, 1024, 32, 1024, 0), (2, 300, 128, 64, 1152, 1024), (20, 300, 1024, 256, 1152, 0),
                                              (1, 77, 256, 512, 256, 0), (1, 1, 32, 32, 32, 0), (5, 129, 1024, 288, 1024, 0),
                                              (6, 129, 512, 256, 512, 0), (3, 300, 256, 256, 256, 0), (2, 33, 1024, 256, 1024, 0)])
def test_assign_gemm_tiles(B, T, D, K, ld, off):
    """K1 and its backward on the bf16 pipe through the C ABI (frame_level_models.py:2781-2789 and TF autodiff of it):
    logits + per-workgroup column statistics, dx += dl . W^T, dW = x^T . dl.  Ragged frame counts (zero-padded tail
    tiles), strided inputs, K below / across / at the column-block limits.  K = 256 with a tile count divisible by four
    takes the 128-row workgroup form, whose four-tile groups straddle clips (20 x 300, 6 x 129, 2 x 33 frames); 3 x 300 does
    not divide and stays on the 64-row form."""
    from learnablepoolingmethods_amd import _capi
    from learnablepoolingmethods_amd._capi import ptr, stream_ptr
    lib = _capi.load()
    dev = cuda()
    M = B * T
    g = torch.Generator().manual_seed(M + K)
    full = torch.randn(M, ld, generator=g).to(dev)
    W = (torch.randn(D, K, generator=g) / D ** 0.5).to(dev)
    dl = torch.randn(M, K, generator=g).to(dev)
    dx0 = torch.randn(M, D, generator=g).to(dev)
    x = full[:, off:off + D]
    assert lib._lpm_assign_gemm_tiles_supported(T, D, K)

    def buf(n):
        return torch.empty(n // 4, dtype=torch.int32, device=dev)
    st = stream_ptr()
    xr, wt = buf(lib._lpm_row_tiles_bytes(B, T, D)), buf(lib._lpm_weight_tiles_bytes(D, K))
    nblk = lib._lpm_assign_gemm_tiles_nblk(B, T)
    logits = torch.full((M, K), float("nan"), device=dev)
    partial = torch.full((nblk, 2, K), float("nan"), device=dev)
    lib.check(lib._lpm_split_rows_tiles(ptr(x), x.stride(0), B, T, D, ptr(xr), st), "split_rows_tiles")
    lib.check(lib._lpm_split_weight_tiles(ptr(W), D, K, 0, ptr(wt), st), "split_weight_tiles")
    lib.check(lib._lpm_assign_gemm_tiles_fwd(ptr(xr), ptr(wt), B, T, D, K, ptr(logits), ptr(partial), st), "assign_gemm_tiles_fwd")
    x64, W64, dl64 = x.double().cpu(), W.double().cpu(), dl.double().cpu()
    ref = x64 @ W64
    assert_close(logits, ref, 2e-5, "logits")
    assert_close(partial[:, 0].sum(0), ref.sum(0), 1e-4, "column sums", floor=1e-3 * float(ref.abs().sum(0).max()))
    assert_close(partial[:, 1].sum(0), (ref * ref).sum(0), 1e-4, "column square sums")
    # backward
    dlr, wtt = buf(lib._lpm_row_tiles_bytes(B, T, K)), buf(lib._lpm_weight_tiles_bytes(K, D))
    lib.check(lib._lpm_split_rows_tiles(ptr(dl), K, B, T, K, ptr(dlr), st), "split_rows_tiles")
    lib.check(lib._lpm_split_weight_tiles(ptr(W), K, D, 1, ptr(wtt), st), "split_weight_tiles")
    dx = dx0.clone()
    lib.check(lib._lpm_assign_gemm_tiles_bwd_dx(ptr(dlr), ptr(wtt), B, T, D, K, ptr(dx), D, st), "assign_gemm_tiles_bwd_dx")
    assert_close(dx, dx0.double().cpu() + dl64 @ W64.t(), 2e-5, "dx")
    xt, dlt = buf(lib._lpm_xt_bytes(B, T, D)), buf(lib._lpm_xt_bytes(B, T, K))
    lib.check(lib._lpm_split_frames(ptr(x), x.stride(0), B, T, D, ptr(xt), st), "split_frames")
    lib.check(lib._lpm_split_frames(ptr(dl), K, B, T, K, ptr(dlt), st), "split_frames")
    wsb = lib._lpm_assign_gemm_tiles_bwd_dw_workspace_bytes(B, T, D, K)
    ws = buf(max(wsb, 4))
    dW = torch.full((D, K), float("nan"), device=dev)
    lib.check(lib._lpm_assign_gemm_tiles_bwd_dw(ptr(xt), ptr(dlt), B, T, D, K, ptr(dW), ptr(ws), wsb, st), "assign_gemm_tiles_bwd_dw")
    assert_close(dW, x64.t() @ dl64, 2e-5, "dW")


@pytest.mark.parametrize("B,T,D,K", [(2, 30, 128, 16), (2, 300, 1024, 256), (3, 17, 256, 64)])
def test_vlad_aggregate_v2_form(B, T, D, K, vlad_precision):
    """NetVladAttenCluster tail: similarities may be negative, no softmax (video_pooling_modules.py:1646-1658)."""
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    g = torch.Generator().manual_seed(B + T)
    sims, x, C = torch.randn(B, T, K, generator=g), torch.randn(B * T, D, generator=g), torch.randn(D, K, generator=g) / D ** .5
    dout = torch.randn(B, D * K, generator=g)
    sd, xd, Cd = (t.double().requires_grad_(True) for t in (sims, x, C))
    ref = O.vlad_aggregate(sd, xd.reshape(B, T, D), Cd)
    ref.backward(dout.double())
    sg, xg, Cg = (t.to(dev).requires_grad_(True) for t in (sims, x, C))
    out = ops.vlad_aggregate(sg, xg, Cg, T)
    assert_close(out, ref, what="v2 aggregate fwd")
    out.backward(dout.to(dev))
    assert_close(sg.grad, sd.grad, what="dsims")
    assert_close(xg.grad, xd.grad, what="dx")
    assert_close(Cg.grad, Cd.grad, what="dcentres")


def test_vlad_degenerate_zero_column(vlad_precision):
    """A cluster with zero mass hits tf.nn.l2_normalize's 1e-12 clamp (forward 0, backward unprojected)."""
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    B, T, D, K = 2, 8, 128, 8
    g = torch.Generator().manual_seed(1)
    sims, x, C = torch.randn(B, T, K, generator=g), torch.randn(B * T, D, generator=g), torch.randn(D, K, generator=g)
    sims[:, :, 3] = 0.0
    dout = torch.randn(B, D * K, generator=g)
    sd, xd, Cd = (t.double().requires_grad_(True) for t in (sims, x, C))
    ref = O.vlad_aggregate(sd, xd.reshape(B, T, D), Cd)
    ref.backward(dout.double())
    sg, xg, Cg = (t.to(dev).requires_grad_(True) for t in (sims, x, C))
    out = ops.vlad_aggregate(sg, xg, Cg, T)
    assert torch.isfinite(out).all()
    assert_close(out, ref, what="degenerate fwd")
    out.backward(dout.to(dev))
    assert_close(sg.grad, sd.grad, what="degenerate dsims")
    assert_close(Cg.grad, Cd.grad, what="degenerate dcentres")


def test_frame_permutation_invariance_full_size():
    """Size-independent property at BASELINE cfg-2 shapes: the descriptor sums over frames, so permuting
    the frames of every clip identically (BN statistics unchanged) leaves it unchanged."""
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    B, T, D, K = 80, 300, 1024, 256
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B, T, 1152, device=dev, generator=g)
    W = torch.randn(D, K, device=dev, generator=g) / 32
    W2 = torch.randn(1, D, K, device=dev, generator=g) / 32
    bn = lambda: (torch.ones(K, device=dev), torch.zeros(K, device=dev), torch.zeros(K, device=dev), torch.ones(K, device=dev))
    a = ops.netvlad(x.reshape(B * T, 1152)[:, :D], W, W2, T, bn=bn())
    perm = torch.randperm(T, device=dev, generator=g)
    b = ops.netvlad(x[:, perm].reshape(B * T, 1152)[:, :D], W, W2, T, bn=bn())
    assert rel_err(a, b) < 1e-4
    o = a.reshape(B, D, K)
    assert torch.allclose(o.norm(dim=(1, 2)), torch.ones(B, device=dev), atol=1e-5)


@pytest.mark.parametrize("B,L,h,d", [(2, 256, 4, 16), (3, 64, 16, 8), (2, 300, 8, 16), (1, 33, 2, 16), (2, 16, 1, 8), (4, 12, 16, 8),
                                     (2, 500, 2, 16)])
def test_mha_core(B, L, h, d, mha_precision):
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    g = torch.Generator().manual_seed(L)
    F = h * d
    q, k, v, do = (torch.randn(B, L, F, generator=g) for _ in range(4))
    sc = d ** -0.5
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    ref = O._combine_heads(O.attention_core(O._split_heads(qd, h), O._split_heads(kd, h), O._split_heads(vd, h), sc))
    ref.backward(do.double())
    qg, kg, vg = (t.to(dev).requires_grad_(True) for t in (q, k, v))
    out = ops.mha_core(qg, kg, vg, h, sc)
    assert_close(out, ref, what="mha fwd")
    out.backward(do.to(dev))
    assert_close(qg.grad, qd.grad, what="dq")
    assert_close(kg.grad, kd.grad, what="dk")
    assert_close(vg.grad, vd.grad, what="dv")


@pytest.mark.parametrize("L,h,d,bn", [(256, 4, 16, False), (64, 4, 8, False), (300, 4, 16, True), (500, 2, 16, False)])
@pytest.mark.parametrize("gscale", [1e-9, 1.0, 3e4])
def test_mha_backward_two_terms_over_the_gradient_range(L, h, d, bn, gscale):
    """Round 6: the backward's products behind dS on two fp16 terms (lpm_mha_bwd_set_terms(2); opt-in).  fp16 has five exponent bits and the
    gradient reaching the attention core spans 1e-9 ... 20 over a run: the kernels scale dO by a power of two taken from max |dO| -- per
    query in the dq kernel, per (batch, head) in the dkv kernel -- so the result must be as good at 1e-9 and at 3e4 as at 1, with one
    query row 1e6 x smaller than the rest (its dq still to 1e-3 of ITS scale: the per-query scale).  Also prints the two-term
    form's distance from the fp64 oracle beside the three-term form's (transformer_utils.py:570-578, 640-661)."""
    from learnablepoolingmethods_amd import _capi, ops
    lib = _capi.load()
    dev = cuda()
    B = 2
    g = torch.Generator().manual_seed(7 * L + d)
    F = h * d
    q, k, v, do = (torch.randn(B, L, F, generator=g) for _ in range(4))
    do = do * gscale
    do[:, 3] *= 1e-6
    sc = 1.0 if bn else d ** -0.5
    gamma, beta = 1 + 0.2 * torch.randn(L, generator=g), 0.1 * torch.randn(L, generator=g)
    p = {"bn/gamma": gamma.double().requires_grad_(True), "bn/beta": beta.double().requires_grad_(True),
         "bn/moving_mean": torch.zeros(L).double(), "bn/moving_variance": torch.ones(L).double()}
    if bn:
        q, k = 0.5 * q, 0.5 * k
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    fn = (lambda lg: O.batch_norm(lg, p, "bn", True, {})) if bn else None
    ref = O._combine_heads(O.attention_core(O._split_heads(qd, h), O._split_heads(kd, h), O._split_heads(vd, h), sc, fn))
    ref.backward(do.double())
    dgamma_ref, dbeta_ref = p["bn/gamma"].grad, p["bn/beta"].grad
    errs = {}
    for terms in (2, 3):
        prev = lib._lpm_mha_bwd_set_terms(terms)
        try:
            qg, kg, vg = (t.to(dev).requires_grad_(True) for t in (q, k, v))
            if bn:
                gg, bg = gamma.to(dev).requires_grad_(True), beta.to(dev).requires_grad_(True)
                out = ops.mha_core_bn(qg, kg, vg, h, gg, bg, torch.zeros(L, device=dev), torch.ones(L, device=dev), is_training=True)
            else:
                out = ops.mha_core(qg, kg, vg, h, sc)
            out.backward(do.to(dev))
            errs[terms] = (rel_err(qg.grad, qd.grad), rel_err(kg.grad, kd.grad), rel_err(vg.grad, vd.grad),
                           rel_err(qg.grad[:, 3], qd.grad[:, 3]))
            if bn:
                errs[terms] += (rel_err(gg.grad, dgamma_ref), rel_err(bg.grad, dbeta_ref))
        finally:
            lib._lpm_mha_bwd_set_terms(prev)
    print(f"[K4 backward L={L} d={d} bn={bn} |dO|~{gscale:g}] two terms (dq, dk, dv, dq of the small row, ...): "
          + ", ".join(f"{e:.1e}" for e in errs[2]) + "; three terms: " + ", ".join(f"{e:.1e}" for e in errs[3]))
    assert max(errs[2]) <= 1e-3, f"two-term backward: {errs[2]}"
    assert max(errs[3]) <= 1e-3, f"three-term backward: {errs[3]}"


@pytest.mark.parametrize("B,L,h,d,training", [(2, 48, 2, 16, True), (2, 300, 8, 16, True), (2, 30, 8, 16, False), (4, 12, 64, 16, True),
                                              (4, 12, 16, 8, True),
                                              (36, 22, 64, 16, True)])      # 2304 (batch, head) rows of statistics: the 4-column reductions
def test_mha_core_logits_bn(B, L, h, d, training, mha_precision):
    """MultiHeadAttentionBN core: batch_norm over the key-position channel of [B,h,Lq,Lk] (transformer_utils.py:652-659)."""
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    g = torch.Generator().manual_seed(L + 1)
    F = h * d
    q, k, v, do = (0.5 * torch.randn(B, L, F, generator=g) for _ in range(4))
    gamma, beta = 1 + 0.2 * torch.randn(L, generator=g), 0.1 * torch.randn(L, generator=g)
    mm, mv = 0.1 * torch.randn(L, generator=g), 1 + 0.3 * torch.rand(L, generator=g)
    p = {"bn/gamma": gamma.double().requires_grad_(True), "bn/beta": beta.double().requires_grad_(True),
         "bn/moving_mean": mm.double(), "bn/moving_variance": mv.double()}
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    upd = {}
    ref = O._combine_heads(O.attention_core(O._split_heads(qd, h), O._split_heads(kd, h), O._split_heads(vd, h), 1.0,
                                            lambda lg: O.batch_norm(lg, p, "bn", training, upd)))
    ref.backward(do.double())
    qg, kg, vg, gg, bg = (t.to(dev).requires_grad_(True) for t in (q, k, v, gamma, beta))
    mmg, mvg = mm.to(dev), mv.to(dev)
    out = ops.mha_core_bn(qg, kg, vg, h, gg, bg, mmg, mvg, is_training=training)
    assert_close(out, ref, what="mha-bn fwd")
    out.backward(do.to(dev))
    assert_close(qg.grad, qd.grad, what="dq")
    assert_close(kg.grad, kd.grad, what="dk")
    assert_close(vg.grad, vd.grad, what="dv")
    assert_close(gg.grad, p["bn/gamma"].grad, what="dgamma")
    assert_close(bg.grad, p["bn/beta"].grad, what="dbeta")
    if training:
        assert_close(mmg, mm.double() * 0.999 + upd["bn/moving_mean"] * 0.001, tol=1e-5, what="moving_mean")
        assert_close(mvg, mv.double() * 0.999 + upd["bn/moving_variance"] * 0.001, tol=1e-5, what="moving_var")


@pytest.mark.parametrize("B,L,h,d,fmt", [(2, 300, 8, 16, "bf16x3"), (2, 300, 8, 16, "fp16"), (3, 40, 4, 8, "fp16"), (4, 12, 64, 16, "bf16x3"),
                                         (2, 300, 8, 16, None)])
def test_mha_logits_bn_backward_writes_the_qkv_gradient_image(B, L, h, d, fmt):
    """logits_bn's one-pass backward with [dq | dk | dv] leaving as the q/k/v layer's gradient image (lpm_mha_bwd_x3_bn_image_fmt twice +
    lpm_mha_bn_dk_correct_image; transformer_utils.py:652-661 in front of :559-561, backward): the image is, bit for bit, lpm_split_rows of the
    plain entry points' fp32 gradients in the same operand format, and the recorded max |x| is the same number."""
    from learnablepoolingmethods_amd import _capi, ops
    dev = cuda()
    g = torch.Generator().manual_seed(7 * L + h)
    F = h * d
    qkv = (0.5 * torch.randn(B, L, 3 * F, generator=g)).to(dev)            # column views of one buffer, as the fused projection hands them over
    q, k, v = qkv[..., :F], qkv[..., F:2 * F], qkv[..., 2 * F:]
    do = (0.3 * torch.randn(B, L, F, generator=g)).to(dev)
    gamma, beta = (1 + 0.2 * torch.randn(L, generator=g)).to(dev), (0.1 * torch.randn(L, generator=g)).to(dev)
    mm, mv = torch.zeros(L, device=dev), torch.ones(L, device=dev)
    ctx = ops._SubCtx()
    ops._MHACoreBN.forward(ctx, q, k, v, gamma, beta, mm, mv, h, True)
    plain = ops._MHACoreBN.backward(ctx, do)
    dqkv = torch.cat([t.reshape(B * L, F) for t in plain[:3]], dim=1).contiguous()
    amax_a = torch.zeros(_capi.LPM_OPERAND_AMAX_SUB * _capi.LPM_OPERAND_AMAX_STRIDE, device=dev)
    amax_b = torch.zeros_like(amax_a)
    mk = lambda amax: None if fmt is None else ops.OperandSite(fmt == "fp16", 2.0 ** 9, amax.data_ptr(), role="g")
    want = ops._split_rows(dqkv, grad=True, site=mk(amax_a))
    got = ops._MHACoreBN.backward(ctx, do, image=True, site=mk(amax_b))
    assert got[1] is None and got[2] is None and got[0].dtype == want.dtype and tuple(got[0].shape) == tuple(want.shape)
    assert torch.equal(got[0].view(torch.int16), want.view(torch.int16))
    assert torch.equal(got[3], plain[3]) and torch.equal(got[4], plain[4])                 # dgamma, dbeta: the same statistics
    if fmt is not None:
        assert float(amax_b.max()) == float(amax_a.max()) == float(dqkv.abs().max())


@pytest.mark.parametrize("B,MF,F,S", [(4, 30, 1024, 30), (3, 300, 1152, 300), (2, 300, 1152, 256), (5, 40, 128, 7)])
def test_frame_sample_bn(B, MF, F, S):
    from learnablepoolingmethods_amd import model_utils, ops
    dev = cuda()
    x, nf, _ = O.make_synthetic_batch(B, MF, F, 10, seed=S)
    ref_s = O.sample_uniform_frames(x, nf, S)
    got_s = model_utils.SampleUniformFrames(x.to(dev), nf.to(dev), S)
    assert torch.equal(got_s.cpu(), ref_s), "gather must be bit-exact (index arithmetic is integer work)"
    g = torch.Generator().manual_seed(2)
    gamma, beta = 1 + 0.2 * torch.randn(F, generator=g), 0.1 * torch.randn(F, generator=g)
    p = {"input_bn/gamma": gamma.double().requires_grad_(True), "input_bn/beta": beta.double().requires_grad_(True)}
    upd = {}
    ref = O.batch_norm(ref_s.double().reshape(-1, F), p, "input_bn", True, upd)
    dy = torch.randn(B * S, F, generator=g)
    ref.backward(dy.double())
    gg, bg = gamma.to(dev).requires_grad_(True), beta.to(dev).requires_grad_(True)
    mm, mv = torch.zeros(F, device=dev), torch.ones(F, device=dev)
    y = ops.frame_sample_bn(x.to(dev), nf.to(dev), S, gg, bg, mm, mv, True)
    assert_close(y, ref, what="input_bn fwd")
    y.backward(dy.to(dev))
    assert_close(gg.grad, p["input_bn/gamma"].grad, what="input_bn dgamma")
    assert_close(bg.grad, p["input_bn/beta"].grad, what="input_bn dbeta")
    assert_close(mm, upd["input_bn/moving_mean"] * 0.001, tol=1e-4, what="moving_mean")


@pytest.mark.parametrize("B,MF,S", [(3, 300, 300), (2, 90, 70), (5, 64, 64)])
def test_frame_sample_bn_split_is_the_joint_form_in_two_matrices(B, MF, S):
    """ops.frame_sample_bn_split (round 6; model_utils.py:101-122 + frame_level_models.py:2265-2271 for NetVladV2): the rgb / audio blocks
    of the sampled, batch-normalised frames as two contiguous matrices -- bit for bit the column slices of the joint form, the same
    moving statistics, the frame tiles of each found for it (and equal to lpm_split_frames of it), gamma / beta gradients bit for bit the
    joint form's from the concatenated gradient."""
    from learnablepoolingmethods_amd import _capi, ops
    from learnablepoolingmethods_amd._capi import ptr, stream_ptr
    dev = cuda()
    F, Dv = 1152, 1024
    x, nf, _ = O.make_synthetic_batch(B, MF, F, 10, seed=S)
    g = torch.Generator().manual_seed(3)
    gamma, beta = 1 + 0.2 * torch.randn(F, generator=g), 0.1 * torch.randn(F, generator=g)
    dv, da = torch.randn(B * S, Dv, generator=g).to(dev), torch.randn(B * S, F - Dv, generator=g).to(dev)
    res = []
    for split in (False, True):
        gg, bg = gamma.to(dev).requires_grad_(True), beta.to(dev).requires_grad_(True)
        mm, mv = torch.zeros(F, device=dev), torch.ones(F, device=dev)
        if split:
            assert ops.frame_sample_bn_split_ok(x.to(dev), Dv)
            yv, ya = ops.frame_sample_bn_split(x.to(dev), nf.to(dev), S, gg, bg, mm, mv, True, Dv)
            assert yv.is_contiguous() and ya.is_contiguous()
            lib = _capi.load()
            for t, D in ((yv, Dv), (ya, F - Dv)):
                got = ops._cached_tiles(t, B, S, D)
                assert got is not None, "the tiles written with the matrices must be found for them"
                want = torch.empty(lib._lpm_xt_bytes(B, S, D) // 4, dtype=torch.int32, device=dev)
                lib.check(lib._lpm_split_frames(ptr(t), t.stride(0), B, S, D, ptr(want), stream_ptr()), "lpm_split_frames")
                assert torch.equal(got, want)
            torch.autograd.backward([yv, ya], [dv, da])
        else:
            y = ops.frame_sample_bn(x.to(dev), nf.to(dev), S, gg, bg, mm, mv, True)
            yv, ya = y[:, :Dv], y[:, Dv:]
            y.backward(torch.cat([dv, da], dim=1))
        res.append((yv.detach().clone(), ya.detach().clone(), mm, mv, gg.grad.clone(), bg.grad.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("B,MF,F,S", [(3, 300, 1152, 300), (2, 90, 1024, 70), (2, 64, 1152, 64)])
def test_frame_sample_bn_tile_copies_are_the_split_of_its_output(B, MF, F, S, monkeypatch):
    """lpm_frame_apply_tiles2: the frame tiles (K2's operand) and row tiles (K1's operand) written with the fp32 matrix are, bit
    for bit, what lpm_split_frames / lpm_split_rows_tiles produce from that matrix."""
    from learnablepoolingmethods_amd import _capi, ops
    from learnablepoolingmethods_amd.ops import ptr, stream_ptr
    dev = cuda()
    lib = _capi.load()
    x, nf, _ = O.make_synthetic_batch(B, MF, F, 10, seed=S, min_frames=MF // 3)
    g = torch.Generator().manual_seed(2)
    gamma, beta = (1 + 0.2 * torch.randn(F, generator=g)).to(dev), (0.1 * torch.randn(F, generator=g)).to(dev)
    mm, mv = torch.zeros(F, device=dev), torch.ones(F, device=dev)
    monkeypatch.setattr(ops, "FRAME_ROW_TILES", True)
    y = ops.frame_sample_bn(x.to(dev), nf.to(dev), S, gamma, beta, mm, mv, True)
    for name, c0, D in (("video", 0, 1024), ("audio", 1024, F - 1024)):
        if D == 0:
            continue
        xs = y[:, c0:c0 + D]
        xr = ops._cached_tiles(xs, B, S, D, rows=True)
        xt = ops._cached_tiles(xs, B, S, D)
        assert xr is not None and xt is not None, name
        want_r = torch.empty(lib._lpm_row_tiles_bytes(B, S, D) // 4, dtype=torch.int32, device=dev)
        lib.check(lib._lpm_split_rows_tiles(ptr(xs), xs.stride(0), B, S, D, ptr(want_r), stream_ptr()), "lpm_split_rows_tiles")
        want_t = torch.empty(lib._lpm_xt_bytes(B, S, D) // 4, dtype=torch.int32, device=dev)
        lib.check(lib._lpm_split_frames(ptr(xs), xs.stride(0), B, S, D, ptr(want_t), stream_ptr()), "lpm_split_frames")
        assert xr.numel() == want_r.numel() and torch.equal(xr, want_r), f"{name}: row tiles differ"
        assert xt.numel() == want_t.numel() and torch.equal(xt, want_t), f"{name}: frame tiles differ"


def test_clip_adam_matches_oracle():
    from learnablepoolingmethods_amd import ops
    from learnablepoolingmethods_amd.train import ARENA_ALIGN
    dev = cuda()
    g = torch.Generator().manual_seed(0)
    shapes = [(700, 33), (5,), (4096,), (123, 7), (1,)]
    scales = [3.0, 0.01, 0.05, 1.0, 5.0]          # some variables clip, some do not
    ps = [torch.randn(s, generator=g) for s in shapes]
    gs = [torch.randn(s, generator=g) * c for s, c in zip(shapes, scales)]
    offs, cur = [], 0
    for p in ps:
        offs.append(cur)
        cur += (p.numel() + ARENA_ALIGN - 1) // ARENA_ALIGN * ARENA_ALIGN
    offs.append(cur)
    P, G, M, V = (torch.zeros(cur, device=dev) for _ in range(4))
    for p, gr, o in zip(ps, gs, offs):
        P[o:o + p.numel()] = p.flatten().to(dev)
        G[o:o + p.numel()] = gr.flatten().to(dev)
    offsets = torch.tensor(offs, dtype=torch.int64, device=dev)
    ref_p = [p.double() for p in ps]
    ref_m = [torch.zeros_like(p).double() for p in ps]
    ref_v = [torch.zeros_like(p).double() for p in ps]
    for step in (1, 2, 3):
        ops.clip_adam_step(P, G, M, V, offsets, len(ps), 1.0, 2e-4, step)
        cl = O.clip_gradient_norms({i: g_.double() for i, g_ in enumerate(gs)}, 1.0)
        for i in range(len(ps)):
            ref_p[i], ref_m[i], ref_v[i] = O.adam_tf_update(ref_p[i], cl[i], ref_m[i], ref_v[i], 2e-4, step)
    for p, rp, rm, o in zip(ps, ref_p, ref_m, offs):
        assert_close(P[o:o + p.numel()].reshape(p.shape), rp, tol=1e-6, what="adam param")
        assert_close(M[o:o + p.numel()].reshape(p.shape), rm, tol=1e-5, what="adam m")


def test_clip_adam_adds_the_l2_penalty_gradient_on_the_fly():
    """lpm_multi_tensor_clip_adam_l2 (round 6): the gradient of a variable's L2 penalty, coefficient * w (slim.l2_regularizer on the MoE
    weights, video_level_models.py:84-100; part of the loss whose gradient utils.py:170-189 clips), formed inside the norm pass and the
    update pass -- against the fp64 oracle on grad + coefficient * w, and against the plain entry point behind an explicit add pass."""
    from learnablepoolingmethods_amd import ops
    from learnablepoolingmethods_amd.train import ARENA_ALIGN
    dev = cuda()
    g = torch.Generator().manual_seed(1)
    shapes = [(700, 33), (5,), (9000,), (123, 7)]
    scales = [3.0, 0.01, 1e-4, 1.0]
    coefs = [0.0, 0.5, 30.0, 1e-2]                 # (the third variable's penalty decides whether it clips)
    ps = [torch.randn(s, generator=g) for s in shapes]
    gs = [torch.randn(s, generator=g) * c for s, c in zip(shapes, scales)]
    offs, cur = [], 0
    for p in ps:
        offs.append(cur)
        cur += (p.numel() + ARENA_ALIGN - 1) // ARENA_ALIGN * ARENA_ALIGN
    offs.append(cur)
    P, G, M, V = (torch.zeros(cur, device=dev) for _ in range(4))
    for p, gr, o in zip(ps, gs, offs):
        P[o:o + p.numel()] = p.flatten().to(dev)
        G[o:o + p.numel()] = gr.flatten().to(dev)
    offsets = torch.tensor(offs, dtype=torch.int64, device=dev)
    l2 = torch.tensor(coefs, dtype=torch.float32, device=dev)
    P2, M2, V2 = P.clone(), M.clone(), V.clone()
    ref_p = [p.double() for p in ps]
    ref_m = [torch.zeros_like(p).double() for p in ps]
    ref_v = [torch.zeros_like(p).double() for p in ps]
    for step in (1, 2, 3):
        ops.clip_adam_step(P, G, M, V, offsets, len(ps), 1.0, 2e-4, step, l2=l2)
        G2 = G.clone()
        for c, p, o in zip(coefs, ps, offs):
            G2[o:o + p.numel()].add_(P2[o:o + p.numel()], alpha=c)
        ops.clip_adam_step(P2, G2, M2, V2, offsets, len(ps), 1.0, 2e-4, step)
        cl = O.clip_gradient_norms({i: g_.double() + c * rp for i, (g_, c, rp) in enumerate(zip(gs, coefs, ref_p))}, 1.0)
        for i in range(len(ps)):
            ref_p[i], ref_m[i], ref_v[i] = O.adam_tf_update(ref_p[i], cl[i], ref_m[i], ref_v[i], 2e-4, step)
    for p, rp, rm, o in zip(ps, ref_p, ref_m, offs):
        assert_close(P[o:o + p.numel()].reshape(p.shape), rp, tol=1e-6, what="adam param (l2 on the fly)")
        assert_close(M[o:o + p.numel()].reshape(p.shape), rm, tol=1e-5, what="adam m (l2 on the fly)")
    assert_close(P, P2.double(), tol=1e-7, what="against the add pass + the plain entry point")
    assert_close(M, M2.double(), tol=1e-6, what="m against the add pass + the plain entry point")


@pytest.mark.parametrize("R,N1,N2,gscale", [(32, 1000, 64, 1.0), (80, 4096 + 96, 512, 1e-3), (128, 2048, 1024, 0.05), (160, 640, 128, 1.0)])
def test_factored_clip_adam_matches_oracle(R, N1, N2, gscale):
    """lpm_factored_clip_adam: the hidden projection's weight update straight from the two factors of its gradient (dW = X^T DY is
    never written) against clip_gradient_norms + adam_tf_update on the materialised fp64 gradient, three steps with changing factors;
    R = 160: two towers' tile buffers concatenated along R (the data-parallel form).  gscale puts the norm on either side of the clip."""
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    g = torch.Generator().manual_seed(R + N1)
    p0 = torch.randn(N1, N2, generator=g)
    P, M, V = p0.clone().to(dev), torch.zeros(N1, N2, device=dev), torch.zeros(N1, N2, device=dev)
    rp, rm, rv = p0.double(), torch.zeros(N1, N2, dtype=torch.float64), torch.zeros(N1, N2, dtype=torch.float64)
    fg = ops.FactoredGradient()
    clipped = []
    for step in (1, 2, 3):
        x = torch.randn(R, N1, generator=g)
        dy = torch.randn(R, N2, generator=g) * gscale
        fg.clear()
        if R == 160:                      # two towers: each splits its own 80 rows, the buffers are concatenated
            halves = []
            for h in range(2):
                t = ops.FactoredGradient()
                t.put(x[80 * h:80 * h + 80].to(dev), dy[80 * h:80 * h + 80].to(dev))
                halves.append(t)
            fg.xt, fg.dyt = torch.cat([t.xt for t in halves]), torch.cat([t.dyt for t in halves])
            fg.R, fg.N1, fg.N2 = R, N1, N2
        else:
            fg.put(x.to(dev), dy.to(dev))
        gref = x.double().t() @ dy.double()
        assert_close(fg.materialise(), gref, tol=2e-5, what="materialised factors")
        if R != 160:
            # the norm by both routes: a first tile-GEMM pass, and the quadratic forms x_n1^T (DY DY^T) x_n1 (lpm_factored_clip_adam_q)
            norms = []
            for quad in (False, True):
                ops.FACTORED_NORM_QUADFORM = quad
                Pc, Mc, Vc = P.clone(), M.clone(), V.clone()
                sc = fg.clip_adam(Pc.view(-1), Mc.view(-1), Vc.view(-1), 1.0, 2e-4, step)
                torch.cuda.synchronize()
                norms.append(float(sc[-3]))
            ops.FACTORED_NORM_QUADFORM = True
            assert abs(norms[0] - norms[1]) <= 2e-6 * norms[0], f"norm by GEMM pass {norms[0]} vs by quadratic forms {norms[1]}"
        scratch = fg.clip_adam(P.view(-1), M.view(-1), V.view(-1), 1.0, 2e-4, step)
        torch.cuda.synchronize()
        factor, norm = float(scratch[-4]), float(scratch[-3])
        assert abs(norm - float(gref.norm())) <= 1e-5 * float(gref.norm()), (norm, float(gref.norm()))
        assert abs(factor - 1.0 / max(float(gref.norm()), 1.0)) < 1e-5
        clipped.append(factor < 1.0)
        cl = O.clip_gradient_norms({0: gref}, 1.0)[0]
        rp, rm, rv = O.adam_tf_update(rp, cl, rm, rv, 2e-4, step)
    # (an element whose gradient is small against the tile GEMM's 5e-6-of-scale error moves by a visibly different fraction of lr)
    assert_close(P, rp, tol=3e-6, what="factored adam param")
    assert_close(M, rm, tol=2e-5, what="factored adam m")
    assert_close(V, rv, tol=4e-5, what="factored adam v")
    assert all(clipped) == (gscale * (R * N1 * N2) ** 0.5 > 1.0)


@pytest.mark.parametrize("B,T,D,K,bn", [(5, 300, 1024, 256, True), (3, 47, 256, 128, True), (2, 64, 128, 512, False), (80, 300, 1024, 256, True)])
def test_softmax_inside_the_aggregation_kernel_is_bitwise_the_two_kernel_chain(B, T, D, K, bn):
    """lpm_vlad_aggregate_raw_kmajor_smx_fwd (row statistics + ONE kernel: logits -> softmax -> residual sums, no assignment tiles)
    against lpm_assign_tiles + lpm_vlad_aggregate_raw_kmajor_fwd on the same logits: the same assignment bits enter the same MFMAs in
    the same order, so the un-normalised sums, the assignment sums and the partial norms must be IDENTICAL; and the chain itself
    against the fp64 oracle."""
    from learnablepoolingmethods_amd import _capi, ops
    from learnablepoolingmethods_amd.ops import ptr, stream_ptr
    dev = cuda()
    lib = _capi.load()
    assert lib._lpm_vlad_smx_supported(T, D, K)
    g = torch.Generator().manual_seed(B * T + K)
    x = torch.randn(B * T, D, generator=g)
    x = x / x.norm(dim=1, keepdim=True)
    logits = (torch.randn(B * T, K, generator=g) * 3).to(dev)
    scale = (1 + 0.3 * torch.randn(K, generator=g)).to(dev) if bn else None
    shift = (0.2 * torch.randn(K, generator=g)).to(dev)
    centres = (0.05 * torch.randn(D, K, generator=g)).to(dev)
    xd = x.to(dev)
    xt = torch.empty(lib._lpm_xt_bytes(B, T, D) // 4, dtype=torch.int32, device=dev)
    lib.check(lib._lpm_split_frames(ptr(xd), D, B, T, D, ptr(xt), stream_ptr()), "lpm_split_frames")
    flags = ops.LPM_VLAD_SOFTMAX | ops.LPM_VLAD_RESIDUAL
    P = D // 128
    out = {}
    for fused in (False, True):
        raw = torch.full((B, K, D), float("nan"), device=dev)
        asum, part = torch.empty(B, K, device=dev), torch.empty(B, P, K, device=dev)
        if fused:
            stats = torch.empty(lib._lpm_vlad_smx_stats_bytes(B, T) // 4, dtype=torch.float32, device=dev)
            lib.check(lib._lpm_vlad_aggregate_raw_kmajor_smx_fwd(ptr(logits), ptr(scale), ptr(shift), ptr(xt), ptr(centres), B, T, D, K, flags,
                                                                 ptr(raw), ptr(asum), ptr(part), ptr(stats), stream_ptr()), "smx")
        else:
            at = torch.empty(lib._lpm_at_bytes(B, T, K) // 4, dtype=torch.int32, device=dev)
            lib.check(lib._lpm_assign_tiles(ptr(logits), ptr(scale), ptr(shift), B, T, K, flags, ptr(at), stream_ptr()), "lpm_assign_tiles")
            lib.check(lib._lpm_vlad_aggregate_raw_kmajor_fwd(ptr(at), ptr(xt), ptr(centres), B, T, D, K, ops.LPM_VLAD_RESIDUAL, ptr(raw),
                                                             ptr(asum), ptr(part), stream_ptr()), "raw_kmajor")
        torch.cuda.synchronize()
        out[fused] = (raw, asum, part)
    for a, b, what in zip(out[True], out[False], ("un-normalised sums", "assignment sums", "partial norms")):
        assert torch.isfinite(a).all(), what
        assert torch.equal(a, b), f"{what}: fused softmax differs from the two-kernel chain (max abs {float((a - b).abs().max()):.3e})"
    # and against fp64: softmax(logits * scale + shift), U[b, k, d] = sum_t a x - (sum_t a) centres
    z = logits.double().cpu() * (scale.double().cpu() if bn else 1.0) + shift.double().cpu()
    a = torch.softmax(z, dim=1).reshape(B, T, K)
    U = torch.einsum("btk,btd->bkd", a, x.double().reshape(B, T, D)) - a.sum(1).unsqueeze(2) * centres.double().cpu().t().unsqueeze(0)
    assert_close(out[True][0], U, tol=2e-5, what="fused-softmax un-normalised sums")
    assert_close(out[True][1], a.sum(1), tol=2e-5, what="fused-softmax assignment sums")


@pytest.mark.parametrize("B,T,D,K,mode", [(80, 300, 1024, 256, "rounds"), (5, 300, 1024, 256, "all"), (5, 300, 1024, 256, "none"),
                                          (3, 47, 256, 128, "rounds"), (2, 64, 128, 512, "rounds"), (67, 33, 1024, 256, "rounds")])
def test_kmajor_scaled_aggregation_in_one_launch(B, T, D, K, mode):
    """lpm_vlad_aggregate_kmajor_scaled_fwd (vlad_kmajor.hip: K2 on wide workgroups at K = 256 + the row scales by the last workgroup
    of every clip, ONE launch) against the chain it replaces -- lpm_vlad_aggregate_raw_kmajor_fwd + lpm_vlad_row_scales -- on the same
    assignment tiles, and against fp64 (frame_level_models.py:2803-2822).  Every MFMA sees the same operands in the same order in
    both, so with 128 x 128 items only ("none", and any K != 256) the sums and the assignment sums must be IDENTICAL; a wide item adds
    its assignment sums in another (fixed) order, and the column norms are summed over d in another fixed order in every form:
    last-bit differences, held to 2e-6 of the tensor scale."""
    from learnablepoolingmethods_amd import _capi, ops
    from learnablepoolingmethods_amd.ops import ptr, stream_ptr
    dev = cuda()
    lib = _capi.load()
    g = torch.Generator().manual_seed(B * T + K + 1)
    x = torch.randn(B * T, D, generator=g)
    x = x / x.norm(dim=1, keepdim=True)
    logits = (torch.randn(B * T, K, generator=g) * 3).to(dev)
    scale = (1 + 0.3 * torch.randn(K, generator=g)).to(dev)
    shift = (0.2 * torch.randn(K, generator=g)).to(dev)
    centres = (0.05 * torch.randn(D, K, generator=g)).to(dev)
    xd = x.to(dev)
    xt = torch.empty(lib._lpm_xt_bytes(B, T, D) // 4, dtype=torch.int32, device=dev)
    lib.check(lib._lpm_split_frames(ptr(xd), D, B, T, D, ptr(xt), stream_ptr()), "lpm_split_frames")
    at = torch.empty(lib._lpm_at_bytes(B, T, K) // 4, dtype=torch.int32, device=dev)
    lib.check(lib._lpm_assign_tiles(ptr(logits), ptr(scale), ptr(shift), B, T, K, ops.LPM_VLAD_SOFTMAX | ops.LPM_VLAD_RESIDUAL, ptr(at),
                                    stream_ptr()), "lpm_assign_tiles")
    P = D // 128
    nan = float("nan")
    # the two-launch chain
    raw0 = torch.full((B, K, D), nan, device=dev)
    asum0, part0 = torch.empty(B, K, device=dev), torch.empty(B, P, K, device=dev)
    rs0, colsq0, csq0 = (torch.full((B, K), nan, device=dev) for _ in range(3))
    gsq0 = torch.full((B,), nan, device=dev)
    lib.check(lib._lpm_vlad_aggregate_raw_kmajor_fwd(ptr(at), ptr(xt), ptr(centres), B, T, D, K, ops.LPM_VLAD_RESIDUAL, ptr(raw0), ptr(asum0),
                                                     ptr(part0), stream_ptr()), "raw_kmajor")
    lib.check(lib._lpm_vlad_row_scales(ptr(part0), P, B, K, ptr(rs0), ptr(colsq0), ptr(csq0), ptr(gsq0), stream_ptr()), "row_scales")
    # one launch (twice into the same buffers: the per-call counters must start from zero each time)
    fl = ops.LPM_VLAD_RESIDUAL | {"rounds": 0, "all": _capi.LPM_VLAD_WIDE_ALL, "none": _capi.LPM_VLAD_WIDE_NONE}[mode]
    wsb = lib._lpm_vlad_kmajor_workspace_bytes(B, D, K)
    ws = torch.empty(wsb // 4, dtype=torch.float32, device=dev)
    for _ in range(2):
        raw1 = torch.full((B, K, D), nan, device=dev)
        asum1, rs1, colsq1, csq1 = (torch.full((B, K), nan, device=dev) for _ in range(4))
        gsq1 = torch.full((B,), nan, device=dev)
        lib.check(lib._lpm_vlad_aggregate_kmajor_scaled_fwd(ptr(at), ptr(xt), ptr(centres), B, T, D, K, fl, ptr(raw1), ptr(rs1), ptr(asum1),
                                                            ptr(colsq1), ptr(csq1), ptr(gsq1), ptr(ws), wsb, stream_ptr()), "kmajor_scaled")
    torch.cuda.synchronize()
    pairs = (("un-normalised sums", raw1, raw0), ("assignment sums", asum1, asum0), ("row scales", rs1, rs0), ("column norms", colsq1, colsq0),
             ("csq", csq1, csq0), ("gsq", gsq1, gsq0))
    wide = K == 256 and (mode == "all" or (mode == "rounds" and B >= 64))
    for what, a, b in pairs:
        assert torch.isfinite(a).all(), what
        if wide or what not in ("un-normalised sums", "assignment sums"):
            assert_close(a, b, tol=2e-6, what=what)      # (the column norms are summed over d in another fixed order than the chain's)
        else:
            assert torch.equal(a, b), f"{what}: differs from the two-launch chain (max abs {float((a - b).abs().max()):.3e})"
    if wide and mode == "rounds":           # the clips past the last whole round ran as 128 x 128 items: sums identical to the chain's
        nl = (B // 64) * 64
        assert torch.equal(raw1[nl:], raw0[nl:]) and torch.equal(asum1[nl:], asum0[nl:])
    z = logits.double().cpu() * scale.double().cpu() + shift.double().cpu()
    a = torch.softmax(z, dim=1).reshape(B, T, K)
    U = torch.einsum("btk,btd->bkd", a, x.double().reshape(B, T, D)) - a.sum(1).unsqueeze(2) * centres.double().cpu().t().unsqueeze(0)
    assert_close(raw1, U, tol=2e-5, what="un-normalised sums vs fp64")
    n = U.pow(2).sum(2)
    nrm = U / n.clamp_min(1e-12).sqrt().unsqueeze(2)
    want = nrm / nrm.pow(2).sum((1, 2)).clamp_min(1e-12).sqrt().view(B, 1, 1)
    assert_close(raw1.double().cpu() * rs1.double().cpu().unsqueeze(2), want, tol=2e-5, what="scaled descriptor vs fp64")


@pytest.mark.parametrize("B,T,D,K,residual", [(80, 300, 1024, 256, True), (5, 300, 1024, 256, False), (3, 47, 256, 256, True),
                                              (2, 64, 96, 256, True), (7, 33, 1152, 256, True), (4, 16, 384, 256, True)])
def test_clip_wide_aggregation(B, T, D, K, residual):
    """lpm_vlad_aggregate_clip_kmajor_fwd (vlad_clip.hip: all 256 clusters x a third of a clip's columns per workgroup, operand roles
    swapped so that everything per cluster is per lane) + lpm_vlad_row_scales against fp64 (frame_level_models.py:2803-2822) and -- where
    the 128 x 128 form covers the shape -- against lpm_vlad_aggregate_raw_kmajor_fwd on the same tiles: the same three MFMA terms in the
    same order over the same frame steps, so the un-normalised sums must be IDENTICAL when there is no residual (the assignment sums
    are added in another fixed order: last-bit differences with the residual)."""
    from learnablepoolingmethods_amd import _capi, ops
    from learnablepoolingmethods_amd.ops import ptr, stream_ptr
    dev = cuda()
    lib = _capi.load()
    g = torch.Generator().manual_seed(B * T + D + 5)
    x = torch.randn(B * T, D, generator=g)
    x = x / x.norm(dim=1, keepdim=True)
    logits = (torch.randn(B * T, K, generator=g) * 3).to(dev)
    scale = (1 + 0.3 * torch.randn(K, generator=g)).to(dev)
    shift = (0.2 * torch.randn(K, generator=g)).to(dev)
    centres = (0.05 * torch.randn(D, K, generator=g)).to(dev)
    xd = x.to(dev)
    xt = torch.empty(lib._lpm_xt_bytes(B, T, D) // 4, dtype=torch.int32, device=dev)
    lib.check(lib._lpm_split_frames(ptr(xd), D, B, T, D, ptr(xt), stream_ptr()), "lpm_split_frames")
    at = torch.empty(lib._lpm_at_bytes(B, T, K) // 4, dtype=torch.int32, device=dev)
    lib.check(lib._lpm_assign_tiles(ptr(logits), ptr(scale), ptr(shift), B, T, K, ops.LPM_VLAD_SOFTMAX | ops.LPM_VLAD_RESIDUAL, ptr(at),
                                    stream_ptr()), "lpm_assign_tiles")
    fl = ops.LPM_VLAD_RESIDUAL if residual else 0
    P = lib._lpm_vlad_clip_slabs(D, K)
    assert P == -(-(D // 32) // 11) and lib._lpm_vlad_clip_slabs(D, 128) == 0 and lib._lpm_vlad_clip_slabs(80, 256) == 0
    nan = float("nan")
    for _ in range(2):
        raw = torch.full((B, K, D), nan, device=dev)
        asum, part = torch.full((B, K), nan, device=dev), torch.full((B, P, K), nan, device=dev)
        rs, colsq, csq = (torch.full((B, K), nan, device=dev) for _ in range(3))
        gsq = torch.full((B,), nan, device=dev)
        lib.check(lib._lpm_vlad_aggregate_clip_kmajor_fwd(ptr(at), ptr(xt), ptr(centres), B, T, D, K, fl, ptr(raw), ptr(asum), ptr(part),
                                                          stream_ptr()), "clip_kmajor")
        lib.check(lib._lpm_vlad_row_scales(ptr(part), P, B, K, ptr(rs), ptr(colsq), ptr(csq), ptr(gsq), stream_ptr()), "row_scales")
    torch.cuda.synchronize()
    for what, t in (("sums", raw), ("assignment sums", asum), ("partial norms", part), ("row scales", rs), ("gsq", gsq)):
        assert torch.isfinite(t).all(), what
    z = logits.double().cpu() * scale.double().cpu() + shift.double().cpu()
    a = torch.softmax(z, dim=1).reshape(B, T, K)
    U = torch.einsum("btk,btd->bkd", a, x.double().reshape(B, T, D))
    if residual:
        U = U - a.sum(1).unsqueeze(2) * centres.double().cpu().t().unsqueeze(0)
    assert_close(raw, U, tol=2e-5, what="un-normalised sums vs fp64")
    assert_close(asum, a.sum(1), tol=2e-5, what="assignment sums vs fp64")
    n = U.pow(2).sum(2)
    assert_close(colsq, n, tol=2e-5, what="column norms vs fp64")
    nrm = U / n.clamp_min(1e-12).sqrt().unsqueeze(2)
    want = nrm / nrm.pow(2).sum((1, 2)).clamp_min(1e-12).sqrt().view(B, 1, 1)
    assert_close(raw.double().cpu() * rs.double().cpu().unsqueeze(2), want, tol=2e-5, what="scaled descriptor vs fp64")
    if lib._lpm_vlad_tiles3_supported(D, K):
        raw0 = torch.full((B, K, D), nan, device=dev)
        asum0, part0 = torch.empty(B, K, device=dev), torch.empty(B, D // 128, K, device=dev)
        lib.check(lib._lpm_vlad_aggregate_raw_kmajor_fwd(ptr(at), ptr(xt), ptr(centres), B, T, D, K, fl, ptr(raw0), ptr(asum0), ptr(part0),
                                                         stream_ptr()), "raw_kmajor")
        torch.cuda.synchronize()
        if residual:
            assert_close(raw, raw0, tol=2e-6, what="sums vs the 128 x 128 form")
        else:
            assert torch.equal(raw, raw0), f"sums differ from the 128 x 128 form (max abs {float((raw - raw0).abs().max()):.3e})"
        assert_close(asum, asum0, tol=2e-6, what="assignment sums vs the 128 x 128 form")


@pytest.mark.parametrize("Z,K,N,nouts", [(4, 128, 384, 3), (8, 64, 64, 1), (2, 96, 256, 2), (1, 32, 12, 3)])
def test_sum_splits_into_column_block_destinations(Z, K, N, nouts):
    """lpm_sum_splits: the split-K partial sums [Z, K, N] of a weight-gradient GEMM added in slice order into nouts separate [K, N / nouts]
    matrices (the q | k | v gradient slots) -- the same additions in the same order as torch.sum over the slices."""
    from learnablepoolingmethods_amd import _capi
    from learnablepoolingmethods_amd.ops import ptr, stream_ptr
    dev = cuda()
    lib = _capi.load()
    g = torch.Generator().manual_seed(Z * K + N)
    part = torch.randn(Z, K, N, generator=g).to(dev)
    outs = [torch.full((K, N // nouts), float("nan"), device=dev) for _ in range(nouts)]
    p = [ptr(o) for o in outs] + [None] * (3 - nouts)
    lib.check(lib._lpm_sum_splits(ptr(part), Z, K, N, p[0], p[1], p[2], nouts, stream_ptr()), "lpm_sum_splits")
    torch.cuda.synchronize()
    ref = part[0].clone()
    for z in range(1, Z):
        ref += part[z]
    for i, o in enumerate(outs):
        assert torch.equal(o, ref[:, i * (N // nouts):(i + 1) * (N // nouts)])
    assert lib._lpm_sum_splits(ptr(part), Z, K, N, p[0], None, None, 2, stream_ptr()) != 0      # a missing destination is refused


def test_weight_pack_matches_the_single_weight_entry_points():
    """lpm_weight_pack (weight_pack.hip): every operand form of a list of weights -- among them the column blocks of a concatenated
    q | k | v weight -- from ONE launch, bit for bit what lpm_split_weight / lpm_split_weight_tiles write one weight at a time
    (transformer_utils.py:559-561,583,701-711: the kernels of tf.layers.dense, constant within a step); and ops.WeightPack around it:
    nothing on the first armed step (the requests are recorded), everything from the second, nothing outside a step."""
    import ctypes as C
    from learnablepoolingmethods_amd import _capi, ops
    from learnablepoolingmethods_amd.ops import ptr, stream_ptr
    dev = cuda()
    lib = _capi.load()
    g = torch.Generator().manual_seed(3)
    Wq, Wk, Wv = (torch.randn(128, 96 if i == 1 else 64, generator=g).to(dev) for i in range(3))
    W1 = torch.randn(64, 256, generator=g).to(dev)
    W2 = torch.randn(256, 64, generator=g).to(dev)

    def single(W, need_t=True):
        K, N = W.shape
        w3n = torch.empty((N, 3 * K), dtype=torch.bfloat16, device=dev)
        w3k = torch.empty((K, 3 * N), dtype=torch.bfloat16, device=dev) if need_t else None
        lib.check(lib._lpm_split_weight(ptr(W), K, N, ptr(w3n), ptr(w3k), stream_ptr()), "split_weight")
        return w3n, w3k

    def tiles(W, R, N, tr):
        wt = torch.empty(lib._lpm_weight_tiles_bytes(R, N) // 4, dtype=torch.int32, device=dev)
        lib.check(lib._lpm_split_weight_tiles(ptr(W), R, N, tr, ptr(wt), stream_ptr()), "split_weight_tiles")
        return wt
    cat = torch.cat([Wq, Wk, Wv], 1)
    want = {"qkv": single(cat), "w1": (single(W1)[1], tiles(W1, 64, 256, 0)), "w2": (single(W2, False)[0], tiles(W2, 64, 256, 1))}
    pack = ops.WeightPack()
    assert pack.take([W1], ["k"]) is None                       # not armed: consumers compute their own
    for step in range(3):
        pack.begin_step()
        got_qkv = pack.take([Wq, Wk, Wv], ["n", "k"])
        got_w1 = pack.take([W1], ["k", "wt"])
        got_w2 = pack.take([W2.detach()], ["n", "wtt"])          # (a fresh tensor object over the same storage: autograd's saved weight)
        if step == 0:
            assert got_qkv is None and got_w1 is None and got_w2 is None
        else:
            torch.cuda.synchronize()
            assert torch.equal(got_qkv["n"], want["qkv"][0]) and torch.equal(got_qkv["k"], want["qkv"][1])
            assert torch.equal(got_w1["k"], want["w1"][0]) and torch.equal(got_w1["wt"], want["w1"][1])
            assert torch.equal(got_w2["n"], want["w2"][0]) and torch.equal(got_w2["wtt"], want["w2"][1])
        pack.end_step()
    assert len(pack.plan) == 3
    # shapes the kernel does not take go through the consumers' own calls: never recorded, never an error
    pack.begin_step()
    assert pack.take([torch.randn(40, 64, device=dev)], ["n"]) is None and len(pack.plan) == 3
    pack.end_step()
    # the C entry refuses what it cannot do
    j = _capi.WeightPackJob()
    j.w, j.K, j.N, j.ldw, j.Ntot, j.n_off, j.w3n = W1.data_ptr(), 64, 250, 256, 250, 0, want["w1"][0].data_ptr()
    arr = (_capi.WeightPackJob * 1)(j)
    assert lib._lpm_weight_pack(C.cast(arr, C.c_void_p), 1, stream_ptr()) != 0 and "N % 32" in lib.last_error().replace("%%", "%")


@pytest.mark.parametrize("M,C,relu", [(24000, 4096, True), (1200, 256, True), (777, 128, False), (20000, 1024, False)])
def test_bias_act_in_place(M, C, relu):
    """ops.bias_act: tf.layers.dense's bias add (+ ReLU) as one in-place pass; backward = ReLU mask from the saved output + the bias
    gradient's column sums, against autograd on the plain formula."""
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    g = torch.Generator().manual_seed(M + C)
    y0, b0, dy = torch.randn(M, C, generator=g), torch.randn(C, generator=g), torch.randn(M, C, generator=g)
    yd, bd = y0.double().requires_grad_(True), b0.double().requires_grad_(True)
    ref = yd + bd
    ref = torch.relu(ref) if relu else ref
    ref.backward(dy.double())
    src = y0.to(dev).requires_grad_(True)
    bg = b0.to(dev).requires_grad_(True)
    pre = src * 1.0                      # a fresh non-leaf tensor, as a GEMM's output is
    assert ops.bias_act_ok(pre, bg)
    out = ops.bias_act(pre, bg, relu)
    assert out.data_ptr() == pre.data_ptr(), "in place"
    assert_close(out, ref.detach(), tol=1e-6, what="bias_act fwd")
    out.backward(dy.to(dev))
    assert_close(src.grad, yd.grad, tol=1e-6, what="bias_act dx")
    assert_close(bg.grad, bd.grad, tol=2e-5, what="bias_act dbias")


def test_capi_rejects_bad_shapes_loudly():
    from learnablepoolingmethods_amd import _capi, ops
    dev = cuda()
    x = torch.randn(10, 100, device=dev)     # D = 100 unsupported
    W = torch.randn(100, 8, device=dev)
    with pytest.raises(_capi.LpmError):
        ops.netvlad(x, W, None, 5, bn=None, bias=torch.zeros(8, device=dev))
    with pytest.raises(_capi.LpmError):
        ops.mha_core(torch.randn(1, 8, 24, device=dev), torch.randn(1, 8, 24, device=dev), torch.randn(1, 8, 24, device=dev), 2, 1.0)


@pytest.mark.parametrize("M,K,N", [(2048, 1024, 1024), (4096, 128, 512), (1536, 4096, 1024)])
def test_dense_split_bf16(M, K, N):
    """Encoder dense layers on the bf16 pipe with split operands: fp32-grade accuracy forward and backward."""
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    g = torch.Generator().manual_seed(M)
    x, W, dy = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g) / K ** 0.5, torch.randn(M, N, generator=g)
    xd, Wd = x.double().requires_grad_(True), W.double().requires_grad_(True)
    (xd @ Wd).backward(dy.double())
    xg, Wg = x.to(dev).requires_grad_(True), W.to(dev).requires_grad_(True)
    y = ops.dense_x3(xg, Wg)
    assert_close(y, (xd @ Wd).detach(), tol=5e-5, what="dense_x3 fwd")
    y.backward(dy.to(dev))
    assert_close(xg.grad, xd.grad, tol=5e-5, what="dense_x3 dx")
    assert_close(Wg.grad, Wd.grad, tol=5e-5, what="dense_x3 dW")


@pytest.mark.parametrize("B,L,F,res", [(3, 256, 1024, True), (2, 64, 128, True), (4, 300, 128, False), (2, 7, 256, True)])
def test_residual_layer_norm(B, L, F, res):
    """tf.contrib.layers.layer_norm defaults (joint moments over L*F) with the residual add fused."""
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    g = torch.Generator().manual_seed(L)
    a, r, dy = (torch.randn(B, L, F, generator=g) for _ in range(3))
    gamma, beta = 1 + 0.2 * torch.randn(F, generator=g), 0.1 * torch.randn(F, generator=g)
    p = {"ln/gamma": gamma.double().requires_grad_(True), "ln/beta": beta.double().requires_grad_(True)}
    ad, rd = a.double().requires_grad_(True), r.double().requires_grad_(True)
    ref = O.layer_norm(ad + rd if res else ad, p, "ln")
    ref.backward(dy.double())
    ag, rg, gg, bg = (t.to(dev).requires_grad_(True) for t in (a, r, gamma, beta))
    y = ops.residual_layer_norm(ag, rg if res else None, gg, bg)
    assert_close(y, ref, tol=1e-5, what="layer_norm fwd")
    y.backward(dy.to(dev))
    assert_close(ag.grad, ad.grad, tol=1e-4, what="layer_norm da")
    if res:
        assert_close(rg.grad, rd.grad, tol=1e-4, what="layer_norm dr")
    assert_close(gg.grad, p["ln/gamma"].grad, tol=1e-4, what="layer_norm dgamma")
    assert_close(bg.grad, p["ln/beta"].grad, tol=1e-4, what="layer_norm dbeta")


@pytest.mark.parametrize("B,L,F,res,relu", [(3, 256, 1024, True, True), (2, 64, 128, True, False), (4, 300, 128, False, True),
                                             (2, 7, 256, True, True)])
def test_residual_layer_norm_fused_bias_activation(B, L, F, res, relu):
    """layer_norm(act(a + bias) + r): the dense layer's bias add / ReLU fused into the residual layer norm
    (transformer_utils.py:583 + :405-407 and :708-713), backward incl. dbias and the ReLU mask."""
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    g = torch.Generator().manual_seed(L + F)
    a, r, dy = (torch.randn(B, L, F, generator=g) for _ in range(3))
    gamma, beta = 1 + 0.2 * torch.randn(F, generator=g), 0.1 * torch.randn(F, generator=g)
    bias = 0.3 * torch.randn(F, generator=g)
    p = {"ln/gamma": gamma.double().requires_grad_(True), "ln/beta": beta.double().requires_grad_(True)}
    ad, rd, bd = a.double().requires_grad_(True), r.double().requires_grad_(True), bias.double().requires_grad_(True)
    t = ad + bd
    if relu:
        t = torch.relu(t)
    ref = O.layer_norm(t + rd if res else t, p, "ln")
    ref.backward(dy.double())
    ag, rg, gg, bg, biasg = (x.to(dev).requires_grad_(True) for x in (a, r, gamma, beta, bias))
    y = ops.residual_layer_norm(ag, rg if res else None, gg, bg, bias=biasg, relu=relu)
    assert_close(y, ref, tol=1e-5, what="layer_norm fwd")
    y.backward(dy.to(dev))
    assert_close(ag.grad, ad.grad, tol=1e-4, what="layer_norm da")
    if res:
        assert_close(rg.grad, rd.grad, tol=1e-4, what="layer_norm dr")
    assert_close(gg.grad, p["ln/gamma"].grad, tol=1e-4, what="layer_norm dgamma")
    assert_close(bg.grad, p["ln/beta"].grad, tol=1e-4, what="layer_norm dbeta")
    assert_close(biasg.grad, bd.grad, tol=1e-4, what="layer_norm dbias")


@pytest.mark.parametrize("B,L,F,relu,image,dtype", [(3, 300, 1024, False, True, torch.uint8), (2, 64, 128, False, False, torch.bool),
                                                       (2, 7, 256, True, True, torch.uint8)])
def test_residual_layer_norm_with_a_dropout_between_dense_and_norm(B, L, F, relu, image, dtype):
    """layer_norm(dropout(act(a + bias)) + r) with the keep mask applied inside the layer norm's passes (NetVladV2's encoder:
    tf.layers.dropout between output_transform and the layer norm, transformer_utils.py:450-454): forward, the operand image, the gradient
    of the dense layer's raw output through the mask, dbias, the residual's gradient -- against fp64 autograd of the separate steps."""
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    g = torch.Generator().manual_seed(L + F)
    a, r, dy = (torch.randn(B, L, F, generator=g) for _ in range(3))
    gamma, beta = 1 + 0.2 * torch.randn(F, generator=g), 0.1 * torch.randn(F, generator=g)
    bias = 0.3 * torch.randn(F, generator=g)
    keep, rate = (torch.rand(B, L, F, generator=g) < 0.1), 0.9
    p = {"ln/gamma": gamma.double().requires_grad_(True), "ln/beta": beta.double().requires_grad_(True)}
    ad, rd, bd = a.double().requires_grad_(True), r.double().requires_grad_(True), bias.double().requires_grad_(True)
    t = ad + bd
    if relu:
        t = torch.relu(t)
    ref = O.layer_norm(t * keep.double() / (1.0 - rate) + rd, p, "ln")
    ref.backward(dy.double())
    ag, rg, gg, bg, biasg = (x.to(dev).requires_grad_(True) for x in (a, r, gamma, beta, bias))
    y = ops.residual_layer_norm(ag, rg, gg, bg, bias=biasg, relu=relu, image=image, mask=keep.to(dtype).to(dev), mask_scale=1.0 / (1.0 - rate))
    assert_close(y, ref, tol=1e-5, what="layer_norm fwd")
    if image:
        y3, _, _ = y._lpm_y3
        hi, lo = y3[:, :F].float(), y3[:, F:2 * F].float()
        assert torch.equal(y3[:, 2 * F:], y3[:, :F])
        assert_close(hi + lo, ref.reshape(B * L, F), tol=2e-5, what="operand image hi + lo")
    y.backward(dy.to(dev))
    assert_close(ag.grad, ad.grad, tol=1e-4, what="layer_norm da (through the dropout)")
    assert float(ag.grad[~keep.to(dev)].abs().max()) == 0.0, "dropped elements must receive no gradient"
    assert_close(rg.grad, rd.grad, tol=1e-4, what="layer_norm dr")
    assert_close(gg.grad, p["ln/gamma"].grad, tol=1e-4, what="layer_norm dgamma")
    assert_close(bg.grad, p["ln/beta"].grad, tol=1e-4, what="layer_norm dbeta")
    assert_close(biasg.grad, bd.grad, tol=1e-4, what="layer_norm dbias")


def test_dropout_keep_mask_is_a_repeatable_bernoulli_draw():
    """lpm_dropout_keep_mask (round 6): the keep mask of tf.layers.dropout (transformer_utils.py:450, keep probability 0.1) as one launch
    -- bytes are 0 / 1, the kept fraction is keep_prob to four standard deviations overall, per frame row and per feature column, a
    neighbour's state says nothing about an element's, the same torch seed gives the same mask and another seed another one."""
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    B, L, F, p = 80, 300, 1024, 0.1
    torch.manual_seed(5)
    m1 = ops.dropout_keep_mask((B, L, F), p, dev)
    m2 = ops.dropout_keep_mask((B, L, F), p, dev)
    torch.manual_seed(5)
    m1b = ops.dropout_keep_mask((B, L, F), p, dev)
    assert m1.dtype == torch.uint8 and int(m1.max()) == 1 and int(m1.min()) == 0
    assert torch.equal(m1, m1b) and not torch.equal(m1, m2)
    k = m1.float()
    n = k.numel()
    sd = (p * (1 - p)) ** 0.5
    assert abs(float(k.mean()) - p) < 4 * sd / n ** 0.5
    assert float((k.mean(dim=2) - p).abs().max()) < 6 * sd / F ** 0.5                    # every frame row (24 000 of them: 6 sigma)
    assert float((k.mean(dim=(0, 1)) - p).abs().max()) < 5 * sd / (B * L) ** 0.5          # every feature column
    for a, b in ((k[..., 1:], k[..., :-1]), (k[:, 1:], k[:, :-1]), (m1.float(), m2.float())):
        cov = float((a * b).mean()) - float(a.mean()) * float(b.mean())
        assert abs(cov) < 5 * p * (1 - p) / a.numel() ** 0.5, "neighbouring elements / successive masks must be uncorrelated"
    # other keep probabilities, 16-bit resolution
    for q in (0.5, 0.9, 1.0):
        assert abs(float(ops.dropout_keep_mask((64, 4096), q, dev).float().mean()) - q) < 4 * max((q * (1 - q)) ** 0.5, 1e-3) / (64 * 4096) ** 0.5 + 2e-5


@pytest.mark.parametrize("B,L,F,fmt", [(3, 300, 1024, "fp16"), (2, 64, 128, "bf16x3"), (2, 300, 128, None)])
def test_masked_layer_norm_backward_writes_the_gradient_image(B, L, F, fmt):
    """lpm_layer_norm_act_mask_bwd_fmt (round 6): the gradient of the dense layer's raw output THROUGH the dropout mask leaves the layer
    norm's backward as that layer's operand image (the V2 encoder's attention half as one node) -- bit for bit lpm_split_rows of the fp32
    gradient the plain form returns, in the same operand format, with the same recorded max |x|; the residual's gradient with a second
    gradient added on the way out (ops.GradJoin's share) is dz + extra."""
    from learnablepoolingmethods_amd import _capi, ops
    dev = cuda()
    g = torch.Generator().manual_seed(B + L + F)
    a, r, dy, extra = (torch.randn(B, L, F, generator=g).to(dev) for _ in range(4))
    gamma, beta = (1 + 0.2 * torch.randn(F, generator=g)).to(dev), (0.1 * torch.randn(F, generator=g)).to(dev)
    bias = (0.3 * torch.randn(F, generator=g)).to(dev)
    keep = (torch.rand(B, L, F, generator=g) < 0.1).to(torch.uint8).to(dev)
    ctx = ops._SubCtx()
    ops._ResidualLayerNorm.forward(ctx, a, r, gamma, beta, bias, False, None, None, image=False, mask=keep, mask_scale=10.0, site=None)
    plain = ops._ResidualLayerNorm.backward(ctx, dy)
    da, dz = plain[0], plain[1]
    amax_a = torch.zeros(_capi.LPM_OPERAND_AMAX_SUB * _capi.LPM_OPERAND_AMAX_STRIDE, device=dev)
    amax_b = torch.zeros_like(amax_a)
    mk = lambda amax: None if fmt is None else ops.OperandSite(fmt == "fp16", 2.0 ** 7, amax.data_ptr(), role="g")
    want = ops._split_rows(da.reshape(B * L, F), grad=True, site=mk(amax_a))
    got = ops._ResidualLayerNorm.backward(ctx, dy, dr_extra=extra, da_image=True, site=mk(amax_b))
    assert got[0].dtype == want.dtype and tuple(got[0].shape) == tuple(want.shape)
    assert torch.equal(got[0].view(torch.int16), want.view(torch.int16))
    assert_close(got[1], (dz + extra).double(), tol=1e-6, what="residual gradient + the second gradient")
    for i in (2, 3, 4):
        assert torch.equal(got[i], plain[i])                # dgamma, dbeta, dbias: the same passes
    if fmt is not None:
        assert float(amax_b.max()) == float(amax_a.max()) == float(da.abs().max())


@pytest.mark.parametrize("M,F,C,N", [(2400, 128, 512, 64), (24000, 1024, 4096, 256)])
def test_ffn_mod_one_node(M, F, C, N):
    """FeedForwardNetworkMod up to its second dense layer, BN(relu(y W1 + b1)) W2 (transformer_utils.py:741-756), as ONE node
    (ops.ffn_mod_x3: the batch norm writes only the second GEMM's operand image, its backward only the first layer's gradient image)
    against fp64 autograd and against the separate nodes it replaces (dense_x3 -> batch_norm_rows_act -> dense_x3): values, every
    gradient, moving statistics.  (24000 x 1024 x 4096 x 256 = NetVladV2's video encoder at cfg-3.)"""
    from learnablepoolingmethods_amd import ops
    from tests._util import rel_l2
    dev = cuda()
    g = torch.Generator().manual_seed(M + C)
    y, W1, b1 = torch.randn(M, F, generator=g), torch.randn(F, C, generator=g) / F ** .5, 0.3 * torch.randn(C, generator=g)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    W2, dout = torch.randn(C, N, generator=g) / C ** .5, torch.randn(M, N, generator=g)
    yd, W1d, b1d, gd, bd, W2d = (t.double().requires_grad_(True) for t in (y, W1, b1, gamma, beta, W2))
    a = torch.relu(yd @ W1d + b1d)
    mu, var = a.mean(0), a.var(0, unbiased=False)
    ref = ((a - mu) * torch.rsqrt(var + 1e-3) * gd + bd) @ W2d
    ref.backward(dout.double())
    outs = {}
    for fused in (True, False):
        t = [x.to(dev).requires_grad_(True) for x in (y, W1, b1, gamma, beta, W2)]
        mm, mv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        if fused:
            out = ops.ffn_mod_x3(t[0], t[1], t[2], t[3], t[4], mm, mv, t[5])
        else:
            pre = ops.dense_x3(t[0], t[1])
            f = ops.batch_norm_rows_act(pre, t[2], True, t[3], t[4], mm, mv, True)
            out = ops.dense_x3(f, t[5])
        out.backward(dout.to(dev))
        outs[fused] = (out.detach(), [x.grad for x in t], mm, mv)
    out, grads, mm, mv = outs[True]
    assert_close(out, ref, tol=5e-5, what="ffn_mod forward")
    assert_close(mm, 0.001 * mu, tol=1e-4, what="moving mean")
    assert_close(mv, 0.999 + 0.001 * var, tol=1e-4, what="moving variance (biased: rank-3 slim.batch_norm)")
    for got, want, nm in zip(grads, (yd, W1d, b1d, gd, bd, W2d), ("dy", "dW1", "db1", "dgamma", "dbeta", "dW2")):
        e = rel_l2(got, want.grad)
        assert e <= 5e-3, f"ffn_mod {nm}: relative L2 error {e:.3e}"          # (ReLU units within rounding of zero flip: see the FFN test below)
    # the two routes compute the same thing from the same GEMMs: agreement far below the ReLU-flip noise against fp64
    o2, g2, mm2, mv2 = outs[False]
    assert_close(out, o2, tol=2e-6, what="one node vs separate nodes")
    for a_, b_, nm in zip(grads, g2, ("dy", "dW1", "db1", "dgamma", "dbeta", "dW2")):
        assert rel_l2(a_, b_) <= 2e-5, f"one node vs separate nodes, {nm}: {rel_l2(a_, b_):.3e}"
    assert torch.equal(mm, mm2) and torch.equal(mv, mv2)


@pytest.mark.parametrize("M,K,N", [(2048, 512, 768), (1984, 256, 512), (20480, 1024, 1024)])
@pytest.mark.parametrize("form", [1, 2, 3, 4])
def test_dense_tile_gemm_forms(M, K, N, form):
    """lpm_dense_tiles_fwd: an encoder dense layer y = x W (transformer_utils.py:559-561,583,701-711) on the split-bf16 tile GEMM in its
    four workgroup forms -- 64-row, 128-row pipelined (K1's), 128-row with two workgroups per CU, 256-row with four row tiles per wave --
    against fp64.  A form whose shape conditions do not hold (1984 rows = 62 row tiles: not a multiple of 4 or 8) must fall back to the
    64-row form, not fail: same result either way."""
    from learnablepoolingmethods_amd import _capi
    from learnablepoolingmethods_amd.ops import ptr, stream_ptr
    dev = cuda()
    lib = _capi.load()
    g = torch.Generator().manual_seed(M + K + N)
    x = torch.randn(M, K, generator=g)
    W = torch.randn(K, N, generator=g) / K ** 0.5
    xd, Wd = x.to(dev), W.to(dev)
    xr = torch.empty(lib._lpm_row_tiles_bytes(1, M, K) // 4, dtype=torch.int32, device=dev)
    wt = torch.empty(lib._lpm_weight_tiles_bytes(K, N) // 4, dtype=torch.int32, device=dev)
    lib.check(lib._lpm_split_rows_tiles(ptr(xd), K, 1, M, K, ptr(xr), stream_ptr()), "rows")
    lib.check(lib._lpm_split_weight_tiles(ptr(Wd), K, N, 0, ptr(wt), stream_ptr()), "weight")
    y = torch.full((M, N), float("nan"), device=dev)
    lib.check(lib._lpm_dense_tiles_fwd(ptr(xr), ptr(wt), M, K, N, ptr(y), N, form, stream_ptr()), "dense")
    torch.cuda.synchronize()
    ref = x.double() @ W.double()
    assert torch.isfinite(y).all()
    assert_close(y, ref, tol=2e-5, what=f"dense tiles form {form}")


@pytest.mark.parametrize("M,F,H,tiles", [(2048, 128, 512, False), (2048, 256, 1024, True), (20480, 1024, 4096, True), (2048, 256, 1024, False)])
def test_ffn_split_bf16_fused_bias_relu(M, F, H, tiles):
    """FeedForwardNetwork core relu(y W1 + b1) W2 (transformer_utils.py:701-711) with the inner bias + ReLU fused into the operand
    split -- as a separate pass behind the library GEMM, or (tiles: M % 256 == 0, F >= 256, H % 256 == 0; cfg-2's video encoder is
    the 20480 x 1024 x 4096 case) in the epilogue of the hand-written 256-row tile GEMM, whose backward twin applies the ReLU mask,
    sums the bias gradient and splits the result."""
    from learnablepoolingmethods_amd import _capi, ops
    dev = cuda()
    g = torch.Generator().manual_seed(3)
    old = ops.FFN_TILES
    ops.FFN_TILES = tiles
    assert bool(_capi.load()._lpm_dense_tiles_supported(M, F, H)) == (F >= 256)
    y, W1, b1, W2, dout = (torch.randn(M, F, generator=g), torch.randn(F, H, generator=g) / F ** .5, 0.3 * torch.randn(H, generator=g),
                           torch.randn(H, F, generator=g) / H ** .5, torch.randn(M, F, generator=g))
    yd, W1d, b1d, W2d = (t.double().requires_grad_(True) for t in (y, W1, b1, W2))
    ref = torch.relu(yd @ W1d + b1d) @ W2d
    ref.backward(dout.double())
    yg, W1g, b1g, W2g = (t.to(dev).requires_grad_(True) for t in (y, W1, b1, W2))
    out = ops.ffn_x3(yg, W1g, b1g, W2g)
    assert_close(out, ref, tol=5e-5, what="ffn fwd")
    out.backward(dout.to(dev))
    # Frobenius norm: a pre-activation within the GEMM's rounding of zero flips its ReLU mask (a handful of the 1M
    # units here), which moves single gradient entries by O(1) in max-norm without being an error of either side
    from tests._util import rel_l2
    for got, want, nm in ((yg, yd, "dy"), (W1g, W1d, "dW1"), (b1g, b1d, "db1"), (W2g, W2d, "dW2")):
        e = rel_l2(got.grad, want.grad)
        assert e <= 5e-3, f"ffn {nm}: relative L2 error {e:.3e}"
    # and the flips must be isolated: all but a few rows of dy agree to 1e-4 of the tensor scale
    err = (yg.grad.double().cpu() - yd.grad).abs().amax(dim=1) / yd.grad.abs().max()
    assert int((err > 1e-4).sum()) <= max(20, M // 100), f"{int((err > 1e-4).sum())} of {M} dy rows differ: not ReLU-flip noise"
    ops.FFN_TILES = old


@pytest.mark.parametrize("B,KV,H", [(80, 33792, 512), (16, 4224, 64), (6, 2048, 96), (128, 16896, 1024), (13, 2064, 512), (48, 4112, 512),
                                    (80, 270336, 512), (1, 2048, 1024), (97, 1168, 512), (90, 4112, 512), (65, 8208, 1024)])
def test_projection_skinny_gemms(B, KV, H):
    """VLAD -> hidden1 projection (frame_level_models.py:2314-2319): forward and dx by the weight-stream kernels (csrc/proj_gemm.hip:
    H a multiple of 512; cfg-2's and cfg-5's shapes, ragged row counts, an odd number of 16-row slabs) or the library (the other
    shapes), and the weight gradient written by the tile GEMM straight into a caller-owned buffer (the trainer's gradient arena)."""
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    g = torch.Generator().manual_seed(B + H)
    x = torch.randn(B, KV, generator=g).to(dev).requires_grad_(True)
    W = (torch.randn(KV, H, generator=g) / KV ** 0.5).to(dev).requires_grad_(True)
    dy = torch.randn(B, H, generator=g).to(dev)
    view = torch.full((KV, H), float("nan"), device=dev)
    W._lpm_grad_view = view
    old = ops.PROJ_DX_STREAM_MIN_N
    ops.PROJ_DX_STREAM_MIN_N = 512            # the hand-written dx kernel on every shape it supports, not only where it is the default
    try:
        y = ops.projection(x, W)
        y.backward(dy)
    finally:
        ops.PROJ_DX_STREAM_MIN_N = old
    x64, W64, dy64 = x.detach().double().cpu(), W.detach().double().cpu(), dy.double().cpu()
    assert_close(y, x64 @ W64, 2e-5, "y")
    assert_close(x.grad, dy64 @ W64.t(), 2e-5, "dx")
    assert_close(view, x64.t() @ dy64, 2e-5, "dW")
    assert W.grad is None and W._lpm_grad_written, "the weight gradient lives in the caller's buffer only"
    del W._lpm_grad_view                       # without a caller-owned buffer the gradient goes through autograd
    ops.projection(x, W).backward(dy)
    assert_close(W.grad, x64.t() @ dy64, 2e-5, "dW (autograd path)")


@pytest.mark.parametrize("B,D,K,NA,H,factored", [(80, 1024, 256, 8192, 512, True), (16, 128, 128, 0, 512, False), (13, 256, 128, 2048, 512, False),
                                                  (96, 128, 256, 64, 1024, True), (128, 128, 128, 512, 512, True)])
def test_projection_parts(B, D, K, NA, H, factored):
    """The projection of a lazily normalised d-major descriptor (frame_level_models.py:2445 + :2319 with the normalisation of
    video_pooling_modules.py:1655-1658 applied where the operand is read): y = [x1 * scale | x2] . W, dx as views of one buffer, the weight
    gradient from tiles that carry the scale -- through the caller-owned buffer, autograd, and the factored route's operands."""
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    g = torch.Generator().manual_seed(B + K + NA)
    raw = (torch.randn(B, D * K, generator=g) * 3).to(dev)
    scale = (torch.rand(B, K, generator=g) + 0.5).to(dev) / (D * K) ** 0.5
    x2 = (torch.randn(B, NA, generator=g) / max(NA, 1) ** 0.5).to(dev).requires_grad_(True) if NA else None
    Kd = D * K + NA
    W = (torch.randn(Kd, H, generator=g) / Kd ** 0.5).to(dev).requires_grad_(True)
    dy = torch.randn(B, H, generator=g).to(dev)
    x1 = raw.clone().requires_grad_(True)
    x1._lpm_row_scale, x1._lpm_scale_ks = scale, K
    assert ops.projection_parts_ok(x1, scale, K, x2, W)
    xm = (raw.double().cpu().view(B, D, K) * scale.double().cpu().unsqueeze(1)).reshape(B, D * K)
    x64 = torch.cat([xm, x2.detach().double().cpu()], 1) if NA else xm
    W64, dy64 = W.detach().double().cpu(), dy.double().cpu()
    assert_close(ops.materialise(x1), xm, 1e-6, "materialise (d-major)")
    view = torch.full((Kd, H), float("nan"), device=dev)
    W._lpm_grad_view = view
    y = ops.projection_parts(x1, x2, W)
    y.backward(dy)
    assert_close(y, x64 @ W64, 2e-5, "y")
    dx = dy64 @ W64.t()
    assert_close(x1.grad, dx[:, :D * K], 2e-5, "dx1 (w.r.t. the normalised descriptor)")
    if NA:
        assert_close(x2.grad, dx[:, D * K:], 2e-5, "dx2")
    if B % 16 == 0:
        assert_close(view, x64.t() @ dy64, 2e-5, "dW")
        assert W.grad is None and W._lpm_grad_written
    del W._lpm_grad_view, W._lpm_grad_written
    W.grad = None
    ops.projection_parts(x1, x2, W).backward(dy)
    assert_close(W.grad, x64.t() @ dy64, 2e-5, "dW (autograd path)")
    if factored:
        fg = ops.FactoredGradient()
        fg.armed = True
        W._lpm_factored = fg
        W.grad = None
        ops.projection_parts(x1, x2, W).backward(dy)
        assert W.grad is None and fg.pending and fg.x_in_tiles
        assert_close(fg.materialise(), x64.t() @ dy64, 2e-5, "dW from the factored operands")
        # clip + Adam from the tiles, the norm by the quadratic forms over the tiles
        param = W.detach().clone().reshape(-1)
        m, v = torch.zeros_like(param), torch.zeros_like(param)
        sc = fg.clip_adam(param, m, v, 1.0, 1e-3, 1)
        gref = x64.t() @ dy64
        nrm = float(gref.norm())
        assert abs(float(sc[-3]) - nrm) <= 1e-4 * nrm, "gradient norm from the quadratic forms"
        gc = gref * (1.0 / max(nrm, 1.0))
        assert_close(m.view(Kd, H), 0.1 * gc, 1e-4, "Adam m after one step")
        del W._lpm_factored


def test_projection_parts_bf16_sums_behind_a_handle():
    """bf16 storage (BASELINE configs[4]): the un-normalised sums are bf16, autograd sees an fp32 handle of the descriptor's shape that
    is never written (ops._NetVLAD._forward_bf16, lazy); forward, dx and the weight-gradient tiles read the bf16 sums x the scale."""
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    B, D, K, NA, H = 32, 128, 128, 256, 512
    g = torch.Generator().manual_seed(5)
    raw = (torch.randn(B, D * K, generator=g) * 3).to(dev).to(torch.bfloat16)
    scale = (torch.rand(B, K, generator=g) + 0.5).to(dev) / (D * K) ** 0.5
    x2 = (torch.randn(B, NA, generator=g) / NA ** 0.5).to(dev).requires_grad_(True)
    Kd = D * K + NA
    W = (torch.randn(Kd, H, generator=g) / Kd ** 0.5).to(dev).requires_grad_(True)
    dy = torch.randn(B, H, generator=g).to(dev)
    handle = torch.full((B, D * K), float("nan"), device=dev).requires_grad_(True)
    handle._lpm_row_scale, handle._lpm_scale_ks, handle._lpm_raw = scale, K, raw
    xm = (raw.double().cpu().view(B, D, K) * scale.double().cpu().unsqueeze(1)).reshape(B, D * K)
    x64 = torch.cat([xm, x2.detach().double().cpu()], 1)
    W64, dy64 = W.detach().double().cpu(), dy.double().cpu()
    assert_close(ops.materialise(handle), xm, 1e-6, "materialise (bf16 sums)")
    y = ops.projection_parts(handle, x2, W)
    y.backward(dy)
    assert_close(y, x64 @ W64, 2e-5, "y")
    dx = dy64 @ W64.t()
    assert handle.grad.dtype == torch.float32
    assert_close(handle.grad, dx[:, :D * K], 2e-5, "dx1")
    assert_close(x2.grad, dx[:, D * K:], 2e-5, "dx2")
    assert_close(W.grad, x64.t() @ dy64, 2e-5, "dW")


@pytest.mark.parametrize("B,D,K,NA,H", [(32, 128, 128, 256, 512), (128, 128, 512, 128 * 16, 1024), (80, 64, 96, 0, 512), (7, 64, 64, 64, 576)])
def test_projection_from_the_bf16_compute_copy(B, D, K, NA, H):
    """bf16 storage with a bf16 COMPUTE COPY of the projection weight ("master fp32 + bf16 compute copy"; BASELINE
    configs[4]; frame_level_models.py:2309-2319): forward and input gradient read ops.ComputeCopy's buffer -- y = bf16(x1 * scale | x2) .
    bf16(W), dx = bf16(dy) . bf16(W)^T with fp32 accumulation, held to the fp64 product of the SAME rounded operands (1e-5: only the
    accumulation differs) and to the exact product at the bf16 tolerance; the weight gradient keeps its own path (exact operands).
    H = 576 is not a multiple of 64... of 512: the projection stream does not take it and nothing changes."""
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    g = torch.Generator().manual_seed(B + H)
    raw = (torch.randn(B, D * K, generator=g) * 3).to(dev).to(torch.bfloat16)
    scale = (torch.rand(B, K, generator=g) + 0.5).to(dev) / (D * K) ** 0.5
    x2 = (torch.randn(B, NA, generator=g) / NA ** 0.5).to(dev).requires_grad_(True) if NA else None
    Kd = D * K + NA
    W = (torch.randn(Kd, H, generator=g) / Kd ** 0.5).to(dev).requires_grad_(True)
    dy = torch.randn(B, H, generator=g).to(dev)
    handle = torch.full((B, D * K), float("nan"), device=dev).requires_grad_(True)
    handle._lpm_row_scale, handle._lpm_scale_ks, handle._lpm_raw = scale, K, raw
    if not ops.projection_parts_ok(raw, scale, K, x2, W):
        assert H % 512 != 0
        return
    cc = ops.ComputeCopy(W)
    W._lpm_w16 = cc
    y = ops.projection_parts(handle, x2, W)
    y.backward(dy)
    assert cc.refreshes == 1 and torch.equal(cc.buf, W.detach().to(torch.bfloat16))
    bf = lambda t: t.to(torch.bfloat16).double().cpu()
    xm = (raw.float().view(B, D, K) * scale.unsqueeze(1)).reshape(B, D * K)          # fp32, as the loader forms it
    xr = torch.cat([bf(xm), bf(x2.detach())], 1) if NA else bf(xm)
    xe = torch.cat([xm.double().cpu(), x2.detach().double().cpu()], 1) if NA else xm.double().cpu()
    Wr, We = bf(W.detach()), W.detach().double().cpu()
    assert_close(y, xr @ Wr, 1e-5, "y vs the rounded operands")
    assert_close(y, xe @ We, 1e-2, "y vs exact")
    dxr = bf(dy) @ Wr.t()
    assert_close(handle.grad, dxr[:, :D * K], 1e-5, "dx1 vs the rounded operands")
    assert_close(handle.grad, (dy.double().cpu() @ We.t())[:, :D * K], 1e-2, "dx1 vs exact")
    if NA:
        assert_close(x2.grad, dxr[:, D * K:], 1e-5, "dx2 vs the rounded operands")
    assert_close(W.grad, xe.t() @ dy.double().cpu(), 2e-5, "dW (exact operands, its own path)")
    # a write to the master through torch makes the copy stale: rebuilt at the next use, never read
    with torch.no_grad():
        W.mul_(0.5)
    y2 = ops.projection_parts(handle, x2, W)
    assert cc.refreshes == 2
    assert_close(y2, 0.5 * (xr @ Wr), 1e-5, "y after a write to the master")
    del W._lpm_w16


def test_factored_update_keeps_the_bf16_compute_copy():
    """lpm_factored_clip_adam_copy: the update pass of the factored gradient (utils.py:170-189 per-variable clip, TF-Adam) writes bf16(new
    weight) beside the fp32 master from its epilogue -- master and moments bit-identical to the pass without a copy, the copy exactly
    the rounded master, on both norm routes (quadratic forms over the tiles / the GEMM pass)."""
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    R, N1, N2 = 128, 4096 + 96, 1024
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(R, N1, generator=g) / N1 ** 0.5).to(dev)
    dy = torch.randn(R, N2, generator=g).to(dev)
    p0 = (torch.randn(N1 * N2, generator=g) / 30).to(dev)
    m0, v0 = (torch.randn(N1 * N2, generator=g) * 1e-3).to(dev), (torch.rand(N1 * N2, generator=g) * 1e-5).to(dev)
    for quad in (True, False):
        res = []
        for copy in (False, True):
            fg = ops.FactoredGradient()
            fg.put(x, dy)
            if not quad:
                fg.x = fg.dy = None
            p, m, v = p0.clone(), m0.clone(), v0.clone()
            c16 = torch.full((N1, N2), float("nan"), dtype=torch.bfloat16, device=dev) if copy else None
            fg.clip_adam(p, m, v, 1.0, 2e-4, 3, param_bf16=c16)
            res.append((p, m, v, c16))
        (p_a, m_a, v_a, _), (p_b, m_b, v_b, c16) = res
        # (without a copy this shape takes the tile-GEMM form as well: N2 x steps is beyond the whole-row form)
        assert torch.equal(p_a, p_b) and torch.equal(m_a, m_b) and torch.equal(v_a, v_b), f"quad={quad}: the copy changed the update"
        assert torch.equal(c16.reshape(-1), p_b.to(torch.bfloat16)), f"quad={quad}: the copy is not the rounded master"
        assert not torch.equal(p_b, p0)


@pytest.mark.parametrize("R,N1,N2", [(128, 4096 + 64, 1024), (80, 512, 256), (32, 192, 128), (16, 64, 384)])
def test_factored_update_returns_the_projection_input_gradient(R, N1, N2, monkeypatch):
    """lpm_factored_clip_adam_copy_dx (round 6): the update pass of the variable with a bf16 compute copy also returns the projection's
    input gradient dx = DY W_old^T (frame_level_models.py:2314-2319, backward) from the weights it streams.  The update is
    lpm_factored_clip_adam_copy's bit for bit (master, moments, copy); dx is the product of the two operands rounded once to bf16 --
    lpm_proj_dx_w16's arithmetic -- to fp32 summation order, and within 2e-3 of the fp64 product of the unrounded operands."""
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    g = torch.Generator().manual_seed(R + N2)
    x = (torch.randn(R, N1, generator=g) / N1 ** 0.5).to(dev)
    dy = torch.randn(R, N2, generator=g).to(dev)
    p0 = (torch.randn(N1 * N2, generator=g) / 30).to(dev)
    m0, v0 = (torch.randn(N1 * N2, generator=g) * 1e-3).to(dev), (torch.rand(N1 * N2, generator=g) * 1e-5).to(dev)
    res = []
    for fold in (False, True):
        fg = ops.FactoredGradient()
        fg.put(x, dy)
        assert fg.fold_supported()
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        c16 = p0.view(N1, N2).to(torch.bfloat16).contiguous()
        dx = torch.full((R, N1), float("nan"), device=dev) if fold else None
        fg.clip_adam(p, m, v, 1.0, 2e-4, 3, param_bf16=c16, dx=dx)
        res.append((p, m, v, c16, dx))
    (p_a, m_a, v_a, c_a, _), (p_b, m_b, v_b, c_b, dx) = res
    assert torch.equal(p_a, p_b) and torch.equal(m_a, m_b) and torch.equal(v_a, v_b) and torch.equal(c_a, c_b), "the fold changed the update"
    assert not torch.equal(p_b, p0)
    w16 = p0.view(N1, N2).to(torch.bfloat16).double()
    want = dy.to(torch.bfloat16).double() @ w16.t()
    assert float((dx.double() - want).norm() / want.norm()) < 2e-6
    exact = dy.double() @ p0.view(N1, N2).double().t()
    assert float((dx.double() - exact).norm() / exact.norm()) < 4e-3
    # the row-block form WITHOUT the input gradient (LPM_FA_FOLD=2 selects it for the A/B of the two streaming patterns) is the same update too
    lib = ops._capi.load()
    assert lib._lpm_factored_fold_supported(R, N1, N2) == 1 and lib._lpm_factored_fold_supported(R, N1 + 32, N2) == 0


@pytest.mark.parametrize("B,T,D,K", [(3, 70, 256, 128), (3, 70, 256, 256), (2, 300, 1024, 256)])
def test_vlad_aggregate_lazy_matches_the_finalize_form(B, T, D, K):
    """NetVladAttenCluster's tail (video_pooling_modules.py:1641-1658) as the lazily normalised d-major descriptor: the un-normalised sums
    x the row scales ARE the finalize form's descriptor, and the gradients of both forms agree (K3 is the same code).  K = 256 takes the
    clip-wide K2 with d-major stores (one and three column slabs per clip), K = 128 the 128 x 128 form."""
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    assert ops.vlad_aggregate_lazy_ok(T, D, K)
    g = torch.Generator().manual_seed(11)
    sims, x, C = torch.randn(B, T, K, generator=g), torch.randn(B * T, D, generator=g), torch.randn(D, K, generator=g) / D ** .5
    dout = torch.randn(B, D * K, generator=g).to(dev)
    res = []
    for lazy in (False, True):
        sg, xg, cg = (t.to(dev).requires_grad_(True) for t in (sims, x, C))
        out = ops.vlad_aggregate(sg, xg, cg, T, lazy=lazy)
        if lazy:
            assert ops.row_scale_of(out) is not None and out._lpm_scale_ks == K
            out = ops.materialise(out)
        out.backward(dout)
        res.append((out.detach(), sg.grad, xg.grad, cg.grad))
    # (K = 256: two different K2 kernels -- another summation order of the un-normalised sums, which the normalisations' Jacobian amplifies in
    # the gradients exactly as between the k-major forms; K = 128: the same kernel both times)
    for a, b, what in zip(res[1], res[0], ("descriptor", "dsims", "dx", "dcentres")):
        assert_close(a, b, 2e-6 if K != 256 else (5e-6 if what == "descriptor" else 2e-3), what)
    sd, xd, Cd = (t.double().requires_grad_(True) for t in (sims, x, C))
    ref = O.vlad_aggregate(sd, xd.reshape(B, T, D), Cd)
    assert_close(res[1][0], ref, 1e-4, "descriptor vs the oracle")


def test_fused_qkv_projection_through_attention():
    """q, k, v projections as one split-bf16 GEMM (transformer_utils.py:559-561) feeding the attention kernel through
    column views, and the backward consuming dq|dk|dv from one buffer: against fp64 autograd of the unfused maths."""
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    B, L, F, h = 5, 256, 128, 8
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B * L, F, generator=g)
    Ws = [torch.randn(F, F, generator=g) / F ** 0.5 for _ in range(3)]
    do = torch.randn(B, L, F, generator=g)
    xg = x.to(dev).requires_grad_(True)
    Wg = [w.to(dev).requires_grad_(True) for w in Ws]
    q, k, v = ops.qkv_x3(xg, *Wg)
    assert q.data_ptr() + 4 * F == k.data_ptr(), "q, k, v must be column views of one buffer"
    o = ops.mha_core(q.view(B, L, F), k.view(B, L, F), v.view(B, L, F), h, (F // h) ** -0.5)
    o.backward(do.to(dev))
    x64 = x.double().requires_grad_(True)
    W64 = [w.double().requires_grad_(True) for w in Ws]
    q64, k64, v64 = ((x64 @ w).view(B, L, h, F // h).transpose(1, 2) for w in W64)
    p = torch.softmax(q64 @ k64.transpose(-1, -2) * (F // h) ** -0.5, dim=-1)
    o64 = (p @ v64).transpose(1, 2).reshape(B, L, F)
    o64.backward(do.double())
    assert_close(o, o64, 1e-4, "attention output")
    assert_close(xg.grad, x64.grad, 1e-4, "dx")
    for name, a, b in zip("qkv", Wg, W64):
        assert_close(a.grad, b.grad, 1e-4, f"dW{name}")


@pytest.mark.parametrize("shape", [(3, 30, 1152), (80, 7, 1024), (2, 5, 128), (1, 1, 2048)])
def test_l2_normalize_rows(shape):
    """tf.nn.l2_normalize(model_input_raw, 2) (train.py:262-264), including all-zero (padded) frames (eps clamp)."""
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    g = torch.Generator().manual_seed(shape[1])
    x = torch.randn(*shape, generator=g) * 3
    x[0, 0] = 0.0
    y = ops.l2_normalize_rows(x.to(dev))
    assert_close(y, O.l2_normalize(x.double(), 2), 1e-6, "l2_normalize")
    assert float(y[0, 0].abs().max()) == 0.0


@pytest.mark.parametrize("B,MF,F", [(3, 30, 1152), (5, 300, 1152), (2, 7, 128)])
def test_dequantize_l2_normalize(B, MF, F):
    """Reader tail + input normalisation in one pass (readers.py:176-193, utils.py:28-43, train.py:262-264): quantised uint8
    frames -> Dequantize -> exact zeros past num_frames -> per-frame L2 normalisation."""
    from learnablepoolingmethods_amd import ops, utils
    dev = cuda()
    g = torch.Generator().manual_seed(MF)
    q = torch.randint(0, 256, (B, MF, F), generator=g, dtype=torch.uint8)
    nf = torch.randint(1, MF + 1, (B,), generator=g, dtype=torch.int32)
    nf[0] = MF
    y = ops.dequantize_l2_normalize(q.to(dev), nf.to(dev))
    t = torch.arange(MF).view(1, -1, 1)
    x = torch.where(t < nf.view(-1, 1, 1), utils.Dequantize(q.double()), torch.zeros((), dtype=torch.float64))
    assert_close(y, O.l2_normalize(x, 2), 1e-6, "dequantize + l2_normalize")
    for b in range(B):
        assert float(y[b, int(nf[b]):].abs().max() if int(nf[b]) < MF else 0.0) == 0.0


@pytest.mark.parametrize("B,V,m", [(80, 3862, 2), (5, 40, 4), (3, 17, 1)])
def test_moe_cross_entropy_fused(B, V, m):
    """MoeModel mixture tail + CrossEntropyLoss as one kernel pair (video_level_models.py:116-126, losses.py:41-51)."""
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    g = torch.Generator().manual_seed(V + m)
    ga, ea = 2 * torch.randn(B, V * (m + 1), generator=g), 2 * torch.randn(B, V * m, generator=g)
    y = (torch.rand(B, V, generator=g) < 0.05).float()
    dpred = 0.01 * torch.randn(B, V, generator=g)
    gad, ead = ga.double().requires_grad_(True), ea.double().requires_grad_(True)
    gating = torch.softmax(gad.reshape(-1, m + 1), dim=-1)
    pr = (gating[:, :m] * torch.sigmoid(ead.reshape(-1, m))).sum(1).reshape(B, V)
    ls = O.cross_entropy_loss(pr, y.double())
    (1.7 * ls + (pr * dpred.double()).sum()).backward()
    gag, eag = ga.to(dev).requires_grad_(True), ea.to(dev).requires_grad_(True)
    p, l = ops.moe_cross_entropy(gag, eag, y.to(dev), m)
    assert_close(p, pr, 1e-5, "predictions")
    assert_close(l, ls, 1e-5, "loss")
    (1.7 * l + (p * dpred.to(dev)).sum()).backward()
    assert_close(gag.grad, gad.grad, 1e-4, "d gate activations")
    assert_close(eag.grad, ead.grad, 1e-4, "d expert activations")
    p2, none = ops.moe_cross_entropy(ga.to(dev), ea.to(dev), None, m)
    assert none is None
    assert_close(p2, pr, 1e-5, "predictions without labels")


@pytest.mark.parametrize("B,L,C", [(4, 300, 1024), (3, 17, 256), (2, 5, 4096)])
def test_batch_norm_rows_rank3(B, L, C):
    """slim.batch_norm on a [B, L, C] tensor (transformer_utils.py:666,747,760): batch statistics over B*L rows, the BIASED
    variance into the moving average (TF's non-fused path), backward through the statistics."""
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    g = torch.Generator().manual_seed(C + L)
    x, dy = 2 * torch.randn(B, L, C, generator=g) + 0.5, torch.randn(B, L, C, generator=g)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    mm, mv = 0.1 * torch.randn(C, generator=g), 1 + 0.3 * torch.rand(C, generator=g)
    p = {"bn/gamma": gamma.double().requires_grad_(True), "bn/beta": beta.double().requires_grad_(True),
         "bn/moving_mean": mm.double(), "bn/moving_variance": mv.double()}
    xd = x.double().requires_grad_(True)
    upd = {}
    ref = O.batch_norm(xd, p, "bn", True, upd)
    ref.backward(dy.double())
    xg, gg, bg = (t.to(dev).requires_grad_(True) for t in (x, gamma, beta))
    mmg, mvg = mm.to(dev), mv.to(dev)
    y = ops.batch_norm_rows(xg, gg, bg, mmg, mvg, biased_moving_variance=True)
    assert_close(y, ref, 1e-5, "batch_norm fwd")
    y.backward(dy.to(dev))
    assert_close(xg.grad, xd.grad, 1e-4, "dx")
    assert_close(gg.grad, p["bn/gamma"].grad, 1e-4, "dgamma")
    assert_close(bg.grad, p["bn/beta"].grad, 1e-4, "dbeta")
    assert_close(mmg, mm.double() * 0.999 + upd["bn/moving_mean"] * 0.001, tol=1e-6, what="moving_mean")
    assert_close(mvg, mv.double() * 0.999 + upd["bn/moving_variance"] * 0.001, tol=1e-6, what="moving_variance")


@pytest.mark.parametrize("B,L,C,relu", [(4, 300, 4096, True), (3, 300, 256, True), (5, 64, 1024, False), (2, 300, 128, True)])
def test_batch_norm_rows_with_the_dense_bias_and_relu_inside(B, L, C, relu):
    """ops.batch_norm_rows_act: slim.batch_norm(act(x + bias)) with x the raw dense output (transformer_utils.py:741-760) -- bias add
    and ReLU inside the statistics / apply passes and both backward passes -- against the composed fp64 formula: output, the gradient
    of x (ReLU mask), of the bias, of gamma / beta, and the moving statistics."""
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    g = torch.Generator().manual_seed(C + L + relu)
    x, dy = 2 * torch.randn(B, L, C, generator=g), torch.randn(B, L, C, generator=g)
    bias = 0.5 * torch.randn(C, generator=g)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    mm, mv = 0.1 * torch.randn(C, generator=g), 1 + 0.3 * torch.rand(C, generator=g)
    p = {"bn/gamma": gamma.double().requires_grad_(True), "bn/beta": beta.double().requires_grad_(True),
         "bn/moving_mean": mm.double(), "bn/moving_variance": mv.double()}
    xd, bd = x.double().requires_grad_(True), bias.double().requires_grad_(True)
    upd = {}
    a = xd + bd
    a = torch.relu(a) if relu else a
    ref = O.batch_norm(a, p, "bn", True, upd)
    ref.backward(dy.double())
    xg, bbg, gg, bg = (t.to(dev).requires_grad_(True) for t in (x, bias, gamma, beta))
    mmg, mvg = mm.to(dev), mv.to(dev)
    assert ops.batch_norm_rows_act_ok(xg, bbg)
    y = ops.batch_norm_rows_act(xg, bbg, relu, gg, bg, mmg, mvg, biased_moving_variance=True)
    assert_close(y, ref, 1e-5, "batch_norm(act) fwd")
    y.backward(dy.to(dev))
    assert_close(xg.grad, xd.grad, 1e-4, "dx")
    # (without the ReLU a batch norm removes any per-column constant: the bias gradient is exactly zero, ours is rounding noise --
    # measured against the scale of the gradients that are not)
    assert_close(bbg.grad, bd.grad, 1e-4, "dbias", floor=float(p["bn/beta"].grad.abs().max()))
    assert_close(gg.grad, p["bn/gamma"].grad, 1e-4, "dgamma")
    assert_close(bg.grad, p["bn/beta"].grad, 1e-4, "dbeta")
    assert_close(mmg, mm.double() * 0.999 + upd["bn/moving_mean"] * 0.001, tol=1e-6, what="moving_mean")
    assert_close(mvg, mv.double() * 0.999 + upd["bn/moving_variance"] * 0.001, tol=1e-6, what="moving_variance")


def test_netvlad_batch_split_invariance_full_size():
    """Size-independent property at BASELINE cfg-2 shapes, forward AND backward: with inference-mode batch norm (a fixed
    affine) clips are independent, so pooling the 80-clip batch equals pooling its two halves -- descriptors and input
    gradients clip by clip, weight gradients as the sum of the halves'."""
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    B, T, D, K = 80, 300, 1024, 256
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(B * T, 1152, device=dev, generator=g)
    W = (torch.randn(D, K, device=dev, generator=g) / 32).requires_grad_(True)
    W2 = (torch.randn(1, D, K, device=dev, generator=g) / 32).requires_grad_(True)
    bn = (1 + 0.1 * torch.randn(K, device=dev, generator=g), 0.1 * torch.randn(K, device=dev, generator=g),
          0.1 * torch.randn(K, device=dev, generator=g), 1 + 0.2 * torch.rand(K, device=dev, generator=g))
    R = torch.randn(B, D * K, device=dev, generator=g)

    def run(rows, r):
        xi = x[rows, :D].detach().requires_grad_(True)
        out = ops.netvlad(xi, W, W2, T, bn=bn, is_training=False)
        gx, gW, gW2 = torch.autograd.grad((out * r).sum(), [xi, W, W2])
        return out.detach(), gx, gW, gW2
    full = run(slice(0, B * T), R)
    h = B // 2
    a, b = run(slice(0, h * T), R[:h]), run(slice(h * T, B * T), R[h:])
    assert rel_err(torch.cat([a[0], b[0]]), full[0]) < 1e-6
    assert rel_err(torch.cat([a[1], b[1]]), full[1]) < 1e-5
    assert rel_err(a[2] + b[2], full[2]) < 1e-4 and rel_err(a[3] + b[3], full[3]) < 1e-4


def test_attention_properties_full_size(mha_precision):
    """Size-independent properties of the attention core at the cfg-2 video-encoder shape (B=80, L=256, h=64, d=16):
    invariance to a joint permutation of keys and values; softmax rows sum to one (constant values come back unchanged) and,
    with constant values, no gradient reaches the queries or keys."""
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    B, L, h, d = 80, 256, 64, 16
    g = torch.Generator(device=dev).manual_seed(2)
    q, k, v, do = (torch.randn(B, L, h * d, device=dev, generator=g) for _ in range(4))
    o = ops.mha_core(q, k, v, h, d ** -0.5)
    perm = torch.randperm(L, device=dev, generator=g)
    assert rel_err(ops.mha_core(q, k[:, perm], v[:, perm], h, d ** -0.5), o) < 2e-5
    qg, kg = q.clone().requires_grad_(True), k.clone().requires_grad_(True)
    ones = torch.full_like(v, 0.75)
    oc = ops.mha_core(qg, kg, ones, h, d ** -0.5)
    assert float((oc - 0.75).abs().max()) < 2e-5
    oc.backward(do)
    scale = float(do.abs().max())
    assert float(qg.grad.abs().max()) < 1e-4 * scale and float(kg.grad.abs().max()) < 1e-4 * scale


_K1_FORM_SCRIPT = r"""
import sys, torch
from learnablepoolingmethods_amd import _capi
from learnablepoolingmethods_amd._capi import ptr, stream_ptr
lib = _capi.load()
dev = torch.device("cuda:0")
B, T, D, K = 8, 300, 512, 256
g = torch.Generator().manual_seed(5)
x = torch.randn(B * T, D, generator=g).to(dev)
W = (torch.randn(D, K, generator=g) / D ** 0.5).to(dev)
buf = lambda n: torch.empty(n // 4, dtype=torch.int32, device=dev)
xr, wt = buf(lib._lpm_row_tiles_bytes(B, T, D)), buf(lib._lpm_weight_tiles_bytes(D, K))
logits = torch.zeros(B * T, K, device=dev)
partial = torch.zeros(lib._lpm_assign_gemm_tiles_nblk(B, T), 2, K, device=dev)
st = stream_ptr()
lib.check(lib._lpm_split_rows_tiles(ptr(x), D, B, T, D, ptr(xr), st), "split")
lib.check(lib._lpm_split_weight_tiles(ptr(W), D, K, 0, ptr(wt), st), "split")
lib.check(lib._lpm_assign_gemm_tiles_fwd(ptr(xr), ptr(wt), B, T, D, K, ptr(logits), ptr(partial), st), "k1")
torch.cuda.synchronize()
torch.save({"logits": logits.cpu(), "partial": partial.cpu()}, sys.argv[1])
"""


@pytest.mark.gpu
def test_assign_gemm_row_forms_bit_identical(tmp_path):
    """K1's 128-row workgroup form (default at K = 256 when the tile count divides by four) and its 64-row form
    (LPM_TILE_GEMM_WIDE=0, read once per process: hence two child processes) accumulate every output in the same order:
    logits and the per-64-row statistics rows must agree bit for bit."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for wide in ("1", "0"):
        out = tmp_path / f"k1_{wide}.pt"
        env = dict(os.environ, LPM_TILE_GEMM_WIDE=wide, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
        r = subprocess.run([sys.executable, "-c", _K1_FORM_SCRIPT, str(out)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(torch.load(out))
    assert torch.equal(outs[0]["logits"], outs[1]["logits"])
    assert torch.equal(outs[0]["partial"], outs[1]["partial"])
    assert float(outs[0]["logits"].abs().max()) > 0


_MEASURE_SCRIPT = r"""
import sys, torch
from learnablepoolingmethods_amd import _capi
from learnablepoolingmethods_amd._capi import ptr, stream_ptr
lib = _capi.load()
dev = torch.device("cuda:0")
st = stream_ptr()
ints = lambda nbytes: torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
g = torch.Generator().manual_seed(17)
# K2 for bf16 storage on clip-wide items (vlad_clip16.hip): the smallest shape with lpm_vlad_clip16_slabs > 0
B, T, D, K = 2, 64, 384, 256
P = lib._lpm_vlad_clip16_slabs(D, K)
assert P > 0
x = torch.randn(B * T, D, generator=g).to(dev)
a = torch.rand(B * T, K, generator=g).to(torch.bfloat16).to(dev)
cen = (torch.randn(D, K, generator=g) / D ** 0.5).to(dev)
xt = ints(lib._lpm_frame_tiles_bf16_bytes(B, T, D))
lib.check(lib._lpm_split_frames_bf16(ptr(x), D, B, T, D, ptr(xt), st), "lpm_split_frames_bf16")
at = ints(B * (K // 32) * lib._lpm_frame_steps_bf16(T) * 1024)
lib.check(lib._lpm_assign_tiles_bf16(ptr(a), None, None, B, T, K, 0, ptr(at), st), "lpm_assign_tiles_bf16")
nrm = torch.zeros((B, D, K), dtype=torch.bfloat16, device=dev)
asum, part = torch.zeros((B, K), device=dev), torch.zeros((B, P, K), device=dev)
lib.check(lib._lpm_vlad_aggregate_clip_fwd_bf16(ptr(at), ptr(xt), ptr(cen), B, T, D, K, _capi.LPM_VLAD_RESIDUAL, ptr(nrm), ptr(asum), ptr(part),
                                                st), "lpm_vlad_aggregate_clip_fwd_bf16")
# one 128-row tile GEMM store (tile_gemm.hip): four row tiles, 16 reduction steps, one 256-column block
M, Kd, N = 128, 256, 256
xd = torch.randn(M, Kd, generator=g).to(dev)
W = (torch.randn(Kd, N, generator=g) / Kd ** 0.5).to(dev)
xr, wt = ints(lib._lpm_row_tiles_bytes(1, M, Kd)), ints(lib._lpm_weight_tiles_bytes(Kd, N))
lib.check(lib._lpm_split_rows_tiles(ptr(xd), Kd, 1, M, Kd, ptr(xr), st), "lpm_split_rows_tiles")
lib.check(lib._lpm_split_weight_tiles(ptr(W), Kd, N, 0, ptr(wt), st), "lpm_split_weight_tiles")
y = torch.zeros(M, N, device=dev)
lib.check(lib._lpm_dense_tiles_fwd(ptr(xr), ptr(wt), M, Kd, N, ptr(y), N, 2, st), "lpm_dense_tiles_fwd")
torch.cuda.synchronize()
torch.save({"measure_build": lib._lpm_measure_build(), "nrm": nrm.cpu(), "asum": asum.cpu(), "part": part.cpu(), "y": y.cpu(),
            "y_ref": (xd.double() @ W.double()).cpu()}, sys.argv[1])
"""


@pytest.mark.gpu
def test_measurement_variables_are_ignored_by_the_default_build(tmp_path):
    """The measurement instantiations (kernels that skip their main loop, their stores, their MFMAs: garbage by design) and the reads of the
    variables that select them exist only in -DLPM_MEASURE builds (docs/switches.md).  The bf16 clip-wide K2 and a 128-row tile GEMM store,
    once in a clean environment and once with LPM_VB_DBG=1 (no main loop) LPM_TG_DBG=2 (no stores) LPM_VC_DBG=1 LPM_FA_FOLD_DBG=16 set
    (read once per process: hence two child processes): the default build writes the same bits, and they are the right ones."""
    import os, subprocess, sys
    from learnablepoolingmethods_amd import _capi
    if _capi.load()._lpm_measure_build():
        pytest.skip("a measurement build honours these variables")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = ("LPM_VB_DBG", "LPM_VB_DELAY", "LPM_TG_DBG", "LPM_VC_DBG", "LPM_VK_DBG", "LPM_FA_DBG", "LPM_FA_FOLD_DBG", "LPM_K1_WIDE_DBG")
    clean = {k: v for k, v in os.environ.items() if k not in names}
    clean["PYTHONPATH"] = root + os.pathsep + os.environ.get("PYTHONPATH", "")
    outs = []
    for extra in ({}, {"LPM_VB_DBG": "1", "LPM_TG_DBG": "2", "LPM_VC_DBG": "1", "LPM_FA_FOLD_DBG": "16"}):
        out = tmp_path / f"measure_{len(outs)}.pt"
        r = subprocess.run([sys.executable, "-c", _MEASURE_SCRIPT, str(out)], env=dict(clean, **extra), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]                 # (a failed first child ends the test: the second never starts)
        assert "measurement mode" not in r.stderr, r.stderr[-2000:]
        outs.append(torch.load(out))
    assert outs[0]["measure_build"] == 0 and outs[1]["measure_build"] == 0
    for k in ("nrm", "asum", "part", "y"):
        assert torch.equal(outs[0][k], outs[1][k]), k
    assert float(outs[0]["nrm"].float().abs().max()) > 0 and float(outs[0]["asum"].abs().max()) > 0
    assert_close(outs[0]["y"], outs[0]["y_ref"], tol=2e-5, what="128-row tile GEMM store")


@pytest.mark.gpu
@pytest.mark.parametrize("kmajor", [False, True])
def test_netvlad_raw_nrm_matches_normalised_nrm(kmajor, monkeypatch):
    """LPM_VLAD_NRM_RAW (the finalize pass leaves nrm un-normalised, K3's tile form rebuilds U * rsqrt(max(colsq, eps)) where it
    reads it) against the path that stores the intra-normalised copy: same descriptor bit for bit, gradients to rounding of
    the one product that is formed in a different place.  frame_level_models.py:2803-2824 and TF autodiff of it."""
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    if ops.VLAD_PRECISION != "bf16x3":
        pytest.skip("the raw form belongs to the bf16x3 tile path")
    B, T, D, K = 3, 77, 256, 128
    g = torch.Generator().manual_seed(11)
    x0 = torch.randn(B * T, D, generator=g).to(dev)
    W0 = (torch.randn(D, K, generator=g) / D ** 0.5).to(dev)
    W20 = (torch.randn(1, D, K, generator=g) / D ** 0.5).to(dev)
    dout = torch.randn(B, K, D, generator=g).to(dev) if kmajor else torch.randn(B, D * K, generator=g).to(dev)
    res = []
    for raw in (True, False):
        if not raw:
            monkeypatch.setattr(ops, "_nrm_raw_ok", lambda lib, T, D, K: False)
        else:
            assert ops._nrm_raw_ok(__import__("learnablepoolingmethods_amd")._capi.load(), T, D, K)
        x, W, W2 = (t.clone().requires_grad_(True) for t in (x0, W0, W20))
        gam, bet = torch.ones(K, device=dev, requires_grad=True), torch.zeros(K, device=dev, requires_grad=True)
        out = ops.netvlad(x, W, W2, T, bn=(gam, bet, torch.zeros(K, device=dev), torch.ones(K, device=dev)), kmajor=kmajor)
        out.backward(dout)
        res.append((out.detach(), x.grad, W.grad, W2.grad, gam.grad, bet.grad))
    assert torch.equal(res[0][0], res[1][0])
    for a, b, what in zip(res[0][1:], res[1][1:], ("dx", "dW", "dW2", "dgamma", "dbeta")):
        assert_close(a, b.double().cpu(), 1e-5, what)


@pytest.mark.gpu
def test_raw_nrm_flag_is_rejected_by_the_fp32_backward():
    from learnablepoolingmethods_amd import _capi
    from learnablepoolingmethods_amd._capi import ptr, stream_ptr
    lib = _capi.load()
    dev = cuda()
    B, T, D, K = 1, 16, 128, 32
    z = lambda *s: torch.zeros(*s, device=dev)
    wsb = lib._lpm_vlad_bwd_workspace_bytes(B, D, K)
    ws = torch.empty(max(wsb, 16) // 4, dtype=torch.int32, device=dev)
    rc = lib._lpm_vlad_aggregate_bwd(ptr(z(B, D * K)), ptr(z(B, D, K)), ptr(z(B, K)), ptr(z(B, K)), ptr(z(B, K)), ptr(z(B)),
                                     ptr(z(B * T, K)), None, None, ptr(z(B * T, D)), D, None, B, T, D, K, _capi.LPM_VLAD_NRM_RAW,
                                     ptr(z(B * T, K)), ptr(z(B * T, D)), D, 0, None, ptr(ws), ws.numel() * 4, stream_ptr())
    assert rc != 0
    with pytest.raises(_capi.LpmError, match="NRM_RAW"):
        lib.check(rc, "lpm_vlad_aggregate_bwd")


# ---- bf16 storage (BASELINE configs[4]) ------------------------------------------------------------------------------------------
BF16_FWD_TOL = 2e-2     # vs the exact fp64 oracle, max-norm relative: x, W, logits, assignment and descriptor are each rounded to bf16
BF16_GRAD_TOL = 4e-2    # (2^-9 relative per element); measured: forward 8e-3, gradients 2e-3 ... 2.5e-2 (printed by the test)


def _bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _ste(t):
    """Round to bf16 in the forward, identity in the backward (what storing a tensor as bf16 between two fp32 computations does)."""
    return t + (_bf(t) - t).detach()


def _oracle_netvlad_bf16(x, W, gamma, beta, W2, T, dout):
    """The oracle's NetVLAD (frame_level_models.py:2773-2824) with a bf16 rounding at every point where the bf16-storage path keeps a
    tensor in HBM as bf16: frames, cluster weights (operand tiles), logits, assignment (operand tiles), descriptor."""
    p = {"W": W.double().requires_grad_(True), "gamma": gamma.double().requires_grad_(True), "beta": beta.double().requires_grad_(True),
         "W2": W2.double().requires_grad_(True)}
    xr = _bf(x.double())
    logits = xr @ _ste(p["W"])
    mean, var = logits.mean(0), logits.var(0, unbiased=False)          # statistics come from the fp32 accumulators
    lr = _ste(logits)
    a = torch.softmax((lr - mean) * torch.rsqrt(var + O.BN_EPS) * p["gamma"] + p["beta"], dim=-1)
    a = _ste(a).reshape(-1, T, a.shape[-1])
    out = _ste(O.vlad_aggregate(a, xr.reshape(-1, T, xr.shape[-1]), p["W2"]))
    out.backward(_bf(dout.double()))
    return out.detach(), p


def test_netvlad_bf16_storage():
    """ops.netvlad(storage='bf16') on both streams of a 1152-wide input at the cfg-5 layer sizes (video 1024 x 512, audio 128 x 128):
    forward and the gradients of every variable against (i) the oracle with bf16 roundings at the same storage points -- what the path
    is supposed to compute, tight -- and (ii) the exact fp64 oracle under the documented bf16 tolerance."""
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    B, T = 4, 300
    g = torch.Generator().manual_seed(12)
    raw = torch.randn(B, T, 1152, generator=g)
    nf = torch.full((B,), T, dtype=torch.int32)                 # T of T frames: the uniform sampler is the identity
    y = ops.frame_sample_bn(raw.to(dev), nf.to(dev), T, storage="bf16", materialize=False)
    res = {}
    for name, off, D, K in (("video", 0, 1024, 512), ("audio", 1024, 128, 128)):
        gg = torch.Generator().manual_seed(K)
        W = torch.randn(D, K, generator=gg) / D ** 0.5
        gamma, beta = 1 + 0.3 * torch.randn(K, generator=gg), 0.2 * torch.randn(K, generator=gg)
        W2 = torch.randn(1, D, K, generator=gg) / D ** 0.5
        dout = torch.randn(B, D * K, generator=gg)
        x = raw.reshape(B * T, 1152)[:, off:off + D]
        ref_b, pb = _oracle_netvlad_bf16(x, W, gamma, beta, W2, T, dout)
        ref, _, pe, _ = _oracle_netvlad(x, W, gamma, beta, W2, T, dout)
        Wg, gmg, btg, W2g = (t.to(dev).requires_grad_(True) for t in (W, gamma, beta, W2))
        with torch.no_grad():
            xs = y[:, off:off + D]
        out = ops.netvlad(xs, Wg, W2g, T, bn=(gmg, btg, torch.zeros(K, device=dev), torch.ones(K, device=dev)), is_training=True,
                          storage="bf16")
        assert out.dtype == torch.bfloat16 and out.shape == (B, D * K)
        out.backward(dout.to(dev).to(torch.bfloat16))
        e = {"fwd vs bf16 oracle": rel_err(out.float(), ref_b), "fwd vs exact": rel_err(out.float(), ref)}
        for nm, got, kb, ke in (("dW", Wg.grad, "W", "s/cluster_weights"), ("dgamma", gmg.grad, "gamma", "s/cluster_bn/gamma"),
                                ("dbeta", btg.grad, "beta", "s/cluster_bn/beta"), ("dW2", W2g.grad, "W2", "s/cluster_weights2")):
            e[nm + " vs bf16 oracle"] = rel_l2(got, pb[kb].grad)
            e[nm + " vs exact"] = rel_l2(got, pe[ke].grad)
        res[name] = e
        print(f"[bf16 storage {name} D={D} K={K}] " + ", ".join(f"{k}: {v:.1e}" for k, v in e.items()))
        # two bf16 ulps (2^-8 each) of the largest element: the stored descriptor is rounded once here and once in the emulation, from
        # values that differ in the last fp32 bits
        assert e["fwd vs bf16 oracle"] <= 8e-3, f"{name}: {e['fwd vs bf16 oracle']:.2e}"
        assert e["fwd vs exact"] <= BF16_FWD_TOL
        for k, v in e.items():
            if k.startswith("d") and k.endswith("bf16 oracle"):
                assert v <= 3e-2, f"{name} {k}: {v:.2e}"           # the backward rounds dU, dl and the frames once more for its tiles
            elif k.startswith("d"):
                assert v <= BF16_GRAD_TOL, f"{name} {k}: {v:.2e}"
        o = out.float().reshape(B, D, K)                          # norm invariants at bf16 resolution
        assert torch.allclose(o.norm(dim=(1, 2)), torch.ones(B, device=dev), atol=4e-3)
    # the fp32 frames were not materialised: an op that would read them says so instead of computing on garbage
    with pytest.raises(Exception, match="bf16 operand tiles only"):
        ops.netvlad(y[:, :1024].detach(), torch.zeros(1024, 128, device=dev), None, T, bias=torch.zeros(128, device=dev))


@pytest.mark.parametrize("B,T,D,K", [(5, 33, 384, 256), (2, 130, 416, 512), (3, 64, 800, 256), (1, 300, 1024, 512)])
def test_k2_bf16_clip_wide_items_on_other_slab_shapes(B, T, D, K):
    """lpm_vlad_aggregate_clip_fwd_bf16 through the C ABI on operand tiles made here (lpm_split_frames_bf16, lpm_assign_tiles_bf16 without
    the softmax: the tiles hold the given bf16 values) against the fp64 sums of the SAME rounded operands: one slab of 12 column tiles
    (D = 384), 13 = 7 + 6 (D = 416), 25 = 9 + 8 + 8 in groups of 5 + 4 / 4 + 4 (D = 800), the benched 11 / 11 / 10.  The un-normalised
    sums to one bf16 rounding, assignment sums and square norms (over the P slabs) to 1e-5."""
    from learnablepoolingmethods_amd import _capi, ops
    lib = _capi.load()
    dev = cuda()
    P = lib._lpm_vlad_clip16_slabs(D, K)
    assert P > 0
    g = torch.Generator().manual_seed(D + T)
    x = torch.randn(B * T, D, generator=g).to(torch.bfloat16).float()
    a = torch.rand(B * T, K, generator=g).to(torch.bfloat16)
    cen = torch.randn(D, K, generator=g) / D ** 0.5
    st = ops.stream_ptr()
    xg, ag, cg_ = x.to(dev), a.to(dev), cen.to(dev)
    steps = lib._lpm_frame_steps_bf16(T)
    xt = torch.empty(lib._lpm_frame_tiles_bf16_bytes(B, T, D) // 4, dtype=torch.int32, device=dev)
    lib.check(lib._lpm_split_frames_bf16(ops.ptr(xg), D, B, T, D, ops.ptr(xt), st), "lpm_split_frames_bf16")
    at = torch.empty(B * (K // 32) * steps * 256, dtype=torch.int32, device=dev)
    lib.check(lib._lpm_assign_tiles_bf16(ops.ptr(ag), None, None, B, T, K, 0, ops.ptr(at), st), "lpm_assign_tiles_bf16")
    nrm = torch.empty((B, D, K), dtype=torch.bfloat16, device=dev)
    asum, part = torch.empty((B, K), device=dev), torch.empty((B, P, K), device=dev)
    lib.check(lib._lpm_vlad_aggregate_clip_fwd_bf16(ops.ptr(at), ops.ptr(xt), ops.ptr(cg_), B, T, D, K, _capi.LPM_VLAD_RESIDUAL, ops.ptr(nrm),
                                                    ops.ptr(asum), ops.ptr(part), st), "lpm_vlad_aggregate_clip_fwd_bf16")
    a64, x64 = a.double().reshape(B, T, K), x.double().reshape(B, T, D)
    s_ref = a64.sum(1)                                                    # [B, K]
    u_ref = torch.einsum("btk,btd->bdk", a64, x64) - s_ref[:, None, :] * cen.double()[None]
    got = nrm.float().cpu().double()
    scale = float(u_ref.abs().max())
    assert (got - u_ref).abs().le(2.0 ** -8 * u_ref.abs() + 2e-6 * scale).all(), f"sums: {float((got - u_ref).abs().max() / scale):.2e} of the largest"
    assert rel_err(asum, s_ref) <= 1e-5
    assert rel_err(part.sum(1), (u_ref ** 2).sum(1)) <= 1e-5


@pytest.mark.parametrize("B,T,D,K", [(128, 300, 1024, 512), (3, 77, 1024, 512), (2, 300, 1024, 256), (1, 1, 1024, 512)])
def test_k2_bf16_clip_wide_items_against_the_128_x_128_form(B, T, D, K):
    """Round 6: K2 for bf16 storage on clip-wide items (csrc/vlad_clip16.hip: 256 clusters x a third of a clip's
    columns per workgroup, 2 x 6 register tiles, d-major bf16 stores through a wave-private LDS tile; frame_level_models.py:2803-2822)
    against the 128 x 128 form it replaces on the same operand tiles, through the C ABI: the un-normalised bf16 sums within ONE bf16
    rounding of each other (the fp32 accumulation orders differ), assignment sums and the clusters' square norms to 1e-5, and the
    normalised descriptor of ops.netvlad(storage='bf16') against the fp64 oracle at the bf16 tolerance.  Shapes: the benched one (128 x
    300, K = 512: 768 workgroups), ragged clips, one cluster half (K = 256), a single frame."""
    from learnablepoolingmethods_amd import _capi, ops
    lib = _capi.load()
    dev = cuda()
    assert lib._lpm_vlad_clip16_slabs(D, K) > 0
    g = torch.Generator().manual_seed(B * 7 + T)
    ld = 1152
    raw = torch.randn(B, T, ld, generator=g)
    nf = torch.full((B,), T, dtype=torch.int32)
    y = ops.frame_sample_bn(raw.to(dev), nf.to(dev), T, storage="bf16", materialize=False)
    W = torch.randn(D, K, generator=g) / D ** 0.5
    gamma, beta = 1 + 0.3 * torch.randn(K, generator=g), 0.2 * torch.randn(K, generator=g)
    W2 = torch.randn(1, D, K, generator=g) / D ** 0.5
    outs = {}
    old = ops.VLAD_CLIP16
    try:
        for form in (True, False):
            ops.VLAD_CLIP16 = form
            with torch.no_grad():
                xs = y[:, :D]
            Wg, gmg, btg, W2g = (t.to(dev).requires_grad_(True) for t in (W, gamma, beta, W2))
            out = ops.netvlad(xs, Wg, W2g, T, bn=(gmg, btg, torch.zeros(K, device=dev), torch.ones(K, device=dev)), is_training=True, storage="bf16")
            ctx = out.grad_fn
            saved = {n: t for n, t in zip(("nrm", "asum", "colsq", "csq", "gsq"), ctx.saved_tensors[9:14])}
            outs[form] = (out.float().cpu(), {k: v.float().cpu() for k, v in saved.items()})
    finally:
        ops.VLAD_CLIP16 = old
    (o1, s1), (o0, s0) = outs[True], outs[False]
    scale = float(s0["nrm"].abs().max())
    d = float((s1["nrm"] - s0["nrm"]).abs().max())
    print(f"[K2 bf16 clip-wide B={B} T={T} D={D} K={K}] raw sums: max |clip-wide - 128x128| = {d / scale:.1e} of the largest; asum "
          f"{rel_err(s1['asum'], s0['asum']):.1e}, colsq {rel_err(s1['colsq'], s0['colsq']):.1e}, descriptor {rel_err(o1, o0):.1e}")
    # one bf16 rounding apart: 2^-8 of the element, and elements are at most `scale`
    assert (s1["nrm"] - s0["nrm"]).abs().le(2.0 ** -7 * s0["nrm"].abs() + 1e-6 * scale).all(), "un-normalised sums differ by more than a bf16 rounding"
    assert rel_err(s1["asum"], s0["asum"]) <= 1e-5 and rel_err(s1["colsq"], s0["colsq"]) <= 1e-5 and rel_err(s1["gsq"], s0["gsq"]) <= 1e-5
    assert rel_err(o1, o0) <= 2.0 ** -7
    # (S of S frames: the uniform sampler's fp32 index arithmetic is NOT the identity for every S -- 77 repeats frames -- so the oracle samples too)
    x = O.sample_uniform_frames(raw, nf, T).reshape(B * T, ld)[:, :D]
    ref, _, _, _ = _oracle_netvlad(x, W, gamma, beta, W2, T, torch.zeros(B, D * K))
    assert rel_err(o1, ref) <= BF16_FWD_TOL, f"descriptor against the fp64 oracle: {rel_err(o1, ref):.2e}"


@pytest.mark.parametrize("B,T", [(128, 300), (3, 77), (1, 300), (7, 129), (2, 33), (1, 1)])
def test_k1_plain_bf16_at_k512(B, T):
    """K1 on plain bf16 tiles at BASELINE configs[4]'s video sizes (1024 -> 512 clusters; frame_level_models.py:2781-2789) through the C
    ABI: 160-row x 512-column workgroups when the statistics array has a row per workgroup (B T / 160 <= B ceil(T / 64): 128 x 300 is one
    round of 240 workgroups; 7 x 129 and 3 x 77 straddle clips and end in a partial group), the flat 96-row form otherwise (1 x 300, 1 x 1).
    Logits = bf16(frames) . bf16(weights) accumulated in fp32 and stored as bf16: within one bf16 rounding of the fp64 product of the
    rounded operands; the batch-norm statistics come from the fp32 accumulators."""
    from learnablepoolingmethods_amd import _capi, ops
    from learnablepoolingmethods_amd._capi import ptr, stream_ptr
    lib = _capi.load()
    dev = cuda()
    D, K, M = 1024, 512, B * T
    g = torch.Generator().manual_seed(B * 1000 + T)
    raw = torch.randn(B, T, 1152, generator=g)
    nf = torch.full((B,), T, dtype=torch.int32)
    y = ops.frame_sample_bn(raw.to(dev), nf.to(dev), T, storage="bf16", materialize=True)
    xr = ops._cached_tiles(y[:, :D], B, T, D, rows=True, storage="bf16")
    assert xr is not None
    W = (torch.randn(D, K, generator=g) / D ** 0.5).to(dev)
    wt = torch.empty(lib._lpm_weight_tiles_bytes(D, K) // 8, dtype=torch.int32, device=dev)
    st = stream_ptr()
    lib.check(lib._lpm_split_weight_tiles_bf16(ptr(W), D, K, 0, ptr(wt), st), "lpm_split_weight_tiles_bf16")
    nblk = lib._lpm_assign_gemm_tiles_nblk(B, T)
    logits = torch.full((M, K), float("nan"), dtype=torch.bfloat16, device=dev)
    partial = torch.full((nblk, 2, K), float("nan"), device=dev)
    lib.check(lib._lpm_assign_gemm_tiles_fwd_bf16(ptr(xr), ptr(wt), B, T, D, K, ptr(logits), ptr(partial), st), "lpm_assign_gemm_tiles_fwd_bf16")
    x64 = y[:, :D].to(torch.bfloat16).double().cpu()
    ref = x64 @ W.to(torch.bfloat16).double().cpu()
    got = logits.double().cpu()
    assert torch.isfinite(got).all() and torch.isfinite(partial).all()
    err = (got - ref).abs()
    assert bool((err <= 2.0 ** -8 * ref.abs() + 1e-6).all()), f"logits: worst {float((err / (ref.abs() + 1e-3)).max()):.2e}"
    assert_close(partial[:, 0].sum(0), ref.sum(0), 1e-4, "column sums", floor=1e-3 * float(ref.abs().sum(0).max()))
    assert_close(partial[:, 1].sum(0), (ref * ref).sum(0), 1e-4, "column square sums")


def test_k1_selfcheck_passes_and_the_form_switch_works():
    """ops._k1_selfcheck: K1's hand-scheduled forward kernels against the tile-GEMM form of the same entry point, once per
    process -- on this build they agree (no warning, no form switched off); lpm_k1_forms_disable(3) really routes the entry
    points to the tile-GEMM form (the check would otherwise compare a kernel with itself)."""
    import warnings
    from learnablepoolingmethods_amd import _capi, ops
    lib = _capi.load()
    dev = cuda()
    assert lib._lpm_k1_forms_disable(0) == 0, "no form is switched off on a good build"
    ops._K1_CHECKED.clear()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ops._k1_selfcheck(lib, 2, dev)
        ops._k1_selfcheck(lib, 1, dev)
    assert ops._K1_CHECKED == {1, 2} and lib._lpm_k1_forms_disable(0) == 0
    # the switch changes the kernel that runs: the same call, timed, with and without the flat form (cfg-2's video shape)
    from learnablepoolingmethods_amd._capi import ptr, stream_ptr
    B, T, D, K = 80, 300, 1024, 256
    x = torch.randn(B * T, D, device=dev)
    W = torch.randn(D, K, device=dev) / 32
    st = stream_ptr()
    xr = torch.empty(lib._lpm_row_tiles_bytes(B, T, D) // 4, dtype=torch.int32, device=dev)
    wt = torch.empty(lib._lpm_weight_tiles_bytes(D, K) // 4, dtype=torch.int32, device=dev)
    lib.check(lib._lpm_split_rows_tiles(ptr(x), D, B, T, D, ptr(xr), st), "rows")
    lib.check(lib._lpm_split_weight_tiles(ptr(W), D, K, 0, ptr(wt), st), "weights")
    nblk = lib._lpm_assign_gemm_tiles_nblk(B, T)
    out = {}
    try:
        for mask in (0, 3):
            lib._lpm_k1_forms_disable(mask)
            lg, pt = torch.zeros(B * T, K, device=dev), torch.zeros(nblk, 2, K, device=dev)
            for _ in range(3):
                lib.check(lib._lpm_assign_gemm_tiles_fwd(ptr(xr), ptr(wt), B, T, D, K, ptr(lg), ptr(pt), st), "k1")
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                lib.check(lib._lpm_assign_gemm_tiles_fwd(ptr(xr), ptr(wt), B, T, D, K, ptr(lg), ptr(pt), st), "k1")
            e1.record()
            torch.cuda.synchronize()
            out[mask] = (lg.clone(), e0.elapsed_time(e1) / 10, int((pt.abs().sum((1, 2)) > 0).sum()))
    finally:
        lib._lpm_k1_forms_disable(0)
    assert float((out[0][0] - out[3][0]).abs().max()) <= 2e-5 * float(out[3][0].abs().max()), "the two forms agree to fp32 rounding"
    print(f"[K1 forms] flat {out[0][1] * 1e3:.1f} us ({out[0][2]} statistics rows in use), tile-GEMM form {out[3][1] * 1e3:.1f} us ({out[3][2]})")
    # another kernel runs with the mask set: the flat form reduces its statistics per 96-row group (250 rows of the partial array at this
    # shape), the tile-GEMM form per 64- / 128-row block of a clip (not a timing assertion: the box may be shared)
    assert out[0][2] == (B * T + 95) // 96 and out[3][2] != out[0][2]


@pytest.mark.parametrize("M,C,act", [(80, 512, 1), (80, 512, 2), (128, 1024, 2), (7, 40, 0), (250, 96, 1), (2, 33, 2)])
def test_bn_small_one_launch_each_way(M, C, act):
    """lpm_bn_small_fwd / _bwd: the clip-level batch norms with what follows them (frame_level_models.py:2321-2337: hidden1_bn + relu6;
    :2354-2368: gating_bn + the context gate) against fp64 autograd of the plain formulas; moving statistics with the unbiased variance."""
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    g = torch.Generator().manual_seed(M + C + act)
    x, mul, dy = torch.randn(M, C, generator=g) * 2 + 0.5, torch.randn(M, C, generator=g), torch.randn(M, C, generator=g)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    mm, mv = 0.1 * torch.randn(C, generator=g), 1 + 0.3 * torch.rand(C, generator=g)
    xd, md, gd, bd = (t.double().requires_grad_(True) for t in (x, mul, gamma, beta))
    mu, var = xd.mean(0), xd.var(0, unbiased=False)
    z = (xd - mu) * torch.rsqrt(var + ops.BN_EPS) * gd + bd
    ref = z if act == 0 else (torch.clamp(z, 0.0, 6.0) if act == 1 else md * torch.sigmoid(z))
    ref.backward(dy.double())
    xg, mg, gg, bg = (t.to(dev).requires_grad_(True) for t in (x, mul, gamma, beta))
    mmg, mvg = mm.to(dev), mv.to(dev)
    assert ops.bn_small_ok(xg, mg if act == 2 else None)
    out = ops.bn_small(xg, gg, bg, mmg, mvg, act=act, mul=mg if act == 2 else None)
    assert_close(out, ref, 1e-5, "bn_small fwd")
    out.backward(dy.to(dev))
    assert_close(xg.grad, xd.grad, 2e-5, "dx")
    assert_close(gg.grad, gd.grad, 2e-5, "dgamma")
    assert_close(bg.grad, bd.grad, 2e-5, "dbeta")
    if act == 2:
        assert_close(mg.grad, md.grad, 1e-5, "dmul")
    unb = var.detach() * (M / (M - 1))
    assert_close(mmg, mm.double() * ops.BN_DECAY + mu.detach() * (1 - ops.BN_DECAY), 1e-6, "moving_mean")
    assert_close(mvg, mv.double() * ops.BN_DECAY + unb * (1 - ops.BN_DECAY), 1e-6, "moving_variance")


@pytest.mark.parametrize("B,L,F,lazy", [(3, 64, 128, False), (2, 256, 1024, True)])
def test_layer_norm_image_is_the_split_of_its_output(B, L, F, lazy):
    """lpm_layer_norm_act_image_fwd: y3 must be bit for bit what lpm_split_rows makes of y (planes [hi | lo | hi]), y itself unchanged."""
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    g = torch.Generator(device=dev).manual_seed(F + L)
    a, r = torch.randn(B, L, F, device=dev, generator=g), torch.randn(B, L, F, device=dev, generator=g)
    gamma, beta, bias = (torch.randn(F, device=dev, generator=g) for _ in range(3))
    rs = (torch.rand(B * L, device=dev, generator=g) + 0.5) if lazy else None
    c0, c1 = ops._SubCtx(), ops._SubCtx()
    y0 = ops._ResidualLayerNorm.forward(c0, a, r, gamma, beta, bias, False, None, rs)
    y1 = ops._ResidualLayerNorm.forward(c1, a, r, gamma, beta, bias, False, None, rs, image=True)
    assert torch.equal(y0, y1)
    y3, dptr, ver = y1._lpm_y3                      # (the image travels with the identity of the tensor it images: ops._FFNBlockX3)
    assert dptr == y1.data_ptr() and ver == y1._version
    assert y3.shape == (B * L, 3 * F) and y3.dtype == torch.bfloat16
    assert torch.equal(y3.view(torch.int16), ops._split_rows(y1.view(B * L, F)).view(torch.int16))


@pytest.mark.parametrize("B,L,h,d", [(3, 300, 8, 16), (2, 40, 4, 8)])
def test_logit_stats_moments(B, L, h, d):
    """lpm_mha_logit_stats_moments: the same partial statistics as lpm_mha_logit_stats, and the (batch, head) moments of q it hands to the
    backward: Qm = sum_q q q^T, Sq = sum_q q."""
    from learnablepoolingmethods_amd import _capi, ops
    dev = cuda()
    lib = _capi.load()
    g = torch.Generator(device=dev).manual_seed(L)
    F = h * d
    q, k = torch.randn(B, L, F, device=dev, generator=g), torch.randn(B, L, F, device=dev, generator=g)
    p0, p1 = (torch.empty(B * h, 2, L, device=dev) for _ in range(2))
    mo = torch.empty(B * h, d * d + d, device=dev)
    st = ops.stream_ptr()
    lib.check(lib._lpm_mha_logit_stats(ops.ptr(q), ops.ptr(k), F, B, L, h, d, ops.ptr(p0), st), "stats")
    lib.check(lib._lpm_mha_logit_stats_moments(ops.ptr(q), ops.ptr(k), F, B, L, h, d, ops.ptr(p1), ops.ptr(mo), st), "moments")
    assert torch.equal(p0, p1)
    qh = q.double().view(B, L, h, d).permute(0, 2, 1, 3).reshape(B * h, L, d)
    assert_close(mo[:, :d * d].reshape(B * h, d, d), qh.transpose(1, 2) @ qh, 1e-5, "Qm")
    assert_close(mo[:, d * d:], qh.sum(1), 1e-5, "Sq")
