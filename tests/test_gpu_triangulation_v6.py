"""-m gpu: ops.triangulation_onefc_pool (csrc/triangulation_onefc.hip), TriangulationV6Module.fused_pool and JuhanTestModelV6 against the
fp64 restatement on the CPU (tests/_triangulation_v6_ref.py) -- never against the op itself.

The bound is tests/test_gpu_triangulation.py's rule: per part and per gradient the restatement evaluated in fp32 torch on the CPU carries
an error err32 against fp64 (maximum absolute error over the maximum absolute reference); the op's error must be <= max(8 err32, 1e-6).
dalpha and dshift are sums of terms that nearly cancel: their error and their err32 are taken relative to the fp64 sum |dz A| and
sum |dz|.  A part whose fp64 reference is identically zero must be exactly zero in the op.  Every figure is printed before any is
asserted.  All inputs are drawn in fp32 and widened, so the op and the reference read the same numbers.

Conditions, asserted on the fp64 restatement before any launch: no residual squared norm and no |z|^2 below 1e-6, the largest softmax
weight at most 0.9 (T >= 2: with one frame the weight is 1 by definition) and, for T >= 3, every (clip, cluster)'s largest weight at
least 1.5 / T -- under uniform attention a wrong logit kernel would go unseen.  The scale of attention_weight that meets both weight
conditions depends on the shape: SEEDS holds the scale and the seeds found by a search on the CPU, with the margins measured there
(largest weight over the seeds, smallest (clip, cluster) maximum times T over the seeds)."""
import functools
import math

import pytest
import torch

from tests import _triangulation_v6_ref as R
from tests._util import cuda

pytestmark = pytest.mark.gpu

SEEDS = {  # (B, T, D, K, C): (scale of W, seeds, largest weight, smallest clip-cluster maximum x T)
    (3, 1, 128, 1, 1): (2.0, (0, 1, 2), 1.0, 1.0),            # one frame: p is exactly 1, dW exactly zero
    (2, 7, 128, 5, 3): (2.0, (0, 1, 2), 0.776, 1.91),         # everything odd
    (2, 30, 1024, 3, 8): (2.0, (0, 1, 2), 0.315, 2.31),       # video width at the model's T, audio's C
    (2, 33, 128, 16, 64): (2.0, (0, 1, 2), 0.690, 2.32),      # T past a 32-row tile at the largest C
    (1, 70, 128, 4, 5): (3.0, (0, 1, 2), 0.679, 11.7),
    (1, 320, 128, 2, 2): (3.0, (0, 1, 2), 0.405, 39.8),       # the largest T
}
CASES = [(shape, seed) for shape, (_, seeds, _, _) in SEEDS.items() for seed in seeds]
GRADS = ("x", "anchors", "gamma", "beta", "w", "alpha", "shift")
WORST = {"ratio": 0.0, "what": ""}


def _err(a, ref, scale=None):
    ref = ref.double()
    s = float(ref.abs().max()) if scale is None else float(scale)
    return float((a.detach().double().cpu() - ref).abs().max()) / max(s, 1e-300)


def _widen(inp32):
    return {k: v.double() for k, v in inp32.items()}


def _reference(inp32, T, batch_norm=True, stats32=None):
    """fp64 parts and gradients, and the fp32 CPU evaluation's"""
    stats64 = None if stats32 is None else tuple(s.double() for s in stats32)
    p64, g64 = R.gradients(_widen(inp32), T, batch_norm, stats64)
    p32, g32 = R.gradients(inp32, T, batch_norm, stats32)
    return dict(p64=p64, g64=g64, p32=p32, g32=g32)


@functools.lru_cache(maxsize=None)
def _random_case(shape, seed):
    B, T, D, K, C = shape
    inp32 = R.make_inputs(B, T, D, K, C, seed, w_scale=SEEDS[shape][0], dtype=torch.float32)
    return inp32, _reference(inp32, T)


def _assert_conditions(tag, inp32, T, batch_norm=True, stats32=None, saturated=False, clamped=False):
    stats64 = None if stats32 is None else tuple(s.double() for s in stats32)
    c = R.conditions(_widen(inp32), T, batch_norm, stats64)
    print(f"[triangulation_v6] {tag} conditions: min residual^2 {c['min_q']:.3e}, min |z|^2 {c['min_z2']:.3e}, largest weight "
          f"{c['max_p']:.4f}, smallest clip-cluster maximum x T {c['min_pmax_T']:.3f}")
    assert clamped or c["min_q"] >= 1e-6
    assert c["min_z2"] >= 1e-6
    if not saturated:
        assert T < 2 or c["max_p"] <= 0.9
        assert T < 3 or c["min_pmax_T"] >= 1.5


def _run_op(inp32, T, dev, batch_norm=True, stats32=None):
    from learnablepoolingmethods_amd import ops
    leaves = {n: inp32[n].to(dev).requires_grad_(True) for n in R.NAMES}
    stats = None if stats32 is None else tuple(s.to(dev) for s in stats32)
    y, bstats = ops.triangulation_onefc_pool(leaves["x"], leaves["anchors"], leaves["gamma"] if batch_norm else None,
                                             leaves["beta"] if batch_norm else None, leaves["w"], leaves["alpha"], leaves["shift"], T,
                                             batch_norm=batch_norm, stats=stats)
    names = [n for n in GRADS if batch_norm or n not in ("gamma", "beta")]
    grads = torch.autograd.grad((y * inp32["dy"].to(dev)).sum(), [leaves[n] for n in names])
    return y, bstats, dict(zip(names, grads))


def _check(tag, y, bstats, grads, ref, values_only=False):
    """Every figure is printed before anything is asserted.  -> the worst error-over-bound ratio"""
    p64, g64, p32, g32 = ref["p64"], ref["g64"], ref["p32"], ref["g32"]
    rows = [("y", y, p64["y"], p32["y"], None)]
    if bstats is not None:
        rows += [("mean", bstats[0], p64["mean"], p32["mean"], None), ("var", bstats[1], p64["var"], p32["var"], None)]
    for n in ([] if values_only else grads):
        scale = {"alpha": g64["dalpha_abs"], "shift": g64["dshift_abs"]}.get(n)
        rows.append(("d" + n, grads[n], g64[n], g32[n], scale))
    figures = []
    for n, op, r64, r32, scale in rows:
        zero = float(r64.abs().max()) == 0.0
        if zero:
            e_op, e32 = float(op.detach().abs().max()), 0.0
            print(f"[triangulation_v6] {tag} {n}: the fp64 reference is identically zero; largest |op| {e_op:.3e}")
        else:
            e_op, e32 = _err(op, r64, scale), _err(r32, r64, scale)
            print(f"[triangulation_v6] {tag} {n}: op error {e_op:.3e}, fp32 evaluation error {e32:.3e}, bound {max(8 * e32, 1e-6):.3e}, "
                  f"ratio {e_op / max(8 * e32, 1e-6):.3f}")
        figures.append((n, zero, e_op, e32))
    worst = max([e_op / max(8 * e32, 1e-6) for _, zero, e_op, e32 in figures if not zero], default=0.0)
    if worst > WORST["ratio"]:
        WORST["ratio"], WORST["what"] = worst, tag
    print(f"[triangulation_v6] {tag}: worst error over bound {worst:.3f} (so far over all cases: {WORST['ratio']:.3f} at {WORST['what']})")
    for n, zero, e_op, e32 in figures:
        if zero:
            assert e_op == 0.0, f"{tag} {n}: must be exactly zero, largest |op| {e_op:.3e}"
        else:
            assert math.isfinite(e_op) and e_op <= max(8 * e32, 1e-6), f"{tag} {n}: op error {e_op:.3e} > max(8 x {e32:.3e}, 1e-6)"
    return worst


@pytest.mark.parametrize("shape,seed", CASES)
def test_op_matches_fp64(shape, seed):
    dev = cuda()
    T = shape[1]
    inp32, ref = _random_case(shape, seed)
    tag = f"{shape} seed {seed}"
    _assert_conditions(tag, inp32, T)
    y, bstats, grads = _run_op(inp32, T, dev)
    assert y.shape == (shape[0], shape[4] * shape[3] * shape[2])
    assert not bstats[0].requires_grad and not bstats[1].requires_grad
    _check(tag, y, bstats, grads, ref)
    if T == 1:
        assert float(ref["g64"]["w"].abs().max()) == 0.0       # (the zero rule above was applied to dW)


SMALL = (2, 7, 128, 5, 3)


def test_without_batch_norm():
    dev = cuda()
    inp32 = R.make_inputs(*SMALL, seed=0, w_scale=40.0, dtype=torch.float32)      # (s is ~ 1 / sqrt(J) without the batch norm's scale)
    _assert_conditions("no batch norm", inp32, SMALL[1], batch_norm=False)
    y, bstats, grads = _run_op(inp32, SMALL[1], dev, batch_norm=False)
    assert bstats is None
    _check("no batch norm", y, None, grads, _reference(inp32, SMALL[1], batch_norm=False))


def _given_stats(J):
    g = torch.Generator().manual_seed(11)
    return (0.01 * torch.randn(J, generator=g), (0.5 + torch.rand(J, generator=g)) / J)


def test_given_statistics():
    """Inference mode: normalised with the given constants; the statistics returned are still the batch's own"""
    dev = cuda()
    B, T, D, K, C = SMALL
    inp32 = R.make_inputs(*SMALL, seed=1, w_scale=2.0, dtype=torch.float32)
    stats32 = _given_stats(K * D)
    _assert_conditions("given statistics", inp32, T, stats32=stats32)
    y, bstats, grads = _run_op(inp32, T, dev, stats32=stats32)
    _check("given statistics", y, bstats, grads, _reference(inp32, T, stats32=stats32))


@pytest.mark.parametrize("alpha", [-1.5, 0.0])
def test_negative_and_zero_alpha(alpha):
    """alpha = 0: z = shift in every element, y is constant, and every gradient but dalpha and dshift is exactly zero"""
    dev = cuda()
    inp32 = R.make_inputs(*SMALL, seed=2, w_scale=2.0, alpha=alpha, shift=0.05, dtype=torch.float32)
    _assert_conditions(f"alpha {alpha}", inp32, SMALL[1])
    y, bstats, grads = _run_op(inp32, SMALL[1], dev)
    assert all(bool(torch.isfinite(g).all()) for g in grads.values()) and bool(torch.isfinite(y).all())
    _check(f"alpha {alpha}", y, bstats, grads, _reference(inp32, SMALL[1]))


def test_saturated_softmax():
    """W ~ 30 N(0, 1): every (clip, cluster)'s largest weight is above 0.9999 in fp64, and dW is small but not identically zero"""
    dev = cuda()
    inp32 = R.make_inputs(*SMALL, seed=0, w_scale=30.0, dtype=torch.float32)
    _assert_conditions("saturated", inp32, SMALL[1], saturated=True)
    y, bstats, grads = _run_op(inp32, SMALL[1], dev)
    assert all(bool(torch.isfinite(g).all()) for g in grads.values()) and bool(torch.isfinite(y).all())
    _check("saturated", y, bstats, grads, _reference(inp32, SMALL[1]))


def test_frame_equal_to_an_anchor():
    """The clamped value: e of that (frame, anchor) is zero and the row's second norm runs over the other anchors"""
    dev = cuda()
    inp32 = R.make_inputs(*SMALL, seed=3, w_scale=2.0, dtype=torch.float32)
    inp32["x"][4] = inp32["anchors"][:, 2]
    _assert_conditions("clamped", inp32, SMALL[1], clamped=True)
    ref = _reference(inp32, SMALL[1])
    assert float(ref["p64"]["q"].min()) == 0.0
    y, bstats, grads = _run_op(inp32, SMALL[1], dev)
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    _check("clamped", y, bstats, grads, ref, values_only=True)


def test_two_runs_give_the_same_bits():
    dev = cuda()
    shape = (2, 33, 128, 16, 64)
    inp32, _ = _random_case(shape, 0)
    a = _run_op(inp32, shape[1], dev)
    b = _run_op(inp32, shape[1], dev)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1][0], b[1][0]) and torch.equal(a[1][1], b[1][1])
    for n in GRADS:
        assert torch.equal(a[2][n], b[2][n]), n


def test_refusals():
    from learnablepoolingmethods_amd import ops
    from learnablepoolingmethods_amd._capi import LpmError
    dev = cuda()
    B, T, D, K, C = 2, 4, 128, 2, 3
    J = K * D
    ok = dict(x=torch.randn(B * T, D, device=dev), anchors=torch.randn(D, K, device=dev), gamma=torch.ones(J, device=dev),
              beta=torch.zeros(J, device=dev), attention_weight=torch.randn(J, C, device=dev), alpha=torch.ones(1, device=dev),
              shift=torch.zeros(1, device=dev), max_frames=T)
    ops.triangulation_onefc_pool(**ok)
    ops.triangulation_onefc_pool(**{**ok, "gamma": None, "beta": None, "batch_norm": False})
    bad = [
        ("cpu x", {"x": ok["x"].cpu()}),
        ("feature size", {"x": torch.randn(B * T, 256, device=dev), "anchors": torch.randn(256, K, device=dev),
                          "attention_weight": torch.randn(256 * K, C, device=dev), "gamma": torch.ones(256 * K, device=dev),
                          "beta": torch.zeros(256 * K, device=dev)}),
        ("no frames", {"max_frames": 0}),
        ("too many frames", {"x": torch.randn(321, D, device=dev), "max_frames": 321}),
        ("rows not divided", {"max_frames": 3}),
        ("no clusters", {"attention_weight": torch.randn(J, 0, device=dev)}),
        ("too many clusters", {"attention_weight": torch.randn(J, 65, device=dev)}),
        ("weight rows", {"attention_weight": torch.randn(J + 1, C, device=dev)}),
        ("x not contiguous", {"x": torch.randn(B * T, 2 * D, device=dev)[:, :D]}),
        ("x fp16", {"x": ok["x"].half()}),
        ("weight fp64", {"attention_weight": ok["attention_weight"].double()}),
        ("gamma shape", {"gamma": torch.ones(J + 1, device=dev)}),
        ("gamma missing", {"gamma": None}),
        ("alpha shape", {"alpha": torch.ones(2, device=dev)}),
        ("shift cpu", {"shift": torch.zeros(1)}),
        ("stats length", {"stats": (torch.zeros(J, device=dev),)}),
        ("stats without batch norm", {"batch_norm": False, "stats": (torch.zeros(J, device=dev), torch.ones(J, device=dev))}),
    ]
    for what, change in bad:
        with pytest.raises(LpmError):
            ops.triangulation_onefc_pool(**{**ok, **change})
            pytest.fail(f"{what}: not refused")


def _moving(mean, var, n):
    """layers.batch_norm's rank-2 rule from zeros / ones: moving mean, then moving variance (the unbiased estimate)"""
    from learnablepoolingmethods_amd import layers
    return [(1 - layers.BN_DECAY) * mean, layers.BN_DECAY + (1 - layers.BN_DECAY) * var * n / (n - 1)]


def test_module_on_the_gpu_fused_against_pool():
    """fused_pool and pool with the same variables on the GPU: the pooled rows, the gradients and the moving averages, each held to the
    rule against the same fp64 yardstick"""
    from learnablepoolingmethods_amd import variables as vs, video_pooling_modules as M
    dev = cuda()
    B, T, D, K, C = SMALL
    J = K * D
    inp32, ref = _random_case(SMALL, 0)
    _assert_conditions("module", inp32, T)
    moving_names = ("spatial_bn/moving_mean", "spatial_bn/moving_variance")
    mv64 = _moving(ref["p64"]["mean"], ref["p64"]["var"], B * T)
    mv32 = _moving(ref["p32"]["mean"], ref["p32"]["var"], B * T)
    for path in ("pool", "fused_pool"):
        leaves = {n: inp32[n].to(dev).requires_grad_(True) for n in R.NAMES}
        store = vs.VariableStore(device=dev)
        for name, v, tr in (("anchor_weights", leaves["anchors"], True), ("spatial_bn/beta", leaves["beta"], True),
                            ("spatial_bn/gamma", leaves["gamma"], True), ("spatial_bn/moving_mean", torch.zeros(J, device=dev), False),
                            ("spatial_bn/moving_variance", torch.ones(J, device=dev), False), ("one_fc_attention_weight", leaves["w"], True),
                            ("alpha", leaves["alpha"], True), ("beta", leaves["shift"], True)):
            store.vars[name], store.trainable[name] = v, tr
        with vs.use_store(store):
            module = M.TriangulationV6Module(D, T, K, False, 6, 5, 7, C, True, True, True)
            y = getattr(module, path)(leaves["x"])
        assert len(store.vars) == 8
        grads = dict(zip(GRADS, torch.autograd.grad((y * inp32["dy"].to(dev)).sum(), [leaves[n] for n in GRADS])))
        _check(f"module.{path}", y, None, grads, ref)
        rows = [(n, _err(store.vars[n], r64), _err(r32, r64)) for n, r64, r32 in zip(moving_names, mv64, mv32)]
        for n, e_op, e32 in rows:
            print(f"[triangulation_v6] module.{path} {n}: error {e_op:.3e}, fp32 evaluation error {e32:.3e}")
        for n, e_op, e32 in rows:
            assert e_op <= max(8 * e32, 1e-6), f"module.{path} {n}"


MODEL = dict(iterations=6, video_anchor_size=4, audio_anchor_size=2, video_cluster_size=3, audio_cluster_size=2, video_output_dim=16,
             audio_output_dim=8)
MODEL_SEED = 41
MODEL_W_SCALE = {"video": 115.0, "audio": 14.0}    # x the xavier draw of one_fc_attention_weight, searched like SEEDS: largest weight
# 0.859 / 0.841, smallest clip-cluster maximum x T 1.611 / 1.593 (video / audio)


def _model_run(state, xin, nf, lab, u, device, dtype, fused):
    """One training forward + backward of JuhanTestModelV6 from ``state``: predictions, loss and every trainable variable's gradient."""
    from learnablepoolingmethods_amd import FLAGS, losses, registry, variables as vs
    store = vs.VariableStore(device=device)
    for n, (v, tr) in state.items():
        store.vars[n] = v.to(device=device, dtype=dtype).clone().requires_grad_(tr)
        store.trainable[n] = tr
    FLAGS.triangulation_v6_fused = fused
    try:
        with vs.use_store(store), vs.variable_scope("tower"):
            result = registry.get_model("JuhanTestModelV6").create_model(xin.to(device=device, dtype=dtype), num_frames=nf.to(device),
                                                                         vocab_size=lab.shape[1], is_training=True, frame_uniform=u, **MODEL)
        store.pop_regularization_losses()
    finally:
        FLAGS.reset()
    pred = result["predictions"]
    loss = losses.CrossEntropyLoss().calculate_loss(pred, lab.to(device))
    names = [n for n, tr in store.trainable.items() if tr]
    grads = torch.autograd.grad(loss, [store.vars[n] for n in names])
    return dict(predictions=pred.detach(), loss=loss.detach().reshape(1), **{"grad " + n: g for n, g in zip(names, grads)})


def _model_state():
    """The synthetic batch, the frame draws and the variables of the model test (one_fc_attention_weight rescaled per stream)"""
    from oracle import lpm_oracle as O
    from learnablepoolingmethods_amd import layers, registry, variables as vs
    Vn, B, MF = 20, 4, 8
    x, nf, lab = O.make_synthetic_batch(B, MF, 1152, Vn, seed=MODEL_SEED, min_frames=MODEL["iterations"])
    xin = layers.l2_normalize(x, 2)                        # train.normalize_input's formula, once, for all three runs
    g = torch.Generator().manual_seed(42)
    u = torch.stack([(torch.randperm(int(n), generator=g)[:MODEL["iterations"]].float() + 0.5) / float(n) for n in nf])
    init = vs.VariableStore(device="cpu", seed=3)
    with vs.use_store(init), vs.variable_scope("tower"):
        registry.get_model("JuhanTestModelV6").create_model(xin, num_frames=nf, vocab_size=Vn, is_training=False, frame_uniform=u, **MODEL)
    init.pop_regularization_losses()
    state = {n: (v.detach().clone(), init.trainable[n]) for n, v in init.vars.items()}
    for name, scale in MODEL_W_SCALE.items():
        state[f"tower/{name}_triangulation_embedding/one_fc_attention_weight"][0].mul_(scale)
    return xin, nf, lab, u, state


def _model_conditions(xin, nf, u, state):
    """The op's conditions per stream, on the rows the stream's module reads (behind video_bn / audio_bn in training mode)"""
    from learnablepoolingmethods_amd import model_utils
    T = MODEL["iterations"]
    frames = model_utils.SampleRandomFrames(xin, nf.reshape(-1, 1), T, uniform=u).reshape(-1, 1152).double()
    out = {}
    for name, cols in (("video", slice(0, 1024)), ("audio", slice(1024, None))):
        s = f"tower/{name}_triangulation_embedding/"
        rows = R.batch_norm(frames[:, cols], state[f"tower/{name}_bn/gamma"][0].double(), state[f"tower/{name}_bn/beta"][0].double())
        inp = {"x": rows, "anchors": state[s + "anchor_weights"][0].double(), "gamma": state[s + "spatial_bn/gamma"][0].double(),
               "beta": state[s + "spatial_bn/beta"][0].double(), "w": state[s + "one_fc_attention_weight"][0].double(),
               "alpha": state[s + "alpha"][0].double(), "shift": state[s + "beta"][0].double()}
        out[name] = R.conditions(inp, T)
    return out


def test_juhan_test_model_v6_fused_on_the_gpu_against_the_fp64_cpu_path():
    """B = 4, 6 sampled frames, anchors 4 / 2, clusters 3 / 2, output 16 / 8, vocab 20: the model with FLAGS.triangulation_v6_fused on the
    GPU against the model built on the fp64 CPU path from the same variables and frame draws; err32 is the fp32 CPU path's.  No variable
    of this model has a gradient that is zero in exact arithmetic (no bias stands in front of a batch norm, and alpha and beta share
    the one direction the row normalisation removes), so every variable is held to the rule on its own scale."""
    dev = cuda()
    xin, nf, lab, u, state = _model_state()
    for name, c in _model_conditions(xin, nf, u, state).items():
        print(f"[triangulation_v6] model {name} stream conditions: min residual^2 {c['min_q']:.3e}, min |z|^2 {c['min_z2']:.3e}, largest "
              f"weight {c['max_p']:.4f}, smallest clip-cluster maximum x T {c['min_pmax_T']:.3f}")
        assert c["min_q"] >= 1e-6 and c["min_z2"] >= 1e-6 and c["max_p"] <= 0.9 and c["min_pmax_T"] >= 1.5, name
    r64 = _model_run(state, xin, nf, lab, u, "cpu", torch.float64, False)
    r32 = _model_run(state, xin, nf, lab, u, "cpu", torch.float32, False)
    got = _model_run(state, xin, nf, lab, u, dev, torch.float32, True)
    assert got["predictions"].shape == (4, 20) and set(got) == set(r64)
    rows = [(n, _err(got[n], r64[n]), _err(r32[n], r64[n])) for n in r64]
    for n, e_op, e32 in rows:
        print(f"[triangulation_v6] model {n}: error {e_op:.3e}, fp32 evaluation error {e32:.3e}, bound {max(8 * e32, 1e-6):.3e}, "
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
    FLAGS.triangulation_v6_fused = True
    try:
        tr = Trainer(registry.get_model("JuhanTestModelV6"), vocab_size=Vn, batch_size=B, base_learning_rate=1e-3, device=dev, seed=3,
                     model_kwargs=MODEL)
        training.run(tr, iter(batches), log_every=1, log=lambda s: None, on_step=lambda out, batch: losses.append(float(out["loss"])))
    finally:
        FLAGS.reset()
    print(f"[triangulation_v6] run loop losses {losses}")
    assert len(losses) == 3 and all(math.isfinite(v) for v in losses)
