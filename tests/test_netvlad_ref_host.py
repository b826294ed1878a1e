"""What tests/test_gpu_netvlad_bounds.py rests on, proven without a GPU: the restatement (tests/_netvlad_ref.py) is the oracle's
NetVLAD to 1e-12, the split-operand product mm3 meets its derived bound and has the stated backward, every seed of the GPU file meets its
conditions -- and the bounds BITE: a restatement with cluster_bn's epsilon at 1e-5, or normalising with the unbiased variance, exceeds
both bounds of every random-regime case that has a training-mode batch norm and more than one frame per clip."""
import pytest
import torch

from oracle import lpm_oracle as O
from tests import _netvlad_ref as R
from tests import test_gpu_netvlad_bounds as G


def _err(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("B,T,D,K", [(2, 37, 128, 64), (3, 9, 32, 16)])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("light", [False, True])
def test_restatement_is_the_oracle(B, T, D, K, training, light):
    inp = R.make_inputs(B, T, D, K, seed=3)
    form = "light" if light else "netvlad"
    parts = R.values_and_grads(inp, T, torch.float64, form=form, training=training)
    p = {"s/cluster_weights": inp["W"].double().requires_grad_(True), "s/cluster_bn/gamma": inp["gamma"].double().requires_grad_(True),
         "s/cluster_bn/beta": inp["beta"].double().requires_grad_(True), "s/cluster_weights2": inp["W2"].double().requires_grad_(True),
         "s/cluster_bn/moving_mean": inp["moving"][0].double(), "s/cluster_bn/moving_variance": inp["moving"][1].double()}
    x = inp["x"].double().requires_grad_(True)
    upd = {}
    out = (O.lightvlad_forward if light else O.netvlad_forward)(x, p, "s", T, True, training, upd)
    (out * inp["upstream"].double()).sum().backward()
    want = dict(out=out.detach(), dx=x.grad, dW=p["s/cluster_weights"].grad, dgamma=p["s/cluster_bn/gamma"].grad,
                dbeta=p["s/cluster_bn/beta"].grad)
    if not light:
        want["dW2"] = p["s/cluster_weights2"].grad
    if training:
        want.update(batch_mean=upd["s/cluster_bn/moving_mean"], batch_var=upd["s/cluster_bn/moving_variance"])
    assert set(parts) == set(want)
    for n in want:
        assert _err(parts[n], want[n]) <= 1e-12, n


@pytest.mark.parametrize("B,T,D,K", [(2, 37, 128, 64), (3, 9, 32, 16)])
def test_bias_branch_and_aggregate_are_the_oracle(B, T, D, K):
    inp = R.make_inputs(B, T, D, K, seed=4)
    parts = R.values_and_grads(inp, T, torch.float64, form="bias")
    p = {"s/cluster_weights": inp["W"].double().requires_grad_(True), "s/cluster_biases": inp["bias"].double().requires_grad_(True),
         "s/cluster_weights2": inp["W2"].double().requires_grad_(True)}
    x = inp["x"].double().requires_grad_(True)
    out = O.netvlad_forward(x, p, "s", T, False, True)
    (out * inp["upstream"].double()).sum().backward()
    want = dict(out=out.detach(), dx=x.grad, dW=p["s/cluster_weights"].grad, dbias=p["s/cluster_biases"].grad, dW2=p["s/cluster_weights2"].grad)
    assert set(parts) == set(want)
    for n in want:
        assert _err(parts[n], want[n]) <= 1e-12, n
    parts = R.values_and_grads(inp, T, torch.float64, form="aggregate")
    s, x, c = (inp[k].double().requires_grad_(True) for k in ("sims", "x", "W2"))
    out = O.vlad_aggregate(s, x.reshape(B, T, D), c[0])
    (out * inp["upstream"].double()).sum().backward()
    for n, w in dict(out=out.detach(), dsims=s.grad, dx=x.grad, dcentres=c.grad).items():
        assert _err(parts[n], w) <= 1e-12, n


@pytest.mark.parametrize("training", [True, False])
def test_input_bn_is_the_oracles_batch_norm(training):
    g = torch.Generator().manual_seed(5)
    frames = torch.randn(77, 96, generator=g, dtype=torch.float64) * 3 + 1
    p = {"bn/gamma": torch.randn(96, generator=g, dtype=torch.float64), "bn/beta": torch.randn(96, generator=g, dtype=torch.float64),
         "bn/moving_mean": torch.randn(96, generator=g, dtype=torch.float64), "bn/moving_variance": torch.rand(96, generator=g, dtype=torch.float64) + 0.5}
    upd = {}
    want = O.batch_norm(frames, p, "bn", training, upd)
    y, mean, uvar = R.input_bn(frames, p["bn/gamma"], p["bn/beta"], training=training, moving=(p["bn/moving_mean"], p["bn/moving_variance"]))
    assert _err(y, want) <= 1e-12
    if training:
        assert _err(mean, upd["bn/moving_mean"]) <= 1e-12 and _err(uvar, upd["bn/moving_variance"]) <= 1e-12
    else:
        assert mean is None and uvar is None


def test_mm3_meets_its_derived_bound():
    """|mm3(a, b) - a b| <= 3 * 2^-18 (|a| |b|) componentwise, inner sizes 16 / 128 / 1024, operand scales 1e-3 / 1 / 37."""
    worst = 0.0
    g = torch.Generator().manual_seed(0)
    for inner in (16, 128, 1024):
        for sa in (1e-3, 1.0, 37.0):
            for sb in (1e-3, 1.0, 37.0):
                a = (torch.randn(48, inner, generator=g) * sa).double()
                b = (torch.randn(inner, 40, generator=g) * sb).double()
                ratio = float(((R.mm3(a, b) - a @ b).abs() / (a.abs() @ b.abs())).max()) * 2 ** 18
                worst = max(worst, ratio)
                assert ratio <= 3.0, (inner, sa, sb, ratio)
    print(f"[netvlad ref] mm3: worst componentwise |mm3(a, b) - a b| / (|a| |b|) = {worst:.3f} * 2^-18 (bound 3)")
    # the batched form is the 2-D form per batch entry
    a, b = torch.randn(3, 5, 16, generator=g).double(), torch.randn(3, 16, 7, generator=g).double()
    assert torch.equal(R.mm3(a, b), torch.stack([R.mm3(a[i], b[i]) for i in range(3)]))


def test_mm3_backward_is_the_three_term_product_of_the_gradient():
    """The stated backward: da = three_term(g, b^T), db = three_term(a^T, g), bit for bit; and against autograd of the written-out forward
    ah bh + ah bl + al bh with the operand splits detached (leaves): its gradient for the hi part, g (bh + bl)^T, is the same product
    with g unsplit and is met within the derived bound."""
    g_ = torch.Generator().manual_seed(1)
    a = torch.randn(24, 128, generator=g_).double().requires_grad_(True)
    b = torch.randn(128, 40, generator=g_).double().requires_grad_(True)
    g = torch.randn(24, 40, generator=g_).double()
    da, db = torch.autograd.grad((R.mm3(a, b) * g).sum(), [a, b])
    assert torch.equal(da, R.three_term(g, b.detach().t())) and torch.equal(db, R.three_term(a.detach().t(), g))
    ah, al = (t.requires_grad_(True) for t in R.split_bf16(a.detach()))
    bh, bl = (t.requires_grad_(True) for t in R.split_bf16(b.detach()))
    written = ah @ bh + ah @ bl + al @ bh
    assert torch.equal(written, R.mm3(a, b).detach())
    dah, dbh = torch.autograd.grad((written * g).sum(), [ah, bh])
    lim = 3 * 2.0 ** -18
    assert bool(((da - dah).abs() <= lim * (g.abs() @ b.detach().abs().t())).all())
    assert bool(((db - dbh).abs() <= lim * (a.detach().abs().t() @ g.abs())).all())


def _all_seeded():
    for key, seeds in G.SEEDS.items():
        name, regime = (key, "random") if isinstance(key, str) else key
        for seed in seeds:
            yield name, regime, seed


def test_seed_table_covers_every_case_and_regime():
    assert {k for k in G.SEEDS if isinstance(k, str)} == set(G.CASES)
    assert {k for k in G.SEEDS if not isinstance(k, str)} == {(n, r) for n in G.REGIME_CASES for r in R.REGIMES[1:]}
    for name in G.REGIME_CASES:
        assert len(G.SEEDS[name]) == 3 and all(len(G.SEEDS[(name, r)]) == 3 for r in R.REGIMES[1:])
    # every route is a list of tracked entry names, and every tracked name but the unreachable one is reached by some case
    reached = set()
    for name, case in G.CASES.items():
        for prec in case["precisions"]:
            assert G.route_of(name, prec) <= G.TRACKED
            reached |= G.route_of(name, prec)
    assert G.TRACKED - reached == {"lpm_assign_gemm_tiles_bwd_dx"}


@pytest.mark.parametrize("name,regime,seed", list(_all_seeded()))
def test_every_seed_meets_the_conditions(name, regime, seed):
    ok, cond = G.reference(name, seed, regime)[4]
    print(f"[netvlad ref] {name} {regime} seed {seed}: " + ", ".join(f"{v:.2e}" for v in cond))
    assert ok, cond


def _bn_cases():
    """Random-regime cases with a training-mode batch norm and more than one frame per clip (without batch statistics, or with T = 1, where
    the descriptor does not depend on the assignment, neither injected error changes anything: k64_eval, k64_bias, k128_kmajor_eval,
    one_frame, the vlad_aggregate cases)."""
    for name, case in G.CASES.items():
        B, T, _, _ = case["shape"]
        if case["form"] in ("netvlad", "light", "input_affine") and case["opts"].get("training", True) and T > 1:
            yield name


@pytest.mark.parametrize("name", list(_bn_cases()))
def test_the_bound_bites(name):
    case = G.CASES[name]
    B, T, _, _ = case["shape"]
    for seed in G.seeds_of(name):
        inputs, p64, _, _, _ = G.reference(name, seed)
        bnd = G.bounds(name, seed)
        others = [n for n in p64 if n not in ("out", "batch_mean", "batch_var")]
        for wrong in (dict(eps=1e-5), dict(normalise_unbiased=True)):
            pw = R.values_and_grads(inputs, T, torch.float64, form=case["form"], **wrong)
            fig = {n: R.figure(pw[n], p64[n], n, B) for n in ["out"] + others}
            over = {n: fig[n] > bnd[n][3] and fig[n] > bnd[n][2] for n in fig}
            print(f"[netvlad ref] {name} seed {seed} {wrong}: " + ", ".join(
                f"{n} {fig[n]:.1e} / f32 bound {bnd[n][2]:.1e} / bf16x3 bound {bnd[n][3]:.1e}" for n in fig))
            assert over["out"], (name, wrong, fig["out"], bnd["out"])
            assert sum(over[n] for n in others) >= len(others) - 1, (name, wrong, over)
