"""What tests/test_gpu_layer_norm_bounds.py rests on, proven without a GPU: the restatement (tests/_layer_norm_ref.py) is the oracle's
layer_norm composed with the same pre-steps to 1e-12 on every form, the pair is two single norms, the error figure and the conditions
behave on hand-made cases, every seed of the GPU file meets its conditions -- and the rule BITES in the offset regimes: the same
evaluation with the variance formed as mean(z^2) - mean(z)^2 from fp32 sums exceeds the bound at mean / std = 30."""
import pytest
import torch

from oracle import lpm_oracle as O
from tests import _layer_norm_ref as R
from tests import test_gpu_layer_norm_bounds as G


def _err(a, b):
    return float((a.detach().double() - b.detach().double()).abs().max() / b.detach().double().abs().max().clamp_min(1e-300))


def _oracle_parts(inp, form):
    """The oracle's layer_norm behind the form's pre-steps, written out here step by step in fp64; gradients by autograd."""
    f = R.FORMS[form]
    up = inp["upstream"].double()
    leaf = lambda t: t.double().clone().requires_grad_(True)
    a = leaf(inp["a"])
    p = {"ln/gamma": leaf(inp["gamma"]), "ln/beta": leaf(inp["beta"]), "ln2/gamma": leaf(inp["gamma2"]), "ln2/beta": leaf(inp["beta2"])}
    leaves = dict(da=a, dgamma=p["ln/gamma"], dbeta=p["ln/beta"])
    t = a
    if f.get("bias"):
        leaves["dbias"] = leaf(inp["bias"])
        t = t + leaves["dbias"]
    if f.get("relu"):
        t = torch.relu(t)
    if f.get("mask"):
        t = t * inp["mask"].double() * 10.0
    if f.get("res"):
        r = inp["r"].double()
        if f.get("row_scale"):
            r = r * inp["r_scale"].double().reshape(r.shape[0], r.shape[1], 1)
        leaves["dr"] = leaf(r)
        t = t + leaves["dr"]
    y = O.layer_norm(t, p, "ln")
    if f.get("pair"):
        y = O.layer_norm(y + leaves["dr"], p, "ln2")
        leaves = dict(da1=a, dzy=leaves["dr"], dgamma1=p["ln/gamma"], dbeta1=p["ln/beta"], dgamma2=p["ln2/gamma"], dbeta2=p["ln2/beta"],
                      dbias=leaves["dbias"])
    names = list(leaves)
    return dict(y=y.detach(), **dict(zip(names, torch.autograd.grad((y * up).sum(), [leaves[n] for n in names]))))


@pytest.mark.parametrize("regime", ["random", "offset10"])
@pytest.mark.parametrize("form", list(R.FORMS))
def test_restatement_is_the_oracle(form, regime):
    assert R.LN_EPS == O.LN_EPS
    inp = R.make_inputs(3, 5, 32, seed=3, regime=regime)
    got, want = R.layer_norm_ref(inp, torch.float64, form), _oracle_parts(inp, form)
    assert set(got) == set(want)
    for n in want:
        assert _err(got[n], want[n]) <= 1e-12, (form, n)


def test_pair_is_two_single_norms():
    """y = LN2(LN1(relu(a + bias) + r) + r): the values of two single calls, and the chain rule through them -- the second norm's dr is the
    gradient of n and of r alike, the first norm's backward takes it as dy and the residual collects both shares."""
    inp = R.make_inputs(3, 5, 32, seed=4)
    pair = R.layer_norm_ref(inp, torch.float64, "pair")
    first = R.layer_norm_ref(inp, torch.float64, "bias_relu_residual", upstream=torch.zeros_like(inp["upstream"]))
    second_in = dict(inp, a=first["y"], gamma=inp["gamma2"], beta=inp["beta2"])
    second = R.layer_norm_ref(second_in, torch.float64, "residual")
    assert _err(second["y"], pair["y"]) <= 1e-12
    back = R.layer_norm_ref(inp, torch.float64, "bias_relu_residual", upstream=second["da"])
    assert _err(back["da"], pair["da1"]) <= 1e-12 and _err(back["dr"] + second["dr"], pair["dzy"]) <= 1e-12
    assert _err(back["dgamma"], pair["dgamma1"]) <= 1e-12 and _err(back["dbeta"], pair["dbeta1"]) <= 1e-12
    assert _err(back["dbias"], pair["dbias"]) <= 1e-12
    assert _err(second["dgamma"], pair["dgamma2"]) <= 1e-12 and _err(second["dbeta"], pair["dbeta2"]) <= 1e-12


def test_make_inputs_follows_its_description():
    B, L, F = 4, 6, 32
    base, off, spread = (R.make_inputs(B, L, F, 7, regime) for regime in ("random", "offset30", "scale_spread"))
    assert torch.equal(R.make_inputs(B, L, F, 7)["a"], base["a"]) and not torch.equal(R.make_inputs(B, L, F, 8)["a"], base["a"])
    assert torch.equal(off["r"], base["r"] + 30.0) and torch.equal(off["a"], base["a"])
    s = torch.tensor([1e-2, 10 ** (-2 / 3), 10 ** (2 / 3), 1e2])
    assert torch.allclose(spread["a"], base["a"] * s.reshape(B, 1, 1), rtol=1e-6) and torch.allclose(spread["r"], base["r"] * s.reshape(B, 1, 1), rtol=1e-6)
    up = base["upstream"].reshape(B, -1).std(1)
    assert torch.allclose(up.log10(), torch.tensor([-3.0, -1.0, 1.0, 3.0]), atol=0.1)
    assert float(R.make_inputs(1, L, F, 7)["upstream"].std()) == pytest.approx(1.0, abs=0.2)
    assert 0.5 <= float(base["r_scale"].min()) and float(base["r_scale"].max()) <= 2.0 and base["r_scale"].shape == (B * L,)
    assert base["mask"].dtype == torch.bool and 0.03 < float(base["mask"].float().mean()) < 0.2


def test_figure_is_per_example_for_the_parts_with_an_example_axis():
    ref = torch.tensor([[1.0, -2.0], [1e-3, 5e-4]], dtype=torch.float64)
    got = ref.clone()
    got[1, 1] += 1e-6                         # 1e-3 of example 1's maximum, 5e-7 of the tensor's
    assert R.figure(got, ref, "y", 2) == pytest.approx(1e-3)
    assert R.figure(got, ref, "dgamma", 2) == pytest.approx(5e-7)
    zero = torch.zeros(2, 2, dtype=torch.float64)
    assert R.figure(zero, zero, "da", 2) == 0.0 and R.figure(zero, zero, "dbeta", 2) == 0.0
    leak = zero.clone()
    leak[0, 0] = 1e-30
    assert R.figure(leak, zero, "da", 2) == float("inf")
    assert R.figure(torch.stack([ref[0], leak[0]]), torch.stack([ref[0], zero[0]]), "dr", 2) == float("inf")


def test_conditions_on_hand_made_cases():
    B, L, F = 2, 4, 8
    inp = R.make_inputs(B, L, F, 0, "offset10")
    p64 = R.layer_norm_ref(inp, torch.float64, "residual")
    ok, (lo, hi, var, least) = R.conditions(inp, "residual", p64, "offset10")
    z = (inp["a"] + inp["r"]).double().reshape(B, -1)
    want = z.mean(1).abs() / z.var(1, unbiased=False).sqrt()
    assert ok and lo == pytest.approx(float(want.min())) and hi == pytest.approx(float(want.max()))
    assert var == pytest.approx(float(z.var(1, unbiased=False).min())) and least > 0
    assert not R.conditions(inp, "residual", p64, "offset30")[0]                      # mean / std about 7: outside [15, 45]
    assert R.conditions(inp, "residual", p64, "random")[0]
    flat = dict(inp, a=inp["a"].clone(), r=inp["r"].clone())                          # example 1 nearly constant: variance below 1e-6
    flat["a"][1], flat["r"][1] = 1e-4 * inp["a"][1], 1.0
    okf, condf = R.conditions(flat, "residual", R.layer_norm_ref(flat, torch.float64, "residual"), "random")
    assert not okf and condf[2] < R.MIN_VARIANCE
    dead = dict(p64, dr=p64["dr"].clone())                                            # a part that is identically zero in one example
    dead["dr"][0] = 0
    okd, condd = R.conditions(inp, "residual", dead, "offset10")
    assert not okd and condd[3] == 0.0


def test_seed_table_covers_every_case_and_regime():
    assert {k for k in G.SEEDS if isinstance(k, str)} == set(G.CASES)
    assert {k for k in G.SEEDS if not isinstance(k, str)} == {(n, r) for n in G.REGIME_CASES for r in R.REGIMES[1:]}
    for (name, regime), seeds in ((k, v) for k, v in G.SEEDS.items() if not isinstance(k, str)):
        assert len(seeds) == (3 if regime in R.OFFSET else 1), (name, regime)
    for case in G.CASES.values():
        assert case["form"] in R.FORMS and case["shape"][2] in (128, 256, 512, 1024)


def _listed():
    for key, seeds in G.SEEDS.items():
        name, regime = (key, "random") if isinstance(key, str) else key
        for seed in seeds:
            yield pytest.param(name, regime, seed, id=f"{name}-{regime}-{seed}")


@pytest.mark.parametrize("name,regime,seed", list(_listed()))
def test_every_seed_meets_the_conditions(name, regime, seed):
    ok, cond = G.reference(name, seed, regime)[3]
    print(f"[layer_norm ref] {name} {regime} seed {seed}: " + ", ".join(f"{v:.2e}" for v in cond))
    assert ok, cond
    assert all(e32 > 0 for e32, _ in G.bounds(name, seed, regime).values())           # (the fp32 evaluation is not the fp64 one)


def _one_pass_y(inp, form):
    """y with the moments as raw fp32 sums: mean = s/n, var = q/n - mean^2 (s, q fp32 sums, the fold in fp64), the rest in fp32."""
    d = {k: v.float() for k, v in inp.items()}
    z = R.pre_norm(d["a"], d["r"], d["bias"], form, d["mask"])
    flat = z.reshape(z.shape[0], -1)
    n = flat.shape[1]
    s, q = flat.sum(1).double(), (flat * flat).sum(1).double()
    mu = s / n
    var = (q / n - mu * mu).clamp_min(0)
    mean, rstd = mu.float().reshape(-1, 1, 1), torch.rsqrt(var + R.LN_EPS).float().reshape(-1, 1, 1)
    return (z - mean) * rstd * d["gamma"] + d["beta"]


@pytest.mark.parametrize("name", ["ragged", "two_rounds", "wide"])
def test_the_bound_bites_on_the_raw_moment_form(name):
    """At mean / std = 30 the raw-sum variance misses max(8 err32, 1e-6) on y for every listed seed; without an offset it meets it."""
    form, B = G.CASES[name]["form"], G.CASES[name]["shape"][0]
    for regime, bites in (("offset30", True), ("random", False)):
        for seed in G.seeds_of(name, regime):
            inp, p64, _, _ = G.reference(name, seed, regime)
            e32, bound = G.bounds(name, seed, regime)["y"]
            e1 = R.figure(_one_pass_y(inp, form), p64["y"], "y", B)
            print(f"[layer_norm ref] {name} {regime} seed {seed}: raw-moment form {e1:.3e}, err32 {e32:.3e}, bound {bound:.3e}")
            assert (e1 > bound) == bites
