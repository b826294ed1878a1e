"""What tests/test_gpu_bn_bounds.py rests on, proven without a GPU: the restatement (tests/_bn_ref.py) is the oracle's batch_norm composed with
the same pre-steps and tails to 1e-12 on every case's shape (forward, every gradient, both moving statistics), the inputs, the error figure
and the conditions behave on hand-made cases, every seed of the GPU file meets its conditions -- and the rule BITES in the offset regime:
the raw-moment form emulated on the CPU (64-row fp32 block sums, fp64 fold, var = q / n - mu^2) misses the bound on batch_var and dx at
mean / std = 30 for every listed seed, and meets it without an offset."""
import pytest
import torch

from oracle import lpm_oracle as O
from tests import _bn_ref as R
from tests import test_gpu_bn_bounds as G


def _err(a, b):
    a, b = a.detach().double(), b.detach().double().reshape(a.shape)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _oracle_parts(inp, bias, relu, act, biased):
    """The oracle's batch_norm behind the pre-steps and in front of the tail, step by step in fp64; gradients by autograd.  The oracle feeds
    the moving variance the biased batch variance for a rank-3 input and the unbiased one for a rank-2 input."""
    leaf = lambda t: t.double().clone().requires_grad_(True)
    x = leaf(inp["x"])
    p = {"bn/gamma": leaf(inp["gamma"]), "bn/beta": leaf(inp["beta"])}
    leaves = dict(dx=x, dgamma=p["bn/gamma"], dbeta=p["bn/beta"])
    a = x
    if bias:
        leaves["dbias"] = leaf(inp["bias"])
        a = a + leaves["dbias"]
    if relu:
        a = torch.relu(a)
    upd = {}
    z = O.batch_norm(a if biased else a.reshape(-1, a.shape[-1]), p, "bn", True, upd).reshape(x.shape)
    if act == 1:
        y = torch.clamp(z, 0.0, 6.0)
    elif act == 2:
        leaves["dmul"] = leaf(inp["mul"])
        y = leaves["dmul"] * torch.sigmoid(z)
    else:
        y = z
    names = list(leaves)
    out = dict(y=y.detach(), **dict(zip(names, torch.autograd.grad((y * inp["upstream"].double()).sum(), [leaves[n] for n in names]))))
    out.update(moving_mean=R.ONE_MINUS_DECAY * upd["bn/moving_mean"], moving_var=R.ONE_MINUS_DECAY * upd["bn/moving_variance"])
    return out


def _shapes():
    seen = {}
    for name, case in G.CASES.items():
        kw = G.ref_kwargs(name)
        seen.setdefault((case["shape"], tuple(sorted(kw.items()))), name)
    return sorted(seen.values())


@pytest.mark.parametrize("name", _shapes())
def test_restatement_is_the_oracle(name):
    assert R.BN_EPS == O.BN_EPS
    kw = G.ref_kwargs(name)
    for biased in (True, False):
        for regime in ("random", "offset10"):
            inp = R.make_inputs(*G.CASES[name]["shape"], 3, regime)
            got = R.bn_ref(inp, torch.float64, **dict(kw, biased_moving_variance=biased))
            want = _oracle_parts(inp, kw["bias"], kw["relu"], kw["act"], biased)
            assert set(want) <= set(got)
            for n in want:
                if n == "dbias" and not kw["relu"]:            # zero but for rounding, either way
                    assert float((got[n] - want[n]).abs().max()) <= 1e-12 * float(got["dbeta"].abs().max()), (name, n)
                else:
                    assert _err(got[n], want[n]) <= 1e-12, (name, regime, biased, n)
    # the batch statistics are what the moving ones are made of
    assert _err(got["batch_mean"] * R.ONE_MINUS_DECAY, got["moving_mean"]) <= 1e-15
    n = inp["x"].numel() // inp["x"].shape[-1]
    assert _err(got["batch_var"] * R.ONE_MINUS_DECAY * n / (n - 1), got["moving_var"]) <= 1e-14


def test_make_inputs_follows_its_description():
    B, L, C = 4, 40, 32
    inp = {r: R.make_inputs(B, L, C, 7, r) for r in R.REGIMES}
    base = inp["random"]
    assert torch.equal(R.make_inputs(B, L, C, 7)["x"], base["x"]) and not torch.equal(R.make_inputs(B, L, C, 8)["x"], base["x"])
    x = base["x"].double().reshape(-1, C)
    assert 0.4 < float(x.std(0).min()) and float(x.std(0).max()) < 1.7 and float(x.mean(0).abs().max()) < 1.2
    for r, off in R.OFFSET.items():
        xo = inp[r]["x"].double().reshape(-1, C)
        ratio = xo.mean(0) / xo.std(0)
        assert float((ratio - off).abs().max()) < 0.2 * off, r
        for k in ("gamma", "beta", "bias", "upstream", "mul"):
            assert torch.equal(inp[r][k], base[k])
    mixed = inp["mixed_offset"]["x"].reshape(-1, C)
    assert torch.equal(mixed[:, 1::2], base["x"].reshape(-1, C)[:, 1::2]) and torch.equal(mixed[:, 0::2], inp["offset30"]["x"].reshape(-1, C)[:, 0::2])
    spread = inp["column_spread"]["x"].double().reshape(-1, C).std(0)
    assert torch.allclose(spread.log10(), torch.linspace(-2, 2, C, dtype=torch.float64), atol=0.15)
    up = base["upstream"].reshape(B, -1).std(1)
    assert torch.allclose(up.log10(), torch.tensor([-3.0, -1.0, 1.0, 3.0]), atol=0.1)
    assert float(R.make_inputs(1, L, C, 7)["upstream"].std()) == pytest.approx(1.0, abs=0.2)
    dead = inp["dead_relu"]
    assert torch.equal(dead["x"], base["x"])
    pre = (dead["x"] + dead["bias"]).reshape(-1, C)
    assert bool((pre[:, R.dead_columns(C)] < 0).all())
    cols, k = R.near_dead_columns(C)
    assert torch.equal((pre[:, cols] > 0).sum(0), k) and set(k.tolist()) == {1, 2}
    rest = torch.ones(C, dtype=torch.bool)
    rest[R.dead_columns(C)] = rest[cols] = False
    assert torch.equal(dead["bias"][rest], base["bias"][rest])


def test_figure_is_per_example_and_per_column():
    ref = torch.tensor([[[1.0, -2.0]], [[1e-3, 5e-4]]], dtype=torch.float64)          # [B = 2, L = 1, C = 2]
    got = ref.clone()
    got[1, 0, 1] += 1e-6                        # 1e-3 of example 1's maximum, 5e-7 of column 1's
    assert R.figure(got, ref, "y", 2) == pytest.approx(1e-3)
    assert R.figure(got, ref, "dgamma", 2) == pytest.approx(5e-7)
    ref2 = torch.tensor([[[1.0, 1e-4]], [[-2.0, 2e-4]]], dtype=torch.float64)         # column 1 is small in every example
    got2 = ref2.clone()
    got2[0, 0, 1] += 1e-7                       # 1e-7 of example 0's maximum, 5e-4 of column 1's
    assert R.figure(got2, ref2, "dx", 2) == pytest.approx(5e-4)
    assert R.figure(got2, ref2, "dbeta", 2) == pytest.approx(5e-8)
    assert R.figure(got2, ref2, "dbias", 2, floor=10.0) == pytest.approx(1e-8)
    # a column that is identically zero in fp64 is left out of the figure and held by exactly_zero
    ref3 = torch.tensor([[[1.0, 0.0]], [[-2.0, 0.0]]], dtype=torch.float64)
    assert R.figure(ref3, ref3, "dx", 2) == 0.0 and R.exactly_zero(ref3, ref3, "dx", None)
    leak = ref3.clone()
    leak[1, 0, 1] = 1e-30
    assert not R.exactly_zero(leak, ref3, "dx", None) and R.exactly_zero(leak, ref3 + leak, "dx", None)
    dead = torch.tensor([False, True])          # a column part: only a dead column's zero is held exactly
    assert not R.exactly_zero(torch.tensor([1.0, 1e-30]), torch.tensor([1.0, 0.0]), "dgamma", dead)
    assert R.exactly_zero(torch.tensor([1.0, 1e-30]), torch.tensor([1.0, 0.0]), "dgamma", ~dead)
    zero = torch.zeros(2, 1, 2, dtype=torch.float64)
    assert R.figure(zero, zero, "dx", 2) == 0.0 and R.figure(leak - ref3, zero, "dx", 2) == float("inf")
    assert R.figure(torch.zeros(2), torch.zeros(2), "dbias", 2) == 0.0 and R.figure(torch.tensor([0.0, 1e-30]), torch.zeros(2), "dbias", 2) == float("inf")


def test_conditions_on_hand_made_cases():
    B, L, C = 2, 40, 16
    inp = R.make_inputs(B, L, C, 0, "offset10")
    p64 = R.bn_ref(inp, torch.float64)
    ok, (lo, hi, var, least, distance) = R.conditions(inp, p64, "offset10")
    x = inp["x"].double().reshape(-1, C)
    want = x.mean(0).abs() / x.var(0, unbiased=False).sqrt()
    assert ok and lo == pytest.approx(float(want.min())) and hi == pytest.approx(float(want.max()))
    assert var == pytest.approx(float(x.var(0, unbiased=False).min())) and least > 0 and distance == float("inf")
    assert not R.conditions(inp, p64, "offset30")[0] and R.conditions(inp, p64, "random")[0]
    assert not R.conditions(inp, p64, "mixed_offset")[0]
    hollow = dict(p64, dx=p64["dx"].clone())                                          # a part that is identically zero in one example
    hollow["dx"][0] = 0
    okd, condd = R.conditions(inp, hollow, "offset10")
    assert not okd and condd[3] == 0.0
    column = dict(p64, dx=p64["dx"].clone())                                          # ... in one column
    column["dx"][:, :, 3] = 0
    assert not R.conditions(inp, column, "offset10")[0]
    # act 1: one z moved to within 1e-6 of 6
    near = dict(p64, z=p64["z"].clone())
    assert R.conditions(inp, near, "offset10", act=1)[0] == (R.conditions(inp, near, "offset10", act=1)[1][4] >= R.MIN_ACT1_DISTANCE)
    near["z"][1, 2, 3] = 6.0 - 1e-6
    okn, condn = R.conditions(inp, near, "offset10", act=1)
    assert not okn and condn[4] == pytest.approx(1e-6, rel=1e-3)
    # dead_relu: the regime's own inputs qualify; one dead column brought to life does not
    dead = R.make_inputs(B, L, C, 0, "dead_relu")
    pd = R.bn_ref(dead, torch.float64, bias=True, relu=True)
    assert R.conditions(dead, pd, "dead_relu", bias=True, relu=True)[0]
    alive = dict(dead, bias=dead["bias"].clone())
    alive["bias"][8] = 0.0
    assert not R.conditions(alive, R.bn_ref(alive, torch.float64, bias=True, relu=True), "dead_relu", bias=True, relu=True)[0]


def test_seed_table_covers_every_case_and_regime():
    assert {k for k in G.SEEDS if isinstance(k, str)} == set(G.CASES)
    assert {k for k in G.SEEDS if not isinstance(k, str)} == set(G.REGIME_PARAMS)
    assert len(G.REGIME_PARAMS) == 5 * 5 + 2
    for key, seeds in G.SEEDS.items():
        assert len(seeds) == (1 if isinstance(key, str) else 3) and len(set(seeds)) == len(seeds), key
    assert not any(c["shape"][0] * c["shape"][1] == 256 and c["shape"][2] == 1024 for c in G.CASES.values())
    for (M, C), (B, L) in G.SMALL_SHAPES.items():
        assert B * L == M <= 256


def _listed():
    for key, seeds in G.SEEDS.items():
        name, regime = (key, "random") if isinstance(key, str) else key
        for seed in seeds:
            yield pytest.param(name, regime, seed, id=f"{name}-{regime}-{seed}")


@pytest.mark.parametrize("name,regime,seed", list(_listed()))
def test_every_seed_meets_the_conditions(name, regime, seed):
    inputs, p64, p32, (ok, cond) = G.reference(name, seed, regime)
    print(f"[bn ref] {name} {regime} seed {seed}: " + ", ".join(f"{v:.2e}" for v in cond))
    assert ok, cond
    kw = G.ref_kwargs(name)
    for n, (e32, _) in G.bounds(name, seed, regime).items():                         # (the fp32 evaluation is not the fp64 one)
        assert e32 > 0 or float(p64[n].abs().max()) == 0.0, n
        assert R.exactly_zero(p32[n], p64[n], n, p64["batch_var"] == 0) or G.floor_of(name, n, inputs, p64) is not None, n
    if kw["act"] == 1:                          # no element is ever masked out of a comparison: fp32 and fp64 clamp the same elements
        assert cond[4] >= 1e-5
        for lim in (0.0, 6.0):
            assert torch.equal(p32["z"] > lim, p64["z"] > lim)
    if regime == "dead_relu":
        C = inputs["x"].shape[-1]
        a = torch.relu(inputs["x"].double() + inputs["bias"].double()).reshape(-1, C)
        assert float(a[:, R.dead_columns(C)].abs().max()) == 0.0
        cols, k = R.near_dead_columns(C)
        assert torch.equal((a[:, cols] > 0).sum(0), k)
        for n in ("dx", "dgamma", "dbias", "batch_var", "moving_mean"):
            assert float(p64[n].reshape(-1, C)[:, R.dead_columns(C)].abs().max()) == 0.0, n
        assert torch.equal(p64["y"].reshape(-1, C)[:, R.dead_columns(C)], inputs["beta"].double()[R.dead_columns(C)].expand(a.shape[0], -1))


ROWS_REGIME_CASES = [n for n in G.REGIME_CASES if G.CASES[n]["form"] != "small"]      # (bn_small is two-pass: no raw sums to emulate)


@pytest.mark.parametrize("name", ROWS_REGIME_CASES)
def test_the_bound_bites_on_the_raw_moment_form(name):
    """At mean / std = 30 the raw-sum variance misses max(8 err32, 1e-6) on batch_var and on dx for every listed seed; without an offset it
    meets it on batch_var, y and dx."""
    kw, B = G.ref_kwargs(name), G.CASES[name]["shape"][0]
    for regime, bites in (("offset30", True), ("random", False)):
        for seed in G.seeds_of(name, regime):
            inp, p64, _, _ = G.reference(name, seed, regime)
            bnd = G.bounds(name, seed, regime)
            raw = R.raw_moment_parts(inp, bias=kw["bias"], relu=kw["relu"])
            ratios = {n: R.figure(raw[n], p64[n], n, B) / bnd[n][1] for n in ("batch_var", "dx", "y", "batch_mean")}
            print(f"[bn ref] {name} {regime} seed {seed}: raw-moment form, error / bound " + ", ".join(f"{n} {v:.2f}" for n, v in ratios.items()))
            if bites:
                assert ratios["batch_var"] > 1 and ratios["dx"] > 1
            else:
                assert max(ratios["batch_var"], ratios["dx"], ratios["y"]) <= 1
