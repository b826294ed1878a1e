"""What tests/test_gpu_attention_bounds.py rests on, proven without a GPU, for the seeds, shapes and regimes that file uses:

* the restatement (tests/_attention_ref.py) is transformer_utils.py:564-581 / :652-661 on hand-made cases, and every seed meets its
  regime's condition on the fp64 values;
* the bounds can be MET: a second evaluation of the restatement in fp32 in another order (keys, queries and the columns of a head permuted:
  every sum of the forward and the backward runs in another order) stays within max(8 err32, 1e-6) of fp64, and the same permuted
  evaluation with mm3 within max(8 (err32 + errx3), 1e-6), in every regime;
* the bounds BITE: each deliberately wrong restatement exceeds them on ``out`` in the regime named for it -- eps = 1e-5 and the unbiased
  variance in static, statistics per head and the scale applied twice in random -- under the "f32" bound on every regime shape and seed,
  and under the "bf16x3" bound too (the unbiased variance there on below128 and ragged: at128's 1 040 statistics rows make it a 1e-4
  effect, 1.2 .. 2.2 of that bound, printed);
* the raw-sum variance (per-(batch, head) sums of s and s^2 in fp32, var = sum s^2 / n - mean^2) exceeds the "f32" bound on batch_var and
  on out in offset and stays inside it in random; so does the statistics kernel's own arithmetic as it stood before the shifted sums
  (kernel_moments "quad_raw": the d x d moments of q on the fp32 matrix pipe, then k^T G k), on batch_var in offset AND offset_low;
* the form the kernels use now (kernel_moments "quad_taken": the raw sums where mean^2 <= var, the sums about the per-(batch, head) pivot
  q_0 . k_j elsewhere, the groups put together in fp64) meets the bound on every part in random, offset and offset_low, and in random
  takes the raw sums in every column -- the values are then the raw form's, bit for bit."""
import pytest
import torch

from tests import _attention_ref as R
from tests import test_gpu_attention_bounds as G


def test_restatement_on_hand_made_cases():
    g = torch.Generator().manual_seed(3)
    B, L, h, d = 2, 5, 3, 4
    q, k, v = (torch.randn(B, L, h * d, generator=g, dtype=torch.float64) for _ in range(3))
    # heads are column blocks of the last axis, and split / combine are inverse
    assert torch.equal(R.split_heads(q, h)[1 * h + 2], q[1, :, 2 * d:3 * d]) and torch.equal(R.combine_heads(R.split_heads(q, h), h), q)
    out, mean, uvar = R.attention(q, k, v, h)
    want = torch.stack([torch.softmax(q[1, :, d:2 * d] @ k[1, :, d:2 * d].t() / d ** 0.5, -1) @ v[1, :, d:2 * d]])
    assert mean is None and uvar is None and float((out[1, :, d:2 * d] - want[0]).abs().max()) <= 1e-15
    # equal keys: every probability is 1 / L;  one key: out = v
    flat, _, _ = R.attention(q, k[:, :1].expand(B, L, h * d), v, h)
    assert float((flat - v.mean(1, keepdim=True)).abs().max()) <= 1e-15
    one, _, _ = R.attention(q[:, :1], k[:, :1], v[:, :1], h)
    assert torch.equal(one, v[:, :1])
    # logits_bn: the channel is the key position, the statistics run over (batch, head, query); biased variance normalises, eps = 1e-3
    gamma, beta = torch.rand(L, generator=g, dtype=torch.float64) + 0.5, torch.randn(L, generator=g, dtype=torch.float64)
    s = torch.einsum("blhd,bmhd->bhlm", q.reshape(B, L, h, d), k.reshape(B, L, h, d))
    m, var = s.mean((0, 1, 2)), s.var((0, 1, 2), unbiased=False)
    z = (s - m) / torch.sqrt(var + 1e-3) * gamma + beta
    want = torch.einsum("bhlm,bmhd->blhd", torch.softmax(z, -1), v.reshape(B, L, h, d)).reshape(B, L, h * d)
    out, mean, uvar = R.attention(q, k, v, h, bn=(gamma, beta))
    assert float((out - want).abs().max()) <= 1e-14 and float((mean - m).abs().max()) <= 1e-15
    assert float((uvar - s.var((0, 1, 2), unbiased=True)).abs().max()) <= 1e-14
    moving = (torch.randn(L, generator=g, dtype=torch.float64), torch.rand(L, generator=g, dtype=torch.float64) + 0.5)
    z = (s - moving[0]) / torch.sqrt(moving[1] + 1e-3) * gamma + beta
    want = torch.einsum("bhlm,bmhd->blhd", torch.softmax(z, -1), v.reshape(B, L, h, d)).reshape(B, L, h * d)
    out, mean, _ = R.attention(q, k, v, h, bn=(gamma, beta), training=False, moving=moving)
    assert mean is None and float((out - want).abs().max()) <= 1e-14
    # the kernels' forms are the same moments, up to fp32
    qh, kh = R.split_heads(q, h), R.split_heads(k, h)
    for form in ("quad_raw", "quad_taken"):
        km, kv = R.kernel_moments(qh, kh, form)
        assert float((km.reshape(-1) - m).abs().max()) <= 1e-5 and float((kv.reshape(-1) - var).abs().max()) <= 1e-4
    rm, rv = R.raw_sum_moments(s.reshape(B * h, L, L))
    assert float((rm.reshape(-1) - m).abs().max()) <= 1e-5 and float((rv.reshape(-1) - var).abs().max()) <= 1e-4


def test_figure_is_per_clip_for_the_parts_with_a_clip_axis():
    ref = torch.tensor([[[1.0, -2.0]], [[1e-3, 1e-3]]], dtype=torch.float64)
    got = ref.clone()
    got[1, 0, 0] += 1e-6                                    # 1e-3 of clip 1's maximum, 5e-7 of the tensor's
    assert R.figure(got, ref, "dq", 2) == pytest.approx(1e-3) and R.figure(got, ref, "dgamma", 2) == pytest.approx(5e-7)
    zero = torch.zeros(2, 1, 2, dtype=torch.float64)
    assert R.figure(zero, zero, "dk", 2) == 0.0 and R.figure(zero + 1e-30, zero, "dk", 2) == float("inf")


def test_make_inputs_follows_its_description():
    B, L, h, d = 3, 48, 2, 16
    inp = {r: R.make_inputs(B, L, h, d, 5, r) for r in R.REGIMES + ("offset_low",)}
    base = inp["random"]
    assert torch.equal(R.make_inputs(B, L, h, d, 5)["q"], base["q"]) and not torch.equal(R.make_inputs(B, L, h, d, 6)["q"], base["q"])
    assert float(base["q"].std()) == pytest.approx(0.5, rel=0.1) and float(base["upstream"].std()) == pytest.approx(1.0, rel=0.1)
    for r in ("offset", "offset_low"):
        a, sigma = R.OFFSET_LEVELS[r]
        c = inp[r]["q"].double().mean((0, 1))
        assert float((c[:d] - c[d:]).abs().max()) < 4 * sigma / (B * L) ** 0.5 * 2          # one c for every head ...
        assert float((inp[r]["k"].double().mean((0, 1)) - c).abs().max()) < 4 * sigma / (B * L) ** 0.5 * 2     # ... and for q and k
        assert float((inp[r]["q"].double() - c).std()) == pytest.approx(sigma, rel=0.1)
    assert torch.equal(inp["saturated"]["gamma"], base["gamma"] * R.SATURATED_GAMMA)
    assert torch.equal(inp["saturated"]["q_plain"], base["q"] * R.SATURATED_Q) and torch.equal(inp["saturated"]["q"], base["q"])
    ks = inp["static"]["k"].double()
    assert float((ks - ks[:, :1]).abs().max()) <= R.STATIC_NOISE and float(ks.abs().max()) < 6 * R.STATIC_KEY
    up = inp["decades"]["upstream"].reshape(B, -1).std(1)
    assert torch.allclose(up.log10(), torch.tensor([-3.0, 0.0, 3.0]), atol=0.1)
    for r in ("offset", "static", "decades"):
        assert torch.equal(inp[r]["v"], base["v"]) and torch.equal(inp[r]["gamma"], base["gamma"])


def _listed():
    for name in G.CASES:
        yield name, "random"
    for name in G.REGIME_CASES:
        for regime in G.REGIMES:
            yield name, regime


@pytest.mark.parametrize("name,regime", list(_listed()))
def test_every_seed_meets_the_condition_and_has_an_fp32_error(name, regime):
    for seed in G.SEEDS:
        for mode in G.MODES:
            _, p64, p32, _, (ok, cond) = G.reference(name, seed, regime, mode)
            print(f"[attention ref] {name} {regime} {mode} seed {seed}: condition {ok} {cond:.3e}")
            assert ok, cond
            want = ["out", "dq", "dk", "dv"] + (["dgamma", "dbeta"] if mode != "plain" else []) + \
                (["batch_mean", "batch_var"] if mode == "bn_train" else [])
            assert list(p64) == want
            for n in p64:
                assert bool(torch.isfinite(p64[n]).all()) and bool(torch.isfinite(p32[n]).all())
                if float(p64[n].abs().max()) > 0 and name != "one_key":          # (one key: out = v and dv = upstream, exactly, in any format)
                    assert R.figure(p32[n], p64[n], n, G.CASES[name][0]) > 0, n


def _permuted(name, inputs, mode, dtype, mm, seed):
    """The restatement evaluated with keys, queries and the columns of every head in another order -> parts in the ORIGINAL order."""
    B, L, h, d = G.CASES[name]
    g = torch.Generator().manual_seed(1000 + seed)
    pk, pq, pd = torch.randperm(L, generator=g), torch.randperm(L, generator=g), torch.randperm(d, generator=g)
    cols = (torch.arange(h).unsqueeze(1) * d + pd).reshape(-1)
    ik, iq, ic = torch.argsort(pk), torch.argsort(pq), torch.argsort(cols)
    p = dict(inputs)
    for n in ("q", "q_plain", "upstream"):
        if n in p:
            p[n] = inputs[n][:, pq][:, :, cols] if n != "upstream" else inputs[n][:, pq]
    p["k"], p["v"] = inputs["k"][:, pk][:, :, cols], inputs["v"][:, pk]
    p["gamma"], p["beta"], p["moving"] = inputs["gamma"][pk], inputs["beta"][pk], tuple(m[pk] for m in inputs["moving"])
    parts = R.values_and_grads(p, dtype, mm, h=h, bn=mode != "plain", training=mode != "bn_eval")
    back = dict(out=parts["out"][:, iq], dq=parts["dq"][:, iq][:, :, ic], dk=parts["dk"][:, ik][:, :, ic], dv=parts["dv"][:, ik])
    back.update({n: t[ik] for n, t in parts.items() if n not in back})
    return back


@pytest.mark.parametrize("regime", ("random",) + G.REGIMES)
@pytest.mark.parametrize("name", G.REGIME_CASES)
def test_the_bounds_can_be_met_by_an_evaluation_in_another_order(name, regime):
    B = G.CASES[name][0]
    for seed in G.SEEDS:
        for mode in G.MODES:
            inputs, p64, _, _, _ = G.reference(name, seed, regime, mode)
            bnd = G.bounds(name, seed, regime, mode)
            for prec, (dtype, mm) in (("f32", (torch.float32, torch.matmul)), ("bf16x3", (torch.float64, R.mm3))):
                got = _permuted(name, inputs, mode, dtype, mm, seed)
                ratio = {n: R.figure(got[n], p64[n], n, B) / bnd[n][2 if prec == "f32" else 3] for n in p64}
                print(f"[attention ref] {name} {regime} {mode} seed {seed} {prec}, another order, error / bound: "
                      + ", ".join(f"{n} {v:.2f}" for n, v in ratio.items()))
                assert max(ratio.values()) <= 1, (seed, mode, prec, ratio)


WRONG = (("eps", dict(eps=1e-5), "static", "bn_train"), ("unbiased", dict(unbiased=True), "static", "bn_train"),
         ("stats_per_head", dict(stats_per_head=True), "random", "bn_train"), ("scale_twice", dict(scale_twice=True), "random", "plain"))


@pytest.mark.parametrize("switch,kw,regime,mode", WRONG, ids=[w[0] for w in WRONG])
def test_each_wrong_switch_exceeds_the_bound_on_out(switch, kw, regime, mode):
    for name in G.REGIME_CASES:
        B, _, h, _ = G.CASES[name]
        for seed in G.SEEDS:
            inputs, p64, _, _, _ = G.reference(name, seed, regime, mode)
            _, _, b32, bx3 = G.bounds(name, seed, regime, mode)["out"]
            wrong = R.values_and_grads(inputs, torch.float64, h=h, bn=mode != "plain", training=True, **kw)
            e = R.figure(wrong["out"], p64["out"], "out", B)
            print(f"[attention ref] {switch} in {regime}, {name} seed {seed}: out off by {e:.3e}, {e / b32:.1f} of the f32 bound, "
                  f"{e / bx3:.1f} of the bf16x3 bound")
            assert e > b32
            if not (switch == "unbiased" and name == "at128"):
                assert e > bx3


def _ratios(name, seed, regime, **kw):
    B, _, h, _ = G.CASES[name]
    inputs, p64, _, _, _ = G.reference(name, seed, regime, "bn_train")
    bnd = G.bounds(name, seed, regime, "bn_train")
    got = R.values_and_grads(inputs, torch.float64, h=h, bn=True, training=True, **kw)
    return {n: R.figure(got[n], p64[n], n, B) / bnd[n][2] for n in p64}


@pytest.mark.parametrize("name", G.REGIME_CASES)
def test_the_raw_sum_variance_misses_in_offset_and_the_shifted_sums_meet_the_bound(name):
    B, _, h, _ = G.CASES[name]
    for seed in G.SEEDS:
        for regime in ("random", "offset", "offset_low"):
            r = {form: _ratios(name, seed, regime, **kw) for form, kw in (("raw_sum_variance", dict(raw_sum_variance=True)),
                                                                            ("quad_raw", dict(statistics="quad_raw")),
                                                                            ("quad_taken", dict(statistics="quad_taken")))}
            for form, v in r.items():
                print(f"[attention ref] {name} {regime} seed {seed} {form}, error / f32 bound: " + ", ".join(f"{n} {x:.2f}" for n, x in v.items()))
            if regime == "offset":
                assert r["raw_sum_variance"]["batch_var"] > 1 and r["raw_sum_variance"]["out"] > 1, (seed, r["raw_sum_variance"])
            if regime != "random":
                assert r["quad_raw"]["batch_var"] > 1, (seed, regime, r["quad_raw"])
            else:
                assert max(r["raw_sum_variance"].values()) <= 1 and max(r["quad_raw"].values()) <= 1, (seed, r)
                inputs = G.reference(name, seed, regime, "bn_train")[0]
                qh, kh = R.split_heads(inputs["q"], h), R.split_heads(inputs["k"], h)
                for a, b in zip(R.kernel_moments(qh, kh, "quad_raw"), R.kernel_moments(qh, kh, "quad_taken")):
                    assert torch.equal(a, b)                  # every column takes the raw sums: nothing moves
            assert max(r["quad_taken"].values()) <= 1, (seed, regime, r["quad_taken"])
