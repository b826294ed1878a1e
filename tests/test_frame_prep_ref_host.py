"""What tests/test_gpu_frame_prep_bounds.py rests on, proven without a GPU: the restatement (tests/_frame_prep_ref.py) is the reader's tail
and the oracle's sampling and batch norm on hand-made cases, the inputs follow their description, every listed seed meets its conditions
for the uniform index and for the index table -- and the rule BITES: frame_stats_kernel's statistics emulated on the CPU as they stood
before the shifted sums (32-row fp32 block sums s += v, q = fma(v, v, q), fp64 fold, var = q / n - mean^2) miss max(8 err32, 1e-6) on
batch_var in offset10, offset30, mixed and q8_narrow and on y in offset10 and offset30 for every listed seed and meet it in random (on
batch_var only where the one-frame clip is a minority of the batch: where it is half of it they stand at the bound, 1.02), while the form
with the shifted sums beside them (pivot: eight gathered rows spread over the batch) meets it on every part in every regime.
What the emulation shows of the pivots that were tried is printed and held by test_pivot_choices (worst error / bound on batch_var over the three regime shapes, three seeds, both index kinds):
row 0 alone up to 3.1, the first eight rows up to 1.9, eight rows spread over all B S rows at most 0.32 in every offset regime; where
every clip has its own column means (clip_offsets) the first eight rows -- rows of ONE clip -- leave 1.11, the spread rows 0.24."""
import pytest
import torch

from oracle import lpm_oracle as O
from tests import _frame_prep_ref as R
from tests import test_gpu_frame_prep_bounds as G

BITES = {"batch_var": ("offset10", "offset30", "mixed", "q8_narrow"), "y": ("offset10", "offset30")}


def test_restatement_on_hand_made_cases():
    q = torch.tensor([[[0, 255, 128, 64]], [[1, 2, 3, 4]]], dtype=torch.uint8)
    x = R.dequantize(q, torch.float64)
    assert x[0, 0, 0] == pytest.approx(4 / 512 - 2, abs=1e-15) and x[0, 0, 1] == pytest.approx(2 + 4 / 512, abs=1e-15)
    assert x[0, 0, 2] == pytest.approx(128 * 4 / 255 + 4 / 512 - 2, abs=1e-15)
    frames = torch.arange(2 * 3 * 4, dtype=torch.float64).reshape(2, 3, 4) + 1
    nf = torch.tensor([3, 1])
    z = R.zero_padding(frames, nf)
    assert torch.equal(z[0], frames[0]) and torch.equal(z[1, 0], frames[1, 0]) and float(z[1, 1:].abs().max()) == 0
    n = R.l2_normalize_rows(z)
    assert torch.allclose((n[0] ** 2).sum(-1), torch.ones(3, dtype=torch.float64)) and float(n[1, 1:].abs().max()) == 0
    tiny = R.l2_normalize_rows(torch.full((1, 4), 1e-9, dtype=torch.float64))       # squared norm 4e-18, below the 1e-12 clamp
    assert torch.allclose(tiny, torch.full((1, 4), 1e-3, dtype=torch.float64))
    nf2 = torch.tensor([40, 17, 1])
    assert torch.equal(R.uniform_index(nf2, 7), torch.from_numpy(O.sample_uniform_frame_index(nf2.numpy(), 7)).long())
    inputs = dict(frames=frames.float(), nf=nf, random_index=torch.tensor([[2, 2, 0], [0, 0, 0]]))
    rows = R.sampled_rows(inputs, torch.float64, False, 3)
    assert torch.equal(rows, torch.stack([frames[0, 2], frames[0, 2], frames[0, 0], frames[1, 0], frames[1, 0], frames[1, 0]]))
    # the batch norm is the oracle's over the sampled rows
    g = torch.Generator().manual_seed(0)
    v, gamma, beta = torch.randn(12, 8, generator=g).double(), torch.rand(8, generator=g).double() + 0.5, torch.randn(8, generator=g).double()
    upd = {}
    want = O.batch_norm(v, {"bn/gamma": gamma, "bn/beta": beta}, "bn", True, upd)
    y, mean, uvar = R.input_bn(v, gamma, beta, training=True)
    assert float((y - want).abs().max()) <= 1e-12
    assert float((mean - v.mean(0)).abs().max()) <= 1e-15 and float((uvar - v.var(0, unbiased=True)).abs().max()) <= 1e-14


def test_make_inputs_follows_its_description():
    B, MF, F, S = 4, 60, 32, 9
    inp = {r: R.make_inputs(B, MF, F, S, 5, r) for r in R.REGIMES}
    base = inp["random"]
    assert torch.equal(R.make_inputs(B, MF, F, S, 5)["frames"], base["frames"])
    assert not torch.equal(R.make_inputs(B, MF, F, S, 6)["frames"], base["frames"])
    assert int(base["nf"][0]) == MF and int(base["nf"][-1]) == 1 and bool((base["nf"] >= 1).all()) and bool((base["nf"] <= MF).all())
    idx = base["random_index"]
    assert bool((idx < base["nf"].unsqueeze(1)).all()) and torch.equal(idx[:, -1], base["nf"] - 1) and torch.equal(idx[:, 0], idx[:, 1])
    up = base["up"].reshape(B, -1).std(1)
    assert torch.allclose(up.log10(), torch.tensor([-3.0, -1.0, 1.0, 3.0]), atol=0.1)
    x = base["frames"].double().reshape(-1, F)
    assert 0.4 < float(x.std(0).min()) and float(x.std(0).max()) < 1.7 and float(x.mean(0).abs().max()) < 1.3
    for r, off in R.OFFSET.items():
        xo = inp[r]["frames"].double().reshape(-1, F)
        assert float(((xo.mean(0).abs() / xo.std(0)) - off).abs().max()) < 0.25 * off, r
        for k in ("gamma", "beta", "up", "nf", "random_index"):
            assert torch.equal(inp[r][k], base[k])
    assert bool((inp["offset30"]["frames"].reshape(-1, F).mean(0) < 0).any()) and bool((inp["offset30"]["frames"].reshape(-1, F).mean(0) > 0).any())
    mixed = inp["mixed"]["frames"].reshape(-1, F)
    assert torch.equal(mixed[:, 1::2], base["frames"].reshape(-1, F)[:, 1::2])
    assert torch.equal(mixed[:, 0::2], inp["offset30"]["frames"].reshape(-1, F)[:, 0::2])
    spread = inp["column_spread"]["frames"].double().reshape(-1, F).std(0)
    assert torch.allclose(spread.log10(), torch.linspace(-4, 0, F, dtype=torch.float64), atol=0.15)
    clips = inp["clip_offsets"]["frames"].double()
    within, between = clips.std(1).mean(0), clips.mean(1).std(0)
    assert float((within / between).median()) == pytest.approx(R.CLIP_WITHIN, rel=0.5)
    for r in R.Q8_REGIMES:
        assert inp[r]["q"].dtype == torch.uint8 and "frames" not in inp[r]
    q = inp["q8_random"]["q"].double()
    assert float(q.min()) == 0 and float(q.max()) == 255 and float(q.mean()) == pytest.approx(127.5, abs=3)
    qn = inp["q8_narrow"]["q"].double().reshape(-1, F)
    assert 39 <= float(qn.mean(0).min()) and float(qn.mean(0).max()) <= 217
    assert float(qn.std(0).mean()) == pytest.approx(R.Q8_NARROW_LEVELS, rel=0.1)


def test_figure_of_y_is_per_clip_and_per_column():
    ref = torch.tensor([[1.0, 1e-4], [-2.0, 2e-4], [1e-3, 1e-4], [1e-3, 3e-4]], dtype=torch.float64)         # B = 2 clips of S = 2 rows
    got = ref.clone()
    got[0, 1] += 1e-7                           # 5e-8 of clip 0's maximum, 3.3e-4 of column 1's
    assert R.part_figure(got, ref, "y", 2) == pytest.approx(1e-7 / 3e-4)
    got2 = ref.clone()
    got2[2, 0] += 1e-6                          # 1e-3 of clip 1's maximum, 5e-7 of column 0's
    assert R.part_figure(got2, ref, "y", 2) == pytest.approx(1e-3)
    assert R.part_figure(got2[:, 0], ref[:, 0], "dgamma", 2) == pytest.approx(5e-7)


def test_conditions_on_hand_made_cases():
    shape = (5, 40, 128, 7)
    B, MF, F, S = shape
    inp = R.make_inputs(B, MF, F, S, 0, "offset10")
    p64, p32 = (R.frame_prep_ref(inp, dt, S) for dt in (torch.float64, torch.float32))
    ok, (e32, norm, median, most, var) = R.conditions(inp, S, p64, p32, regime="offset10")
    ratio, v = R.column_ratio(R.sampled_rows(inp, torch.float64, True, S))
    assert ok and norm == float("inf") and median == pytest.approx(float(ratio.median())) and most == pytest.approx(float(ratio.max()))
    assert var == pytest.approx(float(v.min())) and e32 > 0
    assert not R.conditions(inp, S, p64, p32, regime="offset30")[0] and R.conditions(inp, S, p64, p32, regime="random")[0]
    assert not R.conditions(inp, S, p64, p32, regime="mixed")[0]
    assert not R.conditions(inp, S, p64, p64, regime="offset10")[0]                     # err32 = 0: the fp32 evaluation is not one
    padded = dict(inp, random_index=inp["random_index"].clone())
    padded["random_index"][1, 0] = int(inp["nf"][1])                                    # a sampled row past num_frames
    assert not R.conditions(padded, S, p64, p32, uniform=False, regime="offset10")[0]
    q = R.make_inputs(B, MF, F, S, 0, "q8_narrow")
    q64, q32 = (R.frame_prep_ref(q, dt, S) for dt in (torch.float64, torch.float32))
    assert R.conditions(q, S, q64, q32, regime="q8_narrow")[0]
    assert not R.conditions(R.make_inputs(B, MF, F, S, 0, "q8_random"), S, q64, q32, regime="q8_narrow")[0]
    constant = dict(inp, frames=inp["frames"].clone())
    constant["frames"][:, :, 3] = 1.5                                                  # a column without variance
    assert not R.conditions(constant, S, p64, p32, regime="random")[0]


def test_seed_table_covers_every_shape_and_regime():
    assert set(G.SEEDS) == set((tuple(s), r) for s, r in G._cases())
    for (shape, regime), seeds in G.SEEDS.items():
        assert len(seeds) == (3 if shape in G.REGIME_SHAPES else 1) and len(set(seeds)) == len(seeds), (shape, regime)
    assert all(B * S > 1 for B, _, _, S in G.REGIME_SHAPES + G.OTHER_SHAPES)            # no single-row batch
    assert len(list(G._params())) == 2 * (len(R.REGIMES) * (3 + 5 + 5) + len(G.OTHER_REGIMES) * (3 + 3 + 3 + 5))


def _listed(shapes=None):
    for shape, regime in G._cases():
        if shapes is None or shape in shapes:
            for uniform in (True, False):
                yield pytest.param(shape, regime, uniform, id=f"{'x'.join(map(str, shape))}-{regime}-{'uniform' if uniform else 'table'}")


@pytest.mark.parametrize("shape,regime,uniform", list(_listed()))
def test_every_seed_meets_the_conditions(shape, regime, uniform):
    for seed in G.seeds_of(shape, regime):
        for training in (True, False):
            _, p64, _, e32, _, (ok, cond) = G.reference(shape, seed, regime, uniform, training)
            print(f"[frame_prep ref] {shape} {regime} seed {seed} training={training}: " + ", ".join(f"{v:.2e}" for v in cond))
            assert ok, cond
            assert min(e32.values()) > 0 and list(p64) == (["y", "dgamma", "dbeta", "batch_mean", "batch_var"] if training else ["y", "dgamma", "dbeta"])


def _ratios(shape, regime, uniform, seed, pivot):
    B, _, _, S = shape
    inp, p64, _, e32, _, _ = G.reference(shape, seed, regime, uniform, True)
    emu = R.emulated_parts(inp, S, uniform=uniform, pivot=pivot)
    return {n: R.part_figure(emu[n], p64[n], n, B) / max(8 * e32[n], 1e-6) for n in p64}


@pytest.mark.parametrize("shape,regime,uniform", list(_listed(G.REGIME_SHAPES)))
def test_the_bound_bites_on_the_raw_sums_and_the_shifted_sums_meet_it(shape, regime, uniform):
    for seed in G.seeds_of(shape, regime):
        raw, new = (_ratios(shape, regime, uniform, seed, pivot) for pivot in (None, "spread8"))
        for name, r in (("raw sums", raw), ("with shifted sums", new)):
            print(f"[frame_prep ref] {shape} {regime} {'uniform' if uniform else 'table'} seed {seed}: {name}, error / bound " +
                  ", ".join(f"{n} {v:.2f}" for n, v in r.items()))
        for part, regimes in BITES.items():
            if regime in regimes:
                assert raw[part] > 1, (seed, part, raw[part])
        if regime == "random":
            # The raw sums meet the bound without an offset -- on batch_var only where the one-frame clip is a minority of the batch.  At
            # (2, 40, 1024, 32) its 32 equal rows are HALF the batch: equal addends round the same way every time, columns reach
            # |mean| / std = 0.9 .. 1 there, and the raw sums stand AT the bound (1.02 emulated for one listed seed, 1.02 measured on the
            # GPU: DESIGN.md section 35).  There batch_var is held below twice the bound only: apart from the offset regimes, whose
            # least figure is 1.7.
            assert max(v for n, v in raw.items() if n != "batch_var") <= 1, (seed, raw)
            assert raw["batch_var"] <= (1 if shape[0] > 2 else 2), (seed, raw)
        # the form with the shifted sums: every part, every regime
        assert max(new.values()) <= 1, (seed, new)


def test_pivot_choices():
    """The pivots that were tried, on batch_var in the offset regimes: row 0 alone and the first eight rows (rows of one clip whenever
    S >= 8) leave some seed beyond the bound; eight rows spread over all B S rows leave none beyond 0.5.  The same for clip_offsets."""
    worst = {p: 0.0 for p in ("row0", "first8", "spread8")}
    for shape in G.REGIME_SHAPES:
        for regime in ("offset3", "offset10", "offset30"):
            for uniform in (True, False):
                for seed in G.seeds_of(shape, regime):
                    for p in worst:
                        worst[p] = max(worst[p], _ratios(shape, regime, uniform, seed, p)["batch_var"])
    print("[frame_prep ref] worst batch_var error / bound in the offset regimes: " + ", ".join(f"{p} {v:.2f}" for p, v in worst.items()))
    assert worst["row0"] > 1 and worst["first8"] > 1 and worst["spread8"] <= 0.5
    # every clip with its own column means: the first eight rows are rows of one clip and their mean is that clip's, not the batch's
    clips = {p: 0.0 for p in ("first8", "spread8")}
    for shape in G.REGIME_SHAPES:
        for uniform in (True, False):
            for seed in G.seeds_of(shape, "clip_offsets"):
                for p in clips:
                    clips[p] = max(clips[p], _ratios(shape, "clip_offsets", uniform, seed, p)["batch_var"])
    print("[frame_prep ref] worst batch_var error / bound in clip_offsets: " + ", ".join(f"{p} {v:.2f}" for p, v in clips.items()))
    assert clips["first8"] > 1 and clips["spread8"] <= 0.5
    assert R.pivot_rows(35, "spread8") == [0, 4, 8, 13, 17, 21, 26, 30] and R.pivot_rows(3, "spread8") == [0, 1, 2]
    assert R.pivot_rows(3, "first8") == [0, 1, 2] and R.pivot_rows(600, "spread8") == [0, 75, 150, 225, 300, 375, 450, 525]
