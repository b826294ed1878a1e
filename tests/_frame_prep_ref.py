"""Restatement of the frame-prep family (csrc/frame_prep.hip) in plain torch on the CPU, written from the formulas of the reader's tail and
of oracle/lpm_oracle.py and never from the package.  Every function computes in the dtype it is given: fp64 is the reference, fp32 gives the
evaluation error err32 the GPU bounds are built from.

    uint8 frames:  x = u * range / 255 + range / 512 + min     (utils.Dequantize, range (2, -2));   frames at and past num_frames := 0;
                   x <- x rsqrt(max(sum_f x^2, 1e-12))          (train.py: tf.nn.l2_normalize over the feature axis)
    fp32 frames:   as they are
    rows = frames[b, index[b, j]]   (index: oracle.sample_uniform_frame_index, or a table);   y = input_bn(rows)   (tests/_netvlad_ref)

Gradients of gamma / beta come from autograd with the loss sum(y * upstream); clip b's upstream gradient is N(0, 1) x clip_decades(B)[b].

The two emulations at the end are NOT references: they restate in fp32, operation by operation, how frame_stats_kernel + the fold form the
batch statistics -- from the raw sums alone (the form before the shifted sums) and with the shifted sums beside them -- so that the host
test can show without a GPU that the bound separates the two."""
import torch

from oracle import lpm_oracle as O
from tests._netvlad_ref import BN_EPS, DECAY, L2_EPS, ONE_MINUS_DECAY, clip_decades, figure, gather_rows, input_bn  # noqa: F401

QUANT_MAX, QUANT_MIN = 2.0, -2.0
F32_REGIMES = ("random", "offset3", "offset10", "offset30", "mixed", "column_spread", "clip_offsets")
Q8_REGIMES = ("q8_random", "q8_narrow")
REGIMES = F32_REGIMES + Q8_REGIMES
OFFSET = {"offset3": 3.0, "offset10": 10.0, "offset30": 30.0}
Q8_NARROW_LEVELS = 3.0
CLIP_WITHIN = 0.05                   # clip_offsets: within-clip std / between-clip spread
PARTS_TRAINING = ("y", "batch_mean", "batch_var", "dgamma", "dbeta")
PARTS_EVAL = ("y", "dgamma", "dbeta")
FP_ROWS = 32                         # gathered rows per statistics block of frame_stats_kernel
PIVOT_ROWS = 8
FOLD_TAKE = 4.0                      # lpm_frame_bn_fold takes the shifted sums where FOLD_TAKE mean^2 > var


# ---- the formulas ----
def dequantize(q, dtype):
    """utils.Dequantize: q * range / 255 + range / 512 + min."""
    rng = QUANT_MAX - QUANT_MIN
    return q.to(dtype) * (rng / 255.0) + (rng / 512.0 + QUANT_MIN)


def zero_padding(x, num_frames):
    """x [B, MF, F] with the frames at and past num_frames[b] set to zero (the reader pads after dequantising)."""
    keep = torch.arange(x.shape[1]).unsqueeze(0) < num_frames.reshape(-1, 1)
    return x * keep.unsqueeze(-1).to(x.dtype)


def l2_normalize_rows(x):
    return x * torch.rsqrt(torch.clamp((x * x).sum(-1, keepdim=True), min=L2_EPS))


def dequantize_l2_normalize(q, num_frames, dtype):
    return l2_normalize_rows(zero_padding(dequantize(q, dtype), num_frames))


def uniform_index(num_frames, S):
    return torch.from_numpy(O.sample_uniform_frame_index(num_frames.numpy(), S)).long()


def prepared_frames(inputs, dtype):
    """The frames the gather reads: the fp32 frames as they are, or the dequantised, zero-padded, L2-normalised uint8 frames."""
    if "q" in inputs:
        return dequantize_l2_normalize(inputs["q"], inputs["nf"], dtype)
    return inputs["frames"].to(dtype)


def sampled_rows(inputs, dtype, uniform, S):
    index = uniform_index(inputs["nf"], S) if uniform else inputs["random_index"]
    return gather_rows(prepared_frames(inputs, dtype), index)


# ---- inputs ----
def make_inputs(B, MF, F, S, seed, regime="random"):
    """-> dict: frames fp32 [B, MF, F] (the fp32 regimes) or q uint8 [B, MF, F] (q8_*), nf int64 [B] (ragged; nf[0] = MF, nf[-1] = 1 when
    B > 1), gamma, beta [F], up [B S, F] (N(0, 1) x the clip's decade), random_index int64 [B, S] (uniform below nf, with a repeated row
    and the last valid frame of every clip that has room for them), noise_mean, noise_var [F] for the eval-mode moving statistics.
    random: column c is sd_c N(0, 1) + 0.3 N(0, 1), sd_c in (0.5, 1.5) (the distribution of tests/test_gpu_input_bn_bounds.py).
    offsetR: column c is sd_c N(0, 1) + R sd_c sign_c.  mixed: every other column as in offset30, the rest as in random.
    column_spread: sd_c = 10^(4 c / (F - 1) - 4), column c is sd_c (N(0, 1) + 0.3 N(0, 1)): the variance runs from 1e-8 to 1.
    clip_offsets: frame (b, t) of column c is spread_c (m_bc + 0.05 N(0, 1)), one m_bc ~ N(0, 1) per clip and column.
    q8_random: uniform bytes.  q8_narrow: column c has a centre in [40, 216), the bytes are round(centre + 3 N(0, 1))."""
    assert regime in REGIMES
    g = torch.Generator().manual_seed(seed)
    n = torch.randn(B, MF, F, generator=g)
    sd = 0.5 + torch.rand(F, generator=g)
    m = 0.3 * torch.randn(F, generator=g)
    nf = torch.randint(2, MF + 1, (B,), generator=g) if MF > 1 else torch.ones(B, dtype=torch.long)
    nf[0] = MF
    if B > 1:
        nf[-1] = 1                                                 # a full clip and a clip of one frame
    gamma, beta = 1 + 0.3 * torch.randn(F, generator=g), 0.2 * torch.randn(F, generator=g)
    up = torch.randn(B, S * F, generator=g) * clip_decades(B).float().unsqueeze(1)
    random_index = (torch.rand(B, S, generator=g) * nf.unsqueeze(1)).long().clamp_max(MF - 1)
    if S >= 3:
        random_index[:, -1] = nf - 1                               # the last valid frame
        random_index[:, 1] = random_index[:, 0]                    # a repeated row
    noise_mean, noise_var = torch.randn(F, generator=g), torch.rand(F, generator=g)
    sign = torch.where(torch.rand(F, generator=g) < 0.5, -1.0, 1.0)
    clip_mean = torch.randn(B, 1, F, generator=g)
    centre = 40.0 + 176.0 * torch.rand(F, generator=g)
    out = dict(nf=nf, gamma=gamma, beta=beta, up=up.reshape(B * S, F), random_index=random_index, noise_mean=noise_mean,
               noise_var=noise_var)
    if regime == "q8_random":
        out["q"] = torch.randint(0, 256, (B, MF, F), generator=g).to(torch.uint8)
        return out
    if regime == "q8_narrow":
        out["q"] = torch.round(centre + Q8_NARROW_LEVELS * n).clamp(0, 255).to(torch.uint8)
        return out
    x = sd * n + m
    if regime in OFFSET:
        x = sd * n + OFFSET[regime] * sd * sign
    elif regime == "mixed":
        x = torch.where(torch.arange(F) % 2 == 0, sd * n + OFFSET["offset30"] * sd * sign, x)
    elif regime == "column_spread":
        sd = (10.0 ** (4.0 * torch.arange(F, dtype=torch.float64) / max(F - 1, 1) - 4.0)).float()
        x = sd * (n + m)
    elif regime == "clip_offsets":
        x = sd * (clip_mean + CLIP_WITHIN * n)
    out["frames"] = x.contiguous()
    return out


def moving_for_eval(inputs, uniform, S):
    """The eval-mode moving statistics, fp32: the true moments of the sampled rows plus noise -- mean + 0.1 std N(0, 1), variance x (0.5 .. 1.5)."""
    rows = sampled_rows(inputs, torch.float64, uniform, S)
    mean = rows.mean(0)
    var = ((rows - mean) ** 2).mean(0)
    return ((mean + 0.1 * var.sqrt() * inputs["noise_mean"].double()).float(), (var * (0.5 + inputs["noise_var"].double())).float())


def frame_prep_ref(inputs, dtype, S, *, uniform=True, training=True, moving=None):
    """-> {part: tensor} in ``dtype``: y [B S, F], dgamma, dbeta and, in training mode, batch_mean and the unbiased batch_var."""
    rows = sampled_rows(inputs, dtype, uniform, S)
    gamma, beta = (inputs[k].detach().to(dtype).clone().requires_grad_(True) for k in ("gamma", "beta"))
    y, mean, uvar = input_bn(rows, gamma, beta, training=training, moving=None if training else tuple(t.to(dtype) for t in moving))
    dgamma, dbeta = torch.autograd.grad((y * inputs["up"].to(dtype)).sum(), [gamma, beta])
    parts = dict(y=y.detach(), dgamma=dgamma, dbeta=dbeta)
    if training:
        parts.update(batch_mean=mean.detach(), batch_var=uvar.detach())
    return parts


# ---- figures ----
def part_figure(got, ref, name, B):
    """y [B S, F]: the larger of the per-clip figure (max over clips of max |error| / max |fp64| in the clip) and the same quotient per
    column; every other part: max |error| / max |fp64| over the tensor (tests/_netvlad_ref.figure)."""
    if name != "y":
        return figure(got, ref, name, B)
    ref = ref.detach().double().cpu()
    got = got.detach().double().cpu().reshape(ref.shape)
    return max(figure(got, ref, "out", B), figure(got.t().contiguous(), ref.t().contiguous(), "out", ref.shape[1]))


def column_ratio(rows64):
    """|mean| / std per column of the sampled rows, fp64 (std floored at 1e-300)."""
    mean = rows64.mean(0)
    var = ((rows64 - mean) ** 2).mean(0)
    return mean.abs() / var.sqrt().clamp_min(1e-300), var


def conditions(inputs, S, parts64, parts32, *, uniform=True, regime="random"):
    """What seed selection rests on, evaluated on the fp64 restatement -> (ok, values), values = (min err32 over the parts, least squared
    norm of a sampled, unpadded row before the normalisation (inf for fp32 frames), median and maximum over the held columns of
    |mean| / std, least column variance).  ok: err32 > 0 for every part; no sampled, unpadded row has a zero norm, and no sampled row is
    padding; offsetR: the median |mean| / std of the columns is at least 0.5 R and no column is below 0.25 R (mixed: the even columns
    with R = 30, and the odd ones' median stays below 1.5); q8_narrow: the median is at least 10; no column has zero variance."""
    B = inputs["nf"].shape[0]
    e32 = min(part_figure(parts32[n], parts64[n], n, B) for n in parts64)
    ok = e32 > 0
    index = uniform_index(inputs["nf"], S) if uniform else inputs["random_index"]
    ok = ok and bool((index < inputs["nf"].unsqueeze(1)).all())
    least_norm = float("inf")
    if "q" in inputs:
        raw = gather_rows(zero_padding(dequantize(inputs["q"], torch.float64), inputs["nf"]), index)
        least_norm = float((raw * raw).sum(1).min())
        ok = ok and least_norm > 1e-6
    ratio, var = column_ratio(sampled_rows(inputs, torch.float64, uniform, S))
    held = ratio[0::2] if regime == "mixed" else ratio
    if regime in OFFSET or regime == "mixed":
        R = OFFSET.get(regime, OFFSET["offset30"])
        ok = ok and float(held.median()) >= 0.5 * R and float(held.min()) >= 0.25 * R
        if regime == "mixed":
            ok = ok and float(ratio[1::2].median()) <= 1.5
    elif regime == "q8_narrow":
        ok = ok and float(held.median()) >= 10.0
    ok = ok and float(var.min()) > 0
    return bool(ok), (e32, least_norm, float(held.median()), float(held.max()), float(var.min()))


# ---- the kernels' statistics, emulated in fp32 (not references) ----
def _fma32(a, b, c):
    """fp32 fma(a, b, c): the product of two fp32 values is exact in fp64."""
    return (a.double() * b.double() + c.double()).float()


def pivot_rows(rows, choice):
    """The gathered rows whose mean is the pivot.  spread8: rows (u n) // p, u < p = min(n, 8) -- spread evenly over all B S rows;
    first8: the first min(n, 8) rows (rows of ONE clip whenever S >= 8);  row0: the first row alone."""
    p = min(rows, PIVOT_ROWS)
    if choice == "spread8":
        return [(u * rows) // p for u in range(p)]
    if choice == "first8":
        return list(range(p))
    assert choice == "row0"
    return [0]


def emulate_stats(rows32, gamma, beta, pivot=None):
    """frame_stats_kernel + the fold on the fp32 rows [n, F]: per 32-row block, row by row, s += v and q = fma(v, v, q) in fp32; the blocks
    folded in fp64, mean = s / n, var = q / n - mean^2.  pivot = None: that is all (the form before the shifted sums).  pivot = a choice
    of pivot_rows: beside them s' += v - K and q' = fma(v - K, v - K, q'), K = fp32 mean of the pivot rows summed in order; the fold
    also forms mean = K + s' / n, var = q' / n - (s' / n)^2 and takes it where FOLD_TAKE x that mean^2 > that var, the raw form elsewhere; where it
    is taken the apply pass centres the frames on the fp32 mean before scale and shift.
    -> dict(batch_mean, batch_var (unbiased; both as read back from zero moving statistics), mean, var (fp32, biased: what the backward
    reads), scale, shift, y)"""
    n, F = rows32.shape
    K = None
    if pivot is not None:
        pr = pivot_rows(n, pivot)
        K = torch.zeros(F)
        for r in pr:
            K = K + rows32[r]
        K = K * torch.tensor(1.0 / len(pr), dtype=torch.float32)
    s64, q64, ss64, sq64 = (torch.zeros(F, dtype=torch.float64) for _ in range(4))
    for r0 in range(0, n, FP_ROWS):
        s, q, ss, sq = (torch.zeros(F) for _ in range(4))
        for r in range(r0, min(n, r0 + FP_ROWS)):
            v = rows32[r]
            s = s + v
            q = _fma32(v, v, q)
            if K is not None:
                d = v - K
                ss = ss + d
                sq = _fma32(d, d, sq)
        s64, q64, ss64, sq64 = s64 + s.double(), q64 + q.double(), ss64 + ss.double(), sq64 + sq.double()
    mu = s64 / n
    vr = (q64 / n - mu * mu).clamp_min(0)
    take = torch.zeros(F, dtype=torch.bool)
    if K is not None:
        dm = ss64 / n
        mu_s = K.double() + dm
        vr_s = (sq64 / n - dm * dm).clamp_min(0)
        take = FOLD_TAKE * mu_s * mu_s > vr_s
        mu, vr = torch.where(take, mu_s, mu), torch.where(take, vr_s, vr)
    unbias = n / (n - 1) if n > 1 else 1.0
    mean32, var32 = mu.float(), vr.float()
    scale = gamma * (1.0 / torch.sqrt(vr + BN_EPS)).float()
    # the apply pass: y = (x - centre) scale + shift, centre = the fp32 mean where the shifted sums were taken, 0 elsewhere
    centre = torch.where(take, mean32, torch.zeros(F))
    shift = torch.where(take, (beta.double() - (mu - mean32.double()) * scale.double()).float(), _fma32(-mean32, scale, beta))
    y = _fma32(rows32 - centre, scale.expand_as(rows32), shift.expand_as(rows32))
    # the moving statistics from zero, moving = 0 * decay + batch * (1.f - decay) in fp32, read back as the GPU test reads them
    blend = torch.tensor(ONE_MINUS_DECAY, dtype=torch.float32)
    batch_mean, batch_var = ((t.float() * blend).double() / ONE_MINUS_DECAY for t in (mu, vr * unbias))
    return dict(batch_mean=batch_mean, batch_var=batch_var, mean=mean32, var=var32, scale=scale, shift=shift, y=y)


def emulate_backward(rows32, up32, mean32, var32, centred=False):
    """frame_bn_bwd_partial_kernel + frame_bn_bwd_reduce_kernel: per 32-row block s += dy and q = fma(dy, x - c0, q) in fp32, folded in
    fp64, dgamma = rstd (q - (mean - c0) s) with rstd = 1 / sqrt(var + eps) in fp64 from the fp32 mean and var; c0 = 0 (the form before
    the centre), or with ``centred`` the fp32 mean where mean^2 > var.  -> (dgamma, dbeta)"""
    n, F = rows32.shape
    c0 = torch.where(mean32 * mean32 > var32, mean32, torch.zeros(F)) if centred else torch.zeros(F)
    s64, q64 = torch.zeros(F, dtype=torch.float64), torch.zeros(F, dtype=torch.float64)
    for r0 in range(0, n, FP_ROWS):
        s, q = torch.zeros(F), torch.zeros(F)
        for r in range(r0, min(n, r0 + FP_ROWS)):
            s = s + up32[r]
            q = _fma32(up32[r], rows32[r] - c0, q)
        s64, q64 = s64 + s.double(), q64 + q.double()
    rstd = 1.0 / torch.sqrt(var32.double() + BN_EPS)
    return (rstd * (q64 - (mean32.double() - c0.double()) * s64)).float(), s64.float()


def emulated_parts(inputs, S, *, uniform=True, pivot=None):
    """The training-mode parts as the kernels form them, on the fp32 rows of the fp32 restatement."""
    rows32 = sampled_rows(inputs, torch.float32, uniform, S)
    st = emulate_stats(rows32, inputs["gamma"], inputs["beta"], pivot)
    dgamma, dbeta = emulate_backward(rows32, inputs["up"], st["mean"], st["var"], centred=pivot is not None)
    return dict(y=st["y"], batch_mean=st["batch_mean"], batch_var=st["batch_var"], dgamma=dgamma, dbeta=dbeta)
