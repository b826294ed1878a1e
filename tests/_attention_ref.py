"""Restatement of the attention core K4 in plain torch on the CPU, written from transformer_utils.py:564-581 (MultiHeadAttention: split
heads, q *= depth^-0.5, softmax(q k^T) v, combine heads) and :652-661 (MultiHeadAttentionBN: slim.batch_norm over the rank-4 logits
[B, h, query, key] -- its channel is the KEY position, its statistics run over (B, h, query) -- then softmax . v), never from the kernels.
Every function computes in the dtype of its inputs: fp64 is the reference, fp32 gives the evaluation error err32 the GPU bounds are built
from.

    s = q k^T per (batch, head);  z = (s - mean_j) rsqrt(var_j + 1e-3) gamma_j + beta_j  (training: batch statistics, biased variance; eval:
    the moving ones)  or  z = depth^-0.5 s;  out = softmax_j(z) v.

``mm`` is the product used for q k^T and P v and, through autograd, for every product of the backward.  tests/_netvlad_ref.mm3 is the
split-operand model of "bf16x3" (hi + lo bf16 per operand, lo x lo dropped), proved in tests/test_netvlad_ref_host.py.

The moving statistics blend as in tests/_netvlad_ref (ONE_MINUS_DECAY): from zero moving statistics the op leaves ONE_MINUS_DECAY x (batch
mean, UNBIASED batch variance), which is what the parts batch_mean / batch_var are."""
import torch

from tests._netvlad_ref import DECAY, ONE_MINUS_DECAY, clip_decades, mm3  # noqa: F401  (DECAY / ONE_MINUS_DECAY: for the GPU file)

BN_EPS = 1e-3
REGIMES = ("random", "offset", "saturated", "static", "decades")
# the regimes' constants (see make_inputs)
RANDOM_SCALE = 0.5
OFFSET_LEVELS = {"offset": (1.0, 0.1), "offset_low": (1.0, 0.3)}     # (a, sigma): q = a c + sigma n, k = a c + sigma n'
OFFSET_MIN_RATIO = {"offset": 100.0, "offset_low": 10.0}              # the worst column's mean^2 / var in fp64 is at least this
SATURATED_GAMMA, SATURATED_Q = 30.0, 128.0
STATIC_KEY, STATIC_NOISE = 0.01, 1e-3                                 # key rows of a clip: STATIC_KEY N(0, 1) + U(-1/2, 1/2) STATIC_NOISE
CLIP_PARTS = ("out", "dq", "dk", "dv")                               # parts with a clip axis: the error figure is taken per clip
WRONG = ("eps", "unbiased", "stats_per_head", "scale_twice", "raw_sum_variance")


# ---- the formulas ----
def split_heads(x, h):
    """[B, L, h d] -> [B h, L, d]"""
    B, L, F = x.shape
    return x.reshape(B, L, h, F // h).transpose(1, 2).reshape(B * h, L, F // h)


def combine_heads(x, h):
    """[B h, L, d] -> [B, L, h d]"""
    Bh, L, d = x.shape
    return x.reshape(Bh // h, h, L, d).transpose(1, 2).reshape(Bh // h, L, h * d)


def moments(s, *, unbiased=False, stats_per_head=False):
    """s [B h, query, key] -> (mean, the variance that normalises, unbiased variance), over (B h, query) per key column -- or, WRONG, over
    the query axis of each (batch, head) alone."""
    dims = (1,) if stats_per_head else (0, 1)
    n = s.shape[1] * (1 if stats_per_head else s.shape[0])
    mean = s.mean(dims, keepdim=True)
    var = ((s - mean) ** 2).mean(dims, keepdim=True)
    uvar = var * (n / max(n - 1, 1))
    return mean, (uvar if unbiased else var), uvar


def raw_sum_moments(s):
    """The WRONG statistics of the raw-sum form: per (batch, head) the column sums of s and s^2 over the queries in fp32, folded in fp64,
    var = sum s^2 / n - mean^2.  -> (mean, biased variance) [1, 1, key] in fp64."""
    s32 = s.detach().float()
    n = s.shape[0] * s.shape[1]
    mean = s32.sum(1).double().sum(0) / n
    var = ((s32 * s32).sum(1).double().sum(0) / n - mean * mean).clamp_min(0)
    return mean.reshape(1, 1, -1), var.reshape(1, 1, -1)


def _mfma_gram(x):
    """sum_q x_q x_q^T over the rows of x [G, L, d] as the exact-fp32 matrix pipe accumulates it: four rows per step, fp32 accumulator."""
    G, L, d = x.shape
    pad = (-L) % 4
    if pad:
        x = torch.cat([x, x.new_zeros(G, pad, d)], 1)
    acc = x.new_zeros(G, d, d)
    for i in range(0, x.shape[1], 4):
        blk = x[:, i:i + 4]
        acc = acc + blk.transpose(1, 2) @ blk
    return acc


def quad_form_partials(qh, kh, pivot):
    """The statistics kernel's arithmetic, emulated in fp32: per (batch, head) G = sum_q u u^T (the matrix pipe, fp32 accumulator),
    S = sum_q u, then per key  sum_q (u . k_j) = k_j . S  and  sum_q (u . k_j)^2 = k_j^T G k_j.  pivot False: u = q, the raw sums.
    pivot True: u = q - q_0 (the (batch, head)'s first query row), the sums about the pivot p_j = k_j . q_0.
    -> (sum [G, key], sum of squares [G, key], pivot [G, key] or None), fp32."""
    q32, k32 = qh.detach().float(), kh.detach().float()
    p = None
    if pivot:
        q0 = q32[:, :1]
        p = (k32 @ q0.transpose(1, 2)).squeeze(-1)
        q32 = q32 - q0
    gram = _mfma_gram(q32)
    ssum = q32.sum(1, keepdim=True)
    return (k32 @ ssum.transpose(1, 2)).squeeze(-1), ((k32 @ gram) * k32).sum(-1), p


def kernel_moments(qh, kh, form, take=1.0):
    """The statistics of the kernels' forms, folded in fp64 -> (mean, biased variance) [1, 1, key] in fp64.
    "quad_raw": the raw sums alone (what the op did before the shifted sums).  "quad_taken": the raw sums where take mean^2 <= var, as
    the raw sums give the two, and the sums about the per-(batch, head) pivots elsewhere: with a = sum (s - p), b = sum (s - p)^2 over
    the n queries of a group, sum s = a + n p and sum s^2 = b + 2 p a + n p^2, formed in fp64 (every product of two fp32 numbers is exact
    there)."""
    n_q = qh.shape[1]
    n = qh.shape[0] * n_q
    a, b, _ = quad_form_partials(qh, kh, False)
    mean = a.double().sum(0) / n
    var = (b.double().sum(0) / n - mean * mean).clamp_min(0)
    if form == "quad_taken":
        a, b, p = (t.double() for t in quad_form_partials(qh, kh, True))
        mean_s = (a + n_q * p).sum(0) / n
        var_s = ((b + 2 * p * a + n_q * p * p).sum(0) / n - mean_s * mean_s).clamp_min(0)
        taken = take * mean * mean > var                # (the raw moments decide: the fold reads the pivoted sums only where they say so)
        mean, var = torch.where(taken, mean_s, mean), torch.where(taken, var_s, var)
    else:
        assert form == "quad_raw"
    return mean.reshape(1, 1, -1), var.reshape(1, 1, -1)


def attention(q, k, v, h, mm=torch.matmul, *, bn=None, training=True, moving=None, eps=BN_EPS, unbiased=False, stats_per_head=False,
              scale_twice=False, raw_sum_variance=False, statistics=None):
    """q, k, v [B, L, h d] -> (out [B, L, h d], batch mean, unbiased batch variance [L]; None, None without training-mode batch norm).
    bn = (gamma, beta) [L] or None.  eps, unbiased, stats_per_head, scale_twice, raw_sum_variance: the host test's deliberately WRONG
    restatements.  statistics: None, or "quad_raw" / "quad_taken" -- the values of (mean, variance) replaced by kernel_moments' (the
    gradient still flows through the exact ones), as raw_sum_variance does with raw_sum_moments."""
    d = q.shape[-1] // h
    qh, kh, vh = (split_heads(t, h) for t in (q, k, v))
    mean = uvar = None
    if bn is None:
        qh = qh * d ** -0.5
        if scale_twice:
            qh = qh * d ** -0.5
        z = mm(qh, kh.transpose(1, 2).contiguous())
    else:
        s = mm(qh, kh.transpose(1, 2).contiguous())
        gamma, beta = bn
        if training:
            mean, var, uvar = moments(s, unbiased=unbiased, stats_per_head=stats_per_head)
            if raw_sum_variance or statistics:
                m_w, v_w = raw_sum_moments(s) if raw_sum_variance else kernel_moments(qh, kh, statistics)
                n = s.shape[0] * s.shape[1]
                mean = mean + (m_w.to(s.dtype) - mean).detach()
                var = var + (v_w.to(s.dtype) - var).detach()
                uvar = var * (n / max(n - 1, 1))
        else:
            mean, var = (m.reshape(1, 1, -1) for m in moving)
        z = (s - mean) * torch.rsqrt(var + eps) * gamma + beta
        if not training or stats_per_head:
            mean = uvar = None
    out = combine_heads(mm(torch.softmax(z, -1), vh), h)
    if mean is not None:
        mean, uvar = mean.reshape(-1), uvar.reshape(-1)
    return out, mean, uvar


# ---- inputs ----
def make_inputs(B, L, h, d, seed, regime="random"):
    """-> dict of fp32 tensors: q, k, v [B, L, h d], gamma, beta [L], moving = (mean, variance) [L] for eval mode, upstream [B, L, h d].
    random: q, k, v = 0.5 N(0, 1), gamma = 1 + 0.3 N, beta = 0.2 N, upstream N(0, 1).
    offset / offset_low: q = a c + sigma n, k = a c + sigma n' with ONE vector c [d] ~ N(0, 1) shared by all heads and clips (what the
      bias of the q/k/v projection produces), (a, sigma) = OFFSET_LEVELS[regime].
    saturated: gamma times SATURATED_GAMMA for the logits_bn form; the plain form multiplies q by SATURATED_Q (inputs["q_plain"]).
    static: the key rows of a clip are STATIC_KEY N(0, 1) (one row per clip) + STATIC_NOISE U(-1/2, 1/2): equal up to 1e-3.
    decades: the upstream gradient of clip b times 10^(6 b / (B - 1) - 3).
    Eval mode's moving statistics: (0.1 N, 1 + 0.2 U) in random; elsewhere the GPU file and the host test put the fp64 batch statistics
    there (batch_statistics)."""
    assert regime in REGIMES or regime in OFFSET_LEVELS
    g = torch.Generator().manual_seed(seed)
    F = h * d
    q, k, v = (RANDOM_SCALE * torch.randn(B, L, F, generator=g) for _ in range(3))
    gamma = 1 + 0.3 * torch.randn(L, generator=g)
    beta = 0.2 * torch.randn(L, generator=g)
    up = torch.randn(B, L, F, generator=g)
    moving = (0.1 * torch.randn(L, generator=g), 1 + 0.2 * torch.rand(L, generator=g))
    c = torch.randn(d, generator=g).repeat(h)
    key_row = torch.randn(B, 1, F, generator=g)
    key_noise = torch.rand(B, L, F, generator=g) - 0.5
    if regime in OFFSET_LEVELS:
        a, sigma = OFFSET_LEVELS[regime]
        q, k = a * c + sigma * q / RANDOM_SCALE, a * c + sigma * k / RANDOM_SCALE
    elif regime == "static":
        k = STATIC_KEY * key_row + STATIC_NOISE * key_noise
    elif regime == "decades":
        up = up * clip_decades(B).float().reshape(B, 1, 1)
    inputs = dict(q=q, k=k, v=v, gamma=gamma, beta=beta, moving=moving, upstream=up)
    if regime == "saturated":
        inputs["gamma"] = gamma * SATURATED_GAMMA
        inputs["q_plain"] = q * SATURATED_Q
    return inputs


def batch_statistics(inputs, h):
    """-> (mean, BIASED variance) [L] of the logits in fp64: eval mode's moving statistics outside the random regime."""
    s = split_heads(inputs["q"].double(), h) @ split_heads(inputs["k"].double(), h).transpose(1, 2)
    mean, var, _ = moments(s)
    return mean.reshape(-1), var.reshape(-1)


def values_and_grads(inputs, dtype, mm=torch.matmul, *, h, bn, training=True, upstream=None, **wrong):
    """-> {part: tensor} evaluated in ``dtype`` on the CPU, gradients by autograd with the loss sum(out * upstream): out, dq, dk, dv;
    with bn dgamma, dbeta; with bn in training mode batch_mean, batch_var (the unbiased variance).  ``wrong``: see attention()."""
    up = (inputs["upstream"] if upstream is None else upstream).to(dtype)

    def leaf(name):
        return inputs[name].detach().to(dtype).clone().requires_grad_(True)
    leaves = dict(dq=leaf("q_plain" if (not bn and "q_plain" in inputs) else "q"), dk=leaf("k"), dv=leaf("v"))
    if bn:
        leaves.update(dgamma=leaf("gamma"), dbeta=leaf("beta"))
    out, mean, uvar = attention(leaves["dq"], leaves["dk"], leaves["dv"], h, mm, bn=(leaves["dgamma"], leaves["dbeta"]) if bn else None,
                                training=training, moving=tuple(m.to(dtype) for m in inputs["moving"]), **wrong)
    names = list(leaves)
    grads = torch.autograd.grad((out * up).sum(), [leaves[n] for n in names])
    parts = dict(out=out.detach(), **dict(zip(names, grads)))
    if mean is not None:
        parts.update(batch_mean=mean.detach(), batch_var=uvar.detach())
    return parts


def figure(got, ref, name, B):
    """The error figure of one part: max |got - ref| / max |ref|, per clip (the maximum over the B clips) for the parts with a clip axis
    and over the tensor for the others.  Where the reference is identically zero (in a clip): 0 if ``got`` is exactly zero there, inf
    otherwise -- a part whose fp64 value is identically zero must be exactly zero."""
    ref = ref.detach().double().cpu()
    got = got.detach().double().cpu().reshape(ref.shape)
    rows = B if name in CLIP_PARTS else 1
    err = (got - ref).abs().reshape(rows, -1).max(1).values
    scale = ref.abs().reshape(rows, -1).max(1).values
    fig = torch.where(scale > 0, err / scale.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), err))
    return float(fig.max())


def conditions(inputs, h, regime, *, bn):
    """The condition of the regime, evaluated on the fp64 restatement -> (ok, value).
    offset / offset_low: the worst column's mean^2 / var is at least OFFSET_MIN_RATIO (value: that ratio).
    saturated: at least half the query rows have a largest probability above 0.99 and no row of out is non-finite (value: the fraction).
    static: the batch variance is below BN_EPS in every column (value: the largest).  random, decades: nothing (value 0)."""
    d = {n: t.double() for n, t in inputs.items() if torch.is_tensor(t)}
    mean, var = batch_statistics(inputs, h)
    if regime in OFFSET_LEVELS:
        ratio = float((mean * mean / var).max())
        return ratio >= OFFSET_MIN_RATIO[regime], ratio
    if regime == "static":
        return float(var.max()) < BN_EPS, float(var.max())
    if regime == "saturated":
        F = d["q"].shape[-1]
        if bn:
            s = split_heads(d["q"], h) @ split_heads(d["k"], h).transpose(1, 2)
            z = (s - mean) * torch.rsqrt(var + BN_EPS) * d["gamma"] + d["beta"]
        else:
            z = (F // h) ** -0.5 * split_heads(d["q_plain"], h) @ split_heads(d["k"], h).transpose(1, 2)
        p = torch.softmax(z, -1)
        frac = float(p.max(-1).values.gt(0.99).double().mean())
        return frac >= 0.5 and bool(torch.isfinite(p @ split_heads(d["v"], h)).all()), frac
    return True, 0.0
