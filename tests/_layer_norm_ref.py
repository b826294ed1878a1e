"""Restatement of the residual layer norm of the encoders (transformer_utils.py:405-411, 450-454, 708-713) in plain torch on the CPU, written
from the formula of oracle/lpm_oracle.layer_norm and never from the package.  Every function computes in the dtype it is given: fp64 is the
reference, fp32 gives the evaluation error err32 the GPU bounds are built from.

    z = mask * mask_scale * act(a + bias) + r * r_scale;   mean = mean_e(z);  var = mean_e((z - mean)^2)   (e: all L F elements of an example)
    y = (z - mean) rsqrt(var + 1e-12) gamma + beta          (gamma, beta over F)

The moments are two-pass, as tf.nn.moments (and the oracle) forms them: the mean first, then the mean of the squared differences.
pair: y = LN2(LN1(relu(a + bias) + r) + r) with the SAME residual, the two layer norms at the end of the V1 encoder's feed-forward block.
Gradients come from autograd with the loss sum(y * upstream)."""
import torch

LN_EPS = 1e-12
REGIMES = ("random", "offset3", "offset10", "offset30", "scale_spread")
OFFSET = {"offset3": 3.0, "offset10": 10.0, "offset30": 30.0}
KEEP_PROBABILITY, MASK_SCALE = 0.1, 10.0

# form -> what z is made of
FORMS = {
    "plain": dict(),                                               # z = a: no residual, no bias
    "residual": dict(res=True),
    "bias_residual": dict(res=True, bias=True),
    "bias_relu_residual": dict(res=True, bias=True, relu=True),
    "row_scale": dict(res=True, row_scale=True),                    # the residual is raw rows times one factor per (example, row)
    "masked": dict(res=True, bias=True, relu=True, mask=True),      # a dropout between the dense layer and the norm
    "pair": dict(res=True, bias=True, relu=True, pair=True),
}
EXAMPLE_PARTS = ("y", "da", "dr", "da1", "dzy")                    # parts with an example axis: the error figure is taken per example


def layer_norm(z, gamma, beta):
    """Joint moments over every non-batch axis, two-pass; gamma / beta over the last axis."""
    red = tuple(range(1, z.dim()))
    mean = z.mean(dim=red, keepdim=True)
    var = ((z - mean) ** 2).mean(dim=red, keepdim=True)
    return (z - mean) * torch.rsqrt(var + LN_EPS) * gamma + beta


def pre_norm(a, r, bias, form, mask=None, r_scale=None):
    """z of a single layer norm (or of the first one of the pair); r is the residual AS IT IS ADDED (already times its row scale)."""
    f = FORMS[form]
    t = a
    if f.get("bias"):
        t = t + bias
    if f.get("relu"):
        t = torch.relu(t)
    if f.get("mask"):
        t = t * mask * MASK_SCALE
    if f.get("res"):
        t = t + r
    return t


def example_decades(B, span, low):
    """10^(span b / (B - 1) + low) per example (1 for a single example)."""
    if B == 1:
        return torch.ones(1, dtype=torch.float64)
    return 10.0 ** (span * torch.arange(B, dtype=torch.float64) / (B - 1) + low)


def make_inputs(B, L, F, seed, regime="random"):
    """-> dict of fp32 tensors (mask: bool): a, r [B, L, F], gamma, beta, gamma2, beta2, bias [F], r_scale [B L] in (0.5, 2), mask [B, L, F]
    (kept with probability 0.1), upstream [B, L, F] = N(0, 1) times 10^(6 b / (B - 1) - 3) for example b.
    random: a, r ~ N(0, 1).  offsetR: r = R + N(0, 1), so the mean / std of z is about R.  scale_spread: example b's a and r times
    10^(4 b / (B - 1) - 2), so rstd spans four decades over the batch."""
    assert regime in REGIMES
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(B, L, F, generator=g)
    r = torch.randn(B, L, F, generator=g)
    gamma, beta = 1 + 0.2 * torch.randn(F, generator=g), 0.1 * torch.randn(F, generator=g)
    bias = 0.3 * torch.randn(F, generator=g)
    up = torch.randn(B, L, F, generator=g) * example_decades(B, 6.0, -3.0).float().reshape(B, 1, 1)
    gamma2, beta2 = 1 + 0.2 * torch.randn(F, generator=g), 0.1 * torch.randn(F, generator=g)
    r_scale = 0.5 + 1.5 * torch.rand(B * L, generator=g)
    mask = torch.rand(B, L, F, generator=g) < KEEP_PROBABILITY
    if regime in OFFSET:
        r = r + OFFSET[regime]
    elif regime == "scale_spread":
        s = example_decades(B, 4.0, -2.0).float().reshape(B, 1, 1)
        a, r = a * s, r * s
    return dict(a=a, r=r, gamma=gamma, beta=beta, bias=bias, upstream=up, gamma2=gamma2, beta2=beta2, r_scale=r_scale, mask=mask)


def layer_norm_ref(inputs, dtype, form, upstream=None):
    """-> {part: tensor} evaluated in ``dtype`` on the CPU, gradients by autograd with the loss sum(y * upstream):
    y, da (no da for the pair), dr (forms with a residual; row_scale: with respect to the residual as it is added, r * r_scale), dgamma, dbeta,
    dbias (forms with a bias);  pair: y, da1 (gradient of a), dzy (gradient of the shared residual: both norms' shares), dgamma1, dbeta1,
    dgamma2, dbeta2, dbias."""
    f = FORMS[form]
    up = (inputs["upstream"] if upstream is None else upstream).to(dtype)

    def leaf(t):
        return t.detach().to(dtype).clone().requires_grad_(True)
    a, gamma, beta = leaf(inputs["a"]), leaf(inputs["gamma"]), leaf(inputs["beta"])
    leaves = dict(da=a, dgamma=gamma, dbeta=beta)
    r = bias = None
    if f.get("res"):
        r = inputs["r"].to(dtype)
        if f.get("row_scale"):
            r = r * inputs["r_scale"].to(dtype).reshape(r.shape[0], r.shape[1], 1)
        r = leaves["dr"] = leaf(r)
    if f.get("bias"):
        bias = leaves["dbias"] = leaf(inputs["bias"])
    y = layer_norm(pre_norm(a, r, bias, form, inputs["mask"].to(dtype)), gamma, beta)
    if f.get("pair"):
        gamma2, beta2 = leaf(inputs["gamma2"]), leaf(inputs["beta2"])
        y = layer_norm(y + r, gamma2, beta2)
        leaves = dict(da1=a, dzy=r, dgamma1=gamma, dbeta1=beta, dgamma2=gamma2, dbeta2=beta2, dbias=bias)
    names = list(leaves)
    grads = torch.autograd.grad((y * up).sum(), [leaves[n] for n in names])
    return dict(y=y.detach(), **dict(zip(names, grads)))


def figure(got, ref, part, B):
    """The error figure of one part: max |got - ref| / max |ref|, per example (the maximum over the B examples) for the parts with an
    example axis and over the tensor for the others.  Where the reference is identically zero (in an example): 0 if ``got`` is exactly
    zero there, inf otherwise -- a part whose fp64 value is identically zero must be exactly zero."""
    ref = ref.detach().double().cpu()
    got = got.detach().double().cpu().reshape(ref.shape)
    rows = B if part in EXAMPLE_PARTS else 1
    err = (got - ref).abs().reshape(rows, -1).max(1).values
    scale = ref.abs().reshape(rows, -1).max(1).values
    fig = torch.where(scale > 0, err / scale.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), err))
    return float(fig.max())


def moments64(inputs, form):
    """-> (mean, variance) in fp64, [B] each, of every layer norm's z of the form (one norm, or the pair's two: [2 B])."""
    d = {k: v.double() for k, v in inputs.items()}
    r = d["r"] * d["r_scale"].reshape(d["r"].shape[0], -1, 1) if FORMS[form].get("row_scale") else d["r"]
    zs = [pre_norm(d["a"], r, d["bias"], form, d["mask"])]
    if FORMS[form].get("pair"):
        zs.append(layer_norm(zs[0], d["gamma"], d["beta"]) + r)
    z = torch.cat([t.reshape(t.shape[0], -1) for t in zs])
    mean = z.mean(1)
    return mean, ((z - mean.unsqueeze(1)) ** 2).mean(1)


MIN_VARIANCE = 1e-6


def conditions(inputs, form, parts64, regime="random"):
    """The conditions a seed must meet, evaluated in fp64 -> (ok, values): in the offset regimes every example's |mean| / std of z (of both
    norms for the pair) within [0.5 R, 1.5 R]; every part's maximum > 0 (in every example for the parts with an example axis); every
    example's variance >= 1e-6.  values: (min |mean| / std, max |mean| / std, min variance, min over parts and examples of max |part|)."""
    B = inputs["a"].shape[0]
    mean, var = moments64(inputs, form)
    ratio = mean.abs() / var.clamp_min(1e-300).sqrt()
    ok = float(var.min()) >= MIN_VARIANCE
    if regime in OFFSET:
        R = OFFSET[regime]
        ok = ok and float(ratio.min()) >= 0.5 * R and float(ratio.max()) <= 1.5 * R
    least = min(float(v.abs().reshape(B if n in EXAMPLE_PARTS else 1, -1).max(1).values.min()) for n, v in parts64.items())
    ok = ok and least > 0
    return ok, (float(ratio.min()), float(ratio.max()), float(var.min()), least)
