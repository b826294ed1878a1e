"""Restatement of the training-mode batch norm (slim.batch_norm: frame_level_models.py:2321-2368, transformer_utils.py:666, 741-760) in plain
torch on the CPU, written from the formula of oracle/lpm_oracle.batch_norm and never from the package.  Every function computes in the dtype
it is given: fp64 is the reference, fp32 gives the evaluation error err32 the GPU bounds are built from.

    a = act(x + bias)   (bias and ReLU optional);   mean = mean_rows(a);  var = mean_rows((a - mean)^2)        (eps = 1e-3, two-pass)
    y = (a - mean) rsqrt(var + eps) gamma + beta;   the bn_small tails: act 0 nothing, act 1 clamp(y, 0, 6), act 2 mul * sigmoid(y)
    moving statistics left from zero: ONE_MINUS_DECAY x (mean, biased or unbiased var)   (tests/_netvlad_ref.ONE_MINUS_DECAY)

Gradients come from autograd with the loss sum(y * upstream).  The rows are the B x L rows of B examples; example b's upstream gradient is
N(0, 1) x 10^(6 b / (B - 1) - 3)."""
import torch

from tests._netvlad_ref import ONE_MINUS_DECAY

BN_EPS = 1e-3
REGIMES = ("random", "offset3", "offset10", "offset30", "mixed_offset", "column_spread", "dead_relu")
OFFSET = {"offset3": 3.0, "offset10": 10.0, "offset30": 30.0}
ROW_PARTS = ("y", "dx", "dmul")                       # parts with a row axis: the figure is taken per example and per column
MIN_ACT1_DISTANCE = 1e-5
DEAD_BIAS = -8.0


def example_decades(B, span, low):
    """10^(span b / (B - 1) + low) per example (1 for a single example)."""
    if B == 1:
        return torch.ones(1, dtype=torch.float64)
    return 10.0 ** (span * torch.arange(B, dtype=torch.float64) / (B - 1) + low)


def dead_columns(C):
    return torch.arange(0, C, 8)


def near_dead_columns(C):
    """-> (columns, positive rows wanted: 1 and 2 in turn)"""
    cols = torch.arange(4, C, 8)
    return cols, 1 + (torch.arange(len(cols)) % 2)


def make_inputs(B, L, C, seed, regime="random"):
    """-> dict of fp32 tensors: x, upstream, mul [B, L, C]; gamma, beta, bias [C].
    random: column c is std_c x N(0, 1) + m_c with std_c in (0.5, 1.5) and one m_c = 0.3 N(0, 1) per column.
    offsetR: column c is std_c x (N(0, 1) + R), so mean / std is about R in every column.
    mixed_offset: the even columns as in offset30, the odd ones as in random.
    column_spread: std_c = 10^(4 c / (C - 1) - 2) and column c is std_c x (N(0, 1) + m_c): the variance runs from 1e-4, far below eps, to 1e4.
    dead_relu (the bias + ReLU forms): x as in random; bias -8 on columns 0, 8, 16, ... (relu(x + bias) is identically 0 there) and, on
    columns 4, 12, 20, ..., minus the midpoint between the k-th and (k + 1)-th largest x of the column, k = 1, 2 in turn (exactly k rows
    are positive).  bias is 0.3 N(0, 1) elsewhere and in every other regime."""
    assert regime in REGIMES
    g = torch.Generator().manual_seed(seed)
    M = B * L
    n = torch.randn(M, C, generator=g)
    std = 0.5 + torch.rand(C, generator=g)
    m = 0.3 * torch.randn(C, generator=g)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    bias = 0.3 * torch.randn(C, generator=g)
    up = torch.randn(B, L, C, generator=g) * example_decades(B, 6.0, -3.0).float().reshape(B, 1, 1)
    mul = torch.randn(B, L, C, generator=g)
    x = std * n + m
    if regime in OFFSET:
        x = std * (n + OFFSET[regime])
    elif regime == "mixed_offset":
        even = (torch.arange(C) % 2 == 0)
        x = torch.where(even, std * (n + OFFSET["offset30"]), x)
    elif regime == "column_spread":
        std = (10.0 ** (4.0 * torch.arange(C, dtype=torch.float64) / max(C - 1, 1) - 2.0)).float()
        x = std * (n + m)
    elif regime == "dead_relu":
        bias = bias.clone()
        bias[dead_columns(C)] = DEAD_BIAS
        cols, k = near_dead_columns(C)
        top = torch.sort(x[:, cols], dim=0, descending=True).values            # [M, len(cols)]
        idx = torch.arange(len(cols))
        bias[cols] = -0.5 * (top[k - 1, idx] + top[k, idx])
    return dict(x=x.reshape(B, L, C).contiguous(), gamma=gamma, beta=beta, bias=bias, upstream=up, mul=mul)


def pre_norm(x, bias, relu):
    a = x if bias is None else x + bias
    return torch.relu(a) if relu else a


def batch_norm(a, gamma, beta):
    """-> (y, mean, biased variance): statistics over every axis but the last, two-pass."""
    red = tuple(range(a.dim() - 1))
    mean = a.mean(dim=red)
    var = ((a - mean) ** 2).mean(dim=red)
    return (a - mean) * torch.rsqrt(var + BN_EPS) * gamma + beta, mean, var


def tail(y, act, mul):
    if act == 1:
        return torch.clamp(y, 0.0, 6.0)
    if act == 2:
        return mul * torch.sigmoid(y)
    return y


def bn_ref(inputs, dtype, bias=False, relu=False, act=0, biased_moving_variance=True):
    """-> {part: tensor} evaluated in ``dtype`` on the CPU: y, dx, dgamma, dbeta, dbias (with a bias), dmul (act 2), batch_mean, batch_var
    (biased), moving_mean, moving_var (from zero: ONE_MINUS_DECAY x the batch mean and the biased or unbiased batch variance), and z, the
    batch norm's own output in front of the tail (not a part: conditions reads it)."""
    def leaf(t):
        return t.detach().to(dtype).clone().requires_grad_(True)
    x, gamma, beta = leaf(inputs["x"]), leaf(inputs["gamma"]), leaf(inputs["beta"])
    leaves = dict(dx=x, dgamma=gamma, dbeta=beta)
    b = mul = None
    if bias:
        b = leaves["dbias"] = leaf(inputs["bias"])
    if act == 2:
        mul = leaves["dmul"] = leaf(inputs["mul"])
    z, mean, var = batch_norm(pre_norm(x, b, relu), gamma, beta)
    y = tail(z, act, mul)
    names = list(leaves)
    grads = torch.autograd.grad((y * inputs["upstream"].to(dtype)).sum(), [leaves[n] for n in names])
    n = x.numel() // x.shape[-1]
    mvar = var if biased_moving_variance else var * (n / max(n - 1, 1))
    out = dict(y=y.detach(), **dict(zip(names, grads)))
    out.update(batch_mean=mean.detach(), batch_var=var.detach(), moving_mean=ONE_MINUS_DECAY * mean.detach(),
               moving_var=ONE_MINUS_DECAY * mvar.detach(), z=z.detach())
    return out


def _quotient(err, scale):
    """err / scale where scale > 0; where the reference is identically zero: 0 if the error is, inf otherwise."""
    return torch.where(scale > 0, err / scale.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), err))


def figure(got, ref, part, B, floor=None):
    """The error figure of one part.  Row-axis parts (y, dx, dmul; [B, L, C]): the larger of the maximum over the examples of
    (max |error| in the example / max |fp64| in the example) and the maximum over the columns of the same quotient per column, a column whose
    fp64 values are all zero left out of the second (exactly_zero holds it).  Every other part: max |error| / max |fp64| over the tensor.
    floor: the error is taken against this scale instead (a part that is about zero: the bias gradient without a ReLU)."""
    ref = ref.detach().double().cpu()
    got = got.detach().double().cpu().reshape(ref.shape)
    err = (got - ref).abs()
    if floor is not None:
        return float(err.max() / floor)
    if part not in ROW_PARTS:
        return float(_quotient(err.max().reshape(1), ref.abs().max().reshape(1)))
    C = ref.shape[-1]
    per_example = _quotient(err.reshape(B, -1).max(1).values, ref.abs().reshape(B, -1).max(1).values)
    col_err, col_scale = err.reshape(-1, C).max(0).values, ref.abs().reshape(-1, C).max(0).values
    live = col_scale > 0
    per_column = _quotient(col_err[live], col_scale[live])
    return float(torch.cat([per_example, per_column]).max())


def exactly_zero(got, ref, part, dead):
    """Is ``got`` exactly zero where the reference is identically zero -- a whole column of a row-axis part; of any other part the elements
    of the columns ``dead`` (a bool mask: the columns whose activation is constant, fp64 batch variance 0) that are zero in fp64?  (Elsewhere a
    zero of a column part is a sum that cancels, the bias gradient of a column no ReLU clips: rounding noise in any evaluation.)"""
    ref = ref.detach().double().cpu()
    got = got.detach().double().cpu().reshape(ref.shape)
    if part in ROW_PARTS:
        C = ref.shape[-1]
        zero = ref.abs().reshape(-1, C).max(0).values == 0
        return bool((got.reshape(-1, C)[:, zero] == 0).all())
    return bool((got[dead & (ref == 0)] == 0).all())


def raw_moment_parts(inputs, bias=False, relu=False, block=64):
    """The raw-moment form, emulated in fp32 on the CPU: per 64-row block the fp32 sums of a and a^2, the blocks folded in fp64,
    var = q / n - mu^2; then y = a * scale + shift and the backward of the rows kernels with those statistics, all in fp32.
    -> dict(y, dx, batch_mean, batch_var)"""
    d = {k: v.float() for k, v in inputs.items()}
    a = pre_norm(d["x"], d["bias"] if bias else None, relu)
    C = a.shape[-1]
    a2 = a.reshape(-1, C)
    M = a2.shape[0]
    s = torch.zeros(C, dtype=torch.float64)
    q = torch.zeros(C, dtype=torch.float64)
    for r0 in range(0, M, block):
        blk = a2[r0:r0 + block]
        s += blk.sum(0).double()
        q += (blk * blk).sum(0).double()
    mu = s / M
    var = (q / M - mu * mu).clamp_min(0)
    mean32, var32 = mu.float(), var.float()
    scale = d["gamma"] * (1.0 / torch.sqrt(var + BN_EPS)).float()
    shift = d["beta"] - mean32 * scale
    y = a2 * scale + shift
    rs = torch.rsqrt(var32 + BN_EPS)
    up = d["upstream"].reshape(-1, C)
    xh = (a2 - mean32) * rs
    dbeta, dgamma = up.sum(0), (up * xh).sum(0)
    dx = d["gamma"] * rs * (up - dbeta / M - xh * dgamma / M)
    if relu:
        dx = torch.where(a2 > 0, dx, torch.zeros_like(dx))
    return dict(y=y.reshape(a.shape), dx=dx.reshape(a.shape), batch_mean=mean32, batch_var=var32)


def conditions(inputs, parts64, regime="random", bias=False, relu=False, act=0):
    """What seed selection rests on, in fp64 -> (ok, values), values = (min and max over the live columns of |mean| / std, the least column
    variance, the least maximum of a part per example and per live column, the least distance of any z from 0 and 6 (act 1; else inf)).
    ok: the offset regimes' columns (mixed_offset: the even ones) have |mean| / std within [0.5 R, 1.5 R]; without a ReLU or relu6 no column
    of any part is identically zero (with one a column can be dead: exactly_zero holds it); every part's maximum in every example is > 0; act 1: the distance is at least 1e-5; dead_relu: the dead
    columns of relu(x + bias) are exactly zero and the near-dead ones have the stated number of positive rows, none within 1e-4 of zero."""
    B, _, C = inputs["x"].shape
    mean, var = parts64["batch_mean"].double(), parts64["batch_var"].double()
    live = var > 0
    ratio = (mean.abs() / var.clamp_min(1e-300).sqrt())[live]
    ok = True
    if regime in OFFSET or regime == "mixed_offset":
        R = OFFSET.get(regime, OFFSET["offset30"])
        held = ratio if regime in OFFSET else (mean.abs() / var.sqrt())[0::2]
        ok = ok and float(held.min()) >= 0.5 * R and float(held.max()) <= 1.5 * R
        if regime == "mixed_offset":
            ok = ok and float((mean.abs() / var.sqrt())[1::2].max()) <= 3.0
    least = float("inf")
    for n, v in parts64.items():
        if n == "z":
            continue
        v = v.double().abs()
        if n in ROW_PARTS:
            least = min(least, float(v.reshape(B, -1).max(1).values.min()))
            cols = v.reshape(-1, C).max(0).values
            if not (relu or act == 1):
                ok = ok and float(cols.min()) > 0
            least = min(least, float(cols[cols > 0].min()))
        else:
            least = min(least, float(v.max()))
    ok = ok and least > 0
    if not relu:
        ok = ok and bool(live.all())
    distance = float("inf")
    if act == 1:
        z = parts64["z"].double()
        distance = float(torch.minimum(z.abs(), (z - 6.0).abs()).min())
        ok = ok and distance >= MIN_ACT1_DISTANCE
    if regime == "dead_relu":
        assert bias and relu
        pre = (inputs["x"].double() + inputs["bias"].double()).reshape(-1, C)
        ok = ok and bool((pre[:, dead_columns(C)] <= 0).all()) and bool((~live[dead_columns(C)]).all())
        cols, k = near_dead_columns(C)
        ok = ok and bool(((pre[:, cols] > 0).sum(0) == k).all()) and float(pre[:, cols].abs().min()) >= 1e-4
        ok = ok and int((~live).sum()) == len(dead_columns(C))
    return ok, (float(ratio.min()), float(ratio.max()), float(var.min()), least, distance)
