"""Restatement of NetVLAD / LightVLAD (frame_level_models.py:2773-2877), of the NetVladAttenCluster aggregation tail
(video_pooling_modules.py:1646-1658) and of input_bn (slim.batch_norm over the sampled rows) in plain torch on the CPU, written from the
formulas of oracle/lpm_oracle.py (_assignment, batch_norm, vlad_aggregate, l2_normalize) and never from the package.  Every function
computes in the dtype of its inputs: fp64 is the reference, fp32 gives the evaluation error err32 the GPU bounds are built from.

    logits = x W;  act = (logits - mean) rsqrt(var + 1e-3) gamma + beta  (batch statistics, biased variance; or the moving ones; or
    logits + bias);  A = softmax(act);  V[b, d, k] = sum_t A[b, t, k] x[b, t, d] - (sum_t A[b, t, k]) W2[d, k];
    out = l2n(flatten_d_major(l2n(V, over d)))  with  l2n(v) = v rsqrt(max(sum v^2, 1e-12)).

``mm`` is the product used for the two GEMMs of the forward (logits, A^T x) and, through autograd, for the GEMMs of the gradient.
mm3 is the split-operand model of "bf16x3" (include/lpm_hip.h, csrc/operand_format.h): every operand of a matrix product is rounded to
bf16 hi + bf16 lo, the lo x lo product is dropped, everything else is exact.  |a - ah - al| <= 2^-18 |a| (two roundings to 8 significant
bits), so |mm3(a, b) - a b| <= 3 * 2^-18 (|a| |b|) componentwise up to second-order terms; tests/test_netvlad_ref_host.py
asserts the bound on random matrices with inner sizes 16 .. 1024 and prints the worst componentwise ratio it meets (2.4 * 2^-18)."""
import torch

BN_EPS = 1e-3
L2_EPS = 1e-12
# The kernel's blend is moving = moving * decay + batch * (1.f - decay) in fp32 with decay = fp32(0.999) (csrc/bn.hip, bn_fold_kernel and
# the small-matrix form beside it): its factor is 1 - fp32(0.999) = 0.00099998713, 1.29e-5 below 0.001 relatively.  That offset is a property
# of this kernel's documented arithmetic (a blend factor formed in double and rounded once would be fp32(0.001)); it leaves a moving statistic
# 1.3e-5 low in the steady state and is put into the model here, not taken out of the kernel: from zero moving statistics the op leaves
# ONE_MINUS_DECAY x the batch statistics -- measured on the MI355X as a constant 1.29e-5 against 0.001 x, in every case and both precisions.
DECAY = float(torch.tensor(0.999, dtype=torch.float32))
ONE_MINUS_DECAY = float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(0.999, dtype=torch.float32))
REGIMES = ("random", "saturated", "near_centre", "small_mass")
SMALL_MASS_K1, SMALL_MASS_K2 = 3, 5          # the two clusters of the small-mass regime (see make_inputs)
SMALL_MASS_BETA = (-9.0, -20.0)


# ---- the split-operand product ----
def split_bf16(a):
    """-> (hi, lo) in fp64: a rounded to bf16, and the remainder rounded to bf16."""
    ah = a.float().bfloat16().double()
    al = (a.double() - ah).float().bfloat16().double()
    return ah, al


def three_term(a, b):
    ah, al = split_bf16(a)
    bh, bl = split_bf16(b)
    return ah @ bh + ah @ bl + al @ bh


class _MM3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        return three_term(a, b)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        return three_term(g, b.transpose(-1, -2)), three_term(a.transpose(-1, -2), g)


def mm3(a, b):
    """fp64 in, fp64 out; both operands of the same rank (2-D, or batched 3-D)."""
    return _MM3.apply(a, b)


# ---- the formulas ----
def l2_normalize(x, dim):
    return x * torch.rsqrt(torch.clamp((x * x).sum(dim=dim, keepdim=True), min=L2_EPS))


def raw_sums(assign, x, centres, mm=torch.matmul):
    """assign [B, T, K], x [B, T, D], centres [D, K] or None -> V [B, D, K], un-normalised."""
    v = mm(assign.transpose(1, 2).contiguous(), x).transpose(1, 2)
    if centres is not None:
        v = v - assign.sum(dim=1, keepdim=True) * centres.reshape(1, centres.shape[-2], centres.shape[-1])
    return v


def normalise(v):
    """V [B, D, K] -> [B, D K] d-major: l2n over d, flatten, l2n."""
    return l2_normalize(l2_normalize(v, 1).reshape(v.shape[0], -1), 1)


def aggregate(sims, x, centres, T, mm=torch.matmul):
    """The V2 form: similarities [B, T, K] used as they are (no softmax), x [B T, D] -> [B, D K] d-major."""
    return normalise(raw_sums(sims, x.reshape(-1, T, x.shape[-1]), centres, mm))


def batch_moments(v):
    """-> (mean, biased variance, unbiased variance) over the rows of v [n, C]."""
    n = v.shape[0]
    mean = v.mean(0)
    var = ((v - mean) ** 2).mean(0)
    return mean, var, var * (n / max(n - 1, 1))


def netvlad(x, W, gamma, beta, W2, T, *, training, moving=None, bias=None, mm=torch.matmul, eps=BN_EPS, normalise_unbiased=False):
    """x [B T, D] -> (descriptor [B, D K] d-major, batch mean, unbiased batch variance of the logits; the two are None outside training-mode
    batch norm).  W2 = None: LightVLAD.  gamma = None: the cluster_biases branch.  training = False: the moving statistics normalise.
    ``eps`` and ``normalise_unbiased`` exist for the host test's deliberately WRONG restatements only."""
    logits = mm(x, W)
    mean = uvar = None
    if gamma is not None:
        if training:
            mean, var, uvar = batch_moments(logits)
            if normalise_unbiased:
                var = uvar
        else:
            mean, var = moving
        act = (logits - mean) * torch.rsqrt(var + eps) * gamma + beta
        if not training:
            mean = None
    else:
        act = logits + bias
    assign = torch.softmax(act, dim=-1).reshape(-1, T, act.shape[-1])
    centres = W2.reshape(W2.shape[-2], W2.shape[-1]) if W2 is not None else None
    return normalise(raw_sums(assign, x.reshape(-1, T, x.shape[-1]), centres, mm)), mean, uvar


def input_bn(frames, gamma, beta, *, training, moving=None):
    """frames [n, F] (the sampled rows) -> (y, batch mean, unbiased batch variance): slim batch norm, eps 1e-3, biased variance to
    normalise, unbiased variance for the moving average; training = False normalises with ``moving`` = (mean, variance)."""
    if training:
        mean, var, uvar = batch_moments(frames)
    else:
        (mean, var), uvar = moving, None
    y = (frames - mean) * torch.rsqrt(var + BN_EPS) * gamma + beta
    return (y, mean, uvar) if training else (y, None, None)


def gather_rows(frames, index):
    """frames [B, MF, F], index [B, S] (long) -> [B S, F]."""
    B = frames.shape[0]
    return frames[torch.arange(B).unsqueeze(1), index].reshape(-1, frames.shape[-1])


# ---- inputs ----
def clip_decades(B):
    """Factor of clip b's upstream gradient: 10^(6 b / (B - 1) - 3), six decades from the first clip to the last (1 for a single clip)."""
    if B == 1:
        return torch.ones(1)
    return 10.0 ** (6.0 * torch.arange(B, dtype=torch.float64) / (B - 1) - 3.0)


def make_inputs(B, T, D, K, seed, regime="random"):
    """-> dict of fp32 tensors: x [B T, D], W [D, K], gamma, beta, bias [K], W2 [1, D, K], sims [B, T, K], moving = (mean, variance) for
    eval mode, frames [B T, D] / in_gamma / in_beta [D] for the input_affine form, upstream [B, D K] d-major (N(0, 1) times the clip's decade).
    random: as tests/test_gpu_kernels._netvlad_inputs.  saturated: gamma times 30.  near_centre: x = W2[:, t % 4] + 1e-2 noise / sqrt(D).
    small_mass: beta[SMALL_MASS_K1] = -9 (the column still normalises to 1 / sqrt(K)), beta[SMALL_MASS_K2] = -20 (squared norm below
    l2_normalize's 1e-12 clamp: the column comes out as raw * 1e6)."""
    assert regime in REGIMES
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B * T, D, generator=g)
    W = torch.randn(D, K, generator=g) / D ** 0.5
    gamma = 1 + 0.3 * torch.randn(K, generator=g)
    beta = 0.2 * torch.randn(K, generator=g)
    W2 = torch.randn(1, D, K, generator=g) / D ** 0.5
    up = torch.randn(B, D * K, generator=g) * clip_decades(B).float().unsqueeze(1)
    bias = torch.randn(K, generator=g)
    sims = torch.randn(B, T, K, generator=g)
    moving = (0.1 * torch.randn(K, generator=g), 1 + 0.2 * torch.rand(K, generator=g))
    frames = torch.randn(B * T, D, generator=g) * (0.5 + torch.rand(D, generator=g)) + 0.3 * torch.randn(D, generator=g)
    in_gamma = 1 + 0.3 * torch.randn(D, generator=g)
    in_beta = 0.2 * torch.randn(D, generator=g)
    if regime == "saturated":
        gamma = gamma * 30
    elif regime == "near_centre":
        k_of_t = torch.arange(B * T) % 4
        x = W2[0].t()[k_of_t] + 1e-2 * x / D ** 0.5
    elif regime == "small_mass":
        beta[SMALL_MASS_K1], beta[SMALL_MASS_K2] = SMALL_MASS_BETA
    return dict(x=x, W=W, gamma=gamma, beta=beta, W2=W2, bias=bias, sims=sims, moving=moving, frames=frames, in_gamma=in_gamma,
                in_beta=in_beta, upstream=up)


FORMS = ("netvlad", "light", "bias", "aggregate", "input_affine")
CLIP_PARTS = ("out", "dx", "dsims")          # parts with a clip axis: the error figure is taken per clip


def values_and_grads(inputs, T, dtype, mm=torch.matmul, upstream=None, *, form="netvlad", training=True, **wrong):
    """-> {part: tensor} evaluated in ``dtype`` on the CPU, gradients by autograd with the loss sum(out * upstream):
    netvlad / light: out, dx, dW, dgamma, dbeta (, dW2) (, batch_mean, batch_var in training mode);  bias: out, dx, dW, dbias, dW2;
    aggregate: out, dsims, dx, dcentres;  input_affine (x = input_bn(frames) in training mode, then NetVLAD): out, dW, dgamma, dbeta, dW2,
    d_in_gamma, d_in_beta, batch_mean, batch_var.  ``wrong``: eps / normalise_unbiased for netvlad()."""
    assert form in FORMS
    up = (inputs["upstream"] if upstream is None else upstream).to(dtype)

    def leaf(name):
        return inputs[name].detach().to(dtype).clone().requires_grad_(True)
    if form == "aggregate":
        leaves = dict(dsims=leaf("sims"), dx=leaf("x"), dcentres=leaf("W2"))
        out = aggregate(leaves["dsims"], leaves["dx"], leaves["dcentres"][0], T, mm)
        mean = uvar = None
    else:
        leaves = dict(dW=leaf("W"))
        if form == "input_affine":
            leaves.update(d_in_gamma=leaf("in_gamma"), d_in_beta=leaf("in_beta"))
            x = input_bn(inputs["frames"].to(dtype), leaves["d_in_gamma"], leaves["d_in_beta"], training=True)[0]
        else:
            x = leaves["dx"] = leaf("x")
        if form == "bias":
            leaves["dbias"] = leaf("bias")
        else:
            leaves.update(dgamma=leaf("gamma"), dbeta=leaf("beta"))
        if form != "light":
            leaves["dW2"] = leaf("W2")
        moving = tuple(m.to(dtype) for m in inputs["moving"])
        out, mean, uvar = netvlad(x, leaves["dW"], leaves.get("dgamma"), leaves.get("dbeta"), leaves.get("dW2"), T, training=training,
                                  moving=moving, bias=leaves.get("dbias"), mm=mm, **wrong)
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


def column_figure(got, ref, B, K, k):
    """The figure of ``out`` [B, D K] d-major for cluster column k alone, per clip."""
    ref = ref.detach().double().cpu().reshape(B, -1, K)[:, :, k]
    got = got.detach().double().cpu().reshape(B, -1, K)[:, :, k]
    return figure(got, ref, "out", B)


# Both sides must agree on which side of l2_normalize's 1e-12 clamp a cluster column's squared norm lies (the forward is continuous
# there, the gradient is not: projected above, raw * 1e6 below).  Two decades either side, except in the saturated regime: with gamma
# times 30 most clusters of a clip win no frame and their squared norms spread evenly over 1e-50 .. 1 (10 to 20 columns of every seed lie
# in [1e-14, 1e-10]: 400 seeds searched, none free), so there the band is a factor 2 either side -- a thousand times the 1e-3 by which
# any evaluation held to these tests' bounds can move a squared norm -- and columns below it are expected.
CLAMP_BAND = (1e-14, 1e-10)
SATURATED_BAND = (5e-13, 2e-12)


def conditions(inputs, T, parts64, parts32, *, form="netvlad", training=True, regime="random"):
    """The conditions a seed must meet, evaluated on the fp64 restatement -> (ok, values): no cluster column's squared norm in
    CLAMP_BAND (small_mass: column SMALL_MASS_K2 below it, every other above; saturated: SATURATED_BAND, and most frames' largest softmax
    weight above 0.999), no clip whose fp64 dx is identically zero, err32 > 0 for every part that is not identically zero.
    values: (min colsq above the band, max colsq below it or 0, min over clips of max |dx|, min err32 over the non-zero parts)."""
    d = {k: (v.double() if torch.is_tensor(v) else v) for k, v in inputs.items()}
    B = d["upstream"].shape[0]
    if form == "aggregate":
        v = raw_sums(d["sims"], d["x"].reshape(B, T, -1), d["W2"][0])
    else:
        x = input_bn(d["frames"], d["in_gamma"], d["in_beta"], training=True)[0] if form == "input_affine" else d["x"]
        logits = x @ d["W"]
        if form == "bias":
            act = logits + d["bias"]
        else:
            mean, var = batch_moments(logits)[:2] if training else tuple(m.double() for m in inputs["moving"])
            act = (logits - mean) * torch.rsqrt(var + BN_EPS) * d["gamma"] + d["beta"]
        v = raw_sums(torch.softmax(act, -1).reshape(B, T, -1), x.reshape(B, T, -1), None if form == "light" else d["W2"][0])
    colsq = (v * v).sum(1)                                        # [B, K]
    lo, hi = SATURATED_BAND if regime == "saturated" else CLAMP_BAND
    above = colsq[colsq > hi]
    below = colsq[colsq < lo]
    ok = above.numel() + below.numel() == colsq.numel()
    if regime == "saturated":
        ok = ok and float(torch.softmax(act, -1).max(-1).values.gt(0.999).float().mean()) > 0.5
    elif regime == "small_mass":
        low = torch.zeros_like(colsq, dtype=torch.bool)
        low[:, SMALL_MASS_K2] = True
        ok = ok and bool(((colsq < 1e-14) == low).all())
    else:
        ok = ok and below.numel() == 0
    min_dx = float("inf")
    if "dx" in parts64:
        min_dx = float(parts64["dx"].abs().reshape(B, -1).max(1).values.min())
        ok = ok and min_dx > 0
    e32 = [figure(parts32[n], parts64[n], n, B) for n in parts64 if float(parts64[n].abs().max()) > 0]
    ok = ok and min(e32) > 0
    return ok, (float(above.min()) if above.numel() else float("inf"), float(below.max()) if below.numel() else 0.0, min_dx, min(e32))
