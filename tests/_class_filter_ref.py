"""Plain-torch restatement of the class filter behind MoeModel2 / JuhanMoeModel (reference: video_level_models.py:441-541, :544-622),
independent of the dtype of its inputs: the tests evaluate it in fp64 (the reference) and in fp32 on the CPU (the error a faithful fp32
evaluation carries).  It never calls ops.class_filter or the package's models.

One stage, for a [B, C]:
    pre = a (+ bias) (+ residual);  u = act(pre);  v = gamma (u - mean) / sqrt(var + eps) + beta;  y = v * keep / keep_prob
training: mean and the BIASED variance of the batch, two-pass; the moving statistics become decay * old + (1 - decay) * (mean | var);
eval: the moving statistics, no mask."""
import torch

EPS = 1e-3
DECAY = 0.99
ALPHA = 0.2
KEEP_PROB = 0.8
NUM_MIXTURES = 3
STAGES = {  # the three configurations the models use: (bias, residual, batch norm, keep mask, activation or None = the model's)
    "filter1": dict(bias=True, residual=False, bn=True, keep=True, act=None),
    "residual": dict(bias=False, residual=True, bn=True, keep=False, act=None),
    "output": dict(bias=True, residual=False, bn=False, keep=False, act="sigmoid"),
}


def activation(pre, act):
    if act == "relu":
        return torch.where(pre > 0, pre, torch.zeros_like(pre))
    if act == "leaky_relu":
        return torch.where(pre > 0, pre, ALPHA * pre)
    if act == "sigmoid":
        return 1 / (1 + torch.exp(-pre))
    raise ValueError(act)


def pre_activation(inp):
    pre = inp["a"]
    if inp.get("bias") is not None:
        pre = pre + inp["bias"]
    if inp.get("residual") is not None:
        pre = pre + inp["residual"]
    return pre


def stage(inp, act, is_training, keep_prob=KEEP_PROB, decay=DECAY, eps=EPS):
    """inp: a, bias | None, residual | None, gamma / beta / moving_mean / moving_variance (all or none), keep | None (0 / 1, any dtype)
    -> dict(y, u, mean, rstd, moving_mean, moving_variance) (the last four None without batch norm; the moving statistics are the NEW
    ones in training, the given ones in eval)."""
    u = activation(pre_activation(inp), act)
    out = dict(u=u, mean=None, rstd=None, moving_mean=None, moving_variance=None)
    v = u
    if inp.get("gamma") is not None:
        if is_training:
            mean = u.mean(dim=0)
            var = ((u - mean) ** 2).mean(dim=0)
            out["moving_mean"] = decay * inp["moving_mean"] + (1 - decay) * mean.detach()
            out["moving_variance"] = decay * inp["moving_variance"] + (1 - decay) * var.detach()
        else:
            mean, var = inp["moving_mean"], inp["moving_variance"]
            out["moving_mean"], out["moving_variance"] = mean, var
        rstd = 1 / torch.sqrt(var + eps)
        v = (u - mean) * rstd * inp["gamma"] + inp["beta"]
        out["mean"], out["rstd"] = mean.detach(), rstd.detach()
    if is_training and inp.get("keep") is not None:
        v = v * inp["keep"].to(v.dtype) / keep_prob
    out["y"] = v
    return out


GRAD_NAMES = ("a", "bias", "residual", "gamma", "beta")


def stage_gradients(inp, act, is_training, dy, **kw):
    """-> (stage's dict, {name: d sum(y dy) / d name}) for the differentiable inputs that are given"""
    leaves = dict(inp)
    names = [n for n in GRAD_NAMES if inp.get(n) is not None]
    for n in names:
        leaves[n] = inp[n].detach().clone().requires_grad_(True)
    out = stage(leaves, act, is_training, **kw)
    grads = torch.autograd.grad((out["y"] * dy).sum(), [leaves[n] for n in names])
    return {k: (v.detach() if v is not None else None) for k, v in out.items()}, dict(zip(names, grads))


def make_stage_inputs(B, C, kind, act, seed, dtype=torch.float32, offset=0.0, dead=False):
    """Inputs of one stage configuration (STAGES[kind]) whose pre-activation is sign(z) (|z| + 0.01), z ~ N(0, 1) -- nothing sits on the
    kink of a ReLU.  offset: column c's pre-activations are shifted by +-offset (the sign alternates with c; always + under relu, where a
    negative column would be dead); dead: every pre-activation negative.  Everything is drawn in fp32."""
    cfg = STAGES[kind]
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, C, generator=g)
    pre = torch.sign(z) * (z.abs() + 0.01)
    pre = torch.where(pre == 0, torch.full_like(pre, 0.01), pre)
    if dead:
        pre = -pre.abs()
    if offset:
        sgn = torch.ones(C) if act == "relu" else torch.where(torch.arange(C) % 2 == 0, torch.ones(C), -torch.ones(C))
        pre = pre + offset * sgn
    inp = {}
    rest = pre
    if cfg["bias"]:
        inp["bias"] = 0.5 * torch.randn(C, generator=g)
        rest = rest - inp["bias"]
    if cfg["residual"]:
        inp["residual"] = torch.rand(B, C, generator=g)                 # (probabilities)
        rest = rest - inp["residual"]
    inp["a"] = rest
    if cfg["bn"]:
        inp["gamma"] = 1 + 0.3 * torch.randn(C, generator=g)
        inp["beta"] = 0.3 * torch.randn(C, generator=g)
        inp["moving_mean"] = 0.2 * torch.randn(C, generator=g)
        inp["moving_variance"] = 0.5 + torch.rand(C, generator=g)
    if cfg["keep"]:
        inp["keep"] = (torch.rand(B, C, generator=g) < KEEP_PROB).to(torch.uint8)
    dy = torch.randn(B, C, generator=g)
    return {k: (v.to(dtype) if v.dtype.is_floating_point else v) for k, v in inp.items()}, dy.to(dtype)


def widen(inp):
    return {k: (v.double() if v is not None and v.dtype.is_floating_point else v) for k, v in inp.items()}


# ---- the whole models from a dict of variables (names without the tower prefix) -----------------------------------------------------
def mixture(x, p):
    V = p["experts/biases"].shape[0] // NUM_MIXTURES
    gates = torch.softmax((x @ p["gates/weights"]).reshape(-1, NUM_MIXTURES + 1), dim=-1)
    experts = torch.sigmoid((x @ p["experts/weights"] + p["experts/biases"]).reshape(-1, NUM_MIXTURES))
    return (gates[:, :NUM_MIXTURES] * experts).sum(dim=1).reshape(-1, V)


def model(name, x, p, is_training, masks=None):
    """name "MoeModel2" | "JuhanMoeModel"; x [B, F] (already L2-normalised); p: the variables; masks: {"probabilities", "filter1"} keep
    masks (training).  -> (predictions, {moving statistic: new value})"""
    act = {"MoeModel2": "relu", "JuhanMoeModel": "leaky_relu"}[name]
    masks = masks or {}
    prob = mixture(x, p)
    if name == "JuhanMoeModel" and is_training:
        prob = prob * masks["probabilities"].to(prob.dtype) / KEEP_PROB

    def bn(scope):
        return {k: p[f"{scope}/{k}"] for k in ("gamma", "beta", "moving_mean", "moving_variance")}

    s1 = stage(dict(a=prob @ p["v-filter1/kernel"], bias=p["v-filter1/bias"], keep=masks.get("filter1"), **bn("batch_normalization")),
               act, is_training)
    s2 = stage(dict(a=s1["y"] @ p["v-filter2/kernel"], residual=prob, **bn("batch_normalization_1")), act, is_training)
    s3 = stage(dict(a=s2["y"] @ p["v-final_output/kernel"], bias=p["v-final_output/bias"]), "sigmoid", is_training)
    stats = {"batch_normalization/moving_mean": s1["moving_mean"], "batch_normalization/moving_variance": s1["moving_variance"],
             "batch_normalization_1/moving_mean": s2["moving_mean"], "batch_normalization_1/moving_variance": s2["moving_variance"]}
    return s3["y"], stats


def cross_entropy(pred, labels, eps=1e-5):
    """losses.py:41-51: the mean over the batch of the row sums"""
    y = labels.to(pred.dtype)
    return (-(y * torch.log(pred + eps) + (1 - y) * torch.log(1 - pred + eps))).sum(dim=1).mean()


VARIABLES = {  # name -> shape as a function of (F, V); the moving statistics are not trainable
    "gates/weights": lambda F, V: (F, 4 * V), "experts/weights": lambda F, V: (F, 3 * V), "experts/biases": lambda F, V: (3 * V,),
    "v-filter1/kernel": lambda F, V: (V, 2 * V), "v-filter1/bias": lambda F, V: (2 * V,),
    "batch_normalization/gamma": lambda F, V: (2 * V,), "batch_normalization/beta": lambda F, V: (2 * V,),
    "batch_normalization/moving_mean": lambda F, V: (2 * V,), "batch_normalization/moving_variance": lambda F, V: (2 * V,),
    "v-filter2/kernel": lambda F, V: (2 * V, V),
    "batch_normalization_1/gamma": lambda F, V: (V,), "batch_normalization_1/beta": lambda F, V: (V,),
    "batch_normalization_1/moving_mean": lambda F, V: (V,), "batch_normalization_1/moving_variance": lambda F, V: (V,),
    "v-final_output/kernel": lambda F, V: (V, V), "v-final_output/bias": lambda F, V: (V,),
}
STATISTICS = tuple(n for n in VARIABLES if n.endswith(("/moving_mean", "/moving_variance")))


def make_variables(F, V, seed):
    """fp32 variables with every vector away from its initial value (a test that leaves beta at 0 and gamma at 1 sees neither)"""
    g = torch.Generator().manual_seed(seed)
    p = {}
    for n, shape in VARIABLES.items():
        s = shape(F, V)
        if n.endswith("/moving_variance"):
            p[n] = 0.5 + torch.rand(s, generator=g)
        elif n.endswith("/gamma"):
            p[n] = 1 + 0.3 * torch.randn(s, generator=g)
        elif len(s) == 1:
            p[n] = 0.3 * torch.randn(s, generator=g)
        else:
            p[n] = torch.randn(s, generator=g) * (2.0 / (s[0] + s[1])) ** 0.5 * 2
    return p
