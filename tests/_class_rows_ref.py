"""Plain-torch restatement of the row-wise glue over [B, C] class scores (ops.class_rows), of FishMoeModel3 (reference:
video_level_models.py:367-438) and of the five class-gating modules (attention_modules.py:157-362), independent of the dtype of its
inputs: the tests evaluate it in fp64 (the reference) and in fp32 on the CPU (the error a faithful fp32 evaluation carries).  It never
calls ops.class_rows, ops.class_filter or the package's models and modules.

One stage, for a [B, C]:
    t = a (+ bias);  pre = phi(t) (+ residual);  y = pre | softmax(pre) over the row | gamma (pre - mean) / sqrt(var + eps) + beta
phi: identity | relu6 (tf.nn.relu6, attention_modules.py:187) | neg_relu6 = -relu6(-t) (:192-194); the layer norm is
tf.contrib.layers.layer_norm at rank 2 (video_level_models.py:434): the mean and the BIASED variance of the row, two-pass, eps 1e-12."""
import torch

LN_EPS = 1e-12
BN_EPS = 1e-3
TF_LAYERS_MOMENTUM = 0.99          # tf.layers.batch_normalization (video_level_models.py:425, :428, :435)
SLIM_DECAY = 0.999                 # slim.batch_norm (attention_modules.py:349)
FORMS = {  # every (phi, norm) pair the models use
    "ln": dict(bias=True, residual=True, phi="identity", norm="layer_norm"),           # video_level_models.py:431-434
    "softmax": dict(bias=True, residual=False, phi="identity", norm="softmax"),        # :436
    "p_gate": dict(bias=False, residual=True, phi="relu6", norm="none"),               # attention_modules.py:186-188
    "p_gate_softmax": dict(bias=False, residual=True, phi="relu6", norm="softmax"),    # :235-238, :268-271
    "n_gate_softmax": dict(bias=False, residual=True, phi="neg_relu6", norm="softmax"),   # :191-196
}
GRAD_NAMES = ("a", "bias", "residual", "gamma", "beta")


def relu6(t):
    return torch.clamp(t, min=0.0, max=6.0)


def gate(t, phi):
    if phi == "identity":
        return t
    if phi == "relu6":
        return relu6(t)
    if phi == "neg_relu6":
        return -relu6(-t)
    raise ValueError(phi)


def gate_argument(inp):
    return inp["a"] if inp.get("bias") is None else inp["a"] + inp["bias"]


def kink_distance(t):
    """the smallest distance of an element of t from 0 and from +-6"""
    return float(torch.minimum(t.abs(), (t.abs() - 6).abs()).min())


def rows(inp, phi, norm, eps=LN_EPS):
    """inp: a, bias | None, residual | None, gamma / beta (layer_norm) -> dict(y, pre, stats [B, 2] = (mean, rstd) | None)"""
    pre = gate(gate_argument(inp), phi)
    if inp.get("residual") is not None:
        pre = pre + inp["residual"]
    out = dict(pre=pre, stats=None)
    if norm == "none":
        out["y"] = pre
    elif norm == "softmax":
        e = torch.exp(pre - pre.max(dim=1, keepdim=True).values)
        out["y"] = e / e.sum(dim=1, keepdim=True)
    elif norm == "layer_norm":
        mean = pre.mean(dim=1, keepdim=True)
        var = ((pre - mean) ** 2).mean(dim=1, keepdim=True)
        rstd = 1 / torch.sqrt(var + eps)
        out["y"] = (pre - mean) * rstd * inp["gamma"] + inp["beta"]
        out["stats"] = torch.cat([mean, rstd], dim=1).detach()
    else:
        raise ValueError(norm)
    return out


def rows_gradients(inp, phi, norm, dy, eps=LN_EPS):
    """-> (rows' dict, {name: d sum(y dy) / d name}) for the differentiable inputs that are given"""
    leaves = dict(inp)
    names = [n for n in GRAD_NAMES if inp.get(n) is not None]
    for n in names:
        leaves[n] = inp[n].detach().clone().requires_grad_(True)
    out = rows(leaves, phi, norm, eps)
    grads = torch.autograd.grad((out["y"] * dy).sum(), [leaves[n] for n in names])
    return {k: (v.detach() if v is not None else None) for k, v in out.items()}, dict(zip(names, grads))


def make_rows_inputs(B, C, form, seed, regime=None):
    """fp32 inputs of FORMS[form] and dy.  The gate's argument t walks the four bands (-9, -6.01), (-5.99, -0.01), (0.01, 5.99),
    (6.01, 9) with the element index (band (row + column) mod 4), uniform inside its band: every four neighbours cover all pieces of
    relu6 and of neg_relu6, and nothing is nearer than 0.01 to a kink.  regime "offset" (layer norm): the residual of a row is shifted
    by +-1.2e3 times the row's standard deviation; "shift": the scores of a softmax row by +1e3; "spread": the scores of a softmax row
    span 200 (the identity: the outer bands reach +-100; a gate: the residual uniform in (-100, 100))."""
    cfg = FORMS[form]
    g = torch.Generator().manual_seed(seed)
    lo = torch.tensor([-9.0, -5.99, 0.01, 6.01])
    hi = torch.tensor([-6.01, -0.01, 5.99, 9.0])
    band = (torch.arange(B).view(B, 1) + torch.arange(C).view(1, C)) % 4
    if regime == "spread" and cfg["phi"] == "identity":
        lo, hi = torch.tensor([-100.0, -5.99, 0.01, 6.01]), torch.tensor([-6.01, -0.01, 5.99, 100.0])
    t = lo[band] + (hi[band] - lo[band]) * torch.rand(B, C, generator=g)
    if regime == "shift" and not cfg["residual"]:
        t = t + 1e3
    inp = {}
    if cfg["bias"]:
        inp["bias"] = 0.5 * torch.randn(C, generator=g)
        inp["a"] = t - inp["bias"]
    else:
        inp["a"] = t
    if cfg["residual"]:
        r = torch.rand(B, C, generator=g)                              # (probabilities)
        if regime == "spread":
            r = 200.0 * r - 100.0
        if regime == "shift":
            r = r + 1e3
        if regime == "offset":
            pre = gate(t, cfg["phi"]) + r
            sgn = torch.where(torch.arange(B) % 2 == 0, torch.ones(B), -torch.ones(B)).view(B, 1)
            r = r + 1.2e3 * pre.std(dim=1, keepdim=True) * sgn
        inp["residual"] = r
    if cfg["norm"] == "layer_norm":
        inp["gamma"] = 1 + 0.3 * torch.randn(C, generator=g)
        inp["beta"] = 0.3 * torch.randn(C, generator=g)
    dy = torch.randn(B, C, generator=g)
    return inp, dy


def widen(inp):
    return {k: (v.double() if v is not None else None) for k, v in inp.items()}


# ---- batch norms ---------------------------------------------------------------------------------------------------------------------
def _batch_norm(x, p, scope, is_training, decay, unbiased_moving, stats):
    """gamma (x - mean) / sqrt(var + 1e-3) + beta over the batch; training: the batch mean and the biased batch variance, and the new
    moving statistics decay * old + (1 - decay) * (mean | var -- the unbiased one where ``unbiased_moving``) into ``stats``"""
    if is_training:
        n = x.shape[0]
        mean = x.mean(dim=0)
        var = ((x - mean) ** 2).mean(dim=0)
        moving_var = var * (n / max(n - 1, 1)) if unbiased_moving else var
        stats[scope + "/moving_mean"] = (decay * p[scope + "/moving_mean"] + (1 - decay) * mean).detach()
        stats[scope + "/moving_variance"] = (decay * p[scope + "/moving_variance"] + (1 - decay) * moving_var).detach()
    else:
        mean, var = p[scope + "/moving_mean"], p[scope + "/moving_variance"]
    return (x - mean) / torch.sqrt(var + BN_EPS) * p[scope + "/gamma"] + p[scope + "/beta"]


# ---- FishMoeModel3 from a dict of variables (names without the tower prefix) --------------------------------------------------------
def fish_moe3(x, p, is_training, num_mixtures=2):
    """video_level_models.py:396-438.  tf.layers.dropout(r_activation0, 0.9) (:430) has no training=: the identity.
    -> (predictions, {moving statistic: new value}, the smallest |argument| of the relu)"""
    V = p["dense_2/bias"].shape[0]
    stats = {}
    gates = torch.softmax((x @ p["gates/weights"]).reshape(-1, num_mixtures + 1), dim=-1)                    # :399-416
    experts = torch.sigmoid((x @ p["experts/weights"] + p["experts/biases"]).reshape(-1, num_mixtures))     # :407-419
    p0 = (gates[:, :num_mixtures] * experts).sum(dim=1).reshape(-1, V)                                       # :421-424
    p0 = _batch_norm(p0, p, "batch_normalization", is_training, TF_LAYERS_MOMENTUM, False, stats)           # :425
    pre0 = p0 @ p["dense/kernel"] + p["dense/bias"]                                                          # :427
    r0 = _batch_norm(torch.where(pre0 > 0, pre0, torch.zeros_like(pre0)), p, "batch_normalization_1", is_training, TF_LAYERS_MOMENTUM,
                     False, stats)                                                                           # :428 (:430: a no-op)
    p1 = rows(dict(a=r0 @ p["dense_1/kernel"], bias=p["dense_1/bias"], residual=p0, gamma=p["LayerNorm/gamma"], beta=p["LayerNorm/beta"]),
              "identity", "layer_norm")["y"]                                                                 # :431-434
    p1 = _batch_norm(p1, p, "batch_normalization_2", is_training, TF_LAYERS_MOMENTUM, False, stats)         # :435
    p2 = rows(dict(a=p1 @ p["dense_2/kernel"], bias=p["dense_2/bias"]), "identity", "softmax")["y"]          # :436
    return p2, stats, float(pre0.detach().abs().min())


def fish_moe3_variables(F, V, num_mixtures=2, filter_size=2):
    """name -> shape in creation order; the moving statistics are not trainable"""
    shapes = {"gates/weights": (F, V * (num_mixtures + 1)), "experts/weights": (F, V * num_mixtures), "experts/biases": (V * num_mixtures,)}

    def bn(scope, C):
        for n in ("gamma", "beta", "moving_mean", "moving_variance"):
            shapes[f"{scope}/{n}"] = (C,)

    bn("batch_normalization", V)
    shapes.update({"dense/kernel": (V, V * filter_size), "dense/bias": (V * filter_size,)})
    bn("batch_normalization_1", V * filter_size)
    shapes.update({"dense_1/kernel": (V * filter_size, V), "dense_1/bias": (V,), "LayerNorm/beta": (V,), "LayerNorm/gamma": (V,)})
    bn("batch_normalization_2", V)
    shapes.update({"dense_2/kernel": (V, V), "dense_2/bias": (V,)})
    return shapes


# ---- the five class-gating modules: x [B, V] -> (output, new moving statistics, the smallest distance of a relu / relu6 argument from
# a kink) ------------------------------------------------------------------------------------------------------------------------------
def _gate_stage(a, residual, phi, norm):
    return rows(dict(a=a, residual=residual), phi, norm)["y"], kink_distance(a.detach())


def pn_gate(x, p, is_training):                                        # attention_modules.py:186-196
    g, k1 = _gate_stage(x @ p["p_pn_gate"], x, "relu6", "none")
    y, k2 = _gate_stage(g @ p["n_pn_gate"], g, "neg_relu6", "softmax")
    return y, {}, min(k1, k2)


def np_gate(x, p, is_training):                                        # :229-238
    g, k1 = _gate_stage(x @ p["n_np_gate"], x, "neg_relu6", "none")
    y, k2 = _gate_stage(g @ p["p_np_gate"], g, "relu6", "softmax")
    return y, {}, min(k1, k2)


def p_gate(x, p, is_training):                                         # :268-271
    y, k = _gate_stage(x @ p["p_p_gate"], x, "relu6", "softmax")
    return y, {}, k


def cor_nn_gate(x, p, is_training):                                    # :295-316
    pre1 = x @ p["vocab_gate1_v1/weights"] + p["vocab_gate1_v1/biases"]
    pre2 = torch.relu(pre1) @ p["vocab_gate2_v1/weights"] + p["vocab_gate2_v1/biases"]
    pre3 = torch.relu(pre2) @ p["vocab_gate3_v1/weights"] + p["vocab_gate3_v1/biases"]
    return torch.sigmoid(pre3), {}, float(torch.minimum(pre1.detach().abs().min(), pre2.detach().abs().min()))


def context_gate_v1(x, p, is_training):                                # :342-362 (slim.batch_norm at rank 2: the unbiased variance
    stats = {}                                                         # goes into the moving average)
    gates = _batch_norm(x @ p["vocab_gate_v1"], p, "vocab_gate_bn_v1", is_training, SLIM_DECAY, True, stats)
    return x * torch.sigmoid(gates), stats, float("inf")


MODULES = {  # class name -> (restatement, {variable: shape as a function of V} in creation order)
    "PnGateModule": (pn_gate, {"p_pn_gate": lambda V: (V, V), "n_pn_gate": lambda V: (V, V)}),
    "NpGateModule": (np_gate, {"p_np_gate": lambda V: (V, V), "n_np_gate": lambda V: (V, V)}),
    "PGateModule": (p_gate, {"p_p_gate": lambda V: (V, V)}),
    "CorNNGateModule": (cor_nn_gate, {f"vocab_gate{i}_v1/{n}": (lambda V: (V, V)) if n == "weights" else (lambda V: (V,))
                                      for i in (1, 2, 3) for n in ("weights", "biases")}),
    "ContextGateV1": (context_gate_v1, {"vocab_gate_v1": lambda V: (V, V), "vocab_gate_bn_v1/beta": lambda V: (V,),
                                        "vocab_gate_bn_v1/gamma": lambda V: (V,), "vocab_gate_bn_v1/moving_mean": lambda V: (V,),
                                        "vocab_gate_bn_v1/moving_variance": lambda V: (V,)}),
}


def is_statistic(name):
    return name.endswith(("/moving_mean", "/moving_variance"))


def make_variables(shapes, seed):
    """fp32 variables with every vector away from its initial value (a test that leaves beta at 0 and gamma at 1 sees neither)"""
    g = torch.Generator().manual_seed(seed)
    p = {}
    for n, s in shapes.items():
        if n.endswith("/moving_variance"):
            p[n] = 0.5 + torch.rand(s, generator=g)
        elif n.endswith("/gamma"):
            p[n] = 1 + 0.3 * torch.randn(s, generator=g)
        elif len(s) == 1:
            p[n] = 0.3 * torch.randn(s, generator=g)
        else:
            p[n] = torch.randn(s, generator=g) * (2.0 / (s[0] + s[1])) ** 0.5 * 2
    return p


# FishMoeModel3 in training: LayerNorm/beta adds a constant to every column of the tensor that batch_normalization_2 centres over the
# batch, so its gradient -- the column sums of that batch norm's input gradient -- cancels to zero in exact arithmetic and the fp64
# reference holds rounding noise only.  Its error is taken relative to the norm of dLayerNorm/gamma: the same upstream gradient, the
# same shape, no cancellation.
CANCELLING = {"LayerNorm/beta": "LayerNorm/gamma"}


def gradient_error(name, got, want, g64, training):
    """|got - want|_2 over |want|_2 -- over the norm of the fp64 gradient of CANCELLING[name] for a gradient that cancels in training"""
    want = want.detach().double().cpu()
    scale = g64[CANCELLING[name]] if training and name in CANCELLING else want
    return float((got.detach().double().cpu() - want).norm() / scale.double().norm())


def cross_entropy(pred, labels, eps=1e-5):
    """losses.py:41-51: the mean over the batch of the row sums"""
    y = labels.to(pred.dtype)
    return (-(y * torch.log(pred + eps) + (1 - y) * torch.log(1 - pred + eps))).sum(dim=1).mean()
