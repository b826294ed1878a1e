"""Restatement of TriangulationMagnitudeNsCnnNetVladModule (video_pooling_modules.py:891-1105) for the tests: plain torch on the CPU, in
the dtype of its inputs (fp64 is the yardstick; the same code in fp32 gives the error an fp32 evaluation of the reference's own formulas
carries).  Independent of the package's modules and of the ops.  The front end is the sibling's (tests/_triangulation_v3_ref.embeddings:
tile, subtract, norm, normalise per anchor, roll the FEATURE axis, drop frame 0, norm, normalise per anchor again); here every frame's row
[relu(conv) | norm] is kept (:1016-1039) and handed to a NetVLAD per stream -- the reference's frame_level_models.NetVLAD.forward
(:2773-2824) and a bias-free matmul -- then batch norms, the fusion layer and a batch norm (:1062-1102)."""
import torch

from tests._triangulation_v2_ref import EPS, GRADS, convolve
from tests._triangulation_v3_ref import _norm, conditions, embeddings
from tests._triangulation_v3_ref import make_inputs as _v3_inputs

BN_EPS = 1e-3                                    # slim.batch_norm's default
PARTS = ("s_conv", "s_norm", "s_pad", "t_conv", "t_norm", "t_pad")
VLAD_VARS = ("cluster_weights", "cluster_bn/gamma", "cluster_bn/beta", "cluster_weights2", "hidden1_weights")

__all__ = ["EPS", "GRADS", "PARTS", "VLAD_VARS", "conditions", "make_inputs", "features", "split_parts", "features_and_grads",
           "netvlad_inputs", "netvlad", "netvlad_and_grads", "head", "module_and_grads", "model_variable_shapes"]


def padded(W, pad_to):
    return (W + pad_to - 1) // pad_to * pad_to


def make_inputs(B, T, D, K, F, seed, pad_to=1, anchor_scale=0.25):
    """_triangulation_v3_ref.make_inputs' frames, anchors and cnn weights (bit for bit), with N(0,1) upstream gradients for the two feature
    matrices [B*T, Wp] and [B*(T-1), Wp] from a generator of their own (the padding columns get one too: it must change nothing)."""
    x, anchors, cnn, _ = _v3_inputs(B, T, D, K, F, seed, anchor_scale)
    g = torch.Generator().manual_seed(104729 + seed)
    Wp = padded(K * F + K, pad_to)
    return x, anchors, cnn, [torch.randn(B * T, Wp, generator=g), torch.randn(B * (T - 1), Wp, generator=g)]


def features(x, anchors, cnn, T, pad_to=1):
    """-> (feat_s [B*T, Wp], feat_t [B*(T-1), Wp]): [relu(conv) | norm | zeros]."""
    e, h, q, p = embeddings(x, anchors, T)
    K = anchors.shape[1]
    out = []
    for v, sq, w_cnn in ((e, q, cnn[0]), (h, p, cnn[1])):
        f = torch.cat([torch.relu(convolve(v, w_cnn)), _norm(sq).reshape(-1, K)], 1)                 # :1019-1039
        Wp = padded(f.shape[1], pad_to)
        out.append(torch.cat([f, f.new_zeros(f.shape[0], Wp - f.shape[1])], 1))
    return out


def split_parts(feat_s, feat_t, K, F):
    KF, W = K * F, K * F + K
    parts = []
    for f in (feat_s, feat_t):
        parts += [f[:, :KF], f[:, KF:W], f[:, W:]]
    return dict(zip(PARTS, parts))


def features_and_grads(x, anchors, cnn, T, upstream, pad_to=1):
    """Values and the gradients GRADS by autograd in the inputs' dtype."""
    leaves = [t.detach().clone().requires_grad_(True) for t in (x, anchors, *cnn)]
    outs = features(leaves[0], leaves[1], leaves[2:], T, pad_to)
    loss = sum((o * g.to(o.dtype)).sum() for o, g in zip(outs, upstream))
    return [o.detach() for o in outs], list(torch.autograd.grad(loss, leaves))


# ---- loupe_modules.NetVLAD: frame_level_models.NetVLAD.forward (:2773-2824) + the projection ----
def _l2n(x, dim):
    return x * torch.rsqrt(torch.clamp((x * x).sum(dim=dim, keepdim=True), min=EPS))


def _batch_norm(v, gamma, beta):
    """slim.batch_norm in training mode on [n, C]: the batch mean and the BIASED batch variance."""
    mean = v.mean(0)
    var = ((v - mean) ** 2).mean(0)
    return (v - mean) * torch.rsqrt(var + BN_EPS) * gamma + beta


def netvlad_inputs(B, S, D, C, O, seed):
    """Rows shaped like the module's (non-negative, a share of exact zeros), the variables at their initialisers' scales with gamma and
    beta off their initial 1 and 0, and an N(0,1) upstream gradient [B, O]."""
    g = torch.Generator().manual_seed(15485863 + seed)
    x = torch.relu(torch.randn(B * S, D, generator=g)) * 0.3
    v = {"cluster_weights": torch.randn(D, C, generator=g) / D ** 0.5,
         "cluster_bn/gamma": 1.0 + 0.2 * torch.randn(C, generator=g),
         "cluster_bn/beta": 0.2 * torch.randn(C, generator=g),
         "cluster_weights2": torch.randn(1, D, C, generator=g) / D ** 0.5,
         "hidden1_weights": torch.randn(C * D, O, generator=g) / C ** 0.5}
    return x, v, torch.randn(B, O, generator=g)


def netvlad(x, v, S, mm=torch.matmul, centre=None):
    """x [(B*S), D], v: VLAD_VARS -> [B, O].  ``mm``: the product of the two NetVLAD stages (tests/_netvlad_ref.mm3: the split-bf16 model
    of the kernels).  ``centre`` (default: with any product but torch.matmul): the rows are centred on their mean first and
    cluster_weights2 moved alike, as loupe_modules.NetVLAD hands them to the kernels -- in exact arithmetic the same function (a
    training-mode batch norm removes the logits' shift), and what a model of the kernels' rounding has to see."""
    D, C = v["cluster_weights"].shape
    if (mm is not torch.matmul) if centre is None else centre:
        c = x.detach().mean(0, keepdim=True)
        x, v = x - c, dict(v, cluster_weights2=v["cluster_weights2"] - c.reshape(1, -1, 1))
    act = mm(x, v["cluster_weights"])                                                                # :2781
    act = _batch_norm(act, v["cluster_bn/gamma"], v["cluster_bn/beta"])                              # :2783-2789
    act = torch.softmax(act, dim=-1).reshape(-1, S, C)                                               # :2798-2801
    a = act.sum(dim=1, keepdim=True) * v["cluster_weights2"]                                         # :2803-2810
    vlad = mm(act.transpose(1, 2).contiguous(), x.reshape(-1, S, D)).transpose(1, 2) - a             # :2812-2817
    vlad = _l2n(_l2n(vlad, 1).reshape(-1, C * D), 1)                                                 # :2819-2822
    return vlad.matmul(v["hidden1_weights"])


def netvlad_and_grads(x, v, S, upstream, dtype, mm=torch.matmul, centre=None):
    """-> {"out", "dx", "d<variable>"} evaluated in ``dtype``."""
    xl = x.to(dtype).clone().requires_grad_(True)
    vl = {n: t.to(dtype).clone().requires_grad_(True) for n, t in v.items()}
    out = netvlad(xl, vl, S, mm, centre)
    grads = torch.autograd.grad((out * upstream.to(dtype)).sum(), [xl] + [vl[n] for n in VLAD_VARS])
    return dict(out=out.detach(), dx=grads[0], **{"d" + n: g for n, g in zip(VLAD_VARS, grads[1:])})


def head(feat_s, feat_t, T, v, add_relu=False, mm=torch.matmul):
    """The two streams' rows [.., W] -> [B, output_dim] with v the module's variables by name (training-mode batch norms; :1041-1102).
    ``mm``: the product of the NetVLAD stages, as in ``netvlad``."""
    def bn(t, scope):
        return _batch_norm(t, v[scope + "/gamma"], v[scope + "/beta"])

    def act(t):
        return torch.relu(t) if add_relu else t
    aggs = []
    for name, f, S in (("spatial", feat_s, T), ("temporal", feat_t, T - 1)):
        sub = {n: v[f"{name}_vlad/{n}"] for n in VLAD_VARS}
        aggs.append(act(bn(netvlad(f, sub, S, mm), f"{name}_activation_bn")))
    return act(bn(torch.cat(aggs, 1).matmul(v["spa_temp_fusion"]), "activation_bn"))


def module_and_grads(x, v, T, upstream, mm=torch.matmul):
    """The whole module in fp64 from v (name -> tensor; every entry but the moving statistics trainable): -> {"out", "dx", "grad <name>"}."""
    leaves = {n: t.double().clone().requires_grad_(True) for n, t in v.items() if not n.endswith(("moving_mean", "moving_variance"))}
    xl = x.double().clone().requires_grad_(True)
    feats = features(xl, leaves["anchor_weights"], [leaves["spatial_cnn_weights"], leaves["temporal_cnn_weights"]], T)
    out = head(*feats, T, leaves, mm=mm)
    grads = torch.autograd.grad((out * upstream.double()).sum(), [xl] + list(leaves.values()))
    return dict(out=out.detach(), dx=grads[0], **{"grad " + n: g for n, g in zip(leaves, grads[1:])})


# ---- JuhanTestModelV4 (frame_level_models.py:411-487) ----
def model_variable_shapes(kv, ka, fv, fa, hv, ha, ov, oa, clusters, feature_size=1152, batch_norm=True):
    """name -> shape of every variable of the model's two streams, in creation order (no batch norm before or behind them)."""
    shapes = {}

    def bn(scope, c):
        for name in ("beta", "gamma", "moving_mean", "moving_variance"):
            shapes[f"{scope}/{name}"] = (c,)
    for name, D, K, F, H, O in (("video", 1024, kv, fv, hv, ov), ("audio", feature_size - 1024, ka, fa, ha, oa)):
        s = f"{name}_triangulation_embedding"
        W = K * F + K
        shapes[f"{s}/anchor_weights"] = (D, K)
        shapes[f"{s}/spatial_cnn_weights"] = shapes[f"{s}/temporal_cnn_weights"] = (K, F, D)
        for vlad in ("spatial_vlad", "temporal_vlad"):
            shapes[f"{s}/{vlad}/cluster_weights"] = (W, clusters)
            if batch_norm:
                bn(f"{s}/{vlad}/cluster_bn", clusters)
            else:
                shapes[f"{s}/{vlad}/cluster_biases"] = (clusters,)
            shapes[f"{s}/{vlad}/cluster_weights2"] = (1, W, clusters)
            shapes[f"{s}/{vlad}/hidden1_weights"] = (clusters * W, H)
        if batch_norm:
            bn(f"{s}/spatial_activation_bn", H)
            bn(f"{s}/temporal_activation_bn", H)
        shapes[f"{s}/spa_temp_fusion"] = (2 * H, O)
        if batch_norm:
            bn(f"{s}/activation_bn", O)
    return shapes
