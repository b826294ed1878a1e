"""Restatement of TriangulationMagnitudeNsCnnIndirectAttentionModule's pooling (video_pooling_modules.py:684-814, the attention Gram as
resolved in SURVEY App. C39) for the tests: plain torch on the CPU, in the dtype of its inputs (fp64 is the yardstick; the same code in
fp32 gives the error an fp32 evaluation of the reference's own formulas carries).  Independent of the package's module and of the op: it
tiles, subtracts, takes the norm and normalises per anchor (:698-709), rolls the FEATURE axis of the flattened [(B*T), K*D] embedding
(:718), drops frame 0, takes the norm and normalises per anchor again (:725-732), forms the relu'd Grams' row sums over the frames of a
clip and their softmax, convolves per anchor, rectifies (:793-794), appends the norm columns (:799-801), and takes the weighted mean
divided by T' once more and the unweighted mean of squared deviations."""
import torch

from tests._triangulation_v2_ref import EPS, GRADS, attention, convolve
from tests._triangulation_v2_ref import make_inputs as _v2_inputs

PARTS = ("s_mean_conv", "s_mean_norm", "s_var_conv", "s_var_norm", "t_mean_conv", "t_mean_norm", "t_var_conv", "t_var_norm")


def make_inputs(B, T, D, K, F, seed, anchor_scale=0.25, add_norm=True):
    """_triangulation_v2_ref.make_inputs' frames, anchors and cnn weights, with N(0,1) upstream gradients for the pools of this module:
    [B, 2 (K*F + K)] each (drawn from a generator of their own, so the other tensors are V2's bit for bit)."""
    x, anchors, cnn, _ = _v2_inputs(B, T, D, K, F, seed, anchor_scale)
    g = torch.Generator().manual_seed(7919 + seed)
    W = K * F + (K if add_norm else 0)
    return x, anchors, cnn, [torch.randn(B, 2 * W, generator=g) for _ in range(2)]


def embeddings(x, anchors, T):
    """-> e [(B*T), J], h [(B*(T-1)), J], the squared norms q [(B*T), K] and p [(B*(T-1)), K]."""
    D, K = anchors.shape
    spatial = x.repeat(1, K) - anchors.t().reshape(1, K * D)                     # :692-698
    spatial = spatial.reshape(-1, K, D)                                          # :701
    q = (spatial * spatial).sum(dim=2)                                           # :702 (tf.norm = sqrt of it)
    spatial = spatial * torch.rsqrt(q.unsqueeze(2).clamp_min(EPS))               # :706
    spatial = spatial.reshape(-1, K * D)
    temporal = spatial - torch.roll(spatial, shifts=1, dims=1)                   # :718-719: the feature axis
    temporal = temporal.reshape(-1, T, K * D)[:, 1:].reshape(-1, K, D)           # :720-725: frame 0 dropped
    p = (temporal * temporal).sum(dim=2)                                         # :726
    temporal = temporal * torch.rsqrt(p.unsqueeze(2).clamp_min(EPS))             # :732
    return spatial, temporal.reshape(-1, K * D), q, p


def _norm(sq):
    """sqrt with the gradient defined as zero where the squared norm does not exceed EPS (the reference: 0 / 0)."""
    safe = sq > EPS
    return torch.where(safe, torch.sqrt(torch.where(safe, sq, torch.ones_like(sq))), torch.sqrt(sq.detach()))


def pools(x, anchors, cnn, T, self_attention=True, add_norm=True, detail=False):
    """-> (spatial_pool, temporal_pool), each [B, 2 W] = [mean | var], W = K F + K; ``detail``: also the Grams, the weights, q, p and the
    convolutions' pre-activations."""
    spatial, temporal, q, p = embeddings(x, anchors, T)
    J = spatial.shape[1]
    K = anchors.shape[1]
    out, extra, pre = [], [], []
    for v, sq, w_cnn, Tz in ((spatial, q, cnn[0], T), (temporal, p, cnn[1], T - 1)):
        a = convolve(v, w_cnn)                                                                                   # :777-791
        pre.append(a)
        o = torch.relu(a).reshape(-1, Tz, w_cnn.shape[0] * w_cnn.shape[1])                                       # :793-797
        if add_norm:
            o = torch.cat([o, _norm(sq).reshape(-1, Tz, K)], 2)                                                  # :799-801
        G, w = attention(v.reshape(-1, Tz, J))                                                                   # :741-756 (C39)
        mean = (o * w.unsqueeze(2)).mean(dim=1) if self_attention else o.mean(dim=1)                             # :803-808
        var = ((o - o.mean(dim=1, keepdim=True)) ** 2).mean(dim=1)                                               # :810-811 reduce_var
        out.append(torch.cat([mean, var], 1))
        extra += [G, w]
    if detail:
        return out, extra, q, p, pre
    return out


def split_parts(spatial_pool, temporal_pool, KF):
    """The eight PARTS; without the norm columns (W == KF) the four *_norm parts are empty."""
    W = spatial_pool.shape[1] // 2
    parts = []
    for pool in (spatial_pool, temporal_pool):
        parts += [pool[:, :KF], pool[:, KF:W], pool[:, W:W + KF], pool[:, W + KF:]]
    return dict(zip(PARTS, parts))


def pools_and_grads(x, anchors, cnn, T, upstream, self_attention=True, add_norm=True):
    """Values and the gradients GRADS by autograd in the inputs' dtype."""
    leaves = [t.detach().clone().requires_grad_(True) for t in (x, anchors, *cnn)]
    outs = pools(leaves[0], leaves[1], leaves[2:], T, self_attention, add_norm)
    loss = sum((o * g.to(o.dtype)).sum() for o, g in zip(outs, upstream))
    return [o.detach() for o in outs], list(torch.autograd.grad(loss, leaves))


def conditions(x, anchors, cnn, T):
    """On the fp64 restatement: the smallest squared norm (q and p alike), the smallest |G| / max |G| over the clips of either Gram, the
    largest softmax weight over the clips with at least three rows (0 when there is none), the smallest share of negative entries over
    the two Grams (the 1 x 1 temporal Gram and the spatial Gram at T = 2 left out: 1.0 when nothing is left), and of the convolutions'
    pre-activations the smallest |a| / max |a| and the smallest share of negative ones over the two streams."""
    dt = torch.float64
    _, (Gs, ws, Gt, wt), q, p, pre = pools(x.to(dt), anchors.to(dt), [c.to(dt) for c in cnn], T, True, True, detail=True)
    ratio = min(float((G.abs().flatten(1).min(dim=1).values / G.abs().flatten(1).max(dim=1).values).min()) for G in (Gs, Gt))
    weight = max([float(w.max()) for w in (ws, wt) if w.shape[1] >= 3], default=0.0)
    negative = min([float((G < 0).double().mean()) for G in (Gs, Gt) if G.shape[1] >= 3], default=1.0)
    return dict(smallest=min(float(q.min()), float(p.min())), gram_ratio=ratio, weight=weight, negative=negative,
                conv_ratio=min(float(a.abs().min() / a.abs().max()) for a in pre),
                conv_negative=min(float((a < 0).double().mean()) for a in pre))


# ---- JuhanTestModelV3 (frame_level_models.py:302-378) ----
def model_variable_shapes(vocab, kv, ka, fv, fa, hv, ha, ov, oa, feature_size=1152, batch_norm=True):
    """name -> shape of every variable of the model's two streams, in creation order (no batch norm before or behind them)."""
    shapes = {}

    def bn(scope, c):
        if batch_norm:
            for name in ("beta", "gamma", "moving_mean", "moving_variance"):
                shapes[f"{scope}/{name}"] = (c,)
    da = feature_size - 1024
    for name, D, K, F, H, O in (("video", 1024, kv, fv, hv, ov), ("audio", da, ka, fa, ha, oa)):
        s = f"{name}_triangulation_embedding"
        W = K * F + K
        shapes[f"{s}/anchor_weights"] = (D, K)
        shapes[f"{s}/spatial_cnn_weights"] = shapes[f"{s}/temporal_cnn_weights"] = (K, F, D)
        bn(f"{s}/spatial_pool_bn", 2 * W)
        bn(f"{s}/temporal_pool_bn", 2 * W)
        shapes[f"{s}/spatial_hidden"] = shapes[f"{s}/temporal_hidden"] = (2 * W, H)
        bn(f"{s}/spatial_activation_bn", H)
        bn(f"{s}/temporal_activation_bn", H)
        shapes[f"{s}/spa_temp_fusion"] = (2 * H, O)
        bn(f"{s}/activation_bn", O)
    return shapes
