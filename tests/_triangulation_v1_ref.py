"""Restatement of TriangulationCnnIndirectAttentionModule's pooling (video_pooling_modules.py:476-571) for the tests: plain torch on the
CPU, in the dtype of its inputs (fp64 is the yardstick; the same code in fp32 gives the error an fp32 evaluation of the reference's own
formulas carries).  Independent of the package's module and of the op: it tiles, subtracts, normalises per anchor, rolls the FEATURE
axis of the flattened [(B*T), K*D] embedding (:506), drops frame 0, applies slim.batch_norm's training-mode (or, with ``stats``,
inference-mode) formula per feature, forms the relu'd Gram's row sums, their softmax, the weighted mean divided by T' once more, and the
unweighted mean of squared deviations."""
import math

import torch

EPS = 1e-12
BN_EPS = 1e-3
PARTS = ("s_mean", "s_var", "t_mean", "t_var")
GRADS = ("dx", "danchors", "dgamma_s", "dbeta_s", "dgamma_t", "dbeta_t")


def make_inputs(B, T, D, K, seed):
    """L2-normalised N(0,1) frames, anchors N(0, 1/K), gamma = U(0.5, 1.5) / sqrt(J), beta = 0.1 N(0,1) / sqrt(J), N(0,1) upstream
    gradients for both pools.  (At gamma = 1 the Gram's row sums are about J and the softmax is one-hot to rounding.)"""
    g = torch.Generator().manual_seed(seed)
    J = K * D
    x = torch.randn(B * T, D, generator=g)
    x = x / x.norm(dim=1, keepdim=True)
    anchors = torch.randn(D, K, generator=g) / math.sqrt(K)
    affine = []
    for _ in range(2):
        affine.append((0.5 + torch.rand(J, generator=g)) / math.sqrt(J))
        affine.append(0.1 * torch.randn(J, generator=g) / math.sqrt(J))
    up = [torch.randn(B, 2 * J, generator=g) for _ in range(2)]
    return x, anchors, affine, up


def embeddings(x, anchors, T):
    """-> spatial [(B*T), J], temporal [(B*(T-1)), J], the spatial squared norms [(B*T), K]."""
    D, K = anchors.shape
    spatial = x.repeat(1, K) - anchors.t().reshape(1, K * D)                     # :485-491
    spatial = spatial.reshape(-1, K, D)
    q = (spatial * spatial).sum(dim=2)
    spatial = spatial * torch.rsqrt(q.unsqueeze(2).clamp_min(EPS))               # :496
    spatial = spatial.reshape(-1, K * D)
    temporal = spatial - torch.roll(spatial, shifts=1, dims=1)                   # :506-507: the feature axis
    temporal = temporal.reshape(-1, T, K * D)[:, 1:].reshape(-1, K * D)          # :508-513: frame 0 dropped
    return spatial, temporal, q


def batch_norm(v, gamma, beta, stats):
    """slim.batch_norm on a rank-2 tensor: batch mean and BIASED variance in training mode, the given (mean, var) otherwise."""
    if stats is None:
        mean = v.mean(dim=0)
        var = ((v - mean) ** 2).mean(dim=0)
    else:
        mean, var = stats
    return (v - mean) * torch.rsqrt(var + BN_EPS) * gamma + beta, mean, var


def attention(v):
    """[B, T', J] -> (G [B, T', T'], w [B, T'])  (:539-554)."""
    G = v.matmul(v.transpose(1, 2))
    return G, torch.softmax(torch.relu(G).sum(dim=2), dim=1)


def pools(x, anchors, affine, T, self_attention=True, use_bn=True, stats=None, detail=False):
    """-> (spatial_pool, temporal_pool), each [B, 2 J] = [mean | var]; ``detail``: also the Grams, the weights, q and the batch statistics."""
    spatial, temporal, q = embeddings(x, anchors, T)
    J = spatial.shape[1]
    bstats = []
    if use_bn:
        spatial, m, v = batch_norm(spatial, affine[0], affine[1], None if stats is None else stats[0:2])      # :518-523
        bstats += [m, v]
        temporal, m, v = batch_norm(temporal, affine[2], affine[3], None if stats is None else stats[2:4])    # :525-530
        bstats += [m, v]
    out, extra = [], []
    for v, Tz in ((spatial.reshape(-1, T, J), T), (temporal.reshape(-1, T - 1, J), T - 1)):
        G, w = attention(v)
        mean = (v * w.unsqueeze(2)).mean(dim=1) if self_attention else v.mean(dim=1)                            # :560-565
        var = ((v - v.mean(dim=1, keepdim=True)) ** 2).mean(dim=1)                                               # :567-568 reduce_var
        out.append(torch.cat([mean, var], 1))
        extra += [G, w]
    if detail:
        return out, extra, q, bstats
    return out


def batch_statistics(x, anchors, T):
    """(mean_s, var_s, mean_t, var_t) of the raw embeddings: what the op returns as batch_stats whatever it normalises with."""
    spatial, temporal, _ = embeddings(x, anchors, T)
    return [spatial.mean(0), ((spatial - spatial.mean(0)) ** 2).mean(0), temporal.mean(0), ((temporal - temporal.mean(0)) ** 2).mean(0)]


def split_parts(spatial_pool, temporal_pool):
    J = spatial_pool.shape[1] // 2
    return dict(zip(PARTS, (spatial_pool[:, :J], spatial_pool[:, J:], temporal_pool[:, :J], temporal_pool[:, J:])))


def pools_and_grads(x, anchors, affine, T, upstream, self_attention=True, use_bn=True, stats=None):
    """Values and the gradients GRADS (the four affine ones only with batch norm) by autograd in the inputs' dtype."""
    leaves = [t.detach().clone().requires_grad_(True) for t in (x, anchors, *(affine if use_bn else ()))]
    outs = pools(leaves[0], leaves[1], leaves[2:], T, self_attention, use_bn, stats)
    loss = sum((o * g.to(o.dtype)).sum() for o, g in zip(outs, upstream))
    return [o.detach() for o in outs], list(torch.autograd.grad(loss, leaves))


def conditions(x, anchors, affine, T, use_bn=True, stats=None):
    """On the fp64 restatement: the smallest spatial squared norm, the smallest |G| / max |G| over the clips of either Gram, and the
    largest softmax weight over the clips with at least three rows (0 when there is none)."""
    dt = torch.float64
    st = None if stats is None else [s.to(dt) for s in stats]
    _, (Gs, ws, Gt, wt), q, _ = pools(x.to(dt), anchors.to(dt), [a.to(dt) for a in affine], T, True, use_bn, st, detail=True)
    ratio = min(float((G.abs().flatten(1).min(dim=1).values / G.abs().flatten(1).max(dim=1).values).min()) for G in (Gs, Gt))
    weight = max([float(w.max()) for w in (ws, wt) if w.shape[1] >= 3], default=0.0)
    return dict(smallest=float(q.min()), gram_ratio=ratio, weight=weight)


# ---- JuhanTestModelV1 (frame_level_models.py:59-154) ----
def model_variable_shapes(vocab, kv, ka, hv, ha, ov, oa, feature_size=1152, batch_norm=True):
    """name -> shape of every variable of the model, in creation order (trainable and moving statistics)."""
    shapes = {}

    def bn(scope, c):
        if batch_norm:
            for name in ("beta", "gamma", "moving_mean", "moving_variance"):
                shapes[f"{scope}/{name}"] = (c,)
    da = feature_size - 1024
    for name, D, K, H, O in (("video", 1024, kv, hv, ov), ("audio", da, ka, ha, oa)):
        s = f"{name}_triangulation_embedding"
        J = K * D
        shapes[f"{s}/anchor_weights"] = (D, K)
        bn(f"{s}/spatial_bn", J)
        bn(f"{s}/temporal_bn", J)
        shapes[f"{s}/spatial_hidden"] = shapes[f"{s}/temporal_hidden"] = (2 * J, H)
        bn(f"{s}/spatial_activation_bn", H)
        bn(f"{s}/temporal_activation_bn", H)
        shapes[f"{s}/spa_temp_fusion"] = (2 * H, O)
        bn(f"{s}/activation_bn", O)
    return shapes
