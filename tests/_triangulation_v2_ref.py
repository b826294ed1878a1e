"""Restatement of TriangulationNsCnnIndirectAttentionModule's pooling (video_pooling_modules.py:1156-1268, as resolved in SURVEY App. C39)
for the tests: plain torch on the CPU, in the dtype of its inputs (fp64 is the yardstick; the same code in fp32 gives the error an fp32
evaluation of the reference's own formulas carries).  Independent of the package's module and of the op: it tiles, subtracts, normalises
per anchor, rolls the FEATURE axis of the flattened [(B*T), K*D] embedding (:1185), drops frame 0, convolves per anchor, forms the relu'd
Gram's row sums over the frames of a clip, their softmax, the weighted mean divided by T' once more, and the unweighted mean of squared
deviations."""
import math

import torch

EPS = 1e-12
PARTS = ("s_mean", "s_var", "t_mean", "t_var")
GRADS = ("dx", "danchors", "dcnn_s", "dcnn_t")


def make_inputs(B, T, D, K, F, seed, anchor_scale=0.25):
    """Unit random frames, anchors = ``anchor_scale`` x orthonormal columns (QR of a normal draw), cnn weights N(0, 1 / (F D)), N(0,1)
    upstream gradients for both pools.  (At scale 1, the model's own initialisation, every Gram entry is positive.)  The frames are
    L2-normalised N(0,1) rows at D <= 128; a wider frame is such a row times one N(0,1) [128, D] matrix, normalised: dense rows from a
    128-dimensional subspace, whose inner products keep the standard deviation 1 / sqrt(128).  Isotropic rows at D = 1024 have 1 / 32,
    half the anchors' 0.25^2 offset, and leave about 2 % of a Gram's entries negative (measured: 0.02 to 0.03 over seeds 0 to 5 at
    (2, 30, 1024, 3)) where the relu mask wants 10 %."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B * T, min(D, 128), generator=g)
    if D > 128:
        x = x.matmul(torch.randn(128, D, generator=g))
    x = x / x.norm(dim=1, keepdim=True)
    qm, r = torch.linalg.qr(torch.randn(D, K, generator=g, dtype=torch.float64))
    anchors = (anchor_scale * qm * torch.sign(torch.diagonal(r))).float()
    cnn = [torch.randn(K, F, D, generator=g) / math.sqrt(F * D) for _ in range(2)]
    up = [torch.randn(B, 2 * K * F, generator=g) for _ in range(2)]
    return x, anchors, cnn, up


def embeddings(x, anchors, T):
    """-> spatial [(B*T), J], temporal [(B*(T-1)), J], the spatial squared norms [(B*T), K]."""
    D, K = anchors.shape
    spatial = x.repeat(1, K) - anchors.t().reshape(1, K * D)                     # :1164-1170
    spatial = spatial.reshape(-1, K, D)
    q = (spatial * spatial).sum(dim=2)
    spatial = spatial * torch.rsqrt(q.unsqueeze(2).clamp_min(EPS))               # :1175
    spatial = spatial.reshape(-1, K * D)
    temporal = spatial - torch.roll(spatial, shifts=1, dims=1)                   # :1185-1186: the feature axis
    temporal = temporal.reshape(-1, T, K * D)[:, 1:].reshape(-1, K * D)          # :1187-1192: frame 0 dropped
    return spatial, temporal, q


def attention(v):
    """[B, T', J] -> (G [B, T', T'], w [B, T'])  (:1201-1216 over the frames of a clip: C39)."""
    G = v.matmul(v.transpose(1, 2))
    return G, torch.softmax(torch.relu(G).sum(dim=2), dim=1)


def convolve(v, cnn):
    """[M, J], [K, F, D] -> [M, K * F], element k * F + f (:1237-1250)."""
    K, F, D = cnn.shape
    return torch.einsum("mkd,kfd->mkf", v.reshape(-1, K, D), cnn).reshape(-1, K * F)


def pools(x, anchors, cnn, T, self_attention=True, detail=False):
    """-> (spatial_pool, temporal_pool), each [B, 2 K F] = [mean | var]; ``detail``: also the Grams, the weights and q."""
    spatial, temporal, q = embeddings(x, anchors, T)
    J = spatial.shape[1]
    out, extra = [], []
    for v, w_cnn, Tz in ((spatial, cnn[0], T), (temporal, cnn[1], T - 1)):
        o = convolve(v, w_cnn).reshape(-1, Tz, w_cnn.shape[0] * w_cnn.shape[1])                                   # :1253-1254
        G, w = attention(v.reshape(-1, Tz, J))
        mean = (o * w.unsqueeze(2)).mean(dim=1) if self_attention else o.mean(dim=1)                             # :1257-1262
        var = ((o - o.mean(dim=1, keepdim=True)) ** 2).mean(dim=1)                                               # :1264-1265 reduce_var
        out.append(torch.cat([mean, var], 1))
        extra += [G, w]
    if detail:
        return out, extra, q
    return out


def split_parts(spatial_pool, temporal_pool):
    W = spatial_pool.shape[1] // 2
    return dict(zip(PARTS, (spatial_pool[:, :W], spatial_pool[:, W:], temporal_pool[:, :W], temporal_pool[:, W:])))


def pools_and_grads(x, anchors, cnn, T, upstream, self_attention=True):
    """Values and the gradients GRADS by autograd in the inputs' dtype."""
    leaves = [t.detach().clone().requires_grad_(True) for t in (x, anchors, *cnn)]
    outs = pools(leaves[0], leaves[1], leaves[2:], T, self_attention)
    loss = sum((o * g.to(o.dtype)).sum() for o, g in zip(outs, upstream))
    return [o.detach() for o in outs], list(torch.autograd.grad(loss, leaves))


def conditions(x, anchors, cnn, T):
    """On the fp64 restatement: the smallest spatial squared norm, the smallest |G| / max |G| over the clips of either Gram, the largest
    softmax weight over the clips with at least three rows (0 when there is none), and the smallest share of negative entries over the
    two Grams (the 1 x 1 temporal Gram and the spatial Gram at T = 2 left out: 1.0 when nothing is left)."""
    dt = torch.float64
    _, (Gs, ws, Gt, wt), q = pools(x.to(dt), anchors.to(dt), [c.to(dt) for c in cnn], T, True, detail=True)
    ratio = min(float((G.abs().flatten(1).min(dim=1).values / G.abs().flatten(1).max(dim=1).values).min()) for G in (Gs, Gt))
    weight = max([float(w.max()) for w in (ws, wt) if w.shape[1] >= 3], default=0.0)
    negative = min([float((G < 0).double().mean()) for G in (Gs, Gt) if G.shape[1] >= 3], default=1.0)
    return dict(smallest=float(q.min()), gram_ratio=ratio, weight=weight, negative=negative)


# ---- JuhanTestModelV2 (frame_level_models.py:158-268) ----
def model_variable_shapes(vocab, kv, ka, fv, fa, hv, ha, ov, oa, feature_size=1152, batch_norm=True):
    """name -> shape of every variable of the model's two streams and the joined batch norm, in creation order."""
    shapes = {}

    def bn(scope, c):
        if batch_norm:
            for name in ("beta", "gamma", "moving_mean", "moving_variance"):
                shapes[f"{scope}/{name}"] = (c,)
    da = feature_size - 1024
    for name, D, K, F, H, O in (("video", 1024, kv, fv, hv, ov), ("audio", da, ka, fa, ha, oa)):
        s = f"{name}_triangulation_embedding"
        shapes[f"{s}/anchor_weights"] = (D, K)
        shapes[f"{s}/spatial_cnn_weights"] = shapes[f"{s}/temporal_cnn_weights"] = (K, F, D)
        bn(f"{s}/spatial_pool_bn", 2 * K * F)
        bn(f"{s}/temporal_pool_bn", 2 * K * F)
        shapes[f"{s}/spatial_hidden"] = shapes[f"{s}/temporal_hidden"] = (2 * K * F, H)
        bn(f"{s}/spatial_activation_bn", H)
        bn(f"{s}/temporal_activation_bn", H)
        shapes[f"{s}/spa_temp_fusion"] = (2 * H, O)
        bn(f"{s}/activation_bn", O)
    bn("final_activation_bn", ov + oa)
    return shapes
