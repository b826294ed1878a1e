"""Restatement of TriangulationV5Module's pooling (video_pooling_modules.py:182-276) for the tests: plain torch on the CPU, in the dtype
of its inputs (fp64 is the yardstick; the same code in fp32 gives the error an fp32 evaluation of the reference's own formulas carries).
Independent of the package's module and of the op: it tiles, subtracts, rolls the FEATURE axis of the flattened [(B*T), K*D] embedding
(:216 -- ``tf.manip.roll(..., axis=1)``), drops frame 0, normalises, applies an einsum per anchor, appends the norms and takes the mean
and the mean of squared deviations over the frames.

``clamped=True`` states the convention of the fused op where a squared norm does not exceed 1e-12: e (h) is the clamped l2_normalize's
value and the tf.norm output of that (frame, anchor) carries no gradient (the reference would produce 0 / 0)."""
import math

import torch

EPS = 1e-12
PARTS = ("s_conv_mean", "s_norm_mean", "s_conv_var", "s_norm_var", "t_conv_mean", "t_norm_mean", "t_conv_var", "t_norm_var")
GRADS = ("dx", "danchors", "dcnn_s", "dcnn_t")


def glorot(shape, generator):
    """tf.contrib.layers.xavier_initializer (uniform): fan_in = shape[-2] * prod(shape[:-2]), fan_out = shape[-1] * prod(shape[:-2])."""
    rec = math.prod(shape[:-2])
    lim = math.sqrt(6.0 / ((shape[-2] + shape[-1]) * rec))
    return (torch.rand(shape, generator=generator) * 2 - 1) * lim


def make_inputs(B, T, D, K, F, seed):
    """N(0,1) frames, Glorot anchors and convolution weights, N(0,1) upstream gradients for both pools."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B * T, D, generator=g)
    anchors = glorot((D, K), g)
    cnn_s, cnn_t = glorot((K, F, D), g), glorot((K, F, D), g)
    up = [torch.randn(B, 2 * (K * F + K), generator=g) for _ in range(2)]
    return x, anchors, cnn_s, cnn_t, up


def _norm(v, clamped):
    q = (v * v).sum(dim=2)
    if not clamped:
        return q.sqrt()
    safe = q > EPS                                               # no gradient where the reference's would be 0 / 0
    return torch.where(safe, torch.where(safe, q, torch.ones_like(q)).sqrt(), q.detach().sqrt())


def _l2_normalize(v):
    return v * torch.rsqrt((v * v).sum(dim=2, keepdim=True).clamp_min(EPS))


def embeddings(x, anchors, T, clamped=False):
    """-> e [(B*T), K, D], n [(B*T), K], h [(B*(T-1)), K, D], tau [(B*(T-1)), K]."""
    D, K = anchors.shape
    spatial = x.repeat(1, K) - anchors.t().reshape(1, K * D)                     # :198-203
    spatial = spatial.reshape(-1, K, D)
    n = _norm(spatial, clamped)                                                 # :206
    e = _l2_normalize(spatial)                                                  # :208
    flat = e.reshape(-1, K * D)
    temporal = flat - torch.roll(flat, shifts=1, dims=1)                        # :216-217: the feature axis
    temporal = temporal.reshape(-1, T, K * D)[:, 1:]                            # :218-222: frame 0 dropped
    temporal = temporal.reshape(-1, K, D)
    tau = _norm(temporal, clamped)                                              # :224
    h = _l2_normalize(temporal)                                                 # :225
    return e, n, h, tau


def smallest_squared_norm(x, anchors, T):
    e, n, h, tau = embeddings(x, anchors, T)
    return float(torch.minimum((n * n).min(), (tau * tau).min()))


def moments(v):
    """[B, T', C] -> [B, 2C]: the mean and reduce_var (the mean of squared deviations from the mean) over the frames."""
    m = v.mean(dim=1, keepdim=True)
    return torch.cat([m.squeeze(1), ((v - m) ** 2).mean(dim=1)], 1)


def pools(x, anchors, cnn_s, cnn_t, T, clamped=False):
    """-> (spatial_pool, temporal_pool), each [B, 2 (K*F + K)] = [mean | var] of [conv (element k * F + f) | norm]."""
    K, F, D = cnn_s.shape
    e, n, h, tau = embeddings(x, anchors, T, clamped)
    so = torch.einsum("mkd,kfd->mkf", e, cnn_s).reshape(-1, T, K * F)            # :249-262
    to = torch.einsum("mkd,kfd->mkf", h, cnn_t).reshape(-1, T - 1, K * F)
    so = torch.cat([so, n.reshape(-1, T, K)], 2)                                # :266-267
    to = torch.cat([to, tau.reshape(-1, T - 1, K)], 2)
    return moments(so), moments(to)


def split_parts(spatial_pool, temporal_pool, K, F):
    """The eight parts (PARTS) of the two pools."""
    out = []
    for p in (spatial_pool, temporal_pool):
        W = K * F + K
        out += [p[:, :K * F], p[:, K * F:W], p[:, W:W + K * F], p[:, W + K * F:]]
    return dict(zip(PARTS, out))


def pools_and_grads(x, anchors, cnn_s, cnn_t, T, upstream, clamped=False):
    """Values and (dx, danchors, dcnn_s, dcnn_t) by autograd in the inputs' dtype."""
    leaves = [t.detach().clone().requires_grad_(True) for t in (x, anchors, cnn_s, cnn_t)]
    outs = pools(*leaves, T, clamped=clamped)
    loss = sum((o * g.to(o.dtype)).sum() for o, g in zip(outs, upstream))
    return [o.detach() for o in outs], list(torch.autograd.grad(loss, leaves))


def differenced_weight_identity_error(x, anchors, cnn_t, T):
    """max |to - (1/tau) (sum_d V e - Wt[k,f,0] e[t, (k-1) mod K, D-1])| with V[k,f,d] = Wt[k,f,d] - Wt[k,f,d+1], Wt[k,f,D] := 0."""
    K, F, D = cnn_t.shape
    e, n, h, tau = embeddings(x, anchors, T)
    to = torch.einsum("mkd,kfd->mkf", h, cnn_t)
    V = cnn_t - torch.cat([cnn_t[:, :, 1:], torch.zeros_like(cnn_t[:, :, :1])], 2)
    et = e.reshape(-1, T, K, D)[:, 1:].reshape(-1, K, D)
    last_of_previous = torch.roll(et[:, :, D - 1], shifts=1, dims=1)             # e[t, (k-1) mod K, D-1]
    alt = (torch.einsum("mkd,kfd->mkf", et, V) - cnn_t[:, :, 0].unsqueeze(0) * last_of_previous.unsqueeze(2)) / tau.unsqueeze(2)
    return float((alt - to).abs().max())


# ---- JuhanTestModelV5 (frame_level_models.py:491-606), restated functionally ----
def model_variable_shapes(vocab, kv, ka, fv, fa, hv, ha, ov, oa, feature_size=1152):
    """name -> shape of every variable of the model, in creation order (trainable and moving statistics)."""
    shapes = {}

    def bn(scope, c):
        for name in ("beta", "gamma", "moving_mean", "moving_variance"):
            shapes[f"{scope}/{name}"] = (c,)
    da = feature_size - 1024
    bn("video_bn", 1024)
    bn("audio_bn", da)
    for name, D, K, F, H, O in (("video", 1024, kv, fv, hv, ov), ("audio", da, ka, fa, ha, oa)):
        s = f"{name}_triangulation_embedding"
        W = 2 * (K * F + K)
        shapes[f"{s}/anchor_weights"] = (D, K)
        shapes[f"{s}/spatial_cnn_weights"] = shapes[f"{s}/temporal_cnn_weights"] = (K, F, D)
        bn(f"{s}/spatial_pool_bn", W)
        bn(f"{s}/temporal_pool_bn", W)
        shapes[f"{s}/spatial_hidden"] = shapes[f"{s}/temporal_hidden"] = (W, H)
        bn(f"{s}/spatial_activation_bn", H)
        bn(f"{s}/temporal_activation_bn", H)
        shapes[f"{s}/spatial_hidden2"] = shapes[f"{s}/temporal_hidden2"] = (H, H)
        bn(f"{s}/spatial_pool2_bn", H)
        bn(f"{s}/temporal_pool2_bn", H)
        shapes[f"{s}/spa_temp_fusion"] = (2 * H, O)
        bn(f"{s}/st_fuse_activation_bn", O)
    shapes["fc1_weights"] = (ov + oa, vocab)
    bn("fc1_activation_bn", vocab)
    for i in (2, 3):
        shapes[f"fc{i}_weights"] = (vocab, vocab)
        bn(f"fc{i}_activation_bn", vocab)
    shapes["fc4_weights"] = (vocab, vocab)
    shapes["fc4_bias"] = (vocab,)
    return shapes
