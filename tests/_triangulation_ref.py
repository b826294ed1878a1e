"""Restatement of the triangulation-embedding formulas for the tests: plain torch on the CPU, in the dtype of its inputs (fp64 is the
yardstick; the same code in fp32 gives the error an fp32 evaluation of the reference's own formulas carries).

Per (b, t, k):  r = x[b,t,:] - anchors[:,k];  e = s r rsqrt(max(sum r^2, 1e-12));  t >= 1: u = e[t] - e[t-1],
f = u rsqrt(max(sum u^2, 1e-12)); pooled over t: max and mean of e (T frames) and of f (T - 1 frames), laid out k-major.
The maximum belongs to the FIRST frame that attains it (argmax), in the value and in the gradient."""
import math

import torch

EPS = 1e-12


def l2n(x, dim):
    return x * torch.rsqrt(torch.clamp((x * x).sum(dim=dim, keepdim=True), min=EPS))


def embeddings(x, anchors, T, scale):
    """x [B*T, D], anchors [D, K] -> e [B, T, K*D], f [B, T-1, K*D] (element k*D + d)."""
    D, K = anchors.shape
    B = x.shape[0] // T
    r = x.reshape(B, T, 1, D) - anchors.t().reshape(1, 1, K, D)
    e = scale * l2n(r, 3)
    f = l2n(e[:, 1:] - e[:, :-1], 3)
    return e.reshape(B, T, K * D), f.reshape(B, T - 1, K * D)


def first_max(v):
    """max over dim 1 with the first index winning -> (values, indices)."""
    idx = v.argmax(dim=1, keepdim=True)
    return v.gather(1, idx).squeeze(1), idx.squeeze(1)


def pool(x, anchors, T, scale):
    """-> (max_d, mean_d, max_t, mean_t), each [B, K*D]."""
    e, f = embeddings(x, anchors, T, scale)
    return first_max(e)[0], e.mean(dim=1), first_max(f)[0], f.mean(dim=1)


def near_ties(x, anchors, T, scale, reach=1e-5):
    """Boolean [B, K*D] masks (for max_d, max_t): the runner-up over t lies within ``reach`` of the maximum without being equal to it
    (an exact tie -- identical frames -- is decided by the first-index rule on every side)."""
    out = []
    for v in embeddings(x, anchors, T, scale):
        if v.shape[1] < 2:
            out.append(torch.zeros(v.shape[0], v.shape[2], dtype=torch.bool))
            continue
        top = torch.topk(v, 2, dim=1).values
        gap = top[:, 0] - top[:, 1]
        out.append((gap < reach) & (gap > 0))
    return out


def pool_and_grads(x, anchors, T, scale, upstream):
    """Values and (dx, danchors) for the four upstream gradients, by autograd in the inputs' dtype."""
    x = x.detach().clone().requires_grad_(True)
    a = anchors.detach().clone().requires_grad_(True)
    outs = pool(x, a, T, scale)
    loss = sum((o * g.to(o.dtype)).sum() for o, g in zip(outs, upstream))
    dx, da = torch.autograd.grad(loss, [x, a])
    return [o.detach() for o in outs], dx, da


def make_inputs(B, T, D, K, seed):
    """N(0,1) frames, anchors N(0, 1/K) (the variable's initialisation), N(0,1) upstream gradients; fp32."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B * T, D, generator=g)
    anchors = torch.randn(D, K, generator=g) / math.sqrt(K)
    upstream = [torch.randn(B, K * D, generator=g) for _ in range(4)]
    return x, anchors, upstream


# ---- RegularizedTriangulationModel (frame_level_models.py:1148-1307 with the resolutions of SURVEY App. C17-C21), restated functionally ----
BN_EPS, LN_EPS = 1e-3, 1e-12


def model_variable_shapes(vocab, kv, ka, feature_size=1152):
    """name -> shape of every variable of the model, in creation order (trainable and moving statistics)."""
    shapes = {}

    def bn(scope, c):
        for n in ("beta", "gamma", "moving_mean", "moving_variance"):
            shapes[f"{scope}/{n}"] = (c,)
    bn("input_bn", feature_size)
    shapes["video_t_emb/anchor_weights"] = (1024, kv)
    shapes["audio_t_emb/anchor_weights"] = (feature_size - 1024, ka)
    dv, da = 2 * kv * 1024, 2 * ka * (feature_size - 1024)
    shapes["video_projection"] = (dv, 1024)
    bn("video_projection_bn", 1024)
    shapes["audio_projection"] = (da, 128)
    bn("audio_projection_bn", 128)
    shapes["temp_projection_1"] = (dv + da, 1152)
    bn("temp_projection_bn", 1152)
    shapes["dis_projection_2"] = (1152, 2048)
    bn("dis_activation_bn", 2048)
    shapes["temp_projection_2"] = (1152, 2048)
    bn("temp_activation_bn", 2048)
    shapes["fully_connected/weights"] = (4096, vocab)
    shapes["LayerNorm/beta"] = shapes["LayerNorm/gamma"] = (vocab,)
    shapes["fully_connected_1/weights"] = (vocab, vocab)
    shapes["LayerNorm_1/beta"] = shapes["LayerNorm_1/gamma"] = (vocab,)
    shapes["fully_connected_2/weights"] = (vocab, vocab)
    shapes["fully_connected_2/biases"] = (vocab,)
    return shapes


def is_trainable(name):
    return "moving_" not in name


def _bn_train(x, p, scope):
    mean = x.mean(dim=0)
    var = ((x - mean) ** 2).mean(dim=0)
    return (x - mean) * torch.rsqrt(var + BN_EPS) * p[scope + "/gamma"] + p[scope + "/beta"]


def _layer_norm(x, p, scope):
    mean = x.mean(dim=1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=1, keepdim=True)
    return (x - mean) * torch.rsqrt(var + LN_EPS) * p[scope + "/gamma"] + p[scope + "/beta"]


def model_loss(p, raw, num_frames, labels, frame_uniform, masks, iterations, l1=1e-5, l2=1.0, fc_l2=1e-8, penalty=1.0):
    """Training-mode forward in the dtype of ``p``: (predictions, label loss, final loss = label loss + penalty * regularisation)."""
    dt = next(iter(p.values())).dtype
    x = l2n(raw.to(dt), 2)                                                                     # train.py:262-264
    idx = (frame_uniform.float() * num_frames.reshape(-1, 1).float()).to(torch.int32).long()   # SampleRandomFrames, in fp32 as the model does
    x = x[torch.arange(x.shape[0]).unsqueeze(1), idx]
    B, T, F = x.shape
    x = _bn_train(x.reshape(-1, F), p, "input_bn")
    agg_d, agg_t = [], []
    for scope, cols in (("video_t_emb", slice(0, 1024)), ("audio_t_emb", slice(1024, None))):
        a = p[scope + "/anchor_weights"]
        K = a.shape[1]
        # the weighted embedding: every anchor block l2-normalised, then the whole row of K blocks once more
        e, _ = embeddings(x[:, cols], a, T, 1.0)
        e = l2n(e, 2)
        D = a.shape[0]
        f = l2n((e[:, 1:] - e[:, :-1]).reshape(B, T - 1, K, D), 3).reshape(B, T - 1, K * D)
        agg_d.append(torch.cat([first_max(e)[0], e.mean(dim=1)], 1))
        agg_t.append(torch.cat([first_max(f)[0], f.mean(dim=1)], 1))
    video = _bn_train(agg_d[0].matmul(p["video_projection"]), p, "video_projection_bn")
    audio = _bn_train(agg_d[1].matmul(p["audio_projection"]), p, "audio_projection_bn")
    temp = _bn_train(torch.cat(agg_t, 1).matmul(p["temp_projection_1"]), p, "temp_projection_bn")
    dis = _bn_train(torch.cat([video, audio], 1).matmul(p["dis_projection_2"]), p, "dis_activation_bn")
    tmp = _bn_train(temp.matmul(p["temp_projection_2"]), p, "temp_activation_bn")
    h = torch.cat([dis, tmp], 1)
    h = torch.nn.functional.leaky_relu(_layer_norm(h.matmul(p["fully_connected/weights"]), p, "LayerNorm"), 0.2)
    h = h * masks["fc1"].to(dt) / 0.5
    h = torch.nn.functional.leaky_relu(_layer_norm(h.matmul(p["fully_connected_1/weights"]), p, "LayerNorm_1"), 0.2)
    h = h * masks["fc2"].to(dt) / 0.5
    pred = torch.sigmoid(h.matmul(p["fully_connected_2/weights"]) + p["fully_connected_2/biases"])
    y = labels.to(dt)
    label_loss = (-(y * torch.log(pred + 10e-6) + (1 - y) * torch.log(1 - pred + 10e-6))).sum(dim=1).mean()
    reg = sum(l1 * p[n].abs().sum() + l2 * 0.5 * (p[n] ** 2).sum() for n in ("dis_projection_2", "temp_projection_2"))
    reg = reg + sum(fc_l2 * 0.5 * (p[n] ** 2).sum() for n in ("fully_connected/weights", "fully_connected_1/weights", "fully_connected_2/weights"))
    return pred, label_loss, label_loss + penalty * reg
