"""Restatement of TriangulationCnnClusterModel's pooling for the tests: plain torch on the CPU, in the dtype of its inputs (fp64 is the
yardstick; the same code in fp32 gives the error an fp32 evaluation of the reference's own formulas carries).
Built on tests/_triangulation_ref.py (embeddings, l2n) and tests/_soft_attention_ref.py (attention weights, make_inputs).

The embeddings e [B, T, K*D] and f [B, T-1, K*D] are MATERIALISED and the per-anchor convolution (video_pooling_modules.py:1345-1392,
``cnn_weights`` [K, F, D]) is applied to every frame BEFORE the pooling, in the reference's order:
    agg_d = (1/T) sum_t w[t] conv_d(e_t),  w = softmax_t(sum_s relu(<e_t, e_s>));      agg_t = (1/(T-1)) sum_t conv_t(f_t)
``mean_pool`` is the inner op's restatement (the pooled means without the convolution)."""
import math

import torch

from tests import _soft_attention_ref as S
from tests import _triangulation_ref as R

NAMES = ("agg_d", "agg_t")
GRADS = ("dx", "danchors", "dcnn_d", "dcnn_t")


def conv(v, cnn):
    """[B, T, K*D], [K, F, D] -> [B, T, K*F] (element k * F + j): matmul over [K, B*T, D] as :1386-1390."""
    K, F, D = cnn.shape
    B, T = v.shape[:2]
    out = v.reshape(B * T, K, D).transpose(0, 1).matmul(cnn.transpose(1, 2))     # [K, B*T, F]
    return out.transpose(0, 1).reshape(B, T, K * F)


def cnn_pool(x, anchors, cnn_d, cnn_t, T, scale=1.0):
    """Project, then pool -> (agg_d, agg_t), each [B, K*F]."""
    e, f = R.embeddings(x, anchors, T, scale)
    return S.attention_mean(e, conv(e, cnn_d)), conv(f, cnn_t).mean(dim=1)


def mean_pool(x, anchors, T, scale=1.0):
    """-> (m_d, m_t), each [B, K*D]."""
    e, f = R.embeddings(x, anchors, T, scale)
    return S.attention_mean(e, e), f.mean(dim=1)


def project(m, cnn):
    """Pool, then project: [B, K*D], [K, F, D] -> [B, K*F]."""
    K, F, D = cnn.shape
    return torch.einsum("bkd,kfd->bkf", m.reshape(-1, K, D), cnn).reshape(-1, K * F)


def gram_d(x, anchors, T, scale=1.0):
    return S.gram(R.embeddings(x, anchors, T, scale)[0])


def smallest_gram_d(x, anchors, T, scale=1.0):
    """The smallest |G_d| entry: the caller asserts that it is at least 1e-5 (a relu mask that flips between fp32 and fp64 moves dx by
    far more than any tolerance and says nothing about the code under test)."""
    return float(gram_d(x, anchors, T, scale).abs().min())


def make_weights(B, D, K, F, seed):
    """cnn_d, cnn_t [K, F, D] ~ N(0, 1 / (F D)) (the variables' initialisation) and N(0,1) upstream gradients for agg_d, agg_t [B, K*F]
    and for m_d, m_t [B, K*D]; a generator of their own, apart from the inputs'."""
    g = torch.Generator().manual_seed(1000 + seed)
    cnn = [torch.randn(K, F, D, generator=g) / math.sqrt(F * D) for _ in range(2)]
    up = [torch.randn(B, K * F, generator=g) for _ in range(2)]
    up_m = [torch.randn(B, K * D, generator=g) for _ in range(2)]
    return cnn[0], cnn[1], up, up_m


def cnn_pool_and_grads(x, anchors, cnn_d, cnn_t, T, upstream):
    """Values and (dx, danchors, dcnn_d, dcnn_t) by autograd in the inputs' dtype."""
    leaves = [t.detach().clone().requires_grad_(True) for t in (x, anchors, cnn_d, cnn_t)]
    outs = cnn_pool(*leaves, T)
    loss = sum((o * g.to(o.dtype)).sum() for o, g in zip(outs, upstream))
    return [o.detach() for o in outs], list(torch.autograd.grad(loss, leaves))


def mean_pool_and_grads(x, anchors, T, upstream):
    leaves = [t.detach().clone().requires_grad_(True) for t in (x, anchors)]
    outs = mean_pool(*leaves, T)
    loss = sum((o * g.to(o.dtype)).sum() for o, g in zip(outs, upstream))
    return [o.detach() for o in outs], list(torch.autograd.grad(loss, leaves))


# ---- TriangulationCnnClusterModel (frame_level_models.py:757-939 with the resolutions of SURVEY App. C22-C28), restated functionally ----
def model_variable_shapes(vocab, kv, ka, fv, fa, hv, ha, feature_size=1152):
    """name -> shape of every variable of the model, in creation order (trainable and moving statistics)."""
    shapes = {}

    def bn(scope, c):
        for n in ("beta", "gamma", "moving_mean", "moving_variance"):
            shapes[f"{scope}/{n}"] = (c,)
    da = feature_size - 1024
    bn("video_bn", 1024)
    bn("audio_bn", da)
    for name, D, K, F in (("video", 1024, kv, fv), ("audio", da, ka, fa)):
        scope = f"{name}_triangulation_embedding"
        shapes[f"{scope}/anchor_weights"] = (D, K)
        shapes[f"{scope}/{name}_d/cnn_weights"] = shapes[f"{scope}/{name}_t/cnn_weights"] = (K, F, D)
        bn(f"{scope}/agg_{name}_bn", 2 * K * F)
    shapes["video_hidden"] = (2 * kv * fv, hv)
    shapes["audio_hidden"] = (2 * ka * fa, ha)
    shapes["fully_connected/weights"] = (hv + ha, vocab)
    shapes["LayerNorm/beta"] = shapes["LayerNorm/gamma"] = (vocab,)
    for i in (1, 2):
        shapes[f"fully_connected_{i}/weights"] = (vocab, vocab)
        shapes[f"LayerNorm_{i}/beta"] = shapes[f"LayerNorm_{i}/gamma"] = (vocab,)
    shapes["fully_connected_3/weights"] = (vocab, vocab)
    shapes["fully_connected_3/biases"] = (vocab,)
    return shapes


def model_streams(p, raw, num_frames, frame_uniform):
    """S.model_streams: the batch-normalised (training mode) streams and their normalised anchors (the variable names agree)."""
    return S.model_streams(p, raw, num_frames, frame_uniform)


def model_loss(p, raw, num_frames, labels, frame_uniform, fc_l2=1e-8, penalty=1.0):
    """Training-mode forward in the dtype of ``p``: (predictions, label loss, final loss = label loss + penalty * regularisation)."""
    dt = next(iter(p.values())).dtype
    streams, T = model_streams(p, raw, num_frames, frame_uniform)
    acts = []
    for name, (xs, anchors) in zip(("video", "audio"), streams):
        scope = f"{name}_triangulation_embedding"
        agg_d, agg_t = cnn_pool(xs, anchors, p[f"{scope}/{name}_d/cnn_weights"], p[f"{scope}/{name}_t/cnn_weights"], T)
        a = R._bn_train(torch.cat([agg_d, agg_t], 1), p, f"{scope}/agg_{name}_bn")
        acts.append(a.matmul(p[name + "_hidden"]))
    h = torch.cat(acts, 1)
    weights = []
    for i in range(3):
        suffix = f"_{i}" if i else ""
        weights.append(f"fully_connected{suffix}/weights")
        h = torch.nn.functional.leaky_relu(R._layer_norm(h.matmul(p[weights[-1]]), p, "LayerNorm" + suffix), 0.2)
    weights.append("fully_connected_3/weights")
    pred = torch.sigmoid(h.matmul(p[weights[-1]]) + p["fully_connected_3/biases"])
    y = labels.to(dt)
    label_loss = (-(y * torch.log(pred + 10e-6) + (1 - y) * torch.log(1 - pred + 10e-6))).sum(dim=1).mean()
    reg = sum(fc_l2 * 0.5 * (p[n] ** 2).sum() for n in weights)
    return pred, label_loss, label_loss + penalty * reg


def model_smallest_gram(p, raw, num_frames, frame_uniform):
    """The smallest |G_d| over both streams of the model's own inputs."""
    streams, T = model_streams(p, raw, num_frames, frame_uniform)
    return min(smallest_gram_d(xs, anchors, T) for xs, anchors in streams)
