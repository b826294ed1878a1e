"""Restatement of the soft-attention pooling of the triangulation embedding for the tests: plain torch on the CPU, in the dtype of its
inputs (fp64 is the yardstick; the same code in fp32 gives the error an fp32 evaluation of the reference's own formulas carries).
Built on tests/_triangulation_ref.py (embeddings, first_max, l2n, make_inputs).

With v = e over the T frames or v = f over the T - 1 frame differences (aggregation_modules.py:84-108):
    G[t,s] = <v_t, v_s> over all K*D;  l[t] = sum_s relu(G[t,s]);  w = softmax_t(l);  mean = (1/T') sum_t w[t] v_t;  max = max_t v_t
The maximum belongs to the FIRST frame that attains it, in the value and in the gradient; relu'(0) = 0."""
import torch

from tests import _triangulation_ref as R

NAMES = ("mean_d", "max_d", "mean_t", "max_t")


def gram(v):
    """[B, T, F] -> [B, T, T]."""
    return v.matmul(v.transpose(1, 2))


def attention_weights(v):
    """-> [B, T, 1]."""
    return torch.softmax(torch.relu(gram(v)).sum(dim=2, keepdim=True), dim=1)


def attention_mean(t_inputs, c_inputs):
    return (c_inputs * attention_weights(t_inputs)).mean(dim=1)


def pool_embeddings(e, f):
    """-> (mean_d, max_d, mean_t, max_t), each [B, K*D]."""
    return attention_mean(e, e), R.first_max(e)[0], attention_mean(f, f), R.first_max(f)[0]


def pool(x, anchors, T, scale=1.0):
    return pool_embeddings(*R.embeddings(x, anchors, T, scale))


def grams(x, anchors, T, scale=1.0):
    """-> (G_d [B, T, T], G_t [B, T-1, T-1])."""
    return tuple(gram(v) for v in R.embeddings(x, anchors, T, scale))


def near_zero_gram(x, anchors, T, reach=1e-5, scale=1.0, nonzero_only=False):
    """The smallest |G| over both kinds (``nonzero_only``: over the entries that are not exactly zero).  The caller asserts that it is
    at least ``reach`` (entries nearer to zero than that are printed): a relu mask that flips between fp32 and fp64 moves dx by far
    more than any tolerance and says nothing about the code under test."""
    smallest = float("inf")
    for g in grams(x, anchors, T, scale):
        a = g.abs()
        if nonzero_only:
            a = a[a > 0]
        if a.numel():
            smallest = min(smallest, float(a.min()))
            if float(a.min()) < reach:
                print(f"[soft attention] a Gram entry {float(a.min()):.3e} lies within {reach:.0e} of zero")
    return smallest


def pool_and_grads(x, anchors, T, upstream, scale=1.0):
    """Values and (dx, danchors) for the four upstream gradients (order of NAMES), by autograd in the inputs' dtype."""
    x = x.detach().clone().requires_grad_(True)
    a = anchors.detach().clone().requires_grad_(True)
    outs = pool(x, a, T, scale)
    loss = sum((o * g.to(o.dtype)).sum() for o, g in zip(outs, upstream))
    dx, da = torch.autograd.grad(loss, [x, a])
    return [o.detach() for o in outs], dx, da


def make_inputs(B, T, D, K, seed):
    """R.make_inputs with the anchors L2-normalised over axis 0 (what TriangulationEmbedding hands on); scale 1."""
    x, anchors, upstream = R.make_inputs(B, T, D, K, seed)
    return x, R.l2n(anchors, 0), upstream


# ---- SoftAttentionTriangulationModel (frame_level_models.py:965-1145 with the resolutions of SURVEY App. C22-C25), restated functionally ----
def model_variable_shapes(vocab, kv, ka, bv, ba, feature_size=1152):
    """name -> shape of every variable of the model, in creation order (trainable and moving statistics)."""
    shapes = {}

    def bn(scope, c):
        for n in ("beta", "gamma", "moving_mean", "moving_variance"):
            shapes[f"{scope}/{n}"] = (c,)
    da = feature_size - 1024
    bn("video_bn", 1024)
    bn("audio_bn", da)
    shapes["video_triangulation_embedding/anchor_weights"] = (1024, kv)
    shapes["audio_triangulation_embedding/anchor_weights"] = (da, ka)
    for name, dim, units in (("video", 2 * kv * 1024, bv), ("audio", 2 * ka * da, ba)):
        shapes[f"{name}_d_projection"] = shapes[f"{name}_t_projection"] = (dim, units)
    for name, units in (("video", bv), ("audio", ba)):
        bn(f"{name}_d_activation_bn", units)
        bn(f"{name}_t_activation_bn", units)
    shapes["video_projection"] = (2 * bv, bv)
    shapes["audio_projection"] = (2 * ba, ba)
    bn("video_activation_bn", bv)
    bn("audio_activation_bn", ba)
    shapes["fully_connected/weights"] = (bv + ba, vocab)
    shapes["LayerNorm/beta"] = shapes["LayerNorm/gamma"] = (vocab,)
    for i in (1, 2):
        shapes[f"fully_connected_{i}/weights"] = (vocab, vocab)
        shapes[f"LayerNorm_{i}/beta"] = shapes[f"LayerNorm_{i}/gamma"] = (vocab,)
    shapes["fully_connected_3/weights"] = (vocab, vocab)
    shapes["fully_connected_3/biases"] = (vocab,)
    return shapes


def model_streams(p, raw, num_frames, frame_uniform):
    """The batch-normalised (training mode) streams and their normalised anchors: [(x [B*T, D], anchors [D, K]), ...], T."""
    dt = next(iter(p.values())).dtype
    x = R.l2n(raw.to(dt), 2)                                                                   # train.py:262-264
    idx = (frame_uniform.float() * num_frames.reshape(-1, 1).float()).to(torch.int32).long()   # SampleRandomFrames, in fp32 as the model does
    x = x[torch.arange(x.shape[0]).unsqueeze(1), idx]
    B, T, F = x.shape
    x = x.reshape(-1, F)
    out = []
    for name, cols in (("video", slice(0, 1024)), ("audio", slice(1024, None))):
        xs = R._bn_train(x[:, cols], p, name + "_bn")
        out.append((xs, R.l2n(p[name + "_triangulation_embedding/anchor_weights"], 0)))
    return out, T


def model_loss(p, raw, num_frames, labels, frame_uniform, fc_l2=1e-8, penalty=1.0):
    """Training-mode forward in the dtype of ``p``: (predictions, label loss, final loss = label loss + penalty * regularisation)."""
    dt = next(iter(p.values())).dtype
    streams, T = model_streams(p, raw, num_frames, frame_uniform)
    acts = []
    for name, (xs, anchors) in zip(("video", "audio"), streams):
        mean_d, max_d, mean_t, max_t = pool(xs, anchors, T)
        d = R._bn_train(torch.cat([mean_d, max_d], 1).matmul(p[name + "_d_projection"]), p, name + "_d_activation_bn")
        t = R._bn_train(torch.cat([mean_t, max_t], 1).matmul(p[name + "_t_projection"]), p, name + "_t_activation_bn")
        acts.append(R._bn_train(torch.cat([d, t], 1).matmul(p[name + "_projection"]), p, name + "_activation_bn"))
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
    """The smallest |G| over both streams and both kinds of the model's own inputs."""
    streams, T = model_streams(p, raw, num_frames, frame_uniform)
    return min(near_zero_gram(xs, anchors, T) for xs, anchors in streams)
