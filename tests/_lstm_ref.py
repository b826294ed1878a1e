"""Restatement of TF1's BasicLSTMCell(H, forget_bias=1.0) under tf.nn.dynamic_rnn(sequence_length=...), of rnn_modules'
LstmLastHiddenModule / LstmConcatAverageModule and of TriangulationRelationalModel (frame_level_models.py:1511-1630) in plain torch,
written from the semantics and never calling the package.  Every function computes in the dtype of its inputs: fp64 is the reference,
fp32 on the CPU gives the evaluation error err32 the GPU bounds are built from.  Gradients come from autograd.

    z = [x_t, h] kernel + bias, columns gate-major i | j | f | o;  c' = c sigmoid(f + forget_bias) + sigmoid(i) tanh(j);
    h' = tanh(c') sigmoid(o);  zero initial state;  for t >= min(lengths[b], T) the state is copied through and outputs[b, t] = 0."""
import math

import torch

CELL = "rnn/multi_rnn_cell/cell_%d/basic_lstm_cell/"
BN_EPS = 1e-3
HIDDEN = 2048


def lstm_layer(x, kernel, bias, lengths, forget_bias=1.0):
    """x [B, T, In], kernel [In + H, 4H], bias [4H], lengths [B] -> (outputs [B, T, H], h_last, c_last)."""
    B, T, _ = x.shape
    H = bias.numel() // 4
    h = torch.zeros(B, H, dtype=x.dtype)
    c = torch.zeros(B, H, dtype=x.dtype)
    outputs = []
    for t in range(T):
        z = torch.cat([x[:, t], h], 1) @ kernel + bias
        i, j, f, o = z[:, :H], z[:, H:2 * H], z[:, 2 * H:3 * H], z[:, 3 * H:]
        c_new = c * torch.sigmoid(f + forget_bias) + torch.sigmoid(i) * torch.tanh(j)
        h_new = torch.tanh(c_new) * torch.sigmoid(o)
        live = (lengths > t).reshape(B, 1)
        outputs.append(torch.where(live, h_new, torch.zeros_like(h_new)))
        h = torch.where(live, h_new, h)
        c = torch.where(live, c_new, c)
    return torch.stack(outputs, 1), h, c


def make_inputs(B, T, In, H, seed, lengths=None):
    """-> (x, kernel, bias, lengths, (g_outputs, g_h, g_c)) in fp32: N(0, 1) frames, a glorot-uniform kernel, a small random bias, lengths
    drawn from 0 .. T + 2 unless given, N(0, 1) upstream gradients for all three results."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, In, generator=g)
    lim = math.sqrt(6.0 / (In + H + 4 * H))
    kernel = (torch.rand(In + H, 4 * H, generator=g) * 2 - 1) * lim
    bias = 0.1 * torch.randn(4 * H, generator=g)
    if lengths is None:
        lengths = torch.randint(0, T + 3, (B,), generator=g)
        lengths[0] = T                                             # (at least one full row)
    up = (torch.randn(B, T, H, generator=g), torch.randn(B, H, generator=g), torch.randn(B, H, generator=g))
    return x, kernel, bias, torch.as_tensor(lengths), up


NAMES = ("outputs", "h_last", "c_last", "dx", "dkernel", "dbias")


def layer_and_grads(x, kernel, bias, lengths, up, dtype):
    """-> {name: tensor} for NAMES, evaluated in ``dtype`` on the CPU."""
    leaves = [t.detach().to(dtype).clone().requires_grad_(True) for t in (x, kernel, bias)]
    outs = lstm_layer(*leaves, lengths)
    loss = sum((o * u.to(dtype)).sum() for o, u in zip(outs, up))
    grads = torch.autograd.grad(loss, leaves)
    return dict(zip(NAMES, [o.detach() for o in outs] + list(grads)))


# ---- the modules ----
def l2_normalize(x, dim):
    return x * torch.rsqrt(torch.clamp((x * x).sum(dim=dim, keepdim=True), min=1e-12))


def lstm_stack(x, cells, lengths):
    """cells: [(kernel, bias)] bottom first -> (the top layer's outputs, [(c, h)] per layer)."""
    states = []
    for kernel, bias in cells:
        x, h, c = lstm_layer(x, kernel, bias, lengths)
        states.append((c, h))
    return x, states


def last_hidden(x, cells, lengths):
    return lstm_stack(x, cells, lengths)[1][-1][1]


def concat_average(x, cells, lengths):
    """[l2n(sum_t outputs) | c_0, h_0, c_1, h_1, ... | l2n(sum_t inputs)]."""
    outputs, states = lstm_stack(x, cells, lengths)
    flat = [t for c, h in states for t in (c, h)]
    return torch.cat([l2_normalize(outputs.sum(1), 1)] + flat + [l2_normalize(x.sum(1), 1)], 1)


def cell_shapes(in_size, H, layers):
    """name -> shape of a stack's variables, in creation order."""
    shapes = {}
    for layer in range(layers):
        shapes[CELL % layer + "kernel"] = ((in_size if layer == 0 else H) + H, 4 * H)
        shapes[CELL % layer + "bias"] = (4 * H,)
    return shapes


# ---- TriangulationRelationalModel ----
def model_variable_shapes(vocab, kv, ka, feature_size=1152, mixtures=2):
    """name -> shape of every variable of the model, in creation order (trainable and moving statistics)."""
    shapes = {}

    def bn(scope, c):
        for name in ("beta", "gamma", "moving_mean", "moving_variance"):
            shapes[f"{scope}/{name}"] = (c,)
    bn("input_bn", feature_size)
    width = 0
    for scope, D, K in (("video_t_emb", 1024, kv), ("audio_t_emb", feature_size - 1024, ka)):
        shapes[f"{scope}/anchor_weights"] = (D, K)
        for n, s in cell_shapes(D * K, D * K, 1).items():
            shapes[f"{scope}/{n}"] = s
        width += D * K
    shapes["lstm_hidden_1"] = (width, HIDDEN)
    bn("activation_1_bn", HIDDEN)
    shapes["lstm_hidden_2"] = (HIDDEN, HIDDEN)
    bn("activation_2_bn", HIDDEN)
    shapes["gates/weights"] = (HIDDEN, vocab * (mixtures + 1))
    shapes["experts/weights"] = (HIDDEN, vocab * mixtures)
    shapes["experts/biases"] = (vocab * mixtures,)
    return shapes


def _batch_norm(x, gamma, beta):
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    return (x - mean) * torch.rsqrt(var + BN_EPS) * gamma + beta


def model(v, frames, num_frames, uniform, labels, masks, iterations, mixtures=2, moe_l2=1e-8):
    """Training-mode forward of the model from the variables ``v`` (name -> tensor, no tower prefix) on L2-normalised frames [B, F_max, 1152]:
    SampleRandomFrames with the given uniforms (idx = int32(fp32(u) fp32(num_frames))), input_bn, per stream the triangulation embedding
    [B, T, D K] and a one-layer LSTM of hidden size D K over it with the RAW num_frames as lengths, concat, two hidden layers (batch norm,
    leaky_relu(0.2), dropout by the given KEEP masks / 0.5), the mixture of experts -> (predictions [B, V], loss): the cross entropy
    (epsilon 10e-6, sum over classes, mean over the batch) plus moe_l2 sum(w^2) / 2 over the two MoE weight matrices."""
    dt = frames.dtype
    B = frames.shape[0]
    idx = (uniform.float() * num_frames.reshape(-1, 1).float()).to(torch.int32).long()
    x = frames[torch.arange(B).unsqueeze(1), idx]                                 # [B, T, F]
    T, F = x.shape[1], x.shape[2]
    x = _batch_norm(x.reshape(B * T, F), v["input_bn/gamma"], v["input_bn/beta"])
    last = []
    for scope, cols in (("video_t_emb", slice(0, 1024)), ("audio_t_emb", slice(1024, None))):
        a = l2_normalize(v[scope + "/anchor_weights"], 0)                          # [D, K]
        e = l2_normalize(x[:, cols].unsqueeze(1) - a.t().unsqueeze(0), 2)           # [B T, K, D]
        e = e.reshape(B, T, -1)
        last.append(last_hidden(e, [(v[scope + "/" + CELL % 0 + "kernel"], v[scope + "/" + CELL % 0 + "bias"])], num_frames))
    act = torch.cat(last, 1)
    for n, key in (("1", "hidden_1"), ("2", "hidden_2")):
        act = act @ v["lstm_hidden_" + n]
        act = _batch_norm(act, v[f"activation_{n}_bn/gamma"], v[f"activation_{n}_bn/beta"])
        act = torch.where(act > 0, act, 0.2 * act)
        act = act * (masks[key] != 0).to(dt) / 0.5
    V = labels.shape[1]
    gate = torch.softmax((act @ v["gates/weights"]).reshape(-1, mixtures + 1), -1)
    expert = torch.sigmoid((act @ v["experts/weights"] + v["experts/biases"]).reshape(-1, mixtures))
    p = (gate[:, :mixtures] * expert).sum(1).reshape(-1, V)
    y = labels.to(dt)
    ce = -(y * torch.log(p + 10e-6) + (1 - y) * torch.log(1 - p + 10e-6)).sum(1).mean()
    reg = moe_l2 * 0.5 * ((v["gates/weights"] ** 2).sum() + (v["experts/weights"] ** 2).sum())
    return p, ce + reg
