"""Attention-cluster pooling, the per-head transformer block (attention_modules.py:22-161) and the five
class-gating modules over [B, vocab_size] class scores (:157-362) of the reference's attention_modules.py, on the hot path's kernels:

* ``OneFcAttention``: the weighted frame sums are K2's aggregation (similarities given, no softmax over clusters) and their
  backward is K3.  Because the attention is a softmax over the FRAMES of a clip, every cluster's weights sum to one, so the
  shift ``alpha * act + beta`` is exactly K2's residual term with the constant centre ``-beta / alpha``
  (``sum_t a (x - c) = act - c``) up to the sign of alpha, and ``l2_normalize(., 1) / sqrt(K)`` is K2's intra-normalisation
  followed by its global L2 (K unit-norm clusters have global norm sqrt(K)).  The k-major descriptor layout is the
  reference's ``[B, num_cluster * num_feature]``.
* ``MultiHeadAttention``: every head owns its relu(dense) q / k / v; the per-head cores run as ONE K4 launch over the
  concatenated heads when the head width is one K4 covers (8 or 16), as library batched GEMMs otherwise.
* ``TransformerEncoderBlock``: dense / conv1d(kernel_size=1) layers through ``layers.dense`` (split-bf16 library GEMMs).
* ``PGateModule`` / ``PnGateModule`` / ``NpGateModule``: every clipped gate behind its [V, V] product is one ``layers.class_rows``
  (ops.class_rows on the GPU: relu6 or -relu6(-t), the residual add and the closing softmax over the row in one launch).
* ``CorNNGateModule``: three slim.fully_connected of width V, bias + relu / relu / sigmoid as ops.class_filter stages on the GPU.
* ``ContextGateV1``: x * sigmoid(BN(x W)), host torch like MoeModel's probability gating.

Variable names are the ones TF1 assigns by default (``dense``, ``dense_1``, ``conv1d``, ``LayerNorm_1`` ...) for the first
block built under a variable scope; build further blocks under their own ``variable_scope``."""
from __future__ import annotations

import math

import torch

from . import FLAGS, layers, modules, ops
from . import variables as vs


def _constant_initializer(value: float):
    return lambda shape, dev, gen: torch.full(tuple(shape), float(value), device=dev)


class OneFcAttention(modules.BaseModule):
    """attention_modules.py:22-64."""

    def __init__(self, num_features, num_frames, num_cluster, do_shift=True):
        self.num_feature = int(num_features)
        self.num_frames = int(num_frames)
        self.num_cluster = int(num_cluster)
        self.do_shift = do_shift

    def forward(self, inputs, **unused_params):
        """inputs [(B * num_frames), F] -> [B, num_cluster * F] (cluster-major)."""
        F_, T, K = self.num_feature, self.num_frames, self.num_cluster
        attention_weights = vs.get_variable("one_fc_attention_weight", [F_, K], vs.glorot_uniform_initializer(),
                                            device=inputs.device)                                   # :30-33
        rows = inputs.shape[0]
        if layers.use_split_gemm(inputs, rows, K):
            attention = ops.dense_x3(inputs, attention_weights)                                     # :34
        else:
            attention = inputs.matmul(attention_weights)
        attention = torch.softmax(attention.reshape(-1, T, K) * (1.0 / math.sqrt(F_)), dim=1)     # :35-37 (over frames)
        if not self.do_shift:
            activation = torch.bmm(attention.transpose(1, 2), inputs.reshape(-1, T, F_))           # :39-41
            return activation.reshape(-1, K * F_)
        alpha = vs.get_variable("alpha", [1], _constant_initializer(1.0), device=inputs.device)    # :47-50
        beta = vs.get_variable("beta", [1], _constant_initializer(0.01), device=inputs.device)     # :51-54
        # :56-59 as K2's residual + intra-L2 + global L2 (module docstring); alpha == 0 has no such form and gives inf / nan
        centres = (-(beta / alpha)).expand(F_, K).contiguous()
        pooled = ops.vlad_aggregate(attention, inputs, centres, T, kmajor=True)                     # [B, K, F]
        return (pooled * torch.sign(alpha)).reshape(-1, K * F_)                                     # :61


class MultiHeadAttention(modules.BaseModule):
    """attention_modules.py:67-112."""

    def __init__(self, num_heads, num_units, max_frames, block_id):
        self.num_heads = int(num_heads)
        self.num_units = int(num_units)
        self.max_frames = int(max_frames)
        self.block_id = block_id

    def _projections(self, inputs, scope_id):
        with vs.variable_scope("Block{}Layer{}".format(self.block_id, scope_id)):                   # :79
            return [layers.dense(inputs, self.num_units, use_bias=True, name=name, activation=torch.relu)
                    .reshape(-1, self.max_frames, self.num_units) for name in ("dense", "dense_1", "dense_2")]   # :81-89

    def forward(self, inputs, **unused_params):
        """inputs [(B * max_frames), F] -> [B, max_frames, num_units * num_heads]."""
        heads = [self._projections(inputs, i) for i in range(self.num_heads)]
        q, k, v = (torch.cat([h[j] for h in heads], dim=2) for j in range(3))
        scale = 1.0 / float(self.num_units)                      # logits / sqrt(u) / sqrt(u)  (:95-96)
        if q.is_cuda and self.num_units in (8, 16) and self.max_frames <= 512:
            return ops.mha_core(q, k, v, self.num_heads, scale)                                      # :92-98, all heads at once
        B, L, h, u = q.shape[0], self.max_frames, self.num_heads, self.num_units
        qh, kh, vh = (t.reshape(B, L, h, u).permute(0, 2, 1, 3) for t in (q, k, v))
        att = torch.softmax(torch.matmul(qh, kh.transpose(-1, -2)) * scale, dim=-1)
        return torch.matmul(att, vh).permute(0, 2, 1, 3).reshape(B, L, h * u)                        # :104-110


def _conv1d_k1(x, filters, name, activation=None):
    """tf.layers.conv1d(kernel_size=1, use_bias=True): a dense layer whose kernel variable is [1, in, out]."""
    with vs.variable_scope(name):
        g = vs.glorot_uniform_initializer()
        kernel = vs.get_variable("kernel", [1, x.shape[-1], filters],
                                 lambda shape, dev, gen: g(shape[1:], dev, gen).reshape(shape), device=x.device)
        bias = vs.get_variable("bias", [filters], vs.zeros_initializer(), device=x.device)
    rows = x.numel() // x.shape[-1]
    if layers.use_split_gemm(x, rows, filters):
        y = ops.dense_x3(x.reshape(rows, x.shape[-1]), kernel[0]).reshape(*x.shape[:-1], filters)
    else:
        y = x.matmul(kernel[0])
    y = y + bias
    return activation(y) if activation is not None else y


class TransformerEncoderBlock(modules.BaseModule):
    """attention_modules.py:115-161."""

    def __init__(self, is_training, num_units, max_frames, feature_size, num_heads, block_id):
        self.is_training = is_training
        self.num_units = int(num_units)
        self.max_frames = int(max_frames)
        self.feature_size = int(feature_size)
        self.num_heads = int(num_heads)
        self.block_id = block_id

    def forward(self, inputs, **unused_params):
        """inputs [(B * max_frames), feature_size] -> same shape (num_units must equal feature_size, :156)."""
        multi_head_layer = MultiHeadAttention(self.num_heads, self.num_units, self.max_frames, self.block_id)
        attention_output = multi_head_layer.forward(inputs)                                          # :133-135
        attention_output = attention_output.reshape(-1, self.num_units * self.num_heads)             # :138
        attention_output = layers.dense(attention_output, self.feature_size, use_bias=True, name="dense",
                                        activation=torch.relu)                                       # :141
        attention_output = layers.layer_norm(attention_output + inputs, "LayerNorm")                 # :145-146 (rank 2: per row)
        output = attention_output.reshape(-1, self.max_frames, self.feature_size)                    # :149
        output = _conv1d_k1(output, 4 * self.num_units, "conv1d", activation=torch.relu)             # :150-151
        output = _conv1d_k1(output, self.num_units, "conv1d_1")                                      # :152
        output = layers.layer_norm(output, "LayerNorm_1")                                            # :155 (rank 3: frames x units)
        return output.reshape(-1, self.feature_size)                                                 # :156


def _gate_variable(name, vocab_size, device):
    """A [V, V] gate of the P / N gate modules: random_normal(stddev = 1 / sqrt(V)) (:176-183)."""
    return vs.get_variable(name, [vocab_size, vocab_size], vs.random_normal_initializer(1 / math.sqrt(vocab_size)), device=device)


class _ClassGateModule(modules.BaseModule):
    """The constructor the class-gating modules share (:158-168, :201-211, :244-254)."""

    def __init__(self, vocab_size, is_training, scope_id=None):
        self.vocab_size = int(vocab_size)
        self.scope_id = scope_id
        self.is_training = is_training


class PnGateModule(_ClassGateModule):
    """attention_modules.py:157-197: vocabularies -> P gate -> N gate -> softmax."""

    def forward(self, inputs, **unused_params):
        """inputs [B, vocab_size] -> [B, vocab_size]."""
        p_gating_weights = _gate_variable("p_pn_gate", self.vocab_size, inputs.device)                       # :176-179
        n_gating_weights = _gate_variable("n_pn_gate", self.vocab_size, inputs.device)                       # :180-183
        p_gate = layers.class_rows(inputs.matmul(p_gating_weights), residual=inputs, phi="relu6")            # :186-188
        return layers.class_rows(p_gate.matmul(n_gating_weights), residual=p_gate, phi="neg_relu6", norm="softmax")   # :191-196


class NpGateModule(_ClassGateModule):
    """attention_modules.py:200-240: vocabularies -> N gate -> P gate -> softmax.  The P gate's variable is created first, as written."""

    def forward(self, inputs, **unused_params):
        """inputs [B, vocab_size] -> [B, vocab_size]."""
        p_gating_weights = _gate_variable("p_np_gate", self.vocab_size, inputs.device)                       # :219-222
        n_gating_weights = _gate_variable("n_np_gate", self.vocab_size, inputs.device)                       # :223-226
        n_gate = layers.class_rows(inputs.matmul(n_gating_weights), residual=inputs, phi="neg_relu6")        # :229-232
        return layers.class_rows(n_gate.matmul(p_gating_weights), residual=n_gate, phi="relu6", norm="softmax")   # :235-238


class PGateModule(_ClassGateModule):
    """attention_modules.py:243-273: vocabularies -> P gate -> softmax."""

    def forward(self, inputs, **unused_params):
        """inputs [B, vocab_size] -> [B, vocab_size]."""
        p_gating_weights = _gate_variable("p_p_gate", self.vocab_size, inputs.device)                        # :262-265
        return layers.class_rows(inputs.matmul(p_gating_weights), residual=inputs, phi="relu6", norm="softmax")   # :268-271


def _scope_suffix(scope_id):
    return "" if scope_id is None else str(scope_id)


class CorNNGateModule(modules.BaseModule):
    """attention_modules.py:276-316: three slim.fully_connected of width vocab_size -- relu, relu, sigmoid -- under
    vocab_gate{1,2,3}_v1{scope_id}/{weights,biases}.  ``batch_norm`` is accepted and read nowhere, as written."""

    def __init__(self, vocab_size, is_training, batch_norm=True, scope_id=None):
        self.vocab_size = int(vocab_size)
        self.is_training = is_training
        self.batch_norm = batch_norm
        self.scope_id = scope_id

    def _fully_connected(self, x, scope, act):
        """slim.fully_connected(x, vocab_size, activation_fn=act): xavier weights, zero biases.  FLAGS.class_filter_fused on the GPU: the
        bias and the activation are one ops.class_filter stage (no batch norm) behind the product."""
        with vs.variable_scope(scope):
            w = vs.get_variable("weights", [x.shape[1], self.vocab_size], vs.glorot_uniform_initializer(), device=x.device)
            b = vs.get_variable("biases", [self.vocab_size], vs.zeros_initializer(), device=x.device)
        a = x.matmul(w)
        if FLAGS.class_filter_fused and a.is_cuda and ops.class_filter_ok(a, b, None, act, None, bool(self.is_training)):
            return ops.class_filter(a, b, act=act, is_training=bool(self.is_training))
        return (torch.relu if act == "relu" else torch.sigmoid)(a + b)

    def forward(self, inputs, **unused_params):
        """inputs [B, vocab_size] -> [B, vocab_size]."""
        s = _scope_suffix(self.scope_id)
        fc1_out = self._fully_connected(inputs, "vocab_gate1_v1" + s, "relu")                                # :295-300
        fc2_out = self._fully_connected(fc1_out, "vocab_gate2_v1" + s, "relu")                               # :302-307
        return self._fully_connected(fc2_out, "vocab_gate3_v1" + s, "sigmoid")                               # :309-316


class ContextGateV1(modules.BaseModule):
    """attention_modules.py:319-362 (WILLOW's context gating): x * sigmoid(BN(x W)), W ``vocab_gate_v1{scope_id}`` [V, V] created without
    an initializer (tf.get_variable's default: glorot uniform), BN slim.batch_norm under ``vocab_gate_bn_v1{scope_id}`` when
    ``batch_norm``; there is no bias otherwise.  Host torch."""

    def __init__(self, vocab_size, is_training, batch_norm=True, scope_id=None):
        self.vocab_size = int(vocab_size)
        self.is_training = is_training
        self.batch_norm = batch_norm
        self.scope_id = scope_id

    def forward(self, inputs, **unused_params):
        """inputs [B, vocab_size] -> [B, vocab_size]."""
        s = _scope_suffix(self.scope_id)
        gating_weights = vs.get_variable("vocab_gate_v1" + s, [self.vocab_size, self.vocab_size], vs.glorot_uniform_initializer(),
                                         device=inputs.device)                                               # :342-343
        gates = inputs.matmul(gating_weights)                                                                # :346
        if self.batch_norm:
            gates = layers.batch_norm(gates, self.is_training, "vocab_gate_bn_v1" + s)                       # :348-354
        return inputs * torch.sigmoid(gates)                                                                 # :356-362
