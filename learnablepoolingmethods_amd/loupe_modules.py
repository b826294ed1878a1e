"""``loupe_modules.NetVLAD``, the pooling TriangulationMagnitudeNsCnnNetVladModule names (reference: video_pooling_modules.py:1041-1060).
The reference ships no loupe_modules file; this class is a RESOLUTION: the reference's own
``frame_level_models.NetVLAD.forward`` (:2773-2824), the same pooling from the same source, followed by the bias-free projection onto
``output_dim`` that the constructor's ``output_dim`` asks for (``hidden1_weights``, initialised as every hidden1_weights of the reference
is: N(0, 1 / sqrt(cluster_size))).  ``gating=True`` is refused: the one caller passes False.

On the GPU the pooling is ops.netvlad (d-major, fp32 storage, with the gradient for the frames) and the projection ops.projection where
lpm_proj_supported allows.  The NetVLAD kernels take certain feature widths only (``padded_size``: the assignment GEMM and the backward
every multiple of 32, the aggregation forward multiples of 128 with clusters that are, else 128 / 256 / 512 / 1024); other widths are
zero-padded, which is exact: a zero feature column adds nothing to the logits, with a zero row in ``cluster_weights2`` it gives zero
descriptor entries, and it changes neither L2 norm.  So the input is padded to (or arrives at:
ops.triangulation_magnitude_frames(pad_to=...)) that width -- 2080 -> 2176 and 136 -> 256 at JuhanTestModelV4's defaults -- the two
[feature_size, cluster_size] matrices get zero rows through torch.nn.functional.pad (autograd carries their gradients back), and the first
feature_size * cluster_size columns of the d-major descriptor, which are contiguous, are kept.  The variables keep the reference's shapes.
The kernels are handed the rows centred on their mean, to which NetVLAD is invariant and their split-bf16 products are not
(``NetVLAD._fused_descriptor``).  A shape ops.netvlad does not take, and the CPU, go through the torch formulation of the same lines."""
from __future__ import annotations

import math

import torch

from . import layers, ops
from . import variables as vs

STREAMING_WIDTHS = (128, 256, 512, 1024)       # the widths of the register-streaming aggregation forward (lpm_vlad_aggregate_tiles_fwd)


def padded_size(feature_size, cluster_size):
    """The width ops.netvlad is given for ``feature_size`` feature columns: the smallest one not below it that an aggregation forward
    takes -- a multiple of 128 with clusters that are a multiple of 128 (the LDS-shared form, lpm_vlad_tiles3_supported), else one of
    STREAMING_WIDTHS; None when there is none.  (The assignment GEMM and the backward take every multiple of 32; the forward does not.)"""
    D, K = int(feature_size), int(cluster_size)
    if K % 128 == 0:
        return (D + 127) // 128 * 128
    return next((w for w in STREAMING_WIDTHS if w >= D), None)


def fused_ok(max_samples, feature_size, cluster_size):
    """ops.netvlad takes (max_samples, the padded width, cluster_size): an aggregation forward exists for it, and the tile forms of the
    assignment GEMM and of the aggregation's backward (clusters a multiple of 32, at most 512)."""
    Dp = padded_size(feature_size, cluster_size)
    return Dp is not None and ops.netvlad_input_shortcut_ok(int(max_samples), Dp, int(cluster_size))


class NetVLAD():
    """forward(reshaped_input [(B*max_samples), feature_size]) -> [B, output_dim]."""

    # None: zero-pad the features iff ops.netvlad runs; False: never (the torch formulation); a width: pad to it in the torch formulation,
    # which takes any (the tests' and the benchmark's handle on the padding and on the kernels)
    pad_features = None

    def __init__(self, feature_size, max_samples, cluster_size, output_dim, gating, add_batch_norm, is_training):
        if gating:
            raise NotImplementedError("loupe_modules.NetVLAD(gating=True): the reference ships no loupe_modules and its one caller "
                                      "(TriangulationMagnitudeNsCnnNetVladModule) passes gating=False; there is nothing to follow")
        self.feature_size = int(feature_size)
        self.max_samples = int(max_samples)
        self.cluster_size = int(cluster_size)
        self.output_dim = int(output_dim)
        self.gating = gating
        self.add_batch_norm = add_batch_norm
        self.is_training = is_training

    def forward(self, reshaped_input):
        """``reshaped_input`` may also arrive padded, [(B*max_samples), padded_size(feature_size)] with zeros in the extra columns."""
        D, K, S, dev = self.feature_size, self.cluster_size, self.max_samples, reshaped_input.device
        Dp = padded_size(D, K) or D
        if isinstance(self.pad_features, int) and not isinstance(self.pad_features, bool):
            Dp = max(int(self.pad_features), D)
        if reshaped_input.dim() != 2 or reshaped_input.shape[1] not in (D, Dp) or reshaped_input.shape[0] % S:
            raise ValueError(f"loupe_modules.NetVLAD: expected [(B*{S}), {D}] (or {Dp} columns, zero-padded); got {tuple(reshaped_input.shape)}")
        std = 1 / math.sqrt(D)
        cluster_weights = vs.get_variable("cluster_weights", [D, K], vs.random_normal_initializer(std), device=dev)       # :2775
        bn = bias = None
        if self.add_batch_norm:
            bn = layers.bn_variables("cluster_bn", K, dev)                                                              # :2783-2789
        else:
            bias = vs.get_variable("cluster_biases", [K], vs.random_normal_initializer(std), device=dev)                # :2790-2796
        cluster_weights2 = vs.get_variable("cluster_weights2", [1, D, K], vs.random_normal_initializer(std), device=dev)  # :2805-2808
        hidden1_weights = vs.get_variable("hidden1_weights", [K * D, self.output_dim], vs.random_normal_initializer(1 / math.sqrt(K)),
                                          device=dev)
        fused = reshaped_input.is_cuda and reshaped_input.dtype == torch.float32 and fused_ok(S, D, K) and self.pad_features is None
        width = Dp if (fused or self.pad_features) else D
        x, w, w2 = reshaped_input, cluster_weights, cluster_weights2
        if x.shape[1] != width:
            x = torch.nn.functional.pad(x, (0, Dp - D)) if width == Dp else x[:, :D]
        if width != D:
            w, w2 = torch.nn.functional.pad(w, (0, 0, 0, Dp - D)), torch.nn.functional.pad(w2, (0, 0, 0, Dp - D))
        if fused:
            vlad = self._fused_descriptor(x.contiguous(), w, bn, bias, w2)                                        # [B, width * K], d-major
        else:
            vlad = self._torch_descriptor(x, w, bias, w2)
        vlad = vlad[:, :D * K]                                       # (d-major: the columns of the features d < D, contiguous)
        if vlad.is_cuda and vlad.dtype == torch.float32 and ops.projection_ok(vlad.shape[0], D * K, self.output_dim):
            return ops.projection(vlad, hidden1_weights)
        return vlad.matmul(hidden1_weights)

    def _fused_descriptor(self, x, cluster_weights, bn, bias, cluster_weights2):
        """ops.netvlad over rows CENTRED on their mean c (a constant of the call: no gradient).  NetVLAD is invariant to it -- the
        residual x - w2 = (x - c) - (w2 - c), and the logits move by c W per cluster, which a training-mode cluster_bn removes with the
        batch mean and the cluster_biases branch takes as bias + c W -- and the kernels' split-bf16 products are not: this module's rows
        [relu(conv) | norm] of a clip differ by a twentieth of their length (the norm columns are all about 1), the backward's
        dU . (x - w2) cancels that common part, and an operand rounded at 2^-16 of the whole row leaves 20 x the error in what is left
        (2e-4 -> 1e-5 in a module's gradients).  The moving mean is kept of the logits as they are (batch mean = c W
        + the centred logits' mean).  Eval-mode batch norm (no batch mean, no gradients wanted) runs on the rows as they are."""
        S = self.max_samples
        if bn is not None and not self.is_training:
            return ops.netvlad(x, cluster_weights, cluster_weights2, S, bn=bn, is_training=False)
        c = x.detach().mean(0)
        x, cluster_weights2 = x - c, cluster_weights2 - c.reshape(1, -1, 1)
        shift = c.matmul(cluster_weights)                                                        # c W [clusters]
        if bn is None:
            return ops.netvlad(x, cluster_weights, cluster_weights2, S, bias=bias + shift, is_training=self.is_training)
        gamma, beta, moving_mean, moving_variance = bn
        # the blend moving = moving decay + batch (1 - decay) of the batch mean c W + mean(centred logits): the kernel leaves the second
        # term's share in a zeroed stand-in, the rest is added here (no difference of two numbers of the size of c W is formed)
        share = torch.zeros_like(moving_mean)
        vlad = ops.netvlad(x, cluster_weights, cluster_weights2, S, bn=(gamma, beta, share, moving_variance), is_training=True)
        with torch.no_grad():
            decay = torch.tensor(layers.BN_DECAY, dtype=torch.float32, device=x.device)
            moving_mean.mul_(decay).add_(share).add_((1.0 - decay) * shift)
        return vlad

    def _torch_descriptor(self, x, cluster_weights, bias, cluster_weights2):
        """frame_level_models.py:2781-2822 in torch (any device, any dtype): x [(B*S), D'] -> [B, D' * cluster_size], d-major."""
        D, K, S = x.shape[1], self.cluster_size, self.max_samples
        activation = x.matmul(cluster_weights)                                                                          # :2781
        if self.add_batch_norm:
            activation = layers.batch_norm(activation, self.is_training, "cluster_bn")                                  # :2783-2789
        else:
            activation = activation + bias                                                                              # :2796
        activation = torch.softmax(activation, dim=-1).reshape(-1, S, K)                                                # :2798-2801
        a_sum = activation.sum(dim=1, keepdim=True)                                                                     # :2803
        a = a_sum * cluster_weights2                                                                                    # :2810
        vlad = activation.transpose(1, 2).matmul(x.reshape(-1, S, D)).transpose(1, 2) - a                               # :2812-2817
        vlad = layers.l2_normalize(vlad, 1)                                                                             # :2819
        return layers.l2_normalize(vlad.reshape(-1, K * D), 1)                                                          # :2821-2822
