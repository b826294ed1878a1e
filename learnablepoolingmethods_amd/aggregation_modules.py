"""Frame-axis pooling modules (reference: aggregation_modules.py:56-165): [B, T, F] -> [B, F] or [B, 2 F].

Host-side torch code, CPU and GPU: the drop-in surface and the small-shape path.  The triangulation models' training path does not
come through here -- ``ops.triangulation_pool`` / ``ops.triangulation_attention_pool`` produce the pooled vectors without the
[B, T, F] tensor these modules read.
The maximum routes its gradient to the FIRST frame that attains it (``torch.max(dim)``), the rule of the fused kernels.
``GemPoolingModule`` (marked incomplete in the reference) is not carried over."""
from __future__ import annotations

import torch

from . import layers, modules


def _indirect_attention(t_inputs):
    """softmax over the frames of the row sums of relu(V V^T) (:37-45 / :90-97) -> [B, T, 1]."""
    attention = torch.relu(t_inputs.matmul(t_inputs.transpose(1, 2)))       # [B, T, T]
    return torch.softmax(attention.sum(dim=2, keepdim=True), dim=1)


class IndirectClusterMeanPoolModule(modules.BaseModule):
    """Attention-weighted mean over the frames (:21-53): the weights come from ``t_inputs``, the pooling is over ``c_inputs``.
    The weights sum to one and ``reduce_mean`` follows them, as written: the result is 1 / T of the weighted sum."""

    def __init__(self, l2_normalize):
        self.l2_normalize = l2_normalize

    def forward(self, t_inputs, c_inputs, **unused_params):
        mean_pool = (c_inputs * _indirect_attention(t_inputs)).mean(dim=1)
        if self.l2_normalize:
            mean_pool = layers.l2_normalize(mean_pool, 1)
        return mean_pool


class IndirectClusterMaxMeanPoolModule(modules.BaseModule):
    """[attention-weighted mean | max] over the frames (:74-108) -- the mean FIRST, the other order than MaxMeanPoolingModule; each
    half L2-normalised when asked.  Materialises [B, T, T] from a [B, T, F] input: the CPU path and the drop-in surface;
    ``ops.triangulation_attention_pool`` is the training path of SoftAttentionTriangulationModel on the GPU."""

    def __init__(self, l2_normalize):
        self.l2_normalize = l2_normalize

    def forward(self, inputs, **unused_params):
        mean_pool = (inputs * _indirect_attention(inputs)).mean(dim=1)
        max_pool = inputs.max(dim=1).values
        if self.l2_normalize:
            mean_pool = layers.l2_normalize(mean_pool, 1)
            max_pool = layers.l2_normalize(max_pool, 1)
        return torch.cat([mean_pool, max_pool], 1)


class MeanPooling(modules.BaseModule):
    """Average over the frames (:152-165).  ``l2_normalize`` is accepted and unused, as written."""

    def __init__(self, l2_normalize=False):
        self.l2_normalize = l2_normalize

    def forward(self, inputs, **unused_params):
        return inputs.mean(dim=1)


class MaxPoolingModule(modules.BaseModule):
    """Maximum over the frames (:136-149).  ``l2_normalize`` is accepted and unused, as written."""

    def __init__(self, l2_normalize=False):
        self.l2_normalize = l2_normalize

    def forward(self, inputs, **unused_params):
        return inputs.max(dim=1).values


class MaxMeanPoolingModule(modules.BaseModule):
    """[max | mean] over the frames, each half L2-normalised when asked (:111-133)."""

    def __init__(self, l2_normalize=True):
        self.l2_normalize = l2_normalize

    def forward(self, inputs, **unused_params):
        max_pooled = inputs.max(dim=1).values
        avg_pooled = inputs.mean(dim=1)
        if self.l2_normalize:
            max_pooled = layers.l2_normalize(max_pooled, 1)
            avg_pooled = layers.l2_normalize(avg_pooled, 1)
        return torch.cat([max_pooled, avg_pooled], 1)


class MeanStdPoolModule(modules.BaseModule):
    """Returns the mean only, as written (:56-71): no standard deviation is computed, ``l2_normalize`` is unused."""

    def __init__(self, l2_normalize):
        self.l2_normalize = l2_normalize

    def forward(self, inputs, **unused_params):
        return inputs.mean(dim=1)
