"""Frame-axis pooling modules (reference: aggregation_modules.py:56-165): [B, T, F] -> [B, F] or [B, 2 F].

Host-side torch code, CPU and GPU: the drop-in surface and the small-shape path.  The triangulation models' training path does not
come through here -- ``ops.triangulation_pool`` produces the pooled vectors without the [B, T, F] tensor these modules read.
The maximum routes its gradient to the FIRST frame that attains it (``torch.max(dim)``), the rule of the fused kernel.
``IndirectCluster*`` and ``GemPoolingModule`` (marked incomplete in the reference) are not carried over."""
from __future__ import annotations

import torch

from . import layers, modules


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
