"""-m gpu: the three poolings of the triangulation embedding form e and f with one walk (csrc/triangulation_common.h:
tp_walk_fwd_kernel).  "e, f exactly as in triangulation_pool" is the contract the attention-weighted ops state; here it is held to the
bit: what does not depend on the weights -- both maxima, and the unweighted mean of f -- must come out of two ops with the same bits,
a scale that is no power of two and an identical consecutive pair of frames (u = 0 exactly) included."""
import functools

import pytest
import torch

from tests import _triangulation_ref as R
from tests._util import cuda

pytestmark = pytest.mark.gpu

SHAPES = [  # B, T, D, K, scale
    (2, 34, 128, 5, 1 / 3),                  # crosses the 32-frame partial sum; a partly filled group of four anchors
    (1, 33, 1024, 2, 1 / 3),                 # video width
    (3, 2, 128, 1, 0.7),                     # one temporal difference, one anchor
]


@functools.lru_cache(maxsize=None)
def _outputs(B, T, D, K, s):
    """(max_d, mean_d, max_t, mean_t) of triangulation_pool, (mean_d, max_d, mean_t, max_t) of triangulation_attention_pool and
    (m_d, m_t) of triangulation_mean_pool for one x, anchors and scale; frames T-2 and T-1 of clip 0 are identical."""
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    x, anchors, _ = R.make_inputs(B, T, D, K, 7)
    x[T - 1] = x[T - 2]
    xg, ag = x.to(dev), R.l2n(anchors, 0).to(dev)
    with torch.no_grad():
        return (ops.triangulation_pool(xg, ag, T, scale=s), ops.triangulation_attention_pool(xg, ag, T, scale=s),
                ops.triangulation_mean_pool(xg, ag, T, scale=s))


@pytest.mark.parametrize("B,T,D,K,s", SHAPES)
def test_pool_and_attention_pool_share_the_maxima(B, T, D, K, s):
    pool, attention, _ = _outputs(B, T, D, K, s)
    assert torch.equal(pool[0], attention[1]), "max_d"
    assert torch.equal(pool[2], attention[3]), "max_t"


@pytest.mark.parametrize("B,T,D,K,s", SHAPES)
def test_pool_and_mean_pool_share_the_temporal_mean(B, T, D, K, s):
    pool, _, mean = _outputs(B, T, D, K, s)
    assert torch.equal(pool[3], mean[1]), "mean_t"
