"""-m gpu: the frame-prep ops in front of NetVLAD -- ops.frame_sample_bn on fp32 frames and ops.frame_gather_bn_split -- against the fp64
restatement tests/_netvlad_ref.input_bn over the sampled rows, under the rule of tests/test_gpu_netvlad_bounds.py: per named part the op's
error is at most max(8 err32, 1e-6), err32 the error of the same restatement evaluated in fp32 on the CPU (these kernels are exact fp32).
Parts: y per clip (max over clips of max |error| / max |fp64 value| in the clip; clip b's upstream gradient is N(0, 1) times
10^(6 b / (B - 1) - 3)), dgamma, dbeta and, in training mode from zero moving statistics, 0.001 x the batch mean and 0.001 x the unbiased batch
variance (precisely (1 - fp32(0.999)) x: tests/_netvlad_ref.ONE_MINUS_DECAY).  Ragged num_frames, one clip with a single frame.  That the
gather moves the right rows bit for bit stays with tests/test_gpu_frame_gather.py and tests/test_gpu_kernels.test_frame_sample_bn.
This file runs ONE regime (|mean| / std about 1, fp32 frames, two ops); the offset, spread, clip-offset and quantised regimes, the uint8
forms and the other apply forms are held by tests/test_gpu_frame_prep_bounds.py, which is also where the raw-sum variance of these kernels
(var = q / n - mean^2) was measured and replaced.

Measured on the MI355X, worst error / bound over the parts:
MEASURED-BEGIN
First run: batch_mean / batch_var off by the constant 1.29e-5 of 1 - fp32(0.999) (ratio 7 .. 13), everything else within the bound; with
tests/_netvlad_ref.ONE_MINUS_DECAY in the model:
op, (B, MF, F, S)                           training (part)        eval (part)
frame_sample_bn (2,7,128,7)                0.49 (y)               0.08 (dbeta)
frame_sample_bn (5,40,128,7)               0.19 (batch_var)       0.10 (y)
frame_sample_bn (3,33,1152,33)             0.47 (batch_var)       0.11 (dbeta)
frame_sample_bn (2,300,1152,64)            0.64 (batch_var)       0.13 (dbeta)
frame_gather_bn_split (2,7,128,7)          0.53 (y)               0.08 (dbeta)
frame_gather_bn_split (5,40,128,7)         0.28 (batch_var)       0.09 (dbeta)
frame_gather_bn_split (3,33,1152,33)       0.32 (batch_var)       0.13 (dbeta)
frame_gather_bn_split (2,300,1152,64)      0.56 (batch_var)       0.17 (dbeta)
MEASURED-END"""
import functools
import math

import pytest
import torch

from oracle import lpm_oracle as O
from tests import _netvlad_ref as R
from tests._util import cuda

pytestmark = pytest.mark.gpu

SHAPES = [(2, 7, 128, 7), (5, 40, 128, 7), (3, 33, 1152, 33), (2, 300, 1152, 64)]          # B, MF, F, S


@functools.lru_cache(maxsize=None)
def _inputs(B, MF, F, S, seed):
    g = torch.Generator().manual_seed(seed)
    frames = torch.randn(B, MF, F, generator=g) * (0.5 + torch.rand(F, generator=g)) + 0.3 * torch.randn(F, generator=g)
    nf = torch.randint(2, MF + 1, (B,), generator=g)
    nf[0], nf[-1] = MF, 1                                          # a full clip and a clip of one frame
    gamma, beta = 1 + 0.3 * torch.randn(F, generator=g), 0.2 * torch.randn(F, generator=g)
    moving = (0.1 * torch.randn(F, generator=g), 0.5 + torch.rand(F, generator=g))
    up = torch.randn(B, S * F, generator=g) * R.clip_decades(B).float().unsqueeze(1)
    random_index = (torch.rand(B, S, generator=g) * nf.unsqueeze(1)).long().clamp_max(MF - 1)
    return dict(frames=frames, nf=nf, gamma=gamma, beta=beta, moving=moving, up=up.reshape(B * S, F), random_index=random_index)


@functools.lru_cache(maxsize=None)
def _reference(B, MF, F, S, seed, training, uniform):
    """-> (fp64 parts, err32 per part) of input_bn over the rows the op samples."""
    inp = _inputs(B, MF, F, S, seed)
    index = torch.from_numpy(O.sample_uniform_frame_index(inp["nf"].numpy(), S)).long() if uniform else inp["random_index"]
    parts = {}
    for dt in (torch.float64, torch.float32):
        gamma, beta = (inp[k].to(dt).requires_grad_(True) for k in ("gamma", "beta"))
        y, mean, uvar = R.input_bn(R.gather_rows(inp["frames"].to(dt), index), gamma, beta, training=training,
                                   moving=tuple(m.to(dt) for m in inp["moving"]))
        dgamma, dbeta = torch.autograd.grad((y * inp["up"].to(dt)).sum(), [gamma, beta])
        parts[dt] = dict(y=y.detach(), dgamma=dgamma, dbeta=dbeta)
        if training:
            parts[dt].update(batch_mean=mean.detach(), batch_var=uvar.detach())
    p64, p32 = parts[torch.float64], parts[torch.float32]
    return p64, {n: _figure(p32[n], p64[n], n, B) for n in p64}


def _figure(got, ref, name, B):
    return R.figure(got, ref, "out" if name == "y" else name, B)


def _check(tag, got, B, p64, e32):
    rows = [(n, _figure(got[n], p64[n], n, B), e32[n], max(8 * e32[n], 1e-6)) for n in p64]
    for n, e_op, e, bound in rows:
        print(f"[input_bn] {tag} {n}: op {e_op:.3e}, err32 {e:.3e}, bound {bound:.3e}, ratio {e_op / bound:.3f}")
    for n, e_op, e, bound in rows:
        assert e > 0, f"{tag} {n}: err32 is zero"
        assert math.isfinite(e_op) and e_op <= bound, f"{tag} {n}: op error {e_op:.3e} > max(8 x {e:.3e}, 1e-6)"


def _run(op, inp, dev, training, F):
    """op(gamma, beta, moving_mean, moving_var) -> y [B S, F]; moving statistics from zeros in training mode."""
    gamma, beta = (inp[k].to(dev).requires_grad_(True) for k in ("gamma", "beta"))
    mm, mv = (torch.zeros(F, device=dev), torch.zeros(F, device=dev)) if training else (m.to(dev) for m in inp["moving"])
    y = op(gamma, beta, mm, mv)
    dgamma, dbeta = torch.autograd.grad((y * inp["up"].to(dev)).sum(), [gamma, beta])
    torch.cuda.synchronize()
    got = dict(y=y.detach(), dgamma=dgamma, dbeta=dbeta)
    if training:
        got.update(batch_mean=mm / R.ONE_MINUS_DECAY, batch_var=mv / R.ONE_MINUS_DECAY)
    return got


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("B,MF,F,S", SHAPES)
def test_frame_sample_bn_meets_the_bound(B, MF, F, S, training):
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    inp = _inputs(B, MF, F, S, 0)
    p64, e32 = _reference(B, MF, F, S, 0, training, True)
    frames, nf = inp["frames"].to(dev), inp["nf"].to(dev)
    got = _run(lambda g, b, mm, mv: ops.frame_sample_bn(frames, nf, S, g, b, mm, mv, is_training=training), inp, dev, training, F)
    _check(f"frame_sample_bn ({B},{MF},{F},{S}) training={training}", got, B, p64, e32)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("B,MF,F,S", SHAPES)
def test_frame_gather_bn_split_meets_the_bound(B, MF, F, S, training):
    from learnablepoolingmethods_amd import ops
    dev = cuda()
    inp = _inputs(B, MF, F, S, 1)
    p64, e32 = _reference(B, MF, F, S, 1, training, False)
    frames, nf = inp["frames"].to(dev), inp["nf"].to(dev)
    index = inp["random_index"].to(torch.int32).to(dev)
    Dv = 1024 if F == 1152 else 64

    def op(g, b, mm, mv):
        return torch.cat(ops.frame_gather_bn_split(frames, nf, index, g, b, mm, mv, training, Dv), 1)
    got = _run(op, inp, dev, training, F)
    _check(f"frame_gather_bn_split ({B},{MF},{F},{S}) training={training}", got, B, p64, e32)
