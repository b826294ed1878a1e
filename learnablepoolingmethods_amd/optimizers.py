"""The update rules ``--optimizer`` selects by name (reference: train.py:106, ``find_class_by_name(FLAGS.optimizer, [tf.train])`` :577,
``optimizer_class(learning_rate)`` :252): for each class of tf.train that can be built from a learning rate alone, the hyper-parameters
TF1 gives it then, the slot variables it keeps, their initial values and the names a TF checkpoint stores them under.

With ``g`` the gradient after the per-variable clip_by_norm (utils.py:170-189; the analytic L2 term included where ``moe_l2`` applies)
and ``lr`` the decayed learning rate of the step, in this order of operations:

    GradientDescentOptimizer  p -= lr*g
    MomentumOptimizer         a = mu*a + g;  p -= lr*a                                   a (0) -> <var>/Momentum
    AdagradOptimizer          a = a + g*g;  p -= lr*g/sqrt(a)                            a (0.1) -> <var>/Adagrad
    RMSPropOptimizer          s = s + (g*g - s)*(1 - decay);  p -= lr*g/sqrt(s + eps)    s (1) -> <var>/RMSProp
    AdadeltaOptimizer         a = rho*a + (1 - rho)*g*g;  u = sqrt(d + eps)/sqrt(a + eps)*g;  d = rho*d + (1 - rho)*u*u;  p -= lr*u
                                                                                         a (0) -> <var>/Adadelta, d (0) -> <var>/Adadelta_1

On the GPU the rules run as lpm_multi_tensor_clip_update (csrc/clip_update.hip, ops.clip_update_step); ``host_clip_update`` is the
same arithmetic in fp32 torch for a trainer on the CPU device.  AdamOptimizer, the default, keeps its own kernels and its own host
route (train.Trainer); its spec is here for the slot names only.

Not kept: RMSProp's second slot.  TF creates a ``<var>/RMSProp_1`` momentum slot whatever the momentum; with the momentum of 0 that
``RMSPropOptimizer(learning_rate)`` has, it is written every step and read by nothing.  It is neither allocated nor saved here.

MomentumOptimizer has no default momentum: the reference's own ``optimizer_class(learning_rate)`` raises for it.  The build-extension
flag ``optimizer_momentum`` supplies one; without it the name is refused.  Nesterov momentum is off, TF's default.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import FLAGS
from ._capi import LpmError

# the kinds of lpm_multi_tensor_clip_update (include/lpm_hip.h); 0: Adam, which that entry point does not serve
ADAM, GRADIENT_DESCENT, MOMENTUM, ADAGRAD, RMSPROP, ADADELTA = 0, 1, 2, 3, 4, 5


@dataclass(frozen=True)
class OptimizerSpec:
    name: str
    kind: int
    h0: float = 0.0                            # Momentum: mu; RMSProp: decay; Adadelta: rho
    h1: float = 0.0                            # RMSProp, Adadelta: epsilon
    slot_init: Tuple[float, ...] = ()          # one entry per slot arena: its initial value
    slot_keys: Tuple[str, ...] = ()            # ... and the suffix of its checkpoint key, "<var>/<suffix>"

    @property
    def slots(self) -> int:
        return len(self.slot_init)


SUPPORTED = ("AdamOptimizer", "GradientDescentOptimizer", "MomentumOptimizer", "AdagradOptimizer", "RMSPropOptimizer", "AdadeltaOptimizer")
# the suffixes of the slot variables in a checkpoint, "<var>/<suffix>" (what a reader of the variables alone has to drop)
SLOT_KEYS = {"AdamOptimizer": ("Adam", "Adam_1"), "GradientDescentOptimizer": (), "MomentumOptimizer": ("Momentum",),
             "AdagradOptimizer": ("Adagrad",), "RMSPropOptimizer": ("RMSProp",), "AdadeltaOptimizer": ("Adadelta", "Adadelta_1")}
# classes of tf.train the reference's lookup would find and this project does not implement
NOT_IMPLEMENTED = ("FtrlOptimizer", "ProximalGradientDescentOptimizer", "ProximalAdagradOptimizer", "AdagradDAOptimizer")


def by_name(name: str, momentum: Optional[float] = None) -> OptimizerSpec:
    """The spec of tf.train's class ``name`` as ``optimizer_class(learning_rate)`` builds it.  ``momentum``: MomentumOptimizer's, None
    = FLAGS.optimizer_momentum."""
    if name == "AdamOptimizer":
        return OptimizerSpec(name, ADAM, slot_init=(0.0, 0.0), slot_keys=SLOT_KEYS[name])
    if name == "GradientDescentOptimizer":
        return OptimizerSpec(name, GRADIENT_DESCENT)
    if name == "MomentumOptimizer":
        mu = FLAGS.optimizer_momentum if momentum is None else momentum
        if mu is None:
            raise LpmError("MomentumOptimizer cannot be built from a learning rate alone (the reference's optimizer_class(learning_rate) "
                           "raises for it too): pass --optimizer_momentum (FLAGS.optimizer_momentum), which has no default")
        return OptimizerSpec(name, MOMENTUM, h0=float(mu), slot_init=(0.0,), slot_keys=SLOT_KEYS[name])
    if name == "AdagradOptimizer":
        return OptimizerSpec(name, ADAGRAD, slot_init=(0.1,), slot_keys=SLOT_KEYS[name])
    if name == "RMSPropOptimizer":
        return OptimizerSpec(name, RMSPROP, h0=0.9, h1=1e-10, slot_init=(1.0,), slot_keys=SLOT_KEYS[name])
    if name == "AdadeltaOptimizer":
        return OptimizerSpec(name, ADADELTA, h0=0.95, h1=1e-8, slot_init=(0.0, 0.0), slot_keys=SLOT_KEYS[name])
    why = "is not implemented" if name in NOT_IMPLEMENTED else "is not an optimizer this project knows"
    raise LpmError(f"--optimizer {name!r} {why}; the supported ones are {', '.join(SUPPORTED)}")


def _f32(x) -> float:
    return float(np.float32(x))


@torch.no_grad()
def apply_rule(spec: OptimizerSpec, p: torch.Tensor, g: torch.Tensor, slots: Sequence[torch.Tensor], lr: float):
    """One variable, in place, given its CLIPPED gradient: update_element of csrc/clip_update.hip in torch -- the same operations in
    the same order, each rounded on its own, the scalars rounded to fp32 first as the kernel's arguments are."""
    lr, h0, h1 = _f32(lr), _f32(spec.h0), _f32(spec.h1)
    one_minus = _f32(np.float32(1.0) - np.float32(h0))
    if spec.kind == GRADIENT_DESCENT:
        p.sub_(g * lr)
    elif spec.kind == MOMENTUM:
        a, = slots
        a.mul_(h0).add_(g)
        p.sub_(a * lr)
    elif spec.kind == ADAGRAD:
        a, = slots
        a.add_(g * g)
        p.sub_(g * lr / a.sqrt())
    elif spec.kind == RMSPROP:
        s, = slots
        s.add_((g * g - s) * one_minus)
        p.sub_(g * lr / (s + h1).sqrt())
    elif spec.kind == ADADELTA:
        a, d = slots
        a.mul_(h0).add_(g * one_minus * g)
        u = (d + h1).sqrt() / (a + h1).sqrt() * g
        d.mul_(h0).add_(u * one_minus * u)
        p.sub_(u * lr)
    else:
        raise LpmError(f"apply_rule: {spec.name} is not one of the rules of lpm_multi_tensor_clip_update")


@torch.no_grad()
def host_clip_update(spec: OptimizerSpec, arena, clip: float, lr: float):
    """lpm_multi_tensor_clip_update's arithmetic for a trainer on the CPU device, in PyTorch over the arenas: per-variable clip_by_norm
    (utils.py:181-188), then the rule.  Never taken with tensors on a GPU."""
    if arena.param.is_cuda:
        raise LpmError("optimizers.host_clip_update is the CPU route; GPU arenas go through ops.clip_update_step")
    for name in arena.names:
        lo, hi = arena.segment(name)
        g = arena.grad[lo:hi]
        if clip and clip > 0:
            g = g * (clip / torch.clamp(torch.linalg.vector_norm(g), min=clip))
        apply_rule(spec, arena.param[lo:hi], g, [s[lo:hi] for s in arena.slots], lr)
