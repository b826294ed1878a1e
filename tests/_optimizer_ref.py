"""The update rules of ``--optimizer`` restated in fp64 torch from the table of DESIGN.md section 26, for tests/test_optimizers_host.py and
tests/test_gpu_clip_update.py.  Nothing here imports the code under test."""
import torch

MU = 0.9                  # the tests' --optimizer_momentum
RULES = ("GradientDescentOptimizer", "MomentumOptimizer", "AdagradOptimizer", "RMSPropOptimizer", "AdadeltaOptimizer")
# name -> (initial value of each slot, suffix of each slot's checkpoint key): tf.train's classes built from the learning rate alone
TABLE = {
    "GradientDescentOptimizer": ((), ()),
    "MomentumOptimizer": ((0.0,), ("Momentum",)),
    "AdagradOptimizer": ((0.1,), ("Adagrad",)),
    "RMSPropOptimizer": ((1.0,), ("RMSProp",)),
    "AdadeltaOptimizer": ((0.0, 0.0), ("Adadelta", "Adadelta_1")),
}


def clip64(g, clip):
    """utils.clip_gradient_norms (utils.py:170-189) for one variable: g * clip / max(||g||, clip); clip <= 0: no clipping."""
    g = g.double()
    if not clip or clip <= 0:
        return g
    return g * (clip / max(float(g.norm()), clip))


def rule64(name, p, g, slots, lr):
    """-> (p, slots) after one step of rule ``name`` on fp64 tensors; ``g`` is the clipped gradient."""
    if name == "GradientDescentOptimizer":
        return p - lr * g, []
    if name == "MomentumOptimizer":
        a = MU * slots[0] + g
        return p - lr * a, [a]
    if name == "AdagradOptimizer":
        a = slots[0] + g * g
        return p - lr * g / a.sqrt(), [a]
    if name == "RMSPropOptimizer":
        decay, eps = 0.9, 1e-10
        s = slots[0] + (g * g - slots[0]) * (1 - decay)
        return p - lr * g / (s + eps).sqrt(), [s]
    if name == "AdadeltaOptimizer":
        rho, eps = 0.95, 1e-8
        a = rho * slots[0] + (1 - rho) * g * g
        u = (slots[1] + eps).sqrt() / (a + eps).sqrt() * g
        d = rho * slots[1] + (1 - rho) * u * u
        return p - lr * u, [a, d]
    raise KeyError(name)


def check_trainer_steps(tr, name, batches, rel_err, only=None):
    """``Trainer.step`` on each batch against the table: parameters and slots are snapshotted in fp64 before the step, the rule is
    applied in fp64 to ``trainer.gradient(n)`` clipped in fp64, and the step's result must agree to 1e-6 (parameters) and 1e-5 (slots)
    -- the bounds test_clip_adam_matches_oracle holds Adam to -- with every parameter tensor moved.  ``only``: check these variables
    instead of all.  -> the worst two errors."""
    worst_p = worst_s = 0.0
    for x, nf, y in batches:
        tr.build(x.to(tr.device), nf.to(tr.device), y.to(tr.device))
        a = tr.arena
        assert len(a.slots) == len(TABLE[name][0])

        def views(n):
            lo, k = a.segment(n)[0], a.views[n].numel()
            return [s[lo:lo + k].view(a.views[n].shape) for s in a.slots]
        names = list(only) if only is not None else a.names
        before = {n: (a.views[n].detach().double().cpu().clone(), [s.double().cpu().clone() for s in views(n)]) for n in names}
        out = tr.step(x, nf, y)
        lr = float(out["learning_rate"])
        for n in names:
            p0, s0 = before[n]
            g = clip64(tr.gradient(n).detach().cpu(), tr.clip)
            p1, s1 = rule64(name, p0, g, s0, lr)
            got = a.views[n].detach().cpu()
            assert not torch.equal(got.double(), p0), f"{name}: {n} did not move"
            ep = rel_err(got, p1)
            es = max([rel_err(s.cpu(), r) for s, r in zip(views(n), s1)], default=0.0)
            print(f"{name} step {tr.global_step} {n}: parameters {ep:.3e}, slots {es:.3e}")
            assert ep <= 1e-6, f"{name}: {n}: parameters off by {ep:.3e}"
            assert es <= 1e-5, f"{name}: {n}: slots off by {es:.3e}"
            worst_p, worst_s = max(worst_p, ep), max(worst_s, es)
    return worst_p, worst_s
