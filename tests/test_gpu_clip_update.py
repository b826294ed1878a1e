"""-m gpu: lpm_multi_tensor_clip_update (csrc/clip_update.hip) -- per-variable clip_by_norm fused with the update rules ``--optimizer``
offers beside Adam -- against the rules restated in fp64 (tests/_optimizer_ref.py), and the GPU Trainer under every rule."""
import pytest
import torch

from learnablepoolingmethods_amd import FLAGS, _capi, ops, optimizers, registry
from learnablepoolingmethods_amd._capi import LpmError, ptr, stream_ptr
from learnablepoolingmethods_amd.train import ARENA_ALIGN, Trainer

from tests._optimizer_ref import MU, RULES, TABLE, check_trainer_steps, clip64, rule64
from tests._util import assert_close, cuda, rel_err

pytestmark = pytest.mark.gpu

# six chunks, less than one float4, exactly one chunk, one chunk plus one element, single elements; the last variable's gradient is zero
SHAPES = [(700, 33), (5,), (4096,), (4097,), (123, 7), (1,), (300,)]
SCALES = [3.0, 0.01, 0.05, 1e-3, 1.0, 5.0, 0.0]            # some variables clip, some do not; norm 0: factor 1, nothing may become NaN
LR = 1e-2


def _spec(name):
    return optimizers.by_name(name, momentum=MU)


def _arenas(name, shapes, scales, seed, dev):
    """-> (ps, gs, offs, P, G, slots, offsets): host tensors per variable, and the arenas holding them -- every slot arena filled
    with its rule's initial value, padding included, as ParameterArena does."""
    g = torch.Generator().manual_seed(seed)
    ps = [torch.randn(s, generator=g) for s in shapes]
    gs = [torch.randn(s, generator=g) * c for s, c in zip(shapes, scales)]
    offs, cur = [], 0
    for p in ps:
        offs.append(cur)
        cur += (p.numel() + ARENA_ALIGN - 1) // ARENA_ALIGN * ARENA_ALIGN
    offs.append(cur)
    P, G = torch.zeros(cur, device=dev), torch.zeros(cur, device=dev)
    for p, gr, o in zip(ps, gs, offs):
        P[o:o + p.numel()] = p.flatten().to(dev)
        G[o:o + p.numel()] = gr.flatten().to(dev)
    slots = [torch.full((cur,), init, device=dev) for init in TABLE[name][0]]
    return ps, gs, offs, P, G, slots, torch.tensor(offs, dtype=torch.int64, device=dev)


def _reference(name, ps, gs, clip, steps, coefs=None):
    ref_p = [p.double() for p in ps]
    ref_s = [[torch.full_like(p, init).double() for init in TABLE[name][0]] for p in ps]
    for _ in range(steps):
        for i, g in enumerate(gs):
            g = g.double() + (coefs[i] * ref_p[i] if coefs else 0.0)
            ref_p[i], ref_s[i] = rule64(name, ref_p[i], clip64(g, clip), ref_s[i], LR)
    return ref_p, ref_s


def _check(name, ps, offs, P, slots, ref_p, ref_s, what):
    assert bool(torch.isfinite(P).all()) and all(bool(torch.isfinite(s).all()) for s in slots), f"{name}: non-finite values ({what})"
    for i, (p, o) in enumerate(zip(ps, offs)):
        ep = rel_err(P[o:o + p.numel()].reshape(p.shape), ref_p[i])
        es = max([rel_err(s[o:o + p.numel()].reshape(p.shape), r) for s, r in zip(slots, ref_s[i])], default=0.0)
        print(f"{name} {what} variable {i} {tuple(p.shape)}: parameters {ep:.3e}, slots {es:.3e}")
        assert ep <= 1e-6, f"{name} {what}: variable {i}: parameters off by {ep:.3e}"
        assert es <= 1e-5, f"{name} {what}: variable {i}: slots off by {es:.3e}"


@pytest.mark.parametrize("clip", [1.0, 0.0])
@pytest.mark.parametrize("name", RULES)
def test_clip_update_matches_fp64(name, clip):
    dev = cuda()
    ps, gs, offs, P, G, slots, offsets = _arenas(name, SHAPES, SCALES, 0, dev)
    scratch = None
    for _ in range(3):
        scratch = ops.clip_update_step(_spec(name), P, G, slots, offsets, len(ps), clip, LR, scratch=scratch)
    ref_p, ref_s = _reference(name, ps, gs, clip, 3)
    _check(name, ps, offs, P, slots, ref_p, ref_s, f"clip {clip}")
    assert torch.equal(P[offs[-2]:offs[-2] + 300].cpu(), ps[-1])         # the variable whose gradient is zero stays where it is


@pytest.mark.parametrize("name", RULES)
def test_clip_update_adds_the_l2_penalty_gradient_on_the_fly(name):
    """The ``l2`` vector against an explicit ``grad += c * w`` pass in front of the same call without it, and both against fp64 -- the
    shapes and coefficients of test_clip_adam_adds_the_l2_penalty_gradient_on_the_fly (the third variable's penalty decides whether it clips)."""
    dev = cuda()
    shapes, scales, coefs = [(700, 33), (5,), (9000,), (123, 7)], [3.0, 0.01, 1e-4, 1.0], [0.0, 0.5, 30.0, 1e-2]
    ps, gs, offs, P, G, slots, offsets = _arenas(name, shapes, scales, 1, dev)
    l2 = torch.tensor(coefs, dtype=torch.float32, device=dev)
    P2, slots2 = P.clone(), [s.clone() for s in slots]
    for _ in range(3):
        ops.clip_update_step(_spec(name), P, G, slots, offsets, len(ps), 1.0, LR, l2=l2)
        G2 = G.clone()
        for c, p, o in zip(coefs, ps, offs):
            G2[o:o + p.numel()].add_(P2[o:o + p.numel()], alpha=c)
        ops.clip_update_step(_spec(name), P2, G2, slots2, offsets, len(ps), 1.0, LR)
    ref_p, ref_s = _reference(name, ps, gs, 1.0, 3, coefs=coefs)
    _check(name, ps, offs, P, slots, ref_p, ref_s, "l2 on the fly")
    _check(name, ps, offs, P2, slots2, ref_p, ref_s, "l2 by an add pass")
    assert_close(P, P2.double(), tol=1e-7, what=f"{name}: against the add pass + the call without l2")
    for s, s2 in zip(slots, slots2):
        assert_close(s, s2.double(), tol=1e-6, what=f"{name}: slots against the add pass + the call without l2")


@pytest.mark.parametrize("name", RULES)
def test_clip_update_gives_the_same_bits_twice(name):
    dev = cuda()
    runs = []
    for _ in range(2):
        ps, gs, offs, P, G, slots, offsets = _arenas(name, SHAPES, SCALES, 2, dev)
        for _ in range(2):
            ops.clip_update_step(_spec(name), P, G, slots, offsets, len(ps), 1.0, LR)
        runs.append([P] + slots)
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_unused_slots_are_neither_passed_nor_touched():
    """GradientDescent with ``slots=()`` and Adagrad with one slot: the arenas a rule does not keep go in as NULL."""
    dev = cuda()
    for name in ("GradientDescentOptimizer", "AdagradOptimizer"):
        ps, gs, offs, P, G, slots, offsets = _arenas(name, SHAPES, SCALES, 3, dev)
        assert len(slots) == {"GradientDescentOptimizer": 0, "AdagradOptimizer": 1}[name]
        ops.clip_update_step(_spec(name), P, G, tuple(slots), offsets, len(ps), 1.0, LR)
        ref_p, ref_s = _reference(name, ps, gs, 1.0, 1)
        _check(name, ps, offs, P, slots, ref_p, ref_s, "exactly its own slots")
        with pytest.raises(LpmError, match="slot arena"):
            ops.clip_update_step(_spec(name), P, G, slots + [torch.zeros_like(P)], offsets, len(ps), 1.0, LR)


def test_entry_refuses_an_unknown_kind_and_a_missing_slot():
    """Error codes from the entry's argument checks: nothing is launched, the parameter arena keeps its bits."""
    dev = cuda()
    lib = _capi.load()
    ps, gs, offs, P, G, slots, offsets = _arenas("AdadeltaOptimizer", SHAPES[:2], SCALES[:2], 4, dev)
    scratch = torch.empty(lib._lpm_clip_adam_scratch_bytes(P.numel(), 2) // 4, dtype=torch.float32, device=dev)
    before = P.clone()

    def call(kind, s0, s1, total=P.numel()):
        return lib._lpm_multi_tensor_clip_update(kind, ptr(P), ptr(G), ptr(s0), ptr(s1), ptr(offsets), None, 2, total, 1.0, LR, 0.9, 1e-8,
                                                 ptr(scratch), stream_ptr())
    assert call(0, slots[0], slots[1]) != 0 and "unknown kind" in lib.last_error()            # (0 is Adam's: not this entry's)
    assert call(99, slots[0], slots[1]) != 0 and "unknown kind" in lib.last_error()
    for kind in (2, 3, 4, 5):
        assert call(kind, None, slots[1]) != 0 and "null pointer" in lib.last_error()
    assert call(5, slots[0], None) != 0 and "null pointer" in lib.last_error()
    assert call(1, None, None, total=P.numel() - 2) != 0 and "multiple of 4" in lib.last_error()
    assert call(3, slots[0][1:], None) != 0 and "16-byte aligned" in lib.last_error()
    torch.cuda.synchronize()
    assert torch.equal(P, before)


def _batch(seed, B=8, F=16 + 8, V=40):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, F, generator=g) * 3.0, torch.ones(B, dtype=torch.int32), torch.rand(B, V, generator=g) < 0.15


def _moe_trainer(dev, **kw):
    return Trainer(registry.get_model("MoeModel"), vocab_size=40, batch_size=8, base_learning_rate=1e-2, device=dev, seed=3,
                   model_kwargs=dict(num_mixtures=2), **kw)


@pytest.mark.parametrize("name", RULES)
def test_gpu_trainer_steps_follow_the_table_in_fp64(name):
    """MoeModel on [8, 24] features, V = 40 (test_moe_step_against_an_fp64_restatement's shapes), two steps: the GPU's own gradient,
    then the fp64 rule.  (The MoE weights' L2 penalty rides in the update pass: FLAGS.fold_l2_into_update.)"""
    dev = cuda()
    try:
        tr = _moe_trainer(dev, optimizer=name, optimizer_momentum=MU)
        check_trainer_steps(tr, name, [_batch(47), _batch(48)], rel_err)
        assert tr.factored is None and tr.sharded is None and tr.arena.m is None and len(tr.arena.slots) == len(TABLE[name][0])
        assert tr._l2_fold is not None and sorted(tr._l2_folded) == ["tower/experts/weights", "tower/gates/weights"]
    finally:
        FLAGS.reset()


def test_hidden1_weights_takes_the_generic_route_under_another_rule():
    """NetVladV1 (K = 16, hidden 128, 30 x 1152): under a rule other than Adam none of hidden1_weights' Adam routes is taken -- its
    gradient is written into the arena by its producer and the variable is updated with all the others."""
    dev = cuda()
    g = torch.Generator().manual_seed(5)
    x, nf = torch.randn(4, 30, 1152, generator=g), torch.tensor([30, 20, 10, 25], dtype=torch.int32)
    y = torch.rand(4, 50, generator=g) < 0.1
    try:
        tr = Trainer(registry.get_model("NetVladV1"), vocab_size=50, batch_size=4, base_learning_rate=1e-3, device=dev,
                     model_kwargs=dict(iterations=30, cluster_size=16, hidden_size=128), optimizer="MomentumOptimizer", optimizer_momentum=MU)
        tr.build(x.to(dev), nf.to(dev), y.to(dev))
        h1 = "tower/hidden1_weights"
        assert tr.factored is None and tr.sharded is None and tr.w16 is None and h1 in {d[0] for d in tr.arena.direct}
        check_trainer_steps(tr, "MomentumOptimizer", [(x, nf, y)], rel_err, only=(h1, "tower/gates/weights"))
        assert tr._early is None
    finally:
        FLAGS.reset()


def test_adam_is_unchanged_by_spelling_it_out():
    dev = cuda()
    try:
        finals = []
        for kw in ({}, {"optimizer": "AdamOptimizer"}):
            tr = _moe_trainer(dev, **kw)
            for seed in (47, 48):
                tr.step(*_batch(seed))
            assert tr.optimizer.name == "AdamOptimizer" and tr.arena.slots[0] is tr.arena.m and tr.arena.slots[1] is tr.arena.v
            finals.append((tr.arena.param.clone(), tr.arena.m.clone(), tr.arena.v.clone()))
        for a, b in zip(*finals):
            assert torch.equal(a, b)
    finally:
        FLAGS.reset()
