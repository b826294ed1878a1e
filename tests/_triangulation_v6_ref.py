"""The restatement of TriangulationV6Module's pooling and head (video_pooling_modules.py:39-138 with attention_modules.OneFcAttention,
attention_modules.py:22-63), written from those lines and from nothing in the package: plain torch in whatever dtype the inputs have
(fp64 is the reference, fp32 on the CPU gives the error the bound is made from).  Shared by the host and the GPU tests."""
import math

import torch

BN_EPS = 1e-3          # slim.batch_norm's default epsilon
L2_EPS = 1e-12         # tf.nn.l2_normalize's


def l2n(v, dim):
    return v * torch.rsqrt(torch.clamp((v * v).sum(dim, keepdim=True), min=L2_EPS))


def embed(x, anchors):
    """:94-106 -> s [N, K*D], feature k * D + d; and the squared norms of the residuals [N, K]"""
    D, K = anchors.shape
    r = x[:, None, :] - anchors.t()[None]                     # tile, subtract, reshape [N, K, D]
    q = (r * r).sum(2)
    e = l2n(r, 2).reshape(-1, K * D)
    return l2n(e, 1), q


def batch_stats(s):
    return s.mean(0), s.var(0, unbiased=False)


def batch_norm(s, gamma, beta, stats=None):
    mean, var = batch_stats(s) if stats is None else stats
    return (s - mean) * torch.rsqrt(var + BN_EPS) * gamma + beta


def attention(v, w, T):
    """attention_modules.py:34-37 -> p [B, T, C]"""
    J, C = w.shape
    logits = (v @ w).reshape(-1, T, C) * (1.0 / math.sqrt(J))
    return torch.softmax(logits, dim=1)


def pool(x, anchors, gamma, beta, w, alpha, shift, T, batch_norm_on=True, stats=None, parts=False):
    """-> y [B, C*J]; with ``parts``: a dict of s, q, mean, var, p, A, z2 (the squared norms of z) and y"""
    J, C = w.shape
    s, q = embed(x, anchors)
    mean = var = None
    v = s
    if batch_norm_on:
        mean, var = batch_stats(s)
        v = batch_norm(s, gamma, beta, stats)
    p = attention(v, w, T)
    A = p.transpose(1, 2) @ v.reshape(-1, T, J)               # [B, C, J]
    z = (alpha * A.reshape(-1, J) + shift)
    y = (l2n(z, 1) * (1.0 / math.sqrt(C))).reshape(-1, C * J)
    if parts:
        return {"s": s, "q": q, "mean": mean, "var": var, "p": p, "A": A, "z2": (z * z).sum(1), "z": z, "y": y}
    return y


def head(y, hidden_weight, gamma2, beta2, batch_norm_on=True, stats=None):
    """:121-136"""
    h = y @ hidden_weight
    if batch_norm_on:
        h = batch_norm(h, gamma2, beta2, stats)
    return torch.relu(h)


NAMES = ("x", "anchors", "gamma", "beta", "w", "alpha", "shift")


def make_inputs(B, T, D, K, C, seed, w_scale=8.0, alpha=1.0, shift=0.01, dtype=torch.float64):
    """Frames ~ N(0, 1), anchors ~ 0.5 N(0, 1), gamma ~ U(0.5, 1.5), beta ~ 0.1 N(0, 1), W ~ w_scale N(0, 1), and the upstream gradient
    dY ~ N(0, 1); drawn in fp64 on the CPU, then cast."""
    g = torch.Generator().manual_seed(1000 * seed + 7)
    J = K * D
    rn = lambda *sh: torch.randn(*sh, generator=g, dtype=torch.float64)
    d = {
        "x": rn(B * T, D),
        "anchors": 0.5 * rn(D, K),
        "gamma": 0.5 + torch.rand(J, generator=g, dtype=torch.float64),
        "beta": 0.1 * rn(J),
        "w": w_scale * rn(J, C),
        "alpha": torch.tensor([alpha], dtype=torch.float64),
        "shift": torch.tensor([shift], dtype=torch.float64),
        "dy": rn(B, C * J),
    }
    return {k: v.to(dtype) for k, v in d.items()}


def conditions(inp, T, batch_norm_on=True, stats=None):
    """What the GPU tests assert of their inputs before any launch -> dict of the four measured margins"""
    P = pool(*(inp[n] for n in NAMES), T, batch_norm_on, stats, parts=True)
    pmax = P["p"].max(dim=1).values                           # [B, C]
    return {"min_q": float(P["q"].min()), "min_z2": float(P["z2"].min()), "max_p": float(pmax.max()),
            "min_pmax_T": float(pmax.min()) * T}


def gradients(inp, T, batch_norm_on=True, stats=None):
    """-> (parts, grads): the parts of ``pool`` and d<y, dy> / d(each of NAMES) (None where the input is unused), in the dtype of ``inp``;
    plus "dalpha_abs" = sum |dz A| and "dshift_abs" = sum |dz|, the scales the two scalar gradients are measured against"""
    leaves = {n: inp[n].clone().requires_grad_(True) for n in NAMES}
    P = pool(*(leaves[n] for n in NAMES), T, batch_norm_on, stats, parts=True)
    P["z"].retain_grad()
    (P["y"] * inp["dy"]).sum().backward()
    grads = {n: leaves[n].grad for n in NAMES}
    dz = P["z"].grad
    grads["dalpha_abs"] = (dz * P["A"].detach().reshape(dz.shape)).abs().sum()
    grads["dshift_abs"] = dz.abs().sum()
    return {k: (v.detach() if torch.is_tensor(v) else v) for k, v in P.items()}, grads
