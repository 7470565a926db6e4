"""fp64 reference of the attention core the kernels of csrc/prh_attn.hpp / prh_attn16.hpp compute, in plain torch:
o = dropout(softmax(q k^T * scale)) v per head of C / H channels, and its gradients.  Operands come in already rounded
the way the storage under test holds them (bf16 K / V as `x.to(torch.bfloat16).double()`), so that what is left between
a kernel and this reference is the kernel's own arithmetic.  Runs on whatever device the operands live on; no GPU needed.
"""
import torch

QT = 32      # queries per tile: the kernels walk M in tiles of 32 and store dK / dV once per tile


def _heads(x, H):
    B, L, C = x.shape
    return x.double().reshape(B, L, H, C // H).transpose(1, 2)          # (B, H, L, d)


def attn_ref(q, k, v, H, scale, keep=None, p=0.0):
    """q (B, M, C), k / v (B, N, C), keep (B, H, M, N) bool or None.  Returns o (B, M, C) and lse (B, H, M): the
    logsumexp of the scaled scores BEFORE dropout, which is what the kernels store for their backward."""
    B, M, C = q.shape
    s = _heads(q, H) @ _heads(k, H).transpose(-1, -2) * scale         # (B, H, M, N)
    lse = torch.logsumexp(s, dim=-1)
    att = torch.exp(s - lse.unsqueeze(-1))
    if keep is not None:
        att = att * keep.to(att.dtype) / (1.0 - p)
    return (att @ _heads(v, H)).transpose(1, 2).reshape(B, M, C), lse


def attn_grads_ref(q, k, v, up, H, scale, keep=None, p=0.0):
    """Gradients of sum(o * up).  Returns (dq, ck, cv): dq (B, M, C); ck / cv lists with one entry per query tile t
    (QT queries): the CUMULATIVE sums c_t of the tiles' contributions to dK / dV.  Tile t's contribution is the
    autograd gradient with `up` zeroed outside the tile - softmax rows are independent, so the contributions add up
    to the full gradient, which is ck[-1] / cv[-1]; the running sums are what a kernel that stores once per tile
    passes through (and, in bf16 storage, rounds)."""
    q, k, v = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    o, _ = attn_ref(q, k, v, H, scale, keep, p)
    M = q.shape[1]
    tiles = range(0, M, QT)
    dq = torch.zeros_like(q)
    ck, cv = [], []
    for t0 in tiles:
        up_t = torch.zeros_like(o)
        up_t[:, t0:t0 + QT] = up[:, t0:t0 + QT].double()
        gq, gk, gv = torch.autograd.grad((o * up_t).sum(), (q, k, v), retain_graph=t0 + QT < M)
        dq += gq
        ck.append(gk if not ck else ck[-1] + gk)
        cv.append(gv if not cv else cv[-1] + gv)
    return dq, ck, cv


def bf16_store_bound(c, floor_rel=2e-5):
    """Elementwise bound on |stored - c[-1]| for a running sum that is rounded to bf16 once per tile: one
    round-to-nearest moves a value by at most 2^-8 of its magnitude, the values rounded are (to first order) the
    c_t; 1.05 covers the second-order terms, the floor is the fp32 gate on the arithmetic in front of the rounding."""
    return 1.05 * 2.0 ** -8 * sum(t.abs() for t in c) + floor_rel * float(c[-1].abs().max())
