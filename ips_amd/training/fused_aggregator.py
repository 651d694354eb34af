"""With-grad evaluation of the cross-attention aggregator on libipsx's kernels - what ``fused_projector.py`` is for the
feature projector, for ``Transformer.forward`` under autograd (reference training/iterative.py:158-163 calls
``net(mem_patch, mem_pos)`` under ``net.train()``; architecture/transformer.py:43-152).

On stock ops the step projects all B * M embeddings through ``k_w`` and ``v_w`` (two (B M, D) x (D, H D_k) GEMMs forward,
four more backward, K and V kept for backward) to feed H * n_token attention rows per slide.  None of it is needed: the
scaled query folds into ``k_w`` (the no-grad path's ``folded_query``), and the softmax weights sum over the patches BEFORE
``v_w`` is applied.  With R = H * T rows r = h * T + t:

    A[h*T+t, :]   = sum_j Qs[t, h, j] * k_w[h*D_k + j, :]          Qs = (q @ q_w^T) / temperature
    L[b, m, r]    = x[b, m, :] . A[r, :]
    P[b, r, :]    = softmax_m L[b, :, r]          P' = P * keep      (keep: attention dropout, 0 or 1/(1-p); absent = ones)
    Z[b, r, :]    = sum_m P'[b, r, m] * x[b, m, :]
    ctx[b, t, h*D_v + j] = Z[b, h*T+t, :] . v_w[h*D_v + j, :]

Everything before ``A`` and after ``Z`` works on R or B * T rows and stays on stock autograd ops, which also carry the
gradients of ``q``, ``q_w``, ``k_w``, ``v_w``.  ``Z = pool(x, A, keep)`` is ONE autograd node on csrc/attn_pool_train.hip;
its backward (``aten_pool`` below differentiated by hand; c[b, r] = dZ[b, r, :] . Z[b, r, :] is the softmax-backward row
constant, since sum_m P' dP' = dZ . Z):

    dP'[b, r, m] = dZ[b, r, :] . x[b, m, :]
    dL[b, m, r]  = P[b, r, m] * (keep[b, r, m] * dP'[b, r, m] - c[b, r])
    dx[b, m, :]  = sum_r P'[b, r, m] * dZ[b, r, :] + sum_r dL[b, m, r] * A[r, :]
    dA[r, :]     = sum_b sum_m dL[b, m, r] * x[b, m, :]

Modules, parameters and state dicts stay exactly as they are.  Results equal the stock path to fp32 rounding (another
summation order): tests/test_train_aggregator.py.  ``IPSX_TRAIN_AGGREGATOR=0`` switches it off.
"""
import os

import torch
import torch.nn.functional as F
from torch import nn

from .. import hip


def enabled():
    return os.environ.get("IPSX_TRAIN_AGGREGATOR", "1") != "0"


def supported(transf):
    """True for exactly what ``Transformer(...)`` builds - the plain attention / MLP module types, bias-free float32
    ``q_w`` / ``k_w`` / ``v_w`` / ``fc`` - at sizes the kernels take."""
    from ..architecture import transformer as tr
    ca, mlp = getattr(transf, "crs_attn", None), getattr(transf, "mlp", None)
    if not (type(transf) is tr.Transformer and type(ca) is tr.MultiHeadCrossAttention and type(mlp) is tr.MLP
            and type(ca.attention) is tr.ScaledDotProductAttention and type(ca.attention.dropout) is nn.Dropout):
        return False
    for lin in (ca.q_w, ca.k_w, ca.v_w, ca.fc):
        if type(lin) is not nn.Linear or lin.bias is not None or lin.weight.dtype != torch.float32:
            return False
    D = ca.q.shape[2]
    if ca.q.dtype != torch.float32 or ca.k_w.weight.shape != (ca.H * ca.D_k, D) or ca.v_w.weight.shape != (ca.H * ca.D_v, D):
        return False
    return hip.attn_pool_supported(ca.H * ca.n_token, D)


def aten_pool(x, A, keep=None, count=None):
    """The pool in ATen ops (any device and dtype): what ``_AttnPool`` computes, and the definition of its backward.
    ``count`` (an integer tensor (B,), or B ints): image b's softmax runs over its rows m < count[b]; the others are filled
    with -inf first, so they get probability +0.0, add nothing to Z and receive gradient 0."""
    L = torch.matmul(x, A.t())                                                # (B, M, R)
    if count is not None:
        beyond = torch.arange(x.shape[1], device=x.device)[None, :] >= torch.as_tensor(count, device=x.device)[:, None]
        L = L.masked_fill(beyond[:, :, None], float("-inf"))
    P = torch.softmax(L, dim=1).transpose(1, 2)                               # (B, R, M)
    if keep is not None:
        P = P * keep
    return torch.matmul(P, x)


class _AttnPool(torch.autograd.Function):
    """Z = pool(x, A, keep, count) as ONE node.  Saved: x by reference, A, keep, count, P (B, R, M), Z."""

    @staticmethod
    def forward(ctx, x, A, keep, count=None):
        if count is not None:          # (checked once, on the way in: the backward gets the device tensor)
            count = hip.slot_counts("attn_pool", count, x.shape[0], x.shape[1], x.device)
        Z, P = hip.attn_pool_forward(x, A, keep, count)
        ctx.save_for_backward(x, A, keep, count, P, Z)
        return Z

    @staticmethod
    def backward(ctx, dZ):
        x, A, keep, count, P, Z = ctx.saved_tensors
        dx, dA = hip.attn_pool_backward(x, A, keep, P, Z, dZ.contiguous(), want_dx=ctx.needs_input_grad[0], count=count)
        return dx, dA if ctx.needs_input_grad[1] else None, None, None


def hip_pool(x, A, keep=None, count=None):
    return _AttnPool.apply(x if x.is_contiguous() else x.contiguous(), A.contiguous(), keep, count)


def forward(transf, x, keep=None, pool=None, count=None):
    """``transf.mlp(transf.crs_attn(x))`` of (B, M, D) embeddings -> (B, n_token, D), the (B, M) part as one node.
    ``keep``: the attention-dropout factors (B, H * n_token, M); drawn here when the attention dropout is active.
    ``pool``: another evaluation of ``aten_pool`` (default: the HIP node).
    ``count``: the filled slots per image (``aten_pool``); handed to ``pool`` as its fourth argument when given."""
    ca = transf.crs_attn
    B, M, D = x.shape
    H, T = ca.H, ca.n_token
    qs = ca.q_w(ca.q).view(T, H, ca.D_k) / ca.attention.temperature
    A = torch.matmul(qs.transpose(0, 1), ca.k_w.weight.view(H, ca.D_k, D)).reshape(H * T, D)        # row h * T + t
    drop = ca.attention.dropout
    if keep is None and drop.training and drop.p > 0:
        keep = F.dropout(torch.ones((B, H * T, M), dtype=x.dtype, device=x.device), drop.p, True)
    pool = hip_pool if pool is None else pool
    Z = pool(x, A, keep) if count is None else pool(x, A, keep, count)
    ctx = torch.matmul(Z.view(B, H, T, D), ca.v_w.weight.view(H, ca.D_v, D).transpose(1, 2))          # (B, H, T, D_v)
    ctx = ctx.transpose(1, 2).contiguous().view(B, T, -1)
    out = ca.dropout(ca.fc(ctx))
    out += ca.q
    return transf.mlp(ca.layer_norm(out))
