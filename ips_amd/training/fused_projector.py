"""With-grad, training-mode evaluation of the feature projector on libipsx's kernels - what ``fused_encoder.py`` is for the
conv trunks, for nets on pre-extracted features (``is_image: False``; the reference's CAMELYON configuration: F = 2048,
D = 512, M = 5000, B = 16, i.e. 80,000 rows per step).

Reference: ``training/iterative.py:158-163`` calls ``net(mem_patch, mem_pos)`` under ``net.train()``;
``architecture/ips_net.py:54-60`` is ``LayerNorm(F, elementwise_affine=False) -> Linear(F, D) -> BatchNorm1d(D) -> ReLU``.
On stock ops the LayerNorm writes a normalised copy of the batch and keeps it for backward, the two GEMMs go to rocBLAS,
BatchNorm1d and ReLU are four more passes over (rows, D), and half-stored features are widened first.  The LayerNorm has
no parameters and the features need no gradient, so there is no data-gradient GEMM, and

    z  = |rstd_r| * sum_f (x[r, f] - mean_r) W[o, f] + b[o]
    dW = sum_r (dz[r, :] |rstd_r|)^T (x[r, :] - mean_r),   db = sum_r dz[r, :]

take the RAW rows through the fp32 matrix cores once in each direction (csrc/projector_train.hip); ``(mean, rstd)`` per
row are all that is saved of the LayerNorm.  The forward kernel sums z's columns off its accumulators, so the BatchNorm's
batch statistics cost no pass; BatchNorm + ReLU and their backward are ``ipsx_bn_train_forward_partials`` /
``ipsx_bn_train_backward``.  Modules, parameters, buffers and state dicts stay exactly as they are.

Results equal the stock path to fp32 rounding (another summation order): tests/test_train_projector.py.
``IPSX_TRAIN_PROJECTOR=0`` switches it off.

``encode(encoder, x, rows=)`` is the masked encoder pass: the node on the rows ``x[rows]`` alone - the filled
slots of a zero-padded batch - read where they lie through the int32 index, every intermediate packed at ``rows.numel()``
rows; the bits of ``encode(encoder, x[rows])`` without the gathered copy.
"""
import os

import torch
from torch import nn

from .. import hip


def enabled():
    return os.environ.get("IPSX_TRAIN_PROJECTOR", "1") != "0"


def supported(encoder):
    """True for exactly what ``IPSNet.get_projector`` builds - LayerNorm without affine over the last axis, biased Linear,
    affine BatchNorm1d with running statistics and a momentum, ReLU - at sizes the kernels take."""
    mods = list(encoder.children()) if isinstance(encoder, nn.Sequential) else []
    if len(mods) != 4:
        return False
    ln, lin, bn, act = mods
    if not (type(ln) is nn.LayerNorm and type(lin) is nn.Linear and type(bn) is nn.BatchNorm1d and type(act) is nn.ReLU):
        return False
    if ln.elementwise_affine or tuple(ln.normalized_shape) != (lin.in_features,):
        return False
    if lin.bias is None or lin.weight.dtype != torch.float32 or bn.num_features != lin.out_features:
        return False
    if not (bn.affine and bn.track_running_stats and bn.momentum is not None and bn.running_mean is not None):
        return False
    return hip.projector_train_supported(lin.in_features, lin.out_features)


class _Projector(torch.autograd.Function):
    """relu(batch_norm_train(Linear(LayerNorm(x)))) as ONE node; running statistics updated in place.  Saved: x by
    reference, (mean, rstd) per row, z, y and the BatchNorm's batch statistics."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, ln_eps, bn, rows):
        z, stats, partial, slabs, shift = hip.projector_train_forward(x, weight, bias, ln_eps, index=rows)
        y, mean, invstd = hip.bn_train_forward_partials(z, None, gamma, beta, bn.eps, bn.momentum, bn.running_mean,
                                                        bn.running_var, True, partial, slabs, shift)
        ctx.save_for_backward(x, stats, z, y, gamma, mean, invstd)
        ctx.rows = rows                  # (an index, not an activation: kept by reference like x)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, stats, z, y, gamma, mean, invstd = ctx.saved_tensors
        dy = dy.contiguous()
        dz, _, dgamma, dbeta = hip.bn_train_backward(dy, y, z, gamma, mean, invstd, True, False)
        dw = db = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dw, db = hip.projector_wgrad(x, dz, stats, index=ctx.rows)
        return (None, dw if ctx.needs_input_grad[1] else None, db if ctx.needs_input_grad[2] else None,
                dgamma if ctx.needs_input_grad[3] else None, dbeta if ctx.needs_input_grad[4] else None, None, None, None)


def rows_supported(x, rows):
    """Does ``encode(encoder, x, rows=rows)`` take this source and index?  More than one row (the BatchNorm's batch statistics
    need two values per channel) of a source the indexed kernels can address (below 2 GiB)."""
    return rows.numel() > 1 and hip.projector_train_index_supported(x)


def encode(encoder, x, rows=None):
    """(P, F) feature rows (float32 / float16 / bfloat16) -> (P, D) embeddings; same value as ``encoder(x.float())`` in
    train mode, with the same in-place update of the BatchNorm's running statistics and ``num_batches_tracked``.

    ``rows`` (int32, 1-d, on ``x``'s device, entries in [0, P)): -> the packed (rows.numel(), D) embeddings of ``x[rows]``, the
    batch statistics, the running-statistics update and every gradient those of these rows alone; no other row of ``x`` is
    read.  The caller scatters the packed result where it wants it (``IPSNet._embed_filled``: ATen ``index_copy`` into
    zeros, whose backward gathers the packed ``dy``)."""
    ln, lin, bn, _ = encoder.children()
    if x.requires_grad:
        raise ValueError("the fused projector has no data gradient: the features must not require grad")
    y = _Projector.apply(x, lin.weight, lin.bias, bn.weight, bn.bias, ln.eps, bn, rows)
    bn.num_batches_tracked += 1
    return y
