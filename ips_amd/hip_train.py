"""The training step's kernels behind ``training/fused_encoder.py`` (reference training/iterative.py:158-163: the with-grad
forward of the M selected patches and its backward): convolutions forward / data gradient / weight gradient, BatchNorm in
batch-statistics mode, the max-pool - ctypes bindings of csrc/bn_train.hip, conv_wgrad.hip, dgrad_s2.hip, stem_train.hip,
pool_train.hip (split out of ``hip.py`` in round 6; ``ips_amd.hip`` re-exports every public name) - and, behind
``training/fused_projector.py``, the feature projector's two GEMMs (csrc/projector_train.hip), and behind
``training/fused_aggregator.py`` the attention pool on folded queries (csrc/attn_pool_train.hip)."""

import ctypes as C
import os

import torch

from .hip import (lib, _ck, _p, _f32, _stream, _PATCH_DTYPES, Conv, _gpu_device, _one_gpu, _rd, _wr, slot_counts)
from .hip_encoder import _pack_conv


# ---------------------------------------------------------------- training step (with-grad forward of the trunk)
_CL = torch.channels_last


def conv_train_supported(conv):
    """Can the training step's convolutions of ``conv`` (an nn.Conv2d) run on the kernels of libipsx?  Forward and data
    gradient: ``ipsx_conv2d_affine_nhwc`` (C_in % 32 == 0); weight gradient: ``ipsx_conv2d_wgrad_nhwc`` (channels % 64 == 0);
    strided layers need "same" padding for the data gradient's formulation (kernel - 1 = 2 pad)."""
    kh, kw = conv.kernel_size
    s, p = conv.stride[0], conv.padding[0]
    if (conv.bias is not None or conv.groups != 1 or conv.dilation != (1, 1) or conv.stride[0] != conv.stride[1]
            or conv.padding[0] != conv.padding[1] or kh != kw or conv.weight.dtype != torch.float32):
        return False
    if s > 1 and kh - 1 != 2 * p:
        return False
    if conv.in_channels % 32 != 0 and conv.in_channels != 1:    # forward kernels: channels-last (C_in % 32 == 0) or the 1-channel stem
        return False
    return bool(lib().ipsx_conv2d_wgrad_nhwc_supported(conv.in_channels, conv.out_channels, kh, kw, s, p))


def _pack_conv_view(weight, dgrad=False):
    """``_pack_conv`` of a weight tensor as it lies in memory (any strides: no contiguous copy) - or, ``dgrad``, of the
    weights rotated by 180 degrees and transposed: -> (packed, C_out, C_in) of the convolution they describe."""
    _conv_weight("pack_conv_view", weight)
    co, ci, kh, kw = weight.shape
    s_co, s_ci, s_kh, s_kw = weight.stride()
    if dgrad:
        n_out, n_in = ci, co
        base, sn, sc, sky, skx = (kh - 1) * s_kh + (kw - 1) * s_kw, s_ci, s_co, -s_kh, -s_kw
    else:
        n_out, n_in = co, ci
        base, sn, sc, sky, skx = 0, s_co, s_ci, s_kh, s_kw
    packed = torch.empty(lib().ipsx_packed_conv_weight_elems(n_out, n_in, kh, kw), dtype=torch.float32, device=weight.device)
    _ck(lib().ipsx_pack_conv_weight_strided(_p(weight), base, n_out, n_in, kh, kw, sn, sc, sky, skx, _p(packed), _stream()),
        "ipsx_pack_conv_weight_strided")
    return packed, n_out, n_in


def _conv_weight(what, weight, dev=None):
    """An OIHW float32 weight on the GPU (``dev``: on that one), read where it lies - any strides, 4-byte loads."""
    if weight.dim() != 4 or weight.dtype != torch.float32 or not _gpu_device(weight.device) or (dev is not None and weight.device != dev):
        raise ValueError("{}: weight must be a float32 OIHW tensor on the call's GPU, got {} {} on {}".format(
            what, weight.dtype, tuple(weight.shape), weight.device))


class PackJob(C.Structure):
    """``ipsx_pack_job`` of include/ipsx.h"""
    _fields_ = [("w", C.c_void_p), ("base", C.c_int64), ("c_out", C.c_int), ("c_in", C.c_int), ("kh", C.c_int), ("kw", C.c_int),
                ("s_out", C.c_int64), ("s_in", C.c_int64), ("s_ky", C.c_int64), ("s_kx", C.c_int64), ("packed", C.c_void_p)]


_PACK_BATCH_MAX = 32


def pack_conv_views(views):
    """``_pack_conv_view`` of several (weight, dgrad) pairs as ONE launch per 32 (ipsx_pack_conv_weights_batch): the packed
    tensors are slices of one buffer.  -> list of packed tensors, in the order of ``views``."""
    if not views:
        return []
    dev = views[0][0].device
    sizes = []
    for weight, dgrad in views:
        _conv_weight("pack_conv_views", weight, dev)
    for weight, dgrad in views:
        co, ci, kh, kw = weight.shape
        n_out, n_in = (ci, co) if dgrad else (co, ci)
        sizes.append(lib().ipsx_packed_conv_weight_elems(n_out, n_in, kh, kw))
    arena = torch.empty(sum(sizes), dtype=torch.float32, device=dev)
    out, off = [], 0
    for sz in sizes:
        out.append(arena[off:off + sz])
        off += sz
    for k0 in range(0, len(views), _PACK_BATCH_MAX):
        chunk = views[k0:k0 + _PACK_BATCH_MAX]
        jobs = (PackJob * len(chunk))()
        for j, (weight, dgrad) in enumerate(chunk):
            co, ci, kh, kw = weight.shape
            s_co, s_ci, s_kh, s_kw = weight.stride()
            if dgrad:
                jobs[j].c_out, jobs[j].c_in = ci, co
                jobs[j].base, jobs[j].s_out, jobs[j].s_in, jobs[j].s_ky, jobs[j].s_kx = (kh - 1) * s_kh + (kw - 1) * s_kw, s_ci, s_co, -s_kh, -s_kw
            else:
                jobs[j].c_out, jobs[j].c_in = co, ci
                jobs[j].base, jobs[j].s_out, jobs[j].s_in, jobs[j].s_ky, jobs[j].s_kx = 0, s_co, s_ci, s_kh, s_kw
            jobs[j].kh, jobs[j].kw = kh, kw
            jobs[j].w, jobs[j].packed = weight.data_ptr(), out[k0 + j].data_ptr()
        _ck(lib().ipsx_pack_conv_weights_batch(C.byref(jobs), len(chunk), _stream()), "ipsx_pack_conv_weights_batch")
    return out


def conv_lds_supported(conv, h, w):
    """True when ``conv2d_nhwc`` would run this ``nn.Conv2d`` on a kernel that can hand the BatchNorm behind it its batch
    statistics (``conv2d_nhwc(..., stats_shift=...)``): the LDS-resident stage kernels (maps of 32-px patches) and the
    1-channel stem on the matrix cores."""
    kh, kw = conv.kernel_size
    if os.environ.get("IPSX_TRAIN_CONV_STATS", "1") == "0":
        return False
    if conv.in_channels == 1:                    # the 32-px trunk's stem on the matrix cores (csrc/stem_train.hip)
        return bool(os.environ.get("IPSX_TRAIN_STEM_MFMA", "1") != "0" and lib().ipsx_stem7x7s2_nhwc_supported(
            1, conv.out_channels, kh, kw, conv.stride[0], conv.padding[0], h, w))
    return bool(kh == kw and os.environ.get("IPSX_TRAIN_CONV_LDS", "1") != "0"
                and lib().ipsx_conv2d_lds_nhwc_supported(conv.in_channels, conv.out_channels, kh, conv.stride[0], conv.padding[0], h, w))


def _activation(what, name, x, shape=None):
    """A saved activation: float32 channels-last (P, C, H, W) at a 16-byte address (the kernels' 16-byte buffer loads),
    handed over where it lies - anything else is refused, never copied."""
    if x.dim() != 4 or x.dtype != torch.float32 or not x.is_contiguous(memory_format=_CL) or x.data_ptr() % 16 or \
            (shape is not None and tuple(x.shape) != tuple(shape)):
        raise ValueError("{}: {} - expected a float32 channels-last (P, C, H, W){} tensor at a 16-byte address, got {} {} with "
                         "strides {}".format(what, name, " = " + str(tuple(shape)) if shape is not None else "", x.dtype, tuple(x.shape),
                                             x.stride()))
    return x


def conv2d_nhwc(x, weight, stride, pad, dgrad_weights=False, packed=None, stats_shift=None):
    """Plain convolution of a channels-last (P, C_in, h, w) tensor with an OIHW ``weight`` on the fp32 matrix cores
    (conv_nhwc_kernel): -> channels-last (P, C_out, ho, wo).  ``packed``: the weight already packed for this direction
    (``pack_conv_views``).  ``stats_shift`` (a (C_out,) tensor; only where ``conv_lds_supported``): -> (y, partial, slabs),
    the output's per-slab sums around that shift for ``bn_train_forward_partials``."""
    _one_gpu("conv2d_nhwc", x=x, weight=weight, packed=packed, stats_shift=stats_shift)
    _activation("conv2d_nhwc", "x", x)
    _conv_weight("conv2d_nhwc", weight)
    kh, kw = weight.shape[2:]
    n, _, h, w = x.shape
    ho, wo = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
    co, ci = (weight.shape[1], weight.shape[0]) if dgrad_weights else (weight.shape[0], weight.shape[1])
    if x.shape[1] != ci:
        raise ValueError("conv2d_nhwc: x has {} channels, weight takes {}".format(x.shape[1], ci))
    if packed is not None:
        _wr("conv2d_nhwc", "packed", packed, torch.float32, align=16)
    if stats_shift is not None:
        _wr("conv2d_nhwc", "stats_shift", stats_shift, torch.float32, (co,))
    if packed is None:
        packed = _pack_conv_view(weight.detach(), dgrad_weights)[0]
    cv = Conv(ci, co, kh, kw, stride, pad, _p(packed), None, None, None)
    y = torch.empty((n, co, ho, wo), dtype=torch.float32, device=x.device, memory_format=_CL)
    if n == 0:                                  # (an empty batch: nothing to launch)
        return (y, torch.zeros((1, 2, co), dtype=torch.float32, device=x.device), 0) if stats_shift is not None else y
    if stats_shift is not None:
        slabs = int(lib().ipsx_conv2d_lds_nhwc_stats_slabs(n))
        partial = torch.empty((max(slabs, 1), 2, co), dtype=torch.float32, device=x.device)
        if ci == 1:
            _ck(lib().ipsx_stem7x7s2_nhwc(C.byref(cv), _p(x), _p(y), n, _p(stats_shift), _p(partial), _stream()), "ipsx_stem7x7s2_nhwc")
        else:
            _ck(lib().ipsx_conv2d_lds_nhwc_stats(C.byref(cv), _p(x), _p(y), n, h, w, _p(stats_shift), _p(partial), _stream()),
                "ipsx_conv2d_lds_nhwc_stats")
        return y, partial, slabs
    if kh == kw and os.environ.get("IPSX_TRAIN_CONV_LDS", "1") != "0" and lib().ipsx_conv2d_lds_nhwc_supported(ci, co, kh, stride, pad, h, w):
        # the maps of 32-px patches: the fused trunk's stage kernels, map LDS-resident for all taps
        _ck(lib().ipsx_conv2d_lds_nhwc(C.byref(cv), _p(x), _p(y), n, h, w, _stream()), "ipsx_conv2d_lds_nhwc")
    elif ci == 1 and os.environ.get("IPSX_TRAIN_STEM_MFMA", "1") != "0" and lib().ipsx_stem7x7s2_nhwc_supported(ci, co, kh, kw, stride, pad, h, w):
        # the 32-px trunk's stem on the matrix cores (csrc/stem_train.hip)
        _ck(lib().ipsx_stem7x7s2_nhwc(C.byref(cv), _p(x), _p(y), n, None, None, _stream()), "ipsx_stem7x7s2_nhwc")
    elif ci == 1:       # one input channel (NCHW = channels-last memory): the stem kernel, channels-last output
        _ck(lib().ipsx_conv2d_affine_to_nhwc(C.byref(cv), _p(x), None, _p(y), n, h, w, 0, _stream()), "ipsx_conv2d_affine_to_nhwc")
    else:
        _ck(lib().ipsx_conv2d_affine_nhwc(C.byref(cv), _p(x), None, _p(y), n, h, w, 0, _stream()), "ipsx_conv2d_affine_nhwc")
    return y


def conv2d_nhwc_dgrad(dy, weight, stride, pad, in_hw, packed=None):
    """Data gradient of ``conv2d_nhwc``: the same kernel on dy with the weights rotated by 180 degrees and transposed; a
    strided layer first spreads dy over a zero map of the input's size (needs kernel - 1 = 2 pad)."""
    _one_gpu("conv2d_nhwc_dgrad", dy=dy, weight=weight, packed=packed)
    _conv_weight("conv2d_nhwc_dgrad", weight)
    co, ci, kh, kw = weight.shape
    ho, wo = (in_hw[0] + 2 * pad - kh) // stride + 1, (in_hw[1] + 2 * pad - kw) // stride + 1
    if dy.dim() != 4 or tuple(dy.shape[1:]) != (co, ho, wo):
        raise ValueError("conv2d_nhwc_dgrad: dy - expected float32 (P, %d, %d, %d), got %s" % (co, ho, wo, tuple(dy.shape)))
    dy = _rd("conv2d_nhwc_dgrad", "dy", dy, cl=True)          # (a gradient is read only: any layout, copied to channels-last)
    if packed is not None:
        _wr("conv2d_nhwc_dgrad", "packed", packed, torch.float32, align=16)
    if (stride > 1 and kh == kw and os.environ.get("IPSX_TRAIN_DGRAD_S2", "1") != "0"
            and lib().ipsx_conv2d_dgrad_s2_lds_nhwc_supported(ci, co, kh, stride, pad, in_hw[0], in_hw[1])):
        # the 32-px trunk's strided layer by parity class of the input pixel: no spread map (csrc/dgrad_s2.hip)
        if packed is None:
            packed = _pack_conv_view(weight.detach(), True)[0]
        n = dy.shape[0]
        dx = torch.empty((n, ci, in_hw[0], in_hw[1]), dtype=torch.float32, device=dy.device, memory_format=_CL)
        _ck(lib().ipsx_conv2d_dgrad_s2_lds_nhwc(_p(packed), kh, _p(dy), _p(dx), n, _stream()), "ipsx_conv2d_dgrad_s2_lds_nhwc")
        return dx
    if stride > 1:
        n = dy.shape[0]
        spread = torch.empty((n, co, in_hw[0], in_hw[1]), dtype=torch.float32, device=dy.device, memory_format=_CL).zero_()
        spread[:, :, ::stride, ::stride] = dy
        dy = spread
    return conv2d_nhwc(dy, weight, 1, kh - 1 - pad, dgrad_weights=True, packed=packed)


# ipsx_conv2d_wgrad_nhwc addresses x and dy through 32-bit buffer offsets: either activation of ONE call stays below this
# many bytes (csrc/conv_wgrad.hip: "call per slice and add"); conv2d_nhwc_wgrad slices the image axis accordingly
_WGRAD_MAX_BYTES = (1 << 31) - (1 << 20)


def conv2d_nhwc_wgrad(x, dy, weight_shape, stride, pad):
    """Weight gradient of ``conv2d_nhwc`` -> (C_out, C_in, kh, kw) in channels-last memory order (ipsx_conv2d_wgrad_nhwc).
    Activations of 2 GiB and more (the kernel's buffer range) are taken in slices of whole images, the slices' gradients
    added in slice order (deterministic; the forward kernel slices per launch in the same way)."""
    _one_gpu("conv2d_nhwc_wgrad", x=x, dy=dy)
    co, ci, kh, kw = weight_shape
    _activation("conv2d_nhwc_wgrad", "x", x)          # (the saved activation: refused as conv2d_nhwc refuses it)
    n, _, h, w = x.shape
    ho, wo = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
    if x.shape[1] != ci or dy.dim() != 4 or tuple(dy.shape) != (n, co, ho, wo):
        raise ValueError("conv2d_nhwc_wgrad: x {} and dy {} - expected ({}, {}, {}, {}) and ({}, {}, {}, {})".format(
            tuple(x.shape), tuple(dy.shape), n, ci, h, w, n, co, ho, wo))
    dy = _rd("conv2d_nhwc_wgrad", "dy", dy, cl=True)
    per_image = 4 * max(h * w * ci, ho * wo * co)
    step = max(1, min(n, _WGRAD_MAX_BYTES // per_image))
    dw = torch.empty((co, ci, kh, kw), dtype=torch.float32, device=x.device, memory_format=_CL)
    nb = max(lib().ipsx_conv2d_wgrad_nhwc_workspace_bytes(c, ci, co, kh, kw) for c in {step, n - (n - 1) // step * step})
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=x.device)
    part = dw
    for i0 in range(0, max(n, 1), step):
        cnt = min(step, n - i0)
        if i0 > 0 and part is dw:
            part = torch.empty_like(dw)
        _ck(lib().ipsx_conv2d_wgrad_nhwc(_p(x[i0:i0 + cnt]), _p(dy[i0:i0 + cnt]), cnt, h, w, ci, co, kh, kw, stride, pad,
                                         _p(part), _p(ws), nb, _stream()), "ipsx_conv2d_wgrad_nhwc")
        if part is not dw:
            dw += part
    return dw


def _rows_cl(t, name="x"):
    """(P, C, H, W) channels-last tensor, or (rows, C) rows as they lie (BatchNorm1d) -> (rows, C) of its memory.  The
    BatchNorm kernels read and write whole float4 (csrc/bn_train.hip): the address is a multiple of 16."""
    if t.data_ptr() % 16:
        raise ValueError("{}: expected a tensor at a 16-byte address".format(name))
    if t.dim() == 2 and t.dtype == torch.float32 and t.is_contiguous():
        return t.shape[0], t.shape[1]
    if t.dim() != 4 or t.dtype != torch.float32 or not t.is_contiguous(memory_format=torch.channels_last):
        raise ValueError("{}: expected a float32 channels-last (P, C, H, W) tensor, got {} {}".format(name, t.dtype, tuple(t.shape)))
    return t.shape[0] * t.shape[2] * t.shape[3], t.shape[1]


def _bn_args(what, x, residual, gamma, beta, running_mean, running_var, **more):
    """The arguments the two BatchNorm forwards share, checked -> (rows, c, gamma, beta): ``gamma`` / ``beta`` (C,) are read
    as float4 (copied where they are strided or off a 16-byte address); ``running_mean`` / ``running_var`` (C,) are updated
    in place with 4-byte stores: handed over where they lie."""
    _one_gpu(what, x=x, residual=residual, gamma=gamma, beta=beta, running_mean=running_mean, running_var=running_var, **more)
    rows, c = _rows_cl(x)
    if residual is not None and (_rows_cl(residual, "residual") != (rows, c) or residual.shape != x.shape):
        raise ValueError("{}: residual {} beside x {}".format(what, tuple(residual.shape), tuple(x.shape)))
    gamma, beta = _rd(what, "gamma", gamma.detach(), dim=1), _rd(what, "beta", beta.detach(), dim=1)
    if gamma.shape[0] != c or beta.shape[0] != c:
        raise ValueError("{}: gamma {} / beta {} for {} channels".format(what, tuple(gamma.shape), tuple(beta.shape), c))
    for name, t in (("running_mean", running_mean), ("running_var", running_var)):
        if t is not None:
            _wr(what, name, t, torch.float32, (c,))
    return rows, c, gamma, beta


def bn_train_supported(rows, c):
    return bool(lib().ipsx_bn_train_supported(rows, c))


def bn_train_forward(x, residual, gamma, beta, eps, momentum, running_mean, running_var, relu):
    """Batch-statistics BatchNorm2d (+ residual) (+ ReLU) of a channels-last activation; updates the running
    statistics in place.  Returns y (channels-last), mean, invstd."""
    rows, c, gamma, beta = _bn_args("bn_train_forward", x, residual, gamma, beta, running_mean, running_var)
    y = torch.empty_like(x)                        # (preserves channels-last)
    # mean | invstd are saved for backward, so they are an allocation of their own (2 C floats): carved out of the
    # workspace they would keep its ~4 KB x C alive until backward, per BatchNorm (~20 MB per ResNet-18 step)
    stat = torch.empty(2 * c, dtype=torch.float32, device=x.device)
    mean, invstd = stat[:c], stat[c:]
    ws = torch.empty(max(1, _bn_workspace_floats(rows, c)), dtype=torch.float32, device=x.device)
    _ck(lib().ipsx_bn_train_forward(_p(x), _p(residual), rows, c, _p(gamma), _p(beta), eps, momentum,
                                    _p(running_mean), _p(running_var), int(relu), _p(y), _p(mean), _p(invstd),
                                    _p(ws), _stream()), "ipsx_bn_train_forward")
    return y, mean, invstd


def maxpool_train_supported(x):
    """Can ``maxpool_3x3s2_nhwc`` / ``maxpool_3x3s2_bwd_nhwc`` take this activation (the training step's pooling behind the
    stem: float32 on the GPU, 16 x 16 maps, a multiple of 32 channels)?"""
    return bool(x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and os.environ.get("IPSX_TRAIN_POOL", "1") != "0"
                and lib().ipsx_maxpool_3x3s2_bwd_nhwc_supported(x.shape[1], x.shape[2], x.shape[3]))


def maxpool_3x3s2_nhwc(x):
    """nn.MaxPool2d(3, 2, 1) of a channels-last (P, C, h, w) activation -> channels-last (P, C, ho, wo)."""
    _one_gpu("maxpool_3x3s2_nhwc", x=x)
    x = _rd("maxpool_3x3s2_nhwc", "x", x, dim=4, cl=True)         # (float4 loads along the channels)
    n, c, h, w = x.shape
    y = torch.empty((n, c, (h - 1) // 2 + 1, (w - 1) // 2 + 1), dtype=torch.float32, device=x.device, memory_format=_CL)
    _ck(lib().ipsx_maxpool_3x3s2_nhwc(_p(x), _p(y), n, c, h, w, _stream()), "ipsx_maxpool_3x3s2_nhwc")
    return y


def maxpool_3x3s2_bwd_nhwc(x, dy):
    """The gradient of ``maxpool_3x3s2_nhwc`` w.r.t. x (ATen's rule: a window's gradient goes to its first maximum)."""
    _one_gpu("maxpool_3x3s2_bwd_nhwc", x=x, dy=dy)
    x = _rd("maxpool_3x3s2_bwd_nhwc", "x", x, dim=4, cl=True)
    n, c, h, w = x.shape
    if dy.dim() != 4 or tuple(dy.shape) != (n, c, (h - 1) // 2 + 1, (w - 1) // 2 + 1):
        raise ValueError("maxpool_3x3s2_bwd_nhwc: dy {} is not the pooled map of x {}".format(tuple(dy.shape), tuple(x.shape)))
    dy = _rd("maxpool_3x3s2_bwd_nhwc", "dy", dy, cl=True)
    dx = torch.empty_like(x)
    _ck(lib().ipsx_maxpool_3x3s2_bwd_nhwc(_p(x), _p(dy), _p(dx), n, c, h, w, _stream()), "ipsx_maxpool_3x3s2_bwd_nhwc")
    return dx


def bn_train_forward_partials(x, residual, gamma, beta, eps, momentum, running_mean, running_var, relu, partial, slabs, shift):
    """``bn_train_forward`` without its reduction pass: ``partial`` (slabs, 2, C) are the sums ``conv2d_nhwc(..., stats_shift=
    shift)`` took off its accumulators (``shift`` may be ``running_mean`` itself)."""
    rows, c, gamma, beta = _bn_args("bn_train_forward_partials", x, residual, gamma, beta, running_mean, running_var,
                                    partial=partial, shift=shift)
    # (partial: the producer's hand-over, shift: may BE running_mean - both taken where they lie)
    _wr("bn_train_forward_partials", "partial", partial, torch.float32, align=16)
    if partial.dim() != 3 or tuple(partial.shape[1:]) != (2, c) or not 0 <= slabs <= partial.shape[0]:
        raise ValueError("bn_train_forward_partials: partial must be (>= slabs = {}, 2, {}), got {}".format(slabs, c, tuple(partial.shape)))
    _wr("bn_train_forward_partials", "shift", shift, torch.float32, (c,))
    y = torch.empty_like(x)
    stat = torch.empty(2 * c, dtype=torch.float32, device=x.device)
    mean, invstd = stat[:c], stat[c:]
    _ck(lib().ipsx_bn_train_forward_partials(_p(x), _p(residual), rows, c, _p(gamma), _p(beta), eps, momentum,
                                             _p(running_mean), _p(running_var), int(relu), _p(y), _p(mean), _p(invstd),
                                             _p(partial), slabs, _p(shift), _stream()), "ipsx_bn_train_forward_partials")
    return y, mean, invstd


_BN_MAX_SLABS = 512      # csrc/bn_train.hip BN_MAX_SLABS (ipsx_bn_train_workspace_floats never exceeds 2 * 512 * C)
_BN_WS_FLOATS = {}


def _bn_workspace_floats(rows, c):
    """ipsx_bn_train_workspace_floats(rows, c), remembered per shape (a training step asks for the same few shapes)."""
    key = (rows, c)
    n = _BN_WS_FLOATS.get(key)
    if n is None:
        n = _BN_WS_FLOATS[key] = int(lib().ipsx_bn_train_workspace_floats(rows, c))
    return n


def bn_train_backward(dy, y, x, gamma, mean, invstd, relu, want_residual):
    """-> dx, dresidual | None, dgamma, dbeta."""
    _one_gpu("bn_train_backward", dy=dy, y=y, x=x, gamma=gamma, mean=mean, invstd=invstd)
    rows, c = _rows_cl(x)
    if _rows_cl(dy, "dy") != (rows, c) or dy.shape != x.shape:
        raise ValueError("bn_train_backward: dy {} beside x {}".format(tuple(dy.shape), tuple(x.shape)))
    if y is not None and (_rows_cl(y, "y") != (rows, c) or y.shape != x.shape):
        raise ValueError("bn_train_backward: y {} beside x {}".format(tuple(y.shape), tuple(x.shape)))
    gamma, mean, invstd = (_rd("bn_train_backward", name, t.detach(), dim=1) for name, t in
                           (("gamma", gamma), ("mean", mean), ("invstd", invstd)))
    if not gamma.shape[0] == mean.shape[0] == invstd.shape[0] == c:
        raise ValueError("bn_train_backward: gamma / mean / invstd must be ({},)".format(c))
    dx = torch.empty_like(x)
    dres = torch.empty_like(x) if want_residual else None
    dgamma = torch.empty(c, dtype=torch.float32, device=x.device)
    dbeta = torch.empty_like(dgamma)
    ws = torch.empty(max(1, _bn_workspace_floats(rows, c)), dtype=torch.float32, device=x.device)
    _ck(lib().ipsx_bn_train_backward(_p(dy), _p(y), _p(x), rows, c, _p(gamma), _p(mean), _p(invstd), int(relu),
                                     _p(dx), _p(dres), _p(dgamma), _p(dbeta), _p(ws), _stream()),
        "ipsx_bn_train_backward")
    return dx, dres, dgamma, dbeta


# ---------------------------------------------------------------- training step (with-grad feature projector)
def projector_train_supported(f, d):
    """Do ``projector_train_forward`` / ``projector_wgrad`` take a Linear(f, d) (F a multiple of 32; D a power of two
    32 .. 1024, which is also what the BatchNorm kernels behind it take)?"""
    return bool(lib().ipsx_projector_train_supported(f, d) and lib().ipsx_bn_train_supported(2, d))


def _feature_rows(x, f):
    if x.dim() != 2 or x.shape[1] != f or x.dtype not in _PATCH_DTYPES or not _gpu_device(x.device):
        raise ValueError("expected (rows, {}) float32 / bfloat16 / float16 feature rows on the GPU, got {} {}".format(
            f, tuple(x.shape), x.dtype))
    if x.shape[0] == 0:
        raise ValueError("no rows")
    return x if x.is_contiguous() else x.contiguous()


_PT_INDEX_SOURCE_BYTES = (1 << 31) - 65536        # what the indexed kernels address with 32-bit buffer offsets (include/ipsx.h)


def projector_train_index_supported(x):
    """Do ``projector_train_forward`` / ``projector_wgrad`` take ``x`` as the SOURCE of a row index - below 2 GiB?  (A larger
    source goes through a gathered copy and the plain calls.)"""
    return x.numel() * x.element_size() <= _PT_INDEX_SOURCE_BYTES


def _row_index(what, index, x):
    """The row index of the projector's indexed calls: int32, 1-D, at least one entry.  An index that lies on
    the HOST is a host-built one: its entries are checked here against ``x``'s rows, then it is copied to ``x``'s device.  An
    index on ``x``'s GPU is taken where it lies, its entries unread (the kernels clamp them); another device is refused."""
    if not torch.is_tensor(index) or index.dtype != torch.int32:
        raise TypeError("{}: index must be an int32 tensor, got {}".format(what, index.dtype if torch.is_tensor(index) else type(index)))
    if index.dim() != 1 or index.numel() == 0:
        raise ValueError("{}: index must be 1-d with at least one entry, got {}".format(what, tuple(index.shape)))
    if not projector_train_index_supported(x):
        raise ValueError("{}: a source of {} rows is not below 2 GiB - gather the rows and take the plain call".format(what, x.shape[0]))
    if index.device.type == "cpu":
        lo, hi = int(index.min()), int(index.max())
        if lo < 0 or hi >= x.shape[0]:
            raise ValueError("{}: index entries must lie in [0, {}), got {}".format(what, x.shape[0], lo if lo < 0 else hi))
        return index.to(x.device).contiguous()
    if index.device != x.device:
        raise ValueError("{}: index lies on {}, the rows on {}".format(what, index.device, x.device))
    return index if index.is_contiguous() else index.contiguous()


def projector_train_forward(x, weight, bias, ln_eps, index=None):
    """z = Linear(LayerNorm(x)) of (rows, F) feature rows (float32, or float16 / bfloat16 widened in the operand load) with
    the (D, F) ``weight`` and ``bias``, for the BatchNorm1d behind it in batch-statistics mode:
    -> (z, stats, partial, slabs, shift) - ``stats`` (rows, 2) the rows' (mean, rstd), all that backward needs of the
    LayerNorm; ``partial`` (slabs, 2, D) the column sums of z around ``shift`` for ``bn_train_forward_partials``.

    ``index`` (int32, 1-d; ``_row_index``): row j of every result is computed from row ``index[j]`` of ``x``, read where it
    lies - the bits of ``projector_train_forward(x[index], ...)`` without the copy (``ipsx_projector_stats_indexed``,
    ``ipsx_projector_train_forward_indexed``); rows of ``x`` outside the index are not read."""
    _one_gpu("projector_train_forward", x=x, weight=weight, bias=bias)
    if weight.dim() != 2 or bias.dim() != 1 or bias.shape[0] != weight.shape[0]:
        raise ValueError("projector_train_forward: weight (D, F) and bias (D,), got {} and {}".format(tuple(weight.shape), tuple(bias.shape)))
    d, f = weight.shape
    if not projector_train_supported(f, d):
        raise ValueError("the training projector takes F % 32 == 0 and D a power of two in 32 .. 1024, got F = {}, D = {}".format(f, d))
    x = _feature_rows(x, f)
    if index is not None:
        index = _row_index("projector_train_forward", index, x)
    n = x.shape[0] if index is None else index.numel()
    w = _f32(weight.detach())
    b = _f32(bias.detach())
    packed = _pack_conv(w.view(d, f, 1, 1))
    lin = Conv(f, d, 1, 1, 1, 0, _p(packed), None, _p(b), None, None)
    stats = torch.empty((n, 2), dtype=torch.float32, device=x.device)
    if index is None:
        _ck(lib().ipsx_projector_stats_typed(_p(x), _PATCH_DTYPES[x.dtype], n, f, C.c_float(ln_eps), _p(stats), _stream()),
            "ipsx_projector_stats_typed")
    else:
        _ck(lib().ipsx_projector_stats_indexed(_p(x), _PATCH_DTYPES[x.dtype], _p(index), x.shape[0], n, f, C.c_float(ln_eps), _p(stats),
                                               _stream()), "ipsx_projector_stats_indexed")
    slabs = int(lib().ipsx_projector_train_slabs(n))
    z = torch.empty((n, d), dtype=torch.float32, device=x.device)
    partial = torch.empty((slabs, 2, d), dtype=torch.float32, device=x.device)
    shift = torch.empty(d, dtype=torch.float32, device=x.device)
    if index is None:
        _ck(lib().ipsx_projector_train_forward(C.byref(lin), _p(w), _p(x), _PATCH_DTYPES[x.dtype], n, _p(stats), _p(z), _p(shift),
                                               _p(partial), _stream()), "ipsx_projector_train_forward")
    else:
        _ck(lib().ipsx_projector_train_forward_indexed(C.byref(lin), _p(w), _p(x), _PATCH_DTYPES[x.dtype], _p(index), x.shape[0], n,
                                                       _p(stats), _p(z), _p(shift), _p(partial), _stream()),
            "ipsx_projector_train_forward_indexed")
    return z, stats, partial, slabs, shift


def _projector_wgrad_slice_rows(f, d, dtype):
    """Rows of one ``ipsx_projector_wgrad`` call: what keeps either activation below 2 GiB, in whole chunks of the kernel's
    row split.  ``IPSX_TRAIN_PROJECTOR_SLICE_ROWS`` lowers it (tests: the slicing at a small size), to whole chunks as well."""
    chunk = int(lib().ipsx_projector_wgrad_chunk_rows())
    step = int(lib().ipsx_projector_wgrad_max_rows(f, d, _PATCH_DTYPES[dtype]))
    knob = os.environ.get("IPSX_TRAIN_PROJECTOR_SLICE_ROWS")
    if knob:
        step = min(step, max(chunk, int(knob) // chunk * chunk))
    return step


def projector_wgrad(x, dz, stats, index=None):
    """The gradient of ``projector_train_forward``'s z w.r.t. weight and bias -> (dw (D, F), db (D,)): dw = sum over the rows
    of (dz |rstd|)^T (x - mean), on the fp32 matrix cores from the raw rows.  Activations of 2 GiB and more go in slices of
    whole rows, each call adding its chunks onto the result in order: the bits of one call (csrc/projector_train.hip).

    ``index`` (as ``projector_train_forward`` takes it): ``dz`` and ``stats`` are packed - row j goes with row ``index[j]`` of
    ``x`` - and the result is the bits of ``projector_wgrad(x[index], dz, stats)`` (``ipsx_projector_wgrad_indexed``; a slice
    takes the matching slice of the index)."""
    _one_gpu("projector_wgrad", x=x, dz=dz, stats=stats)
    if dz.dim() != 2 or x.dim() != 2:
        raise ValueError("projector_wgrad: x (rows, F) and dz (rows, D), got {} and {}".format(tuple(x.shape), tuple(dz.shape)))
    n, d = dz.shape
    f = x.shape[1]
    x = _feature_rows(x, f)
    if index is not None:
        index = _row_index("projector_wgrad", index, x)
    rows = x.shape[0] if index is None else index.numel()
    if dz.dtype != torch.float32 or rows != n or tuple(stats.shape) != (n, 2) or stats.dtype != torch.float32:
        raise ValueError("dz: expected float32 ({}, D), statistics of the same rows".format(rows))
    stats = _rd("projector_wgrad", "stats", stats, align=8)          # ((mean, rstd) pairs: 8-byte loads)
    if not projector_train_supported(f, d):
        raise ValueError("the training projector takes F % 32 == 0 and D a power of two in 32 .. 1024, got F = {}, D = {}".format(f, d))
    dz = dz if dz.is_contiguous() else dz.contiguous()
    step = _projector_wgrad_slice_rows(f, d, x.dtype)
    dw = torch.empty((d, f), dtype=torch.float32, device=x.device)
    db = torch.empty(d, dtype=torch.float32, device=x.device)
    nb = int(lib().ipsx_projector_wgrad_workspace_bytes(min(n, step), f, d))
    ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
    for i0 in range(0, n, step):
        cnt = min(step, n - i0)
        if index is None:
            _ck(lib().ipsx_projector_wgrad(_p(x[i0:i0 + cnt]), _PATCH_DTYPES[x.dtype], _p(dz[i0:i0 + cnt]), _p(stats[i0:i0 + cnt]), cnt, f,
                                           d, _p(dw), _p(db), int(i0 > 0), _p(ws), nb, _stream()), "ipsx_projector_wgrad")
        else:
            _ck(lib().ipsx_projector_wgrad_indexed(_p(x), _PATCH_DTYPES[x.dtype], _p(index[i0:i0 + cnt]), x.shape[0], _p(dz[i0:i0 + cnt]),
                                                   _p(stats[i0:i0 + cnt]), cnt, f, d, _p(dw), _p(db), int(i0 > 0), _p(ws), nb, _stream()),
                "ipsx_projector_wgrad_indexed")
    return dw, db


# ---------------------------------------------------------------- training step (with-grad cross-attention aggregator)
def attn_pool_supported(R, D):
    """Do ``attn_pool_forward`` / ``attn_pool_backward`` take R = H * n_token folded query rows (1 .. 32) of D (a multiple of
    32 up to 1024)?"""
    return bool(lib().ipsx_attn_pool_supported(int(R), int(D)))


def _attn_pool_args(x, A, keep, count=None):
    """Checks (x (B, M, D), A (R, D), keep (B, R, M) | None, count | None) -> B, M, D, R, count (``slot_counts``: an int32
    (B,) tensor on x's device, or None)."""
    for name, t in (("x", x), ("A", A), ("keep", keep)):
        if t is None:
            continue
        if t.dtype != torch.float32 or not _gpu_device(t.device) or t.device != x.device:
            raise ValueError("{}: expected float32 on the call's GPU, got {} on {}".format(name, t.dtype, t.device))
        if not t.is_contiguous() or (name != "keep" and t.data_ptr() % 16):         # (keep: rows of M, read float by float)
            raise ValueError("{}: expected a contiguous tensor at a 16-byte address (the kernels' float4 loads)".format(name))
    if x.dim() != 3 or A.dim() != 2 or A.shape[1] != x.shape[2]:
        raise ValueError("expected x (B, M, D) and A (R, D), got {} and {}".format(tuple(x.shape), tuple(A.shape)))
    B, M, D = x.shape
    R = A.shape[0]
    if B < 1 or M < 1:
        raise ValueError("no rows")
    if not attn_pool_supported(R, D):
        raise ValueError("the attention pool takes R = H * n_token in 1 .. 32 and D a multiple of 32 up to 1024, got R = {}, D = {}".format(R, D))
    if keep is not None and tuple(keep.shape) != (B, R, M):
        raise ValueError("keep: expected {}, got {}".format((B, R, M), tuple(keep.shape)))
    if count is not None:
        count = slot_counts("attn_pool", count, B, M, x.device)
    return B, M, D, R, count


def _attn_pool_workspace(B, M, R, D, device):
    nb = int(lib().ipsx_attn_pool_workspace_bytes(B, M, R, D))
    if nb == 0:
        raise ValueError("the attention pool takes B <= 65535 and M <= 2^30, got B = {}, M = {}".format(B, M))
    return torch.empty(nb, dtype=torch.uint8, device=device), nb


def attn_pool_forward(x, A, keep=None, count=None):
    """Z[b, r] = sum_m P'[b, r, m] x[b, m] with P = softmax_m(x . A[r]), P' = P * keep, of float32 embeddings ``x`` (B, M, D),
    the folded query ``A`` (R, D) and attention-dropout factors ``keep`` (B, R, M) or None: -> (Z (B, R, D), P (B, R, M)).
    ``count`` (B ints or an integer tensor (B,); None = all M): image b's rows are its first count[b] ones - the softmax runs
    over them, P[b, :, count[b]:] is +0.0, the rows beyond are never read (ipsx_attn_pool_forward_counted).  Host counts are
    checked before any launch (ValueError); a tensor on the GPU is not read back, the kernels clamp its entries into 1 .. M."""
    B, M, D, R, count = _attn_pool_args(x, A, keep, count)
    Z = torch.empty((B, R, D), dtype=torch.float32, device=x.device)
    P = torch.empty((B, R, M), dtype=torch.float32, device=x.device)
    ws, nb = _attn_pool_workspace(B, M, R, D, x.device)
    if count is not None:
        _ck(lib().ipsx_attn_pool_forward_counted(_p(x), _p(A), _p(keep), _p(count), B, M, R, D, _p(Z), _p(P), _p(ws), nb, _stream()),
            "ipsx_attn_pool_forward_counted")
        return Z, P
    _ck(lib().ipsx_attn_pool_forward(_p(x), _p(A), _p(keep), B, M, R, D, _p(Z), _p(P), _p(ws), nb, _stream()), "ipsx_attn_pool_forward")
    return Z, P


def attn_pool_backward(x, A, keep, P, Z, dZ, want_dx=True, count=None):
    """The gradients of ``attn_pool_forward``'s Z: -> (dx (B, M, D) | None, dA (R, D)); ``P``, ``Z`` are what the forward
    returned for the same ``x``, ``A``, ``keep``, ``count``.  With ``count``, dx[b, count[b]:] is exactly zero."""
    B, M, D, R, count = _attn_pool_args(x, A, keep, count)
    for name, t, shape in (("P", P, (B, R, M)), ("Z", Z, (B, R, D)), ("dZ", dZ, (B, R, D))):
        if t.dtype != torch.float32 or not _gpu_device(t.device) or t.device != x.device or tuple(t.shape) != shape:
            raise ValueError("{}: expected float32 {} on the call's GPU, got {} {}".format(name, shape, t.dtype, tuple(t.shape)))
        if not t.is_contiguous() or (name != "P" and t.data_ptr() % 16):            # (P: rows of M, read float by float)
            raise ValueError("{}: expected a contiguous tensor at a 16-byte address".format(name))
    dx = torch.empty_like(x) if want_dx else None
    dA = torch.empty((R, D), dtype=torch.float32, device=x.device)
    ws, nb = _attn_pool_workspace(B, M, R, D, x.device)
    if count is not None:
        _ck(lib().ipsx_attn_pool_backward_counted(_p(x), _p(A), _p(keep), _p(count), _p(P), _p(Z), _p(dZ), B, M, R, D, _p(dx), _p(dA), _p(ws),
                                                  nb, _stream()), "ipsx_attn_pool_backward_counted")
        return dx, dA
    _ck(lib().ipsx_attn_pool_backward(_p(x), _p(A), _p(keep), _p(P), _p(Z), _p(dZ), B, M, R, D, _p(dx), _p(dA), _p(ws), nb, _stream()),
        "ipsx_attn_pool_backward")
    return dx, dA
