"""The two fp32 layer-by-layer convolution kernels over a lattice of geometries: conv_any_kernel (csrc/conv.hip, the public
NCHW entry point ipsx_conv2d_affine and its channels-last twin ipsx_conv2d_affine_to_nhwc) and conv_nhwc_kernel
(csrc/conv_nhwc.hip, ipsx_conv2d_affine_nhwc without row statistics, its three dispatches by C_out).

The cases are the commented lists CONV_LATTICE_NCHW / CONV_LATTICE_NHWC of tests/util.py (the oracle alone is held to the
same bound on them in tests/test_oracle_props.py, without a GPU): kernels that are not square, even kernels, stride 3,
pad 0 / (k-1)/2 / k-1 / k+1, maps narrower than the kernel, 31x31 taps, C_out one off every tile, output-pixel totals on
both sides of every tile edge in M, K loops as short as the operand ring, every branch of the epilogue.

Every case is held
  * to orc_conv2d_affine BIT FOR BIT, and a window that lies wholly in padding to exactly relu(shift + res);
  * to float64 F.conv2d within 1.01 (K + 3) 2^-24 (|alpha| conv(|x|, |w|) + |shift| + |res|) per element - the first-order
    bound of a K-term fp32 fma chain plus the two roundings of the epilogue, derived and not measured;
  * to its guards: x and the residual are views inside larger buffers of NaN, y is pre-filled with NaN between two
    sentinel rows - every output is written, nothing beside it, and no NaN is read into a sum;
  * to independence of the batch: the first and the last image alone give the bits they have inside the full call.

Worst |got - float64| / bound, measured on one MI355X: conv_any_kernel 0.463 (both layouts), conv_nhwc_kernel 0.115 - the
oracle's own figures, as the bits are the oracle's."""

import ctypes as C

import numpy as np
import pytest
import torch

from ips_amd import hip
from ips_amd.hip_encoder import _pack_conv
from tests.util import (CONV_LATTICE_NCHW, CONV_LATTICE_NHWC, conv_bound_ratio, conv_case_f64, conv_case_id, conv_case_inputs,
                        conv_case_oracle, conv_case_out, conv_padding_only_value, ulp_diff)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64              # floats in front of and behind every guarded view (256 bytes: the views stay 16-byte aligned)
SENTINEL = -12345.5


def guarded(a):
    """a copy of the array on the device, as a view inside a buffer whose other elements are NaN"""
    buf = torch.full((a.size + 2 * GUARD,), float("nan"), device=DEV)
    view = buf[GUARD:GUARD + a.size].view(a.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return view


def guarded_out(shape):
    """(buffer, view): a NaN-filled output between two sentinel rows"""
    size = int(np.prod(shape))
    buf = torch.full((size + 2 * GUARD,), SENTINEL, device=DEV)
    view = buf[GUARD:GUARD + size].view(shape)
    view.fill_(float("nan"))
    return buf, view


def read_out(buf, view, what):
    b = buf.cpu().numpy()
    assert np.all(b[:GUARD] == SENTINEL) and np.all(b[-GUARD:] == SENTINEL), what + ": wrote outside y"
    got = view.cpu().numpy()
    assert not np.isnan(got).any(), what + ": outputs left unwritten, or NaN read from outside x / res"
    return got


def nhwc(a):
    return None if a is None else np.ascontiguousarray(a.transpose(0, 2, 3, 1))


class Device:
    """a case's operator on the device: packed weights, affine, the three entry points"""

    def __init__(self, c, wt, alpha, shift):
        self.c = c
        self.keep = [_pack_conv(torch.from_numpy(wt).to(DEV)), None if alpha is None else torch.from_numpy(alpha).to(DEV),
                     None if shift is None else torch.from_numpy(shift).to(DEV)]
        self.cv = hip.Conv(c.c_in, c.c_out, c.kh, c.kw, c.stride, c.pad, self.keep[0].data_ptr(),
                           None if alpha is None else self.keep[1].data_ptr(), None if shift is None else self.keep[2].data_ptr())

    def run(self, entry, x, r, out_shape):
        """x / r: numpy in the entry's layout; returns the output as numpy, guards checked"""
        c = self.c
        xd, rd = guarded(x), (None if r is None else guarded(r))
        buf, y = guarded_out(out_shape)
        hip._ck(getattr(hip.lib(), entry)(C.byref(self.cv), hip._p(xd), hip._p(rd), hip._p(y), x.shape[0], c.h, c.w,
                                          int(c.relu), hip._stream()), entry)
        return read_out(buf, y, entry)


def check_against_the_references(c, got, x, wt, alpha, shift, r, what):
    want = conv_case_oracle(c, x, wt, alpha, shift, r)
    e, bound, A = conv_case_f64(c, x, wt, alpha, shift, r)
    ratio = conv_bound_ratio(got, e, bound)
    print("\n  %s %s: worst |got - float64| / bound %.3f" % (what, conv_case_id(c), ratio))
    assert ulp_diff(got, want) == 0, "max abs diff to the oracle %g" % np.abs(got - want).max()
    assert ratio <= 1.0, ratio
    pad_only, v = conv_padding_only_value(c, shift, r, A)
    assert np.array_equal(got[pad_only], v[pad_only]), "a window wholly in padding is not exactly shift + res"


def ends(n):
    """the images that run alone: the first and the last"""
    return [0] if n == 1 else [0, n - 1]


@pytest.mark.parametrize("i,c", list(enumerate(CONV_LATTICE_NCHW)), ids=[conv_case_id(c) for c in CONV_LATTICE_NCHW])
def test_nchw_lattice(i, c):
    x, wt, alpha, shift, r = conv_case_inputs(c, 100 + i)
    ho, wo = conv_case_out(c)
    op = Device(c, wt, alpha, shift)
    got = op.run("ipsx_conv2d_affine", x, r, (c.n, c.c_out, ho, wo))
    check_against_the_references(c, got, x, wt, alpha, shift, r, "nchw")
    # the channels-last output of the same kernel (its residual is channels-last too): the same bits, permuted
    last = op.run("ipsx_conv2d_affine_to_nhwc", x, nhwc(r), (c.n, ho, wo, c.c_out))
    assert np.array_equal(last.view(np.int32), nhwc(got).view(np.int32)), "to_nhwc differs from the NCHW output permuted"
    for k in ends(c.n):
        rk = None if r is None else r[k:k + 1]
        one = op.run("ipsx_conv2d_affine", x[k:k + 1], rk, (1, c.c_out, ho, wo))
        assert np.array_equal(one.view(np.int32), got[k:k + 1].view(np.int32)), "image %d alone differs" % k
        one = op.run("ipsx_conv2d_affine_to_nhwc", x[k:k + 1], nhwc(rk), (1, ho, wo, c.c_out))
        assert np.array_equal(one.view(np.int32), nhwc(got[k:k + 1]).view(np.int32)), "image %d alone differs (to_nhwc)" % k


@pytest.mark.parametrize("i,c", list(enumerate(CONV_LATTICE_NHWC)), ids=[conv_case_id(c) for c in CONV_LATTICE_NHWC])
def test_nhwc_lattice(i, c):
    x, wt, alpha, shift, r = conv_case_inputs(c, 200 + i)
    ho, wo = conv_case_out(c)
    op = Device(c, wt, alpha, shift)
    got = op.run("ipsx_conv2d_affine_nhwc", nhwc(x), nhwc(r), (c.n, ho, wo, c.c_out)).transpose(0, 3, 1, 2)
    check_against_the_references(c, got, x, wt, alpha, shift, r, "nhwc")
    for k in ends(c.n):
        rk = None if r is None else r[k:k + 1]
        one = op.run("ipsx_conv2d_affine_nhwc", nhwc(x[k:k + 1]), nhwc(rk), (1, ho, wo, c.c_out)).transpose(0, 3, 1, 2)
        assert np.array_equal(np.ascontiguousarray(one).view(np.int32), np.ascontiguousarray(got[k:k + 1]).view(np.int32)), \
            "image %d alone differs" % k


# ---------------------------------------------------------------------------------------------- refusals (nothing is launched)
def _conv(c_in, c_out, kh, kw, stride, pad):
    """an operator whose pointers are real but never read"""
    keep = torch.zeros(hip.lib().ipsx_packed_conv_weight_elems(c_out, c_in, kh, kw), device=DEV)
    return hip.Conv(c_in, c_out, kh, kw, stride, pad, keep.data_ptr(), None, None), keep


def _refused(entry, cv, n, h, w, words=64):
    x, y = torch.zeros(4096, device=DEV), torch.full((words,), float("nan"), device=DEV)
    rc = getattr(hip.lib(), entry)(C.byref(cv), hip._p(x), None, hip._p(y), n, h, w, 0, hip._stream())
    torch.cuda.synchronize()
    assert torch.isnan(y).all(), "a refused call wrote to y"
    return rc, hip.lib().ipsx_last_error().decode()


FP32_ENTRIES = ["ipsx_conv2d_affine", "ipsx_conv2d_affine_to_nhwc", "ipsx_conv2d_affine_nhwc"]


def test_nhwc_refuses_c_in_that_is_no_multiple_of_32():
    cv, _keep = _conv(48, 64, 3, 3, 1, 1)
    rc, msg = _refused("ipsx_conv2d_affine_nhwc", cv, 1, 5, 5)
    assert rc != 0 and "multiple of 32" in msg and "48" in msg, msg
    with pytest.raises(RuntimeError, match="multiple of 32"):
        hip._ck(rc, "conv")


def test_nchw_refuses_kernels_and_k_tables_it_cannot_hold():
    for entry in FP32_ENTRIES[:2]:
        cv, _keep = _conv(1, 8, 32, 32, 1, 0)                      # 32 rows: one more than the tap masks have bits
        rc, msg = _refused(entry, cv, 1, 32, 32)
        assert rc != 0 and "larger than 31x31" in msg, msg
        cv, _keep = _conv(1, 8, 3, 32, 1, 16)
        rc, msg = _refused(entry, cv, 1, 5, 5)
        assert rc != 0 and "larger than 31x31" in msg, msg
        cv, _keep = _conv(9, 8, 31, 31, 1, 15)                     # K = 8649: a table of 67.6 KiB
        rc, msg = _refused(entry, cv, 1, 4, 4)
        assert rc != 0 and "does not fit the k table" in msg, msg
        cv, _keep = _conv(8200, 8, 1, 1, 1, 0)                     # ... and from the channels alone
        rc, msg = _refused(entry, cv, 1, 1, 1)
        assert rc != 0 and "does not fit the k table" in msg, msg


@pytest.mark.parametrize("entry", FP32_ENTRIES)
@pytest.mark.parametrize("k,stride,pad,h,w", [
    (3, 1, 0, 2, 5),        # two rows under three
    (3, 1, 0, 5, 2),        # two columns under three
    (3, 2, 0, 2, 2),        # under stride 2, where (2 - 3) / 2 rounds towards zero: the gate took this for ONE output
    (5, 3, 1, 2, 9),        # the padded map (4 rows) still under the kernel, stride 3
    (7, 2, 2, 2, 2),        # 6 padded rows under 7, stride 2
])
def test_a_map_smaller_than_the_kernel_is_an_empty_output(entry, k, stride, pad, h, w):
    cv, _keep = _conv(32, 32, k, k, stride, pad)
    rc, msg = _refused(entry, cv, 2, h, w)
    assert rc != 0 and "empty output" in msg, msg


@pytest.mark.parametrize("entry", FP32_ENTRIES)
def test_no_images_is_ok_and_writes_nothing(entry):
    cv, _keep = _conv(32, 32, 3, 3, 1, 1)
    rc, _ = _refused(entry, cv, 0, 5, 5)
    assert rc == 0
