"""conv_nhwc_bf16_kernel (csrc/conv_nhwc_bf16.hip, through hip.conv2d_nhwc_bf16) over a lattice of geometries, against the
float64 emulation of tests/util.py (bf16_conv_emulation: the one tests/test_trunk_layered_bf16.py holds the layer shapes
of the shipped trunks to) under that test's bounds, unchanged: with e the emulation before its last rounding and
s = max |e|, every element within 2^-8 |e| + 1e-5 s, and at most max(2, 1e-3 numel) elements different from bf16(e).

The cases are the commented list below: its four dispatches by C_out (<= 64, 65 .. 255, 256 .. 511, >= 512) each with a
whole, a partial and a one-over n-tile, k-step totals below and at the depth of the operand ring (1x1 with C_in = 16, 32,
48: 1, 2, 3 k-steps; the ring is 4 deep at C_out <= 64, 3 above), output-pixel totals on both sides of every workgroup
edge in M, kernels that are not square, even kernels, stride 3, pad 0 / (k-1)/2 / k-1 / k+1, maps narrower than the
kernel, every branch of the epilogue.  x and the residual are views inside larger buffers of NaN, y is pre-filled with
NaN between two sentinel rows, every view at a 16-byte address as the ABI demands; the first and the last image alone
give the bits they have inside the full call.

The cap on the flips is a condition on the inputs, so the seeds are fixed and test_seeds_respect_the_flip_cap_on_the_cpu
(no GPU) holds an fp32-accumulating CPU evaluation of every case - ATen's float32 convolution on the bf16-rounded
operands, the float32 epilogue, one rounding - to the same cap; a seed that does not stay within it is replaced in SEEDS.
That test carries no gpu mark, which is why this file marks its GPU tests one by one.

Measured on one MI355X: 35 of the 42 cases have no element != bf16(e); worst share per dispatch 0 (C_out <= 64), 4.1e-5
(65 .. 255), 7.9e-5 (256 .. 511), 1.08e-4 (>= 512: 8 of 74,304 elements, cap 74); worst |got - e| / bound 0.989 (an element
half a bf16 step from e, as rounding allows).  The CPU evaluation: 0 .. 7 elements per case, at most 1.0e-4 of them."""

import ctypes as C

import pytest
import torch

from ips_amd import hip
from tests.util import ConvCase, bf16_conv_emulation, conv_case_id, conv_case_out, r16

gpu = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64              # bf16 elements in front of and behind every guarded view (128 bytes: 16-byte aligned views)
SENTINEL = -12288.0     # (exact in bf16)
FLIP_CAP = 1e-3
_T, _F = True, False

CONV_LATTICE_BF16 = [ConvCase(*c) for c in [
    # c_in, c_out, kh, kw, stride, pad, h, w, n, residual, relu, affine ("as" alpha and shift, "a", "s", "-" neither)
    # -- k-step totals against the ring: the primed look-ahead re-requests the last k-step and nobody consumes it
    (16, 8, 1, 1, 1, 0, 1, 1, 1, _F, _F, "as"),      # 1 k-step under a ring of 4; 1 pixel, 8 channels: ONE 16-byte store
    (32, 24, 1, 1, 1, 0, 3, 3, 7, _T, _T, "as"),     # 2 k-steps; 63 pixels; C_out = 24: three chunks of the first n-tile
    (48, 64, 1, 1, 1, 0, 2, 2, 16, _F, _T, "s"),     # 3 k-steps; 64 pixels; two whole n-tiles
    (16, 72, 1, 1, 1, 0, 5, 5, 3, _T, _T, "as"),     # 1 k-step under a ring of 3; C_out = 72: one chunk in the second piece
    (32, 256, 1, 1, 1, 0, 1, 1, 127, _F, _T, "a"),   # 2 k-steps under a ring of 3; 127 pixels (workgroup of 128 x 256)
    (48, 512, 1, 1, 1, 0, 1, 1, 63, _T, _F, "as"),   # 3 k-steps = the ring of 3; 63 pixels (workgroup of 64 x 512)
    (16, 520, 1, 1, 2, 0, 3, 3, 5, _F, _F, "-"),     # 1 k-step in the widest dispatch, C_out = 512 + 8; strided 1x1; bare chain
    # -- workgroup edges in M: 255 / 256 / 257 (C_out <= 64 and 65 .. 255), 127 / 128 / 129 (256 .. 511), 63 / 64 / 65 (>= 512)
    (16, 64, 1, 1, 1, 0, 1, 1, 255, _F, _T, "as"),
    (32, 8, 2, 2, 1, 0, 2, 2, 256, _T, _F, "a"),     # 2x2 kernel on 2x2 maps -> 1x1: even kernel, 8 k-steps
    (16, 24, 1, 1, 1, 0, 1, 1, 257, _F, _F, "s"),
    (32, 128, 1, 1, 1, 0, 1, 1, 255, _T, _T, "as"),
    (16, 136, 3, 3, 2, 1, 3, 3, 64, _F, _T, "as"),   # 256 = 64 x (2x2 outputs); C_out = 128 + 8: a second column with one chunk
    (16, 248, 1, 1, 1, 0, 1, 1, 257, _F, _F, "s"),   # C_out = 256 - 8
    (32, 264, 1, 1, 1, 0, 2, 2, 32, _T, _T, "as"),   # 128; C_out = 256 + 8: the second column has one live wave
    (16, 504, 1, 1, 1, 0, 1, 1, 129, _F, _T, "as"),  # C_out = 512 - 8
    (16, 1032, 3, 3, 1, 0, 3, 3, 64, _T, _T, "as"),  # 64; pad 0 under k = 3: 1x1 outputs; C_out = 2 x 512 + 8: three columns
    (32, 520, 1, 1, 1, 0, 1, 1, 65, _T, _F, "a"),
    # -- kernels that are not square, even kernels, stride 3, pad in {0, (k-1)/2, k-1, k+1}, narrow maps
    (16, 128, 1, 3, 1, 1, 4, 5, 2, _F, _T, "as"),    # 1x3 / pad 1 (= kh): 6x5 outputs, the first and last rows are padding
    (32, 64, 3, 1, 2, 1, 7, 4, 3, _T, _T, "as"),     # 3x1 / stride 2 / pad 1: 4x3 outputs
    (16, 136, 5, 3, 1, 2, 6, 5, 2, _T, _F, "s"),     # 5x3, pad (kh-1)/2 = kw-1: 6x7 outputs, residual without ReLU
    (48, 24, 5, 3, 2, 4, 6, 5, 2, _F, _T, "as"),     # 5x3 / stride 2, pad kh-1 = kw+1: corner windows wholly in padding
    (16, 256, 7, 7, 2, 3, 13, 11, 1, _F, _T, "as"),  # 7x7 / stride 2 on an odd map: 7x6 outputs
    (16, 72, 7, 7, 3, 6, 9, 9, 2, _T, _T, "a"),      # 7x7 / stride 3 / pad k-1: 5x5 outputs
    (32, 248, 2, 2, 2, 1, 7, 7, 3, _F, _F, "as"),    # 2x2 / stride 2 / pad k-1: 4x4 outputs
    (80, 8, 2, 2, 1, 3, 3, 3, 2, _T, _T, "as"),      # 2x2, pad k+1: 8x8 outputs, the outer rings are shift + res; C_in = 80
    (48, 504, 3, 3, 1, 4, 2, 2, 1, _T, _T, "as"),    # 3x3, pad k+1 round a 2x2 map: 8x8 outputs, 4 of 64 windows see data
    (16, 128, 3, 3, 1, 2, 5, 5, 1, _F, _F, "-"),     # pad k-1: a corner output sees one pixel; no epilogue at all
    (80, 64, 3, 3, 3, 1, 11, 13, 2, _F, _T, "s"),    # 3x3 / stride 3: 4x5 outputs
    (32, 264, 3, 3, 2, 0, 9, 9, 3, _T, _T, "as"),    # pad 0 under stride 2: 4x4 outputs
    (16, 1032, 1, 1, 3, 0, 7, 7, 2, _F, _T, "as"),   # 1x1 / stride 3: 3x3 outputs
    (16, 24, 1, 1, 1, 2, 3, 3, 4, _F, _F, "as"),     # 1x1 kernel with pad k+1 = 2: 7x7 outputs of which 9 see data
    (80, 72, 3, 3, 1, 1, 1, 1, 33, _T, _T, "as"),    # 1x1 maps under 3x3 / pad 1: only the centre tap is real
    (16, 512, 3, 3, 1, 1, 2, 9, 2, _F, _T, "s"),     # 2 rows under a 3x3 kernel
    (48, 136, 5, 3, 1, 1, 3, 13, 2, _T, _F, "as"),   # 3 rows under a 5-row kernel, pad 1: ONE output row of 13
    (16, 8, 31, 1, 2, 15, 5, 3, 2, _F, _T, "as"),    # 31x1 / stride 2: 3x17 outputs, most of them padding columns
    # -- C_in = 128 and long chains
    (128, 64, 3, 3, 1, 1, 5, 7, 2, _T, _T, "as"),    # 72 k-steps, 8 per tap
    (128, 520, 3, 3, 1, 1, 4, 4, 5, _T, _T, "as"),   # the long chain in the widest dispatch: 80 pixels, a ragged second row tile
    (80, 248, 3, 3, 2, 1, 13, 13, 2, _T, _F, "as"),  # 45 k-steps, 5 per tap; 98 pixels
    (128, 504, 1, 1, 1, 0, 13, 13, 1, _F, _T, "a"),  # 8 k-steps, 169 pixels: two workgroups of 128
    (80, 1032, 3, 3, 1, 1, 3, 3, 8, _F, _T, "s"),    # 72 pixels: two row tiles, the second of 8
    (128, 256, 3, 3, 1, 1, 13, 13, 1, _T, _T, "as"),  # 169 pixels: a whole and a ragged workgroup of 128, shortcut + ReLU
    (48, 128, 3, 3, 1, 1, 13, 13, 2, _F, _T, "as"),  # 338 pixels: two workgroups of 256
]]
IDS = [conv_case_id(c) for c in CONV_LATTICE_BF16]
# seed of every case; one that the CPU evaluation finds above the cap is replaced here
SEEDS = {i: 3000 + i for i in range(len(CONV_LATTICE_BF16))}


def case_inputs(c, seed):
    """the stored tensors of a case on the CPU: x (n, h, w, C_in) bf16, OIHW float32 weights, alpha / shift float32 or
    None, residual (n, ho, wo, C_out) bf16 or None"""
    g = torch.Generator().manual_seed(seed)
    ho, wo = conv_case_out(c)
    x = torch.relu(torch.randn(c.n, c.h, c.w, c.c_in, generator=g)).to(torch.bfloat16)
    wt = torch.randn(c.c_out, c.c_in, c.kh, c.kw, generator=g) * (2.0 / (c.c_in * c.kh * c.kw)) ** 0.5
    alpha, shift = 1 + 0.2 * torch.randn(c.c_out, generator=g), 0.1 * torch.randn(c.c_out, generator=g)
    r = torch.relu(torch.randn(c.n, ho, wo, c.c_out, generator=g)).to(torch.bfloat16)
    return x, wt, (alpha if "a" in c.affine else None), (shift if "s" in c.affine else None), (r if c.res else None)


def flip_cap(e):
    return max(2, int(FLIP_CAP * e.numel()))


@pytest.mark.parametrize("i,c", list(enumerate(CONV_LATTICE_BF16)), ids=IDS)
def test_seeds_respect_the_flip_cap_on_the_cpu(i, c):
    x, wt, alpha, shift, r = case_inputs(c, SEEDS[i])
    e = bf16_conv_emulation(x, wt, alpha, shift, c.stride, c.pad, r, c.relu)
    e32 = bf16_conv_emulation(x, wt, alpha, shift, c.stride, c.pad, r, c.relu, acc=torch.float32)
    assert tuple(e.shape) == (c.n,) + conv_case_out(c) + (c.c_out,) and torch.isfinite(e).all()
    flips = int((r16(e32) != r16(e)).sum())
    print("\n  %s: %d of %d elements of the fp32-accumulating CPU evaluation != bf16(emulation), cap %d"
          % (IDS[i], flips, e.numel(), flip_cap(e)))
    assert flips <= flip_cap(e), (flips, flip_cap(e))


def test_bf16_lattice_reaches_the_seams_it_is_there_for():
    cases = CONV_LATTICE_BF16

    def totals(pick):
        return {c.n * conv_case_out(c)[0] * conv_case_out(c)[1] for c in cases if pick(c)}

    assert {c.c_in for c in cases} >= {16, 32, 48, 80, 128}
    assert {c.c_out for c in cases} >= {8, 24, 64, 72, 128, 136, 248, 256, 264, 504, 512, 520, 1032}
    assert {(c.kh, c.kw) for c in cases} >= {(1, 1), (2, 2), (3, 3), (1, 3), (3, 1), (5, 3), (7, 7)}
    assert {c.stride for c in cases} >= {1, 2, 3} and {c.affine for c in cases} == {"as", "a", "s", "-"}
    assert {(c.res, c.relu) for c in cases} == {(False, False), (False, True), (True, False), (True, True)}
    for k in (2, 3):
        assert {c.pad for c in cases if c.kh == c.kw == k} >= {0, (k - 1) // 2, k - 1, k + 1}, k
    assert any(c.h < c.kh or c.w < c.kw for c in cases)
    for lo, hi in ((1, 64), (65, 255), (256, 511), (512, 1 << 20)):        # k-step totals 1, 2, 3 under both ring depths
        assert {c.kh * c.kw * c.c_in // 16 for c in cases if lo <= c.c_out <= hi} & {1, 2, 3}, lo
    assert {c.kh * c.kw * c.c_in // 16 for c in cases if c.c_out <= 64} >= {1, 2, 3}
    assert {c.kh * c.kw * c.c_in // 16 for c in cases if c.c_out > 64} >= {1, 2, 3, 72}
    assert totals(lambda c: c.c_out <= 64) >= {255, 256, 257} and totals(lambda c: 64 < c.c_out < 256) >= {255, 256, 257}
    assert totals(lambda c: 256 <= c.c_out < 512) >= {127, 128, 129} and totals(lambda c: c.c_out >= 512) >= {63, 64, 65}


# ---------------------------------------------------------------------------------------------- the kernel
def guarded(t):
    """a copy of the bf16 tensor on the device, as a contiguous view inside a buffer whose other elements are NaN"""
    buf = torch.full((t.numel() + 2 * GUARD,), float("nan"), dtype=torch.bfloat16, device=DEV)
    view = buf[GUARD:GUARD + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 0
    return view


def run(c, x, wt, alpha, shift, r):
    """the kernel on guarded operands: the output on the CPU as float64, its guards checked"""
    ho, wo = conv_case_out(c)
    shape = (x.shape[0], ho, wo, c.c_out)
    size = shape[0] * ho * wo * c.c_out
    buf = torch.full((size + 2 * GUARD,), SENTINEL, dtype=torch.bfloat16, device=DEV)
    y = buf[GUARD:GUARD + size].view(shape)
    y.fill_(float("nan"))
    assert y.data_ptr() % 16 == 0
    dev = [None if t is None else t.to(DEV) for t in (wt, alpha, shift)]
    got = hip.conv2d_nhwc_bf16(guarded(x), dev[0], dev[1], dev[2], c.stride, c.pad, None if r is None else guarded(r), c.relu, out=y)
    assert got.data_ptr() == y.data_ptr() and got.dtype == torch.bfloat16 and tuple(got.shape) == shape
    b = buf.cpu().float()
    assert bool((b[:GUARD] == SENTINEL).all()) and bool((b[-GUARD:] == SENTINEL).all()), "wrote outside y"
    got = got.cpu().double()
    assert not torch.isnan(got).any(), "outputs left unwritten, or NaN read from outside x / res"
    assert torch.isfinite(got).all()
    return got


@gpu
@pytest.mark.parametrize("i,c", list(enumerate(CONV_LATTICE_BF16)), ids=IDS)
def test_bf16_lattice(i, c):
    x, wt, alpha, shift, r = case_inputs(c, SEEDS[i])
    got = run(c, x, wt, alpha, shift, r)
    e = bf16_conv_emulation(x, wt, alpha, shift, c.stride, c.pad, r, c.relu)
    s = float(e.abs().max())
    bound = 2.0 ** -8 * e.abs() + 1e-5 * s
    excess = float(((got - e).abs() - bound).max())
    ratio = float(((got - e).abs() / bound.clamp_min(1e-300)).max())
    flips = int((got != r16(e)).sum())
    print("\n  %s: %d of %d elements != bf16(emulation) (share %.2e, cap %d), worst |got - e| / bound %.3f"
          % (IDS[i], flips, e.numel(), flips / float(e.numel()), flip_cap(e), ratio))
    assert excess <= 0.0, excess
    assert flips <= flip_cap(e), (flips, flip_cap(e))
    for k in ([0] if c.n == 1 else [0, c.n - 1]):       # the first and the last image alone: the bits of the full call
        one = run(c, x[k:k + 1], wt, alpha, shift, None if r is None else r[k:k + 1])
        assert torch.equal(one, got[k:k + 1]), "image %d alone differs" % k


# ---------------------------------------------------------------------------------------------- refusals (nothing is launched)
def _abi(c_in, c_out, k, stride, pad, n, h, w, x_offset=0):
    """the C entry point on an operator whose pointers are real but never read: (status, message, y untouched)"""
    lib = hip.lib()
    half = torch.zeros(max(16, lib.ipsx_packed_conv_weight_bf16_bytes(c_out, c_in, k, k)), dtype=torch.uint8, device=DEV)
    cv = hip.Conv(c_in, c_out, k, k, stride, pad, None, None, None, half.data_ptr())
    x = torch.zeros(4096, dtype=torch.bfloat16, device=DEV)[x_offset:]
    y = torch.full((256,), float("nan"), dtype=torch.bfloat16, device=DEV)
    rc = lib.ipsx_conv2d_affine_nhwc_bf16(C.byref(cv), hip._p(x), None, hip._p(y), n, h, w, 0, hip._stream())
    torch.cuda.synchronize()
    assert torch.isnan(y).all(), "a refused call wrote to y"
    return rc, lib.ipsx_last_error().decode(), lib.ipsx_conv2d_affine_nhwc_bf16_supported(C.byref(cv))


@gpu
def test_refusals_of_the_bf16_convolution():
    rc, msg, ok = _abi(24, 64, 3, 1, 1, 1, 5, 5)
    assert rc != 0 and "C_in = 24 is not a multiple of 16" in msg and ok == 0, msg
    rc, msg, ok = _abi(16, 12, 3, 1, 1, 1, 5, 5)
    assert rc != 0 and "16 -> 12, 3x3 / 1 pad 1 is not supported (C_in % 16 == 0, C_out % 8 == 0)" in msg and ok == 0, msg
    rc, msg, ok = _abi(16, 8, 3, 1, 1, 1, 5, 5, x_offset=1)        # (the operator itself is one the kernel takes)
    assert rc != 0 and "activations must start at 16-byte addresses" in msg and ok == 1, msg
    # the same through the Python entry point
    z = torch.zeros
    with pytest.raises(ValueError, match="needs C_in % 16 == 0 and C_out % 8 == 0, got 24 -> 64"):
        hip.conv2d_nhwc_bf16(z(1, 5, 5, 24, dtype=torch.bfloat16, device=DEV), z(64, 24, 3, 3, device=DEV), None, None, 1, 1)
    with pytest.raises(ValueError, match="needs C_in % 16 == 0 and C_out % 8 == 0, got 16 -> 12"):
        hip.conv2d_nhwc_bf16(z(1, 5, 5, 16, dtype=torch.bfloat16, device=DEV), z(12, 16, 3, 3, device=DEV), None, None, 1, 1)
    off = z(1 + 5 * 5 * 16, dtype=torch.bfloat16, device=DEV)[1:].view(1, 5, 5, 16)
    with pytest.raises(RuntimeError, match="activations must start at 16-byte addresses"):
        hip.conv2d_nhwc_bf16(off, z(8, 16, 3, 3, device=DEV), None, None, 1, 1)
    with pytest.raises(ValueError, match="out must be"):
        hip.conv2d_nhwc_bf16(z(1, 5, 5, 16, dtype=torch.bfloat16, device=DEV), z(8, 16, 3, 3, device=DEV), None, None, 1, 1,
                             out=z(1, 5, 5, 16, dtype=torch.bfloat16, device=DEV))


@gpu
@pytest.mark.parametrize("k,stride,pad,h,w", [
    (3, 1, 0, 2, 5),        # two rows under three
    (3, 1, 0, 5, 2),        # two columns under three
    (3, 2, 0, 2, 2),        # under stride 2, where (2 - 3) / 2 rounds towards zero: the gate took this for ONE output
    (5, 3, 1, 2, 9),        # the padded map (4 rows) still under the kernel, stride 3
    (7, 2, 2, 2, 2),        # 6 padded rows under 7, stride 2
])
def test_a_map_smaller_than_the_kernel_is_an_empty_output(k, stride, pad, h, w):
    rc, msg, ok = _abi(16, 8, k, stride, pad, 2, h, w)
    assert rc != 0 and "empty output" in msg and ok == 1, msg


@gpu
def test_no_images_is_ok_and_writes_nothing():
    rc, _, ok = _abi(16, 8, 3, 1, 1, 0, 5, 5)
    assert rc == 0 and ok == 1
