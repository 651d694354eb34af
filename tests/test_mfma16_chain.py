"""v_mfma_f32_16x16x4_f32 accumulates its four k slots as ONE fma chain in slot order: the 4x4 stage of
fused_trunk_kernel rests on it (csrc/fused_trunk.hip: conv_t16).  ipsx_dbg_mfma16_chain computes one 16 x 16 tile with K = 8 as
two of those instructions, slots (k0, k4, k1, k5) then (k2, k6, k3, k7), and - form 1 - the same product the way every other
convolution here does: four v_mfma_f32_32x32x2_f32, lane half h holding k = 4 h + j at step j.  The two must agree BITWISE on
operands whose rounding depends on the order of the chain."""

import ctypes as C

import numpy as np
import pytest
import torch

from ips_amd import hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CONTRACT = (0, 4, 1, 5, 2, 6, 3, 7)


def operands(seed):
    """A (16, 8), B (8, 16): magnitudes 2^-20 .. 2^20 with full mantissas, cancelling pairs, a zero row, a row of -0."""
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal((16, 8)) * np.exp2(rng.integers(-20, 21, (16, 8)))).astype(np.float32)
    b = (rng.standard_normal((8, 16)) * np.exp2(rng.integers(-20, 21, (8, 16)))).astype(np.float32)
    # cancelling pairs: k and k + 4 (neighbours in the chain), and k = 1, 2 (two instructions apart on the 16x16x4 form)
    a[2, 4:] = -a[2, :4]
    b[4:, 3] = b[:4, 3]
    a[5, 2] = a[5, 1]
    b[2, :] = np.where(np.arange(16) % 2 == 0, -b[1, :], b[2, :])
    # a large term early, absorbed or not by what follows
    a[7, 0] = np.float32(2.0 ** 24 + 2.0)
    b[0, 7] = np.float32(1.0)
    a[9, :] = 0.0
    a[11, :] = -0.0
    return a, b


def chain(a, b, order):
    """The fma chain from +0 in the given k order, each step rounded to float32 (products are exact in float64)."""
    acc = np.zeros((16, 16), dtype=np.float32)
    for k in order:
        acc = (a[:, k:k + 1].astype(np.float64) * b[k:k + 1, :].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    return acc


def run(a, b, form):
    fn = hip.lib().ipsx_dbg_mfma16_chain
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    ad, bd = torch.from_numpy(a).to(DEV).contiguous(), torch.from_numpy(b).to(DEV).contiguous()
    out = torch.full((16, 16), float("nan"), device=DEV)
    assert fn(ad.data_ptr(), bd.data_ptr(), out.data_ptr(), form, None) == 0, hip.lib().ipsx_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4, 5])
def test_mfma16_is_a_chain_in_slot_order(seed):
    a, b = operands(seed)
    # the operands tell orders apart: the ascending chain differs from the contract's in at least a row's worth of the tile
    assert np.count_nonzero(chain(a, b, range(8)).view(np.int32) != chain(a, b, CONTRACT).view(np.int32)) >= 16
    c16, c32 = run(a, b, 0), run(a, b, 1)
    differ = np.count_nonzero(c16.view(np.int32) != c32.view(np.int32))
    print("seed %d: entries of 256 that differ between the 16x16x4 and 32x32x2 forms: %d" % (seed, differ))
    assert differ == 0, "max abs diff %g" % float(np.abs(c16 - c32).max())
    assert np.array_equal(c16[9].view(np.int32), np.zeros(16, np.int32))              # the zero row stays +0
    assert np.array_equal(c16[11].view(np.int32), np.zeros(16, np.int32))             # (+0) + (-0 * w) = +0
