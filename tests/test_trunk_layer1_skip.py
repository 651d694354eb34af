"""fused_trunk_kernel tiles layer1 by position across its eight patches and leaves out the MFMAs of the tiles whose taps
read only the zero padding: the top and bottom rows' ky = 0 / ky = 2 taps, the left and right columns' kx = 0 / kx = 2 taps
(DESIGN 5.1).  The oracle runs those fma(0, w, acc) steps; leaving them out changes no bit.  Compared BITWISE
through an int32 view, so a zero of the other sign would show: layer1 weights of one sign only (the post-ReLU inputs are
>= 0, so every padded product is then -0 or +0), patches that are nonzero only on their border, blank patches, and ragged
counts around the eight patches per workgroup, each with an index list."""

import ctypes as C

import numpy as np
import pytest
import torch

from ips_amd import hip
from ips_amd.architecture import IPSNet
from oracle import oracle as orc
from tests.util import Golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAYER1_CONVS = tuple("encoder.4.%d.conv%d.weight" % (b, c) for b in (0, 1) for c in (1, 2))      # the four 3x3 convolutions


@pytest.fixture
def fused_only():
    """Every patch through fused_trunk_kernel (ipsx_dbg_fused_trunk_pair 1), not the pair kernel's remainder rule."""
    fn = hip.lib().ipsx_dbg_fused_trunk_pair
    fn.restype, fn.argtypes = None, [C.c_int]
    fn(1)
    yield
    fn(0)


def nets(layer1_sign=0):
    """(device net, oracle) of the headline's trunk; layer1_sign -1 / +1: layer1's convolutions with -|w| / +|w|."""
    g = Golden("mnist_full")
    cpu = g.net("cpu")
    if layer1_sign:
        sd = cpu.state_dict()
        for k in LAYER1_CONVS:
            sd[k].copy_(layer1_sign * sd[k].abs())
        cpu.load_state_dict(sd)
    net = IPSNet(torch.device(DEV), g.conf)
    net.load_state_dict(cpu.state_dict())
    return net.to(DEV).eval(), orc.Oracle(cpu)


def bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


def check(net, oracle, x, index=None):
    plan = hip.EncoderPlan(net.encoder, True)
    xd = x.to(DEV)
    want = torch.from_numpy(oracle.encode(x.numpy()))
    got = plan.encode(xd)
    assert hip.encoder_kernel_name(plan) == "fused_trunk_kernel"
    assert np.array_equal(bits(got), bits(want)), "max abs diff %g" % float((got.cpu() - want).abs().max())
    if index is not None:
        got_ix = plan.encode_indexed(xd, index.to(torch.int32).to(DEV))
        assert np.array_equal(bits(got_ix), bits(want[index.long()]))


def patches(n, seed, blank=0.3):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn((n, 1, 32, 32), generator=gen)
    x[torch.rand(n, generator=gen) < blank] = 0.0
    return x, torch.randperm(n, generator=gen)


def border_only(n, seed):
    x, index = patches(n, seed, blank=0.0)
    inner = torch.zeros((32, 32), dtype=torch.bool)
    inner[1:31, 1:31] = True
    x[:, :, inner] = 0.0
    return x, index


def test_default_plan_is_fused_trunk_kernel():
    net, _ = nets()
    plan = hip.EncoderPlan(net.encoder, True)
    plan.encode(patches(16, 3)[0].to(DEV))
    assert hip.encoder_kernel_name(plan) == "fused_trunk_kernel"


@pytest.mark.parametrize("n", [1, 7, 8, 9, 203, 2048 + 452, 4096 + 37])
def test_layer1_skip_bitwise_vs_oracle(n, fused_only):
    net, oracle = nets()
    x, index = patches(n, 100 + n)
    check(net, oracle, x, index)


@pytest.mark.parametrize("sign", [-1, 1])
def test_layer1_skip_one_signed_weights(sign, fused_only):
    net, oracle = nets(sign)
    x, index = patches(203, 17)
    check(net, oracle, x, index)


@pytest.mark.parametrize("sign", [0, -1, 1])
def test_layer1_skip_border_only_patches(sign, fused_only):
    """Nonzero only on rows / columns 0 and 31: after the stem and pool the signal sits next to the padded taps."""
    net, oracle = nets(sign)
    x, index = border_only(45, 9)
    check(net, oracle, x, index)


def test_layer1_skip_blank_patches(fused_only):
    net, oracle = nets(-1)
    check(net, oracle, torch.zeros((11, 1, 32, 32)), torch.arange(10, -1, -1))
