"""fused_trunk_kernel leaves out the MFMAs of the 4x4 stage's edge tiles that only multiply the zero padding.
The oracle runs those fma(0, w, acc) steps; leaving them out changes no bit.  Compared BITWISE through an int32
view, so a zero of the other sign would show, on inputs and weights chosen to make such zeros: ragged counts around the
kernel's eight patches per workgroup, index lists, blank patches, patches that are nonzero only on their border, and
4x4-stage weights of one sign only (every padded product is then -0)."""

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
LAYER2_CONVS = tuple("encoder.5.%d.conv%d.weight" % (b, c) for b in (0, 1) for c in (1, 2))      # the 3x3 convolutions of layer2


@pytest.fixture
def fused_only():
    """Every patch through fused_trunk_kernel (ipsx_dbg_fused_trunk_pair 1), not the pair kernel's remainder rule."""
    fn = hip.lib().ipsx_dbg_fused_trunk_pair
    fn.restype, fn.argtypes = None, [C.c_int]
    fn(1)
    yield
    fn(0)


def nets(negative_layer2=False):
    """(device net, oracle) of the headline's trunk; negative_layer2: the 4x4 stage's convolutions with -|w|."""
    g = Golden("mnist_full")
    cpu = g.net("cpu")
    if negative_layer2:
        sd = cpu.state_dict()
        for k in LAYER2_CONVS:
            sd[k].copy_(-sd[k].abs())
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


def test_weights_have_both_signs():
    net, _ = nets()
    sd = net.state_dict()
    for k in LAYER2_CONVS:
        assert bool((sd[k] > 0).any()) and bool((sd[k] < 0).any()), k


@pytest.mark.parametrize("n", [1, 7, 8, 9, 203, 2048 + 452, 4096 + 37])
def test_padding_skip_bitwise_vs_oracle(n, fused_only):
    net, oracle = nets()
    x, index = patches(n, n)
    check(net, oracle, x, index)


def test_padding_skip_blank_patches(fused_only):
    net, oracle = nets()
    check(net, oracle, torch.zeros((13, 1, 32, 32)), torch.arange(12, -1, -1))


@pytest.mark.parametrize("negative_layer2", [False, True])
def test_padding_skip_border_only_patches(negative_layer2, fused_only):
    """Nonzero only on rows / columns 0 and 31: the taps that read the padding are next to the only signal there is."""
    net, oracle = nets(negative_layer2)
    x, index = patches(37, 5, blank=0.0)
    inner = torch.zeros((32, 32), dtype=torch.bool)
    inner[1:31, 1:31] = True
    x[:, :, inner] = 0.0
    check(net, oracle, x, index)


def test_padding_skip_one_signed_layer2_weights(fused_only):
    net, oracle = nets(negative_layer2=True)
    x, index = patches(203, 11)
    check(net, oracle, x, index)
