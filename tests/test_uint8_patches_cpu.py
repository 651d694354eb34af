"""uint8 patch storage, the parts that need no GPU: ``quant.patch_table`` is the datasets' own tensor ops bit for bit, the
ATen path of ``IPSNet.ips`` selects on bytes what it selects on the expanded tensor and returns float32 patches, the state
dict is untouched, and the C ABI carries the three new entry points at version 3.06."""

import ctypes
import os
import re

import pytest
import torch

from ips_amd import hip, quant, synth
from ips_amd.architecture import IPSNet

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ipsx.h")
NEW = ("ipsx_trunk_encode_u8", "ipsx_trunk_encode_indexed_u8", "ipsx_dequant_patches")
TRAFFIC_MEAN, TRAFFIC_STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]        # data/traffic/traffic_dataset.py:287


def rand_table(n_chan, seed):
    t = torch.randn((n_chan, 256), generator=torch.Generator().manual_seed(seed))
    assert bool((t[:, 0] != 0).all())
    return t


def rand_bytes(shape, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)
    flat = q.view(-1, *shape[-3:])
    flat[1::2] = 0                                      # every second patch all zeros: tied scores
    flat[0].view(-1)[:4] = torch.tensor([0, 127, 128, 255], dtype=torch.uint8)
    return q


# ---------------------------------------------------------------------------------------------- the table
def test_patch_table_is_the_datasets_ops_bit_for_bit():
    u = torch.arange(256, dtype=torch.uint8)
    plain = quant.patch_table(1)
    assert plain.shape == (1, 256) and plain.dtype == torch.float32 and torch.equal(plain[0], u.float().div(255))
    three = quant.patch_table(3)
    assert three.shape == (3, 256) and all(torch.equal(three[c], u.float().div(255)) for c in range(3))
    assert float(plain[0, 0]) == 0.0 and float(plain[0, 255]) == 1.0


def test_patch_table_with_the_traffic_sign_normalisation():
    u = torch.arange(256, dtype=torch.uint8)
    t = quant.patch_table(3, TRAFFIC_MEAN, TRAFFIC_STD)
    assert t.shape == (3, 256) and t.dtype == torch.float32
    for c in range(3):
        assert torch.equal(t[c], u.float().div(255).sub(TRAFFIC_MEAN[c]).div(TRAFFIC_STD[c]))
    assert not torch.equal(t[0], t[1]) and not torch.equal(t[1], t[2])
    assert float(t[0, 0]) < -2.0                         # a dequantised pad would not be 0.0f
    # ... which is what ToTensor + Normalize make of an 8-bit image, pixel by pixel
    img = torch.randint(0, 256, (3, 5, 7), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
    x = img.float().div(255)
    x = x.sub(torch.tensor(TRAFFIC_MEAN).view(3, 1, 1)).div(torch.tensor(TRAFFIC_STD).view(3, 1, 1))
    assert torch.equal(quant.dequant(img, t), x)


def test_patch_table_refuses_bad_lengths():
    with pytest.raises(ValueError):
        quant.patch_table(3, [0.5], [0.5])
    with pytest.raises(ValueError):
        quant.patch_table(3, TRAFFIC_MEAN, TRAFFIC_STD[:2])
    with pytest.raises(ValueError):
        quant.patch_table(1, TRAFFIC_MEAN, TRAFFIC_STD)
    with pytest.raises(ValueError):
        quant.patch_table(3, TRAFFIC_MEAN)
    with pytest.raises(ValueError):
        quant.patch_table(0)


# ---------------------------------------------------------------------------------------------- the ATen path
def cpu_net(conf, table_seed=3):
    net = synth.fill_weights(IPSNet(torch.device("cpu"), conf), 1).eval()
    net.set_patch_table(rand_table(conf.n_chan_in, table_seed))
    return net


def run(net, x, seed=4):
    torch.manual_seed(seed)
    mem_patch, mem_pos = net.ips(x)
    return mem_patch, mem_pos, net.last_mem_idx, net.last_mem_emb


@pytest.mark.parametrize("name,shuffle", [("mnist", False), ("mnist", True), ("traffic", False)])
def test_aten_path_selects_on_bytes_what_it_selects_on_the_expanded_tensor(name, shuffle):
    conf = (synth.mnist_conf(N=150, M=16, I=24, shuffle=shuffle, shuffle_style="instance") if name == "mnist" else
            synth.traffic_conf(N=20, M=4, I=6, patch=40))
    net = cpu_net(conf)
    q = rand_bytes((2, conf.N, conf.n_chan_in) + tuple(conf.patch_size), 5)
    x = quant.dequant(q, net.patch_table)
    want, got = run(net, x), run(net, q)
    assert got[0].dtype == torch.float32 and torch.equal(got[0], want[0])
    assert (got[1] is None) == (want[1] is None) and (got[1] is None or torch.equal(got[1], want[1]))
    assert torch.equal(got[2], want[2]) and torch.equal(got[3], want[3])
    if not shuffle:
        for b in range(2):
            assert torch.equal(got[0][b], x[b, got[2][b]])


def test_the_shortcut_returns_the_dequantised_tensor():
    conf = synth.mnist_conf(N=12, M=16, I=16)
    net = cpu_net(conf)
    q = rand_bytes((2, 12, 1, 32, 32), 6)
    want, got = run(net, quant.dequant(q, net.patch_table)), run(net, q)
    assert got[0].dtype == torch.float32 and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert got[2] is None and want[2] is None


def test_bytes_without_a_table_are_refused_and_the_table_is_validated():
    conf = synth.mnist_conf(N=40, M=8, I=8)
    net = synth.fill_weights(IPSNet(torch.device("cpu"), conf), 1).eval()
    q = rand_bytes((1, 40, 1, 32, 32), 7)
    assert net.patch_table is None
    with pytest.raises(TypeError, match="set_patch_table"):
        net.ips(q)
    with pytest.raises(TypeError, match="set_patch_table"):
        net.ips(q[:, :4])                                # the shortcut too
    for bad, exc in ((rand_table(3, 1), ValueError), (rand_table(1, 1)[:, :100], ValueError), (rand_table(1, 1).double(), TypeError),
                     (rand_table(1, 1).view(256), ValueError), (torch.full((1, 256), float("inf")), ValueError)):
        with pytest.raises(exc):
            net.set_patch_table(bad)
    assert net.patch_table is None
    net.set_patch_table(rand_table(1, 1))
    assert net.ips(q)[0].dtype == torch.float32
    net.set_patch_table(None)
    with pytest.raises(TypeError, match="set_patch_table"):
        net.ips(q)
    feat = IPSNet(torch.device("cpu"), synth.camelyon_conf(N=64, M=8, I=8, n_chan_in=32))
    with pytest.raises(TypeError):
        feat.set_patch_table(rand_table(1, 1))


def test_the_state_dict_does_not_know_the_table():
    conf = synth.traffic_conf(N=20, M=4, I=6, patch=40)
    net = IPSNet(torch.device("cpu"), conf)
    before = list(net.state_dict().keys())
    net.set_patch_table(quant.patch_table(3, TRAFFIC_MEAN, TRAFFIC_STD))
    assert list(net.state_dict().keys()) == before
    assert "patch_table" not in dict(net.named_buffers()) and "patch_table" not in dict(net.named_parameters())
    assert net.patch_table.shape == (3, 256)


# ---------------------------------------------------------------------------------------------- the C ABI
def test_header_library_and_binding_carry_the_new_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(ipsx_[a-z0-9_]+)\s*\(", text))
    assert int(re.search(r"#define IPSX_VERSION (\d+)", text).group(1)) == 306
    lib = ctypes.CDLL(hip.library_path())
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in hip._EXPORTS, name
    assert hip.lib().ipsx_version() == 306
    for name in ("ipsx_trunk_encode_u8", "ipsx_trunk_encode_indexed_u8"):
        decl = re.search(r"int %s\((.*?)\);" % name, text, re.S).group(1)
        assert "const uint8_t* patches, const float* table" in decl, decl
    # argument checks come before any device work: no GPU is needed to be refused
    assert hip.lib().ipsx_dequant_patches(None, None, None, 1, 1, 1, None) != 0
    assert b"dequant_patches" in hip.lib().ipsx_last_error()
