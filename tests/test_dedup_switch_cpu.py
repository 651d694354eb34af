"""The three states of ``IPSX_DEDUP_BLANK`` without a GPU: ``0`` (no dedup anywhere), ``1`` (the explicit route of old, with
its refusals) and unset / ``auto`` (dedup inside the one counted launch only, every other route as under ``0`` - it refuses
nothing); the header / binding surface of the export behind ``auto``."""

import re

import pytest
import torch
import torch.distributed as torch_dist

from ips_amd import dist, hip, synth
from ips_amd.architecture import IPSNet
from view_u8_cases import plain_table

STATES = [(None, False, True), ("auto", False, True), ("0", False, False), ("1", True, False)]


def setenv(monkeypatch, value):
    if value is None:
        monkeypatch.delenv("IPSX_DEDUP_BLANK", raising=False)
    else:
        monkeypatch.setenv("IPSX_DEDUP_BLANK", value)


@pytest.mark.parametrize("value,explicit,auto", STATES, ids=[str(s[0]) for s in STATES])
def test_the_switch_has_three_states(value, explicit, auto, monkeypatch):
    setenv(monkeypatch, value)
    assert hip.dedup_blank() is explicit and hip.dedup_auto() is auto


def small_net(**kw):
    conf = synth.mnist_conf(N=40, M=8, I=8, **kw)
    return synth.fill_weights(IPSNet(torch.device("cpu"), conf), 5).eval(), conf


def bytes_images():
    g = torch.Generator().manual_seed(5)
    return torch.randint(0, 256, (2, 1, 80, 112), dtype=torch.uint8, generator=g)   # 32-px patches at stride 16: 24 per image


def uint8_source():
    x = bytes_images()
    return hip.PatchSource(images=x, view=hip.PatchView(x.shape, (32, 32), (16, 16)), table=plain_table(1))


def uint8_call():
    conf = synth.mnist_conf(N=24, M=4, I=6)
    net = synth.fill_weights(IPSNet(torch.device("cpu"), conf), 3).eval()
    net.set_patch_table(plain_table(1))
    return net.ips_image(bytes_images(), (32, 32), (16, 16))


def stream_call():
    net, conf = small_net(use_pos=True)
    x = synth.make_patches(conf, 2, seed=3)
    s = net.ips_stream()
    s.feed(x[:, :10])
    s.feed(x[:, 10:])
    return s.finish()


@pytest.mark.parametrize("value", [None, "auto", "0"])
def test_auto_and_off_refuse_nothing(value, monkeypatch, tmp_path):
    setenv(monkeypatch, value)
    assert uint8_source().dtype == torch.uint8
    assert uint8_call()[0].shape == (2, 4, 1, 32, 32)
    assert stream_call()[0].shape[:2] == (2, 8)
    net, conf = small_net(use_pos=True)
    x = synth.make_patches(conf, 2, seed=3)
    torch_dist.init_process_group("gloo", init_method="file://{}".format(tmp_path / "store"), rank=0, world_size=1)
    try:
        mem_patch, _, mem_idx = dist.ips_sharded(net, x.contiguous(), x.shape[1])
    finally:
        torch_dist.destroy_process_group()
    want = net.ips(x)[0]
    assert torch.equal(mem_patch, want) and torch.equal(mem_idx, net.last_mem_idx)


def test_the_explicit_route_keeps_its_refusals(monkeypatch):
    setenv(monkeypatch, "1")
    with pytest.raises(TypeError, match="dedup"):
        uint8_source()
    with pytest.raises(TypeError, match="dedup"):
        stream_call()
    net, conf = small_net()
    net.set_patch_table(plain_table(1))
    monkeypatch.setattr(hip, "on_device", lambda dev: True)               # (the check of a call on the GPU, which needs none)
    with pytest.raises(TypeError, match="IPSX_DEDUP_BLANK=1 with uint8"):
        net._check_u8(torch.zeros((2, 40, 1, 32, 32), dtype=torch.uint8))
    setenv(monkeypatch, None)
    net._check_u8(torch.zeros((2, 40, 1, 32, 32), dtype=torch.uint8))


def test_header_and_binding_name_the_export():
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ipsx.h")).read()
    for name, n_args in (("ipsx_trunk_encode_parts_dedup", 13), ("ipsx_trunk_parts_dedup_workspace_bytes", 2)):
        decl = re.search(r"^(?:int|size_t) %s\(([^;]*)\);" % name, header, re.M)
        assert decl and decl.group(1).count(",") + 1 == n_args
        assert len(hip._EXPORTS[name][1]) == n_args
        assert len(getattr(hip.lib(), name).argtypes) == n_args
    # refused before anything is launched: no device is needed to see it
    rc = hip.lib().ipsx_trunk_encode_parts_dedup(None, None, None, 0, None, None, 0, None, None, None, 0, None, None)
    assert rc != 0 and b"trunk_encode_parts_dedup" in hip.lib().ipsx_last_error()
    assert hip.lib().ipsx_trunk_parts_dedup_workspace_bytes(None, 100) == 0
