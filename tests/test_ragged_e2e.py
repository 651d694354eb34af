"""``IPSNet.ips_ragged`` on the device against the loop of solo ``net.ips(slide[None])`` calls it replaces - every output of
the contract bit for bit (``mem_patch``, ``mem_pos``, ``last_mem_idx``, ``last_mem_emb``, ``last_shuffle``, both RNG
streams): one encoder pass over all rows, one packed logits table, ONE ``ipsx_scan_ragged``, gathers over global rows."""

import pytest
import torch

import ragged_cases as rc
from ips_amd import hip
from ips_amd.ragged import Ragged

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M = 16


def _on_device(slides):
    return [s.to(DEV) for s in slides]


@pytest.fixture(scope="module")
def feature_nets():
    made = {}

    def get(shuffle, use_pos):
        if (shuffle, use_pos) not in made:
            conf = rc.feature_conf(M=M, shuffle=shuffle is not None, shuffle_style=shuffle or 'batch', use_pos=use_pos)
            made[(shuffle, use_pos)] = (conf, rc.make_net(conf, DEV))
        return made[(shuffle, use_pos)]
    return get


# ('instance' with use_pos: ips() itself raises on a slide shorter than conf.N, ips_ragged refuses it - tests/test_ragged_cpu.py)
@pytest.mark.parametrize("shuffle,use_pos", [(None, False), ("instance", False), (None, True), ("batch", True)])
def test_feature_slides_equal_the_solo_loop(feature_nets, shuffle, use_pos):
    conf, net = feature_nets(shuffle, use_pos)
    slides = _on_device(rc.make_slides(conf, (M + 1, 3 * M, 3 * M + 5, 7 * M)))
    want = rc.solo_loop(net, slides)
    assert (want["shuffle"] is not None) == (shuffle is not None)
    got = rc.ragged_call(net, slides)
    rc.assert_same_record(got, want)
    assert tuple(got["mem_idx"].shape) == (4, M) and tuple(got["mem_emb"].shape) == (4, M, conf.D)


def test_half_rows_under_the_bf16_projector(monkeypatch):
    monkeypatch.setenv("IPSX_PRECISION", "bf16")
    for shuffle in (False, True):
        conf = rc.feature_conf(M=M, shuffle=shuffle, shuffle_style='instance')
        net = rc.make_net(conf, DEV)
        slides = _on_device(rc.make_slides(conf, (M + 1, 3 * M, 3 * M + 5, 7 * M), dtype=torch.float16))
        want = rc.solo_loop(net, slides)
        got = rc.ragged_call(net, slides)
        rc.assert_same_record(got, want)
        assert got["mem_patch"].dtype == torch.float16


@pytest.mark.parametrize("shuffle", [False, True])
def test_image_slides_equal_the_solo_loop(shuffle):
    conf = rc.image_conf(M=M, shuffle=shuffle, shuffle_style='batch')
    net = rc.make_net(conf, DEV)
    slides = _on_device(rc.make_slides(conf, (17, 40, 100)))
    want = rc.solo_loop(net, slides)
    rc.assert_same_record(rc.ragged_call(net, slides), want)
    assert want["mem_pos"] is not None and tuple(want["mem_patch"].shape) == (3, M, 1, 32, 32)


def test_host_and_device_ragged_agree_and_ips_takes_a_ragged(feature_nets):
    conf, net = feature_nets(None, True)
    host = rc.make_slides(conf, (M + 1, 3 * M, 3 * M + 5, 7 * M))
    on_dev = rc.ragged_call(net, Ragged.from_list(_on_device(host)))
    rc.assert_same_record(rc.ragged_call(net, Ragged.from_list(host)), on_dev)
    rc.assert_same_record(rc.ragged_call(net, Ragged.from_list(host).pin_memory()), on_dev)
    rc.assert_same_record(rc.ragged_call(net, Ragged.from_list(_on_device(host)), through_ips=True), on_dev)
    r = Ragged.from_list(host).to(DEV)
    assert r.offsets.device.type == "cuda" and r.to(DEV) is r and r.to(DEV).offsets is r.offsets


def test_one_scan_launch_per_call(feature_nets, monkeypatch):
    """ONE ``ipsx_scan_ragged`` per call, and none of the per-image loop entries."""
    conf, net = feature_nets(None, False)
    slides = _on_device(rc.make_slides(conf, (M + 1, 3 * M, 3 * M + 5, 7 * M)))
    seen = []
    real = hip.scan_ragged

    def counted(*a, **k):
        seen.append("ragged")
        return real(*a, **k)
    monkeypatch.setattr(hip, "scan_ragged", counted)
    for name in ("scan", "scan_range"):
        monkeypatch.setattr(hip, name, lambda *a, _n=name, **k: seen.append(_n))
    net.ips_ragged(slides)
    assert seen == ["ragged"]
