"""``IPSNet.ips_ragged`` on the device against the loop of solo ``net.ips(slide[None])`` calls it replaces - every output of
the contract bit for bit (``mem_patch``, ``mem_pos``, ``last_mem_idx``, ``last_mem_emb``, ``last_shuffle``, both RNG
streams): one encoder pass over all rows, one packed logits table, ONE ``ipsx_scan_ragged``, ONE ``ipsx_ragged_finish``."""

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


# ------------------------------------------------------------------ the call without ``pad`` ends as the padded one does
M8, I4 = 8, 4


@pytest.fixture(scope="module")
def small_cases():
    """A feature net with M = 8, I = 4, four slides, and the solo loop's record for them: made once per configuration."""
    made = {}

    def get(shuffle, use_pos):
        if (shuffle, use_pos) not in made:
            conf = rc.feature_conf(M=M8, shuffle=shuffle, shuffle_style='batch', use_pos=use_pos).clone(I=I4)
            net = rc.make_net(conf, DEV)
            slides = _on_device(rc.make_slides(conf, (M8 + 1, 3 * M8, 3 * M8 + 5, 7 * M8)))
            made[(shuffle, use_pos)] = (net, slides, rc.solo_loop(net, slides))
        return made[(shuffle, use_pos)]
    return get


def test_launches_of_a_call_without_pad(small_cases, monkeypatch):
    """On aligned rows: one encoder pass, one logits table, ONE ``ipsx_scan_ragged``, ONE ``ipsx_ragged_finish`` - and no
    ``gather_rows`` launch until ``last_mem_emb`` is read."""
    net, slides, want = small_cases(False, True)
    seen = []

    def counted(name, real):
        def call(*a, **k):
            seen.append(name)
            return real(*a, **k)
        return call
    for name in ("scan_ragged", "ragged_finish", "gather_rows", "logits", "scan", "scan_range"):
        monkeypatch.setattr(hip, name, counted(name, getattr(hip, name)))
    plan = type(net.plan)                                      # (every eval-mode encoder pass on the device goes through the plan)
    for name in ("encode", "encode_source"):
        monkeypatch.setattr(plan, name, counted("encode", getattr(plan, name)))
    net.ips_ragged(slides)
    assert sorted(seen) == ["encode", "logits", "ragged_finish", "scan_ragged"]
    assert net.last_mem_count is None
    del seen[:]
    assert rc._same(net.last_mem_emb.cpu(), want["mem_emb"])
    assert seen == ["gather_rows"]


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("use_pos", [False, True])
def test_unaligned_rows_without_pad_equal_the_solo_loop(small_cases, monkeypatch, shuffle, use_pos):
    """Rows that are no whole 16-byte units end in the ``gather_rows`` launches (``_finish_aten``)."""
    net, slides, want = small_cases(shuffle, use_pos)
    assert (want["shuffle"] is not None) == shuffle and (want["mem_pos"] is not None) == use_pos
    monkeypatch.setattr(hip, "ragged_finish_supported", lambda rows, pos: False)
    monkeypatch.setattr(hip, "ragged_finish", None)
    got = rc.ragged_call(net, slides)
    rc.assert_same_record(got, want)
    assert net.last_mem_count is None and tuple(got["mem_idx"].shape) == (4, M8)
