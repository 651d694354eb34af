"""``IPSNet.ips_ragged`` end to end at the shapes tests/test_ragged_e2e.py and tests/test_ragged_pad.py leave out: I > M and
I < M (I dividing neither M nor a slide's rows behind the memory), a net whose loop is scan_cam_kernel, one whose loop is
scan_large_kernel, and the 8 heads x 4 tokens image net with I != M - against the loop of solo ``net.ips(slide[None])``
calls (plus zero buffers under ``pad``), bit for bit, as tests/ragged_cases.py and tests/ragged_pad_cases.py state it."""

import pytest
import torch

import ragged_cases as rc
import ragged_pad_cases as pc
from ips_amd import hip, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def feature_net(M, I, lengths, shuffle=False):
    """F = 64, D = 64, D_k = D_v = 8, 8 heads, one token; no positions (a slide may be longer than any fixed conf.N)."""
    conf = synth.camelyon_conf(N=max(lengths), M=M, I=I, n_chan_in=64, D=64, D_k=8, D_v=8, D_inner=128, use_pos=False,
                               shuffle=shuffle, shuffle_style='batch')
    return conf, rc.make_net(conf, DEV)


def _slides(conf, lengths):
    return [s.to(DEV) for s in rc.make_slides(conf, lengths)]


def _count_scans(monkeypatch):
    seen = []

    def counted(name, real):
        def call(*a, **k):
            seen.append(name)
            return real(*a, **k)
        return call
    for name in ("scan_ragged", "scan", "scan_range"):
        monkeypatch.setattr(hip, name, counted(name, getattr(hip, name)))
    return seen


@pytest.mark.parametrize("shuffle", [False, True])
def test_feature_slides_with_chunks_longer_than_the_memory(shuffle):
    """M = 16, I = 24: scan_fast_kernel, I > M."""
    lengths = (17, 41, 40, 100, 65)
    conf, net = feature_net(16, 24, lengths, shuffle)
    assert hip.lib().ipsx_scan_workspace_bytes(1, 16, 24, 8, 1) == 0
    slides = _slides(conf, lengths)
    want = rc.solo_loop(net, slides)
    assert (want["shuffle"] is not None) == shuffle
    got = rc.ragged_call(net, slides)
    rc.assert_same_record(got, want)
    assert tuple(got["mem_idx"].shape) == (5, 16)


@pytest.mark.parametrize("pad,lengths", [(False, (25, 34, 35, 77, 60)), (True, (25, 24, 77, 3, 60))])
def test_feature_slides_with_chunks_shorter_than_the_memory(pad, lengths):
    """M = 24, I = 10: scan_fast_kernel, I < M; with ``pad`` a slide of exactly M rows and one of 3."""
    conf, net = feature_net(24, 10, lengths)
    assert hip.lib().ipsx_scan_workspace_bytes(1, 24, 10, 8, 1) == 0
    slides = _slides(conf, lengths)
    if pad:
        want = pc.expected(net, slides)
        pc.assert_same(pc.padded_call(net, slides), want)
        assert want["count"] == (24, 24, 24, 3, 24)
    else:
        rc.assert_same_record(rc.ragged_call(net, slides), rc.solo_loop(net, slides))


def test_a_net_whose_loop_is_scan_cam_kernel(monkeypatch):
    """M = I = 256, 8 heads, one token; 200 rows: a short slide between long ones."""
    lengths = (257, 612, 200, 1100)
    conf, net = feature_net(256, 256, lengths)
    assert hip.scan_persistent_groupable(256, 256, 8, 1) and hip.lib().ipsx_scan_workspace_bytes(1, 256, 256, 8, 1) == 0
    slides = _slides(conf, lengths)
    want = pc.expected(net, slides)
    seen = _count_scans(monkeypatch)
    got = pc.padded_call(net, slides)
    assert seen == ["scan_ragged"]
    pc.assert_same(got, want)
    assert got["count"] == (256, 256, 200, 256)


def test_a_net_whose_loop_is_scan_large_kernel(monkeypatch):
    """M = 16, I = 400: beyond the LDS-resident loops, the direct gather of 8 heads x one token."""
    lengths = (17, 500, 417, 1300, 9)
    conf, net = feature_net(16, 400, lengths)
    assert hip.lib().ipsx_scan_workspace_bytes(1, 16, 400, 8, 1) > 0
    slides = _slides(conf, lengths)
    want = pc.expected(net, slides)
    seen = _count_scans(monkeypatch)
    got = pc.padded_call(net, slides)
    assert seen == ["scan_ragged"]
    pc.assert_same(got, want)
    assert got["count"] == (16, 16, 16, 16, 9)


def test_image_slides_with_four_tokens_and_chunks_shorter_than_the_memory():
    """32-px patches, 8 heads x 4 tokens, M = 20, I = 12, 'batch' shuffling, positions on, a short slide last."""
    conf = rc.image_conf(M=20, shuffle=True, shuffle_style='batch').clone(I=12)
    net = rc.make_net(conf, DEV)
    assert hip.lib().ipsx_scan_workspace_bytes(1, 20, 12, 8, 4) == 0
    slides = _slides(conf, (21, 33, 70, 5))
    want = pc.expected(net, slides)
    assert want["shuffle"] is not None and want["shuffle"][3] is None and want["mem_pos"] is not None
    pc.assert_same(pc.padded_call(net, slides), want)
    assert tuple(want["mem_patch"].shape) == (4, 20, 1, 32, 32)
