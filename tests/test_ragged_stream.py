"""``IPSNet.ips_ragged_stream()`` on the device, end to end: bit for bit what ``net.ips_ragged`` on the joined
pieces returns and leaves behind - the nets, slide lengths and feeding schedules of tests/test_ragged_stream_cpu.py, pieces
on the host and on the device, a feature net at scan_cam_kernel's shape, float16 rows under ``IPSX_PRECISION=bf16`` -, the
observable state after every feed, the buffer set flipped in both directions within one stream, and a feed in which no slide
completes a chunk."""

import pytest
import torch

from ips_amd import hip
from ips_amd.ragged import Ragged
from tests import ragged_cases as rc
from tests import ragged_stream_cases as rsc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def nets():
    """name -> {pad: (net, host slides, record of ips_ragged on the device, last_mem_count)}: computed once"""
    out = {}
    for name in rsc.NETS:
        net = rsc.make_net(name, DEV)
        out[name] = {}
        for pad in (False, True):
            slides = rc.make_slides(rsc.conf_of(name), rsc.lengths_of(net.M, net.I, pad))
            want, count = rsc.reference(net, [t.to(DEV) for t in slides], pad)
            out[name][pad] = (net, slides, want, count)
    return out


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("schedule", rsc.SCHEDULES)
@pytest.mark.parametrize("pad", [False, True])
@pytest.mark.parametrize("name", rsc.NETS)
def test_the_stream_leaves_what_ips_ragged_leaves(name, pad, schedule, where, nets):
    net, slides, want, count = nets[name][pad]
    s, out = rsc.run_schedule(net, slides, schedule, pad, device=DEV if where == "device" else None)
    assert out[0].device.type == "cuda"
    rc.assert_same_record(rsc.record(net, out), want)
    assert net.last_mem_count == count
    assert torch.equal(s.mem_idx, net.last_mem_idx)
    want_iters = tuple((n - net.M + net.I - 1) // net.I if n > net.M else 0 for n in s.fed)
    assert s.iterations == want_iters


def test_a_host_ragged_in_slabs(nets):
    net, slides, want, _ = nets["image"][True]
    batch = Ragged.from_list(slides, pad=True)
    assert not batch.rows.is_cuda
    rsc._seed()
    out = net.ips_ragged_stream(pad=True).feed_all(batch, 23).finish()
    rc.assert_same_record(rsc.record(net, out), want)


@pytest.mark.parametrize("name", rsc.NETS)
def test_observable_state_after_every_feed(name, nets):
    """``fed``, ``iterations`` and ``mem_idx`` against solo device streams fed the same pieces"""
    net, slides, _, _ = nets[name][True]
    M = net.M
    solo = [net.ips_stream() for _ in slides]

    def after_feed(s, pieces):
        for b, p in enumerate(pieces):
            if p.shape[0]:
                solo[b].feed(p[None])
        assert s.fed == tuple(t.fed for t in solo) and s.iterations == tuple(t.iterations for t in solo)
        idx = s.mem_idx.cpu()
        for b, t in enumerate(solo):
            if t.fed >= M:
                assert torch.equal(idx[b], t.mem_idx[0].cpu()), (b, t.fed)
            else:
                assert (idx[b] == -1).all()

    rsc.run_schedule(net, slides, "mixed", True, after_feed=after_feed)


def test_the_set_flips_in_both_directions_and_a_feed_may_complete_no_chunk(nets):
    """M = I = 16.  Feed 1: 20 | 3 rows, no chunk (append in place, set 0).  Feed 2: 30 | 0, slide 0 selects, slide 1 moves
    (set 1).  Feed 3: 2 | 5, no chunk (append, set 1).  Feed 4: 20 | 30, both select (back to set 0).  Feed 5: 3 | 1, no chunk;
    ``finish()`` runs two ragged last chunks."""
    net, _, _, _ = nets["feature"][False]
    a, b = rc.make_slides(rsc.conf_of("feature"), (75, 39), seed=9)
    rsc._seed()
    want = rsc.record(net, net.ips_ragged([a.to(DEV), b.to(DEV)]))
    feeds = [(20, 3), (30, 0), (2, 5), (20, 30), (3, 1)]
    cur = [0, 1, 1, 0, 0]
    iters = [(0, 0), (2, 0), (2, 0), (3, 1), (3, 1)]
    rsc._seed()
    s = net.ips_ragged_stream()
    lo = [0, 0]
    for k, (na, nb) in enumerate(feeds):
        s.feed([a[lo[0]:lo[0] + na], b[lo[1]:lo[1] + nb].to(DEV)])          # (a host piece and a device piece)
        lo = [lo[0] + na, lo[1] + nb]
        assert s._cur == cur[k] and s.iterations == iters[k], k
    assert s.fed == (75, 39)
    out = s.finish()
    assert s.iterations == (4, 2)
    rc.assert_same_record(rsc.record(net, out), want)


def test_scan_cam_shape_with_padding():
    """M = I = 256 (scan_cam_kernel), F = 64: 700 / 300 / 257 / 100 rows, ``pad=True``"""
    net = rsc.make_net("feature_cam", DEV)
    slides = rc.make_slides(rsc.conf_of("feature_cam"), (700, 300, 257, 100))
    want, count = rsc.reference(net, [t.to(DEV) for t in slides], True)
    assert count == (256, 256, 256, 100)
    for schedule in ("mixed", "feed_all"):
        s, out = rsc.run_schedule(net, slides, schedule, True) if schedule == "feed_all" else _cam_mixed(net, slides)
        rc.assert_same_record(rsc.record(net, out), want)
        assert net.last_mem_count == count and s.iterations == (2, 1, 1, 0)


def _cam_mixed(net, slides):
    """slabs of 300 | 90 | 257 | 40 rows per feed: slides end at different feeds"""
    rsc._seed()
    s = net.ips_ragged_stream(pad=True)
    steps = (300, 90, 257, 40)
    lo = [0] * 4
    while any(lo[b] < slides[b].shape[0] for b in range(4)):
        s.feed([slides[b][lo[b]:lo[b] + steps[b]] for b in range(4)])
        lo = [min(lo[b] + steps[b], slides[b].shape[0]) for b in range(4)]
    return s, s.finish()


def test_float16_rows_under_bf16(monkeypatch):
    monkeypatch.setenv("IPSX_PRECISION", "bf16")
    assert hip.precision() == "bf16"
    net = rsc.make_net("feature", DEV)
    for pad in (False, True):
        slides = rc.make_slides(rsc.conf_of("feature"), rsc.lengths_of(net.M, net.I, pad), dtype=torch.float16)
        want, count = rsc.reference(net, [t.to(DEV) for t in slides], pad)
        for schedule in rsc.SCHEDULES:
            s, out = rsc.run_schedule(net, slides, schedule, pad)
            assert out[0].dtype == torch.float16
            rc.assert_same_record(rsc.record(net, out), want)
            assert net.last_mem_count == count


def test_refusals_on_the_device(monkeypatch):
    net = rsc.make_net("feature", DEV)
    a, b = rc.make_slides(rsc.conf_of("feature"), (40, 9))
    with pytest.raises(TypeError, match="IPSX_PRECISION=bf16"):
        net.ips_ragged_stream().feed([a.half(), b.half()])               # fp32 precision: what the encoder plan would refuse
    s = net.ips_ragged_stream().feed([a[:10], b[:4]])
    free = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match="every length is 0"):
        s.feed([a[:0], b[:0]])
    with pytest.raises(TypeError, match="float64"):
        s.feed([a[:2].double(), b[:2].double()])
    assert torch.cuda.memory_allocated() == free
    s.feed([a[10:], b[4:]])
    with pytest.raises(ValueError, match="slide 1 has 9 rows"):
        s.finish()
