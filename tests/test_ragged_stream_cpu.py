"""``IPSNet.ips_ragged_stream()`` on the CPU device: B solo ``IPSStream`` state machines on ATen ops, held bit for
bit to ``net.ips_ragged`` on the joined pieces for schedules whose pieces end anywhere, observable after every feed, and
its refusals; the header / binding surface of the two exports behind the device route, and the argument checks of
``ipsx_stream_commit_ragged`` and ``ipsx_scan_ragged_spans`` that need no device."""

import ctypes as C
import os
import re

import pytest
import torch

from ips_amd import hip
from ips_amd.ragged import Ragged
from ips_amd.ragged_stream import RaggedIPSStream
from tests import ragged_cases as rc
from tests import ragged_stream_cases as rsc

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ipsx.h")


@pytest.fixture(scope="module")
def nets():
    """name -> {pad: (net, slides, record of ips_ragged, last_mem_count)}: computed once, never changed"""
    out = {}
    for name in rsc.NETS:
        net = rsc.make_net(name, "cpu")
        out[name] = {}
        for pad in (False, True):
            slides = rc.make_slides(rsc.conf_of(name), rsc.lengths_of(net.M, net.I, pad))
            want, count = rsc.reference(net, slides, pad)
            out[name][pad] = (net, slides, want, count)
    return out


@pytest.mark.parametrize("schedule", rsc.SCHEDULES)
@pytest.mark.parametrize("pad", [False, True])
@pytest.mark.parametrize("name", rsc.NETS)
def test_the_stream_leaves_what_ips_ragged_leaves(name, pad, schedule, nets):
    net, slides, want, count = nets[name][pad]
    s, out = rsc.run_schedule(net, slides, schedule, pad)
    assert isinstance(s, RaggedIPSStream)
    rc.assert_same_record(rsc.record(net, out), want)
    assert net.last_mem_count == count and (count is None) == (not pad)
    assert torch.equal(s.mem_idx, net.last_mem_idx)


def test_a_ragged_feed_is_a_list_feed(nets):
    net, slides, want, _ = nets["feature"][True]
    rsc._seed()
    s = net.ips_ragged_stream(pad=True)
    lo = [0] * len(slides)
    for feed in rsc.mixed_schedule([t.shape[0] for t in slides], net.M, net.I):
        s.feed(Ragged.from_list([t[lo[b]:lo[b] + n] for b, (t, n) in enumerate(zip(slides, feed))]))
        lo = [lo[b] + n for b, n in enumerate(feed)]
    rc.assert_same_record(rsc.record(net, s.finish()), want)
    s = net.ips_ragged_stream(pad=True).feed_all(Ragged.from_list(slides), 41)
    rc.assert_same_record(rsc.record(net, s.finish()), want)


@pytest.mark.parametrize("name", rsc.NETS)
def test_observable_state_after_every_feed(name, nets):
    """``fed``, ``iterations`` and ``mem_idx`` against solo streams fed the same pieces"""
    net, slides, _, _ = nets[name][True]
    M = net.M
    solo = [net.ips_stream() for _ in slides]
    fresh = net.ips_ragged_stream(pad=True)
    assert fresh.fed == () and fresh.iterations == () and fresh.mem_idx is None

    def after_feed(s, pieces):
        for b, p in enumerate(pieces):
            if p.shape[0]:
                solo[b].feed(p[None])
        assert s.fed == tuple(t.fed for t in solo) and all(isinstance(v, int) for v in s.fed)
        assert s.iterations == tuple(t.iterations for t in solo)
        idx = s.mem_idx
        assert idx.shape == (len(slides), M) and idx.dtype == torch.int64
        for b, t in enumerate(solo):
            if t.fed >= M:
                assert torch.equal(idx[b], t.mem_idx[0]), (b, t.fed)
            else:
                assert torch.equal(idx[b], torch.full((M,), -1, dtype=torch.int64))

    s, _ = rsc.run_schedule(net, slides, "mixed", True, after_feed=after_feed)
    want_iters = tuple((n - M + net.I - 1) // net.I if n > M else 0 for n in s.fed)
    assert s.iterations == want_iters


# ------------------------------------------------------------------ refusals
def _untouched(net, call, exc, match, monkeypatch, env=None):
    """``call()`` raises ``exc`` and leaves torch's RNG state and ``net.last_*`` as they were, before any allocation"""
    net.ips_ragged(rc.make_slides(rsc.conf_of("feature"), (20, 30)))          # something to keep
    kept = (net.last_mem_idx, net.last_mem_emb, net.last_shuffle, net.last_mem_count)
    rng = torch.get_rng_state()

    def boom(*a, **k):
        raise AssertionError("an allocation or an encoder pass before the refusal")
    with monkeypatch.context() as m:
        for k, v in (env or {}).items():
            m.setenv(k, v)
        for fn in ("empty", "zeros", "full", "cat", "tensor", "arange"):
            m.setattr(torch, fn, boom)
        m.setattr(net, "_embed", boom)
        with pytest.raises(exc, match=match):
            call()
    assert torch.equal(torch.get_rng_state(), rng)
    assert net.last_mem_idx is kept[0] and net.last_mem_emb is kept[1] and net.last_shuffle is kept[2] and net.last_mem_count is kept[3]


def test_refusals_leave_everything_untouched(monkeypatch):
    net = rsc.make_net("feature", "cpu")
    a, b = rc.make_slides(rsc.conf_of("feature"), (40, 9))

    def started(pad=False):
        return net.ips_ragged_stream(pad=pad).feed([a[:10], b[:4]])

    s = started()
    s.feed([a[10:], b[4:4]])
    _untouched(net, s.finish, ValueError, "slide 1 has 4 rows", monkeypatch)            # not above M, without pad
    s = started(pad=True)
    s.feed([a[10:], b[4:]])
    s.finish()
    _untouched(net, lambda: s.feed([a[:1], b[:1]]), RuntimeError, "finished", monkeypatch)
    _untouched(net, s.finish, RuntimeError, "finished", monkeypatch)
    s = net.ips_ragged_stream(pad=True).feed([a, b[:0]])
    _untouched(net, s.finish, ValueError, "slide 1 has no rows", monkeypatch)           # nothing to pad
    s = started()
    _untouched(net, lambda: s.feed([a[:0], b[:0]]), ValueError, "every length is 0", monkeypatch)
    _untouched(net, lambda: s.feed([a[:3]]), ValueError, "stream of B = 2", monkeypatch)
    _untouched(net, lambda: s.feed([a[:3], b[:3], b[:3]]), ValueError, "stream of B = 2", monkeypatch)
    _untouched(net, lambda: s.feed([a[:3, :32], b[:3, :32]]), ValueError, "rows", monkeypatch)
    _untouched(net, lambda: s.feed([a[:3].double(), b[:3].double()]), TypeError, "float64", monkeypatch)
    _untouched(net, lambda: s.feed([a[:3], b[:3].half()]), ValueError, "one row shape and dtype", monkeypatch)
    _untouched(net, lambda: s.feed(a[:3]), ValueError, "a feed is", monkeypatch)
    _untouched(net, lambda: s.feed([a[:3][None], b[:3][None]]), ValueError, "a feed is", monkeypatch)
    _untouched(net, lambda: net.ips_ragged_stream().feed([a[:3].to(torch.uint8), b[:3].to(torch.uint8)]), TypeError, "uint8",
               monkeypatch)
    _untouched(net, lambda: net.ips_ragged_stream().feed([a[:3].double(), b[:3].double()]), TypeError, "float64", monkeypatch)
    _untouched(net, lambda: net.ips_ragged_stream().finish(), RuntimeError, "nothing was fed", monkeypatch)
    hip.weights_changed()                        # what an optimizer step does
    _untouched(net, lambda: s.feed([a[10:12], b[4:5]]), RuntimeError, "weights changed", monkeypatch)
    _untouched(net, s.finish, RuntimeError, "weights changed", monkeypatch)
    _untouched(net, lambda: net.ips_ragged_stream().feed([a, b]), TypeError, "dedup", monkeypatch, env={"IPSX_DEDUP_BLANK": "1"})


def test_positions_refuse_a_slide_that_passes_the_table(monkeypatch):
    net = rsc.make_net("image", "cpu")
    N = net.pos_enc.shape[1]
    a, b = rc.make_slides(rsc.conf_of("image"), (N, 20))
    s = net.ips_ragged_stream().feed([a[:N - 2], b])
    with pytest.raises(ValueError, match="slide 0 would have {} rows".format(N + 1)):
        s.feed([a[:3], b[:0]])
    s.feed([a[N - 2:], b[:0]])                   # exactly conf.N rows are taken
    assert s.fed == (N, 20)
    with pytest.raises(ValueError, match="a feed is"):
        net.ips_ragged_stream().feed([torch.zeros((4, 64)), torch.zeros((4, 64))])          # feature rows for an image net


def test_a_shuffling_net_is_not_refused_and_not_shuffled(nets):
    net, slides, want, _ = nets["feature"][False]
    net.shuffle = True
    rsc._seed()
    try:
        out = net.ips_ragged_stream().feed(slides).finish()
        got = rsc.record(net, out)
    finally:
        net.shuffle = False
    rc.assert_same_record(got, want)


def test_a_training_mode_net_is_restored(nets):
    net, slides, want, _ = nets["image"][False]
    net.train()
    try:
        s, out = rsc.run_schedule(net, slides, "feed_all", False)
        assert net.training and net.encoder.training and net.transf.training
    finally:
        net.eval()
    for key in ("mem_patch", "mem_idx"):
        assert torch.equal(rsc.record(net, out)[key], want[key])


def test_the_uniform_stream_and_the_sharded_call_still_refuse_a_ragged(nets):
    net, slides, _, _ = nets["feature"][False]
    r = Ragged.from_list(slides)
    with pytest.raises(TypeError, match="ips_ragged"):
        net.ips_stream().feed(r)
    with pytest.raises(TypeError, match="ips_ragged"):
        net.ips_stream().feed_rows(r)


# ------------------------------------------------------------------ the two exports: header, binding, argument checks
def test_header_declares_both_exports_inside_the_306_block():
    text = open(HEADER).read()
    assert re.search(r"#define\s+IPSX_VERSION\s+306\b", text)
    block = text[text.index("3.06  (additions only)"):text.index("#define IPSX_VERSION")]
    assert "ipsx_scan_ragged_spans" in block and "ipsx_stream_commit_ragged" in block
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+ipsx_scan_ragged_spans\s*\(", plain) and re.search(r"\bint\s+ipsx_stream_commit_ragged\s*\(", plain)
    assert "ipsx_scan_ragged_spans" in hip._EXPORTS and "ipsx_stream_commit_ragged" in hip._EXPORTS
    lib = hip.lib()
    assert lib.ipsx_version() == 306
    assert len(lib.ipsx_scan_ragged_spans.argtypes) == 15 and len(lib.ipsx_stream_commit_ragged.argtypes) == 9


def test_the_bindings_refuse_host_tensors():
    M, H, T = 4, 8, 1
    lg = torch.zeros((32, H * T))
    spans = torch.tensor([[0, 12], [12, 20]], dtype=torch.int64)
    with pytest.raises(ValueError, match="on the GPU"):
        hip.scan_ragged_spans(lg, spans, 20, M, M, H, T, torch.zeros((2, M), dtype=torch.int64), torch.zeros(2, dtype=torch.int32))
    t = torch.zeros((2, 8, 4))
    with pytest.raises(ValueError, match="on the GPU"):
        hip.stream_commit_ragged([(t, torch.zeros((5, 4)), t)], None, torch.zeros((2, 6), dtype=torch.int64), M, 3)


def test_the_native_entry_points_refuse_bad_arguments_before_any_launch():
    lib = hip.lib()
    buf = (C.c_char * 4096)()
    base = C.addressof(buf)
    one = hip.StreamTable()
    one.held, one.piece, one.dst = base, base + 2048, base + 1024
    one.held_rows, one.held_bstride_rows, one.dst_rows, one.dst_bstride_rows, one.row_bytes = 8, 8, 8, 8, 16
    tabs = (hip.StreamTable * 5)(*([one] * 5))
    slides = (C.c_int64 * 6)()
    sl = C.addressof(slides)

    def refused(rc_, what):
        assert rc_ != 0 and what in lib.ipsx_last_error().decode(), lib.ipsx_last_error()

    commit = lib.ipsx_stream_commit_ragged
    refused(commit(None, 1, None, sl, 1, 4, 4, 4, None), "null tables")
    refused(commit(tabs, 0, None, sl, 1, 4, 4, 4, None), "0 tables")
    refused(commit(tabs, 5, None, sl, 1, 4, 4, 4, None), "5 tables")
    refused(commit(tabs, 1, None, sl, 1, 0, 4, 4, None), "bad sizes")
    refused(commit(tabs, 1, None, sl, 0, 4, 4, 4, None), "bad sizes")
    refused(commit(tabs, 1, None, sl, 1, 4, -1, 4, None), "bad sizes")
    refused(commit(tabs, 1, None, None, 1, 4, 4, 4, None), "null slide table")
    refused(commit(tabs, 1, None, sl, 1, 4, 4, 0, None), "a piece of no rows")

    def with_(**kw):
        t = hip.StreamTable()
        C.memmove(C.addressof(t), C.addressof(one), C.sizeof(one))
        for k, v in kw.items():
            setattr(t, k, v)
        return (hip.StreamTable * 1)(t)

    refused(commit(with_(dst=None), 1, None, sl, 1, 4, 4, 4, None), "no destination")
    refused(commit(with_(row_bytes=0), 1, None, sl, 1, 4, 4, 4, None), "no destination")
    refused(commit(with_(held=None), 1, None, sl, 1, 4, 4, 4, None), "held rows are missing")
    refused(commit(with_(held_bstride_rows=4), 1, None, sl, 2, 4, 4, 4, None), "held rows are missing or overlap")
    refused(commit(with_(held_rows=0, piece=None), 1, None, sl, 1, 4, 4, 4, None), "neither held rows nor a piece")
    refused(commit(with_(piece_bstride_bytes=64), 1, None, sl, 1, 4, 4, 4, None), "one packed tensor")
    refused(commit(with_(dst_rows=0), 1, None, sl, 1, 4, 4, 4, None), "a destination of 0 rows")
    refused(commit(with_(dst_bstride_rows=4), 1, None, sl, 2, 4, 4, 4, None), "between the slides")
    refused(commit(with_(dst=base + 64), 1, None, sl, 1, 4, 4, 4, None), "overlaps the held rows")       # neither in place nor apart
    refused(commit(with_(piece=base + 1024 + 32), 1, None, sl, 1, 4, 4, 4, None), "overlaps the piece")
    refused(commit(with_(dst=base, piece=base + 64), 1, None, sl, 1, 4, 4, 4, None), "overlaps the piece")   # in place, the piece inside
    assert commit(tabs, 1, None, sl, 1, 4, 0, 4, None) == 0                                              # no rows: nothing to launch

    scan = lib.ipsx_scan_ragged_spans
    lg, idx = base, base + 2048
    refused(scan(None, sl, 1, 9, 64, 4, 4, 8, 1, idx, None, None, None, 0, None), "null pointer")
    refused(scan(lg, None, 1, 9, 64, 4, 4, 8, 1, idx, None, None, None, 0, None), "null pointer")
    refused(scan(lg, sl, 1, 9, 64, 4, 4, 8, 1, None, None, None, None, 0, None), "null pointer")
    refused(scan(lg, sl, 0, 9, 64, 4, 4, 8, 1, idx, None, None, None, 0, None), "bad sizes")
    refused(scan(lg, sl, 1, 9, 64, 4, 0, 8, 1, idx, None, None, None, 0, None), "bad sizes")
    refused(scan(lg, sl, 1, 4, 64, 4, 4, 8, 1, idx, None, None, None, 0, None), "than memory slots")
    refused(scan(lg, sl, 1, 65, 64, 4, 4, 8, 1, idx, None, None, None, 0, None), "a table of 64 rows")
    refused(scan(lg, sl, 1, 9, 1 << 31, 4, 4, 8, 1, idx, None, None, None, 0, None), "fewer than 2^31")
