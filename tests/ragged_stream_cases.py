"""What the tests of ``IPSNet.ips_ragged_stream`` share (tests/test_ragged_stream_cpu.py on the host,
tests/test_ragged_stream.py on the device): the nets, the slide lengths, the feeding schedules, and the record a stream
leaves behind in the form ``tests/ragged_cases.assert_same_record`` compares."""

import torch

from ips_amd import synth
from tests import ragged_cases as rc
from tests.stream_cases import piece_patterns

NETS = ("feature", "image", "feature_i12")


def conf_of(name):
    if name == "feature":
        return rc.feature_conf()
    if name == "image":
        return rc.image_conf()
    if name == "feature_i12":          # I != M
        return synth.camelyon_conf(N=256, M=16, I=12, n_chan_in=64, D=64, D_k=8, D_v=8, D_inner=128)
    if name == "feature_cam":          # scan_cam_kernel's shape
        return synth.camelyon_conf(N=1024, M=256, I=256, n_chan_in=64, D=64, D_k=8, D_v=8, D_inner=128)
    raise KeyError(name)


def make_net(name, device):
    net = rc.make_net(conf_of(name), device)
    net.shuffle = False
    return net


def lengths_of(M, I, pad):
    """A ragged last chunk; one candidate in the only chunk; chunks that end on the boundary; with ``pad`` a slide far
    below M rows and one of exactly M."""
    out = (M + 2 * I + I // 2 + 1, M + 1, M + 3 * I, M + I)
    return out + (5, M) if pad else out


PATTERNS = ("short_first", "ones", "long_first", "chunks3p5", "whole", "short_first")
SCHEDULES = ("mixed", "one_feed", "feed_all")


def mixed_schedule(lengths, M, I):
    """Feed k carries piece k of every slide's own pattern (``stream_cases.piece_patterns``, another pattern per slide): the
    slides end at different feeds and receive zero-length pieces afterwards -> [[n_b per slide] per feed]."""
    per_slide = [piece_patterns(n, M, I)[PATTERNS[b % len(PATTERNS)]] for b, n in enumerate(lengths)]
    feeds = max(len(p) for p in per_slide)
    return [[p[k] if k < len(p) else 0 for p in per_slide] for k in range(feeds)]


def pieces_of(slides, sizes):
    """The schedule ``sizes`` cut out of ``slides`` -> [[piece per slide] per feed] (views)."""
    lo = [0] * len(slides)
    out = []
    for feed in sizes:
        out.append([s[lo[b]:lo[b] + n] for b, (s, n) in enumerate(zip(slides, feed))])
        lo = [lo[b] + n for b, n in enumerate(feed)]
    assert lo == [s.shape[0] for s in slides]
    return out


def _seed(seed=11):
    """(nothing is drawn with ``shuffle`` off: the generators' states are compared as part of the record)"""
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


def run_schedule(net, slides, schedule, pad, device=None, after_feed=None):
    """A stream over ``slides`` by ``schedule`` -> the finished stream and (mem_patch, mem_pos).  ``device``: the pieces
    are moved there before they are fed; ``after_feed(stream, pieces)`` runs behind every feed."""
    M, I = net.M, net.I
    _seed()
    s = net.ips_ragged_stream(pad=pad)
    if schedule == "feed_all":
        src = slides if device is None else [t.to(device) for t in slides]
        assert s.feed_all(src, 37) is s              # (37 rows: slabs end inside slides)
    else:
        lengths = [t.shape[0] for t in slides]
        sizes = mixed_schedule(lengths, M, I) if schedule == "mixed" else [lengths]
        for pieces in pieces_of(slides, sizes):
            if device is not None:
                pieces = [p.to(device) for p in pieces]
            assert s.feed(pieces) is s
            if after_feed is not None:
                after_feed(s, pieces)
    assert s.fed == tuple(t.shape[0] for t in slides)
    return s, s.finish()


def record(net, out):
    p, q = out
    return {"mem_patch": rc._host(p), "mem_pos": rc._host(q), "mem_idx": rc._host(net.last_mem_idx), "mem_emb": rc._host(net.last_mem_emb),
            "shuffle": rc._host(net.last_shuffle), "rng": torch.get_rng_state(),
            "rng_cuda": torch.cuda.get_rng_state() if torch.cuda.is_available() else None}


def reference(net, slides, pad):
    """``net.ips_ragged(slides, pad=pad)`` -> (record, last_mem_count)."""
    _seed()
    out = net.ips_ragged(slides, pad=pad)
    return record(net, out), net.last_mem_count
