"""Every part of an ``ips()`` call through the fused fp32 trunk as ONE launch (``ipsx_trunk_encode_parts``): the embeddings are
bit for bit those of the per-part launches, the launch counts each part's patches into its counter, a one-wave kernel
(``ipsx_part_wait``) holds another stream until a part is complete - bounded, with a status bit when it gives up - and the
conditional redo behind it (``ipsx_logits_if`` + ``ipsx_scan_range_if``) repairs a call whose wait gave up.  ``IPSNet.ips``
selects the same bits on the one-launch route (``IPSX_ONE_LAUNCH``, default on) as on the per-part launches."""

import ctypes as C
import itertools

import pytest
import torch

from ips_amd import hip, synth
from ips_amd.architecture import IPSNet
from ips_amd.selection import Selection

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

_SHARED = {}


def trunk():
    """(plan, patches): the MNIST net's encoder with seeded weights and 64 seeded patches - made once."""
    if "trunk" not in _SHARED:
        net = synth.fill_weights(IPSNet(DEV, synth.mnist_conf(N=64, M=8, I=8)), 7).to(DEV).eval()
        g = torch.Generator().manual_seed(11)
        x = torch.rand((64, 1, 32, 32), generator=g).to(DEV)
        plan = hip.EncoderPlan(net.encoder, True)
        assert plan.fused(x.shape)                                        # (also tells the trunk its patch size)
        _SHARED["trunk"] = (plan, x, net)
    return _SHARED["trunk"][:2]


def raw_parts(plan, x, every, ends, done, emb):
    """The entry itself, on a caller's buffers -> its return code."""
    assert plan.fused(x.shape)
    return hip.lib().ipsx_trunk_encode_parts(C.byref(plan.trunk), hip._p(x), hip._p(every), every.numel(), hip._p(emb),
                                             (C.c_int64 * len(ends))(*ends), len(ends), hip._p(done), hip._stream())


def lists_of(sizes, numbers=None):
    numbers = torch.arange(sum(sizes), dtype=torch.int32) if numbers is None else numbers
    out, at = [], 0
    for s in sizes:
        out.append(numbers[at:at + s].to(DEV))
        at += s
    return out


PERMUTED = torch.tensor([13, 2, 40, 7, 63, 0, 21, 7, 33, 58, 5, 19, 40, 1, 62, 9, 27, 3, 50, 11], dtype=torch.int32)   # 7 and 40 twice

CASES = [((8, 8, 8), None),          # edges aligned to workgroups
         ((3, 13, 8), None),         # a workgroup straddling one edge
         ((1, 1, 22), None),         # parts smaller than a workgroup, three parts in one workgroup
         ((5,), None),               # a single short workgroup
         ((17, 9, 7, 4), None),      # P = 4, n not a multiple of 8
         ((7, 13), PERMUTED)]        # a permuted list with repeated patch numbers


@pytest.mark.parametrize("sizes,numbers", CASES, ids=[str(c[0]) + ("" if c[1] is None else " permuted") for c in CASES])
def test_one_launch_equals_the_per_part_launches_and_counts_every_part(sizes, numbers):
    plan, x = trunk()
    lists = lists_of(sizes, numbers)
    every = torch.cat(lists)
    n = every.numel()
    ends = list(itertools.accumulate(sizes))
    want = torch.cat([plan.encode_indexed(x, l) for l in lists])
    buf = torch.full((n + 2, 128), float("nan"), device=DEV)             # emb between two sentinel rows
    done = torch.zeros((len(sizes),), dtype=torch.int32, device=DEV)
    assert raw_parts(plan, x, every, ends, done, buf[1:n + 1]) == 0, hip.lib().ipsx_last_error()
    torch.cuda.synchronize()
    assert torch.equal(buf[1:n + 1], want)
    assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[n + 1]).all())
    assert done.tolist() == list(sizes)
    # and through the plan's method, the way the selection calls it
    done.zero_()
    assert torch.equal(plan.encode_indexed(x, every, parts=(ends, done)), want)
    assert done.tolist() == list(sizes)


def test_rejected_arguments_launch_nothing():
    plan, x = trunk()
    every = torch.arange(24, dtype=torch.int32, device=DEV)
    buf = torch.full((24, 128), float("nan"), device=DEV)
    done = torch.zeros((17,), dtype=torch.int32, device=DEV)

    def refused(ends):
        rc = raw_parts(plan, x, every, ends, done, buf)
        torch.cuda.synchronize()
        return rc != 0 and bool(torch.isnan(buf).all()) and not bool(done.any())

    assert plan.fused(x.shape)
    plan.trunk.precision = 1                                              # bf16
    try:
        assert refused([8, 24])
    finally:
        plan.trunk.precision = 0
    assert refused(list(range(1, 17)) + [24])                             # P = 17
    assert refused([8, 8, 24]) and refused([16, 8, 24])                   # part_end does not increase
    assert refused([8, 16])                                               # does not end on the list's length
    assert raw_parts(plan, x, every, [8, 24], done, buf) == 0             # (the same buffers are fine otherwise)
    torch.cuda.synchronize()
    assert done[:2].tolist() == [8, 16] and not bool(torch.isnan(buf).any())


# ---------------------------------------------------------------------------------------------------- the wait kernel
def test_wait_returns_at_once_on_a_full_counter():
    words = torch.tensor([5, 0], dtype=torch.int32, device=DEV)
    hip.part_wait(words[0:1], 5, words[1:2], 1)
    torch.cuda.synchronize()
    assert words.tolist() == [5, 0]


def timed_wait(bound_ms, bit):
    """A wait on a counter nobody advances, under a bound of ``bound_ms`` -> (device milliseconds, [counter, status])."""
    words = torch.zeros((2,), dtype=torch.int32, device=DEV)
    before = hip.persistent_wait_ms(bound_ms)
    try:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        hip.part_wait(words[0:1], 5, words[1:2], bit)
        e1.record()
        torch.cuda.synchronize()
    finally:
        hip.persistent_wait_ms(before)
    assert hip.persistent_wait_ms(0) == before
    return e0.elapsed_time(e1), words.tolist()


def test_wait_gives_up_within_its_bound_and_says_so():
    """Nobody advances the counter: the kernel sets its bit and ends when the bound has passed without progress - timed on
    the device around a warmed launch.  It follows ``ipsx_set_persistent_wait_ms``: under 1 ms it takes at least 1 ms and a
    few at most (not the default's 50), under 8 ms at least 8 - nothing is left running either way."""
    test_wait_returns_at_once_on_a_full_counter()                         # (the launch path is warm)
    t1, words = timed_wait(1, 4)
    assert words == [0, 4]
    assert 1.0 <= t1 < 4.0, t1
    t8, words = timed_wait(8, 2)
    assert words == [0, 2]
    assert 8.0 <= t8 < 11.0, t8


# ---------------------------------------------------------------------------------------------------- selection end to end
def ips_net(shuffle):
    key = ("net", shuffle)
    if key not in _SHARED:
        conf = synth.mnist_conf(N=200, M=16, I=16, shuffle=shuffle, shuffle_style="instance")
        net = synth.fill_weights(IPSNet(DEV, conf), 7).to(DEV).eval()
        g = torch.Generator().manual_seed(12)
        _SHARED[key] = (net, torch.rand((16, 200, 1, 32, 32), generator=g).to(DEV))
    return _SHARED[key]


def call(net, x, monkeypatch, one_launch, seed=3):
    monkeypatch.setenv("IPSX_ONE_LAUNCH", one_launch)
    torch.manual_seed(seed)
    mem_patch, mem_pos = net.ips(x)
    torch.cuda.synchronize()
    return mem_patch.clone(), mem_pos.clone(), net.last_mem_idx.clone()


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("B", [2, 16])
def test_ips_selects_the_same_bits_on_both_routes(B, shuffle, monkeypatch):
    """N = 200, M = I = 16: 12 iterations in 4 parts (rows 112 | 64 | 16 | 8 of every image).  These batches are far below
    the small-batch limit, which is lifted here so that they take the parts' route."""
    monkeypatch.setattr(Selection, "small_batch_limit", lambda self, dev: 0)
    net, x = ips_net(shuffle)
    x = x[:B].contiguous()
    launches = []
    plan = net.selection.plan()
    inner = plan.encode_source
    monkeypatch.setattr(plan, "encode_source", lambda *a, **kw: (launches.append(kw.get("parts")), inner(*a, **kw))[1], raising=False)
    index_calls = net.selection.index_calls
    want = call(net, x, monkeypatch, "0")
    assert len(launches) == 4 and not any(launches)
    del launches[:]
    got = call(net, x, monkeypatch, "1")
    again = call(net, x, monkeypatch, "1")                                # (cached buffers, counters zeroed again)
    assert len(launches) == 2 and all(p is not None and len(p[0]) == 4 for p in launches)
    assert net.selection.index_calls - index_calls == (3 if shuffle else 0)
    for r in (got, again):
        for a, b in zip(r, want):
            assert torch.equal(a, b)
    assert [tuple(e.shape[:2]) for e in net._emb_parts] == [(B, 112), (B, 64), (B, 16), (B, 8)]


def test_default_route_is_one_trunk_launch_per_call(monkeypatch):
    monkeypatch.setattr(Selection, "small_batch_limit", lambda self, dev: 0)
    monkeypatch.delenv("IPSX_ONE_LAUNCH", raising=False)
    net, x = ips_net(False)
    assert hip.persistent_ok(DEV)
    counts = {"trunk": 0, "wait": 0}
    plan = net.selection.plan()
    inner, inner_wait = plan.encode_source, hip.part_wait

    def encode(*a, **kw):
        counts["trunk"] += 1
        return inner(*a, **kw)

    def wait(*a, **kw):
        counts["wait"] += 1
        return inner_wait(*a, **kw)

    monkeypatch.setattr(plan, "encode_source", encode, raising=False)
    monkeypatch.setattr(hip, "part_wait", wait)
    net.ips(x)
    assert counts == {"trunk": 1, "wait": 3}
    monkeypatch.setenv("IPSX_ONE_LAUNCH", "0")
    counts.update(trunk=0, wait=0)
    net.ips(x)
    assert counts == {"trunk": 4, "wait": 0}
    torch.cuda.synchronize()


def test_conditional_redo_repairs_a_call_whose_wait_gave_up(monkeypatch):
    """The per-part route's indices; then what the one-launch route holds when a wait gave up - finished embeddings, logits
    and memory indices that cannot be trusted, the status bit set (by hand here) - through the conditional launches."""
    monkeypatch.setattr(Selection, "small_batch_limit", lambda self, dev: 0)
    net, x = ips_net(False)
    B, N, M, I = 16, 200, 16, 16
    want = call(net, x, monkeypatch, "0")[2]
    ca = net.transf.crs_attn
    vq, R = ca.folded_query(), ca.H * ca.n_token
    edges = [0, 112, 176, 192, 200]
    ends = Selection.part_ends(B, edges)
    every = torch.cat(Selection.part_lists(B, N, edges, DEV))
    words = torch.zeros((8,), dtype=torch.int32, device=DEV)
    done, status = words[:4], words[4:5]
    emb = net.selection.plan().encode_indexed(x.reshape(B * N, 1, 32, 32), every, parts=(ends, done))
    pos_all = net.pos_enc.expand(B, -1, -1)                              # (no shuffle: the rows ips() scores with)
    tie = torch.zeros((B,), dtype=torch.int32, device=DEV)

    def redo(bit):
        status.fill_(bit)
        logits = torch.full((B, N, R), 1e30, device=DEV)
        mem = torch.full((B, M), -1, dtype=torch.int64, device=DEV)
        starts = [0] + ends[:-1]
        for k in range(4):
            part = emb[starts[k]:ends[k]].view(B, edges[k + 1] - edges[k], -1)
            hip.logits(part, pos_all[:, edges[k]:edges[k + 1]], vq, R, out=logits[:, edges[k]:edges[k + 1]], cond=status)
        hip.scan_range_if(logits, M, I, ca.H, ca.n_token, 0, 12, mem, tie, status, 1)
        torch.cuda.synchronize()
        return logits, mem

    logits, mem = redo(0)                                                # no bit: every launch returns at once
    assert bool((logits == 1e30).all()) and bool((mem == -1).all())
    logits, mem = redo(1)
    assert torch.equal(mem, want)



def test_a_call_whose_waits_gave_up_is_redone_in_the_call(monkeypatch):
    """``Selection.parts_one_launch`` itself with every wait giving up at once (``hip.part_wait`` replaced by a launch that
    only sets the status bit): the parts' logits and iterations then run on the side stream while the trunk launch has
    hardly begun, and the conditional launches at the end of the call must leave the per-part route's bits.  The host sees
    the word one call later and counts the event as the persistent pipelines do."""
    monkeypatch.setattr(Selection, "small_batch_limit", lambda self, dev: 0)
    net, x = ips_net(False)
    want = call(net, x, monkeypatch, "0")
    good = call(net, x, monkeypatch, "1")                                 # (buffers of the route exist; mirror clean)
    events, forced = [], []

    def gave_up(done, want_count, status, bit=1):
        forced.append(want_count)
        status.bitwise_or_(bit)                                           # (on the side stream, where the wait would run)

    monkeypatch.setattr(hip, "part_wait", gave_up)
    monkeypatch.setattr(hip, "persistent_timed_out", lambda dev: events.append(dev) or True)
    calls = hip._PERSIST_CALLS
    got = call(net, x, monkeypatch, "1")
    assert forced == [16 * 112, 16 * 64, 16 * 16] and events == []
    for a, b, c in zip(got, want, good):
        assert torch.equal(a, b) and torch.equal(c, b)
    assert int(net.selection.scan_status_host.item()) & 1                 # mirrored behind the call
    monkeypatch.undo()                                                    # (the real wait kernel again)
    monkeypatch.setattr(Selection, "small_batch_limit", lambda self, dev: 0)
    monkeypatch.setattr(hip, "persistent_timed_out", lambda dev: events.append(dev) or True)
    again = call(net, x, monkeypatch, "1")
    assert len(events) == 1 and hip._PERSIST_CALLS == calls + 2
    assert int(net.selection.scan_status_host.item()) == 0
    for a, b in zip(again, want):
        assert torch.equal(a, b)
