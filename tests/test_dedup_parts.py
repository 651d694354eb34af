"""Exact blank-patch dedup inside the one counted launch (``ipsx_trunk_encode_parts_dedup``): a scan writes the blank
embedding to the rows of the all-zero list entries and counts them, an ordered compaction lists the others, and the trunk launch
encodes only those, each to its own row.  Kernel level: the embeddings are bit for bit those of ``ipsx_trunk_encode_parts`` on
the same lists, every part's counter ends on the part's size, and ``n_encoded`` is the number of non-blank entries.  Route
level: ``IPSNet.ips`` selects the same bits with ``IPSX_DEDUP_BLANK`` unset (the new route) as under ``IPSX_DEDUP_BLANK=0``."""

import itertools

import numpy as np
import pytest
import torch

from ips_amd import hip, synth
from ips_amd.architecture import IPSNet

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

_SHARED = {}
POOL = 1200                    # patches of a kernel-level pool
NEG_ZERO, LAST_ONLY, DENORMAL = 3, 4, 5        # pool rows that every pool carries, whatever its blank fraction


def plan():
    if "plan" not in _SHARED:
        net = synth.fill_weights(IPSNet(DEV, synth.mnist_conf(N=64, M=8, I=8)), 7).to(DEV).eval()
        p = hip.EncoderPlan(net.encoder, True)
        assert p.fused((1, 1, 32, 32))
        _SHARED["plan"] = (p, net)
    return _SHARED["plan"][0]


def pool(blank_frac):
    """(patches (POOL, 1, 32, 32) on the device, blank (POOL,) bool on the host): U[0, 1) patches, a seeded share of them all
    zero, and three special rows - all -0.0 (blank), only the LAST element non-zero (the early exit has read three KiB of
    zeros by then), only one float32 denormal, in the second KiB, non-zero."""
    key = ("pool", blank_frac)
    if key not in _SHARED:
        g = np.random.default_rng(int(blank_frac * 100) + 5)
        x = g.random((POOL, 1, 32, 32), dtype=np.float32) + np.float32(1e-3)        # (no accidental zero)
        blank = g.random(POOL) < blank_frac
        if blank_frac == 1:
            blank[:] = True
        x[blank] = 0
        x[NEG_ZERO] = -0.0
        x[LAST_ONLY] = 0
        x[LAST_ONLY, 0, 31, 31] = 0.5
        x[DENORMAL] = 0
        x.reshape(POOL, -1).view(np.uint32)[DENORMAL, 300] = 1                       # the smallest positive denormal
        blank[[NEG_ZERO, LAST_ONLY, DENORMAL]] = [True, False, False]
        _SHARED[key] = (torch.from_numpy(x).to(DEV), blank)
    return _SHARED[key]


def check(x, blank, numbers, sizes):
    """The list ``numbers`` (pool rows) cut into parts of ``sizes`` through both entries."""
    p = plan()
    every = torch.as_tensor(np.asarray(numbers, dtype=np.int32)).to(DEV)
    n = every.numel()
    assert sum(sizes) == n
    ends = list(itertools.accumulate(sizes))
    done = torch.zeros((len(sizes),), dtype=torch.int32, device=DEV)
    want = p.encode_indexed(x, every, parts=(ends, done))
    torch.cuda.synchronize()
    assert done.tolist() == list(sizes)
    done.zero_()
    buf = torch.full((n + 2, 128), float("nan"), device=DEV)             # emb between two sentinel rows
    got = p.encode_source(hip.PatchSource(x), index=every, parts=(ends, done), dedup=True, out=buf[1:n + 1])
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))    # bit for bit (-0.0 and +0.0 differ)
    assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[n + 1]).all())
    assert done.tolist() == list(sizes)
    assert int(p.n_encoded.item()) == int((~blank[np.asarray(numbers)]).sum())


@pytest.mark.parametrize("blank_frac", [0, 1, 0.5, 0.93])
@pytest.mark.parametrize("n,sizes", [(37, (37,)), (37, (20, 17)), (1100, (700, 300, 60, 40))], ids=["37", "37 in 2", "1100 in 4"])
def test_list_lengths_and_blank_fractions(n, sizes, blank_frac):
    """37: a compacted count that is no multiple of 8, one scan workgroup with a tail; 1,100: more than 1,024 entries, 18 scan
    workgroups, 5 compaction workgroups.  Each list begins with the three special rows."""
    x, blank = pool(blank_frac)
    check(x, blank, np.arange(n), sizes)


@pytest.mark.parametrize("n,sizes", [(37, (37,)), (37, (20, 17)), (1100, (700, 300, 60, 40))], ids=["37", "37 in 2", "1100 in 4"])
def test_lists_of_blank_rows_only(n, sizes):
    """Not one entry to encode: the compaction writes a count of 0, every workgroup of the trunk launch returns at once, the
    scan alone writes every row and fills every counter, and ``n_encoded`` is 0.  The rows are drawn, with repeats, from the
    blank rows of a pool (the all -0.0 row among them)."""
    x, blank = pool(0.93)
    rows = np.flatnonzero(blank)
    assert NEG_ZERO in rows
    numbers = rows[np.random.default_rng(n).integers(0, rows.size, n)]
    numbers[1] = NEG_ZERO
    assert not (~blank[numbers]).any()
    check(x, blank, numbers, sizes)
    assert int(plan().n_encoded.item()) == 0


@pytest.mark.parametrize("order", ["blank dense sparse", "dense blank sparse"])
@pytest.mark.parametrize("few", [1, 2])
def test_workgroups_that_straddle_parts(order, few):
    """Three parts: one without a non-blank entry, one without a blank one (6 entries), one of 9 with ``few`` non-blank ones.
    The trunk's first workgroup then holds entries of two parts, or of the first and the third with the empty one between."""
    x, blank = pool(0.5)
    zero = np.flatnonzero(blank)[:40]
    full = np.flatnonzero(~blank)[:40]
    parts = {"blank": zero[:5], "dense": full[:6], "sparse": np.concatenate([zero[5:9], full[6:6 + few], zero[9:14 - few]])}
    lists = [parts[k] for k in order.split()]
    check(x, blank, np.concatenate(lists), tuple(len(l) for l in lists))


def test_sixteen_parts():
    x, blank = pool(0.5)
    sizes = (1, 2, 9, 3, 17, 1, 8, 5, 4, 30, 2, 7, 11, 6, 1, 13)
    check(x, blank, np.arange(sum(sizes)), sizes)


@pytest.mark.parametrize("blank_frac", [0.5, 0.93])
def test_a_permuted_list_with_repeats(blank_frac):
    x, blank = pool(blank_frac)
    numbers = np.random.default_rng(3).permutation(POOL)[:300]
    numbers[10], numbers[200] = numbers[20], numbers[100]                # two rows twice
    numbers[:3] = [DENORMAL, NEG_ZERO, LAST_ONLY]
    check(x, blank, numbers, (130, 100, 70))


def test_refusals_launch_nothing():
    p = plan()
    x, _ = pool(0.5)
    every = torch.arange(24, dtype=torch.int32, device=DEV)
    done = torch.zeros((2,), dtype=torch.int32, device=DEV)
    buf = torch.full((24, 128), float("nan"), device=DEV)
    assert p.fused(x.shape)
    p.trunk.precision = 1
    try:
        with pytest.raises(Exception):
            p.encode_source(hip.PatchSource(x), index=every, parts=([8, 24], done), dedup=True, out=buf)
    finally:
        p.trunk.precision = 0
    with pytest.raises(Exception):
        p.encode_source(hip.PatchSource(x), index=every, parts=([8, 16], done), dedup=True, out=buf)     # ends short of the list
    # what only the trunk launch would refuse - its 128 -> 128 convolutions' tile16 packing missing - is refused before the scan
    p.blank_embedding(hip.PatchSource(x))                                 # (made while the plan is whole)
    conv = p.trunk.blocks[3].conv[1]
    kept = conv.w_packed_bf16
    conv.w_packed_bf16 = None
    try:
        with pytest.raises(Exception):
            p.encode_source(hip.PatchSource(x), index=every, parts=([8, 24], done), dedup=True, out=buf)
    finally:
        conv.w_packed_bf16 = kept
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all()) and not bool(done.any())


# ---------------------------------------------------------------------------------------------------- selection end to end
def route_case(shuffle, blank_frac):
    """(net, x): the smallest batch of 16 images that takes the one-launch route on this device (``small_batch_limit``)."""
    if ("net", shuffle) not in _SHARED:
        conf0 = synth.mnist_conf(N=64, shuffle=shuffle, shuffle_style="instance")
        probe = IPSNet(DEV, conf0)
        N = -(-probe.selection.small_batch_limit(DEV) // 16) + 1
        net = synth.fill_weights(IPSNet(DEV, synth.mnist_conf(N=N, shuffle=shuffle, shuffle_style="instance")), 7).to(DEV).eval()
        _SHARED[("net", shuffle)] = (net, N)
    net, N = _SHARED[("net", shuffle)]
    if ("x", blank_frac) not in _SHARED:
        g = torch.Generator(device=DEV).manual_seed(12)
        x = torch.rand((16, N, 1, 32, 32), generator=g, device=DEV) + 1e-3
        keep = torch.rand((16, N, 1, 1, 1), generator=g, device=DEV) >= blank_frac
        _SHARED[("x", blank_frac)] = (x * keep, int(keep.sum().item()))
    return (net,) + _SHARED[("x", blank_frac)]


def call(net, x, monkeypatch, dedup, seed=3):
    if dedup is None:
        monkeypatch.delenv("IPSX_DEDUP_BLANK", raising=False)
    else:
        monkeypatch.setenv("IPSX_DEDUP_BLANK", dedup)
    net.selection.plan().n_encoded = None
    torch.manual_seed(seed)
    mem_patch, mem_pos = net.ips(x)
    torch.cuda.synchronize()
    return net.last_mem_idx.clone(), mem_patch.clone(), mem_pos.clone(), net.last_mem_emb.clone()


def same(a, b):
    return all(torch.equal(s, t) for s, t in zip(a, b))


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("blank_frac", [0.93, 0])
def test_ips_selects_the_same_bits_as_without_dedup(blank_frac, shuffle, monkeypatch):
    net, x, nonblank = route_case(shuffle, blank_frac)
    assert x.shape[0] * x.shape[1] >= net.selection.small_batch_limit(DEV)
    want = call(net, x, monkeypatch, "0")
    assert net.selection.plan().n_encoded is None                        # no dedup anywhere
    got = call(net, x, monkeypatch, None)
    assert int(net.selection.plan().n_encoded.item()) == nonblank        # the new route ran, and encoded these only
    again = call(net, x, monkeypatch, None)                              # (cached buffers, counters zeroed again)
    assert same(got, want) and same(again, want)
    assert same(call(net, x, monkeypatch, "auto"), want)


def test_a_weight_change_renews_the_blank_embedding(monkeypatch):
    net, x, nonblank = route_case(False, 0.93)
    first = call(net, x, monkeypatch, None)
    p = net.selection.plan()
    before = p.blank_emb.clone()
    bn = next(m for m in net.encoder.modules() if isinstance(m, torch.nn.BatchNorm2d))
    kept = bn.bias.detach().clone()
    try:
        with torch.no_grad():
            bn.bias.add_(0.25)                                           # (in place: the version counter moves)
        want = call(net, x, monkeypatch, "0")
        got = call(net, x, monkeypatch, None)
        assert same(got, want)
        assert not torch.equal(p.blank_emb, before)
        assert not torch.equal(got[3], first[3])                         # (the change is one the selection's output shows)
    finally:
        with torch.no_grad():
            bn.bias.copy_(kept)
    assert same(call(net, x, monkeypatch, None), first)
