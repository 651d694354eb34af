"""The counted launch behind the blank scan as two launches (``ipsx_trunk_encode_parts_dedup``): whole rounds of the surviving
entries through eight-patch workgroups, the remainder through pair workgroups when the rule says so (``trunk_split_n8``,
ipsx_internal.h; read here through ``ipsx_dbg_trunk_split``).  Kernel level, for every survivor count at which the split can
go wrong and under the switch's three modes (0 the rule, 1 eight-patch workgroups only, 2 pair workgroups only): the embeddings
are bit for bit those of ``encode_indexed(..., parts=)`` on the same list, the sentinel rows either side are untouched, every
part's counter ends on the part's size and ``n_encoded`` is the survivor count.  Route level: ``IPSNet.ips`` selects the same
bits as under ``IPSX_DEDUP_BLANK=0`` on a batch with more than a round of survivors."""

import ctypes as C

import numpy as np
import pytest
import torch

from ips_amd import hip, synth
from ips_amd.architecture import IPSNet

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

_SHARED = {}
FULL, BLANK = 300, 100          # the pool: distinct non-blank patches, then all-zero rows


def plan():
    if "plan" not in _SHARED:
        net = synth.fill_weights(IPSNet(DEV, synth.mnist_conf(N=64, M=8, I=8)), 7).to(DEV).eval()
        p = hip.EncoderPlan(net.encoder, True)
        assert p.fused((1, 1, 32, 32))
        _SHARED["plan"] = p
    return _SHARED["plan"]


def pool():
    if "pool" not in _SHARED:
        g = np.random.default_rng(11)
        x = g.random((FULL + BLANK, 1, 32, 32), dtype=np.float32) + np.float32(1e-3)    # (no accidental zero)
        x[FULL:] = 0
        _SHARED["pool"] = torch.from_numpy(x).to(DEV)
    return _SHARED["pool"]


def units():
    return hip.device_geometry(DEV).cus


def split_entry():
    fn = hip.lib().ipsx_dbg_trunk_split
    fn.restype = C.c_longlong
    fn.argtypes = [C.c_longlong, C.c_int, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.c_int, C.POINTER(C.c_int)]
    return fn


def n8_of(count):
    return int(split_entry()(count, units(), 0, None, None, 0, None))


def thresholds():
    buf, n = (C.c_longlong * 64)(), C.c_int(0)
    split_entry()(0, units(), 0, None, buf, 64, C.byref(n))
    return [int(buf[k]) for k in range(n.value)]


def switch(mode):
    fn = hip.lib().ipsx_dbg_fused_trunk_pair
    fn.restype, fn.argtypes = None, [C.c_int]
    fn(mode)


def make_list(S, spread):
    """A list with S surviving entries (pool rows with repeats) and its part sizes.  Blank entries: none between the survivors,
    or - ``spread`` - 0, 3, 0, 1, ... behind each, so that the rows of one workgroup lie far apart; a run of nine in front of
    survivor n8 + 2 (or the middle one), which is a part of its own between two parts with survivors; five at the end.  The parts
    also end exactly between the last entry of the eight-patch workgroups and the first of the pair workgroups (in front of
    survivor n8, the rule's), between the two entries of the first pair (in front of survivor n8 + 1) and between the two of
    the last pair."""
    g = np.random.default_rng(S + 7 * spread)
    n8 = n8_of(S)
    numbers, pos, cuts = [], [], set()

    def blanks(k):
        numbers.extend((FULL + g.integers(0, BLANK, k)).tolist())

    run_at = n8 + 2 if n8 + 2 < S else S // 2                            # (no pair behind it: in the middle of the list)
    for s in range(S):
        if s == run_at:
            cuts.add(len(numbers))
            blanks(9)
            cuts.add(len(numbers))
        pos.append(len(numbers))
        numbers.append(int(g.integers(0, FULL)))
        if spread:
            blanks((0, 3, 0, 1)[s % 4])
    if S == 0:
        blanks(9)
        cuts.add(len(numbers))
    blanks(5)
    for s in (n8, n8 + 1):                                               # eight | pair, and inside the first pair
        if 0 < s < S:
            cuts.add(pos[s])
    if S - n8 >= 2 and (S - n8) % 2 == 0:                                # inside the last pair
        cuts.add(pos[S - 1])
    n = len(numbers)
    ends = sorted(c for c in cuts if 0 < c < n) + [n]
    assert len(ends) <= 16
    return np.asarray(numbers, dtype=np.int32), [b - a for a, b in zip([0] + ends, ends)], S


def check(numbers, sizes, survivors):
    p, x = plan(), pool()
    every = torch.as_tensor(numbers).to(DEV)
    n = every.numel()
    ends = list(np.cumsum(sizes).tolist())
    assert ends[-1] == n and int((numbers < FULL).sum()) == survivors
    done = torch.zeros((len(sizes),), dtype=torch.int32, device=DEV)
    want = p.encode_indexed(x, every, parts=(ends, done))                # the counted launch without dedup, once per list
    torch.cuda.synchronize()
    assert done.tolist() == list(sizes)
    try:
        for mode in (0, 1, 2):
            switch(mode)
            done.zero_()
            buf = torch.full((n + 2, 128), float("nan"), device=DEV)     # emb between two sentinel rows
            got = p.encode_source(hip.PatchSource(x), index=every, parts=(ends, done), dedup=True, out=buf[1:n + 1])
            torch.cuda.synchronize()
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), mode      # bit for bit
            assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[n + 1]).all()), mode
            assert done.tolist() == list(sizes), mode
            assert int(p.n_encoded.item()) == survivors, mode
    finally:
        switch(0)


def survivor_counts():
    """name -> count, from the device's round R = 8 units and the rule's thresholds t (a remainder of t goes one way, t + 1 the
    other)."""
    R = 8 * units()
    out = {"0": 0, "1": 1, "2": 2, "3": 3, "R": R, "R+1": R + 1, "R+2": R + 2, "R+3": R + 3}
    ts = thresholds()
    for k, t in enumerate(ts):
        for d in (-1, 0, 1):
            out["R+t%d%+d" % (k, d)] = R + t + d
    # a remainder that stays on the eight-patch kernel, with a partial last workgroup
    stay = [r for r in range(R - 3, 0, -1) if r % 8 == 5 and n8_of(R + r) == R + r]
    if stay:
        out["R+stay"] = R + stay[0]
    return out


COUNT_NAMES = ["0", "1", "2", "3", "R", "R+1", "R+2", "R+3", "R+t0-1", "R+t0+0", "R+t0+1", "R+stay"]


@pytest.mark.parametrize("spread", [False, True], ids=["dense", "spread"])
@pytest.mark.parametrize("name", COUNT_NAMES)
def test_survivor_counts_around_the_split(name, spread):
    counts = survivor_counts()
    assert len(thresholds()) == 1, "the rule has one threshold per round: a rule with more needs its counts listed here"
    assert name in counts, "the rule leaves no such remainder"
    check(*make_list(counts[name], spread))


def test_the_rule_sends_this_device_s_remainders_both_ways():
    """What the cases above rest on: below a round everything up to the threshold is the pair workgroups', one entry more is
    the eight-patch workgroups', and a whole round leaves the pair launch empty."""
    R = 8 * units()
    (t,) = thresholds()
    assert n8_of(3) == 0 and n8_of(t) == 0 and n8_of(t + 1) == t + 1
    assert n8_of(R) == R and n8_of(R + 1) == R and n8_of(R + t) == R and n8_of(R + t + 1) == R + t + 1


# ---------------------------------------------------------------------------------------------------- selection end to end
def test_ips_selects_the_same_bits_as_without_dedup_beyond_one_round(monkeypatch):
    """Eight images whose non-blank patches together are more than one round: the eight-patch launch encodes a whole round, the
    pair launch the rest, and the selection is that of the route without dedup."""
    R = 8 * units()
    conf0 = synth.mnist_conf(N=64)
    limit = IPSNet(DEV, conf0).selection.small_batch_limit(DEV)
    B = 8
    N = -(-limit // B) + 1                                               # the smallest batch that takes the one-launch route
    net = synth.fill_weights(IPSNet(DEV, synth.mnist_conf(N=N)), 7).to(DEV).eval()
    g = torch.Generator(device=DEV).manual_seed(21)
    x = torch.rand((B, N, 1, 32, 32), generator=g, device=DEV) + 1e-3
    keep = torch.rand((B, N, 1, 1, 1), generator=g, device=DEV) >= 0.92
    x = x * keep
    nonblank = int(keep.sum().item())
    assert R < nonblank < 2 * R and n8_of(nonblank) == R                 # one round and a pair remainder

    def call(dedup):
        if dedup is None:
            monkeypatch.delenv("IPSX_DEDUP_BLANK", raising=False)
        else:
            monkeypatch.setenv("IPSX_DEDUP_BLANK", dedup)
        net.selection.plan().n_encoded = None
        torch.manual_seed(3)
        mem_patch, mem_pos = net.ips(x)
        torch.cuda.synchronize()
        return net.last_mem_idx.clone(), mem_patch.clone(), mem_pos.clone(), net.last_mem_emb.clone()

    want = call("0")
    assert net.selection.plan().n_encoded is None                        # no dedup anywhere
    got = call(None)
    assert int(net.selection.plan().n_encoded.item()) == nonblank        # the two launches ran, and encoded these only
    assert all(torch.equal(s, t) for s, t in zip(got, want))
