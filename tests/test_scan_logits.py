"""scan_mnist_kernel with the logits prologue (``hip.LogitsParts.scan_range``, csrc/scan_mnist.hip): a range of the selection loop
whose launch computes its own logits, against the launches it replaces - ``logits_kernel<1>`` per part, then the loop's range,
then the conditional redo - which the SAME entry point enqueues with the switch off (``hip.dbg_scan_logits(False)``).
Everything is compared bit for bit: the whole logits table, ``mem_idx`` after every range, the tie flags; and through
``net.ips()`` what the call returns and leaves.

H = 8, 4 tokens, M = I = 64, D = 128 (the kernel's one shape).  Parts are lists of rows per image; a launch takes a run of
whole parts and the iterations whose rows end inside them."""

import numpy as np
import pytest
import torch

from ips_amd import hip, synth
from ips_amd.architecture import IPSNet
from ips_amd.selection import Selection

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M = I = 64
H, T, D, DK = 8, 4, 128, 16
R = H * T

# name -> (rows of every part, launches as (first part, end part, first iteration, end iteration))
PLANS = {
    # N = 64 + 2 * 64 + 17: a ragged last chunk of 17 rows, and a part of 17 rows (no multiple of 32)
    "ragged": ([192, 17], [(0, 1, 0, 2), (1, 2, 2, 3)]),
    # N = 64 + 5 * 64 in 2, 3 and 4 parts; "3": a part of ONE chunk; "4": a part of 20 rows (below a tile of 32), a launch of two
    # parts, part edges off the chunk boundaries
    "2": ([256, 128], [(0, 1, 0, 3), (1, 2, 3, 5)]),
    "3": ([128, 64, 192], [(0, 1, 0, 1), (1, 2, 1, 2), (2, 3, 2, 5)]),
    "4": ([128, 20, 108, 128], [(0, 1, 0, 1), (1, 3, 1, 3), (3, 4, 3, 5)]),
    # N = 64 + 11 * 64: a part of 717 rows - two rounds of the workgroup's 16 tiles, the second ragged (717 = 22 * 32 + 13) - which
    # the redo recomputes together with the 51 rows behind it
    "big": ([717, 51], [(0, 1, 0, 10), (1, 2, 10, 11)]),
}
_VQ = {}


def folded_query():
    if "vq" not in _VQ:
        g = torch.Generator().manual_seed(11)
        qs = (torch.randn((T, H * DK), generator=g) * 0.5).to(DEV)
        wk = (torch.randn((H * DK, D), generator=g) * 0.3).to(DEV)
        _VQ["vq"] = hip.fold_query(qs, wk, H, DK, T)
    return _VQ["vq"]


def inputs(B, rows, pos_kind, seed, tie=False):
    """The parts' embeddings (part-major, as a counted trunk launch leaves them) and the positional rows of whole images."""
    g = torch.Generator().manual_seed(seed)
    N = sum(rows)
    emb = torch.randn((B, N, D), generator=g)
    if tie:
        emb[0, :] = emb[0, 0]                       # image 0: every row the same - every score ties, in every iteration
        if B > 1:
            emb[1, 70:100] = emb[1, 10:40]          # image 1: a stretch of rows again, memory against chunk
    pos = None
    if pos_kind == "shared":
        pos = (torch.randn((1, N, D), generator=g) * 0.5).to(DEV)
    elif pos_kind == "own":
        pos = (torch.randn((B, N, D), generator=g) * 0.5).to(DEV)
    edges = np.concatenate([[0], np.cumsum(rows)])
    embs = [emb[:, edges[k]:edges[k + 1]].contiguous().to(DEV) for k in range(len(rows))]
    return embs, pos


def run(embs, pos, launches, one_launch, redo=None, garbage_until=0):
    """The launches of a plan -> (logits table, mem_idx after every launch, tie flags).  ``redo``: a status word for the LAST
    launch; ``garbage_until``: the launches before that one read other embeddings (rows that 'were not there yet')."""
    B, N = embs[0].shape[0], sum(e.shape[1] for e in embs)
    logits = torch.full((B, N, R), float("nan"), device=DEV)
    mem = torch.full((B, M), -7, dtype=torch.int64, device=DEV)
    tie = torch.zeros((B,), dtype=torch.int32, device=DEV)
    good = hip.LogitsParts(embs)
    early = good
    if garbage_until:
        g = torch.Generator().manual_seed(5)
        early = hip.LogitsParts([torch.randn(tuple(e.shape), generator=g).to(DEV) for e in embs])
    was = hip.dbg_scan_logits(one_launch)
    mems = []
    try:
        for n, (p0, p1, it0, it1) in enumerate(launches):
            last = n == len(launches) - 1
            (early if n < garbage_until else good).scan_range(logits, M, I, H, T, it0, it1, mem, tie, p0, p1, pos, folded_query(),
                                                              redo=redo if last else None)
            mems.append(mem.clone())
        torch.cuda.synchronize()
    finally:
        hip.dbg_scan_logits(was)
    return logits, mems, tie


def same(a, b, what):
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)), what + ": the logits table"
    for n, (x, y) in enumerate(zip(a[1], b[1])):
        assert torch.equal(x, y), "%s: mem_idx after launch %d" % (what, n)
    assert torch.equal(a[2], b[2]), what + ": tie flags"


def test_the_switch_reports_and_restores():
    assert hip.scan_logits_on()
    assert hip.dbg_scan_logits(False) is True and not hip.scan_logits_on()
    assert hip.dbg_scan_logits(True) is False and hip.scan_logits_on()


@pytest.mark.parametrize("pos_kind", ["none", "shared", "own"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("plan", sorted(PLANS))
def test_ranges_with_their_own_logits_leave_the_two_launch_bits(plan, B, pos_kind):
    """Every plan, one image and three, without / with one / with per-image positional rows: the whole table (every row is
    written by exactly one launch - no NaN of the fill is left), mem_idx after every range (ranges 2.. resume from it)."""
    rows, launches = PLANS[plan]
    embs, pos = inputs(B, rows, pos_kind, 100 + B)
    want = run(embs, pos, launches, False)
    got = run(embs, pos, launches, True)
    assert not bool(torch.isnan(want[0]).any())
    same(got, want, "%s B=%d pos=%s" % (plan, B, pos_kind))
    assert int(want[2].sum()) == 0                                      # (continuous inputs: no tie)


@pytest.mark.parametrize("B", [1, 3])
def test_a_range_resumed_from_the_other_routes_memory(B):
    """The first ranges by the two-launch route, the last by the one launch (and the other way round): the state a range
    resumes from is mem_idx and the table's earlier rows alone."""
    rows, launches = PLANS["3"]
    embs, pos = inputs(B, rows, "own", 300 + B)
    want = run(embs, pos, launches, False)
    parts = hip.LogitsParts(embs)
    for first_one_launch in (False, True):
        logits = torch.full((B, sum(rows), R), float("nan"), device=DEV)
        mem = torch.full((B, M), -7, dtype=torch.int64, device=DEV)
        tie = torch.zeros((B,), dtype=torch.int32, device=DEV)
        try:
            for n, (p0, p1, it0, it1) in enumerate(launches):
                hip.dbg_scan_logits(first_one_launch if n < 2 else not first_one_launch)
                parts.scan_range(logits, M, I, H, T, it0, it1, mem, tie, p0, p1, pos, folded_query())
        finally:
            hip.dbg_scan_logits(True)
        same((logits, [mem], tie), (want[0], [want[1][-1]], want[2]), "mixed routes")


@pytest.mark.parametrize("B", [1, 3])
def test_ties_forced_by_duplicate_rows(B):
    """Image 0: all rows equal (every iteration ties at the memory's boundary: the flag is set, torch.topk's order is
    replayed); image 1: a duplicated stretch.  Flags and indices as the two launches leave them."""
    rows, launches = PLANS["4"]
    embs, pos = inputs(B, rows, "none", 400 + B, tie=True)
    want = run(embs, pos, launches, False)
    got = run(embs, pos, launches, True)
    assert int(want[2][0]) == 1, "the inputs were meant to tie"
    same(got, want, "ties B=%d" % B)


@pytest.mark.parametrize("pos_kind", ["none", "own"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("plan", ["ragged", "3", "4", "big"])
def test_the_status_word_set_before_the_last_launch_redoes_the_call(plan, B, pos_kind):
    """The early launches read OTHER embeddings (a wait that gave up: the rows were not there yet), the status word is set by
    hand, the last launch finds every embedding in place: it must recompute every row and run the loop from iteration 0 -
    the clean call's bits, on both routes.  With the word clear the same launch is the plain one."""
    rows, launches = PLANS[plan]
    embs, pos = inputs(B, rows, pos_kind, 500 + B)
    clean = run(embs, pos, launches, False)
    word = torch.zeros((2,), dtype=torch.int32, device=DEV)
    same(run(embs, pos, launches, True, redo=word[0:1]), clean, "status clear")
    word[1] = 1
    for one_launch in (False, True):
        got = run(embs, pos, launches, one_launch, redo=word[1:2], garbage_until=len(launches) - 1)
        same((got[0], [got[1][-1]], got[2]), (clean[0], [clean[1][-1]], clean[2]), "redo, one launch: %s" % one_launch)
        assert not torch.equal(got[1][0], clean[1][0]), "the early launches were meant to go wrong"


@pytest.mark.parametrize("word", [0, 1])
def test_a_launch_with_no_part_of_its_own_carries_the_redo(word):
    """A long last part: its logits by ``hip.logits``, then the loop's launch with part_begin == part_end and the status word.
    Clear: the plain range on the rows that are there.  Set (the earlier launch read other embeddings): all 717 + 51 rows
    again - three rounds of tiles by one workgroup per image - and the loop from iteration 0: the clean call's bits."""
    rows, launches = PLANS["big"]
    B = 3
    embs, pos = inputs(B, rows, "own", 700)
    clean = run(embs, pos, launches, False)
    g = torch.Generator().manual_seed(5)
    early = hip.LogitsParts([torch.randn(tuple(e.shape), generator=g).to(DEV) for e in embs]) if word else hip.LogitsParts(embs)
    good = hip.LogitsParts(embs)
    logits = torch.full((B, sum(rows), R), float("nan"), device=DEV)
    mem = torch.full((B, M), -7, dtype=torch.int64, device=DEV)
    tie = torch.zeros((B,), dtype=torch.int32, device=DEV)
    status = torch.tensor([word], dtype=torch.int32, device=DEV)
    early.scan_range(logits, M, I, H, T, 0, 10, mem, tie, 0, 1, pos, folded_query())
    hip.logits(embs[1], pos[:, rows[0]:], folded_query(), R, out=logits[:, rows[0]:])
    good.scan_range(logits, M, I, H, T, 10, 11, mem, tie, 2, 2, pos, folded_query(), redo=status)
    torch.cuda.synchronize()
    same((logits, [mem], tie), (clean[0], [clean[1][-1]], clean[2]), "status word %d" % word)


def test_arguments_the_kernel_does_not_take_are_refused():
    rows, launches = PLANS["2"]
    embs, pos = inputs(1, rows, "none", 1)
    parts = hip.LogitsParts(embs)
    logits = torch.empty((1, sum(rows), R), device=DEV)
    mem = torch.empty((1, M), dtype=torch.int64, device=DEV)
    tie = torch.zeros((1,), dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="read rows up to"):          # iterations beyond the launch's parts
        parts.scan_range(logits, M, I, H, T, 0, 5, mem, tie, 0, 1, None, folded_query())
    with pytest.raises(RuntimeError, match="outside the loop"):
        parts.scan_range(logits, M, I, H, T, 3, 6, mem, tie, 1, 2, None, folded_query())
    lg16 = torch.empty((1, sum(rows), 8), device=DEV)
    with pytest.raises((RuntimeError, ValueError)):                     # another shape: no such kernel, and no fall-back
        parts.scan_range(lg16, 16, 16, 8, 1, 0, 1, torch.empty((1, 16), dtype=torch.int64, device=DEV), tie, 0, 1, None, folded_query())


# ---------------------------------------------------------------------------------------------------- through net.ips()
def _ips(net, x, one_launch, calls):
    was = hip.dbg_scan_logits(one_launch)
    try:
        n0 = len(calls)
        mem_patch, mem_pos = net.ips(x)
        out = (mem_patch.clone(), mem_pos.clone(), net.last_mem_idx.clone(), net.last_mem_emb.clone())
        torch.cuda.synchronize()
    finally:
        hip.dbg_scan_logits(was)
    return out, len(calls) - n0


@pytest.mark.parametrize("limit", [1 << 30, 100], ids=["every part in the loop's launch", "parts above 100 rows get a logits launch"])
@pytest.mark.parametrize("N, parts", [(320, 2), (64 + 8 * 64 + 17, 4)])
def test_ips_on_a_counted_deduped_batch_returns_the_same_bits(N, parts, limit, monkeypatch):
    """16 images of 320 patches, most of them blank, through ``net.ips()``: the counted, deduped route (the small-batch limit
    is lifted, and - 320 patches are 4 iterations - the route's parts are set to 2 so that it cuts them) with the loop
    computing its logits against the same route with logits launches: what the call returns, ``last_mem_idx`` and
    ``last_mem_emb``, twice (the second call on the cached buffers).  593 patches: the route's own four parts.  With
    ``IPSX_SCAN_LOGITS_ROWS=100`` all parts but the last (17 rows at 593 patches) are "long": a logits launch, then the
    loop's launch with no rows of its own."""
    monkeypatch.setattr(Selection, "SCAN_LOGITS_ROWS", limit)
    monkeypatch.setattr(Selection, "small_batch_limit", lambda self, dev: 0)
    monkeypatch.setattr(Selection, "OVERLAP_PARTS", parts)
    calls = []
    inner = hip.LogitsParts.scan_range
    monkeypatch.setattr(hip.LogitsParts, "scan_range", lambda *a, **kw: (calls.append(a[10:12]), inner(*a, **kw))[1])
    conf = synth.mnist_conf(N=N, M=M, I=I)
    net = synth.fill_weights(IPSNet(torch.device(DEV), conf), 3).to(DEV).eval()
    x = synth.make_patches(conf, 16, seed=4).to(DEV)
    assert hip.persistent_ok(DEV) and float((x.flatten(2).abs().amax(2) == 0).float().mean()) > 0.5
    want, n_off = _ips(net, x, False, calls)
    got, n_on = _ips(net, x, True, calls)
    again, _ = _ips(net, x, True, calls)
    assert n_off == 0 and 1 <= n_on <= parts and (n_on == parts) == (limit > 100), "the counted route with %d parts was meant to run" % parts
    own = [a[1] - a[0] for a in calls[:n_on]]                           # parts of its own per launch (part_end - part_begin)
    assert own == [1] * n_on if limit > 100 or N != 320 else own == [0], own
    for name, a, b, c in zip(("mem_patch", "mem_pos", "last_mem_idx", "last_mem_emb"), got, want, again):
        assert torch.equal(a, b), name
        assert torch.equal(c, b), name + " (second call)"
    assert int(net.selection.scan_status_host.item()) == 0
