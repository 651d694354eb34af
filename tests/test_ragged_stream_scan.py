"""``ipsx_scan_ragged_spans`` (the loop launch of ``IPSNet.ips_ragged_stream``) on logits alone: every case of
tests/ragged_lattice_cases.py - one per instantiation class of the ragged loop - with its slides laid into a strided table
whose gaps and last rows are NaN.  Indices equal the oracle's; indices, scores and tie flags equal, bit for bit, what
``ipsx_scan_ragged`` leaves on the packed table.  Beside the lattice: spans cut to M + k * I rows (what a feed scans), spans
of exactly M rows and of no rows (left untouched), spans in descending address order.  No tolerance anywhere."""

import numpy as np
import pytest
import torch

import ragged_lattice_cases as lc
from ips_amd import hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FEW = ("f8-e2-gt", "f32-e8-lt", "l-r12", "cam")          # one case per kernel family for the tests beside the lattice
GAP, TAIL = 3, 5                                         # NaN rows between two spans, and behind the last
IDX0, SC0, TIE0 = -7, -3.0, 5                            # what the outputs hold before a launch


def strided(name, kind, counts=None, descending=False):
    """The slides of a case laid into one table, ``GAP`` NaN rows in front of each and ``TAIL`` behind the last
    -> (table, spans (B, 2)); ``counts``: the rows of each span that are candidates (the slide's rows lie there whole)."""
    lens, lg = lc.case_table(name, kind)
    st = lc.starts(lens)
    B, R = len(lens), lg.shape[1]
    table = np.full((sum(lens) + GAP * B + TAIL, R), np.nan, dtype=np.float32)
    spans = np.zeros((B, 2), dtype=np.int64)
    at = 0
    for b in (reversed(range(B)) if descending else range(B)):
        at += GAP
        table[at:at + lens[b]] = lg[st[b]:st[b + 1]]
        spans[b] = (at, lens[b] if counts is None else counts[b])
        at += lens[b]
    return table, spans


def scan_spans(table, spans, name, mode, touched=None):
    """One ``ipsx_scan_ragged_spans`` launch under tie order ``mode`` -> (mem_idx, mem_score, tie flags) on the host.  The
    tie flags of the slides in ``touched`` (default: all) start at 0, everything else at its sentinel."""
    M, I, H, T, _ = lc.CASES[name]
    B = len(spans)
    idx = torch.full((B, M), IDX0, dtype=torch.int64, device=DEV)
    sc = torch.full((B, M), SC0, dtype=torch.float32, device=DEV)
    tie = np.full((B,), TIE0, dtype=np.int32)
    tie[list(range(B)) if touched is None else list(touched)] = 0
    tie = torch.from_numpy(tie).to(DEV)
    prev = hip.set_tie_order(mode)
    try:
        hip.scan_ragged_spans(torch.from_numpy(table).to(DEV), torch.from_numpy(spans).to(DEV), int(spans[:, 1].max()), M, I, H, T,
                              idx, tie, mem_score=sc)
        return idx.cpu().numpy(), sc.cpu().numpy(), tie.cpu().numpy()
    finally:
        hip.set_tie_order(prev)


_PACKED = {}


def packed_scan(name, kind, mode):
    """``ipsx_scan_ragged`` on the case's packed table; made once per (case, kind, tie order)."""
    if (name, kind, mode) not in _PACKED:
        M, I, H, T, _ = lc.CASES[name]
        lens, lg = lc.case_table(name, kind)
        prev = hip.set_tie_order(mode)
        try:
            idx, sc = hip.scan_ragged(torch.from_numpy(np.array(lg)).to(DEV), torch.from_numpy(lc.starts(lens)).to(DEV), lens, M, I, H, T,
                                      want_scores=True)
            _PACKED[(name, kind, mode)] = (idx.cpu().numpy(), sc.cpu().numpy(), hip.scan_ragged.last_tie.cpu().numpy())
        finally:
            hip.set_tie_order(prev)
    return _PACKED[(name, kind, mode)]


def same_bits(a, b):
    return np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("kind", ["cont", "dup"])
@pytest.mark.parametrize("name", list(lc.CASES))
def test_spans_match_the_oracle_and_the_packed_launch(name, kind):
    table, spans = strided(name, kind)
    for mode, aten in lc.MODES:
        idx, sc, tie = scan_spans(table, spans, name, mode)
        want = lc.case_oracle(name, kind, aten)
        for b in range(len(spans)):
            print(name, kind, mode, "slide", b, "wrong indices", int((idx[b] != want[b][0]).sum()))
            assert np.array_equal(idx[b], want[b][0]), (name, kind, mode, b, "mem_idx against the oracle")
        p_idx, p_sc, p_tie = packed_scan(name, kind, mode)
        assert np.array_equal(idx, p_idx), (name, kind, mode, "mem_idx against ipsx_scan_ragged")
        assert same_bits(sc, p_sc), (name, kind, mode, "mem_score, bit for bit")
        assert np.array_equal(tie, p_tie), (name, kind, mode, "tie flags")


@pytest.mark.parametrize("name", FEW)
def test_spans_cut_to_whole_chunks(name):
    """What a feed scans: the first M + k * I rows of a slide, k one below the slide's own iteration count - against the
    oracle's loop on that prefix.  The slides with one iteration are cut to M rows: not touched."""
    M, I, H, T, _ = lc.CASES[name]
    lens, lg = lc.case_table(name, "dup")
    st = lc.starts(lens)
    k = [(n - M + I - 1) // I - 1 for n in lens]
    counts = [M + kb * I for kb in k]
    live = [b for b, kb in enumerate(k) if kb > 0]
    assert live and len(live) < len(lens)
    table, spans = strided(name, "dup", counts)
    for mode, aten in lc.MODES:
        idx, sc, tie = scan_spans(table, spans, name, mode, touched=live)
        for b in range(len(lens)):
            if b not in live:
                assert (idx[b] == IDX0).all() and (sc[b] == SC0).all() and tie[b] == TIE0, (name, mode, b, "a span of M rows was touched")
                continue
            cur, last, ties, _ = lc.oracle_loop(lg[st[b]:st[b] + counts[b]], M, I, H, T, aten)
            assert np.array_equal(idx[b], cur), (name, mode, b, "mem_idx")
            assert same_bits(sc[b], last), (name, mode, b, "mem_score")
            assert int(tie[b]) == int(any(ties)), (name, mode, b, "tie flag")


@pytest.mark.parametrize("name", FEW)
def test_spans_of_m_rows_and_of_no_rows_keep_the_sentinel(name):
    M = lc.CASES[name][0]
    lens, _ = lc.case_table(name, "cont")
    counts = list(lens)
    counts[0], counts[2] = M, 0
    table, spans = strided(name, "cont", counts)
    live = [b for b in range(len(lens)) if b not in (0, 2)]
    for mode, _ in lc.MODES:
        idx, sc, tie = scan_spans(table, spans, name, mode, touched=live)
        p_idx, p_sc, p_tie = packed_scan(name, "cont", mode)
        for b in (0, 2):
            assert (idx[b] == IDX0).all() and (sc[b] == SC0).all() and tie[b] == TIE0, (name, mode, b)
        assert np.array_equal(idx[live], p_idx[live]) and same_bits(sc[live], p_sc[live]) and np.array_equal(tie[live], p_tie[live])


@pytest.mark.parametrize("name", FEW)
def test_spans_in_descending_address_order(name):
    table, spans = strided(name, "dup", descending=True)
    assert (np.diff(spans[:, 0]) < 0).all()
    for mode, _ in lc.MODES:
        idx, sc, tie = scan_spans(table, spans, name, mode)
        p_idx, p_sc, p_tie = packed_scan(name, "dup", mode)
        assert np.array_equal(idx, p_idx) and same_bits(sc, p_sc) and np.array_equal(tie, p_tie), (name, mode)
