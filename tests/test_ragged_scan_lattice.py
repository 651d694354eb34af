"""``ipsx_scan_ragged`` held to the oracle's loop (orc_scores_from_logits + orc_topm / orc_topm_loop) at every
instantiation it can reach, with I != M: the eight (EPT, LCH) classes of scan_fast_kernel for 8 and for 32 logit rows, the
three staging paths of scan_large_kernel, and scan_cam_kernel (tests/ragged_lattice_cases.py holds the shapes, the slide
lengths and the tables; tests/test_ragged_lattice_cpu.py shows from the oracle alone that these inputs tell right from
wrong).  One launch per packed table and tie order; slide by slide ``mem_idx`` equal, ``mem_score`` bit for bit, the tie
flag, slide-local indices.  No tolerance anywhere: the oracle follows the kernels' order of arithmetic.

Not tested, on purpose: device offsets that contradict the host lengths or leave the table (the host checks that refuse
them are tested in tests/test_ragged_scan.py; the device-side guard is not to be driven on a shared machine), and tables
of 2^31 rows."""

import numpy as np
import pytest
import torch

import ragged_lattice_cases as lc
from ips_amd import hip
from tests.util import ulp_diff

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FEW = ("f8-e2-gt", "f32-e8-lt", "l-r12", "cam")          # one case per kernel family for the tests beside the lattice
LARGE = [n for n in lc.CASES if n.startswith("l-")]


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)          # (a copy: the cached tables are read-only)


def offsets_of(lens):
    return torch.from_numpy(lc.starts(lens)).to(DEV)


def scan(lg, lens, name, mode, workspace=None):
    """One ``ipsx_scan_ragged`` launch under tie order ``mode`` -> (mem_idx, mem_score, tie flags) on the host."""
    M, I, H, T, _ = lc.CASES[name]
    prev = hip.set_tie_order(mode)
    try:
        idx, sc = hip.scan_ragged(lg, offsets_of(lens), lens, M, I, H, T, want_scores=True, workspace=workspace)
        tie = hip.scan_ragged.last_tie
        return idx.cpu().numpy(), sc.cpu().numpy(), tie.cpu().numpy()
    finally:
        hip.set_tie_order(prev)


_GPU = {}


def case_scan(name, kind, mode):
    """The launch on the case's own table; made once per (case, kind, tie order)."""
    if (name, kind, mode) not in _GPU:
        lens, lg = lc.case_table(name, kind)
        _GPU[(name, kind, mode)] = scan(dev(lg), lens, name, mode)
    return _GPU[(name, kind, mode)]


def check_slide(got, b, want, n, M, what, dup_ok=False):
    """Slide ``b`` of a launch against ``oracle_loop``'s (indices, scores, ties, admitted)."""
    idx, sc, tie = got
    cur, last, ties, _ = want
    print(what, "slide", b, "rows", n, "wrong indices", int((idx[b] != cur).sum()), "oracle tie", int(any(ties)), "flag", int(tie[b]))
    assert np.array_equal(idx[b], cur), (what, b, "mem_idx")
    # (a NaN score has no bits to compare: the host's inf - inf is a negative NaN, the kernels return the canonical one)
    nan = np.isnan(last)
    assert np.array_equal(np.isnan(sc[b]), nan), (what, b, "NaN scores")
    assert nan.all() or ulp_diff(sc[b][~nan], last[~nan]) == 0, (what, b, "mem_score, bit for bit")
    assert int(tie[b]) == int(any(ties)), (what, b, "tie flag", ties)
    assert int(idx[b].min()) >= 0 and int(idx[b].max()) < n, (what, b, "slide-local indices")
    if not (dup_ok and len(set(cur.tolist())) < M):
        assert len(set(idx[b].tolist())) == M, (what, b, "a candidate twice")


@pytest.mark.parametrize("name", list(lc.CASES))
def test_the_library_takes_the_case_where_its_name_says(name):
    """LDS-resident (no workspace) for every ``f*`` case and ``cam``, scan_large_kernel (a workspace) for every ``l-*``;
    scan_cam_kernel's shape for ``cam`` alone.  A disagreement means the case table is wrong: it fails, it does not skip."""
    M, I, H, T, cls = lc.CASES[name]
    nb = hip.lib().ipsx_scan_workspace_bytes(1, M, I, H, T)
    print(name, (M, I, H, T), cls, "workspace bytes per slide:", nb, "scan_cam_kernel's shape:", hip.scan_persistent_groupable(M, I, H, T))
    if name.startswith("l-"):
        assert nb > 0
    else:
        assert nb == 0
        if name.startswith("f"):
            assert lc.fast_class(M, I, H * T) == cls
    assert hip.scan_persistent_groupable(M, I, H, T) == (name == "cam")
    assert not hip.scan_mnist_shape(M, I, H, T)


@pytest.mark.parametrize("kind", lc.KINDS)
@pytest.mark.parametrize("name", list(lc.CASES))
def test_ragged_scan_matches_the_oracle(name, kind):
    M, I, H, T, _ = lc.CASES[name]
    lens = lc.lengths(M, I)
    for mode, aten in lc.MODES:
        got = case_scan(name, kind, mode)
        want = lc.case_oracle(name, kind, aten)
        for b, n in enumerate(lens):
            check_slide(got, b, want[b], n, M, (name, kind, mode), dup_ok=kind == "special")


@pytest.mark.parametrize("name", FEW)
def test_slides_packed_in_reverse_order(name):
    """The same slides packed back to front: the reversed rows of the three outputs."""
    lens, lg = lc.case_table(name, "quant")
    st = lc.starts(lens)
    rev = np.concatenate([lg[st[b]:st[b + 1]] for b in reversed(range(len(lens)))])
    for mode, _ in lc.MODES:
        want = case_scan(name, "quant", mode)
        got = scan(dev(rev), lens[::-1], name, mode)
        assert want[2].any(), "the quantised table ties"
        assert np.array_equal(got[0], want[0][::-1]), (name, mode, "mem_idx")
        assert np.array_equal(got[1].view(np.int32), want[1][::-1].view(np.int32)), (name, mode, "mem_score")
        assert np.array_equal(got[2], want[2][::-1]), (name, mode, "tie flags")


@pytest.mark.parametrize("name", FEW)
def test_special_values_stay_inside_their_slide(name):
    """``special`` is ``cont`` plus a NaN, a +inf and a stretch of -inf in slides 0, 2 and 5: slides 1, 3 and 4 come out as
    from the ``cont`` table, bit for bit, and without a NaN."""
    for mode, _ in lc.MODES:
        cont, spec = case_scan(name, "cont", mode), case_scan(name, "special", mode)
        for b in lc.CLEAN:
            assert np.array_equal(spec[0][b], cont[0][b]), (name, mode, b, "mem_idx")
            assert np.array_equal(spec[1][b].view(np.int32), cont[1][b].view(np.int32)), (name, mode, b, "mem_score")
            assert spec[2][b] == cont[2][b] and not np.isnan(spec[1][b]).any(), (name, mode, b)


@pytest.mark.parametrize("name", FEW)
def test_one_slide(name):
    """B = 1, the longest length (its last chunk one row short)."""
    M = lc.CASES[name][0]
    lens, lg = lc.case_table(name, "quant")
    b = int(np.argmax(lens))
    st = lc.starts(lens)
    for mode, aten in lc.MODES:
        got = scan(dev(lg[st[b]:st[b + 1]]), lens[b:b + 1], name, mode)
        assert got[0].shape == (1, M)
        check_slide(got, 0, lc.case_oracle(name, "quant", aten)[b], lens[b], M, (name, "one slide", mode))


@pytest.mark.parametrize("name", FEW)
def test_many_slides(name):
    """B = 40: the six slides of the table cycled (six full tables and four slides of a seventh), every slide against the
    oracle's result for its content."""
    M = lc.CASES[name][0]
    lens, lg = lc.case_table(name, "quant")
    B = 40
    reps = -(-B // len(lens))
    many = tuple((lens * reps)[:B])
    packed = np.concatenate([lg] * reps)[:sum(many)]
    for mode, aten in lc.MODES:
        got = scan(dev(packed), many, name, mode)
        want = lc.case_oracle(name, "quant", aten)
        assert got[0].shape == (B, M)
        for b in range(B):
            check_slide(got, b, want[b % len(lens)], many[b], M, (name, "many slides", mode))


@pytest.mark.parametrize("name", LARGE)
def test_a_workspace_of_exactly_the_stated_size(name):
    """B times ``ipsx_scan_workspace_bytes(1, ...)`` passed explicitly gives what the default gives; one byte fewer is
    refused by the library with its workspace error, before anything is launched."""
    M, I, H, T, _ = lc.CASES[name]
    lens, lg = lc.case_table(name, "dup")
    nb = len(lens) * hip.lib().ipsx_scan_workspace_bytes(1, M, I, H, T)
    assert nb > 0
    want = case_scan(name, "dup", "torch")
    got = scan(dev(lg), lens, name, "torch", workspace=torch.empty(nb, dtype=torch.uint8, device=DEV))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
    assert np.array_equal(got[1].view(np.int32), want[1].view(np.int32))
    with pytest.raises(RuntimeError, match="needs a workspace of %d B" % nb):
        scan(dev(lg), lens, name, "torch", workspace=torch.empty(nb - 1, dtype=torch.uint8, device=DEV))
