"""``ipsx_scan_ragged`` on logits alone (no encoder): the RAGGED instantiations of scan_fast_kernel, scan_cam_kernel and
scan_large_kernel on packed tables of B = 5 slides against ``ipsx_scan`` called on a contiguous copy of every slide alone -
``mem_idx`` and ``tie_flag`` equal, ``mem_score`` bit for bit (the criterion tests/test_scan_mnist.py uses between two loop
kernels), in both tie orders, on tables that do tie: quantised logits, and a stretch of duplicated rows.

Every shape here has I = M.  Shapes with I != M, every instantiation class of the three kernels, and the oracle's loop as the
criterion: tests/test_ragged_scan_lattice.py."""

import numpy as np
import pytest
import torch

from ips_amd import hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ("torch", "canonical")


def _large_by_size():
    """The smallest M = I from the smallest LDS-resident case upward for which one slide of 8 heads x 1 token needs a
    workspace, i.e. leaves the LDS-resident loops for scan_large_kernel - asked of the library, not written down."""
    L = hip.lib()
    m = 16
    while L.ipsx_scan_workspace_bytes(1, m, m, 8, 1) == 0:
        m += 1
        assert m < 20000
    return m


# name -> (M = I, heads, tokens): one per kernel, at the smallest shape that reaches it
SHAPES = {
    "fast": lambda: (16, 8, 1),             # scan_fast_kernel
    "fast-mnist": lambda: (64, 8, 4),       # scan_fast_kernel through the Megapixel-MNIST shape
    "cam": lambda: (256, 8, 1),             # scan_cam_kernel
    "large-heads": lambda: (16, 3, 1),      # scan_large_kernel: a head count the LDS loops do not cover
    "large-size": lambda: (_large_by_size(), 8, 1),     # scan_large_kernel: candidate sets beyond the LDS
}


def lengths_of(m, i):
    return (m + 1, m + i, m + i + 1, m + 3 * i - 1, m + 3 * i - 1)


def make_table(kind, lengths, m, i, R, pad=0):
    """A packed (sum lengths + pad, R) table; the ``pad`` rows behind the last slide are NaN."""
    g = np.random.default_rng(4100 + 31 * m + R + (0 if kind == "quant" else 1))
    total = sum(lengths)
    if kind == "quant":
        # values from a small set, equal across (head, token): whole candidates tie, and their rows are bit-identical
        lg = np.repeat((g.integers(0, 5, (total, 1)).astype(np.float32) - 1.0) * np.float32(0.75), R, axis=1)
    else:
        lg = (g.standard_normal((total, R)) * 3.0).astype(np.float32)
        lo = 0
        for n in lengths:                     # the slide's last rows are its first rows again (into the ragged last chunk)
            k = min(i, n - m)
            lg[lo + n - k:lo + n] = lg[lo:lo + k]
            lo += n
    if pad:
        lg = np.concatenate([lg, np.full((pad, R), np.nan, dtype=np.float32)])
    return np.ascontiguousarray(lg)


def offsets_of(lengths):
    return torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int64, device=DEV)


def solo_scans(lg, lengths, m, i, h, t):
    """``ipsx_scan`` on a contiguous copy of every slide alone -> (idx (B, m), scores (B, m), tie (B,)) on the host."""
    idx, sc, tie, lo = [], [], [], 0
    for n in lengths:
        slide = lg[lo:lo + n].clone().unsqueeze(0)
        a, b = hip.scan(slide, m, i, h, t, want_scores=True)
        idx.append(a.cpu())
        sc.append(b.cpu())
        tie.append(hip.scan.last_tie.cpu())
        lo += n
    return torch.cat(idx), torch.cat(sc), torch.cat(tie)


def ragged_scan(lg, lengths, m, i, h, t):
    total = sum(lengths)
    idx, sc = hip.scan_ragged(lg[:total], offsets_of(lengths), lengths, m, i, h, t, want_scores=True)
    return idx.cpu(), sc.cpu(), hip.scan_ragged.last_tie.cpu()


def assert_equal(got, want):
    assert torch.equal(got[0], want[0]), "mem_idx"
    assert torch.equal(got[2], want[2]), "tie_flag"
    assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)), "mem_score, bit for bit"


@pytest.mark.parametrize("kind", ["quant", "dup"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_ragged_scan_equals_the_solo_scans(shape, kind):
    m, h, t = SHAPES[shape]()
    i, R = m, h * t
    if shape == "large-size":
        assert hip.lib().ipsx_scan_workspace_bytes(1, m - 1, m - 1, 8, 1) == 0 < hip.lib().ipsx_scan_workspace_bytes(1, m, m, 8, 1)
    lengths = lengths_of(m, i)
    lg = torch.from_numpy(make_table(kind, lengths, m, i, R)).to(DEV)
    tied = False
    for mode in MODES:
        hip.set_tie_order(mode)
        try:
            want = solo_scans(lg, lengths, m, i, h, t)
            got = ragged_scan(lg, lengths, m, i, h, t)
        finally:
            hip.set_tie_order("torch")
        assert_equal(got, want)
        for b, n in enumerate(lengths):        # slide-local indices, no candidate twice
            row = got[0][b]
            assert int(row.min()) >= 0 and int(row.max()) < n and len(set(row.tolist())) == m
        tied = tied or bool(want[2].any())
    if kind == "quant":
        assert tied, "the quantised table was built to tie at the boundary of the memory"


@pytest.mark.parametrize("shape", ["fast", "cam", "large-heads"])
def test_equal_lengths_equal_the_dense_scan(shape):
    m, h, t = SHAPES[shape]()
    i, R = m, h * t
    n = m + 2 * i + 3
    for B in (1, 5):
        lengths = (n,) * B
        lg = torch.from_numpy(make_table("dup", lengths, m, i, R)).to(DEV)
        idx, sc = hip.scan(lg.view(B, n, R), m, i, h, t, want_scores=True)
        want = (idx.cpu(), sc.cpu(), hip.scan.last_tie.cpu())
        assert_equal(ragged_scan(lg, lengths, m, i, h, t), want)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_rows_behind_the_last_slide_are_never_read(shape):
    """The table's rows behind row_offsets[B] are NaN: a NaN that entered any slide's candidates would win its softmax."""
    m, h, t = SHAPES[shape]()
    i, R = m, h * t
    lengths = lengths_of(m, i)
    clean = torch.from_numpy(make_table("dup", lengths, m, i, R)).to(DEV)
    padded = torch.from_numpy(make_table("dup", lengths, m, i, R, pad=2 * i + 7)).to(DEV)
    want = ragged_scan(clean, lengths, m, i, h, t)
    got = ragged_scan(padded, lengths, m, i, h, t)
    assert_equal(got, want)
    assert not torch.isnan(got[1]).any()


def test_the_binding_refuses_what_the_kernel_must_not_see():
    lg = torch.zeros((40, 8), device=DEV)
    with pytest.raises(ValueError, match="slide 1"):
        hip.scan_ragged(lg, offsets_of((24, 16)), (24, 16), 16, 16, 8, 1)
    with pytest.raises(ValueError):
        hip.scan_ragged(lg, offsets_of((24, 17)), (24, 17), 16, 16, 8, 1)          # 41 rows in a table of 40
