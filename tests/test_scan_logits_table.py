"""The part table of ``ipsx_scan_range_logits`` on the host (``ipsx_scan_logits_check`` through ``hip.LogitsParts.check``; no
device): parts tile an image's rows in order, a launch takes a run of whole parts, and the rows its iterations read end
inside the last of them.  Also the table ``hip.LogitsParts`` builds from rows per part, and what ``Selection`` cuts."""

import pytest

from ips_amd import hip
from ips_amd.dist import part_iterations

M = I = 64


def table(rows):
    return hip.LogitsParts(rows=rows)


def test_first_rows_are_the_prefix_sums():
    t = table([1250, 750, 375, 125])
    assert t.first == [0, 1250, 2000, 2375] and t.n == 2500 and len(t) == 4
    assert [(t.array[k].rows, t.array[k].first) for k in range(4)] == [(1250, 0), (750, 1250), (375, 2000), (125, 2375)]


@pytest.mark.parametrize("N", [209, 384, 2500, 3000])
@pytest.mark.parametrize("P", [2, 3, 4])
def test_the_cuts_of_the_counted_route_pass(N, P):
    """Parts cut at the loop's chunk boundaries, as ``Selection.parts_with_ranges`` cuts them: part k and the iterations
    its[k] .. its[k + 1] are a launch; the last launch's redo (all parts, iterations from 0) needs nothing more."""
    n_iter = -(-(N - M) // I)
    its = part_iterations(n_iter, P)
    edges = [0] + [min(N, M + it * I) for it in its[1:]]
    edges[-1] = N
    t = table([edges[k + 1] - edges[k] for k in range(len(its) - 1)])
    for k in range(len(its) - 1):
        t.check(k, k + 1, M, I, its[k], its[k + 1])
    t.check(0, len(its) - 1, M, I, 0, n_iter)


def test_ranges_that_do_not_fit_are_refused():
    t = table([128, 20, 108, 128])                          # N = 384: 5 iterations
    t.check(0, 1, M, I, 0, 1)
    t.check(1, 3, M, I, 1, 3)
    t.check(3, 4, M, I, 3, 5)
    t.check(3, 3, M, I, 1, 3)                               # no part of its own: the rows are earlier launches'
    t.check(4, 4, M, I, 3, 5)
    for bad, msg in (((0, 1, M, I, 0, 2), "read rows up to 192, the parts in front of part 1 end at 128"),     # iteration 1 reads part 1's rows
                     ((1, 2, M, I, 1, 2), "read rows up to 192, the parts in front of part 2 end at 148"),
                     ((0, 0, M, I, 0, 1), "read rows up to 128, the parts in front of part 0 end at 0"),
                     ((3, 4, M, I, 3, 6), "outside the loop"),
                     ((3, 4, M, I, 4, 4), "outside the loop"),                            # an empty range: nothing to launch
                     ((3, 2, M, I, 1, 2), r"parts \[3, 2\) of 4"),
                     ((3, 5, M, I, 3, 5), r"parts \[3, 5\) of 4")):
        with pytest.raises(RuntimeError, match=msg):
            t.check(*bad)


def test_tables_that_do_not_tile_an_image_are_refused():
    t = table([128, 64, 192])
    t.array[2].first = 200                                   # a gap in front of part 2
    with pytest.raises(RuntimeError, match="part 2 starts at row 200, the parts in front of it end at 192"):
        t.check(0, 1, M, I, 0, 1)
    t = table([128, 0, 256])
    with pytest.raises(RuntimeError, match="part 1 has 0 rows"):
        t.check(0, 1, M, I, 0, 1)
    with pytest.raises(RuntimeError, match="1 to 16 parts"):
        table([24] * 17).check(0, 1, M, I, 0, 1)
    t = table([64])                                          # N = M: no loop
    with pytest.raises(RuntimeError, match="more patches"):
        t.check(0, 1, M, I, 0, 1)
    t16 = table([64 + 64] + [64] * 15)                       # 16 parts: the most a launch's arguments hold
    t16.check(15, 16, M, I, 15, 16)
