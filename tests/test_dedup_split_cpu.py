"""The split of a list between the fused trunk's two exact fp32 kernels (``trunk_split_n8``, ipsx_internal.h): the launches
behind the blank scan compute it on the device from a count only the device knows, ``fused_launch`` on the host.  The function
is read through the host-only export ``ipsx_dbg_trunk_split`` (no GPU): the first ``n8`` entries go through eight-patch
workgroups, the other ``count - n8`` through pair workgroups, for which the pair launch's grid must have room."""

import ctypes as C

import pytest

from ips_amd import hip

UNITS = [8, 64, 104, 256, 304]


def entry():
    fn = hip.lib().ipsx_dbg_trunk_split
    fn.restype = C.c_longlong
    fn.argtypes = [C.c_longlong, C.c_int, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.c_int, C.POINTER(C.c_int)]
    return fn


def split(count, cus, mode):
    """(n8, pair workgroups of a launch whose list has at most ``count`` entries)"""
    grid = C.c_longlong(-1)
    n8 = entry()(count, cus, mode, C.byref(grid), None, 0, None)
    return int(n8), int(grid.value)


def thresholds(cus, mode=0):
    buf, n = (C.c_longlong * 64)(), C.c_int(-1)
    entry()(0, cus, mode, None, buf, 64, C.byref(n))
    assert 0 <= n.value <= 64
    return [int(buf[k]) for k in range(n.value)]


def counts(cus):
    """0 .. 5 R: every count within 20 of a multiple of R and of a threshold behind it, every 7th one between."""
    R = 8 * cus
    near = {0, 1, 2, 3}
    for m in range(6):
        for t in [0] + thresholds(cus):
            near.update(range(max(0, m * R + t - 20), m * R + t + 21))
    return sorted(c for c in near.union(range(0, 5 * R + 1, 7)) if c <= 5 * R)


@pytest.mark.parametrize("cus", UNITS)
def test_the_rule_gives_whole_rounds_or_everything_to_the_eight_patch_kernel(cus):
    R = 8 * cus
    ts = thresholds(cus)
    most = 0
    for c in counts(cus):
        n8, _ = split(c, cus, 0)
        assert 0 <= n8 <= c
        assert n8 % R == 0 or n8 == c
        assert c - n8 < R                                                # never more than the remainder
        most = max(most, c - n8)
        # the pair launch of ANY list that can hold c entries has a workgroup for each of its pairs
        for n in (c, c + 1, c + R, 5 * R + 11):
            assert 2 * split(n, cus, 0)[1] >= c - n8
    # the grid is bounded by the largest remainder the rule hands over, not by the list
    assert split(1000 * R, cus, 0)[1] == (most + 1) // 2 <= (R + 1) // 2
    # a pure function of the count: the same remainder, the same decision, in every round
    for r in range(0, R, max(1, R // 61)):
        assert len({split(m * R + r, cus, 0)[0] == m * R for m in range(1, 5)}) == 1
    # the thresholds are where, and only where, the decision changes
    pair = [split(R + r, cus, 0)[0] == R for r in range(1, R)]
    assert [r for r in range(1, R - 1) if pair[r - 1] != pair[r]] == ts


@pytest.mark.parametrize("cus", UNITS)
def test_modes_one_and_two(cus):
    R = 8 * cus
    for c in counts(cus):
        n8, grid = split(c, cus, 1)
        assert n8 == c and grid == 0                                     # the parent's behaviour: no pair launch at all
        n8, grid = split(c, cus, 2)
        assert n8 == 0 and 2 * grid >= c and grid == (c + 1) // 2
    assert thresholds(cus, 1) == [] and thresholds(cus, 2) == []
    assert R == 8 * cus


def test_the_mode_set_by_the_switch_is_the_default():
    lib = hip.lib()
    sw = lib.ipsx_dbg_fused_trunk_pair
    sw.restype, sw.argtypes = None, [C.c_int]
    try:
        for mode in (1, 2, 0):
            sw(mode)
            for c in (0, 5, 2048, 2049, 2810, 4095):
                assert split(c, 256, -1) == split(c, 256, mode)
    finally:
        sw(0)
