"""The 16-row tiles of fused_trunk_kernel's 4x4 stage (csrc/fused_trunk.hip: conv_t16), read back from the kernel's own
tables through the host-only export ipsx_dbg_tile16_layout and checked by brute force over the 4x4 map with pad 1: a tap may
be left out for a tile only where it reads nothing but padding, and the counts are the ones DESIGN 5.1 states."""

import ctypes as C

import pytest

from ips_amd import hip


@pytest.fixture(scope="module")
def layout():
    fn = hip.lib().ipsx_dbg_tile16_layout
    fn.restype, fn.argtypes = None, [C.POINTER(C.c_int)] * 4
    tiles, wave_set, live, pos = (C.c_int * 32)(), (C.c_int * 8)(), (C.c_int * 18)(), (C.c_int * 16)()
    fn(tiles, wave_set, live, pos)
    return ([tuple(tiles[4 * k:4 * k + 4]) for k in range(8)], list(wave_set), [list(live[9 * s:9 * s + 9]) for s in range(2)],
            list(pos))


def reads_padding(pix, ky, kx):
    y, x = pix // 4 + ky - 1, pix % 4 + kx - 1
    return not (0 <= y < 4 and 0 <= x < 4)


def test_every_position_lies_in_exactly_one_tile(layout):
    tiles = layout[0]
    assert sorted(p for t in tiles for p in t[:2]) == list(range(16))


def test_a_tap_is_left_out_iff_both_positions_read_padding(layout):
    tiles, _, live, _ = layout
    for k, (p0, p1, sky, skx) in enumerate(tiles):
        for ky in range(3):
            for kx in range(3):
                out = ky == sky or kx == skx
                assert out == (reads_padding(p0, ky, kx) and reads_padding(p1, ky, kx)), (k, ky, kx)
                assert out == (not (live[k // 4][3 * ky + kx] >> (k % 4) & 1)), (k, ky, kx)


def test_counts_54_of_72_and_27_per_wave(layout):
    tiles, wave_set, live, _ = layout
    per_set = [sum(bin(m).count("1") for m in live[s]) for s in range(2)]
    assert per_set == [27, 27] and sum(per_set) == 54 and 9 * len(tiles) == 72
    assert sorted(wave_set) == [0] * 4 + [1] * 4
    assert all(per_set[wave_set[w]] == 27 for w in range(8))
    assert all(wave_set[w] != wave_set[w + 4] for w in range(4))          # the two waves of a SIMD: one of each set
    # real (position, tap) pairs: all 100 of the map's are covered by the live tile-taps
    real = sum(not reads_padding(p, ky, kx) for p in range(16) for ky in range(3) for kx in range(3))
    assert real == 100


def test_channel_permutation_is_a_bijection_that_groups_the_lane_groups_k(layout):
    pos = layout[3]
    assert sorted(pos) == list(range(16))
    order = [pos.index(p) for p in range(16)]
    assert order == [0, 2, 8, 10, 4, 6, 12, 14, 1, 3, 9, 11, 5, 7, 13, 15]
    # lane group g, component j: instruction (j & 1) of 8-group (j >> 1) takes slots (k0,k4,k1,k5) / (k2,k6,k3,k7)
    for g in range(4):
        for j in range(4):
            assert order[4 * g + j] == 8 * (j >> 1) + (0, 4, 1, 5)[g] + 2 * (j & 1)


def test_pack_tile16_sizes():
    L = hip.lib()
    assert L.ipsx_packed_conv_weight_tile16_elems(128, 128, 3, 3) == 128 * 128 * 9
    assert L.ipsx_packed_conv_weight_tile16_elems(120, 128, 3, 3) == 0
    assert L.ipsx_packed_conv_weight_tile16_elems(128, 24, 3, 3) == 0
