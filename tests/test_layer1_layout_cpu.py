"""The position tiles of fused_trunk_kernel's layer1 (csrc/fused_trunk_eight.h: conv_p1, the trait Geo8), read back from the
kernel's own tables through the host-only export ipsx_dbg_layer1_layout and checked by brute force over the 8x8 map with pad
1: a tap may be left out for a tile only where it reads nothing but padding, and the counts are the ones DESIGN 5.1
states.  The 4x4 stage's tables, of the same type, are checked by tests/test_tile16_layout_cpu.py."""

import ctypes as C

import pytest

from ips_amd import hip


@pytest.fixture(scope="module")
def layout():
    fn = hip.lib().ipsx_dbg_layer1_layout
    fn.restype, fn.argtypes = None, [C.POINTER(C.c_int)] * 3
    tiles, wave_set, live = (C.c_int * 96)(), (C.c_int * 8)(), (C.c_int * 36)()
    fn(tiles, wave_set, live)
    return ([tuple(tiles[6 * k:6 * k + 6]) for k in range(16)], list(wave_set), [list(live[9 * s:9 * s + 9]) for s in range(4)])


def reads_padding(pix, ky, kx):
    y, x = pix // 8 + ky - 1, pix % 8 + kx - 1
    return not (0 <= y < 8 and 0 <= x < 8)


def test_every_position_lies_in_exactly_one_tile(layout):
    tiles = layout[0]
    assert sorted(p for t in tiles for p in t[:4]) == list(range(64))


def test_a_tap_is_left_out_iff_all_four_positions_read_padding(layout):
    tiles, _, live = layout
    for k, t in enumerate(tiles):
        pix, sky, skx = t[:4], t[4], t[5]
        for ky in range(3):
            for kx in range(3):
                out = ky == sky or kx == skx
                assert out == all(reads_padding(p, ky, kx) for p in pix), (k, ky, kx)
                assert out == (not (live[k // 4][3 * ky + kx] >> (k % 4) & 1)), (k, ky, kx)


def test_live_tile_taps_per_set_are_30_30_33_33(layout):
    _, _, live = layout
    per_set = [sum(bin(m).count("1") for m in live[s]) for s in range(4)]
    assert per_set == [30, 30, 33, 33]
    assert sum(per_set) == 126 and 9 * 16 == 144


def test_wave_to_set_map_pairs_the_sets_on_every_simd(layout):
    wave_set = layout[1]
    assert wave_set == [(w + 2 * (w >> 2)) & 3 for w in range(8)] == [0, 1, 2, 3, 2, 3, 0, 1]
    # waves w and w + 4 share a SIMD: T + L, B + R, L + T, R + B (sets T B L R = 0 1 2 3)
    assert [(wave_set[w], wave_set[w + 4]) for w in range(4)] == [(0, 2), (1, 3), (2, 0), (3, 1)]
