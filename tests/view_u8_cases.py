"""Shared by tests/test_patch_view_u8.py and tests/test_patch_view_u8_cpu.py: guarded uint8 images for the patch-grid view
over bytes, their table, and the load width ("tier") each stem's launcher is expected to pick per geometry."""

import numpy as np
import torch

from view_cases import grid

GUARD = 4096                        # bytes of 255 on either side of the images
POISON = 1e30                       # table[c][255]: finite, and no covered pixel (bytes 0..254) can equal it

# the widths (bytes per load, widest first) of every kernel that reads uint8 images (csrc: fused_view_args, fused_stem_pool50)
TIERS = {"fused": (16, 4, 1), "pair": (8, 4, 1), "pool50": (2, 1), "pool100": (4, 1)}


def guard_table(n_chan, seed=0):
    """(n_chan, 256) float32, random per channel, table[c][0] != 0 (a dequantised pad changes bits) and table[c][255] =
    1e30 (a byte read beside a patch or beside the images blows the embedding up)."""
    g = torch.Generator().manual_seed(100 + seed)
    t = torch.randn((n_chan, 256), generator=g)
    t[:, 0] = 0.5 + torch.arange(n_chan, dtype=torch.float32)
    t[:, 255] = POISON
    return t


def plain_table(n_chan, seed=0):
    """(n_chan, 256) float32, random per channel with table[c][0] != 0: for images that use all 256 byte values."""
    t = guard_table(n_chan, seed)
    t[:, 255] = -0.25 - torch.arange(n_chan, dtype=torch.float32)
    return t


def guarded_images_u8(g, k, seed=0, device="cpu"):
    """(B, C, H, W) uint8: pixels some patch covers are seeded bytes in 0..254, pixels no patch covers (leftover rows /
    columns, the gaps of a stride above the patch) are 255, as the slice buf[GUARD + k : ...] of a larger buffer of 255 that
    starts at a 16-byte boundary - so the images start k bytes past one."""
    b, c, h, w, (ph, pw), (sh, sw) = g
    ny, nx = grid(g)
    gen = np.random.default_rng(seed + 7 * h + w)
    img = gen.integers(0, 255, size=(b, c, h, w), dtype=np.uint8)
    rows = np.zeros(h, dtype=bool)
    cols = np.zeros(w, dtype=bool)
    for py in range(ny):
        rows[py * sh:py * sh + ph] = True
    for px in range(nx):
        cols[px * sw:px * sw + pw] = True
    img[:, :, ~rows, :] = 255
    img[:, :, :, ~cols] = 255
    buf = torch.full((GUARD + img.size + GUARD + 16,), 255, dtype=torch.uint8, device=device)
    assert buf.data_ptr() % 16 == 0 and GUARD % 16 == 0
    flat = buf[GUARD + k:GUARD + k + img.size]
    flat.copy_(torch.from_numpy(img).reshape(-1))
    return flat.view(b, c, h, w)


def expected_tier(kind, g, k):
    """The width the launcher must pick for images k bytes past a 16-byte boundary: the widest of the kernel's list that
    divides the address, the row pitch w and the column stride sw - worked out here from the numbers, not from the code."""
    w, sw = g[3], g[5][1]
    for wd in TIERS[kind]:
        if k % wd == 0 and w % wd == 0 and sw % wd == 0:
            return wd
    raise AssertionError("the byte tier takes anything")


# the tier of each geometry of view_cases' lattice at k = 0, written out: {(w, sw): tier}
FUSED_AT_0 = {(128, 32): 16, (112, 16): 16, (117, 20): 1, (128, 6): 1, (140, 36): 4}
POOL50_AT_0 = {(200, 50): 2, (175, 25): 1, (203, 17): 1}
POOL100_AT_0 = {(300, 100): 4, (300, 50): 1, (301, 67): 1}
