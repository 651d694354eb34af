"""Shared by tests/test_patch_view_cpu.py and tests/test_patch_view.py: the geometry lattice of the patch-grid view and
its guarded inputs."""

import numpy as np
import torch

# stem -> [(B, C, H, W, (ph, pw), (sh, sw))]
FUSED = [
    (1, 1, 96, 128, (32, 32), (32, 32)),     # 12 patches: one eight-patch workgroup + the pair kernel's remainder
    (1, 1, 80, 112, (32, 32), (16, 16)),     # overlap
    (1, 1, 100, 117, (32, 32), (24, 20)),    # leftovers, W % 4 != 0
    (1, 1, 104, 128, (32, 32), (32, 6)),     # sw % 4 != 0
    (1, 1, 112, 140, (32, 32), (40, 36)),    # gaps
    (3, 1, 96, 128, (32, 32), (32, 32)),     # B = 3
]
FUSED_ROUND = (1, 1, 392, 392, (32, 32), (8, 8))          # 2,116 patches: a whole round of 256 units + 68
POOL50 = [
    (1, 1, 150, 200, (50, 50), (50, 50)),
    (1, 1, 125, 175, (50, 50), (25, 25)),
    (1, 1, 151, 203, (50, 50), (25, 17)),
]
POOL50_CUT = (1, 1, 825, 850, (50, 50), (25, 25))         # 1,056 patches: across the two-stream cut at 1,024
POOL100 = [
    (2, 3, 200, 300, (100, 100), (100, 100)),
    (1, 3, 200, 300, (100, 100), (50, 50)),
    (1, 3, 200, 301, (100, 100), (100, 67)),
]
GENERIC = (1, 3, 120, 150, (37, 45), (37, 45))
ALL = FUSED + [FUSED_ROUND] + POOL50 + [POOL50_CUT] + POOL100 + [GENERIC]


def geom_id(g):
    b, c, h, w, (ph, pw), (sh, sw) = g
    return "b%d_c%d_%dx%d_p%dx%d_s%dx%d" % (b, c, h, w, ph, pw, sh, sw)


def grid(g):
    b, c, h, w, (ph, pw), (sh, sw) = g
    return (h - ph) // sh + 1, (w - pw) // sw + 1


def guarded_images(g, k, seed=0, device="cpu"):
    """(B, C, H, W) seeded normal floats whose pixels that no patch covers (leftover rows / columns, the gaps of a stride
    above the patch) are NaN, as a slice buf[k : k + numel] of a larger NaN-filled buffer: k = 0 an aligned base, k = 1 a
    base 4 bytes off.  A read outside a patch or outside the images changes bits or breaks finiteness."""
    b, c, h, w, (ph, pw), (sh, sw) = g
    ny, nx = grid(g)
    gen = np.random.default_rng(seed + 7 * h + w)
    img = gen.standard_normal((b, c, h, w)).astype(np.float32)
    rows = np.zeros(h, dtype=bool)
    cols = np.zeros(w, dtype=bool)
    for py in range(ny):
        rows[py * sh:py * sh + ph] = True
    for px in range(nx):
        cols[px * sw:px * sw + pw] = True
    img[:, :, ~rows, :] = np.nan
    img[:, :, :, ~cols] = np.nan
    guard = 4096
    buf = torch.full((guard + img.size + guard + 8,), float("nan"), dtype=torch.float32, device=device)
    flat = buf[guard + k:guard + k + img.size]
    flat.copy_(torch.from_numpy(img).reshape(-1))
    return flat.view(b, c, h, w)


def unfold(images, patch, stride):
    """The reference datasets' unfold (mnist_dataset.py:44-51), batched: (B, C, H, W) -> (B, N, C, ph, pw)."""
    p = images.unfold(2, patch[0], stride[0]).unfold(3, patch[1], stride[1]).permute(0, 2, 3, 1, 4, 5)
    return p.reshape(images.shape[0], -1, images.shape[1], patch[0], patch[1]).contiguous()
