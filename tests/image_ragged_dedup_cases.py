"""Shared by tests/test_image_ragged_dedup_cpu.py and tests/test_image_ragged_dedup.py: images of different sizes whose
content is mostly zero, packed as ``image_ragged_cases.guarded_ragged`` packs them - NaN in every pixel no patch covers,
between the images and around the buffer - and the host's blank rule."""

import numpy as np
import torch

import image_ragged_cases as ic
from ips_amd.ragged_image import RaggedImages
from view_cases import unfold

# name -> (C, [(H, W)], (ph, pw), (sh, sw)): FUSED_MIXED's and FUSED_ALIGNED's load paths, and windows that overlap
STRIDE16 = (1, [(96, 128), (100, 116), (48, 64)], (32, 32), (16, 16))      # 35 + 30 + 6 patches, every width a multiple of 4


def zero_images(case):
    """The host images of ``case``: +0.0 wherever a patch window lies, NaN in the leftover rows and columns."""
    c, sizes, (ph, pw), (sh, sw) = case
    out = []
    for (h, w), (ny, nx) in zip(sizes, ic.grids(case)):
        im = torch.full((c, h, w), float("nan"), dtype=torch.float32)
        rows, cols = torch.zeros(h, dtype=torch.bool), torch.zeros(w, dtype=torch.bool)
        for py in range(ny):
            rows[py * sh:py * sh + ph] = True
        for px in range(nx):
            cols[px * sw:px * sw + pw] = True
        im[:, rows[:, None] & cols[None, :]] = 0.0
        out.append(im)
    return out


def window(case, b, p):
    """(y0, x0) of grid patch ``p`` of image ``b``."""
    ny, nx = ic.grids(case)[b]
    return (p // nx) * case[3][0], (p % nx) * case[3][1]


def fill_windows(case, imgs, packed, seed=0):
    """Seeded normal content (never 0) in the windows of the packed patches ``packed``."""
    gen = np.random.default_rng(seed)
    firsts = np.cumsum([0] + [ny * nx for ny, nx in ic.grids(case)])
    (ph, pw) = case[2]
    for p in packed:
        b = int(np.searchsorted(firsts, p, side="right")) - 1
        y0, x0 = window(case, b, p - int(firsts[b]))
        v = gen.standard_normal((case[0], ph, pw)).astype(np.float32)
        v[v == 0] = 1.0
        imgs[b][:, y0:y0 + ph, x0:x0 + pw] = torch.from_numpy(v)
    return imgs


def pack(case, imgs, k=0, device="cpu"):
    """``imgs`` at 16-byte offsets inside a slice buf[guard + k :] of a NaN-filled buffer (k = 1: a base 4 bytes off), the
    gaps NaN -> (RaggedImages, [the (C, H, W) images on ``device``])."""
    c, sizes, patch, stride = case
    offs, end = ic.offsets16(case)
    guard = 4096
    buf = torch.full((guard + end + guard + 8,), float("nan"), dtype=torch.float32, device=device)
    pixels = buf[guard + k:guard + k + end]
    on_dev = []
    for im, o in zip(imgs, offs):
        pixels[o:o + im.numel()].view(im.shape).copy_(im)
        on_dev.append(im.to(device))
    return RaggedImages(pixels, c, sizes, offs), on_dev


def flat_patches(imgs, patch, stride):
    """The patches of every image in unfold order, one image after the other: (total, C, ph, pw)."""
    return torch.cat([unfold(im[None], patch, stride)[0] for im in imgs]).contiguous()


def host_flags(patches):
    """The blank rule on the host: (n,) int32, 1 where a patch has a bit set outside the sign bit (-0.0 is zero, a denormal
    is not)."""
    bits = patches.contiguous().view(torch.int32).reshape(patches.shape[0], -1)
    return ((bits & 0x7FFFFFFF) != 0).any(dim=1).to(torch.int32)


def host_count(flags):
    """What the dedup route encodes of entries with these flags: the non-blank ones, and one blank one if there is any."""
    flags = flags.to(torch.int64)
    return int(flags.sum()) + (1 if int(flags.numel() - flags.sum()) > 0 else 0)


def planted_images(sizes, seed=5, keep=3):
    """Host float32 (1, H, W) images for the end-to-end calls at patch 32 / stride 32: seeded normal pixels, and every
    32 x 32 window whose (row + column) is no multiple of ``keep`` all-zero (two thirds of the patches blank)."""
    out = ic.make_images(sizes, seed=seed, blank=0.0)
    for im in out:
        for py in range(im.shape[1] // 32):
            for px in range(im.shape[2] // 32):
                if (py + px) % keep:
                    im[:, 32 * py:32 * py + 32, 32 * px:32 * px + 32] = 0.0
    return out
