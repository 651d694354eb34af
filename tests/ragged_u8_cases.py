"""Shared by tests/test_ragged_u8_cpu.py and tests/test_ragged_u8.py: uint8 images of different sizes packed into guarded
byte buffers (255 wherever no patch lies, between the images and around the buffer, as ``view_u8_cases`` guards one-size
images), their float32 expansion through the table, and the load width ("tier") every ragged launcher is expected to pick,
worked out from the numbers."""

import numpy as np
import torch

import image_ragged_cases as ic
from ips_amd.quant import dequant
from ips_amd.ragged_image import RaggedImages
from view_u8_cases import GUARD, TIERS

# name -> (C, [(H, W)], (ph, pw), (sh, sw)); every width and the stride a multiple of 16: the 16-byte tier at an aligned base
ALL16 = (1, [(96, 128), (100, 112), (32, 32), (160, 64)], (32, 32), (32, 32))


def byte_offsets(case, shifts=None):
    """Byte (= element) offsets of the images of ``case`` one after the other, each at a multiple of 16 bytes plus its
    entry of ``shifts`` (default: none) -> (offsets, end)."""
    c, sizes = case[0], case[1]
    shifts = shifts or [0] * len(sizes)
    offs, end = [], 0
    for (h, w), s in zip(sizes, shifts):
        offs.append((end + 15) // 16 * 16 + s)
        end = offs[-1] + c * h * w
    return offs, end


def covered(case, b):
    """(H, W) bool: the pixels of image ``b`` that some patch window covers."""
    c, sizes, (ph, pw), (sh, sw) = case
    (h, w), (ny, nx) = sizes[b], ic.grids(case)[b]
    rows, cols = np.zeros(h, dtype=bool), np.zeros(w, dtype=bool)
    for py in range(ny):
        rows[py * sh:py * sh + ph] = True
    for px in range(nx):
        cols[px * sw:px * sw + pw] = True
    return rows[:, None] & cols[None, :]


def guarded_images_u8(case, seed=0, zero=False):
    """The host uint8 (C, H, W) images of ``case``: seeded bytes 0..254 (``zero``: 0) where a patch window lies, 255 elsewhere."""
    c, sizes = case[0], case[1]
    out = []
    for b, (h, w) in enumerate(sizes):
        gen = np.random.default_rng(seed + 13 * b + 7 * h + w)
        im = np.zeros((c, h, w), dtype=np.uint8) if zero else gen.integers(0, 255, size=(c, h, w), dtype=np.uint8)
        im[:, ~covered(case, b)] = 255
        out.append(torch.from_numpy(im))
    return out


def pack_u8(case, imgs, k=0, shifts=None, device="cpu"):
    """``imgs`` at ``byte_offsets(case, shifts)`` inside the slice buf[GUARD + k :] of a buffer of 255 that starts at a 16-byte
    boundary: the base lies k bytes past one, the gaps between the images are 255 -> (RaggedImages, offsets)."""
    c, sizes = case[0], case[1]
    offs, end = byte_offsets(case, shifts)
    buf = torch.full((GUARD + end + GUARD + 16,), 255, dtype=torch.uint8, device=device)
    assert buf.data_ptr() % 16 == 0
    pixels = buf[GUARD + k:GUARD + k + end]
    for im, o in zip(imgs, offs):
        pixels[o:o + im.numel()].view(im.shape).copy_(im)
    return RaggedImages(pixels, c, sizes, offs), offs


def expanded(images, table):
    """The float32 ``RaggedImages`` ``table[c][byte]`` of a uint8 one: the same offsets in ELEMENTS (so 4 x the bytes), NaN
    between the images."""
    px = torch.full((images.pixels.numel(),), float("nan"), dtype=torch.float32, device=images.device)
    out = RaggedImages(px, images.channels, images.sizes, images.elem_offsets, images.pad)
    for b in range(len(images)):
        out[b].copy_(dequant(images[b], table.to(images.device)))
    return out


def expected_tier(kind, k, offs, case):
    """The widest entry of the kernel's byte list that divides the base address (k bytes past a 16-byte boundary), every
    image's byte offset, every row pitch and the column stride - from the numbers, not from the code."""
    widths, sw = [w for _, w in case[1]], case[3][1]
    for wd in TIERS[kind]:
        if k % wd == 0 and sw % wd == 0 and all(o % wd == 0 for o in offs) and all(w % wd == 0 for w in widths):
            return wd
    raise AssertionError("the byte tier takes anything")


def byte_images(sizes, c=1, seed=5, blank=0.5):
    """Host uint8 (C, H, W) images for the end-to-end calls: seeded bytes over all 256 values, a share of them 0."""
    out = []
    for k, (h, w) in enumerate(sizes):
        gen = np.random.default_rng(seed + 31 * k)
        im = gen.integers(0, 256, size=(c, h, w), dtype=np.uint8)
        im[gen.random((c, h, w)) < blank] = 0
        out.append(torch.from_numpy(im))
    return out
