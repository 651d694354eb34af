"""Shared by tests/test_image_ragged_cpu.py and tests/test_image_ragged.py: lists of images of different sizes, their guarded
pixels, and the contract of ``IPSNet.ips_image_ragged`` - image by image and bit for bit the loop of solo
``net.ips_image(image[None], ...)`` calls, with torch's RNG streams left where that loop leaves them."""

import numpy as np
import torch

from ips_amd.ragged_image import RaggedImages
from view_cases import guarded_images

# name -> (C, [(H, W)], (ph, pw), (sh, sw))
FUSED_MIXED = (1, [(96, 128), (100, 117), (32, 32), (160, 64)], (32, 32), (32, 32))       # W % 4 != 0: dword loads
FUSED_ALIGNED = (1, [(96, 128), (100, 116), (32, 32), (160, 64)], (32, 32), (32, 32))     # every width a multiple of 4: wide loads
FUSED_ROUND = (1, [(392, 392), (104, 168), (40, 48)], (32, 32), (8, 8))    # 2,116 + 180 + 6 = 2,302: a round of 256 units + the pair kernel
POOL50 = (1, [(150, 200), (125, 175), (151, 203), (50, 50)], (50, 50), (25, 25))
POOL50_CUT = (1, [(825, 850), (100, 75)], (50, 50), (25, 25))              # 1,056 + 6: across the two-stream cut at 1,024
POOL50_EVEN = (1, [(150, 200), (100, 76)], (50, 50), (25, 26))               # every width and the stride even: 8-byte loads
POOL100_WIDE = (3, [(200, 300), (100, 104)], (100, 100), (100, 100))       # every width a multiple of 4: 16-byte loads
POOL100 = (3, [(200, 300), (200, 301), (100, 100)], (100, 100), (100, 100))
POOL100_HALF = (3, [(200, 300), (200, 301), (100, 100)], (100, 100), (50, 50))
ONE = (1, [(96, 128)], (32, 32), (32, 32))                                 # B = 1
SEVENTEEN = (1, [(32 + 8 * (k % 5), 32 + 4 * (k % 7) + k) for k in range(17)], (32, 32), (8, 12))   # B = 17
TWO = (3, [(120, 150), (37, 45)], (37, 45), (20, 31))                      # B = 2, a generic patch shape
HOST_LISTS = {"one": ONE, "two": TWO, "seventeen": SEVENTEEN, "fused_mixed": FUSED_MIXED, "pool50": POOL50, "pool100": POOL100_HALF}


def grids(case):
    c, sizes, (ph, pw), (sh, sw) = case
    return [((h - ph) // sh + 1, (w - pw) // sw + 1) for h, w in sizes]


def offsets16(case, shift=0):
    """Element offsets of the images of ``case`` packed one after the other, each at a multiple of 16 bytes (+ ``shift``)."""
    c, sizes = case[0], case[1]
    offs, end = [], 0
    for h, w in sizes:
        offs.append((end + 3) // 4 * 4)
        end = offs[-1] + c * h * w
    return [o + shift for o in offs], end + shift


def guarded_ragged(case, k=0, seed=0, device="cpu"):
    """The images of ``case`` as ``view_cases.guarded_images`` makes them (NaN wherever no patch lies), packed at 16-byte
    offsets into a slice buf[guard + k :] of a NaN-filled buffer - k = 0 an aligned base, k = 1 a base 4 bytes off; the gaps
    between the images are NaN too -> (RaggedImages, [the (C, H, W) images])."""
    c, sizes, patch, stride = case
    offs, end = offsets16(case)
    guard = 4096
    buf = torch.full((guard + end + guard + 8,), float("nan"), dtype=torch.float32, device=device)
    pixels = buf[guard + k:guard + k + end]
    imgs = []
    for b, ((h, w), o) in enumerate(zip(sizes, offs)):
        im = guarded_images((1, c, h, w, patch, stride), 0, seed=seed + 13 * b, device=device)[0]
        pixels[o:o + im.numel()].view(im.shape).copy_(im)
        imgs.append(im.clone())
    return RaggedImages(pixels, c, sizes, offs), imgs


def make_images(sizes, c=1, seed=5, blank=0.5):
    """Host float32 images (C, H, W) for the end-to-end calls: seeded normal pixels, a share of them exactly 0."""
    out = []
    for k, (h, w) in enumerate(sizes):
        gen = np.random.default_rng(seed + 31 * k)
        im = gen.standard_normal((c, h, w)).astype(np.float32)
        im[gen.random((c, h, w)) < blank] = 0.0
        out.append(torch.from_numpy(im))
    return out


def _host(t):
    if t is None:
        return None
    if isinstance(t, (list, tuple)):
        return [_host(v) for v in t]
    return t.detach().cpu()


def _seed(seed):
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


def _rng():
    return torch.get_rng_state(), (torch.cuda.get_rng_state() if torch.cuda.is_available() else None)


def solo_loop(net, images, patch, stride, seed=11):
    """The loop of the contract over images longer than M -> everything it returns and leaves behind, on the host."""
    _seed(seed)
    patch_, pos, idx, emb, shuf = [], [], [], [], []
    for im in images:
        p, q = net.ips_image(im[None], patch, stride)
        patch_.append(_host(p))
        pos.append(_host(q))
        idx.append(_host(net.last_mem_idx))
        emb.append(_host(net.last_mem_emb))
        shuf.append(_host(net.last_shuffle))
    rng, rng_cuda = _rng()
    return {"mem_patch": torch.cat(patch_), "mem_pos": torch.cat(pos) if pos[0] is not None else None,
            "mem_idx": torch.cat(idx), "mem_emb": torch.cat(emb), "shuffle": shuf if shuf[0] is not None else None,
            "rng": rng, "rng_cuda": rng_cuda}


def record(net, out):
    rng, rng_cuda = _rng()
    return {"mem_patch": _host(out[0]), "mem_pos": _host(out[1]), "mem_idx": _host(net.last_mem_idx), "mem_emb": _host(net.last_mem_emb),
            "shuffle": _host(net.last_shuffle), "rng": rng, "rng_cuda": rng_cuda, "count": net.last_mem_count}


def image_call(net, images, patch, stride, seed=11, pad=False, through_ips_image=False):
    """``net.ips_image_ragged(images, ...)`` (``through_ips_image``: ``net.ips_image`` on the ``RaggedImages``) from the seed."""
    _seed(seed)
    if through_ips_image:
        return record(net, net.ips_image(RaggedImages.from_list(images, pad), patch, stride))
    return record(net, net.ips_image_ragged(images, patch, stride, pad=pad))


def patch_call(net, slides, seed=11, pad=False):
    """``net.ips_ragged(slides, pad=pad)`` on materialised patch tensors from the same seed -> the same record."""
    _seed(seed)
    return record(net, net.ips_ragged(slides, pad=pad))


def same_bits(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.is_floating_point:
        ints = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
        return torch.equal(a.contiguous().view(ints), b.contiguous().view(ints))
    return torch.equal(a, b)


def assert_same_padded(got, want):
    """Two records of padded calls (``shuffle`` entries may be None for short images)."""
    for key in ("mem_patch", "mem_pos", "mem_idx", "mem_emb"):
        if want[key] is None:
            assert got[key] is None, key
        else:
            assert got[key] is not None and same_bits(got[key], want[key]), key
    if want["shuffle"] is None:
        assert got["shuffle"] is None
    else:
        assert len(got["shuffle"]) == len(want["shuffle"])
        for b, (g, w) in enumerate(zip(got["shuffle"], want["shuffle"])):
            assert (g is None) == (w is None) and (g is None or (g.shape == w.shape and torch.equal(g, w))), "permutation of image {}".format(b)
    assert got["count"] == want["count"]
    assert torch.equal(got["rng"], want["rng"]), "the CPU generator's state"
    if want["rng_cuda"] is not None:
        assert torch.equal(got["rng_cuda"], want["rng_cuda"]), "the device generator's state"
