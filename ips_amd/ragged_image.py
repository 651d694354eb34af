"""Whole images of different sizes in one ``ips_image()`` call.

``ips_image()`` takes one (B, C, H, W) tensor: every image of a call has the same size.  ``RaggedImages`` holds images of
different sizes one after the other in ONE packed buffer, ``collate_ragged_images`` makes one from a loader's samples, and
``ips_image_ragged`` selects in all of them at once.  The contract is that of the existing routes, image by image and bit for
bit: what

    for b in range(B): out[b] = net.ips_image(images[b][None], patch_size, patch_stride)

returns and leaves behind - which is what ``net.ips_ragged([patchify(images[b]) for b], pad=pad)`` returns and leaves behind -
with torch's RNG streams consumed as that loop consumes them.  On a ROCm device whose stem reads a patch view that is ONE
encoder pass over the grid patches of all images, read where they lie through a ragged view (``hip.RaggedView``: no patch
tensor is made), one packed logits table, ONE selection-loop launch (``ipsx_scan_ragged``) and ONE finish launch
(``ipsx_ragged_finish_view``); everywhere else the patch tensors are materialised and ``ips_ragged`` runs unchanged.

uint8 images (after ``net.set_patch_table``): the same call on a quarter of the bytes - the stems, the blank scan and the
finish launch read the bytes where they lie through the table (the ``_u8`` exports); everything returned and left behind is,
bit for bit, that of the float32 images ``table[c][byte]``, which are never made, and ``mem_patch`` is float32.
"""

import functools
import os

import torch
from torch import nn

from . import hip
from .ragged import _check_facts, _device_route, _leave_count, ips_ragged


class RaggedImages:
    """The images of a call, one after the other: ``pixels`` ONE contiguous 1-d buffer; ``sizes`` the host (H_b, W_b) pairs;
    ``channels`` their common C; ``elem_offsets`` the element offset of every image inside the buffer (``from_list`` rounds
    them up to 16 bytes, so that wide loads stay possible).  ``pad``: what ``net.ips_image(images, ...)`` hands to
    ``ips_image_ragged`` - images with no more grid patches than the memory come back zero-padded to M slots."""

    def __init__(self, pixels, channels, sizes, elem_offsets, pad=False):
        sizes = tuple((int(h), int(w)) for h, w in sizes)
        offs = tuple(int(o) for o in elem_offsets)
        if not torch.is_tensor(pixels) or pixels.dim() != 1:
            raise TypeError("RaggedImages pixels are ONE 1-d buffer")
        channels = int(channels)
        if channels <= 0 or len(offs) != len(sizes) or any(h <= 0 or w <= 0 for h, w in sizes):
            raise ValueError("RaggedImages: {} channels, sizes {}, {} offsets".format(channels, sizes, len(offs)))
        end = 0
        for (h, w), o in zip(sizes, offs):
            if o < end:
                raise ValueError("RaggedImages: element offsets {} run into each other for sizes {}".format(offs, sizes))
            end = o + channels * h * w
        if end > pixels.numel():
            raise ValueError("RaggedImages: the images end at element {}, the buffer holds {}".format(end, pixels.numel()))
        self.pixels = pixels if pixels.is_contiguous() else pixels.contiguous()
        self.channels, self.sizes, self.elem_offsets, self.pad = channels, sizes, offs, bool(pad)
        self._views = {}                                 # (patch_size, patch_stride) -> hip.RaggedView: shared with the copies ``to()`` makes

    @classmethod
    def from_list(cls, images, pad=False):
        """[(C, H_0, W_0), (C, H_1, W_1), ...] tensors of one channel count, dtype and device -> RaggedImages (the pixels are
        joined once; every image starts at a multiple of 16 bytes)."""
        images = list(images)
        if not images:
            return cls(torch.empty((0,)), 1, (), (), pad)
        first = images[0]
        for k, im in enumerate(images):
            if not torch.is_tensor(im) or im.dim() != 3 or im.dtype != first.dtype or im.device != first.device:
                raise TypeError("image {}: every image is a (C, H_b, W_b) tensor of one dtype and device".format(k))
            if im.shape[0] != first.shape[0]:
                raise ValueError("image {} has {} channels, image 0 has {}".format(k, im.shape[0], first.shape[0]))
        unit = max(16 // first.element_size(), 1)
        offs, end = [], 0
        for im in images:
            offs.append((end + unit - 1) // unit * unit)
            end = offs[-1] + im.numel()
        pixels = torch.zeros((end,), dtype=first.dtype, device=first.device)
        for im, o in zip(images, offs):
            pixels[o:o + im.numel()].view(im.shape).copy_(im)
        return cls(pixels, first.shape[0], [im.shape[1:] for im in images], offs, pad)

    def __len__(self):
        return len(self.sizes)

    def __getitem__(self, b):
        """Image ``b``: a (C, H_b, W_b) view of the pixels."""
        b = range(len(self.sizes))[b]
        (h, w), o = self.sizes[b], self.elem_offsets[b]
        return self.pixels[o:o + self.channels * h * w].view(self.channels, h, w)

    def __iter__(self):
        return (self[b] for b in range(len(self)))

    @property
    def device(self):
        return self.pixels.device

    @property
    def dtype(self):
        return self.pixels.dtype

    def _like(self, pixels):
        if pixels is self.pixels:
            return self
        r = RaggedImages.__new__(RaggedImages)
        r.pixels, r.channels, r.sizes, r.elem_offsets, r.pad, r._views = pixels, self.channels, self.sizes, self.elem_offsets, self.pad, self._views
        return r

    def to(self, *args, **kwargs):
        """``Tensor.to`` on the pixels (device and / or dtype, ``non_blocking=``); sizes and offsets stay on the host."""
        return self._like(self.pixels.to(*args, **kwargs))

    def pin_memory(self):
        return self._like(self.pixels.pin_memory())

    def grids(self, patch_size, patch_stride):
        """[(ny_b, nx_b)] of the patch grid over every image; ValueError where a patch or stride does not fit an image."""
        (ph, pw), (sh, sw) = (int(v) for v in patch_size), (int(v) for v in patch_stride)
        out = []
        for b, (h, w) in enumerate(self.sizes):
            if min(ph, pw, sh, sw) <= 0 or ph > h or pw > w:
                raise ValueError("patch {}x{} / stride {}x{} does not fit image {} of {}x{}".format(ph, pw, sh, sw, b, h, w))
            out.append(((h - ph) // sh + 1, (w - pw) // sw + 1))
        return out

    def view(self, patch_size, patch_stride):
        """The ``hip.RaggedView`` of this geometry (its table is built and checked once and kept with the object)."""
        key = (tuple(int(v) for v in patch_size), tuple(int(v) for v in patch_stride))
        if key not in self._views:
            self._views[key] = hip.RaggedView(self.channels, self.sizes, self.elem_offsets, *key)
        return self._views[key]

    def __repr__(self):
        return "RaggedImages(channels={}, sizes={}, dtype={}, device={}{})".format(self.channels, self.sizes, self.dtype, self.device,
                                                                                   ", pad=True" if self.pad else "")


def collate_ragged_images(samples, pad=False):
    """A ``DataLoader`` ``collate_fn`` for ``{'input': (C, H, W) image, task: label}`` samples whose images differ in size:
    ``'input'`` becomes a ``RaggedImages``, everything else is collated as ``default_collate`` does."""
    from torch.utils.data import default_collate
    rest = default_collate([{k: v for k, v in s.items() if k != 'input'} for s in samples])
    rest['input'] = RaggedImages.from_list([torch.as_tensor(s['input']) for s in samples], pad)
    return rest


def _encoder_channels(net):
    for m in net.encoder.modules():
        if isinstance(m, nn.Conv2d):
            return m.in_channels
    return None


def ragged_dedup(env, plan, rview):
    """Does the packed encoder pass of ``_ViewSource`` take the exact blank-patch dedup (``encode_source(dedup=True)``,
    DESIGN 2.8)?  A function of the environment (a mapping), the net's ``EncoderPlan`` and the call's ``hip.RaggedView``
    alone: under ``IPSX_DEDUP_BLANK`` unset or ``auto`` (``0``: plain launches; ``1`` never gets here, ``ragged._check``
    refuses it), and only where the plan's trunk for the view's patch shape is the fused 1x32x32 one - the layered trunks
    have no such route and run plain.  On by default by measurement: dense images pay 0.03 / 0.18 ms of a 7.3 / 27.4 ms call
    at stride 32 / 16, inside the parent's max - min of 0.23 / 0.55 ms (profiles/ips_image_ragged_dedup_dense.json)."""
    if env.get("IPSX_DEDUP_BLANK", "auto") != "auto":
        return False
    return bool(plan.fused(rview.patch_shape))


@torch.no_grad()
def ips_image_ragged(net, images, patch_size, patch_stride, pad=False):
    """``IPSNet.ips_image_ragged``: see there."""
    pad = bool(pad)
    if not net.is_image:
        raise TypeError("ips_image_ragged takes (C, H_b, W_b) images of an image encoder")
    if not isinstance(images, RaggedImages):
        images = RaggedImages.from_list(images, pad)
    if len(images) == 0:
        raise ValueError("ips_image_ragged: an empty batch")
    c_in = _encoder_channels(net)
    if c_in is not None and images.channels != c_in:
        raise ValueError("images have {} channels, the encoder expects {}".format(images.channels, c_in))
    grids = images.grids(patch_size, patch_stride)
    lengths = tuple(ny * nx for ny, nx in grids)
    # ("rows" are grid patches; uint8: a table of C rows, the exact trunk)
    _check_facts(net, lengths, images.dtype, (sum(lengths), images.channels) + tuple(int(v) for v in patch_size), pad)
    net._reset_last()

    rview = None
    if (hip.on_device(net.device) and images.dtype in (torch.float32, torch.uint8)
            and not (net.encoder.training and not net.training)           # (the selection itself puts a training NET into eval mode)
            and not (net.shuffle and net._shuffle_overridden())
            and any(n > net.M for n in lengths)
            and not (net.use_pos and (net.D * net.pos_enc.element_size()) % 16)):
        rview = images.view(patch_size, patch_stride)
        if not net.plan.ragged_view_supported(rview):
            rview = None
    if rview is None:
        # the patch tensors, image by image, and the ragged call unchanged: it refuses what it refuses
        return ips_ragged(net, [net._materialise(images[b].unsqueeze(0), patch_size, patch_stride)[0] for b in range(len(images))], pad)
    out = _device_route(net, _ViewSource(net, images.to(net.device).pixels, rview), short_ok=pad)   # (a host-resident batch is copied whole)
    _leave_count(net, lengths, pad)
    return out


class _ViewSource:
    """What ``ragged._device_route`` selects in, for ``ips_image_ragged``: the grid patches of the images in ``pixels`` (on the
    device) through their ``hip.RaggedView``, read where they lie - no patch tensor is made, so ``rows`` is None."""
    rows = None

    def __init__(self, net, pixels, rview):
        self.net, self.pixels, self.rview = net, pixels, rview
        self.draw_device = net.device                        # (where the solo ips_image() calls draw)
        self.lengths, self.starts = rview.lengths, rview.firsts + (rview.count,)
        self.row_shape, self.dtype = rview.patch_shape, pixels.dtype

    @functools.cached_property
    def offsets(self):
        return torch.tensor(self.starts, dtype=torch.int64).to(self.net.device)

    def row_base(self):
        return torch.repeat_interleave(self.offsets[:-1], torch.tensor(self.lengths, dtype=torch.int64).to(self.net.device),
                                       output_size=self.rview.count)

    def through_index(self, flat):
        """A view is always read through the index; ``IPSX_SHUFFLE=copy`` decides only what ``last_shuffle`` keeps."""
        return os.environ.get("IPSX_SHUFFLE", "index") != "copy", flat

    def encode(self, flat=None):
        """ONE encoder pass over all grid patches (uint8: through the table, never expanded), or over the patches ``flat``; on
        the fused trunk blank ones are encoded once, the same bits."""
        src = hip.PatchSource(images=self.pixels, ragged=self.rview, table=self.net._table_for(self.pixels))
        return self.net.plan.encode_source(src, index=flat, dedup=ragged_dedup(os.environ, self.net.plan, self.rview))

    def finish(self, offsets, mem_idx, flat, pos):
        """ONE launch (``ipsx_ragged_finish_view``): the kept patches are copied out of their images."""
        return hip.ragged_finish_view(self.pixels, self.rview, offsets, mem_idx, self.net.M, flat, pos, table=self.net._table_for(self.pixels))
