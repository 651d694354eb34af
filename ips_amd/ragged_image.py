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

import os

import torch
from torch import nn

from . import hip
from .ragged import _check, ips_ragged
from .shuffle import draw_shuffle


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


class _Grids:
    """The grids of a call as ``ragged._check`` reads slides: "rows" are grid patches."""

    class _Rows:
        @staticmethod
        def dim():
            return 4
        shape = ("sum ny_b nx_b", "C", "ph", "pw")

    def __init__(self, lengths, dtype, channels):
        self.lengths, self.dtype, self.channels, self.rows = tuple(lengths), dtype, channels, self._Rows()

    def __len__(self):
        return len(self.lengths)


class _Drawn:
    """What ``draw_shuffle`` reads of the (1, N_b, ...) patches of an image: their shape and device."""

    def __init__(self, n, device):
        self.shape, self.device = (1, n), device


def _encoder_channels(net):
    for m in net.encoder.modules():
        if isinstance(m, nn.Conv2d):
            return m.in_channels
    return None


def _draw(net, lengths, device, skip):
    """The permutations of a shuffled call, image by image in image order, by the calls ``IPSNet._shuffle`` makes for the
    (1, N_b, ...) patches of one image on ``device`` -> [(N_b,) permutation as drawn] | None (``ragged._draw`` on grids:
    nothing is drawn for the images in ``skip``, they stay in grid order)."""
    perms = []
    for b, n in enumerate(lengths):
        if b in skip:
            perms.append(None)
            continue
        perm = draw_shuffle(_Drawn(n, device), net.shuffle_style)
        if perm is None:                   # an unknown style: do_shuffle leaves everything as it is
            return None
        perms.append(perm.reshape(-1))
    drawn = [p for p in perms if p is not None]
    if not drawn:
        return None
    return [torch.arange(lengths[b], dtype=torch.int64, device=drawn[0].device) if p is None else p for b, p in enumerate(perms)]


def ragged_dedup(env, plan, rview):
    """Does the packed encoder pass of ``_viewed_route`` take the exact blank-patch dedup (``encode_source(dedup=True)``,
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
    _check(net, _Grids(lengths, images.dtype, images.channels), pad)   # (uint8: a table of C rows, the exact trunk)
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
        out = ips_ragged(net, [net._materialise(images[b].unsqueeze(0), patch_size, patch_stride)[0] for b in range(len(images))], pad)
    else:
        out = _viewed_route(net, images, rview, short_ok=pad)
    net._mem_count = tuple(min(n, net.M) for n in lengths) if pad else None
    return out


def _viewed_route(net, images, rview, short_ok):
    """``ragged._device_route`` with the packed rows replaced by the packed grid patches of a ragged view: the encoder pass
    and the finish launch read the images where they lie."""
    B, M, device = len(images), net.M, net.device
    lengths = rview.lengths
    short = frozenset(b for b, n in enumerate(lengths) if n <= M)
    with net._scoring():
        ca = net.transf.crs_attn
        with net.plan.hold():
            dev = images.to(device)                      # a host-resident batch is copied whole
            # (drawn where the solo ips_image() calls draw: on the device the images are selected on)
            perms = _draw(net, lengths, device, short) if net.shuffle else None
            offsets = torch.tensor(rview.firsts + (rview.count,), dtype=torch.int64).to(device)
            base = torch.repeat_interleave(offsets[:-1], torch.tensor(lengths, dtype=torch.int64).to(device), output_size=rview.count)
            flat = local = None
            if perms is not None:
                local = torch.cat([p.to(device) for p in perms])
                flat = (local + base).to(torch.int32)    # packed grid numbers first_b + perm_b[j]
                by_index = os.environ.get("IPSX_SHUFFLE", "index") != "copy"
                net.last_shuffle = [None if b in short else (local[rview.firsts[b]:rview.firsts[b] + lengths[b]] if by_index else perms[b]).unsqueeze(0)
                                    for b in range(B)]
            table = net._table_for(dev)                  # (uint8 pixels: read through the table, never expanded)
            src = hip.PatchSource(images=dev.pixels, ragged=rview, table=table)
            # ONE encoder pass over all grid patches (the fused trunk: blank ones encoded once, the same bits)
            emb = net.plan.encode_source(src, index=flat, dedup=ragged_dedup(os.environ, net.plan, rview))
            pos = None
            if net.use_pos:
                if local is None:
                    local = torch.arange(rview.count, dtype=torch.int64, device=device) - base
                pos = net.pos_enc[0].index_select(0, local)          # positions restart at 0 in every image
            logits = hip.logits(emb.unsqueeze(0), pos.unsqueeze(0) if pos is not None else None, ca.folded_query(), ca.H * ca.n_token)[0]
            mem_idx = hip.scan_ragged(logits, offsets, lengths, M, net.I, ca.H, ca.n_token, short_ok=short_ok)
        mem_patch, mem_pos, mem_idx, grow = hip.ragged_finish_view(dev.pixels, rview, offsets, mem_idx, M, flat, pos, table=table)
    if net.last_shuffle is not None and all(s is None for s in net.last_shuffle):
        net.last_shuffle = None

    padded = any(lengths[b] < M for b in short)
    zero_shape = (1,) + rview.patch_shape

    def emb_of_slots():
        """(B, M, D): the packed pass's rows; the padding holds the embedding of ONE all-zero patch."""
        with torch.no_grad(), net._scoring(), net.plan.hold():
            out = hip.gather_rows(emb.unsqueeze(0), (grow.clamp(min=0) if padded else grow).view(1, B * M)).view(B, M, -1)
            if padded:
                zero = net._embed(torch.zeros(zero_shape, dtype=torch.float32, device=device))
                out = torch.where((grow < 0).unsqueeze(-1), zero.view(1, 1, -1), out)
        return out
    net.last_mem_idx = mem_idx
    net._emb_make = emb_of_slots
    return mem_patch, mem_pos
