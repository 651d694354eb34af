"""Slides of different lengths in one ``ips()`` call.

The reference batches only what has the same number of patches per image; its CAMELYON configuration therefore runs
``B: 16, B_seq: 1`` (config/camelyon_config.yml:3-4): sixteen solo ``ips()`` calls per step.  ``Ragged`` holds the slides
of a call one after the other, ``collate_ragged`` makes one from a loader's samples, and ``ips_ragged`` selects in all of
them at once.  The contract is the solo calls': slide by slide and bit for bit what

    for b in range(B): out[b] = net.ips(slides[b][None])

returns and leaves behind, with torch's RNG streams consumed as that loop consumes them.  On a ROCm device that is one
encoder pass over all rows, one packed logits table, ONE selection-loop launch (``ipsx_scan_ragged``: the loop kernels on
per-slide lengths) and the gathers over global rows; on a CPU device it is that loop.
"""

import os

import torch

from . import hip
from .shuffle import draw_shuffle


class Ragged:
    """The slides of a call, one after the other: ``rows`` (sum N_b, F) | (sum N_b, C, h, w), contiguous; ``lengths`` the
    host ints N_b.  ``offsets`` is their int64 prefix sum (B + 1,) on the rows' device, made once and kept."""

    def __init__(self, rows, lengths):
        lengths = tuple(int(n) for n in lengths)
        if not torch.is_tensor(rows) or rows.dim() not in (2, 4):
            raise TypeError("Ragged rows are a (sum N_b, F) or (sum N_b, C, h, w) tensor")
        if any(n < 0 for n in lengths) or sum(lengths) != rows.shape[0]:
            raise ValueError("lengths {} do not add up to the {} rows".format(lengths, rows.shape[0]))
        self.rows = rows if rows.is_contiguous() else rows.contiguous()
        self.lengths = lengths
        starts = [0]
        for n in lengths:
            starts.append(starts[-1] + n)
        self.starts = tuple(starts)                      # the prefix sum as host ints
        self._cache = {}                                 # device -> [offsets, row_base]: shared with the copies ``to()`` makes

    @classmethod
    def from_list(cls, slides):
        """[(N_0, ...), (N_1, ...), ...] tensors of one row shape, dtype and device -> Ragged (the rows are joined once)."""
        slides = list(slides)
        if not slides:
            return cls(torch.empty((0, 0)), ())
        first = slides[0]
        for k, s in enumerate(slides):
            if not torch.is_tensor(s) or s.dim() not in (2, 4) or s.shape[1:] != first.shape[1:] or s.dtype != first.dtype \
                    or s.device != first.device:
                raise TypeError("slide {}: every slide is a (N_b, F) or (N_b, C, h, w) tensor of one row shape, dtype and device".format(k))
        return cls(torch.cat(slides, 0), [s.shape[0] for s in slides])

    def __len__(self):
        return len(self.lengths)

    def __getitem__(self, b):
        """Slide ``b``: a (N_b, ...) view of the rows."""
        b = range(len(self.lengths))[b]
        return self.rows[self.starts[b]:self.starts[b + 1]]

    def __iter__(self):
        return (self[b] for b in range(len(self)))

    @property
    def offsets(self):
        """(B + 1,) int64 prefix sum of the lengths on the rows' device - made once per device and kept with the object."""
        slot = self._cache.setdefault(self.rows.device, [None, None])
        if slot[0] is None:
            slot[0] = torch.tensor(self.starts, dtype=torch.int64).to(self.rows.device)
        return slot[0]

    @property
    def device(self):
        return self.rows.device

    @property
    def dtype(self):
        return self.rows.dtype

    @property
    def total(self):
        return self.starts[-1]

    def _like(self, rows):
        if rows is self.rows:
            return self
        r = Ragged.__new__(Ragged)
        r.rows, r.lengths, r.starts, r._cache = rows, self.lengths, self.starts, self._cache
        return r

    def to(self, *args, **kwargs):
        """``Tensor.to`` on the rows (device and / or dtype, ``non_blocking=``); the lengths stay on the host."""
        return self._like(self.rows.to(*args, **kwargs))

    def pin_memory(self):
        return self._like(self.rows.pin_memory())

    def row_base(self):
        """(sum N_b,) int64 on the rows' device: the first row of the slide every row belongs to.  Made once and kept."""
        offsets = self.offsets
        slot = self._cache[self.rows.device]
        if slot[1] is None:
            slot[1] = torch.repeat_interleave(offsets[:-1], torch.tensor(self.lengths, dtype=torch.int64).to(self.device),
                                              output_size=self.total)
        return slot[1]

    def __repr__(self):
        return "Ragged(rows={}, lengths={}, dtype={}, device={})".format(tuple(self.rows.shape), self.lengths, self.dtype, self.device)


def collate_ragged(samples):
    """A ``DataLoader`` ``collate_fn`` for the datasets' ``{'input': (N, ...), task: label}`` samples whose inputs differ in
    length: ``'input'`` becomes a ``Ragged``, everything else is collated as ``default_collate`` does."""
    from torch.utils.data import default_collate
    rest = default_collate([{k: v for k, v in s.items() if k != 'input'} for s in samples])
    rest['input'] = Ragged.from_list([torch.as_tensor(s['input']) for s in samples])
    return rest


def refuse(what):
    """``ips_stream()`` feeds and ``dist.ips_sharded`` take tensors of one length per image."""
    raise TypeError("{} takes (B, N, ...) tensors: a Ragged batch goes through IPSNet.ips_ragged".format(what))


def _check(net, slides):
    """Everything ``ips_ragged`` refuses, before the first launch and before the first random number is drawn."""
    if len(slides) == 0:
        raise ValueError("ips_ragged: an empty batch")
    if slides.dtype == torch.uint8:
        raise TypeError("ips_ragged reads float32 rows (float16 / bfloat16 where ips() takes them): uint8 patch storage goes "
                        "through ips() slide by slide")
    if hip.dedup_blank():                      # (as streams do: whatever the device)
        raise TypeError("blank-patch dedup needs batches of one length (IPSX_DEDUP_BLANK=1 with ips_ragged)")
    if slides.rows.dim() != (4 if net.is_image else 2):
        raise TypeError("ips_ragged: {} rows for {}".format(tuple(slides.rows.shape), "an image encoder ((sum N_b, C, h, w))" if net.is_image
                                                            else "a feature net ((sum N_b, F))"))
    for b, n in enumerate(slides.lengths):
        if n <= net.M:
            raise ValueError("slide {} has {} rows and the memory M = {}: the reference returns all {} of them there, the "
                             "batch would not be rectangular (select such a slide with ips())".format(b, n, net.M, n))
        if net.use_pos and n > net.pos_enc.shape[1]:
            raise ValueError("slide {} has {} rows, the positional table conf.N = {}".format(b, n, net.pos_enc.shape[1]))
        if (net.use_pos and net.shuffle and net.shuffle_style == 'instance' and not net._shuffle_overridden()
                and n != net.pos_enc.shape[1]):
            # (shuffle_instance gathers the WHOLE table with the slide's permutation: ips() on this slide alone raises)
            raise ValueError("slide {} has {} rows: shuffle_style 'instance' with use_pos needs slides of exactly conf.N = {} "
                             "rows, as ips() does".format(b, n, net.pos_enc.shape[1]))


def _solo_loop(net, slides):
    """The loop the contract names - the CPU plumbing path (``_select_aten`` per slide), and a ROCm device whose encoder is
    in training mode inside an eval-mode net (batch statistics: no per-row function)."""
    patch, pos, idx, emb, shuf = [], [], [], [], []
    for b in range(len(slides)):
        p, q = net._call(slides[b].unsqueeze(0))
        patch.append(p)
        pos.append(q)
        idx.append(net.last_mem_idx)
        emb.append(net.last_mem_emb)
        shuf.append(net.last_shuffle)
    net.last_mem_idx = torch.cat(idx, 0)
    net._emb_parts, net._ragged_rows = None, None
    net._mem_emb = torch.cat(emb, 0) if all(e is not None for e in emb) else None
    net.last_shuffle = shuf if net.shuffle and any(s is not None for s in shuf) else None
    return torch.cat(patch, 0), (torch.cat(pos, 0) if net.use_pos else None)


def _draw(net, slides):
    """The permutations of a shuffled call, slide by slide in slide order, by the calls ``IPSNet._shuffle`` makes for a
    (1, N_b, ...) input on the device the slides were handed over on -> (perms | None, copies | None): ``perms`` the B
    (N_b,) permutations as drawn; an overridden ``do_shuffle`` is called as ever and returns shuffled COPIES
    [(rows_b, pos_b)] instead (nothing is kept in ``last_shuffle`` then, as in ``ips()``)."""
    if net._shuffle_overridden():
        copies = []
        for b in range(len(slides)):
            x, p = net.do_shuffle(slides[b].unsqueeze(0), net.pos_enc if net.use_pos else None)
            copies.append((x[0], p[0, :x.shape[1]] if torch.is_tensor(p) else None))
        return None, copies
    perms = []
    for b in range(len(slides)):
        perm = draw_shuffle(slides[b].unsqueeze(0), net.shuffle_style)
        if perm is None:                   # an unknown style: do_shuffle leaves everything as it is
            return None, None
        perms.append(perm.reshape(-1))
    return perms, None


def _index_ok(net, rows):
    """May the encoder read the packed rows through an int32 index (``Selection.index_supported`` for one piece)?"""
    if os.environ.get("IPSX_SHUFFLE", "index") == "copy":
        return False
    if not net.is_image:
        return rows.dtype in (torch.float32, torch.float16, torch.bfloat16)
    plan = net.plan
    return rows.dtype == torch.float32 and bool(plan.index_list_supported(rows.shape))


@torch.no_grad()
def ips_ragged(net, slides):
    """``IPSNet.ips_ragged``: see there."""
    if not isinstance(slides, Ragged):
        slides = Ragged.from_list(slides)
    _check(net, slides)
    device = net.device
    if not hip.on_device(device) or (net.encoder.training and not net.training):
        return _solo_loop(net, slides)

    B, M, D = len(slides), net.M, net.D
    lengths, total = slides.lengths, slides.total
    net._emb_parts = net._mem_emb = net.last_shuffle = net.last_mem_idx = net._ragged_rows = None
    with net._scoring():
        perms = copies = None
        if net.shuffle:
            # (drawn where the slides were handed over - a host-resident Ragged draws 'instance' permutations from the CPU
            #  generator, as its solo calls do)
            perms, copies = _draw(net, slides)
        dev = slides.to(device)                      # a host-resident Ragged is copied whole
        rows, offsets = dev.rows, dev.offsets
        ca = net.transf.crs_attn
        vq, R = ca.folded_query(), ca.H * ca.n_token
        with net.plan.hold():
            flat = None                               # int32 (total,): packed row j of the call is row flat[j] of ``rows``
            local = None                              # int64 (total,): the position inside its slide of packed row j
            if perms is not None:
                local = torch.cat(perms).to(device)
                flat = (local + dev.row_base()).to(torch.int32)
                by_index = _index_ok(net, rows)
                # (what the solo calls keep: the device copy where they select through the index, else the permutation as drawn)
                net.last_shuffle = [(local[dev.starts[b]:dev.starts[b + 1]] if by_index else perms[b]).unsqueeze(0) for b in range(B)]
                if not by_index:
                    rows, flat = rows.index_select(0, flat), None
            elif copies is not None:
                rows = torch.cat([c[0] for c in copies], 0).to(device)
            # one encoder pass over all rows
            if flat is None:
                emb = net._embed(rows)
            elif net.is_image:
                emb = net.plan.encode_source(hip.PatchSource(rows, None), index=flat)
            else:
                emb = net.plan.encode(rows, index=flat)
            pos = None
            if net.use_pos:
                if copies is not None:
                    pos = torch.cat([c[1] for c in copies], 0).to(device)
                else:
                    if local is None:
                        local = torch.arange(total, dtype=torch.int64, device=device) - dev.row_base()
                    pos = net.pos_enc[0].index_select(0, local)          # positions restart at 0 in every slide
                pos = pos.unsqueeze(0)
            # one packed (total, R) logits table, ONE loop launch on per-slide lengths
            logits = hip.logits(emb.unsqueeze(0), pos, vq, R)[0]
            mem_idx = hip.scan_ragged(logits, offsets, lengths, M, net.I, ca.H, ca.n_token)
        # the gathers over global rows
        grow = (mem_idx + offsets[:-1].unsqueeze(1)).reshape(1, B * M)
        src_rows = grow if flat is None else flat.index_select(0, grow[0]).to(torch.int64).unsqueeze(0)
        mem_patch = hip.gather_rows(rows.unsqueeze(0), src_rows).view(B, M, *rows.shape[1:])
        mem_pos = hip.gather_rows(pos, grow).view(B, M, D) if net.use_pos else None
    net._emb_parts, net._ragged_rows = [emb.unsqueeze(0)], (grow, mem_idx)
    net.last_mem_idx = mem_idx
    return mem_patch, mem_pos
