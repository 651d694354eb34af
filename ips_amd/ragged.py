"""Slides of different lengths in one ``ips()`` call.

The reference batches only what has the same number of patches per image; its CAMELYON configuration therefore runs
``B: 16, B_seq: 1`` (config/camelyon_config.yml:3-4): sixteen solo ``ips()`` calls per step.  ``Ragged`` holds the slides
of a call one after the other, ``collate_ragged`` makes one from a loader's samples, and ``ips_ragged`` selects in all of
them at once.  The contract is the solo calls': slide by slide and bit for bit what

    for b in range(B): out[b] = net.ips(slides[b][None])

returns and leaves behind, with torch's RNG streams consumed as that loop consumes them.  On a ROCm device that is one
encoder pass over all rows, one packed logits table, ONE selection-loop launch (``ipsx_scan_ragged``: the loop kernels on
per-slide lengths) and ONE finish launch (``ipsx_ragged_finish``); on a CPU device it is that loop.

``pad=True`` takes slides with no more rows than the memory as well: the reference's ``ips()`` returns all N_b rows of such a
slide, unshuffled, and ``fill_batch`` (training/iterative.py) writes them into zero-initialised (B, M, ...) buffers - that
batch is what the padded call returns, by the same route: a call without ``pad`` is the padded call with no short slide,
and the finish launch also writes the zero padding.
"""

import os

import torch

from . import hip
from .shuffle import draw_shuffle_for


class Ragged:
    """The slides of a call, one after the other: ``rows`` (sum N_b, F) | (sum N_b, C, h, w), contiguous; ``lengths`` the
    host ints N_b.  ``offsets`` is their int64 prefix sum (B + 1,) on the rows' device, made once and kept.  ``pad``: what
    ``net.ips(ragged)`` hands to ``ips_ragged`` - slides with N_b <= M come back zero-padded to M rows."""

    def __init__(self, rows, lengths, pad=False):
        lengths = tuple(int(n) for n in lengths)
        if not torch.is_tensor(rows) or rows.dim() not in (2, 4):
            raise TypeError("Ragged rows are a (sum N_b, F) or (sum N_b, C, h, w) tensor")
        if any(n < 0 for n in lengths) or sum(lengths) != rows.shape[0]:
            raise ValueError("lengths {} do not add up to the {} rows".format(lengths, rows.shape[0]))
        self.rows = rows if rows.is_contiguous() else rows.contiguous()
        self.lengths = lengths
        self.pad = bool(pad)
        starts = [0]
        for n in lengths:
            starts.append(starts[-1] + n)
        self.starts = tuple(starts)                      # the prefix sum as host ints
        self._cache = {}                                 # device -> [offsets, row_base]: shared with the copies ``to()`` makes

    @classmethod
    def from_list(cls, slides, pad=False):
        """[(N_0, ...), (N_1, ...), ...] tensors of one row shape, dtype and device -> Ragged (the rows are joined once)."""
        slides = list(slides)
        if not slides:
            return cls(torch.empty((0, 0)), (), pad)
        first = slides[0]
        for k, s in enumerate(slides):
            if not torch.is_tensor(s) or s.dim() not in (2, 4) or s.shape[1:] != first.shape[1:] or s.dtype != first.dtype \
                    or s.device != first.device:
                raise TypeError("slide {}: every slide is a (N_b, F) or (N_b, C, h, w) tensor of one row shape, dtype and device".format(k))
        return cls(torch.cat(slides, 0), [s.shape[0] for s in slides], pad)

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
        r.rows, r.lengths, r.starts, r._cache, r.pad = rows, self.lengths, self.starts, self._cache, self.pad
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
        return "Ragged(rows={}, lengths={}, dtype={}, device={}{})".format(tuple(self.rows.shape), self.lengths, self.dtype, self.device,
                                                                           ", pad=True" if self.pad else "")


def collate_ragged(samples, pad=False):
    """A ``DataLoader`` ``collate_fn`` for the datasets' ``{'input': (N, ...), task: label}`` samples whose inputs differ in
    length: ``'input'`` becomes a ``Ragged``, everything else is collated as ``default_collate`` does."""
    from torch.utils.data import default_collate
    rest = default_collate([{k: v for k, v in s.items() if k != 'input'} for s in samples])
    rest['input'] = Ragged.from_list([torch.as_tensor(s['input']) for s in samples], pad)
    return rest


def collate_ragged_padded(samples):
    """``collate_ragged`` with ``pad=True``: slides with no more rows than the memory come back zero-padded to M rows, as
    ``fill_batch`` leaves them in the (B, M, ...) buffers - the loops of training/iterative.py drive real CAMELYON batches
    (many slides have fewer foreground tiles than M = 5000) unchanged."""
    return collate_ragged(samples, pad=True)


def refuse(what):
    """``ips_stream()`` feeds and ``dist.ips_sharded`` take tensors of one length per image."""
    raise TypeError("{} takes (B, N, ...) tensors: a Ragged batch goes through IPSNet.ips_ragged".format(what))


def _refuse_short(b, n, M, pad):
    """The slide ``b`` of ``n`` rows that no ragged call - ``ips_ragged``, ``ips_image_ragged``, a ragged stream's
    ``finish`` - makes a rectangular batch with: no more rows than the memory without ``pad``, no rows at all with it."""
    if pad and n == 0:
        raise ValueError("slide {} has no rows: nothing to pad".format(b))
    if n <= M and not pad:
        raise ValueError("slide {} has {} rows and the memory M = {}: the reference returns all {} of them there, the "
                         "batch would not be rectangular (select such a slide with ips())".format(b, n, M, n))


def _leave_count(net, lengths, pad):
    """``last_mem_count`` of a ragged call: the filled slots of every slide after ``pad``, else None."""
    net._mem_count = tuple(min(n, net.M) for n in lengths) if pad else None


def _check(net, slides, pad=False):
    _check_facts(net, slides.lengths, slides.dtype, tuple(slides.rows.shape), pad)


def _check_facts(net, lengths, dtype, rows_shape, pad):
    """Everything ``ips_ragged`` refuses, before the first launch and before the first random number is drawn, asked of
    the slides' ``lengths``, the ``dtype`` and the shape of the packed rows (``ips_image_ragged``: of the grid patches).
    ``pad``: slides with N_b <= M are taken (never shuffled, so 'instance' shuffling with positions does not refuse them);
    an empty slide is not."""
    if len(lengths) == 0:
        raise ValueError("ips_ragged: an empty batch")
    if dtype == torch.uint8:                   # what IPSNet._check_u8 asks of the solo calls' (1, N_b, C, h, w) patches
        if not net.is_image or len(rows_shape) != 4:
            raise TypeError("uint8 rows go with the (sum N_b, C, h, w) patches of an image encoder (set_patch_table), "
                            "a feature net reads float rows")
        table = net._table_for(torch.empty(0, dtype=dtype))
        if table.shape[0] != rows_shape[1]:
            raise ValueError("the patch table has {} rows, the patches {} channels".format(table.shape[0], rows_shape[1]))
        if hip.on_device(net.device) and hip.precision() != "fp32":
            raise TypeError("uint8 patches go with the exact trunk (IPSX_PRECISION=fp32), not {}".format(hip.precision()))
    if hip.dedup_blank():                     # (as streams do: whatever the device)
        raise TypeError("blank-patch dedup needs batches of one length (IPSX_DEDUP_BLANK=1 with ips_ragged)")
    if len(rows_shape) != (4 if net.is_image else 2):
        raise TypeError("ips_ragged: {} rows for {}".format(rows_shape, "an image encoder ((sum N_b, C, h, w))" if net.is_image
                                                            else "a feature net ((sum N_b, F))"))
    for b, n in enumerate(lengths):
        _refuse_short(b, n, net.M, pad)
        if net.use_pos and n > net.pos_enc.shape[1]:
            raise ValueError("slide {} has {} rows, the positional table conf.N = {}".format(b, n, net.pos_enc.shape[1]))
        if (net.use_pos and net.shuffle and net.shuffle_style == 'instance' and not net._shuffle_overridden()
                and n > net.M and n != net.pos_enc.shape[1]):
            # (shuffle_instance gathers the WHOLE table with the slide's permutation: ips() on this slide alone raises)
            raise ValueError("slide {} has {} rows: shuffle_style 'instance' with use_pos needs slides of exactly conf.N = {} "
                             "rows, as ips() does".format(b, n, net.pos_enc.shape[1]))


@torch.no_grad()
def ips_ragged(net, slides, pad=False):
    """``IPSNet.ips_ragged``: see there.  ``pad`` decides what ``_check`` refuses, whether the loop launch lets short slides
    through, and whether the call leaves a ``last_mem_count`` - nothing else."""
    pad = bool(pad)
    if not isinstance(slides, Ragged):
        slides = Ragged.from_list(slides, pad)
    _check(net, slides, pad)
    net._reset_last()
    if not hip.on_device(net.device) or (net.encoder.training and not net.training):
        out = _host_route(net, slides)
    else:
        out = _device_route(net, _RowsSource(net, slides), short_ok=pad)
    _leave_count(net, slides.lengths, pad)
    return out


# ------------------------------------------------------------------ the padding of last_mem_emb
def _zero_emb(net, row_shape, dtype):
    """(1, D): the embedding of ONE all-zero row (rows stored as uint8: the padding of ``mem_patch`` is float32 +0.0, not byte 0)."""
    return net._embed(torch.zeros((1,) + tuple(row_shape), device=net.device, dtype=torch.float32 if dtype == torch.uint8 else dtype))


def _pad_emb(net, emb, hole, row_shape, dtype):
    """``last_mem_emb`` of a padded device call: ``emb`` (B, M, D) with ``_zero_emb`` in the empty slots ``hole`` (B, M) - what
    ``forward()`` in eval mode computes from the zero padding."""
    with torch.no_grad(), net._scoring(), net.plan.hold():
        zero = _zero_emb(net, row_shape, dtype)
    return torch.where(hole.unsqueeze(-1), zero.view(1, 1, -1), emb)


# ------------------------------------------------------------------ the host route
def _host_emb(net, long_emb, short_rows):
    """``last_mem_emb`` of a call on the host route, made on first use: the solo calls' embeddings for the long slides; for
    a short one the eval-mode embeddings of its rows in [0, N_b) and, behind them, ``_zero_emb``."""
    if any(e is None for e in long_emb.values()):
        return None
    embs, zero = [], None
    with torch.no_grad(), net._scoring():
        for b in range(len(long_emb) + len(short_rows)):
            if b in long_emb:
                embs.append(long_emb[b][0])
                continue
            rows = short_rows[b]
            e = net._embed(rows)
            if rows.shape[0] < net.M:
                zero = _zero_emb(net, rows.shape[1:], rows.dtype) if zero is None else zero
                e = torch.cat((e, zero.expand(net.M - rows.shape[0], -1)), 0)
            embs.append(e)
    return torch.stack(embs)


def _host_fill(net, lengths, row_shape, dtype, solo):
    """The (B, M, ...) batch of a host route from what ``solo`` yields slide by slide: ``(mem_patch, mem_pos, mem_idx,
    mem_emb)`` of the solo selection in a slide of more than M rows, else the slide's rows on the device (stored bytes
    dequantised) - written in the order given, as ``fill_batch`` writes them, zeros and indices of -1 behind them.  Leaves
    ``last_mem_idx`` and a lazy ``last_mem_emb``; what the solo selections left is theirs, not this call's."""
    B, M, D, device = len(lengths), net.M, net.D, net.device
    mem_patch = torch.zeros((B, M) + tuple(row_shape), dtype=torch.float32 if dtype == torch.uint8 else dtype, device=device)
    mem_pos = torch.zeros((B, M, D), dtype=net.pos_enc.dtype, device=device) if net.use_pos else None
    mem_idx = torch.full((B, M), -1, dtype=torch.int64, device=device)
    long_emb, short_rows = {}, {}
    for b, (n, got) in enumerate(zip(lengths, solo)):
        if n > M:
            p, q, idx, long_emb[b] = got
            mem_patch[b] = p[0]
            if net.use_pos:
                mem_pos[b] = q[0]
            mem_idx[b] = idx[0]
        else:
            short_rows[b] = got
            mem_patch[b, :n] = got
            if net.use_pos:
                mem_pos[b, :n] = net.pos_enc[0, :n]
            mem_idx[b, :n] = torch.arange(n, dtype=torch.int64, device=device)
    net._reset_last()
    net.last_mem_idx = mem_idx
    net._emb_make = lambda: _host_emb(net, long_emb, short_rows)
    return mem_patch, mem_pos


def _host_route(net, slides):
    """The loop the contract names, a solo call per long slide, plus the padding of the short ones on ATen ops - the CPU
    plumbing path (``_select_aten`` per slide), and a ROCm device whose encoder is in training mode inside an eval-mode net
    (batch statistics: no per-row function)."""
    u8, shuf = slides.dtype == torch.uint8, []

    def solo():
        for b, n in enumerate(slides.lengths):
            if n > net.M:
                p, q = net._call(slides[b].unsqueeze(0))
                shuf.append(net.last_shuffle)
                yield p, q, net.last_mem_idx, net.last_mem_emb
            else:                              # what ips() returns before it shuffles (uint8: the bytes dequantised)
                rows = slides[b].to(net.device)
                shuf.append(None)
                yield net._dequant(rows) if u8 else rows
    out = _host_fill(net, slides.lengths, slides.rows.shape[1:], slides.dtype, solo())
    net.last_shuffle = shuf if net.shuffle and any(s is not None for s in shuf) else None
    return out


# ------------------------------------------------------------------ the device route
def _draw(net, lengths, device, skip):
    """The permutations of a shuffled call, slide by slide in slide order, by the calls ``IPSNet._shuffle`` makes for a
    (1, N_b, ...) input on ``device`` -> the B (N_b,) permutations as drawn, or None.  ``skip``: the slides of a padded call
    that ``ips()`` returns before it shuffles (N_b <= M) - nothing is drawn for them, they stay in the order given."""
    perms = [None if b in skip else draw_shuffle_for(1, n, device, net.shuffle_style) for b, n in enumerate(lengths)]
    drawn = [p for p in perms if p is not None]
    if not drawn:                              # (no long slide, or an unknown style: do_shuffle leaves everything as it is)
        return None
    return [torch.arange(n, dtype=torch.int64, device=drawn[0].device) if p is None else p.reshape(-1) for n, p in zip(lengths, perms)]


class _RowsSource:
    """What ``_device_route`` selects in, for ``ips_ragged``: the packed rows of a ``Ragged``.  ``ragged_image._ViewSource``
    answers the same questions for whole images; ``rows`` (there None) are the packed rows where they exist as a tensor."""

    def __init__(self, net, slides):
        # (drawn where the slides were handed over - a host-resident Ragged draws 'instance' permutations from the CPU
        #  generator, as its solo calls do)
        self.net, self.given, self.draw_device = net, slides, slides.device
        dev = slides.to(net.device)                  # a host-resident Ragged is copied whole
        self.rows, self.lengths, self.starts, self.offsets, self.row_base = dev.rows, dev.lengths, dev.starts, dev.offsets, dev.row_base
        self.row_shape, self.dtype = tuple(dev.rows.shape[1:]), dev.dtype

    def shuffled_copies(self, skip):
        """An overridden ``do_shuffle``, called as ever on the slides as given (not on those in ``skip``): its shuffled COPIES
        become the rows -> their packed positional rows | None.  Nothing is kept in ``last_shuffle``, as in ``ips()``."""
        net, rows, pos = self.net, [], []
        for b, n in enumerate(self.lengths):
            x, p = self.given[b], net.pos_enc[0, :n] if net.use_pos else None
            if b not in skip:
                x, p = net.do_shuffle(x.unsqueeze(0), net.pos_enc if net.use_pos else None)
                x, p = x[0], p[0, :x.shape[1]] if torch.is_tensor(p) else None
            rows.append(x)
            pos.append(p)
        self.rows = torch.cat(rows, 0).to(net.device)
        return torch.cat(pos, 0).to(net.device) if net.use_pos else None

    def through_index(self, flat):
        """-> (may the encoder read the rows through the int32 ``flat`` (``Selection.index_supported`` for one piece)?, the
        index it reads through): where it may not, the rows become the permuted copy."""
        net, rows = self.net, self.rows
        if os.environ.get("IPSX_SHUFFLE", "index") == "copy":
            ok = False
        elif not net.is_image:
            ok = rows.dtype in (torch.float32, torch.float16, torch.bfloat16)
        else:   # (uint8 rows come with their table - ``_check`` saw to it - and the list addresses bytes as it addresses floats)
            ok = rows.dtype in (torch.float32, torch.uint8) and bool(net.plan.index_list_supported(rows.shape))
        if ok:
            return True, flat
        self.rows = rows.index_select(0, flat)
        return False, None

    def encode(self, flat):
        net, rows = self.net, self.rows
        if flat is None:
            return net._embed(rows)
        if net.is_image:
            return net.plan.encode_source(hip.PatchSource(rows, net._table_for(rows)), index=flat)
        return net.plan.encode(rows, index=flat)

    def finish(self, offsets, mem_idx, flat, pos):
        """ONE launch: ``ipsx_ragged_finish``, or ``_finish_aten`` for rows that are no whole 16-byte units."""
        net, rows, M = self.net, self.rows, self.net.M
        if hip.ragged_finish_supported(rows, pos):
            mem_patch, mem_pos, mem_idx, grow = hip.ragged_finish(rows, offsets, mem_idx, M, flat, pos)
        else:
            mem_patch, mem_pos, mem_idx, grow = _finish_aten(rows, offsets, self.lengths, mem_idx, M, flat, pos)
        if rows.dtype == torch.uint8:
            # the (B, M) selected byte rows leave as float32 table[c][byte]; the padding behind a short slide's rows is
            # float32 +0.0 (what fill_batch's zero-initialised buffers hold), not table[c][0]
            mem_patch = hip.dequant_patches(mem_patch, net._table_for(rows))
            if min(self.lengths) < M:
                mem_patch.masked_fill_((mem_idx < 0).view(len(self.lengths), M, 1, 1, 1), 0)
        return mem_patch, mem_pos, mem_idx, grow


def _finish_aten(rows, offsets, lengths, mem_idx, M, flat, pos):
    """``hip.ragged_finish`` for rows that are no whole 16-byte units: the ``gather_rows`` launches plus, where a slide is
    short, the padding on ATen ops -> the same four tensors."""
    B, device = len(lengths), rows.device
    n = torch.tensor(lengths, dtype=torch.int64).to(device).unsqueeze(1)
    slot = torch.arange(M, dtype=torch.int64, device=device).unsqueeze(0)
    local = torch.minimum(slot, n - 1).expand(B, M)             # a short slide: its rows in the order given
    if mem_idx is not None:                    # (the rows of short slides come back unwritten from the loop)
        local = torch.where(n <= M, local, torch.minimum(mem_idx.clamp(min=0), n - 1))
    grow = local + offsets[:-1].unsqueeze(1)
    g = grow.reshape(1, B * M)
    src = g if flat is None else flat.index_select(0, g[0]).to(torch.int64).unsqueeze(0)
    mem_patch = hip.gather_rows(rows.unsqueeze(0), src).view(B, M, *rows.shape[1:])
    mem_pos = hip.gather_rows(pos.unsqueeze(0), g).view(B, M, -1) if pos is not None else None
    if min(lengths) >= M:                      # every slot holds a row
        return mem_patch, mem_pos, local, grow
    valid = slot < n
    mem_patch.masked_fill_(~valid.view(B, M, *(1,) * (rows.dim() - 1)), 0)
    if mem_pos is not None:
        mem_pos.masked_fill_(~valid.unsqueeze(-1), 0)
    return mem_patch, mem_pos, torch.where(valid, local, -1), torch.where(valid, grow, -1)


def _device_route(net, source, short_ok):
    """A ragged call on a ROCm device: one encoder pass over all rows of the source, one packed logits table, ONE loop launch
    (the workgroups of short slides return before their first read) and ONE finish launch (selected rows, short slides' rows
    in the order given, the zero padding).  A batch of short slides only launches no encoder, no logits and no loop."""
    M, device, lengths, starts = net.M, net.device, source.lengths, source.starts
    B = len(lengths)
    short = frozenset(b for b, n in enumerate(lengths) if n <= M)
    with net._scoring():
        ca = net.transf.crs_attn
        with net.plan.hold():
            offsets = source.offsets
            flat = None                        # int32 (total,): packed row j of the call is row flat[j] of the source
            local = None                       # int64 (total,): the position inside its slide of packed row j
            pos = None
            copied = net.shuffle and net._shuffle_overridden()      # (rows only: ips_image_ragged materialises the patches then)
            if copied:
                pos = source.shuffled_copies(short)
            elif net.shuffle:
                perms = _draw(net, lengths, source.draw_device, short)
                if perms is not None:
                    local = torch.cat(perms).to(device)
                    by_index, flat = source.through_index((local + source.row_base()).to(torch.int32))
                    # (what the solo calls keep: the device copy where they select through the index, else the permutation as
                    #  drawn; a drawn call has a long slide, so the list is never all None)
                    net.last_shuffle = [None if b in short else (local[starts[b]:starts[b + 1]] if by_index else perms[b]).unsqueeze(0)
                                        for b in range(B)]
            emb = source.encode(flat) if len(short) < B else None
            if net.use_pos and not copied:
                if local is None:
                    local = torch.arange(starts[-1], dtype=torch.int64, device=device) - source.row_base()
                pos = net.pos_enc[0].index_select(0, local)          # positions restart at 0 in every slide
            mem_idx = None
            if emb is not None:
                logits = hip.logits(emb.unsqueeze(0), pos.unsqueeze(0) if pos is not None else None, ca.folded_query(), ca.H * ca.n_token)[0]
                mem_idx = hip.scan_ragged(logits, offsets, lengths, M, net.I, ca.H, ca.n_token, short_ok=short_ok)
        mem_patch, mem_pos, mem_idx, grow = source.finish(offsets, mem_idx, flat, pos)

    unencoded = source.rows if emb is None else None      # (a batch of short slides only: at most B * M rows, kept until they are read)
    padded, row_shape, dtype = min(lengths) < M, source.row_shape, source.dtype

    def emb_of_slots():
        """(B, M, D): the packed pass's rows (made now for a batch of short slides only), the padding by ``_pad_emb``."""
        with torch.no_grad(), net._scoring(), net.plan.hold():
            table = emb if emb is not None else net._embed(unencoded)
            out = hip.gather_rows(table.unsqueeze(0), (grow.clamp(min=0) if padded else grow).view(1, B * M)).view(B, M, -1)
        return _pad_emb(net, out, grow < 0, row_shape, dtype) if padded else out
    net.last_mem_idx = mem_idx
    net._emb_make = emb_of_slots
    return mem_patch, mem_pos
