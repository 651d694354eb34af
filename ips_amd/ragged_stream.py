"""``RaggedIPSStream``: slides of different lengths fed in pieces (``IPSNet.ips_ragged_stream()``).

``ips_stream()`` bounds the memory of a selection but every image must receive the same number of rows in every feed;
``ips_ragged()`` takes slides of different lengths but needs every row of every slide at once.  This stream does both:

    s = net.ips_ragged_stream()                 # or pad=True
    for pieces in source:                       # a Ragged, or a list of B tensors (n_b, F) | (n_b, C, h, w); n_b >= 0, sum n_b >= 1
        s.feed(pieces)
    mem_patch, mem_pos = s.finish()

Every feed carries the next rows of each slide, as many or as few as the caller has - none for a slide that has ended or has
nothing this time - and each slide's chunk loop runs as far as that slide's rows allow.  On a net whose ``shuffle`` is off
``finish()`` returns and leaves behind, bit for bit, what ``net.ips_ragged([torch.cat(pieces of slide b) for b], pad=pad)``
returns and leaves behind, wherever the pieces end.  Like ``IPSStream`` it never shuffles.

On a ROCm device the state is that of ``IPSStream`` - two sets of four tables (B, M + I - 1, ...): patch rows, embeddings,
global ids, logits (the logits table alone grows with the largest number of candidates a slide has had in a feed) - but
every slide has its own numbers: rows held, rows fed, iterations this feed completes.  They are host ints; per feed they go
to the device as ONE small int64 table, and nothing is read back.  A feed is one encoder pass and one ``hip.logits`` over
its packed rows, one launch that puts the piece's logits behind each slide's held logits
(``hip.stream_commit_ragged``, append), ONE loop launch in which slide b scans the first M + k_b * I rows of its block of
the logits table (``hip.scan_ragged_spans``; a slide with k_b = 0 is not touched) and ONE commit launch for all four tables
in which a slide selects, moves (it completed no chunk but the stream flips its buffer set) or idles.  A feed in which no
slide completes a chunk is encoder, logits and one append launch for the four tables.

On a CPU device, and where an encoder alone is in training mode inside an eval-mode net (the fall-back conditions of
``ragged._host_route``), B solo ``IPSStream`` state machines run on ATen ops.

A ragged ROW stream (``net.ips_ragged_stream(pad, patch_size, patch_stride)``) takes the pixel rows of whole
images of different sizes instead:

    s = net.ips_ragged_stream(patch_size=(32, 32), patch_stride=(16, 16))
    for bands in reader:                        # a list of B entries: (C, h_b, W_b) with h_b >= 0, or None; sum h_b >= 1
        s.feed_rows(bands)
    mem_patch, mem_pos = s.finish()

and returns and leaves behind what ``net.ips_image_ragged([torch.cat(bands of image b, 1) for b], patch_size, patch_stride,
pad=pad)`` does, wherever the bands end.  Every image has its own ``BandGeometry`` and carried rows (fewer than ``ph``); a feed
packs the carried rows and the bands into ONE window buffer, and where the encoder reads a ``hip.RaggedView`` the patches the
windows complete are never unfolded: the stems read the window, and ``hip.stream_commit_ragged(..., pixels=, view=)`` copies
the kept patches out of it.  Everywhere else the live patch rows are unfolded and take ``feed()``'s path, or (the ATen
route) B solo row streams run.
"""

import torch

from . import hip
from .ragged import Ragged, _host_fill, _leave_count, _pad_emb, _refuse_short
from .ragged_image import RaggedImages, _ViewSource
from .stream import BandGeometry, IPSStream, StreamState


class RaggedIPSStream(StreamState):
    """The state of one streamed ragged selection.  ``fed``: rows per slide so far; ``iterations``: completed iterations per
    slide; ``mem_idx``: (B, M) int64 row numbers inside each slide, in the order of its last completed iteration (a row of
    -1 for a slide that has not reached M rows; None before the first feed).  A row stream (``patch_size`` / ``patch_stride``
    given) takes ``feed_rows(bands)`` instead of ``feed``; ``rows``: pixel rows per image so far, ``fed``:
    complete patch rows times ``nx_b``; ``view_feeds``: feeds whose piece was read through a ragged view (no patch tensor)."""

    entry = "ips_ragged_stream"

    def __init__(self, net, pad=False, patch_size=None, patch_stride=None):
        super().__init__(net, patch_size, patch_stride)
        self.pad = bool(pad)
        if self._patch_size is not None:
            self._geoms = self._carry = self._widths = self._nx = None   # per image, made by the first feed
            self._view_ok = False        # does the encoder read a ragged view of this patch shape (decided by the first feed)
        self._fed, self._iters, self._held = [], [], []
        self._last_idx = None
        self._solo = None            # the host route: B IPSStream on ATen ops
        self._device_route = None    # decided by the first feed
        self._stage, self._stage_at = [], 0      # pinned (3, B, 6) staging buffers of the per-feed table, used in turn

    # ------------------------------------------------------------------ observable state
    @property
    def rows(self):
        """Pixel rows taken per image so far (a row stream; None before the first feed)."""
        if self._patch_size is None or self._geoms is None:
            return None
        return tuple(g.rows for g in self._geoms)

    @property
    def fed(self):
        return tuple(self._fed)

    @property
    def iterations(self):
        return tuple(self._iters)

    @property
    def mem_idx(self):
        if self._finished:
            return self._last_idx
        if self._B is None:
            return None
        M = self.net.M
        if not self._device_route:
            out = torch.full((self._B, M), -1, dtype=torch.int64, device=self.net.device)
            for b, s in enumerate(self._solo):
                if s.fed >= M:
                    out[b] = s.mem_idx[0]
            return out
        if self._sets is None:               # (a row stream whose bands have completed no patch row yet)
            return torch.full((self._B, M), -1, dtype=torch.int64, device=self.net.device)
        reached = torch.tensor([n >= M for n in self._fed]).to(self.net.device)
        return torch.where(reached.unsqueeze(1), self._sets[self._cur][2][:, :M], -1)

    # ------------------------------------------------------------------ checks, before the first launch or allocation of a call
    def _check_pieces(self, pieces):
        """-> (lengths, row shape, dtype) of a feed, or the refusal."""
        net = self.net
        dim = 4 if net.is_image else 2
        layout = "(n_b, C, h, w) patches of an image encoder" if net.is_image else "(n_b, F) feature rows"
        if isinstance(pieces, Ragged):
            if pieces.rows.dim() != dim:
                raise ValueError("a feed is a Ragged, or a list of B tensors, of {}".format(layout))
            lengths, shape, dtype = pieces.lengths, tuple(pieces.rows.shape[1:]), pieces.dtype
        else:
            if not isinstance(pieces, (list, tuple)) or not pieces or any(not torch.is_tensor(p) or p.dim() != dim for p in pieces):
                raise ValueError("a feed is a Ragged, or a list of B tensors, of {}".format(layout))
            shape, dtype = tuple(pieces[0].shape[1:]), pieces[0].dtype
            for k, p in enumerate(pieces):
                if tuple(p.shape[1:]) != shape or p.dtype != dtype:          # (each piece may lie on the host or on the device)
                    raise ValueError("piece {}: the pieces of a feed have one row shape and dtype".format(k))
            lengths = tuple(int(p.shape[0]) for p in pieces)
        if len(lengths) == 0:
            raise ValueError("a feed of no slides")
        if dtype == torch.uint8:
            raise TypeError("ips_ragged_stream reads float32 rows (float16 / bfloat16 where ips() takes them): uint8 patch storage "
                            "goes through ips_stream() slide by slide")
        if self._B is None:
            if dtype not in (torch.float32, torch.float16, torch.bfloat16):
                raise TypeError("pieces are float32, or float16 / bfloat16 where ips() takes them; got {}".format(dtype))
            if dtype != torch.float32 and self._routes_to_device():
                # (what the encoder plan would refuse at its first launch: said here, before anything is allocated)
                if hip.precision() == "fp32" or (not net.is_image and hip.precision() != "bf16"):
                    raise TypeError("{} pieces need IPSX_PRECISION=bf16{}".format(dtype, " or fp32x3" if net.is_image else ""))
        else:
            if len(lengths) != self._B or shape != self._row_shape:
                raise ValueError("a feed of {} slides with rows {} in a stream of B = {} slides with rows {}".format(
                    len(lengths), shape, self._B, self._row_shape))
            if dtype != self._dtype:
                raise TypeError("a {} feed in a stream of {}".format(dtype, self._dtype))
        if sum(lengths) == 0:
            raise ValueError("a feed carries at least one row (every length is 0)")
        if net.use_pos:
            fed = self._fed or [0] * len(lengths)
            for b, n in enumerate(lengths):
                if fed[b] + n > net.pos_enc.shape[1]:
                    raise ValueError("slide {} would have {} rows, the positional table conf.N = {}".format(
                        b, fed[b] + n, net.pos_enc.shape[1]))
        return lengths, shape, dtype

    def _routes_to_device(self):
        net = self.net
        return hip.on_device(net.device) and not (net.encoder.training and not net.training)

    # ------------------------------------------------------------------ feed
    @torch.no_grad()
    def feed(self, pieces):
        """Take the next rows of every slide: a ``Ragged``, or a list of B tensors (n_b, ...) with n_b >= 0 and at least one
        row in all; on the device or on the host (a host piece is copied to the device as it is, and only the piece).
        Stream-ordered on the current stream, as ``IPSStream.feed``."""
        if self._patch_size is not None:
            raise TypeError("this is a row stream (ips_ragged_stream(patch_size=, patch_stride=)): it takes feed_rows(bands), not patches")
        self._check_open()
        lengths, shape, dtype = self._check_pieces(pieces)
        net = self.net
        if self._B is None:
            self._B, self._row_shape, self._dtype = len(lengths), shape, dtype
            self._fed, self._iters, self._held = [0] * self._B, [0] * self._B, [0] * self._B
            self._device_route = self._routes_to_device()
            if not self._device_route:
                self._solo = [IPSStream(net) for _ in range(self._B)]
                for s in self._solo:
                    s._on_device = False         # (the ATen state machine, also for device tensors)
        if self._device_route:
            with net._scoring():
                self._feed_hip(pieces, lengths)
        else:
            for b, n in enumerate(lengths):
                if n:
                    self._solo[b].feed(pieces[b].unsqueeze(0))
                    self._iters[b] = self._solo[b].iterations
        for b, n in enumerate(lengths):
            self._fed[b] += n
        return self

    def feed_all(self, slides, slab_rows):
        """Walk ``slides`` (a ``Ragged`` or a list of (N_b, ...) tensors) in slabs of at most ``slab_rows`` packed rows - a slab
        may end inside a slide - and feed each: the lazy route for a host batch,
        ``net.ips_ragged_stream(pad=...).feed_all(batch, 65536).finish()``."""
        slab_rows = int(slab_rows)
        if slab_rows < 1:
            raise ValueError("slabs of {} rows".format(slab_rows))
        ragged = slides if isinstance(slides, Ragged) else None
        lengths = ragged.lengths if ragged is not None else tuple(int(s.shape[0]) for s in slides)
        starts = [0]
        for n in lengths:
            starts.append(starts[-1] + n)
        total = starts[-1]
        if total == 0:
            self.feed(slides)                    # (refused there)
        for lo in range(0, total, slab_rows):
            hi = min(lo + slab_rows, total)
            cut = [(min(max(lo, starts[b]), starts[b + 1]) - starts[b], min(max(hi, starts[b]), starts[b + 1]) - starts[b])
                   for b in range(len(lengths))]
            if ragged is not None:               # the slab's rows are one range of the packed rows
                self.feed(Ragged(ragged.rows[lo:hi], [e - s for s, e in cut]))
            else:
                self.feed([slides[b][s:e] for b, (s, e) in enumerate(cut)])
        return self

    # ------------------------------------------------------------------ feed_rows
    def _check_bands(self, bands):
        """Everything that refuses a feed of bands, before the first launch or allocation of the call and before the stream's
        state changes -> (dtype, channels, widths, plans): ``plans[b]`` is ``BandGeometry.plan`` of image b's band, None for an
        image without rows this time; ``widths[b]`` the image's width once a non-empty band has fixed it."""
        net = self.net
        (ph, pw), (sh, sw) = self._patch_size, self._patch_stride
        layout = "a feed is a list of B entries: (C, h_b, W_b) bands - the next h_b >= 0 pixel rows of image b - or None"
        if isinstance(bands, (Ragged, RaggedImages)):
            raise TypeError("feed_rows takes a list of bands; a RaggedImages of whole images goes through feed_rows_all")
        if not isinstance(bands, (list, tuple)) or not bands:
            raise ValueError(layout)
        if self._B is not None and len(bands) != self._B:
            raise ValueError("a feed of {} entries in a stream of B = {} images".format(len(bands), self._B))
        B = len(bands)
        dtype, chans = self._dtype, (self._row_shape[0] if self._row_shape else None)
        widths = list(self._widths) if self._widths else [None] * B
        geoms = self._geoms or [BandGeometry(ph, sh)] * B             # (plan() reads, it takes nothing)
        fed = self._fed or [0] * B
        plans, any_row = [None] * B, False
        for b, band in enumerate(bands):
            if band is None:
                continue
            if not torch.is_tensor(band) or band.dim() != 3 or band.shape[0] < 1 or band.shape[2] < 1:
                raise ValueError("entry {}: {}".format(b, layout))
            Cc, h, W = band.shape
            if dtype is None:                    # the stream's first band
                self._check_first_band(band, Cc, hip.on_device(net.device))
                dtype, chans = band.dtype, Cc
            elif band.dtype != dtype:
                raise TypeError("entry {}: a {} band in a stream of {}".format(b, band.dtype, dtype))
            elif Cc != chans:
                raise ValueError("entry {}: a band of {} channels in a stream of {}".format(b, Cc, chans))
            if widths[b] is not None and W != widths[b]:
                raise ValueError("entry {}: a band {} pixels wide, image {} is {} wide".format(b, W, b, widths[b]))
            if h == 0:
                continue
            if widths[b] is None:
                self._check_patch_fits(W, "entry {}: ".format(b))
                widths[b] = W
            plans[b] = geoms[b].plan(h)
            any_row = True
            n = fed[b] + plans[b][2] * ((W - pw) // sw + 1)
            if net.use_pos and n > net.pos_enc.shape[1]:
                raise ValueError("image {} would have {} patches, the positional table conf.N = {}".format(b, n, net.pos_enc.shape[1]))
        if not any_row:
            raise ValueError("a feed carries at least one pixel row (every entry is None or has no rows)")
        return dtype, chans, widths, plans

    @torch.no_grad()
    def feed_rows(self, bands):
        """Take the next pixel rows of every image: a list of B entries, ``(C, h_b, W_b)`` float32 - or uint8 after
        ``set_patch_table`` - with h_b >= 0, or None for an image that has ended or has nothing this time; at least one pixel
        row in all; each band on the device or on the host.  Image b's width is that of its first non-empty band.  The patch
        rows a feed completes are its piece (none: nothing is launched).  Stream-ordered like ``feed``: when the call returns,
        the caller may overwrite or free the bands."""
        if self._patch_size is None:
            raise TypeError("this is a patch stream: feed_rows() goes with ips_ragged_stream(patch_size=, patch_stride=)")
        if isinstance(bands, (Ragged, RaggedImages)):
            raise TypeError("feed_rows takes a list of bands; a RaggedImages of whole images goes through feed_rows_all")
        self._check_open()
        dtype, chans, widths, plans = self._check_bands(bands)
        net = self.net
        (ph, pw), (sh, sw) = self._patch_size, self._patch_stride
        if self._B is None:
            B = self._B = len(bands)
            self._row_shape, self._dtype = (chans, ph, pw), dtype
            self._fed, self._iters, self._held = [0] * B, [0] * B, [0] * B
            self._geoms, self._carry = [BandGeometry(ph, sh) for _ in range(B)], [None] * B
            self._device_route = self._routes_to_device()
            if self._device_route:
                # (asked of the smallest view of this patch shape: the answer depends on the trunk and the patch alone)
                self._view_ok = bool(net.plan.ragged_view_supported(hip.RaggedView(chans, [(ph, pw)], [0], (ph, pw), (sh, sw))))
            else:
                self._solo = [IPSStream(net, self._patch_size, self._patch_stride) for _ in range(B)]
                for s in self._solo:
                    s._on_device = False         # (the ATen state machine, also for device tensors)
        self._widths = widths
        self._nx = [0 if W is None else (W - pw) // sw + 1 for W in widths]
        if self._device_route:
            self._feed_rows_hip(bands, plans)
        else:
            for b, plan in enumerate(plans):
                if plan is not None:
                    self._solo[b].feed_rows(bands[b].unsqueeze(0))
                    self._iters[b] = self._solo[b].iterations
        for b, plan in enumerate(plans):
            if plan is not None:
                self._geoms[b].take(bands[b].shape[1])
                self._fed[b] += plan[2] * self._nx[b]
        return self

    def feed_rows_all(self, images, band_rows):
        """Walk ``images`` (a ``RaggedImages`` or a list of (C, H_b, W_b) tensors) in bands of at most ``band_rows`` pixel rows
        per image and feed each; an image that has run out drops out of the later feeds.  The lazy route for a host batch,
        ``net.ips_ragged_stream(patch_size=..., patch_stride=...).feed_rows_all(batch, 256).finish()``."""
        band_rows = int(band_rows)
        if band_rows < 1:
            raise ValueError("bands of {} rows".format(band_rows))
        images = list(images)
        if not images or any(not torch.is_tensor(im) or im.dim() != 3 for im in images):
            raise ValueError("feed_rows_all takes a RaggedImages or a list of (C, H_b, W_b) images")
        tallest = max(im.shape[1] for im in images)
        if tallest == 0:
            self.feed_rows(images)               # (refused there)
        for lo in range(0, tallest, band_rows):
            self.feed_rows([im[:, lo:lo + band_rows] if lo < im.shape[1] else None for im in images])
        return self

    def _feed_rows_hip(self, bands, plans):
        """One feed of bands on the device: ONE packed window buffer - per image with rows the carried rows, then the band's,
        as (C, rows_b, W_b) at a 16-byte offset: the only pixel copy of the feed, a host band lands in it -, the selection on
        the patch rows the windows complete (``_feed_hip``: through a ragged view over the LIVE images where the encoder
        reads one, as patch tensors elsewhere), then each image's rows behind its last complete patch row kept as a copy."""
        net = self.net
        (ph, pw), (sh, sw) = self._patch_size, self._patch_stride
        B, dev, Cc = self._B, net.device, self._row_shape[0]
        unit = max(16 // torch.empty((), dtype=self._dtype).element_size(), 1)
        have = [b for b in range(B) if plans[b] is not None and plans[b][1] > 0]
        if not have:                             # every row of the feed lies between two patch rows
            return
        offs, end = {}, 0
        for b in have:
            offs[b] = (end + unit - 1) // unit * unit
            end = offs[b] + Cc * plans[b][1] * self._widths[b]
        window = torch.empty((end,), dtype=self._dtype, device=dev)
        wins = {}
        for b in have:
            drop, rows = plans[b][:2]
            W = self._widths[b]
            win = wins[b] = window[offs[b]:offs[b] + Cc * rows * W].view(Cc, rows, W)
            self._fill_window(win, self._carry[b], bands[b][:, drop:])
        live = [b for b in have if plans[b][2] > 0]
        if live:
            lengths = [plans[b][2] * self._nx[b] if plans[b] is not None and plans[b][1] > 0 else 0 for b in range(B)]
            with net._scoring():
                if self._view_ok:
                    view = hip.RaggedView(Cc, [(plans[b][1], self._widths[b]) for b in live], [offs[b] for b in live],
                                          self._patch_size, self._patch_stride)
                    self._feed_hip(None, lengths, window, view)
                    self.view_feeds += 1
                else:                            # the pieces as patch tensors, through feed()'s path
                    empty = torch.empty((0,) + self._row_shape, dtype=self._dtype, device=dev)
                    pieces = [net._materialise(wins[b][None, :, :(plans[b][2] - 1) * sh + ph], self._patch_size, self._patch_stride)[0]
                              if lengths[b] else empty for b in range(B)]
                    self._feed_hip(pieces, lengths)
        for b in have:                           # (copies: the window itself is released)
            rows, keep = plans[b][1], plans[b][3]
            self._carry[b] = wins[b][:, rows - keep:].clone() if keep else None

    # ------------------------------------------------------------------ the ROCm device
    def _scan_workspace(self, dev):
        """(every slide scans its own span: B times what one image needs)"""
        net = self.net
        ca = net.transf.crs_attn
        nb = hip.lib().ipsx_scan_workspace_bytes(1, net.M, net.I, ca.H, ca.n_token)
        return torch.empty(self._B * nb, dtype=torch.uint8, device=dev) if nb else None

    def _numbers(self, planes, dev, view=None):
        """Up to three (B, 6) planes of host ints -> ONE (3, B, 6) int64 tensor on the device, ONE copy.  The copy leaves from
        pinned memory and does not wait for the device: a few staging buffers are used in turn, each with the event behind
        its last copy.  ``view``: a feed's ``hip.RaggedView`` - its entry table (at most B entries of four words) rides behind
        the planes in the same copy and the view is told where it lies."""
        B = self._B
        planes = planes + [[[0] * 6] * B] * (3 - len(planes))
        host = torch.tensor(planes, dtype=torch.int64)
        if not self._stage:
            self._stage = [[torch.empty((22 * B,), dtype=torch.int64).pin_memory(), None] for _ in range(4)]
        slot = self._stage[self._stage_at % len(self._stage)]
        self._stage_at += 1
        if slot[1] is not None:
            slot[1].synchronize()
        slot[0][:18 * B].copy_(host.view(-1))
        if view is not None:
            entries = torch.frombuffer(bytearray(bytes(view.table)), dtype=torch.int64)
            slot[0][18 * B:18 * B + entries.numel()].copy_(entries)
        out = slot[0].to(dev, non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record()
        if view is not None:
            view.on(out.device, out[18 * B:])
        return out[:18 * B].view(3, B, 6)

    def _pack(self, pieces, lengths, dev):
        """The feed's rows as ONE packed (sum n_b, ...) tensor on the device: a host piece goes over as it is."""
        if isinstance(pieces, Ragged):
            return pieces.rows.to(dev)
        live = [p for p in pieces if p.shape[0]]
        if len(live) == 1:
            p = live[0].to(dev)
            return p if p.is_contiguous() else p.contiguous()
        packed = torch.empty((sum(lengths),) + self._row_shape, dtype=self._dtype, device=dev)
        lo = 0
        for p in live:
            packed[lo:lo + p.shape[0]].copy_(p)
            lo += p.shape[0]
        return packed

    def _scan(self, counts, lcap):
        """ONE loop launch: slide b scans the first counts[b] rows of its block of the current logits table (0: not touched)."""
        net = self.net
        ca = net.transf.crs_attn
        lg = self._sets[self._cur][3]
        hip.scan_ragged_spans(lg.view(self._B * lcap, self._R), self._spans, max(counts), net.M, net.I, ca.H, ca.n_token,
                              self._sel, self._tie, workspace=self._scan_ws)
        hip.scan.last_tie = self._tie

    def _feed_hip(self, pieces, lengths, window=None, view=None):
        """One feed on the device.  ``view``: the feed's patches are those of a ``hip.RaggedView`` over ``window``, the packed
        pixel windows of a row stream's live images - encoded and committed where they lie, no patch tensor; slide b's first
        packed patch is ``starts[b]``, in the view as in the packed embeddings, ids and logits."""
        net = self.net
        M, I, B, dev = net.M, net.I, self._B, net.device
        held, fed = self._held, self._fed
        total = [held[b] + lengths[b] for b in range(B)]
        k = [(t - M) // I if t > M else 0 for t in total]
        starts = [0]
        for n in lengths:
            starts.append(starts[-1] + n)
        any_select = any(k)
        if self._sets is None:
            self._allocate(dev)
        self._logits_room(max(total), dev)
        lcap = self._sets[self._cur][3].shape[1]
        # the per-slide numbers of every launch of this feed: ONE int64 table, ONE copy
        A, S, V, E = hip.COMMIT_APPEND, hip.COMMIT_SELECT, hip.COMMIT_MOVE, hip.COMMIT_IDLE
        append = [[held[b], total[b], 0, starts[b], A if lengths[b] else E, 0] for b in range(B)]
        commit = [[held[b], total[b], M + k[b] * I if k[b] else 0, starts[b], S if k[b] else (V if total[b] else E), 0] for b in range(B)]
        counts = [M + k[b] * I if k[b] else 0 for b in range(B)]
        spans = [[b * lcap, counts[b], lengths[b], fed[b] - starts[b], 0, 0] for b in range(B)]
        table = self._numbers([append, commit, spans], dev, view)
        self._spans = table[2, :, :2].contiguous()

        if view is None:
            packed, piece = self._pack(pieces, lengths, dev), {}
            emb = net._embed(packed)                                      # ONE encoder pass over the packed rows
        else:                                                             # ... over the packed patches of the view
            packed, piece = None, dict(pixels=window, view=view)
            emb = _ViewSource(net, window, view).encode()
        n_tot = starts[-1]
        # the row number inside its slide of every packed row: fed_b + r (ids, and the rows of the positional table)
        ids = torch.arange(n_tot, dtype=torch.int64, device=dev) + torch.repeat_interleave(table[2, :, 3], table[2, :, 2], output_size=n_tot)
        pos = net.pos_enc[0].index_select(0, ids).unsqueeze(0) if net.use_pos else None
        lg_piece = hip.logits(emb.unsqueeze(0), pos, net.transf.crs_attn.folded_query(), self._R)[0]
        cur, dst = self._sets[self._cur], self._sets[self._cur ^ 1]
        if not any_select:                   # no slide completes a chunk: everything goes behind the held rows, in place
            hip.stream_commit_ragged([(cur[0], packed, cur[0]), (cur[1], emb, cur[1]), (cur[2], ids, cur[2]), (cur[3], lg_piece, cur[3])],
                                     None, table[0], M, max(lengths), **piece)
            self._held = total
            return
        hip.stream_commit_ragged([(cur[3], lg_piece, cur[3])], None, table[0], M, max(lengths))
        self._scan(counts, lcap)
        rows_max = max(total[b] - k[b] * I for b in range(B))
        hip.stream_commit_ragged([(cur[0], packed, dst[0]), (cur[1], emb, dst[1]), (cur[2], ids, dst[2]), (cur[3], None, dst[3])],
                                 self._sel, table[1], M, rows_max, **piece)
        self._cur ^= 1
        self._held = [total[b] - k[b] * I for b in range(B)]
        for b in range(B):
            self._iters[b] += k[b]

    def _last_chunks(self):
        """The ragged last chunk of every slide that holds more than M rows: one more iteration, no tail behind it."""
        net = self.net
        M, B, dev = net.M, self._B, net.device
        held = self._held
        if not any(h > M for h in held):
            return
        lcap = self._sets[self._cur][3].shape[1]
        S, V, E = hip.COMMIT_SELECT, hip.COMMIT_MOVE, hip.COMMIT_IDLE
        commit = [[held[b], held[b], held[b], 0, S if held[b] > M else (V if held[b] else E), 0] for b in range(B)]
        counts = [held[b] if held[b] > M else 0 for b in range(B)]
        spans = [[b * lcap, counts[b], 0, 0, 0, 0] for b in range(B)]
        table = self._numbers([commit, spans], dev)
        self._spans = table[1, :, :2].contiguous()
        self._scan(counts, lcap)
        cur, dst = self._sets[self._cur], self._sets[self._cur ^ 1]
        hip.stream_commit_ragged([(cur[0], None, dst[0]), (cur[1], None, dst[1]), (cur[2], None, dst[2])], self._sel, table[0], M, M)
        self._cur ^= 1
        self._held = [min(h, M) for h in held]
        for b in range(B):
            self._iters[b] += 1 if held[b] > M else 0

    # ------------------------------------------------------------------ finish
    @torch.no_grad()
    def finish(self):
        """Run the ragged last chunk of every slide that has one -> (mem_patch (B, M, ...), mem_pos (B, M, D) | None), and
        leave behind what ``ips_ragged`` leaves.  Without ``pad`` a slide with no more than M rows is refused, with ``pad``
        a slide with no rows at all."""
        self._check_open()
        net = self.net
        if self._B is None:
            raise RuntimeError("nothing was fed")
        if self._patch_size is not None:
            for b, g in enumerate(self._geoms):
                if g.patch_rows == 0:        # (ips_image_ragged refuses a patch that does not fit its image)
                    raise ValueError("image {}: the {} pixel rows fed complete no patch row of height {}".format(
                        b, g.rows, self._patch_size[0]))
        for b, n in enumerate(self._fed):
            _refuse_short(b, n, net.M, self.pad)
        net._reset_last()
        if self._device_route:
            mem_patch, mem_pos = self._finish_hip()
        else:
            mem_patch, mem_pos = self._finish_aten()
        _leave_count(net, self._fed, self.pad)
        self._last_idx = net.last_mem_idx
        self._release()
        self._solo, self._stage = None, []
        return mem_patch, mem_pos

    def _finish_hip(self):
        net = self.net
        M, B, dev = net.M, self._B, net.device
        with net._scoring():
            self._last_chunks()
            patch, emb, ids, _ = self._sets[self._cur]
            mem_patch, mem_emb, mem_idx = patch[:, :M].clone(), emb[:, :M].clone(), ids[:, :M].clone()
            u8 = self._dtype == torch.uint8
            if u8:                           # a row stream's byte patch table: the M slots leave as float32, the padding as +0.0
                mem_patch = net._dequant(mem_patch)
            padded = any(n < M for n in self._fed)
            if padded:                       # rows, then +0.0; 0 .. N_b-1, then -1
                n = torch.tensor(self._fed, dtype=torch.int64).to(dev).unsqueeze(1)
                hole = torch.arange(M, dtype=torch.int64, device=dev).unsqueeze(0) >= n
                mem_patch.masked_fill_(hole.view(B, M, *(1,) * (mem_patch.dim() - 2)), 0)
                mem_idx.masked_fill_(hole, -1)
            mem_pos = None
            if net.use_pos:
                mem_pos = net._take(net.pos_enc.expand(B, -1, -1), mem_idx.clamp(min=0) if padded else mem_idx)
                if padded:
                    mem_pos.masked_fill_(hole.unsqueeze(-1), 0)
        net.last_mem_idx = mem_idx
        if not padded:
            net._mem_emb = mem_emb
            return mem_patch, mem_pos
        row_shape, dtype = self._row_shape, self._dtype
        # (the padding holds the embedding of ONE all-zero row, made on first read, as ``ips_ragged`` makes it)
        net._emb_make = lambda: _pad_emb(net, mem_emb, hole, row_shape, dtype)
        return mem_patch, mem_pos

    def _finish_aten(self):
        """What ``ragged._host_route`` builds, from the solo streams: a long slide's selection, a short slide's rows in the
        order given and the zero padding behind them."""
        net = self.net

        def solo():                          # (a row stream's bytes: the solo streams return them dequantised)
            for b, n in enumerate(self._fed):
                p, q = self._solo[b].finish()
                self._iters[b] = self._solo[b].iterations
                yield (p, q, net.last_mem_idx, net.last_mem_emb) if n > net.M else p[0]
        return _host_fill(net, self._fed, self._row_shape, self._dtype, solo())
