"""``IPSStream``: Iterative Patch Selection over patches that arrive in pieces (``IPSNet.ips_stream()``).

``IPSNet.ips`` needs the whole (B, N, ...) input before its first launch.  The reference's loop does not
(architecture/ips_net.py:213-241): per chunk it encodes I patches, scores them together with the memory and keeps M.  A
stream does exactly that with a state of M + I - 1 rows per image, whatever N turns out to be:

    s = net.ips_stream()
    for piece in source:            # (B, n_k, C, h, w) | (B, n_k, F), n_k >= 1 and arbitrary, device or host
        s.feed(piece)
    mem_patch, mem_pos = s.finish()

The chunk boundaries are the reference's - [0, M), then chunks of I, a ragged last chunk at ``finish()`` - wherever the
pieces end: a feed runs every iteration whose chunk is complete and carries the rest (fewer than I rows) to the next one.
With ``IPSX_PRECISION=fp32`` the results (``mem_patch``, ``mem_pos``, ``net.last_mem_idx``, ``net.last_mem_emb``) are those
of ``net.ips(torch.cat(pieces, 1))`` of a net whose ``shuffle`` is off, bit for bit.

The stream never shuffles: the permutation needs N, which a stream does not know.  A net with ``shuffle=True`` is not
refused (every shipped configuration sets it); a caller who wants randomised ties feeds the patches in random order.

On a ROCm device the state is two sets of four tables - patch rows as stored (bytes stay bytes), embeddings, logits,
global patch numbers - used alternately: rows [0, M) are the memory in rank order, the rows behind them the carried, not
yet scored patches.  A feed encodes its piece where it lies, writes the piece's logits behind the held rows of the
logits table, runs the completed iterations from ``it_begin = 0`` on that table (``hip.scan_range_strided``: compact row
numbers come back) and carries the state forward in one launch (``hip.stream_commit``) that reads the piece through its
own base address and batch stride - nothing is concatenated.  The logits table alone grows with the largest piece fed
(H * n_token floats per row); everything else is M + I - 1 rows per image.  On a CPU device the same state machine runs
on ATen ops, one ``score_and_select`` per iteration on the chunks ``IPSNet._select_aten`` would embed.

A ROW stream (``net.ips_stream(patch_size, patch_stride)``) takes the pixel rows of whole images instead:

    s = net.ips_stream(patch_size=(32, 32), patch_stride=(16, 16))
    for band in reader:             # (B, C, h_k, W): the NEXT h_k pixel rows of every image, h_k >= 1 and arbitrary
        s.feed_rows(band)
    mem_patch, mem_pos = s.finish()

and returns what ``net.ips_image(torch.cat(bands, 2), patch_size, patch_stride)`` returns, wherever the bands end.  The
stream owns a window - the pixel rows from the first row of the next incomplete patch row on, fewer than ``ph`` of them
(``BandGeometry``) - and puts every band behind it; the window's complete patch rows are the feed's piece.  Where the
encoder reads a ``hip.PatchView`` that piece is never unfolded: the stems read the window, and ``hip.stream_commit_view``
copies the kept patches out of it.  Everywhere else the piece is unfolded and takes ``feed()``'s path.
"""

import itertools

import torch

from . import hip
from .ragged import Ragged, refuse


class BandGeometry:
    """The integer bookkeeping of a row stream: patch rows of height ``ph`` every ``sh`` pixel rows, over bands of any
    height.  ``take(h)`` says what a band of ``h`` rows does - nothing here touches a tensor.

    ``carry``: rows of the window before the next band (< ph); ``skip``: rows of the coming bands that no patch row will ever
    cover (``sh > ph`` only; ``carry`` is 0 then); ``rows``: pixel rows taken; ``patch_rows``: complete patch rows so far;
    ``first_row``: the image row the window starts at (``patch_rows * sh`` whenever the window is not empty)."""

    def __init__(self, ph, sh):
        if ph < 1 or sh < 1:
            raise ValueError("patch height {} / stride {}".format(ph, sh))
        self.ph, self.sh = int(ph), int(sh)
        self.rows = self.carry = self.skip = self.patch_rows = 0

    @property
    def first_row(self):
        return self.rows - self.carry + self.skip

    def plan(self, h):
        """A band of ``h`` rows, without taking it -> (drop, window_rows, ny_w, carry, skip): its first ``drop`` rows are
        skipped, the window then has ``window_rows`` rows (carried + kept), of which ``ny_w`` patch rows are complete -
        window rows ``i * sh .. i * sh + ph - 1`` for i < ny_w -, and ``carry`` / ``skip`` afterwards."""
        if h < 1:
            raise ValueError("a band has at least one pixel row")
        drop = min(self.skip, h)
        rows = self.carry + h - drop
        skip = self.skip - drop
        if rows < self.ph:
            return drop, rows, 0, rows, skip
        ny_w = (rows - self.ph) // self.sh + 1
        nxt = ny_w * self.sh                       # the window row the next patch row starts at
        return drop, rows, ny_w, max(0, rows - nxt), max(0, nxt - rows)

    def take(self, h):
        out = self.plan(h)
        self.rows += h
        self.patch_rows += out[2]
        self.carry, self.skip = out[3], out[4]
        return out


class StreamState:
    """What ``IPSStream`` and ``RaggedIPSStream`` share: how a row stream is asked for, the checks of an open stream and of a
    row stream's first band, the device buffers (two sets of four tables, the scan's buffers), and the copy that puts
    carried pixel rows and a band into a window.  ``entry``: the ``IPSNet`` method a stream was made by, for the messages."""

    entry = None

    def __init__(self, net, patch_size, patch_stride):
        self.net = net
        self._patch_size = self._patch_stride = None          # ((ph, pw), (sh, sw)) of a row stream
        if patch_size is not None or patch_stride is not None:
            if patch_size is None or patch_stride is None:
                raise ValueError("a row stream needs both patch_size and patch_stride")
            if not net.is_image:
                raise TypeError("a row stream takes bands of whole images: it goes with an image encoder")
            (ph, pw), (sh, sw) = (int(v) for v in patch_size), (int(v) for v in patch_stride)
            if min(ph, pw, sh, sw) <= 0:
                raise ValueError("patch {}x{} / stride {}x{}".format(ph, pw, sh, sw))
            self._patch_size, self._patch_stride = (ph, pw), (sh, sw)
        self.view_feeds = 0
        self._finished = False
        self._generation = hip.weights_generation()
        self._B = self._row_shape = self._dtype = None
        # device state
        self._sets = None            # [[patch, emb, ids, logits], [...]]: the two buffer sets
        self._cur = 0
        self._sel = self._tie = self._scan_ws = None

    # ------------------------------------------------------------------ checks, before the first launch of a call
    def _check_open(self):
        if self._finished:
            raise RuntimeError("this stream has finished (IPSNet.{}() starts another)".format(self.entry))
        if hip.dedup_blank():
            raise TypeError("blank-patch dedup needs the whole input (IPSX_DEDUP_BLANK=1 with {})".format(self.entry))
        if hip.weights_generation() != self._generation:
            raise RuntimeError("the weights changed since this stream began (an optimizer step between feeds would mix "
                               "embeddings of two weight sets)")

    def _check_first_band(self, band, chans, on_device):
        """The first band of a row stream, ``chans`` channels: what every later one must look like."""
        net = self.net
        if band.dtype == torch.uint8:
            table = net._table_for(band)
            if table.shape[0] != chans:
                raise ValueError("the patch table has {} rows, the band {} channels".format(table.shape[0], chans))
            if on_device and hip.precision() != "fp32":
                raise TypeError("uint8 bands go with the exact trunk (IPSX_PRECISION=fp32), not {}".format(hip.precision()))
        elif band.dtype != torch.float32:
            raise TypeError("bands are float32, or uint8 after set_patch_table; got {}".format(band.dtype))
        want = next(net.encoder.children()).in_channels
        if chans != want:
            raise ValueError("a band of {} channels, the encoder expects {}".format(chans, want))

    def _check_patch_fits(self, W, label=""):
        """``label``: which entry of a feed the rows are, in front of the message."""
        if self._patch_size[1] > W:
            raise ValueError("{}patches of width {} do not fit rows of {} pixels".format(label, self._patch_size[1], W))

    # ------------------------------------------------------------------ the ROCm device
    def _allocate(self, dev):
        net = self.net
        B, cap = self._B, net.M + net.I - 1
        ca = net.transf.crs_attn
        self._R = ca.H * ca.n_token
        self._sets = [[torch.empty((B, cap) + self._row_shape, dtype=self._dtype, device=dev),
                       torch.empty((B, cap, net.D), dtype=torch.float32, device=dev),
                       torch.empty((B, cap), dtype=torch.int64, device=dev),
                       None] for _ in range(2)]
        self._sel = torch.empty((B, net.M), dtype=torch.int64, device=dev)
        self._tie = torch.zeros((B,), dtype=torch.int32, device=dev)
        self._scan_ws = self._scan_workspace(dev)

    def _logits_room(self, rows, dev, keep=None):
        """The logits tables hold the held rows AND the piece's: they grow with the largest number of candidates (R floats per
        row).  ``keep``: the rows per image of the current table that go over (None: the whole table)."""
        cur = self._sets[self._cur][3]
        if cur is not None and cur.shape[1] >= rows:
            return
        new = [torch.empty((self._B, rows, self._R), dtype=torch.float32, device=dev) for _ in range(2)]
        if cur is not None and keep is None:
            new[self._cur][:, :cur.shape[1]].copy_(cur)
        elif cur is not None and keep:
            new[self._cur][:, :keep].copy_(cur[:, :keep])
        for k in range(2):
            self._sets[k][3] = new[k]

    @staticmethod
    def _fill_window(window, carried, src):
        """``window`` (..., rows, W) <- the ``carried`` rows (None: none), then ``src`` (..., h, W), the band's rows: the only
        copy of pixels a feed makes - a host band's transfer lands in the window."""
        carry = window.shape[-2] - src.shape[-2]
        if carry:
            window[..., :carry, :].copy_(carried)
        if src.shape[-2]:
            dst = window[..., carry:, :]
            if src.device == window.device or (src.is_contiguous() and dst.is_contiguous()):
                dst.copy_(src)
            else:                        # host rows into a strided window: plane by plane, each transfer contiguous at both ends
                for at in itertools.product(*(range(n) for n in dst.shape[:-2])):
                    dst[at].copy_(src[at])

    def _release(self):
        """The end of the stream: its buffers go."""
        self._finished = True
        self._sets = self._sel = self._scan_ws = None
        if self._patch_size is not None:
            self._carry = None


class IPSStream(StreamState):
    """The state of one streamed selection.  ``fed``: patches per image so far; ``iterations``: completed iterations;
    ``mem_idx``: (B, M) int64 global patch numbers in the order of the last completed iteration (None until M patches
    have arrived).  A row stream (``patch_size`` / ``patch_stride`` given) takes ``feed_rows(band)`` instead of ``feed``;
    ``rows``: pixel rows taken so far, ``fed``: complete patch rows times ``nx``; ``view_feeds``: feeds whose piece was read
    through a patch view (no patch tensor)."""

    entry = "ips_stream"

    def __init__(self, net, patch_size=None, patch_stride=None):
        super().__init__(net, patch_size, patch_stride)
        self._geom = None
        if self._patch_size is not None:
            self._geom = BandGeometry(self._patch_size[0], self._patch_stride[0])
            self._carry = None           # (B, C, carry, W) on net.device: the window before the next band
            self._band_shape = None      # (B, C, W) of the first band
            self._nx = 0
        self.fed = 0
        self.iterations = 0
        self._on_device = hip.on_device(net.device)
        self._held = 0               # valid rows per image in the current set
        # ATen state
        self._mem_patch = self._mem_emb = self._mem_ids = None
        self._pending = None         # (B, t, ...) rows no iteration has consumed

    # ------------------------------------------------------------------ observable state
    @property
    def rows(self):
        """Pixel rows taken so far (a row stream)."""
        return self._geom.rows if self._geom is not None else None

    @property
    def mem_idx(self):
        M = self.net.M
        if self.fed < M or self._finished:
            return self._last_idx if self._finished else None
        if self._on_device:
            return self._sets[self._cur][2][:, :M].clone()
        return self._mem_ids.clone()

    # ------------------------------------------------------------------ checks, before the first launch of a call
    def _check(self, piece=None):
        net = self.net
        self._check_open()
        if piece is None:
            return
        if not torch.is_tensor(piece) or piece.dim() != (5 if net.is_image else 3) or piece.shape[1] < 1 or piece.shape[0] < 1:
            raise ValueError("a piece is (B, n, C, h, w) patches of an image encoder or (B, n, F) feature rows, n >= 1")
        if self._B is None:
            if piece.dtype == torch.uint8:
                net._check_u8(piece)
            elif piece.dtype not in (torch.float32, torch.float16, torch.bfloat16):
                raise TypeError("pieces are float32, float16 / bfloat16 where ips() takes them, or uint8 after set_patch_table; "
                                "got {}".format(piece.dtype))
            elif piece.dtype != torch.float32 and self._on_device:
                # (what the encoder plan would refuse at its first launch: said here, before anything is allocated)
                if hip.precision() == "fp32" or (not net.is_image and hip.precision() != "bf16"):
                    raise TypeError("{} pieces need IPSX_PRECISION=bf16{}".format(piece.dtype, " or fp32x3" if net.is_image else ""))
        else:
            self._check_like_first("piece", piece, piece.shape[0] == self._B and tuple(piece.shape[2:]) == self._row_shape,
                                   lambda: "B = {}, n, {}".format(self._B, ", ".join(str(v) for v in self._row_shape)))
        self._check_fits(piece.shape[1])

    def _check_like_first(self, what, t, same_shape, layout):
        """A later piece / band must look like the first (``layout()``: the shape the stream takes, for the message)."""
        if not same_shape:
            raise ValueError("a {} of shape {} in a stream of ({})".format(what, tuple(t.shape), layout()))
        if t.dtype != self._dtype:
            raise TypeError("a {} {} in a stream of {}".format(t.dtype, what, self._dtype))

    def _check_fits(self, n):
        """Do ``n`` more patches per image still fit the positional table?"""
        net = self.net
        if net.use_pos and self.fed + n > net.pos_enc.shape[1]:
            raise ValueError("{} patches per image pass the {} rows of the positional table (conf.N)".format(
                self.fed + n, net.pos_enc.shape[1]))

    # ------------------------------------------------------------------ feed
    @torch.no_grad()
    def feed(self, piece):
        """Take the next ``piece`` (B, n, ...) of every image.  Stream-ordered on the current stream: when the call
        returns, the caller may overwrite or free the piece with work on that stream.  Host pieces are copied to the
        device as they are."""
        if isinstance(piece, Ragged):
            refuse("ips_stream().feed()")
        if self._geom is not None:
            raise TypeError("this is a row stream (ips_stream(patch_size, patch_stride)): it takes feed_rows(band), not patches")
        self._check(piece)
        if self._B is None:
            self._B, self._row_shape, self._dtype = piece.shape[0], tuple(piece.shape[2:]), piece.dtype
        self._run(piece)
        return self

    def _run(self, piece, view=None):
        """One feed's piece through the selection, in the scoring frame (``IPSNet._scoring``): on the device or on ATen
        ops.  ``view``: ``piece`` is the window of a row stream, its patches those of the view (``_feed_hip``)."""
        net = self.net
        with net._scoring():
            if view is None:
                piece = piece.to(net.device)
                if not piece[0].is_contiguous():  # rows strided inside an image (a crop, channels-last): one copy up front, as ips() makes
                    piece = piece.contiguous()
            if self._on_device:
                self._feed_hip(piece, view)
            else:
                self._feed_aten(piece)
        self.fed += piece.shape[1] if view is None else view.per_image

    # ------------------------------------------------------------------ feed_rows
    def _check_rows(self, band):
        """Everything that refuses a band, before the first launch or allocation of the call -> the geometry's plan."""
        net = self.net
        if self._geom is None:
            raise TypeError("this is a patch stream: feed_rows() goes with ips_stream(patch_size, patch_stride)")
        self._check()
        if not torch.is_tensor(band) or band.dim() != 4 or min(band.shape) < 1:
            raise ValueError("a band is (B, C, h, W): the next h >= 1 pixel rows of every image")
        (ph, pw), (sh, sw) = self._patch_size, self._patch_stride
        B, Cc, h, W = band.shape
        if self._band_shape is None:
            self._check_first_band(band, Cc, self._on_device)
            self._check_patch_fits(W)
        else:
            self._check_like_first("band", band, (B, Cc, W) == self._band_shape,
                                   lambda: "B = {}, C = {}, h, W = {}".format(*self._band_shape))
        plan = self._geom.plan(h)
        self._check_fits(plan[2] * ((W - pw) // sw + 1))
        return plan

    def _window(self, band, drop, rows):
        """The carried rows and the band's rows from ``drop`` on as ONE (B, C, rows, W) tensor on the net's device."""
        B, Cc, _, W = band.shape
        window = torch.empty((B, Cc, rows, W), dtype=band.dtype, device=self.net.device)
        self._fill_window(window, self._carry, band[:, :, drop:])
        return window

    @torch.no_grad()
    def feed_rows(self, band):
        """Take the next pixel rows ``band`` (B, C, h, W) of every image - float32, or uint8 after ``set_patch_table``; on the
        device or on the host.  The patch rows the band completes are this feed's piece (none: nothing is launched).
        Stream-ordered like ``feed``: when the call returns, the caller may overwrite or free the band."""
        if isinstance(band, Ragged):
            refuse("ips_stream().feed_rows()")
        drop, rows, ny_w, carry, _ = self._check_rows(band)
        net = self.net
        (ph, pw), (sh, sw) = self._patch_size, self._patch_stride
        if self._band_shape is None:
            B, Cc, _, W = band.shape
            self._band_shape, self._nx = (B, Cc, W), (W - pw) // sw + 1
            self._B, self._row_shape, self._dtype = B, (Cc, ph, pw), band.dtype
        self._geom.take(band.shape[2])
        if rows == 0:                    # every row of the band lies between two patch rows
            return self
        window = self._window(band, drop, rows)
        self._carry = None
        if ny_w:
            view = None
            # (the frame puts a training NET into eval mode: an encoder that alone is in training mode stays there)
            if self._on_device and not (net.encoder.training and not net.training):
                view = hip.PatchView(window.shape, self._patch_size, self._patch_stride)
                if not net.plan.view_supported(view):
                    view = None
            if view is not None:
                self._run(window, view)
                self.view_feeds += 1
            else:                        # the piece as a patch tensor, through feed()'s path
                self._run(net._materialise(window[:, :, :(ny_w - 1) * sh + ph], self._patch_size, self._patch_stride))
        if carry:                        # (a copy: the window itself is released)
            self._carry = window[:, :, rows - carry:].clone() if ny_w else window
        return self

    # ------------------------------------------------------------------ the ROCm device
    def _scan_workspace(self, dev):
        net = self.net
        ca = net.transf.crs_attn
        return hip.scan_workspace(self._B, net.M, net.I, ca.H, ca.n_token, dev)

    def _encode(self, piece):
        """(B, n, ...) -> (B, n, D) float32, the piece read where it lies: one launch for a contiguous piece, one per image
        for a slice along the patch axis (the rows of an image are contiguous)."""
        net = self.net
        B, n = piece.shape[:2]
        if piece.is_contiguous() or B == 1:
            flat = piece.reshape(B * n, *piece.shape[2:])           # (a view: feed() has made the rows of an image contiguous)
            return net._embed(flat).view(B, n, -1)
        if net.encoder.training:                                     # the stock modules (ips() takes them there too)
            return torch.stack([net._embed(piece[b]) for b in range(B)])
        plan = net.plan
        emb = torch.empty((B, n, net.D), dtype=torch.float32, device=piece.device)
        table = net._table_for(piece)
        with plan.hold():
            for b in range(B):
                plan.encode(piece[b], out=emb[b], table=table)
        return emb

    def _scan(self, n, k):
        """Iterations [0, k) on the first ``n`` rows of the current logits table -> compact rows in ``self._sel``."""
        net = self.net
        ca = net.transf.crs_attn
        hip.scan_range_strided(self._sets[self._cur][3], n, net.M, net.I, ca.H, ca.n_token, 0, k, self._sel, self._tie,
                               self._scan_ws)
        hip.scan.last_tie = self._tie

    def _feed_hip(self, piece, view=None):
        """One feed on the device.  ``view``: ``piece`` is the window (B, C, rows, W) of a row stream and the feed's patches are
        those of its ``hip.PatchView`` - encoded and committed where they lie, no patch tensor."""
        net = self.net
        M, I = net.M, net.I
        n_k, held = piece.shape[1] if view is None else view.per_image, self._held
        if self._sets is None:
            self._allocate(piece.device)
        self._logits_room(held + n_k, piece.device, keep=held)       # (only the held rows of the table hold logits)
        if view is None:
            emb_k = self._encode(piece)
        else:                        # (the view numbers image-major: one launch for all images)
            src = hip.PatchSource(images=piece, view=view, table=net._table_for(piece))
            emb_k = net.plan.encode_source(src, first=0, n=view.count).view(self._B, n_k, -1)
        pos = net.pos_enc[:, self.fed:self.fed + n_k] if net.use_pos else None       # (shared by the images: batch stride 0)
        lg = self._sets[self._cur][3]
        hip.logits(emb_k, pos, net.transf.crs_attn.folded_query(), self._R, out=lg[:, held:held + n_k])
        ids_k = torch.arange(self.fed, self.fed + n_k, dtype=torch.int64, device=piece.device).unsqueeze(0)
        total = held + n_k
        self._advance((total - M) // I if total > M else 0, total, piece, emb_k, ids_k, view)

    def _advance(self, k, total, piece=None, emb_k=None, ids_k=None, view=None):
        """The state update behind ``total`` candidates per image - the held rows and, behind them, a feed's ``piece`` with
        its embeddings and ids (none: the ragged last chunk of ``finish()``): scan ``k`` iterations of the current logits
        table, commit the kept rows and the tail behind iteration k into the OTHER set (ONE launch), flip, count.  ``k`` = 0
        (no chunk is complete): the piece goes behind the held rows of the current set - its logits lie there already.
        ``view``: ``piece`` is a row stream's window, the patch table's piece its view (``hip.stream_commit_view``)."""
        net = self.net
        M, I, held = net.M, net.I, self._held
        cur = self._sets[self._cur]
        dst = self._sets[self._cur ^ 1] if k else cur
        tables = [(cur[0], held, piece if view is None else None, dst[0]), (cur[1], held, emb_k, dst[1]),
                  (cur[2], held, ids_k, dst[2])]
        sel = None
        if k:
            self._scan(total, k)
            sel = self._sel
            if emb_k is not None:    # (finish() scans nothing after its chunk: the logits stay behind)
                tables.append((cur[3], total, None, dst[3]))
        tail_first = min(M + k * I, total) if k else 0
        if view is None:
            hip.stream_commit(tables, sel, M, total, tail_first)
        else:
            hip.stream_commit_view(tables, piece, view, sel, M, total, tail_first)
        if k:
            self._cur ^= 1
        self._held = max(M, total - k * I) if k else total
        self.iterations += k

    # ------------------------------------------------------------------ the CPU device (ATen ops)
    def _iterate_aten(self, chunk):
        """One iteration of ``IPSNet._select_aten``: the memory first, the chunk after."""
        net = self.net
        B, D = self._B, net.D
        lo = self._mem_next
        emb = net._embed(chunk.reshape(-1, *chunk.shape[2:])).view(B, chunk.shape[1], D)
        ids = torch.arange(lo, lo + chunk.shape[1], dtype=torch.int64, device=chunk.device).unsqueeze(0).expand(B, -1)
        self._mem_next = lo + chunk.shape[1]
        if self._mem_emb is None:
            self._mem_emb, self._mem_ids, self._mem_patch = emb, ids, chunk.clone()      # (the caller's piece may be overwritten)
            return
        pos = net.pos_enc.expand(B, -1, -1) if net.use_pos else None
        self._mem_emb, self._mem_ids, top = net._iterate(self._mem_emb, self._mem_ids, emb, ids, pos, rows=True)
        self._mem_patch = net._take(torch.cat((self._mem_patch, chunk), dim=1), top)
        self.iterations += 1

    def _feed_aten(self, piece):
        net = self.net
        M, I = net.M, net.I
        if self._pending is None:
            self._mem_next = 0
        rows = piece if self._pending is None or self._pending.shape[1] == 0 else torch.cat((self._pending, piece), dim=1)
        if self._mem_emb is None and rows.shape[1] >= M:
            self._iterate_aten(rows[:, :M])
            rows = rows[:, M:]
        while self._mem_emb is not None and rows.shape[1] >= I:
            self._iterate_aten(rows[:, :I])
            rows = rows[:, I:]
        self._pending = rows.clone() if rows.shape[1] else rows[:, :0]       # (the caller's piece may be overwritten)

    # ------------------------------------------------------------------ finish
    @torch.no_grad()
    def finish(self):
        """Run the ragged last chunk, if one is left -> (mem_patch (B, M, ...), mem_pos (B, M, D) | None), and set
        ``net.last_mem_idx`` / ``net.last_mem_emb`` as ``ips()`` does.  A total of at most M patches: the fed patches in
        arrival order with ``last_mem_idx = None`` (the ``M >= N`` shortcut of ``ips()``)."""
        self._check()
        net = self.net
        if self._B is None:
            raise RuntimeError("nothing was fed")
        if self._geom is not None and self.fed == 0:
            raise RuntimeError("the {} pixel rows fed complete no patch row of height {}".format(self.rows, self._patch_size[0]))
        M, B = net.M, self._B
        net._reset_last()
        u8 = self._dtype == torch.uint8
        if self.fed <= M:
            mem_patch = (self._sets[self._cur][0][:, :self.fed].clone() if self._on_device else
                         torch.cat((self._mem_patch, self._pending), dim=1) if self._mem_patch is not None else self._pending)
            mem_pos = net.pos_enc[:, :self.fed].expand(B, -1, -1) if net.use_pos else None
            self._close(None)
            return (net._dequant(mem_patch) if u8 else mem_patch), mem_pos
        with net._scoring():
            if self._on_device:
                if self._held > M:       # the ragged last chunk: one more iteration, no tail behind it
                    self._advance(1, self._held)
                patch, emb, ids, _ = self._sets[self._cur]
                mem_patch, mem_emb, mem_idx = patch[:, :M].clone(), emb[:, :M].clone(), ids[:, :M].clone()
            else:
                if self._pending.shape[1]:
                    self._iterate_aten(self._pending)
                mem_patch, mem_emb, mem_idx = self._mem_patch, self._mem_emb, self._mem_ids
            mem_pos = net._take(net.pos_enc.expand(B, -1, -1), mem_idx) if net.use_pos else None
            if u8:                       # the M selected patches leave as float32
                mem_patch = net._dequant(mem_patch)
        self._close(mem_idx)
        net.last_mem_idx, net._mem_emb = mem_idx, mem_emb
        return mem_patch, mem_pos

    def _close(self, mem_idx):
        self._last_idx = mem_idx
        self._release()
        self._mem_patch = self._mem_emb = self._mem_ids = self._pending = None
