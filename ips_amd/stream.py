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
"""

import torch

from . import hip


class IPSStream:
    """The state of one streamed selection.  ``fed``: patches per image so far; ``iterations``: completed iterations;
    ``mem_idx``: (B, M) int64 global patch numbers in the order of the last completed iteration (None until M patches
    have arrived)."""

    def __init__(self, net):
        self.net = net
        self.fed = 0
        self.iterations = 0
        self._finished = False
        self._generation = hip.weights_generation()
        self._B = self._row_shape = self._dtype = None
        self._on_device = hip.on_device(net.device)
        # device state
        self._sets = None            # [[patch, emb, ids, logits], [...]]: the two buffer sets
        self._cur = 0
        self._held = 0               # valid rows per image in the current set
        self._sel = self._tie = self._scan_ws = None
        # ATen state
        self._mem_patch = self._mem_emb = self._mem_ids = None
        self._pending = None         # (B, t, ...) rows no iteration has consumed

    # ------------------------------------------------------------------ observable state
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
        if self._finished:
            raise RuntimeError("this stream has finished (IPSNet.ips_stream() starts another)")
        if hip.dedup_blank():
            raise TypeError("blank-patch dedup needs the whole input (IPSX_DEDUP_BLANK=1 with ips_stream)")
        if hip.weights_generation() != self._generation:
            raise RuntimeError("the weights changed since this stream began (an optimizer step between feeds would mix "
                               "embeddings of two weight sets)")
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
            if piece.shape[0] != self._B or tuple(piece.shape[2:]) != self._row_shape:
                raise ValueError("a piece of shape {} in a stream of (B = {}, n, {})".format(
                    tuple(piece.shape), self._B, ", ".join(str(v) for v in self._row_shape)))
            if piece.dtype != self._dtype:
                raise TypeError("a {} piece in a stream of {}".format(piece.dtype, self._dtype))
        if net.use_pos and self.fed + piece.shape[1] > net.pos_enc.shape[1]:
            raise ValueError("{} patches per image pass the {} rows of the positional table (conf.N)".format(
                self.fed + piece.shape[1], net.pos_enc.shape[1]))

    # ------------------------------------------------------------------ feed
    @torch.no_grad()
    def feed(self, piece):
        """Take the next ``piece`` (B, n, ...) of every image.  Stream-ordered on the current stream: when the call
        returns, the caller may overwrite or free the piece with work on that stream.  Host pieces are copied to the
        device as they are."""
        self._check(piece)
        net = self.net
        if self._B is None:
            self._B, self._row_shape, self._dtype = piece.shape[0], tuple(piece.shape[2:]), piece.dtype
        was_training = net.training
        if was_training:                 # IPS always scores with running BN statistics and no dropout
            net.encoder.eval()
            net.transf.eval()
        try:
            piece = piece.to(net.device)
            if not piece[0].is_contiguous():      # rows strided inside an image (a crop, channels-last): one copy up front, as ips() makes
                piece = piece.contiguous()
            if self._on_device:
                self._feed_hip(piece)
            else:
                self._feed_aten(piece)
        finally:
            if was_training:
                net.encoder.train()
                net.transf.train()
        self.fed += piece.shape[1]
        return self

    # ------------------------------------------------------------------ the ROCm device
    def _allocate(self, piece):
        net = self.net
        B, dev, cap = self._B, piece.device, net.M + net.I - 1
        ca = net.transf.crs_attn
        R = ca.H * ca.n_token
        self._sets = [[torch.empty((B, cap) + self._row_shape, dtype=self._dtype, device=dev),
                       torch.empty((B, cap, net.D), dtype=torch.float32, device=dev),
                       torch.empty((B, cap), dtype=torch.int64, device=dev),
                       None] for _ in range(2)]
        self._sel = torch.empty((B, net.M), dtype=torch.int64, device=dev)
        self._tie = torch.zeros((B,), dtype=torch.int32, device=dev)
        self._scan_ws = hip.scan_workspace(B, net.M, net.I, ca.H, ca.n_token, dev)
        self._R = R

    def _logits_room(self, rows, dev):
        """The logits tables hold the held rows AND the piece's: they grow with the largest piece (R floats per row)."""
        cur = self._sets[self._cur][3]
        if cur is not None and cur.shape[1] >= rows:
            return
        new = [torch.empty((self._B, rows, self._R), dtype=torch.float32, device=dev) for _ in range(2)]
        if cur is not None and self._held:
            new[self._cur][:, :self._held].copy_(cur[:, :self._held])
        for k in range(2):
            self._sets[k][3] = new[k]

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
        if net._plan is None:
            net._plan = hip.EncoderPlan(net.encoder, net.is_image)
        emb = torch.empty((B, n, net.D), dtype=torch.float32, device=piece.device)
        table = net._table_for(piece)
        with net._plan.hold():
            for b in range(B):
                net._plan.encode(piece[b], out=emb[b], table=table)
        return emb

    def _scan(self, n, k):
        """Iterations [0, k) on the first ``n`` rows of the current logits table -> compact rows in ``self._sel``."""
        net = self.net
        ca = net.transf.crs_attn
        hip.scan_range_strided(self._sets[self._cur][3], n, net.M, net.I, ca.H, ca.n_token, 0, k, self._sel, self._tie,
                               self._scan_ws)
        hip.scan.last_tie = self._tie

    def _feed_hip(self, piece):
        net = self.net
        M, I = net.M, net.I
        n_k, held = piece.shape[1], self._held
        if self._sets is None:
            self._allocate(piece)
        self._logits_room(held + n_k, piece.device)
        patch, emb, ids, lg = self._sets[self._cur]
        emb_k = self._encode(piece)
        pos = net.pos_enc[:, self.fed:self.fed + n_k] if net.use_pos else None       # (shared by the images: batch stride 0)
        hip.logits(emb_k, pos, net.transf.crs_attn.folded_query(), self._R, out=lg[:, held:held + n_k])
        ids_k = torch.arange(self.fed, self.fed + n_k, dtype=torch.int64, device=piece.device).unsqueeze(0)
        total = held + n_k
        k = (total - M) // I if total > M else 0
        if k == 0:                   # no chunk is complete: the piece goes behind the held rows (its logits lie there already)
            hip.stream_commit([(patch, held, piece, patch), (emb, held, emb_k, emb), (ids, held, ids_k, ids)], None, M, total)
            self._held = total
            return
        self._scan(total, k)
        nxt = self._sets[self._cur ^ 1]
        hip.stream_commit([(patch, held, piece, nxt[0]), (emb, held, emb_k, nxt[1]), (ids, held, ids_k, nxt[2]),
                           (lg, total, None, nxt[3])], self._sel, M, total, M + k * I)
        self._cur ^= 1
        self._held = total - k * I
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
        cand_emb = torch.cat((self._mem_emb, emb), dim=1)
        cand_ids = torch.cat((self._mem_ids, ids), dim=1)
        cand_pos = None
        if net.use_pos:
            cand_pos = cand_emb + torch.gather(net.pos_enc.expand(B, -1, -1), 1, cand_ids.unsqueeze(-1).expand(-1, -1, D))
        rows = torch.arange(cand_ids.shape[1], dtype=torch.int64, device=chunk.device).unsqueeze(0).expand(B, -1)
        self._mem_emb, top = net.score_and_select(cand_emb, cand_pos, net.M, rows)      # (top: compact candidate rows)
        self._mem_ids = torch.gather(cand_ids, 1, top)
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
        M, B = net.M, self._B
        net._emb_parts = net._mem_emb = None
        net.last_shuffle = None
        u8 = self._dtype == torch.uint8
        if self.fed <= M:
            mem_patch = (self._sets[self._cur][0][:, :self.fed].clone() if self._on_device else
                         torch.cat((self._mem_patch, self._pending), dim=1) if self._mem_patch is not None else self._pending)
            mem_pos = net.pos_enc[:, :self.fed].expand(B, -1, -1) if net.use_pos else None
            self._close(None)
            net.last_mem_idx = None
            return (net._dequant(mem_patch) if u8 else mem_patch), mem_pos
        was_training = net.training
        if was_training:
            net.encoder.eval()
            net.transf.eval()
        try:
            if self._on_device:
                if self._held > M:       # the ragged last chunk: one more iteration, no tail behind it
                    self._scan(self._held, 1)
                    cur, nxt = self._sets[self._cur], self._sets[self._cur ^ 1]
                    hip.stream_commit([(cur[0], self._held, None, nxt[0]), (cur[1], self._held, None, nxt[1]),
                                       (cur[2], self._held, None, nxt[2])], self._sel, M, self._held, self._held)
                    self._cur ^= 1
                    self._held = M
                    self.iterations += 1
                patch, emb, ids, _ = self._sets[self._cur]
                mem_patch, mem_emb, mem_idx = patch[:, :M].clone(), emb[:, :M].clone(), ids[:, :M].clone()
            else:
                if self._pending.shape[1]:
                    self._iterate_aten(self._pending)
                mem_patch, mem_emb, mem_idx = self._mem_patch, self._mem_emb, self._mem_ids
            mem_pos = net._take(net.pos_enc.expand(B, -1, -1), mem_idx) if net.use_pos else None
            if u8:                       # the M selected patches leave as float32
                mem_patch = net._dequant(mem_patch)
        finally:
            if was_training:
                net.encoder.train()
                net.transf.train()
        self._close(mem_idx)
        net.last_mem_idx, net._mem_emb = mem_idx, mem_emb
        return mem_patch, mem_pos

    def _close(self, mem_idx):
        self._finished, self._last_idx = True, mem_idx
        self._sets = self._sel = self._scan_ws = None
        self._mem_patch = self._mem_emb = self._mem_ids = self._pending = None
