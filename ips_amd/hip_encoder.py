"""``EncoderPlan``: the device-side description of ``IPSNet.encoder`` (packed weights + BatchNorm affines) and the entry
points that run it - the fused trunks, the layer-by-layer trunk, the projector and the two persistent producer streams
(split out of ``hip.py`` in round 6; ``ips_amd.hip`` re-exports every name, so ``hip.EncoderPlan`` etc. are unchanged).
Reference: ``IPSNet.encoder``, architecture/ips_net.py:17-60."""

import collections
import ctypes as C
import os

import torch

from .hip import (lib, _ck, _call_twin, _p, _f32, _stream, _patches, PatchSource, PatchView, _PATCH_DTYPES, Conv, Block, Trunk, precision, dedup_blank, weights_generation)


# ------------------------------------------------------------------ encoder plan
def _bn_affine(bn, bias=None):
    """Per-channel (alpha, shift) of an eval-mode BatchNorm, on the device."""
    c = bn.num_features
    out = torch.empty((2, c), dtype=torch.float32, device=bn.weight.device)
    lin_bias = _f32(bias.detach()) if bias is not None else None
    _ck(lib().ipsx_bn_affine(_p(_f32(bn.weight.detach())), _p(_f32(bn.bias.detach())),
                             _p(_f32(bn.running_mean)), _p(_f32(bn.running_var)), _p(lin_bias),
                             C.c_float(bn.eps), c, _p(out[0]), _p(out[1]), _stream()), "ipsx_bn_affine")
    return out


def _pack_conv(weight):
    co, ci, kh, kw = weight.shape
    n = lib().ipsx_packed_conv_weight_elems(co, ci, kh, kw)
    packed = torch.empty(n, dtype=torch.float32, device=weight.device)
    _ck(lib().ipsx_pack_conv_weight(_p(_f32(weight.detach())), co, ci, kh, kw, _p(packed), _stream()),
        "ipsx_pack_conv_weight")
    return packed


def _is_tile16(conv):
    """A 3x3 convolution 128 -> 128 of stride 1 and pad 1: the 4x4 stage of the fused 1x32x32 trunk."""
    return (conv.in_channels == 128 and conv.out_channels == 128 and tuple(conv.kernel_size) == (3, 3)
            and tuple(conv.stride) == (1, 1) and tuple(conv.padding) == (1, 1))


class _PlanHold:
    """``EncoderPlan.hold()``: the plan's weight check runs on entry and is skipped until exit."""
    __slots__ = ("plan",)

    def __init__(self, plan):
        self.plan = plan

    def __enter__(self):
        self.plan._refresh()
        self.plan._held += 1

    def __exit__(self, *exc):
        self.plan._held -= 1


class EncoderPlan:
    """Device-side description of ``IPSNet.encoder``: packed weights + BN affines.

    Parameters change every optimiser step and BatchNorm running statistics move
    in every training-mode forward, so the plan is keyed on the tensors'
    ``_version`` counters / storage pointers and re-packed when any moved.
    """

    def __init__(self, encoder, is_image):
        self.encoder, self.is_image = encoder, is_image
        self._sig = None
        self._holders = None
        self._keep = []
        self._ws = None
        self._ws_small = 0
        self._held = 0
        self.blank_emb = None      # the fused fp32 trunk's embedding of a blank patch that blank_embedding() returned last
        self._blank = {}           # per kind "f32" | "u8": (the row, (stream it was made on, event behind its launch), table, its version)
        self.n_encoded = None      # device int32: what the last dedup call really encoded
        self.bf16 = False          # feature nets: the projector runs on the bf16 matrix pipe (IPSX_PRECISION=bf16)

    def _features(self, x):
        """Feature rows as the projector reads them: float32, or float16 / bfloat16 under the bf16 projector, which widens
        them in its operand load.  Shapes the bf16 projector does not take raise here, before the first launch."""
        if x.dtype in (torch.float16, torch.bfloat16):
            if not self.bf16:
                raise TypeError("{} features need IPSX_PRECISION=bf16 (the {} projector reads float32)".format(x.dtype, precision()))
        else:
            x = _f32(x)
        if self.bf16 and not lib().ipsx_projector_bf16_supported(C.byref(self.lin)):
            raise ValueError("the bf16 projector needs F % 16 == 0 and D % 32 == 0, got F = {}, D = {}".format(
                self.lin.c_in, self.lin.c_out))
        return x if x.is_contiguous() else x.contiguous()

    @staticmethod
    def _index(index, x):
        """A row index of the projector's indexed entry points: flat int32 row numbers into ``x`` (P, F), contiguous, on its device."""
        if index.dtype != torch.int32 or index.dim() != 1 or not index.is_contiguous() or index.device != x.device:
            raise ValueError("index must be a contiguous 1-d int32 tensor on the rows' device")
        return index

    def _stats(self, x, out, index=None):
        if index is not None:
            _ck(lib().ipsx_projector_stats_indexed(_p(x), _PATCH_DTYPES[x.dtype], _p(index), x.shape[0], index.numel(), x.shape[1],
                                                   C.c_float(self.ln_eps), _p(out), _stream()), "ipsx_projector_stats_indexed")
            return out
        _ck(lib().ipsx_projector_stats_typed(_p(x), _PATCH_DTYPES[x.dtype], x.shape[0], x.shape[1], C.c_float(self.ln_eps),
                                             _p(out), _stream()), "ipsx_projector_stats_typed")
        return out

    def _walk(self):
        """The module tree, flattened ONCE: every module's child dictionary (the structural fingerprint is the ids of their
        values, re-read in every call - plain dictionary reads, ~5 us for a ResNet trunk, where ``encoder.modules()`` costs
        ~100 us in front of the first launch of EVERY ips() call), the (dictionary, key) slot of every parameter / buffer
        that exists, and the slots that are None today (a bias or a running statistic that appears later is seen)."""
        kids, slots, empty = [], [], []
        for mod in self.encoder.modules():
            kids.append(mod._modules)
            for d in (mod._parameters, mod._buffers):
                for k, t in d.items():
                    (slots if t is not None else empty).append((d, k))
        return kids, slots, empty

    @staticmethod
    def _structure(kids):
        return tuple(id(c) for d in kids for c in d.values())

    def _signature(self):
        """(storage pointer, version counter) of every parameter and buffer + the ids of every child module: a tensor that
        is replaced, moved or written in place, a child module exchanged at ANY depth (``layer2[0].bn1 = ...``,
        ``convert_sync_batchnorm``), an entry that appears, disappears or stops being None - each re-packs the plan."""
        h = self._holders
        if h is not None:
            try:
                if self._structure(h[1]) != h[0] or any(d[k] is not None for d, k in h[3]):
                    h = None
            except KeyError:
                h = None
        for _ in range(2):
            if h is None:
                kids, slots, empty = self._walk()
                h = self._holders = (self._structure(kids), kids, slots, empty)
            sig = [precision(), weights_generation(), h[0]]
            try:
                for d, k in h[2]:
                    t = d[k]
                    sig.append((t.data_ptr(), t._version))
                return tuple(sig)
            except (KeyError, AttributeError):         # an entry was removed / set to None since the walk: walk again
                h = None
        raise RuntimeError("EncoderPlan: the encoder's parameters changed while they were being read")

    def _conv(self, conv, bn, prec=0, stem=False):
        packed = _pack_conv(conv.weight)
        aff = _bn_affine(bn)
        self._keep += [packed, aff]
        half = None
        if prec and stem:
            if tuple(conv.weight.shape[1:]) == (1, 7, 7):     # the split trunks exist for the 1x32x32 stem only
                w = _f32(conv.weight.detach())
                planes = 1 if prec == 1 else 3
                half = torch.empty(lib().ipsx_packed_stem_weight_split_bytes(w.shape[0], planes), dtype=torch.uint8, device=w.device)
                _ck(lib().ipsx_pack_stem_weight_split(_p(w), w.shape[0], planes, _p(half), _stream()), "ipsx_pack_stem_weight_split")
                self._keep.append(half)
        elif prec:
            w = _f32(conv.weight.detach())
            co, ci, kh, kw = w.shape
            size, pack = ((lib().ipsx_packed_conv_weight_bf16_bytes, lib().ipsx_pack_conv_weight_bf16) if prec == 1 else
                          (lib().ipsx_packed_conv_weight_x3_bytes, lib().ipsx_pack_conv_weight_x3))
            half = torch.empty(size(co, ci, kh, kw), dtype=torch.uint8, device=w.device)
            _ck(pack(_p(w), co, ci, kh, kw, _p(half), _stream()), "ipsx_pack_conv_weight_bf16/x3")
            self._keep.append(half)
        elif not stem and _is_tile16(conv):
            # the fp32 fused trunk's 16-row tiles (csrc/fused_trunk.hip: conv_t16) read these three convolutions in a packing
            # of their own, carried in the descriptor's second pointer, which nothing else reads at precision 0
            w = _f32(conv.weight.detach())
            co, ci, kh, kw = w.shape
            half = torch.empty(lib().ipsx_packed_conv_weight_tile16_elems(co, ci, kh, kw), dtype=torch.float32, device=w.device)
            _ck(lib().ipsx_pack_conv_weight_tile16(_p(w), co, ci, kh, kw, _p(half), _stream()), "ipsx_pack_conv_weight_tile16")
            self._keep.append(half)
        return Conv(conv.in_channels, conv.out_channels, conv.kernel_size[0], conv.kernel_size[1],
                    conv.stride[0], conv.padding[0], _p(packed), _p(aff[0]), _p(aff[1]), _p(half))

    def _rebuild(self):
        self._keep = []
        self.blank_emb = None
        self._blank = {}
        enc = self.encoder
        if self.is_image:
            mods = list(enc.children())
            bf16 = {"fp32": 0, "bf16": 1, "fp32x3": 2}[precision()]
            blocks = []
            for stage in mods[4:-1]:
                for blk in stage.children():
                    b = Block()
                    pairs = [(getattr(blk, "conv%d" % i), getattr(blk, "bn%d" % i))
                             for i in (1, 2, 3) if hasattr(blk, "conv%d" % i)]
                    b.n_conv = len(pairs)
                    for j, (cv, bn) in enumerate(pairs):
                        b.conv[j] = self._conv(cv, bn, bf16)
                    b.has_down = int(blk.downsample is not None)
                    if b.has_down:
                        b.down = self._conv(blk.downsample[0], blk.downsample[1], bf16)
                    blocks.append(b)
            self._blocks = (Block * len(blocks))(*blocks)
            t = Trunk()
            t.stem = self._conv(mods[0], mods[1], bf16, stem=True)
            t.c_in = mods[0].in_channels
            t.n_block = len(blocks)
            t.blocks = C.cast(self._blocks, C.POINTER(Block))
            t.precision = bf16
            t.patch_dtype = 0
            self.trunk = t
            self.d_out = blocks[-1].conv[blocks[-1].n_conv - 1].c_out
        else:
            ln, lin, bn = enc[0], enc[1], enc[2]
            w = lin.weight.detach()
            packed = _pack_conv(w.reshape(w.shape[0], w.shape[1], 1, 1))
            aff = _bn_affine(bn, bias=lin.bias)
            # the LayerNorm in front of the Linear is folded into the GEMM's epilogue: rstd * (x W^T - mean * colsum(W))
            colsum = torch.empty(w.shape[0], dtype=torch.float32, device=w.device)
            wf = _f32(w)
            _ck(lib().ipsx_weight_colsum(_p(wf), w.shape[0], w.shape[1], _p(colsum), _stream()), "ipsx_weight_colsum")
            self._keep += [packed, aff, colsum, wf]
            half = None
            if precision() == "bf16":
                # the bf16 projector's B operand (csrc/projector_bf16.hip): W rounded to bf16, viewed as a 1x1 convolution
                half = torch.empty(lib().ipsx_packed_conv_weight_bf16_bytes(w.shape[0], w.shape[1], 1, 1), dtype=torch.uint8,
                                   device=w.device)
                _ck(lib().ipsx_pack_conv_weight_bf16(_p(wf), w.shape[0], w.shape[1], 1, 1, _p(half), _stream()),
                    "ipsx_pack_conv_weight_bf16")
                self._keep.append(half)
            self.bf16 = half is not None
            self.lin = Conv(w.shape[1], w.shape[0], 1, 1, 1, 0, _p(packed), _p(aff[0]), _p(aff[1]), _p(half), _p(colsum))
            self.ln_eps = float(ln.eps)
            self.d_out = w.shape[0]

    def _workspace(self, nbytes, device):
        # grown on demand; given back when much smaller requests keep coming (one large evaluation call must not pin
        # tens of GiB for the rest of a training run) - after several in a row, not after one: lazy slabs of 1/6, 1/2 and
        # full size, or an eval call between training steps, would otherwise free and re-allocate gigabytes per call
        small = self._ws is not None and self._ws.numel() > (256 << 20) and nbytes < self._ws.numel() // 4
        self._ws_small = self._ws_small + 1 if small else 0
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != device or self._ws_small >= 8:
            self._ws = None
            self._ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
            self._ws_small = 0
        return self._ws

    def _refresh(self):
        if self._held:
            return
        sig = self._signature()
        if sig != self._sig:
            self._rebuild()
            self._sig = sig

    def hold(self):
        """Context manager: check the weights once, then skip the check until the block ends - for a caller that makes
        several encode calls while the weights cannot change (one no-grad ``ips()`` call; the check walks ~80 tensors)."""
        return _PlanHold(self)

    def fused(self, x_shape):
        """True when encode_indexed is available for patches of this (C, h, w)."""
        if not self.is_image:
            return False
        self._refresh()
        t = self._describe(x_shape)
        return x_shape[-3] == t.c_in and lib().ipsx_trunk_kernel(C.byref(t)).startswith(b"fused")

    def _describe(self, patch_shape, patch_dtype=0):
        """The trunk struct, told the (..., C, h, w) patches and storage type the next library call is about.  Every
        question and every encode call says this itself; none relies on what an earlier one wrote."""
        t = self.trunk
        t.h, t.w, t.patch_dtype = patch_shape[-2], patch_shape[-1], patch_dtype
        return t

    def blank_embedding(self, src):
        """(1, D) embedding of a blank patch of ``src``'s shape on the fused fp32 trunk, by the counted launch's own kernel
        on one patch: all 0.0f through ``ipsx_trunk_encode_parts`` for float32 patches and images, all bytes 0 - every pixel
        ``table[c][0]``, which need not be 0.0f - through ``ipsx_trunk_encode_parts_u8`` for uint8 ones.  A view shares its
        tensor kind's row (held to the bit by tests/test_dedup_sources.py).  Kept per kind until ``_refresh()`` sees the
        weights change (``_rebuild`` drops both), the bytes' also only while the table is the same tensor, unwritten
        (the tensor is held here, so its address cannot come back as another table's).  One tiny launch per state, on the
        stream that is current then; a call on another stream waits for that launch's event.  ``blank_emb`` is the row the
        last call returned."""
        dev, tab = src.device, src.table
        kind = "f32" if tab is None else "u8"
        held = self._blank.get(kind)
        if held is not None and (held[0].device != dev or held[2] is not tab or (tab is not None and held[3] != tab._version)):
            held = None
        if held is None:
            zero = torch.zeros((1,) + tuple(src.shape[-3:]), dtype=torch.float32 if tab is None else torch.uint8, device=dev)
            words = torch.zeros((2,), dtype=torch.int32, device=dev)       # the list [0] | the part's counter
            out = torch.empty((1, self.d_out), dtype=torch.float32, device=dev)
            tr, tail = C.byref(self._describe(zero.shape, 0)), (_p(words[0:1]), 1, _p(out), (C.c_int64 * 1)(1), 1, _p(words[1:2]), _stream())
            _call_twin("ipsx_trunk_encode_parts", (tr, _p(zero)), tab, tail)
            ready = (torch.cuda.current_stream(dev), torch.cuda.Event())
            ready[1].record()
            held = self._blank[kind] = (out, ready, tab, None if tab is None else tab._version)
        elif torch.cuda.current_stream(dev) != held[1][0]:
            torch.cuda.current_stream(dev).wait_event(held[1][1])          # made on another stream: behind its launch
        self.blank_emb = held[0]
        return self.blank_emb

    def encode_source(self, src, index=None, first=0, n=None, parts=None, out=None, dedup=False):
        """The image trunk on patches of ``src`` (a ``hip.PatchSource``) -> (n, D) embeddings: of its patches ``index``
        (int32 numbers, on the device), or ``first .. first + n - 1`` (default: all from ``first`` on).  The ONE way into the
        ``ipsx_trunk_encode*`` family; which export runs follows from the source (float32 / half / uint8 patches, a view
        of float32 or uint8 images)
        and from how it is addressed.  An index list: the fused 1x32x32 trunk, or a view on any trunk that reads one.
        ``parts`` = (part_end, done): ``index`` is the index lists of several parts one after the other, ending at the
        list entries ``part_end`` (ints), encoded as ONE launch that counts part k's finished patches into ``done[k]``
        (int32 on the GPU, zeroed by the caller on this stream) - float32 patches, uint8 patches with their table, or a view
        of float32 or uint8 images, on the exact fp32 fused trunk.  ``dedup`` (with ``parts``, any of those four): exact
        blank-patch dedup inside that launch (``ipsx_trunk_encode_parts_dedup`` and its ``_u8`` / ``_view`` / ``_view_u8``
        twins) - the same bits, the rows of the all-zero (bytes: all-zero-byte) entries written from ``blank_embedding``;
        ``n_encoded`` then holds the number of entries the trunk encoded.  A source with a ``hip.RaggedView`` (images of
        different sizes in one packed buffer; float32 pixels, or uint8 pixels with their table - the ``_u8``
        exports, the bits of the float32 expansion ``table[c][byte]``): ``index`` / ``first`` count packed patches, no ``parts``
        (``ipsx_trunk_encode_ragged_view``); ``dedup`` there, on the fused 1x32x32 trunk only (ValueError on any other): the
        explicit route on plain launches - blank scan through the view, ordered compaction, the trunk over the non-blank
        entries and ONE blank one, scatter (``ipsx_trunk_encode_ragged_view_dedup``) - the same bits, and ``n_encoded`` is set."""
        self._refresh()
        # the trunk struct describes THIS call's patches: nothing an earlier call or question left in it is read
        t, L = self._describe(src.shape, 0 if src.table is not None else _PATCH_DTYPES[src.dtype]), lib()
        if src.shape[-3] != t.c_in:
            raise ValueError("patches have {} channels, encoder expects {}".format(src.shape[-3], t.c_in))
        if src.is_view and not L.ipsx_trunk_view_supported(C.byref(t), C.byref(src.view.struct)):
            raise ValueError("this encoder does not read patches through a view (EncoderPlan.view_supported)")
        rv = C.byref(src.ragged.struct) if src.ragged is not None else None
        if rv is not None and (parts is not None or not L.ipsx_trunk_ragged_view_supported(C.byref(t), rv)):
            raise ValueError("this encoder does not read patches through a ragged view (EncoderPlan.ragged_view_supported; "
                             "no parts)")
        if rv is not None and dedup and not L.ipsx_trunk_kernel(C.byref(t)).startswith(b"fused"):
            raise ValueError("blank-patch dedup on a ragged view runs on the fused 1x32x32 trunk only (EncoderPlan.fused)")
        if index is not None:
            if index.dtype != torch.int32 or index.dim() != 1 or not index.is_contiguous() or index.device != src.device:
                raise ValueError("index must be a contiguous 1-d int32 tensor on the patches' device")
            first, n = 0, index.numel()
        elif n is None:
            n = src.count - first
        if first < 0 or n < 0 or (index is None and first + n > src.count):
            raise ValueError("patches {} .. {} of a source of {}".format(first, first + n, src.count))
        if out is None:
            out = torch.empty((n, self.d_out), dtype=torch.float32, device=src.device)
        if n == 0:
            return out
        if index is not None and not src.is_view and rv is None and not L.ipsx_trunk_kernel(C.byref(t)).startswith(b"fused"):
            # a layer-by-layer trunk: its LDS-staging stems take an index list through a view - the patch tensor as
            # src.count images of ONE patch each, grid patch p = patch p
            view = self._rows_view(src.shape)
            if not L.ipsx_trunk_view_supported(C.byref(t), C.byref(view.struct)):
                raise ValueError("this encoder's stem takes no index list (EncoderPlan.index_list_supported)")
            src = PatchSource(images=src.patches.view(-1, *src.shape[-3:]), view=view, table=src.table)
        tr, vs = C.byref(t), C.byref(src.view.struct) if src.is_view else None
        # Every export of the family is name(trunk, base, [table,] ...): the storage's rule (_call_twin) picks the _u8 twin and
        # puts the table behind the base pointer; the view's struct, where there is one, leads what follows
        tab, base = src.table, src.base
        if parts is not None:
            if index is None or not (src.dtype == torch.float32 or (src.dtype == torch.uint8 and tab is not None)):
                raise TypeError("parts=(part_end, done) take float32 patches, or uint8 patches with their table, and the "
                                "parts' index lists")
            ends, done = (C.c_int64 * len(parts[0]))(*parts[0]), _p(parts[1])
            kind = "_view" if vs is not None else ""
            args = ((vs,) if vs is not None else ()) + (_p(index), n, _p(out), ends, len(ends), done)
            if dedup:
                # exact blank-patch dedup inside the launch: the blank embedding of this weight state (bytes: and of this
                # table) goes in front
                blank = self.blank_embedding(src)
                self._describe(src.shape, 0)               # (blank_embedding described its own patch)
                nb = L.ipsx_trunk_parts_dedup_workspace_bytes(tr, n)
                if self.n_encoded is None or self.n_encoded.device != src.device:
                    self.n_encoded = torch.zeros((), dtype=torch.int32, device=src.device)
                _call_twin("ipsx_trunk_encode_parts_dedup" + kind, (tr, _p(base)), tab,
                           args + (_p(blank), _p(self._workspace(nb, src.device)), nb, _p(self.n_encoded), _stream()))
            else:
                _call_twin("ipsx_trunk_encode_parts" + kind, (tr, _p(base)), tab, args + (_stream(),))
            return out
        if index is not None and vs is None and rv is None:    # a patch tensor through an index list: the fused trunk
            _call_twin("ipsx_trunk_encode_indexed", (tr, _p(base)), tab, (_p(index), n, _p(out), _stream()))
            return out
        if rv is not None and dedup:                           # the explicit dedup route through the ragged view
            nb = L.ipsx_trunk_ragged_view_dedup_workspace_bytes(tr, n)
            if self.n_encoded is None or self.n_encoded.device != src.device:
                self.n_encoded = torch.zeros((), dtype=torch.int32, device=src.device)
            # (whole uint8 images: the ONE blank entry is read from its image)
            _call_twin("ipsx_trunk_encode_ragged_view_dedup", (tr, _p(base)), tab,
                       (rv, _p(index), first, n, _p(out), _p(self._workspace(nb, src.device)), nb, _p(self.n_encoded), _stream()))
            return out
        flat = base if vs is not None or rv is not None else base.view(-1, *src.shape[-3:])

        def run(lo, cnt, ws, nb):
            """Patches lo .. lo + cnt of the call - the library's own rule for "the source from patch lo on": the index is
            advanced, else the view's first patch, else the tensor."""
            tail = (cnt, _p(out[lo:lo + cnt]), _p(ws), nb, _stream())
            if rv is not None or vs is not None:           # whole images (of different sizes: index and first count packed patches)
                ix, lo1 = (_p(index[lo:]), 0) if index is not None else (None, first + lo)
                name, grid = ("ipsx_trunk_encode_ragged_view", rv) if rv is not None else ("ipsx_trunk_encode_view", vs)
                _call_twin(name, (tr, _p(flat)), tab, (grid, ix, lo1) + tail)
            else:
                _call_twin("ipsx_trunk_encode", (tr, _p(flat[first + lo:])), tab, tail)

        # Layer-by-layer trunks: the batch goes through in two halves on two streams.  The stem and the max-pool are
        # HBM-bound (together 11-13 % of the trunk's time for 1 % of its arithmetic), the residual stages MFMA-bound:
        # side by side, one half's stem / pool / epilogues fill what the other half's convolutions leave idle
        # (50-px MNIST 14.25 -> 13.89 ms, traffic signs 22.75 -> 22.11 ms; three streams gain less).  Same kernels on
        # the same patches: results are unchanged.  IPSX_LAYERED_STREAMS=1 switches it off.
        ns = int(os.environ.get("IPSX_LAYERED_STREAMS", "2"))
        if ns > 1 and n >= 1024 and not L.ipsx_trunk_kernel(tr).startswith(b"fused"):
            cuts = [n * k // ns for k in range(ns + 1)]
            nb = L.ipsx_trunk_workspace_bytes(tr, max(cuts[k + 1] - cuts[k] for k in range(ns)))
            # the library's budget (a share of the free memory) is per CALL: the ns concurrent calls split it - each
            # chunks its part of the batch to the workspace it is given
            budget = L.ipsx_trunk_workspace_bytes(tr, 1 << 40)
            nb = min(nb, max(budget // ns, L.ipsx_trunk_workspace_bytes(tr, 1)))
            nb -= nb % 256
            ws = self._workspace(ns * nb, src.device)
            if len(getattr(self, "_sides", [])) < ns - 1:
                self._sides = [torch.cuda.Stream(device=src.device) for _ in range(ns - 1)]
            main = torch.cuda.current_stream(src.device)
            for k in range(1, ns):
                st = self._sides[k - 1]
                st.wait_stream(main)
                with torch.cuda.stream(st):
                    run(cuts[k], cuts[k + 1] - cuts[k], ws[k * nb:], nb)
            run(0, cuts[1], ws[:nb], nb)
            for st in self._sides[:ns - 1]:
                main.wait_stream(st)
            return out
        nb = L.ipsx_trunk_workspace_bytes(tr, n)
        run(0, n, self._workspace(nb, src.device), nb)
        return out

    @staticmethod
    def _rows_view(patch_shape):
        """A (..., C, h, w) patch tensor as a view: its patches are images of one patch each."""
        c, h, w = (int(v) for v in patch_shape[-3:])
        return PatchView((int(torch.Size(patch_shape[:-3]).numel()), c, h, w), (h, w), (h, w))

    def index_list_supported(self, patch_shape):
        """Does ``encode_source`` take an index list into a patch tensor of this (..., C, h, w)?  The fused 1x32x32 trunk
        (``fused``), and the layer-by-layer trunks whose stem stages its patch into LDS (1x50x50, 3x100x100, exact fp32):
        they read the list as they read a view's.  The generic stem (``conv_any_kernel``) takes none."""
        if not self.is_image:
            return False
        return self.fused(patch_shape) or self.view_supported(self._rows_view(patch_shape))

    # ---- the entry points of old, each a source and the one call
    def encode_indexed(self, flat, index, table=None, parts=None):
        """flat (P, C, h, w) contiguous on the GPU (uint8: with its ``table`` (C, 256)), index (n,) int32 -> (n, D)
        embeddings of flat[index]; ``parts``: as ``encode_source``."""
        return self.encode_source(PatchSource(flat, table), index=index, parts=parts)

    def encode_view(self, images, view, index=None, first=0, n=None, parts=None, table=None):
        """images (B, C, H, W) float32 on the GPU + their ``hip.PatchView`` -> (n, D) embeddings of grid patches
        ``index`` (int32, device) or ``first .. first + n - 1`` (default: every patch): the bits of ``encode`` on the same
        patches of ``hip.patchify(images, ...)`` - the stems read the images, no patch tensor exists.  uint8 images with
        their ``table`` (C, 256): the bits of the float32 images ``table[c][images]``, which do not exist either."""
        return self.encode_source(PatchSource(images=images, view=view, table=table), index=index, first=first, n=n, parts=parts)

    def encode_plain(self, x, out=None, table=None):
        """The image trunk on every patch of ``x`` (no dedup); uint8 ``x`` with its ``table`` (C, 256)."""
        return self.encode_source(PatchSource(x, table), out=out)

    def view_supported(self, view):
        """Can ``encode_view`` read the patches of this ``hip.PatchView``?  The exact fp32 trunks whose stem stages its
        patch into LDS (1x32x32 fused, 1x50x50, 3x100x100) on a view of their patch shape (``ipsx_trunk_view_supported``)."""
        if not self.is_image:
            return False
        self._refresh()
        return bool(lib().ipsx_trunk_view_supported(C.byref(self._describe(view.patch_size)), C.byref(view.struct)))

    def ragged_view_supported(self, rview):
        """Can ``encode_source`` read the patches of this ``hip.RaggedView`` (images of different sizes)?  What
        ``view_supported`` asks, of the view's patch shape (``ipsx_trunk_ragged_view_supported``)."""
        if not self.is_image:
            return False
        self._refresh()
        return bool(lib().ipsx_trunk_ragged_view_supported(C.byref(self._describe(rview.patch_size)), C.byref(rview.struct)))

    def view_kernel_name(self, view, u8=False):
        """The kernel that reads the images for this view (None: not supported); ``u8``: uint8 images."""
        if not self.view_supported(view):
            return None
        name = lib().ipsx_trunk_kernel(C.byref(self.trunk)).decode()
        kind = "_view_u8_kernel" if u8 else "_view_kernel"
        return "fused_trunk" + kind if name.startswith("fused") else name.split(" ")[0].replace("_kernel", kind)

    def row_stats(self, x, out=None, index=None):
        """(mean, rstd) of every feature row of ``x`` (P, F) -> (P, 2): the LayerNorm moments the projector's GEMM applies
        to its operand; for callers that run this HBM-bound pass ahead of / beside the GEMM (``encode(x, stats=...)``).
        ``index`` (n int32): of the rows ``x[index]`` -> (n, 2), read through the index - nothing is gathered."""
        self._refresh()
        x = self._features(x)
        n = x.shape[0]
        if index is not None:
            n = self._index(index, x).numel()
        if out is None:
            out = torch.empty((n, 2), dtype=torch.float32, device=x.device)
        return self._stats(x, out, index)

    def image_stream_supported(self, x_shape, D, R):
        """Can ``image_stream`` encode patches of this shape (the fused fp32 1x32x32 trunk, 128 features, R <= 32)?"""
        if not self.is_image or not self.fused(x_shape) or precision() != "fp32":
            return False
        return bool(lib().ipsx_trunk_stream_supported(C.byref(self.trunk), int(D), int(R)))

    def image_stream(self, x, pos, vq, R, emb, logits, ctl, ready, workgroups=0, quad_pulls=-1, index=None):
        """Trunk + logits of ONE image's patches ``x`` (P, 1, 32, 32) as one persistent launch that advances ``ready`` (the
        progress word of ``scan_persistent``) as patches complete: ``emb`` (P, 128) and ``logits`` (P, R) are the outputs,
        ``pos`` (P, 128) or None is added to the embeddings for the logits, ``ctl`` =
        ``torch.zeros(image_stream_ctl_words(P), int32)`` zeroed before every call, ``vq`` the folded query.
        ``index`` (n int32 patch numbers inside ``x``, every one in [0, P)): patch j of the stream is ``x[index[j]]`` -
        the bits of ``image_stream(x[index], ...)``, outputs and ``pos`` in j (``ipsx_trunk_stream_indexed``)."""
        self._refresh()
        x = _patches(x)
        self._describe(x.shape)
        if pos is not None and (pos.stride(-1) != 1 or pos.stride(-2) != pos.shape[-1]):
            pos = pos.contiguous()
        if index is not None:
            if index.dtype != torch.int32 or index.dim() != 1 or not index.is_contiguous() or index.device != x.device:
                raise ValueError("index must be a contiguous 1-d int32 tensor on the patches' device")
            _ck(lib().ipsx_trunk_stream_indexed(C.byref(self.trunk), _p(x), _p(index), x.shape[0], index.numel(), _p(emb), _p(pos),
                                                _p(vq), int(R), _p(logits), _p(ctl), _p(ready), int(workgroups), int(quad_pulls),
                                                _stream()), "ipsx_trunk_stream_indexed")
            return emb
        _ck(lib().ipsx_trunk_stream(C.byref(self.trunk), _p(x), x.shape[0], _p(emb), _p(pos), _p(vq), int(R), _p(logits),
                                    _p(ctl), _p(ready), int(workgroups), int(quad_pulls), _stream()), "ipsx_trunk_stream")
        return emb

    @staticmethod
    def image_stream_ctl_words(n):
        return int(lib().ipsx_trunk_stream_ctl_words(int(n)))

    def stream_supported(self, n, R):
        """Can ``stream`` run this projector on ``n`` rows with ``R`` logits per row?"""
        if self.is_image:
            return False
        self._refresh()
        return not self.bf16 and bool(lib().ipsx_projector_stream_supported(C.byref(self.lin), int(n), int(R)))

    def stream(self, x, vq, R, emb, logits, ctl, ready, workgroups=0, short_first=-1, slide_rows=None, index=None):
        """Projector + logits of the feature rows ``x`` (P, F) - one slide, or several one after the other, ``slide_rows``
        each - as one persistent launch that advances ``ready`` (the progress word(s) of ``scan_persistent``, one per
        slide) as rows complete: ``emb`` (P, 512) and ``logits`` (P, R) are the outputs, ``ctl`` =
        ``torch.zeros(stream_ctl_words(P), int32)`` zeroed before every call, ``vq`` the folded query.  The fp32
        projector only: float32 rows, and not under the bf16 projector (IPSX_PRECISION=bf16 runs ``encode`` launch by
        launch) - both refused before the launch."""
        self._refresh()
        if self.bf16:
            raise TypeError("the projector stream runs the fp32 projector; under IPSX_PRECISION=bf16 the projector is "
                            "encode()'s bf16 kernel")
        if x.dtype in (torch.float16, torch.bfloat16):
            raise TypeError("{} features need IPSX_PRECISION=bf16 (the projector stream reads float32)".format(x.dtype))
        x = _f32(x)
        if index is not None:
            # row j of the stream is x[index[j]] (``emb``, ``logits``, ``ready``: in j) - the bits of stream(x[index], ...)
            n = self._index(index, x).numel()
            x = x if x.is_contiguous() else x.contiguous()
            _ck(lib().ipsx_projector_stream_indexed(C.byref(self.lin), _p(x), _p(index), x.shape[0], n, int(slide_rows or n),
                                                    C.c_float(self.ln_eps), _p(emb), _p(vq), int(R), _p(logits), _p(ctl), _p(ready),
                                                    int(workgroups), int(short_first), _stream()), "ipsx_projector_stream_indexed")
            return emb
        _ck(lib().ipsx_projector_stream(C.byref(self.lin), _p(x), x.shape[0], int(slide_rows or x.shape[0]),
                                        C.c_float(self.ln_eps), _p(emb), _p(vq), int(R),
                                        _p(logits), _p(ctl), _p(ready), int(workgroups), int(short_first), _stream()),
            "ipsx_projector_stream")
        return emb

    @staticmethod
    def stream_ctl_words(n):
        return int(lib().ipsx_projector_stream_ctl_words(int(n)))

    @staticmethod
    def stream_ctl_zero_words(n):
        """... of which only the first this many have to be zero when a call starts."""
        return int(lib().ipsx_projector_stream_ctl_zero_words(int(n)))

    def encode(self, x, nonblank=None, stats=None, out=None, publish=None, index=None, table=None):
        """(P, C, h, w) patches or (P, F) feature rows on the GPU  ->  (P, D) float32.  float32 input; patches also
        float16 / bfloat16 under IPSX_PRECISION=bf16 or fp32x3 (``_patches``), feature rows also float16 / bfloat16
        under IPSX_PRECISION=bf16, whose projector widens them in its operand load (``_features``).  uint8 patches with
        their ``table`` ((C, 256) float32, ``ips_amd.quant``): the embeddings of ``table[c][x]``, bit for bit, on the exact
        path only - no reduced precision, no blank-patch dedup (both refused before the first launch).

        ``nonblank`` (P int32, 1 = the patch has a non-zero element; e.g. from ``patchify_sparse``) switches on
        the exact blank-patch dedup without the pass that looks for blank patches.  ``publish`` = (ready, value), with
        ``stats``: the GEMM launch also does ``publish_rows(ready, value)`` for what was enqueued before it.

        ``index`` (n int32, feature rows only): the embeddings of ``x[index]`` -> (n, D), read through the index by the
        row-indexed kernels (``stats``, ``out`` and the result are in the index's order) - the bits of ``encode(x[index])``
        without the gathered copy."""
        self._refresh()
        if table is not None and not self.is_image:
            raise TypeError("a patch table goes with uint8 patches of an image encoder")
        if self.is_image and x.dtype == torch.uint8 and nonblank is not None:
            raise TypeError("blank-patch dedup reads float32 patches")
        src = PatchSource(x, table) if self.is_image else None
        x = src.patches if self.is_image else self._features(x)
        n = x.shape[0]
        if index is not None:
            if self.is_image:
                raise TypeError("a row index goes with feature rows (patches: encode_indexed)")
            n = self._index(index, x).numel()
        if self.is_image and x.dtype != torch.float32 and (dedup_blank() or nonblank is not None):
            raise TypeError("blank-patch dedup reads float32 patches")
        if out is None:
            out = torch.empty((n, self.d_out), dtype=torch.float32, device=x.device)
        elif tuple(out.shape) != (n, self.d_out) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError("out must be a contiguous (P, D) float32 tensor")
        if n == 0:
            return out
        if self.is_image:
            self._describe(x.shape)                        # (the dedup entries read float32 patches)
            if x.shape[1] != self.trunk.c_in:
                raise ValueError("patches have {} channels, encoder expects {}".format(x.shape[1], self.trunk.c_in))
            if (dedup_blank() or nonblank is not None) and \
                    lib().ipsx_trunk_kernel(C.byref(self.trunk)).startswith(b"fused_trunk"):      # any precision
                nb = lib().ipsx_trunk_dedup_workspace_bytes(C.byref(self.trunk), n)
                ws = self._workspace(nb, x.device)
                self.n_encoded = torch.zeros((), dtype=torch.int32, device=x.device)
                if nonblank is not None:
                    if nonblank.dtype != torch.int32 or nonblank.numel() != n or not nonblank.is_contiguous():
                        raise ValueError("nonblank must be a contiguous int32 tensor with one flag per patch")
                    _ck(lib().ipsx_trunk_encode_dedup_flagged(C.byref(self.trunk), _p(x), n, _p(nonblank), _p(out), _p(ws),
                                                              nb, _p(self.n_encoded), _stream()),
                        "ipsx_trunk_encode_dedup_flagged")
                else:
                    _ck(lib().ipsx_trunk_encode_dedup(C.byref(self.trunk), _p(x), n, _p(out), _p(ws), nb,
                                                      _p(self.n_encoded), _stream()), "ipsx_trunk_encode_dedup")
                return out
            if (dedup_blank() or nonblank is not None) and n > 1:
                # layer-by-layer trunks (other patch sizes / depths): the same exact dedup with the index handling in
                # torch - the layered launches are sized on the host, so the number of distinct patches is read back
                # (one synchronisation per call; the fused trunk above needs none)
                flags = nonblank.bool() if nonblank is not None else (x.flatten(1) != 0).any(1)
                keep = torch.nonzero(flags).flatten()
                blank = torch.nonzero(~flags).flatten()
                if blank.numel() > 1:
                    sel = torch.cat((keep, blank[:1]))
                    uniq = self.encode_plain(x[sel])
                    out[keep] = uniq[:keep.numel()]
                    out[blank] = uniq[keep.numel():keep.numel() + 1]
                    self.n_encoded = torch.tensor(sel.numel(), dtype=torch.int32, device=x.device)
                    return out
            return self.encode_source(src, out=out)
        elif self.bf16:
            if stats is None:
                ws = self._workspace(lib().ipsx_projector_workspace_bytes(n), x.device)
                stats = self._stats(x, ws[:8 * n].view(torch.float32).view(n, 2), index)
            elif stats.shape != (n, 2) or stats.dtype != torch.float32 or not stats.is_contiguous():
                raise ValueError("stats must be a contiguous (P, 2) float32 tensor")
            ready, value = publish if publish is not None else (None, 0)
            if index is not None:
                _ck(lib().ipsx_projector_apply_bf16_indexed(C.byref(self.lin), _p(x), _PATCH_DTYPES[x.dtype], _p(index), x.shape[0], n,
                                                            _p(stats), _p(out), _p(ready), int(value), _stream()),
                    "ipsx_projector_apply_bf16_indexed")
                return out
            _ck(lib().ipsx_projector_apply_bf16(C.byref(self.lin), _p(x), _PATCH_DTYPES[x.dtype], n, _p(stats), _p(out), _p(ready),
                                                int(value), _stream()), "ipsx_projector_apply_bf16")
        elif index is not None:
            if stats is None:
                ws = self._workspace(lib().ipsx_projector_workspace_bytes(n), x.device)
                stats = self._stats(x, ws[:8 * n].view(torch.float32).view(n, 2), index)
            elif stats.shape != (n, 2) or stats.dtype != torch.float32 or not stats.is_contiguous():
                raise ValueError("stats must be a contiguous (P, 2) float32 tensor")
            ready, value = publish if publish is not None else (None, 0)
            _ck(lib().ipsx_projector_apply_indexed(C.byref(self.lin), _p(x), _p(index), x.shape[0], n, _p(stats), _p(out), _p(ready),
                                                   int(value), _stream()), "ipsx_projector_apply_indexed")
        elif stats is not None:
            if stats.shape != (n, 2) or stats.dtype != torch.float32 or not stats.is_contiguous():
                raise ValueError("stats must be a contiguous (P, 2) float32 tensor")
            if publish is not None:
                _ck(lib().ipsx_projector_apply_publish(C.byref(self.lin), _p(x), n, _p(stats), _p(out), _p(publish[0]),
                                                       int(publish[1]), _stream()), "ipsx_projector_apply_publish")
            else:
                _ck(lib().ipsx_projector_apply(C.byref(self.lin), _p(x), n, _p(stats), _p(out), _stream()), "ipsx_projector_apply")
        else:
            nb = lib().ipsx_projector_workspace_bytes(n)
            ws = self._workspace(nb, x.device)
            _ck(lib().ipsx_projector(C.byref(self.lin), _p(x), n, C.c_float(self.ln_eps), _p(out),
                                     _p(ws), nb, _stream()), "ipsx_projector")
        return out


def encoder_kernel_name(plan):
    """Which kernel family the plan's encode() launches (for bench.py's roofline record)."""
    if plan is None or plan._sig is None:
        return None
    if not plan.is_image:
        if plan.bf16:
            return "row_moments_typed_kernel + projector_bf16_kernel (bf16 projector)"
        return "row_stats_kernel + conv_nhwc_kernel<NORM> (projector)"
    return lib().ipsx_trunk_kernel(C.byref(plan.trunk)).decode()
