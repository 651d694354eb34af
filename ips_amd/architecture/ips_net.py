"""IPSNet: patch encoder + Iterative Patch Selection + aggregation + task heads.

Drop-in mirror of /root/reference/architecture/ips_net.py:11-283: same class
name, ``IPSNet(device, conf)`` constructor, ``ips(patches) -> (mem_patch,
mem_pos)`` and ``forward(mem_patch, mem_pos=None) -> {task: probs}`` signatures,
same sub-module / parameter names (``encoder.N...``, ``transf...``,
``output_layers.<task>.0``), so the reference's ``main.py`` and
``training/iterative.py`` drive it unchanged and state-dicts interchange.

What is different is how ``ips()`` executes on a ROCm device.  The reference
runs a Python loop of ~75 stock kernels per chunk.  In eval / no-grad mode the
encoder is a pure per-patch function (BatchNorm uses running statistics,
reference :191-193) and a patch's attention logits do not depend on which other
patches are in the candidate set (only the softmax denominator does), so the
HIP path is three launches' worth of work:

  1. ``encode``   every patch once (fused ResNet trunk / projector kernels),
  2. ``logits``   K-projection and q.k per patch, once,
  3. ``scan``     one persistent workgroup per image replays the reference's
                  chunk loop on the cached logits: softmax over memory+chunk,
                  mean over heads and tokens, top-M, repeat,

followed by row gathers of the M winners.  Results are those of the reference
loop: same candidate order (memory first, reference :231-232), same arithmetic
order per patch.  ``last_mem_idx`` exposes the selected indices (the reference
only returns the gathered patches).
"""

import contextlib
import os

import torch
from torch import nn

from .. import hip
from ..ragged import Ragged
from ..ragged_image import RaggedImages
from ..shuffle import draw_shuffle, shuffle_batch, shuffle_instance
from .resnet import load_torchvision_checkpoint, resnet18_trunk, resnet50_trunk
from .transformer import Transformer, pos_enc_1d


class IPSNet(nn.Module):
    """Patch encoder, IPS, cross-attention aggregator and classification heads."""

    # ---------------------------------------------------------------- construction
    def get_conv_patch_enc(self, enc_type, pretrained, n_chan_in, n_res_blocks):
        """ResNet stem + 2 or 4 residual stages + global average pool (reference :17-52)."""
        if enc_type == 'resnet18':
            trunk = resnet18_trunk()
        elif enc_type == 'resnet50':
            trunk = resnet50_trunk()
        else:
            raise ValueError("unknown enc_type {!r}".format(enc_type))
        if pretrained:
            # the reference lets torchvision download IMAGENET1K_V1 (:19-27); this framework targets machines
            # without network access, so the same file is read from a local path instead
            path = os.environ.get("IPSX_PRETRAINED_" + enc_type.upper()) or os.environ.get("IPSX_PRETRAINED")
            if not path:
                raise RuntimeError(
                    "pretrained=True: point IPSX_PRETRAINED_{} (or IPSX_PRETRAINED) at a local torchvision {} "
                    "state-dict file (IMAGENET1K_V1 .pth); this image cannot download it".format(enc_type.upper(), enc_type))
            load_torchvision_checkpoint(trunk, path)
        if n_chan_in == 1:
            # the reference swaps the 3-channel stem for a fresh 1-channel one (:29-31)
            trunk.conv1 = nn.Conv2d(n_chan_in, 64, kernel_size=7, stride=2, padding=3, bias=False)
        stages = [trunk.conv1, trunk.bn1, trunk.relu, trunk.maxpool, trunk.layer1, trunk.layer2]
        if n_res_blocks == 4:
            stages += [trunk.layer3, trunk.layer4]
        stages.append(trunk.avgpool)
        return nn.Sequential(*stages)

    def get_projector(self, n_chan_in, D):
        """LN(no affine) -> Linear -> BatchNorm1d -> ReLU for pre-extracted features (:54-60)."""
        return nn.Sequential(
            nn.LayerNorm(n_chan_in, eps=1e-05, elementwise_affine=False),
            nn.Linear(n_chan_in, D),
            nn.BatchNorm1d(D),
            nn.ReLU(),
        )

    def get_output_layers(self, tasks):
        """One ``Linear(D, n_class) -> softmax|sigmoid`` head per task (:62-83)."""
        heads = nn.ModuleDict()
        for task in tasks.values():
            act = {'softmax': lambda: nn.Softmax(dim=-1), 'sigmoid': nn.Sigmoid}[task['act_fn']]()
            heads[task['name']] = nn.Sequential(nn.Linear(self.D, self.n_class), act)
        return heads

    def __init__(self, device, conf):
        super().__init__()
        hip.install_optimizer_hook()        # every optimizer step invalidates the packed weights (see hip.py)
        self.device = device
        self.n_class = conf.n_class
        self.M, self.I, self.D = conf.M, conf.I, conf.D
        self.use_pos = conf.use_pos
        self.tasks = conf.tasks
        self.shuffle = conf.shuffle
        self.shuffle_style = conf.shuffle_style
        self.is_image = conf.is_image

        if self.is_image:
            self.encoder = self.get_conv_patch_enc(conf.enc_type, conf.pretrained,
                                                   conf.n_chan_in, conf.n_res_blocks)
        else:
            self.encoder = self.get_projector(conf.n_chan_in, self.D)

        self.transf = Transformer(conf.n_token, conf.H, conf.D, conf.D_k, conf.D_v,
                                  conf.D_inner, conf.attn_dropout, conf.dropout)

        # plain tensor attribute, not a buffer - exactly as the reference (:110-113)
        self.pos_enc = pos_enc_1d(conf.D, conf.N).unsqueeze(0).to(device) if conf.use_pos else None

        self.output_layers = self.get_output_layers(conf.tasks)

        # additions that do not change the drop-in surface
        self._reset_last()            # what the last selection left behind: nothing yet
        self._plan = None             # packed-weight cache of the HIP encoder
        self._filled_rows = None      # forward(mask_encoder=True): (key, (int64 rows, int32 rows)) of the last counts (_filled_index)
        self._selection = None        # the HIP selection pipelines (ips_amd/selection.py), built on first use
        self._device_patches = None   # lazy loading: the device copy of the host tensor, when it is kept
        # uint8 patch storage (ips_amd/quant.py): the (n_chan, 256) float32 table of set_patch_table - a plain tensor
        # attribute like pos_enc, not a buffer (state dicts stay those of the reference)
        self.patch_table = None
        if self.is_image and hip.on_device(device):
            # the training step's convolutions run channels-last (training/fused_encoder.py): weights stored that way
            # from the start (before any optimizer state exists) are not re-laid-out in every step.  Shapes, names and
            # values are untouched - state dicts interchange with the reference as before.
            from ..training import fused_encoder
            if fused_encoder.enabled() and fused_encoder.supported(self.encoder):
                self.encoder.to(memory_format=torch.channels_last)

    # ---------------------------------------------------------------- uint8 patch storage
    def set_patch_table(self, table):
        """Let ``ips()`` take uint8 patches: ``table`` ((n_chan, 256) float32, finite; ``ips_amd.quant.patch_table`` builds
        the datasets' own) gives the float32 value of every byte per channel.  The encoders' stems look the pixels up as
        they stage a patch, so the selection is that of the expanded float32 tensor ``table[c][patches]`` bit for bit, and
        ``ips()`` returns ``mem_patch`` as float32 (the selected bytes dequantised) - ``forward()`` and the training step
        see what they always saw.  ``None`` removes the table.  Kept on ``self.device``; not part of the state dict."""
        if table is None:
            self.patch_table = None
            return self
        if not self.is_image:
            raise TypeError("a patch table goes with an image encoder (feature rows are stored as float16 / bfloat16)")
        from ..quant import check_table
        n_chan = next(self.encoder.children()).in_channels
        check_table(table, n_chan)
        if not bool(torch.isfinite(table).all()):
            raise ValueError("the patch table must be finite")
        self.patch_table = table.detach().to(self.device).contiguous()
        return self

    def _table_for(self, x):
        """The table that goes with patches ``x`` - None unless they are uint8; uint8 without a table is an error."""
        if x.dtype != torch.uint8:
            return None
        if self.patch_table is None:
            raise TypeError("uint8 patches need a dequantisation table: call IPSNet.set_patch_table(ips_amd.quant.patch_table(...)) first")
        return self.patch_table

    def _dequant(self, q):
        """float32 ``patch_table[c][q]`` of uint8 patches on ``self.device`` (the HIP kernel there, else by indexing)."""
        table = self._table_for(q)
        if hip.on_device(q):
            return hip.dequant_patches(q, table)
        from ..quant import dequant
        return dequant(q, table)

    def _check_u8(self, patches):
        """uint8 patches: everything that refuses them does so here, before the first launch of the call."""
        if not self.is_image or patches.dim() != 5:
            raise TypeError("uint8 input goes with (B, N, C, h, w) image patches")
        table = self._table_for(patches)
        if table.shape[0] != patches.shape[2]:
            raise ValueError("the patch table has {} rows, the patches {} channels".format(table.shape[0], patches.shape[2]))
        if hip.on_device(self.device):
            if hip.precision() != "fp32":
                raise TypeError("uint8 patches go with the exact trunk (IPSX_PRECISION=fp32), not {}".format(hip.precision()))
            if hip.dedup_blank():
                raise TypeError("blank-patch dedup reads float32 patches (IPSX_DEDUP_BLANK=1 with uint8 patches)")

    # ---------------------------------------------------------------- small pieces
    def do_shuffle(self, patches, pos_enc):
        """Permute the patch axis (and pos_enc identically) to randomise ties (:118-134)."""
        if self.shuffle_style == 'batch':
            patches, perm = shuffle_batch(patches)
            if torch.is_tensor(pos_enc):
                pos_enc, _ = shuffle_batch(pos_enc, perm)
        elif self.shuffle_style == 'instance':
            patches, perm = shuffle_instance(patches, 1)
            if torch.is_tensor(pos_enc):
                pos_enc, _ = shuffle_instance(pos_enc, 1, perm)
        return patches, pos_enc

    def _shuffle_overridden(self):
        """Has ``do_shuffle`` been replaced on this instance or in a subclass?  Then it is called as ever."""
        return 'do_shuffle' in self.__dict__ or type(self).do_shuffle is not IPSNet.do_shuffle

    def _shuffle(self, patches, pos_enc):
        """``do_shuffle`` with the permutation kept (``last_shuffle``) and - where the selection can read the patches
        through an index (device-resident, contiguous, a schedule that supports it; ``IPSX_SHUFFLE=copy`` switches it off) -
        WITHOUT the permuted copy of the patch tensor.  The permutation is drawn by the calls ``do_shuffle`` makes, so the
        RNG streams and the results are those of the copy.  ``pos_enc`` (a few hundred floats per patch) is shuffled by
        copy either way.  ``patches`` may be a ``hip.PatchSource`` (``ips_image``): there is nothing to copy, so it always
        selects through the index, and ``last_shuffle`` keeps what ``ips()`` keeps for the patch tensor - the device copy
        where it would have selected through the index itself, else the permutation as drawn.  An overridden
        ``do_shuffle`` is called as ever.  -> (patches, pos_enc, order): ``order`` is the (B or 1, N) index on the device
        when ``patches`` came back unshuffled, else None."""
        if self._shuffle_overridden():
            return (*self.do_shuffle(patches, pos_enc), None)
        perm = draw_shuffle(patches, self.shuffle_style)
        if perm is None:                   # an unknown style: do_shuffle leaves everything as it is
            return patches, pos_enc, None
        batch = self.shuffle_style == 'batch'
        if torch.is_tensor(pos_enc):
            pos_enc = shuffle_batch(pos_enc, perm)[0] if batch else shuffle_instance(pos_enc, 1, perm)[0]
        source = not torch.is_tensor(patches)
        by_index = (os.environ.get("IPSX_SHUFFLE", "index") != "copy"
                    and (source or (hip.on_device(self.device) and patches.is_cuda and patches.is_contiguous()))
                    and self.selection.index_supported(patches))
        drawn = perm.unsqueeze(0) if batch else perm
        if by_index or source:
            order = drawn.to(patches.device).contiguous()
            self.last_shuffle = order if by_index else drawn
            return patches, pos_enc, order
        self.last_shuffle = drawn
        patches = shuffle_batch(patches, perm)[0] if batch else shuffle_instance(patches, 1, perm)[0]
        return patches, pos_enc, None

    def score_and_select(self, emb, emb_pos, M, idx):
        """Score ``L`` candidates, keep the top ``M`` (:136-155).

        Scores come from ``emb_pos`` when given, the gathered memory from ``emb``.
        """
        scored = emb_pos if torch.is_tensor(emb_pos) else emb
        if hip.on_device(scored):
            top = hip.topm(self.transf.get_scores(scored), M)
        else:
            top = torch.topk(self.transf.get_scores(scored), M, dim=-1)[1]
        mem_emb = torch.gather(emb, 1, top.unsqueeze(-1).expand(-1, -1, emb.shape[2]))
        return mem_emb, torch.gather(idx, 1, top)

    def get_preds(self, embeddings):
        """Task ``t`` reads aggregated token ``t_id`` (:157-166)."""
        fused = hip.on_device(embeddings) and not (
            torch.is_grad_enabled() and (embeddings.requires_grad or
                                         any(p.requires_grad for p in self.output_layers.parameters())))
        preds = {}
        for task in self.tasks.values():
            layer = self.output_layers[task['name']]
            if fused:   # Linear + softmax|sigmoid in one kernel
                preds[task['name']] = hip.head(embeddings, task['id'], layer[0], task['act_fn'])
            else:
                preds[task['name']] = layer(embeddings[:, task['id']])
        return preds

    def _fused_projector(self, x, n):
        """Does the with-grad pass over ``n`` rows of the features ``x`` run on the fused projector node
        (training/fused_projector.py)?  ROCm device, a feature net's encoder in training mode, grad enabled, a projector the
        kernels take, 2-d features that need no gradient, more than one row."""
        if not (hip.on_device(x) and self.encoder.training and not self.is_image and torch.is_grad_enabled()):
            return False
        from ..training import fused_projector
        if getattr(self, "_fused_train_ok", None) is None:
            self._fused_train_ok = fused_projector.supported(self.encoder)
        return self._fused_train_ok and fused_projector.enabled() and x.dim() == 2 and n > 1 and not x.requires_grad

    def _embed(self, x, rows=None):
        """(P, C, h, w) | (P, F)  ->  (P, D) with the encoder's CURRENT mode.  ``rows`` (the pair of ``_filled_index``: the same
        row numbers into ``x`` as int64 and as int32; the masked encoder pass of ``forward(mask_encoder=True)``):
        -> (n_fill, D), the encoder on ``x[rows]`` alone - through the fused projector's row index where that node runs,
        everywhere else on the gathered copy."""
        if rows is not None:
            rows64, rows32 = rows
            if self._fused_projector(x, rows32.numel()):
                from ..training import fused_projector
                if fused_projector.rows_supported(x, rows32):
                    return fused_projector.encode(self.encoder, x, rows=rows32)
            x = x.index_select(0, rows64)
        if hip.on_device(x) and not self.encoder.training and not (
                torch.is_grad_enabled() and any(p.requires_grad for p in self.encoder.parameters())):
            return self.plan.encode(x, table=self._table_for(x))
        if x.dtype == torch.uint8:
            # the stock modules (CPU / ATen path, or an encoder in training mode) compute on the dequantised pixels
            x = self._dequant(x)
        if hip.on_device(x) and self.encoder.training and self.is_image and torch.is_grad_enabled():
            # training step (reference training/iterative.py:158-163): same modules, BatchNorm + add + ReLU fused
            from ..training import fused_encoder
            if getattr(self, "_fused_train_ok", None) is None:        # (the module tree does not change after construction)
                self._fused_train_ok = fused_encoder.supported(self.encoder)
            if self._fused_train_ok and fused_encoder.enabled():
                return fused_encoder.encode(self.encoder, x)
        if self._fused_projector(x, x.shape[0]):
            # the same step of a feature net: LayerNorm + Linear + BatchNorm1d + ReLU as one node, half-stored rows read typed
            from ..training import fused_projector
            return fused_projector.encode(self.encoder, x)
        if not self.is_image and x.dtype in (torch.float16, torch.bfloat16):
            x = x.float()      # half-stored features (IPSX_PRECISION=bf16): the stock modules compute on the exact widening
        return self.encoder(x).flatten(1)

    # ---------------------------------------------------------------- IPS
    @torch.no_grad()
    def ips(self, patches):
        """Iterative Patch Selection (reference :169-262).

        ``patches``: (B, N, C, h, w) images or (B, N, F) features, on the device
        (eager loading) or on the host (lazy loading).  Returns the M selected
        patches ``(B, M, ...)`` and their positional encodings ``(B, M, D)`` (or
        ``None``), both on ``self.device``, ordered by score of the last round.

        uint8 image patches (after ``set_patch_table``): the same selection on a quarter of the bytes; ``mem_patch``
        comes back float32 - the selected bytes dequantised, bit for bit what the call returns for the expanded tensor.

        A ``ips_amd.ragged.Ragged`` (slides of different lengths, e.g. from a loader with ``collate_ragged``) goes to
        ``ips_ragged``, with its ``pad`` flag.
        """
        if isinstance(patches, Ragged):
            return self.ips_ragged(patches, pad=patches.pad)
        B, N = patches.shape[:2]
        u8 = patches.dtype == torch.uint8
        if u8:
            self._check_u8(patches)
        if self.M >= N:  # nothing to select (:185-188)
            self._reset_last()
            mem_patch = patches.to(self.device)
            return (self._dequant(mem_patch) if u8 else mem_patch), (self.pos_enc.expand(B, -1, -1) if self.use_pos else None)
        return self._call(patches)

    @torch.no_grad()
    def ips_ragged(self, slides, pad=False):
        """``ips()`` on slides of DIFFERENT lengths in one call: ``slides`` an ``ips_amd.ragged.Ragged`` or a
        list of (N_b, F) | (N_b, C, h, w) tensors, on the device or on the host (copied whole)
        -> (mem_patch (B, M, ...), mem_pos (B, M, D) | None).  Slide by slide and bit for bit what
        ``for b in range(B): out[b] = net.ips(slides[b][None])`` returns and leaves behind - ``last_mem_idx`` (B, M), local
        to each slide, ``last_mem_emb`` (B, M, D), ``last_shuffle`` the list of the B per-slide permutations (drawn slide by
        slide, in slide order: torch's RNG streams end where that loop leaves them) -, positions restarting at 0 in every
        slide.  On a ROCm device: one encoder pass over all rows, one packed logits table, ONE loop launch
        (``ipsx_scan_ragged``) and ONE finish launch (``ipsx_ragged_finish``; ``gather_rows`` launches where the rows are not
        whole 16-byte units), ``last_mem_emb`` gathered on first read; on a CPU device the loop itself.  With and without
        ``pad`` the route is the same.  Refused before the first launch:
        a slide with N_b <= M (the reference returns N_b patches there: no rectangular result), ``use_pos`` with
        N_b > conf.N (with 'instance' shuffling: N_b != conf.N, where ``ips()`` itself raises), an empty batch,
        ``IPSX_DEDUP_BLANK=1``.

        uint8 (N_b, C, h, w) patch slides of an image net (after ``set_patch_table``): the same call on a quarter of the
        bytes - everything returned and left behind is, bit for bit, that of the float32 slides ``patch_table[c][byte]``,
        ``mem_patch`` float32 (the finish runs on the byte rows, then ``hip.dequant_patches``).  Refused as ``ips()`` refuses
        them: no table, a table whose rows differ from the channel count, ``IPSX_PRECISION`` other than ``fp32`` on a ROCm
        device, a feature net (``TypeError``).

        ``pad=True`` takes slides with N_b <= M as well (an empty slide is refused) and returns the batch ``fill_batch`` of
        training/iterative.py builds from the solo calls: a short slide's rows in the order given in slots [0, N_b) - never
        shuffled, no random number drawn - and +0.0 behind them; ``mem_pos`` ``pos_enc[0, :N_b]`` then zeros;
        ``last_mem_idx`` 0 .. N_b-1 then -1; ``last_mem_emb`` the eval-mode embeddings of its rows, the padding slots the
        embedding of ONE all-zero row (what ``forward()`` in eval mode computes from the padding; uint8 slides: float32
        ``+0.0`` and the all-zero FLOAT patch's embedding, not ``patch_table[c][0]``); its ``last_shuffle`` entry
        None (``last_shuffle`` None when no slide is long).  ``last_mem_count`` holds the B host ints min(N_b, M); nothing
        masks the padding - the reference attends to it as well.  Long slides are as without ``pad``; the finish launch
        writes the padding too, and a batch of short slides only encodes nothing until ``last_mem_emb`` is read."""
        from ..ragged import ips_ragged
        return ips_ragged(self, slides, pad)

    def _reset_last(self):
        """Forget the last selection.  Every entry point (``ips``, ``ips_image``, ``ips_ragged``, a stream's ``finish``, the
        calls of ips_amd/dist.py) begins here, before it launches or draws anything, and then sets what it leaves itself:
        nothing outlives its call.  A call that runs selections of its own inside (the host route of ``ips_ragged``,
        ``dist.ips_tournament``) comes here once more behind them: what they left is theirs."""
        self.last_mem_idx = None      # (B, M) int64 indices chosen by the last selection
        self.last_shuffle = None      # (B, N) | (1, N) int64 permutation of the last shuffled ips() call (see ips), or None
        self._emb_parts = None        # the producers' hand-off (selection.py): eval-mode embeddings of all patches, in parts
        self._mem_emb = None          # (B, M, D): ``last_mem_emb``, once it is made
        self._emb_make = None         # a call that gathers ``last_mem_emb`` another way: () -> (B, M, D) | None, run on first read
        self._mem_count = None        # ``last_mem_count``

    @contextlib.contextmanager
    def _scoring(self):
        """The frame of every selection (``ips``, ``ips_image``, streams, sharded calls): IPS always scores with running BN
        statistics and no dropout, so a net in train mode has its encoder and transformer in eval mode inside the block
        and both back in train mode behind it, also after an exception.  A net in eval mode is left alone."""
        was_training = self.training
        if was_training:
            self.encoder.eval()
            self.transf.eval()
        try:
            yield
        finally:
            if was_training:
                self.encoder.train()
                self.transf.train()

    def _call(self, patches):
        """One selection with N > M, the body of ``ips()`` ((B, N, ...) patches) and ``ips_image()`` (a ``hip.PatchSource``
        with a view: whole images on the device) -> (mem_patch, mem_pos).  The two differ in the last gather alone."""
        device, pos_enc = self.device, self.pos_enc
        viewed = not torch.is_tensor(patches)
        u8 = patches.dtype == torch.uint8
        B = patches.shape[0]
        self._reset_last()
        with self._scoring():
            if self.use_pos:
                pos_enc = pos_enc.expand(B, -1, -1)
            order = None
            if self.shuffle:
                # (the encoder is in eval mode by now: the index path's own condition)
                patches, pos_enc, order = self._shuffle(patches, pos_enc)

            if hip.on_device(device):
                with self.plan.hold():            # weights cannot change inside a no-grad call: check them once
                    self.selection.caller_finishes = True       # (this call ends in finish / take_unfinished + after_call below)
                    try:
                        mem_idx = self._select_hip(patches, pos_enc, order)
                    finally:
                        self.selection.caller_finishes = False
            else:
                mem_idx = self._select_aten(patches, pos_enc)

            src = self._device_patches if self._device_patches is not None else patches
            self._device_patches = None
            sel = self._selection
            # (a call on a source leaves nothing pending: finish returns None before it looks at ``src``)
            done = sel.finish(src, pos_enc if self.use_pos else None, order) if sel is not None else None
            if done is not None:       # a resident loop's call ends in ONE launch: gathers, indices, status word (round 5)
                mem_idx, mem_patch, mem_pos = done
            else:
                if sel is not None:
                    mem_idx = sel.take_unfinished(mem_idx)
                # (through a shuffle index the patches are unshuffled: their rows are order[b, mem_idx[b, m]])
                rows = mem_idx if order is None else torch.gather(order.expand(B, -1), 1, mem_idx)
                if viewed:             # straight out of the images, float32 whatever they store
                    mem_patch = hip.gather_patches_view(src.images, src.view, rows, self._table_for(src))
                else:
                    mem_patch = self._take(src, rows).to(device)
                mem_pos = self._take(pos_enc, mem_idx) if self.use_pos else None
                if sel is not None:
                    sel.after_call()
            if u8 and not viewed:      # the M selected patches leave as float32 (forward / fill_batch read float32)
                mem_patch = self._dequant(mem_patch)

        self.last_mem_idx = mem_idx
        return mem_patch, mem_pos

    @staticmethod
    def _unfold_images(images, patch_size, patch_stride):
        """(B, C, H, W) -> (B, N, C, ph, pw): the reference datasets' unfold (mnist_dataset.py:44-51), batched, on any device."""
        (ph, pw), (sh, sw) = patch_size, patch_stride
        if ph > images.shape[2] or pw > images.shape[3] or min(ph, pw, sh, sw) <= 0:
            raise ValueError("patch {}x{} / stride {}x{} does not fit a {}x{} image".format(ph, pw, sh, sw, *images.shape[2:]))
        p = images.unfold(2, ph, sh).unfold(3, pw, sw).permute(0, 2, 3, 1, 4, 5)
        return p.reshape(images.shape[0], -1, images.shape[1], ph, pw)

    def _materialise(self, images, patch_size, patch_stride):
        """The patch tensor of ``images``, where ``ips_image`` cannot read them through a view."""
        if hip.on_device(self.device):
            images = images.to(self.device)
            if images.dtype == torch.float32:
                return hip.patchify(images, patch_size, patch_stride)
        return self._unfold_images(images, patch_size, patch_stride).contiguous()

    @torch.no_grad()
    def ips_image(self, images, patch_size, patch_stride):
        """``ips()`` on a batch of whole images: ``images`` (B, C, H, W) float32 - or uint8 after ``set_patch_table``, the
        bytes a dataset stores: everything below as for the float32 images ``patch_table[c][images]``, which are never made,
        ``mem_patch`` float32 -, on the device or on the host (copied whole, as stored)
        -> (mem_patch (B, M, C, ph, pw), mem_pos).  Everything ``ips(hip.patchify(images, patch_size, patch_stride))``
        returns and leaves behind (``last_mem_idx``, ``last_mem_emb``, ``last_shuffle``), bit for bit - but the stems of
        the exact fp32 trunks read their patches straight from the image grid (``hip.PatchView``): the
        (B, N, C, ph, pw) tensor, a multiple of the images when patches overlap, is never made.  Where the view is not
        supported (other stems and precisions, blank-patch dedup, a CPU device, an encoder in training mode, an overridden
        ``do_shuffle``, other image types, M >= N) the patch tensor is materialised - uint8 images: as uint8 patches - and
        ``ips()`` runs as ever, refusing what it refuses.

        An ``ips_amd.ragged_image.RaggedImages`` (images of different sizes, e.g. from a loader with
        ``collate_ragged_images``) goes to ``ips_image_ragged``, with its ``pad`` flag."""
        if isinstance(images, RaggedImages):
            return self.ips_image_ragged(images, patch_size, patch_stride, pad=images.pad)
        if not self.is_image or images.dim() != 4:
            raise TypeError("ips_image takes (B, C, H, W) images of an image encoder")
        table = self._table_for(images)    # (uint8 without a table: the error uint8 patches raise)
        view = None
        if (hip.on_device(self.device) and images.dtype in (torch.float32, torch.uint8) and not hip.dedup_blank()
                and not (self.encoder.training and not self.training)       # (ips() itself puts a training NET into eval mode)
                and not (self.shuffle and self._shuffle_overridden())):
            view = hip.PatchView(images.shape, patch_size, patch_stride)
            if self.M >= view.per_image or not self.plan.view_supported(view):
                view = None
        if view is None:
            return self.ips(self._materialise(images, patch_size, patch_stride))
        return self._call(hip.PatchSource(images=images.to(self.device), view=view, table=table))

    @torch.no_grad()
    def ips_image_ragged(self, images, patch_size, patch_stride, pad=False):
        """``ips_image()`` on whole images of DIFFERENT sizes in one call: ``images`` an
        ``ips_amd.ragged_image.RaggedImages`` or a list of (C, H_b, W_b) float32 tensors - or uint8 ones after
        ``set_patch_table``, the bytes a dataset stores: everything below as for the float32 images ``patch_table[c][byte]``,
        which are never made, ``mem_patch`` float32 -, on the device or on the host (copied whole, as stored) -> (mem_patch (B, M, C, ph, pw), mem_pos (B, M, D) | None).  Image by image and bit for bit what
        ``for b in range(B): out[b] = net.ips_image(images[b][None], patch_size, patch_stride)`` returns and leaves behind,
        which is what ``net.ips_ragged([patchify(images[b]) for b], pad=pad)`` returns and leaves behind: ``last_mem_idx``
        (B, M) local to each image's grid, ``last_mem_emb``, ``last_shuffle`` the list of per-image permutations (drawn image
        by image: torch's RNG streams end where that loop leaves them), positions restarting at 0 in every image; with
        ``pad=True`` an image with ny_b * nx_b <= M comes back as ``ips_ragged(pad=True)`` returns a short slide, and
        ``last_mem_count`` is set.  On a ROCm device, float32 or uint8 images, an eval-mode encoder, no overridden ``do_shuffle``, at
        least one image longer than M and a trunk whose stem reads a ragged view (``EncoderPlan.ragged_view_supported``: the
        exact fp32 1x32x32, 1x50x50 and 3x100x100 trunks): ONE encoder pass over the grid patches of all images, read where
        they lie - no patch tensor is made -, one packed logits table, ONE loop launch (``ipsx_scan_ragged``) and ONE finish
        launch (``ipsx_ragged_finish_view``; bytes: the ``_u8`` exports, the load width picked per launch from the images'
        byte offsets and widths).  Everywhere else the per-image patch tensors are materialised - uint8 images: as uint8
        patches - and
        ``ips_ragged(list, pad)`` runs unchanged, with its own refusals.  Refused before the first launch and before a random
        number is drawn: everything ``ips_ragged`` refuses with "rows" read as grid patches, images whose channel counts
        differ from each other or from the encoder's, a patch or stride that does not fit an image, uint8 images without a table
        (TypeError), with a table whose rows differ from the channel count or - on a ROCm device - under ``IPSX_PRECISION``
        other than ``fp32``, a feature net."""
        from ..ragged_image import ips_image_ragged
        return ips_image_ragged(self, images, patch_size, patch_stride, pad)

    def ips_stream(self, patch_size=None, patch_stride=None):
        """``ips()`` over patches that arrive in pieces -> ``ips_amd.stream.IPSStream``: ``feed(piece)`` takes
        (B, n, C, h, w) | (B, n, F) pieces of any length, on the device or the host, ``finish()`` returns what
        ``ips(torch.cat(pieces, 1))`` returns with ``shuffle`` off, bit for bit, and sets ``last_mem_idx`` /
        ``last_mem_emb``.  The state is M + I - 1 rows per image whatever N turns out to be.  The stream
        never shuffles (the permutation needs N): feed in random order for randomised ties.

        With ``patch_size`` (ph, pw) and ``patch_stride`` (sh, sw), as ``ips_image`` takes them, the stream is a ROW stream
        (DESIGN 2.5): ``feed_rows(band)`` takes the next pixel rows (B, C, h, W) of whole images - float32, or uint8 after
        ``set_patch_table`` -, bands of any height, and ``finish()`` returns what
        ``ips_image(torch.cat(bands, 2), patch_size, patch_stride)`` returns, bit for bit.  The stream carries the fewer than
        ph rows a patch row straddling two bands needs; where ``ips_image`` reads a patch view no patch tensor is made."""
        from ..stream import IPSStream
        return IPSStream(self, patch_size, patch_stride)

    def ips_ragged_stream(self, pad=False, patch_size=None, patch_stride=None):
        """``ips_ragged()`` over slides whose rows arrive in pieces -> ``ips_amd.ragged_stream.RaggedIPSStream``:
        ``feed(pieces)`` takes a ``Ragged`` or a list of B tensors (n_b, F) | (n_b, C, h, w) - the next rows of each slide,
        n_b >= 0, on the device or the host -, ``feed_all(slides, slab_rows)`` walks a whole batch in slabs, and ``finish()``
        returns and leaves behind what ``ips_ragged([torch.cat(pieces of slide b) for b], pad=pad)`` does with ``shuffle``
        off, bit for bit.  The state is M + I - 1 rows per slide whatever the lengths turn out to be; a host batch goes over
        slab by slab.  The stream never shuffles.

        With ``patch_size`` (ph, pw) and ``patch_stride`` (sh, sw) - both, as ``ips_stream`` takes them - the stream is a
        ragged ROW stream: ``feed_rows(bands)`` takes a list of B entries, the next pixel rows (C, h_b, W_b) of
        whole images of different sizes - float32, or uint8 after ``set_patch_table``; h_b >= 0 or None, on the device or the
        host -, ``feed_rows_all(images, band_rows)`` walks a ``RaggedImages`` or a list of images in bands, and ``finish()``
        returns and leaves behind what ``ips_image_ragged([torch.cat(bands of image b, 1) for b], patch_size, patch_stride,
        pad=pad)`` does with ``shuffle`` off, bit for bit, wherever the bands end.  Each image carries the fewer than ph rows
        a patch row straddling two bands needs; where ``ips_image_ragged`` reads a ragged view no patch tensor is made."""
        from ..ragged_stream import RaggedIPSStream
        return RaggedIPSStream(self, pad, patch_size, patch_stride)

    def _chunks(self, N):
        """[0, M) then ceil((N-M)/I) chunks of I (last one ragged) - reference :206,217-221."""
        yield 0, self.M
        for start in range(self.M, N, self.I):
            yield start, min(start + self.I, N)

    @staticmethod
    def _take(src, idx):
        """``src[b, idx[b, m]]`` on the device ``src`` lives on."""
        if hip.on_device(src):
            return hip.gather_rows(src, idx)
        idx = idx.to(src.device)
        view = idx.view(*idx.shape, *(1,) * (src.dim() - 2)).expand(-1, -1, *src.shape[2:])
        return torch.gather(src.expand(idx.shape[0], *src.shape[1:]), 1, view)

    @property
    def plan(self):
        """The packed-weight plan of the HIP encoder (``hip.EncoderPlan``), built on first use and kept in ``_plan``."""
        if self._plan is None:
            self._plan = hip.EncoderPlan(self.encoder, self.is_image)
        return self._plan

    @property
    def selection(self):
        """The HIP selection pipelines of this net (ips_amd/selection.py), built on first use."""
        if self._selection is None:
            from ..selection import Selection
            self._selection = Selection(self, owned=True)
        return self._selection

    def _select_hip(self, patches, pos_enc, order=None):
        """encode -> logits -> selection loop on the ROCm device (which producer, how the loop follows it: selection.py);
        patches may still be on the host (lazy loading); ``order``: a shuffle applied as an index (``_shuffle``)."""
        return self.selection.select(patches, pos_enc, order)

    def _iterate(self, mem_emb, mem_ids, emb, ids, pos_table, rows=False):
        """One iteration of the reference's loop on stock ATen ops (:229-241): the memory first, the chunk ``emb`` / ``ids``
        after, positions added through the ids (``pos_table``: (B, N, D), used with ``use_pos``), ``score_and_select``
        -> (mem_emb, mem_ids, top).  ``rows``: ``top`` is the (B, M) compact candidate rows that were kept (a stream
        gathers its patches with them), else None."""
        cand_emb = torch.cat((mem_emb, emb), dim=1)
        cand_ids = torch.cat((mem_ids, ids), dim=1)
        cand_pos = None
        if self.use_pos:
            cand_pos = cand_emb + torch.gather(pos_table, 1, cand_ids.unsqueeze(-1).expand(-1, -1, self.D))
        if not rows:
            return (*self.score_and_select(cand_emb, cand_pos, self.M, cand_ids), None)
        idx = torch.arange(cand_ids.shape[1], dtype=torch.int64, device=emb.device).unsqueeze(0).expand(emb.shape[0], -1)
        mem_emb, top = self.score_and_select(cand_emb, cand_pos, self.M, idx)
        return mem_emb, torch.gather(cand_ids, 1, top), top

    def _select_aten(self, patches, pos_enc):
        """The reference's loop on stock ATen ops (CPU plumbing path)."""
        B, N = patches.shape[:2]
        D, device = self.D, self.device
        order = torch.arange(N, dtype=torch.int64, device=device).unsqueeze(0).expand(B, -1)
        mem_emb = mem_idx = None
        for lo, hi in self._chunks(N):
            part = patches[:, lo:hi].to(device)
            emb = self._embed(part.reshape(-1, *patches.shape[2:])).view(B, hi - lo, D)
            if mem_emb is None:
                mem_emb, mem_idx = emb, order[:, lo:hi]
                continue
            mem_emb, mem_idx, _ = self._iterate(mem_emb, mem_idx, emb, order[:, lo:hi], pos_enc)
        self._mem_emb = mem_emb
        return mem_idx

    @property
    def last_mem_emb(self):
        """(B, M, D) embeddings (without positional encoding) of the patches the last ``ips()`` selected,
        as the encoder computed them in eval mode - or ``None`` (shortcut M >= N).  In eval mode
        ``encoder(mem_patch)`` in ``forward`` recomputes exactly these (reference :273 after :209/:227 with
        running BatchNorm statistics), so an eval loop can hand them back through ``forward(..., mem_emb=)``
        and skip the second encoder pass (SURVEY.md section 8 f, N-a).  Gathered on first use."""
        if self._mem_emb is None and self._emb_make is not None:
            make, self._emb_make = self._emb_make, None
            self._mem_emb = make()
        elif self._mem_emb is None and self._emb_parts and self.last_mem_idx is not None:
            parts, self._emb_parts = self._emb_parts, None
            self._mem_emb = self._take(parts[0] if len(parts) == 1 else torch.cat(parts, dim=1), self.last_mem_idx)
        return self._mem_emb

    @property
    def last_mem_count(self):
        """After ``ips_ragged(slides, pad=True)``: the tuple of the B host ints min(N_b, M) - the slots of every slide that
        hold rows of it, the rest being zero padding.  None after every other selection."""
        return self._mem_count

    # ---------------------------------------------------------------- aggregation
    def _filled_counts(self, mem_count, B, M):
        """The checked counts of ``forward(mask_encoder=True)`` -> a tuple of B host ints; nothing is launched or put on a
        device.  Refuses: no counts, a count tensor on a GPU (the packed sizes are host numbers; reading it back would
        synchronise), another length than B, an entry outside 1 .. M, one filled row in all under an encoder in training mode."""
        if mem_count is None:
            raise ValueError("mask_encoder=True needs mem_count: the filled slots of every slide")
        if torch.is_tensor(mem_count) and mem_count.device.type != "cpu":
            raise ValueError("mask_encoder=True needs mem_count on the host (a sequence of ints or a CPU tensor): the packed "
                             "sizes are host numbers, and reading a device tensor back would synchronise")
        counts = tuple(hip.slot_counts("forward(mask_encoder=True)", mem_count, B, M, torch.device("cpu")).tolist())
        if sum(counts) == 1 and self.encoder.training:
            raise ValueError("Expected more than 1 value per channel when training, got ONE filled row in the batch "
                             "(mask_encoder=True: BatchNorm's batch statistics are taken over the filled rows)")
        return counts

    def _filled_index(self, counts, M, device):
        """-> (rows64, rows32): the flat row numbers ``cat_b(range(b * M, b * M + counts[b]))`` on ``device``, as int64 for ATen
        and as int32 for the fused projector.  Built once per (counts, M, device) and kept."""
        key = (counts, M, torch.device(device))
        kept = self._filled_rows
        if kept is None or kept[0] != key:
            rows = torch.cat([torch.arange(b * M, b * M + c, dtype=torch.int64) for b, c in enumerate(counts)]).to(device)
            kept = self._filled_rows = (key, (rows, rows.to(torch.int32)))
        return kept[1]

    def _embed_filled(self, flat, rows):
        """The masked encoder pass: the encoder, in its current mode, on the filled rows of ``flat`` only (``rows``: the pair of
        ``_filled_index``) -> (B * M, D) with the padding slots exactly +0.0 (ATen ``index_copy`` into zeros: its backward
        gathers the filled rows' gradient, the padding's is exactly 0)."""
        packed = self._embed(flat, rows)
        return packed.new_zeros((flat.shape[0], packed.shape[1])).index_copy(0, rows[0], packed)

    def forward(self, mem_patch, mem_pos=None, mem_emb=None, mem_count=None, mask_encoder=False):
        """Embed the M selected patches, aggregate, classify (reference :264-283).

        ``mem_count`` (optional, not in the reference): the filled slots of every slide of a zero-padded buffer - after a
        ``pad=True`` selection ``net(mem_patch, mem_pos, mem_count=net.last_mem_count)``.  Handed to the aggregator
        (``Transformer.forward(x, count=)``): slide b is classified from its first mem_count[b] slots only, as the solo call
        on them would classify it; the padding is still embedded (with the encoder in training mode it takes part in the
        BatchNorm batch statistics, the running-statistics update and the weight gradients: ``mask_encoder``).  None (the
        default; ``last_mem_count`` is never read here): every slot is attended to, as in the reference.

        ``mask_encoder`` (optional, not in the reference; needs ``mem_count`` as B host integers): the encoder pass runs on
        the filled rows only - ``emb = zeros(B * M, D); emb[rows] = _embed(flat[rows])`` with
        ``rows = cat_b(range(b * M, b * M + mem_count[b]))``.  In training mode the batch statistics, the ``running_*``
        update, ``num_batches_tracked`` and every parameter gradient are those of the encoder on the sum(mem_count) filled rows;
        nothing at or beyond ``mem_count[b]`` is read, whatever it holds; the padding slots of the embedding are exactly
        +0.0.  Refused before anything is launched (ValueError): no ``mem_count``, counts on a GPU, of another length than B
        or outside 1 .. M, and ONE filled row in all with the encoder in training mode (BatchNorm's batch statistics need
        more than one value per channel).  With ``mem_emb`` and the encoder in eval mode there is no encoder pass and the flag
        has nothing to do.  False (the default): every route runs as without the argument.

        ``mem_emb`` (optional, not in the reference): embeddings of ``mem_patch`` already computed by ``ips()``
        in eval mode (``last_mem_emb``); used instead of a second encoder pass when the encoder is in eval
        mode, ignored in train mode where BatchNorm uses batch statistics and the pass carries gradients."""
        B, M = mem_patch.shape[:2]
        counts = self._filled_counts(mem_count, B, M) if mask_encoder else None
        if mem_emb is None or self.encoder.training:
            flat = mem_patch.reshape(-1, *mem_patch.shape[2:])
            if counts is None:
                mem_emb = self._embed(flat)
            else:           # (the index is built here: with mem_emb handed to an eval-mode encoder the flag has nothing to do)
                mem_emb = self._embed_filled(flat, self._filled_index(counts, M, mem_patch.device))
            mem_emb = mem_emb.view(B, M, -1)
        if torch.is_tensor(mem_pos):
            mem_emb = mem_emb + mem_pos
        if mem_count is not None:
            return self.get_preds(self.transf(mem_emb, count=mem_count))
        return self.get_preds(self.transf(mem_emb))
