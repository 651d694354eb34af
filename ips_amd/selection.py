"""How ``IPSNet.ips`` runs on a ROCm device: encode -> logits -> selection loop -> ``mem_idx``.

The reference runs a Python loop of ~75 stock kernels per chunk (architecture/ips_net.py:213-241).  In eval / no-grad
mode a patch's embedding and its attention logits depend on that patch alone, so the HIP path encodes and scores every
patch once and replays the loop on the cached logits.  This module is the scheduling around those
kernels - ONE pipeline with two choices:

  producer   who turns patches into (embeddings, logits), and in which pieces
               ``parts``    a list of launches over slices / index lists of the patch axis (any encoder)
               ``stream``   one persistent launch that publishes rows as they complete (the fused 1x32x32 trunk for one
                            image, the projector for feature slides)
  loop       how the selection loop follows the producer
               ``persistent``  launched once, up front, on a compute unit of its own; waits (bounded) for published rows
               ``ranges``      ``scan_range`` per part on a high-priority side stream (resumes from ``mem_idx``)
               ``after``       one ``scan`` behind the last part (lazy slabs run ranges beside the copies)

Every choice computes the same per-patch arithmetic, so all of them select the same patches
(tests/test_hip_e2e.py::test_every_variant_..., test_one_image_every_schedule_...).

Launch sizes come from the device (``hip.device_geometry``): a producer that runs beside resident loops is sized for the
compute units they leave free on the FULLEST XCD (workgroups are dealt to XCDs round-robin), the fused trunk's
"round" is 8 patches per compute unit.  Whether persistent kernels can run beside their producers at all is established
ONCE per device by a self-test (``hip.persistent_ok``: under counter collection or a serialising debug switch they
cannot), checked again when a loop times out, and revoked for the process when that check fails or loops keep timing out
(``hip.persistent_timed_out``).
"""

import contextlib
import ctypes as C
import gc
import math
import os
import weakref

import torch

from . import hip


@contextlib.contextmanager
def _no_gc_pause():
    """Between the launch of a resident loop and the launch of its producers the host must not stall: the loop gives up
    after 50 ms without progress (the call is then redone, results valid - but it costs 50 ms and counts as a strike).
    What did stall it, once in ~5,000 calls of a soak run (tools/soak.py, profiles/r05_soak.txt): a full collection of the
    interpreter's cyclic garbage collector, 40-60 ms in a process that has torch loaded, landing between the two launches.
    The collector is held off for those few lines (an allocation-count trigger is only postponed)."""
    was = gc.isenabled()
    if was:
        gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


def _env_on(name):
    return os.environ.get(name, "1") != "0"


# IPSX_NATIVE_ORDER when the environment does not set it.  Off: measured against the launches one by one, in one process,
# the ordered one call of a lone slide is 0.006 - 0.016 ms faster, inside the quartiles of either (DESIGN 2.1,
# profiles/shuffle_routes_native_order_ab.json) - not the margin that was asked of it
NATIVE_ORDER_DEFAULT = "0"

# IPSX_SCAN_LOGITS_ROWS when the environment does not set it: the most rows per image of a part whose logits the loop's launch
# computes itself (``Selection.parts_loop_logits``); a longer part gets a logits launch in front of the loop's.  One workgroup
# per image computes such rows on ONE compute unit, ~4.3 us per 100 rows measured, where a launch across the device costs its
# floor of ~5 us and little more: level at ~150 rows, measured to pay at 125 (19.0 -> 18.0 us) and to lose at 375 (43.1 -> 49.7 us;
# DESIGN 5.4, profiles/scan_logits_trace.txt).  128 = one 32-row tile per SIMD of the workgroup's compute unit.
SCAN_LOGITS_ROWS_DEFAULT = "128"
# IPSX_SCAN_TAIL_ROWS when the environment does not set it: the most rows per image the trailing parts of a counted call may
# hold together to go into ONE last launch behind the trunk's, let go by a device-side gate (``Selection.parts_loop_logits``,
# DESIGN 5.4).  Its prologue - 4.3 us per 100 rows - runs beside the side stream's last iterations and has to end before they
# do.  IPSX_SCAN_TAIL=0: the chain as it was.
SCAN_TAIL_ROWS_DEFAULT = "512"

# IPSX_ONE_LAUNCH_U8 when the environment does not set it.  Off: the rule was "faster than the parent's uint8 median by more
# than the parent's own max - min on all three shapes".  16 x 1600x1600 uint8 images met it twice (stride 32: 0.48 / 0.49 ms
# against 0.11 / 0.13; stride 16: 0.93 / 0.85 against 0.44 / 0.23); 16 x 2,500 uint8 patches missed it in the first of two
# sessions (0.45 ms against a max - min of 0.49) and met it in the second (0.49 against 0.34) - DESIGN 2.3,
# profiles/parts_u8_view.json, profiles/uint8_patches{,_parent,_first,_first_parent}.json
ONE_LAUNCH_U8_DEFAULT = "0"


def _native_order_on():
    """Feature slides that select through a shuffle index inside the library's one call (``ipsx_ips_call_run_ordered``,
    DESIGN 2.1): ``IPSX_NATIVE_ORDER=1``.  Otherwise such a call enqueues its launches one by one.  (One image on the
    fused trunk takes the ordered one call either way: its alternative is the copy.)"""
    return os.environ.get("IPSX_NATIVE_ORDER", NATIVE_ORDER_DEFAULT) == "1"


class Selection:
    """The selection pipelines of one ``IPSNet`` (buffers and streams are kept between calls of the same shape: a buffer
    that a side stream has used cannot be recycled by the allocator until that stream's work is known to be over, and
    allocating afresh in every call sends a host that runs ahead of the GPU back to the driver)."""

    OVERLAP_PARTS = 4
    SCAN_LOGITS_ROWS = int(os.environ.get("IPSX_SCAN_LOGITS_ROWS", SCAN_LOGITS_ROWS_DEFAULT))    # (read once, not per call)
    LAZY_SLAB_BYTES = 48 << 20

    def __init__(self, net, owned=False):
        # ``owned``: built by ``IPSNet.selection`` and kept by the net - then the way back is a weak reference, so that a net
        # nobody holds any more releases its call buffers at once and not when the cyclic collector next runs
        self._net = weakref.ref(net) if owned else (lambda: net)
        self._bufs = {}
        self._side = None
        self._copy = None
        self.scan_status = None          # status word of the last persistent loop (device), its host mirror
        self.scan_status_host = None
        self._mirror_pending = None
        self._unfinished = None
        self._side_pending = self._side_event = None     # the event behind the last counted call's side-stream kernels, while no main-stream wait has covered them
        self.caller_finishes = False               # IPSNet._call: the call ends in ``finish`` / ``take_unfinished`` + ``after_call``
        self._done = None                          # (mem_idx, mem_patch, mem_pos) of a call the library enqueued whole
        self._calls = {}                           # hip.IpsCall structures, per pipeline
        self.timing_hook = None                    # callable(rows) -> slot of a library-owned event pair around the producer, or None
        self._part_index = None
        self._order = None                         # the permutation this call selects through (an index, not a copy), or None
        self._order_bn = None                      # ... its call's (B, N)
        self._flat_made = None                     # ... as flat int32 row numbers b * N + perm[b, j], (B, N): made on first use
        self._flat_key = None
        self._flat_base = None
        self._part_map = None                      # parts_with_ranges: where the parts' index lists lie in the flat (B, N) index
        self._one_piece_index = {}                 # index_supported: does a layered trunk's stem take an index list, per patch shape
        self.index_calls = 0                       # select() calls that read the patches through a shuffle index
        self.view_calls = 0                        # select_view() calls: the patches read through a patch-grid view
        self.native_calls = 0                      # calls the library enqueued whole (ipsx_ips_call_run*)
        self.native_ordered_calls = 0              # ... of which through a shuffle index (ipsx_ips_call_run_ordered)

    # ------------------------------------------------------------------ small helpers
    @property
    def net(self):
        return self._net()

    def plan(self):
        return self.net.plan

    @property
    def _flat(self):
        """The call's shuffle index as flat int32 row numbers (B, N), or None - composed on FIRST use: the ordered one-call
        route never asks (the library composes its own, ``ipsx_order_index``)."""
        if self._order is None:
            return None
        if self._flat_made is None:
            self._flat_made = self.flat_index(self._order, *self._order_bn)
        return self._flat_made

    def status_mirror(self):
        """The pinned host mirror of a resident loop's status word, made on first use."""
        if self.scan_status_host is None:
            self.scan_status_host = torch.zeros((1,), dtype=torch.int32).pin_memory()
        return self.scan_status_host

    def check_strike(self, dev):
        """Look at the mirror of the PREVIOUS call's status word (it has long arrived): a loop or a wait that gave up
        clears it and counts as an event (``hip.persistent_timed_out``: the device's self-test again; the persistent
        pipelines go off for the process only after repeated events)."""
        mirror = self.scan_status_host
        if mirror is not None and int(mirror.item()) & 1:
            mirror.zero_()
            hip.persistent_timed_out(dev)

    def n_iter(self, N):
        return math.ceil((N - self.net.M) / self.net.I)

    def streams(self, dev):
        if self._side is None or self._side.device != torch.device(dev):
            self._side = hip.side_stream(dev)      # (one per device and process, high priority: hip.side_stream)
            self._side_pending = self._side_event = None
        return self._side, torch.cuda.current_stream(dev)

    def buffers(self, name, key, make):
        """Per-call device buffers of pipeline ``name``, re-made only when ``key`` (the shape) changes."""
        held = self._bufs.get(name)
        if held is None or held[0] != key:
            bufs = make()
            side = self._side
            for t in bufs:
                if t is not None and side is not None:
                    t.record_stream(side)
            self._bufs[name] = held = (key, bufs)
        return held[1]

    def persistent_allowed(self, dev, M, I, H, T, loops=1, large=False):
        """Resident loops beside their producers: switched on, the shape is covered, the device has units to spare for
        ``loops`` of them (a small partition: the producers need the units more) and it has been SEEN to work there."""
        return (_env_on("IPSX_SCAN_PERSIST") and _env_on("IPSX_OVERLAP_SCAN") and not hip.dedup_blank()
                and (hip.scan_persistent_supported(M, I, H, T) or (large and hip.scan_persistent_large(M, I, H, T)))
                and hip.device_geometry(dev).cus >= 8 * max(1, loops)
                and hip.persistent_ok(dev))

    # ------------------------------------------------------------------ the persistent loop: begin / end
    def persistent_begin(self, logits, mem_idx_buf, zeroed, B, dev, loops=0, scan_ws=None, zero_words=None):
        """Zero the call's words (tie flags | a progress word per image | status | producer control words: ONE fill), launch
        the loop on the side stream and hold the main stream until it is resident.  -> (tie, ready, status, ctl).

        A loop that gave up waiting (no progress for hip.persistent_wait_ms: something serialises the kernels, so that its
        producers cannot run beside it) is REDONE in the same call by the conditional launch of ``persistent_end``, so a
        call's results are valid either way and no host synchronisation is added.  The status word is mirrored into pinned
        host memory, asynchronously, and looked at in the NEXT call - by then it has long arrived: a timeout re-runs the
        device's self-test, and repeated timeouts (``hip.persistent_timed_out``: IPSX_PERSIST_STRIKES, default 3) or a failing
        self-test switch the persistent pipelines off for the rest of the process (the per-part launches take over)."""
        # (first: everything below is host work in front of the call's second launch; zero_words: the projector stream's
        #  control words end in hand-over accumulators that need no zeroing)
        (zeroed if zero_words is None else zeroed[:zero_words]).zero_()
        hip._PERSIST_CALLS += 1
        net = self.net
        ca = net.transf.crs_attn
        self.check_strike(dev)
        side, main = self.streams(dev)
        tie, words, ctl = zeroed[:B], zeroed[B:2 * B + 1], zeroed[2 * B + 1:]
        ready, status = words[:B], words[B:B + 1]
        self.scan_status = status
        side.wait_stream(main)                     # the buffers are the main stream's; previous readers are done
        hip.scan_persistent(logits, net.M, net.I, ca.H, ca.n_token, mem_idx_buf, tie, ready, status, workgroups=loops,
                            workspace=scan_ws, stream=side)
        # producers must not take the compute units before a loop has its own.  (Also true of a persistent producer whose
        # workgroups sit one to a unit and leave a unit per loop free: a workgroup is dealt to an XCD before it looks for a
        # unit there, so a loop that arrives second may be dealt to a FULL XCD and start when the producer ends - measured
        # without the gate: 31 M patches/s with calls back to back against 43 M, one CAMELYON slide.)
        hip.scan_gate(status)
        return tie, ready, status, ctl

    def persistent_end(self, logits, mem_idx_buf, tie, status, n_iter, dev, scan_ws=None):
        net = self.net
        ca = net.transf.crs_attn
        side, main = self.streams(dev)
        main.wait_stream(side)
        hip.scan_range_if(logits, net.M, net.I, ca.H, ca.n_token, 0, n_iter, mem_idx_buf, tie, status, 1,
                          workspace=scan_ws)                                                           # no-op unless timed out
        self._mirror_pending = status              # (copied to the host by after_call: behind the call's gathers)
        hip.scan.last_tie = tie
        # the loop's own buffer - overwritten by the next call: ``finish`` (one launch: both gathers, a fresh copy of these
        # indices, the status word to the host) or ``take_unfinished`` + a copy is the caller's next step
        self._unfinished = mem_idx_buf
        return mem_idx_buf

    def finish(self, src, pos, order=None):
        """The end of an ``ips()`` call whose loop ran resident, as ONE launch (``hip.ips_finish``: both gathers, a fresh copy
        of the selected indices, the loop's status word to its pinned host mirror) -> (mem_idx, mem_patch, mem_pos), or None
        when this call has nothing of the kind pending or the tensors' rows are not whole 16-byte units (the caller then
        gathers itself and ``after_call`` mirrors the status word).  ``order``: the call selected through a shuffle index -
        the patch rows come from the unshuffled ``src`` through it."""
        done, self._done = self._done, None
        if done is not None:
            return done
        buf, self._unfinished = self._unfinished, None
        if buf is None:
            return None
        status = self._mirror_pending
        if status is None or src.dtype == torch.uint8 or not hip.ips_finish_supported(src, pos):     # (uint8: gather, then dequantise)
            self._unfinished = buf
            return None
        self._mirror_pending = None
        return hip.ips_finish(src, pos, buf, status, self.status_mirror(), order=order)

    def take_unfinished(self, mem_idx):
        """``mem_idx`` as a tensor of the caller's own (the loop's buffer is overwritten by the next call)."""
        buf, self._unfinished = self._unfinished, None
        return mem_idx.clone() if buf is not None and mem_idx is buf else mem_idx

    def native_ok(self, src, pos):
        """Can the library enqueue this call whole (``ipsx_ips_call_run``)?  Needs what ``ips_finish`` needs of the tensors."""
        return _env_on("IPSX_NATIVE_CALL") and src.dtype != torch.uint8 and hip.ips_finish_supported(src, pos)

    def native_call(self, name, patches, pos_enc, logits, mem_idx_buf, zeroed, emb_buf, scan_ws, loops, wgs, trunk_pos=None,
                    quad_pulls=-1, short_first=-1):
        """One ips() call with a resident loop, enqueued by ONE library call (csrc/call.hip): fill, loop on the side stream,
        gate, producer (the fused trunk for one image / the projector for feature slides), conditional recovery, and the end
        of the call (both gathers, indices, status word to the host).  Same kernels and results as the launches one by one
        (``IPSX_NATIVE_CALL=0``); the host's share of a call is one ctypes call, and nothing of the interpreter sits between
        the loop's launch and its producer's.  A call that selects through a shuffle index (``self._order``): the same one
        call with the order inside it (``ipsx_ips_call_run_ordered``: ``patches`` is the unshuffled tensor, the flat index is
        composed by the library into a workspace kept with the pipeline's buffers, everything else is in shuffled
        numbering).  -> mem_idx (fresh); ``finish`` hands out (mem_idx, mem_patch, mem_pos)."""
        net, plan = self.net, self.plan()
        B, N = patches.shape[:2]
        dev = patches.device
        ca = net.transf.crs_attn
        vq, R = ca.folded_query(), ca.H * ca.n_token
        self.check_strike(dev)
        mirror = self.status_mirror()
        hip._PERSIST_CALLS += 1
        side, _ = self.streams(dev)
        plan._refresh()
        c = self._calls.get(name)
        if c is None or c[0] is not logits:
            call = hip.IpsCall()
            call.b, call.n, call.m, call.i, call.h, call.n_token = B, N, net.M, net.I, ca.H, ca.n_token
            call.logits, call.mem_idx = logits.data_ptr(), mem_idx_buf.data_ptr()
            call.words, call.words_total = zeroed.data_ptr(), zeroed.numel()
            call.loops = loops
            call.scan_workspace = scan_ws.data_ptr() if scan_ws is not None else None
            call.scan_workspace_bytes = scan_ws.numel() if scan_ws is not None else 0
            call.emb, call.r, call.workgroups = emb_buf.data_ptr(), R, wgs
            call.quad_pulls, call.short_first = quad_pulls, short_first
            call.status_host = mirror.data_ptr()
            call.side_stream = side.cuda_stream
            c = self._calls[name] = (logits, call, (mem_idx_buf, zeroed, emb_buf, scan_ws, mirror))
        call = c[1]
        if net.is_image:
            call.trunk, call.lin = C.pointer(plan.trunk), None
            call.pos = trunk_pos.data_ptr() if trunk_pos is not None else None
        else:
            call.trunk, call.lin, call.ln_eps = None, C.pointer(plan.lin), plan.ln_eps
        call.x = patches.data_ptr()
        call.v_packed = vq.data_ptr()
        M = net.M
        mem_patch = torch.empty((B, M) + tuple(patches.shape[2:]), dtype=patches.dtype, device=dev)
        mem_idx = torch.empty((B, M), dtype=torch.int64, device=dev)
        mem_pos = None
        call.src = patches.data_ptr()
        call.src_row_bytes = patches[0, 0].numel() * patches.element_size()
        call.src_bstride_rows = N if B > 1 else 0
        if pos_enc is not None:
            mem_pos = torch.empty((B, M, pos_enc.shape[2]), dtype=pos_enc.dtype, device=dev)
            call.pos_table = pos_enc.data_ptr()
            call.pos_row_bytes = pos_enc.shape[2] * pos_enc.element_size()
            call.pos_bstride_rows = 0 if (pos_enc.stride(0) == 0 or B == 1) else N
            call.mem_pos = mem_pos.data_ptr()
        else:
            call.pos_table, call.pos_row_bytes, call.pos_bstride_rows, call.mem_pos = None, 0, 0, None
        call.mem_patch, call.mem_idx_out = mem_patch.data_ptr(), mem_idx.data_ptr()
        call.timing_slot = self.timing_hook(B * N) if self.timing_hook is not None else -1
        call.stream = hip._stream().value
        order = self._order
        if order is not None:
            if order.dtype != torch.int64 or order.dim() != 2 or order.shape[1] != N or order.shape[0] not in (1, B) or \
                    not order.is_contiguous() or order.device != dev:
                raise ValueError("order must be a contiguous (B or 1, N) int64 tensor on the patches' device")
            (index_ws,) = self.buffers(name + ".order", (B, N, str(dev)),
                                       lambda: (torch.empty((B * N,), dtype=torch.int32, device=dev),))
            o = hip.IpsCallOrder(order.data_ptr(), N if order.shape[0] > 1 else 0, index_ws.data_ptr())
            hip._ck(hip.lib().ipsx_ips_call_run_ordered(C.byref(call), C.byref(o)), "ipsx_ips_call_run_ordered")
            self.native_ordered_calls += 1
        else:
            hip._ck(hip.lib().ipsx_ips_call_run(C.byref(call)), "ipsx_ips_call_run")
        self.native_calls += 1
        tie, status = zeroed[:B], zeroed[2 * B:2 * B + 1]
        self.scan_status = status
        hip.scan.last_tie = tie
        net._emb_parts = [emb_buf]
        self._done = (mem_idx, mem_patch, mem_pos)
        return mem_idx

    def after_call(self):
        """The last thing an ``ips()`` call enqueues: the status word of its persistent loop goes to its pinned host mirror
        (looked at in the NEXT call) - behind the gathers of the selected patches, not in front of them."""
        status = self._mirror_pending
        if status is not None:
            self._mirror_pending = None
            self.status_mirror().copy_(status, non_blocking=True)

    # ------------------------------------------------------------------ which pipeline
    def source(self, patches):
        """The ``hip.PatchSource`` the parts of a call are index lists into: the one ``select`` was handed, or - image
        patches that are device-resident and contiguous - built here, ONCE per call, with the net's table for bytes; else
        None (feature rows, strided patches)."""
        if not torch.is_tensor(patches):
            return patches
        if self.net.is_image and patches.is_cuda and patches.is_contiguous():
            return hip.PatchSource(patches, self.net._table_for(patches))
        return None

    def select(self, patches, pos_enc, order=None):
        """(B, N, ...) patches (device, or host for lazy loading) -> mem_idx (B, M) int64 on the device.  Image nets also
        take a ``hip.PatchSource``: with a view, whole images whose patch tensor is never made (``select_view``).

        ``order`` ((B or 1, N) int64 on the device; only where ``index_supported``): select as if the patch axis had been
        permuted by it - ``patches`` is the UNSHUFFLED tensor, the encoders read row ``order[b, j]`` where they would read
        row j of the shuffled copy, and everything behind that first read (``pos_enc``, which IS shuffled, embeddings,
        logits, the loops, ``mem_idx``) is in shuffled numbering."""
        net = self.net
        net._device_patches = None
        self._done = self._unfinished = None       # (whatever a call that raised half-way left behind)
        self._order = self._order_bn = self._flat_made = None
        if order is not None:
            self._order, self._order_bn = order, (patches.shape[0], patches.shape[1])
            self.index_calls += 1
        if not torch.is_tensor(patches):
            # the one-image stream and the native one-call route read patch tensors: a view takes the parts (every part an
            # index list of grid patches - the fused trunk's one launch, the small-batch split, layered trunks too) or, for
            # a short loop, one piece
            self.view_calls += patches.is_view
            return self.parts_with_ranges(patches, pos_enc) if self.can_overlap(patches) else self.slabs(patches, pos_enc)
        if patches.is_cuda and patches.is_contiguous() and self.can_stream_image(patches):
            return self.image_stream(patches, pos_enc)
        if patches.is_cuda and self.can_overlap(patches):
            ca = net.transf.crs_attn
            if (not net.is_image and patches.is_contiguous() and patches.shape[0] <= int(os.environ.get("IPSX_PERSIST_MAX_B", "16"))
                    and self.persistent_allowed(patches.device, net.M, net.I, ca.H, ca.n_token, self.feature_loops(patches.shape[0]),
                                                large=_env_on("IPSX_LARGE_PERSIST"))):
                return self.features_persistent(patches, pos_enc)
            return self.parts_with_ranges(patches, pos_enc)
        return self.slabs(patches, pos_enc)

    def select_view(self, images, view, pos_enc, order=None, table=None):
        """``select`` on the patches of whole images (B, C, H, W) on the device - float32, or uint8 with their ``table`` -
        read through ``view`` (a ``hip.PatchView`` the plan supports: ``EncoderPlan.view_supported``).  Patch numbers are
        those of the tensor ``hip.patchify`` would make, so ``order``, ``pos_enc`` and ``mem_idx`` mean what they mean in
        ``select``.  uint8 images take the schedules float32 images take - the one counted launch (``one_launch_ok``) under
        ``IPSX_ONE_LAUNCH_U8=1``."""
        return self.select(hip.PatchSource(images=images, view=view, table=table), pos_enc, order)

    def index_supported(self, patches):
        """Can the schedule ``select`` picks for these patches read them through a shuffle index?  Device-resident,
        contiguous patches on: every feature pipeline (the row-indexed projector kernels), the fused 1x32x32 trunk in
        parts (its index list) and as the one-image stream (the stream's tiles read the same list), and a layer-by-layer
        trunk in one piece whose stem takes an index list (``EncoderPlan.index_list_supported``).  Not: lazy patches, the
        small-batch split and the fused trunk in one piece, layer-by-layer trunks in parts, blank-patch dedup (DESIGN 2.1:
        those shuffle by copy).  uint8 patches: where float32 patches are (the index list addresses bytes; the gather at
        the end of the call reads them through the order, then dequantises), the parts' one counted launch
        (``IPSX_ONE_LAUNCH_U8=1``) included - the one-image stream reads float32."""
        net = self.net
        # (a hip.PatchSource is device-resident and contiguous by construction)
        if (torch.is_tensor(patches) and not (patches.is_cuda and patches.is_contiguous())) or hip.dedup_blank() or net.encoder.training:
            return False
        if not net.is_image:
            return patches.dim() == 3 and patches.dtype in (torch.float32, torch.float16, torch.bfloat16)
        if self.can_stream_image(patches):
            return patches.dtype == torch.float32
        if not self.can_overlap(patches):
            # one piece (``slabs``): a layered trunk reads float32 / uint8 patches through the list where its stem takes one;
            # the fused trunk's small batches keep the copy
            # (asked once per patch shape: the answer is the trunk's geometry, and asking walks the plan's weights)
            key = (tuple(patches.shape[-3:]), hip.precision(), os.environ.get("IPSX_NO_FUSED"))
            if key not in self._one_piece_index:
                plan = self.plan()
                self._one_piece_index[key] = not plan.fused(patches.shape) and plan.index_list_supported(patches.shape)
            return patches.dtype in (torch.float32, torch.uint8) and self._one_piece_index[key]
        B, N = patches.shape[:2]
        if B * N < self.small_batch_limit(patches.device) and self.n_iter(N) < 100:
            return False
        return bool(self.plan().fused(patches.shape))

    def flat_index(self, order, B, N):
        """(B or 1, N) int64 permutation -> (B, N) int32 flat row numbers b * N + order[b, j], composed once per call (one
        permutation for the whole batch: kept as long as the permutation tensor is the same)."""
        shared = order.shape[0] == 1
        key = (id(order), order._version, B, N) if shared else None
        if shared and self._flat_key is not None and self._flat_key[0] == key and self._flat_key[1] is order:
            return self._flat_key[2]
        # (host work in front of the call's first launch: one conversion, and one addition when there are several images -
        #  the images' first rows b * N are kept between calls)
        flat = order.to(torch.int32)
        if B > 1:
            if self._flat_base is None or self._flat_base[0] != (B, N, order.device):
                self._flat_base = ((B, N, order.device), (torch.arange(B, device=order.device, dtype=torch.int32) * N).unsqueeze(1))
            flat = flat + self._flat_base[1]
        self._flat_key = (key, order, flat) if shared else None
        return flat

    def can_overlap(self, patches):
        """Does the loop run beside the encoder (parts + ranges, or a persistent loop)?"""
        net = self.net
        if not _env_on("IPSX_OVERLAP_SCAN") or hip.dedup_blank() or net.encoder.training:
            return False
        B, N = patches.shape[:2]
        n_iter = self.n_iter(N)
        if net.is_image and B * N < self.small_batch_limit(patches.device) and n_iter < 100:
            # a small batch does not fill the GPU four times over: it is encoded in the whole rounds of the fused trunk it
            # fills plus the remainder, the loop over the first part beside the remainder's encoding (small_batch_split);
            # a layer-by-layer trunk cut in two just runs every layer twice at half the occupancy (measured: traffic
            # signs 25.3 ms against 22.7 ms in one piece)
            return self.plan().fused(patches.shape) and self.small_batch_split(B, N, patches.device) is not None
        # (feature inputs: the loop is the long pole whatever its length - a slide at the reference's shipped M = I = 5000
        #  has 7 iterations of 10,000 candidates - so any loop of a few iterations runs beside the projector's later parts)
        return n_iter >= (2 * self.OVERLAP_PARTS if net.is_image else 3)

    def can_stream_image(self, patches):
        """ONE image on the fused fp32 1x32x32 trunk: trunk + logits as one persistent launch beside a resident loop
        (contiguous patches: the caller's to check)."""
        net = self.net
        if (not net.is_image or patches.shape[0] != 1 or net.encoder.training
                or not _env_on("IPSX_IMAGE_STREAM") or patches.shape[1] < net.M + 2 * net.I
                or patches.dtype == torch.uint8):          # (the stream kernel reads float32: uint8 goes through the parts)
            return False
        ca = net.transf.crs_attn
        return (self.persistent_allowed(patches.device, net.M, net.I, ca.H, ca.n_token)
                and self.plan().image_stream_supported(patches.shape, net.D, ca.H * ca.n_token)
                and ca.folded_query().dtype == torch.float32)

    # ------------------------------------------------------------------ sizes that come from the device
    @staticmethod
    def round_patches(dev):
        """Patches of one full round of the fused trunk: 8 per compute unit (two workgroups of four wavefronts = patches)."""
        return 8 * hip.device_geometry(dev).cus

    def small_batch_limit(self, dev):
        return 16 * self.round_patches(dev)

    def free_units(self, dev, loops):
        """Compute units a single-round launch can count on beside ``loops`` resident loop workgroups: workgroups are
        dealt to the XCDs round-robin whatever is free there, so it is the free units of the FULLEST XCD, times the XCDs."""
        g = hip.device_geometry(dev)
        return g.xcds * (g.cus_per_xcd - -(-loops // g.xcds))

    def small_batch_split(self, B, N, dev):
        """How to cut a small image batch (one round of the fused trunk and a remainder): (edges, its) - part k encodes rows
        edges[k]..edges[k+1] of every image and the loop then runs iterations its[k]..its[k+1], those whose rows are
        encoded by then - or None when that leaves nothing on either side.  The parts are the ENCODER's units: half a round
        first (one wavefront per SIMD), then half a round less one workgroup per XCD and shader-engine pair - a compute
        unit stays free for the loop of the part before wherever the dispatcher lands (on a unit it shares with fp32 MFMA
        wavefronts an iteration takes 24 us instead of 6.7, tools/scan_beside.py) - then the rest, which goes through the
        two-wavefronts-per-patch kernel.  On 256 units: 1,024 + 992 + 484 patches of one 2,500-patch image, iterations
        15 + 15 + 9.  Measured (bench.py --config b1 / --batch 2): +8 % at one round + remainder, -4 % at two rounds."""
        M, I = self.net.M, self.net.I
        n_iter = self.n_iter(N)
        rnd = self.round_patches(dev)
        if (B * N) // rnd != 1:
            return None
        half = rnd // 2
        g = hip.device_geometry(dev)
        edges, its = [0], [0]
        for total in (half, half + half - 4 * g.xcds):
            e = total // B
            it = (e - M) // I                                  # iterations whose rows lie inside the first e of every image
            if e < N and its[-1] < it < n_iter:
                edges.append(e)
                its.append(it)
        if len(its) == 1:
            return None
        return edges + [N], its + [n_iter]

    def feature_loops(self, B):
        """Resident loop workgroups of a call of B slides: one per slide, or - shapes whose loop kernel takes its slides
        in turn (ipsx_scan_persistent_on) - two for any number of slides."""
        net = self.net
        ca = net.transf.crs_attn
        if B > 2 and hip.scan_persistent_groupable(net.M, net.I, ca.H, ca.n_token):
            return max(1, min(B, int(os.environ.get("IPSX_CAM_LOOPS", "2"))))
        return B

    def feature_parts(self, B, N, dev, persistent):
        """Iterations at which the rows of ONE slide are cut into projector launches.  Persistent loops (each owns a compute
        unit, the projector goes slide by slide): equal parts that fill the other units exactly once; otherwise every
        launch takes its rows of all B slides and is sized to fill every unit once."""
        M, I = self.net.M, self.net.I
        n_iter = self.n_iter(N)
        rows = self.free_units(dev, B) * 64 if persistent else hip.device_geometry(dev).cus * 64 // max(B, 1)
        cap = max(I, rows // I * I)                          # most rows of a slide one launch can take, whole chunks
        n_part = min(16, max(1, math.ceil(N / cap)))
        its = [0]
        for k in range(1, n_part):                           # equal parts: edge k at about k * N / n_part rows
            nxt = max(its[-1] + 1, round((k * N / n_part - M) / I))
            if nxt >= n_iter:
                break
            its.append(nxt)
        its.append(n_iter)
        ca = self.net.transf.crs_attn
        if not persistent and n_iter >= 3 and hip.lib().ipsx_scan_workspace_bytes(1, M, I, ca.H, ca.n_token) > 0:
            # a candidate set beyond the LDS (the shipped CAMELYON M = I = 5000: 7 iterations of 0.2 ms): the loop is the
            # long pole and every further launch costs it a hand-over - TWO parts: the rows of the first two iterations,
            # then all the rest beside them (measured at 38,000 rows: parts 2+2+3 17.1 M patches/s, 2+5 17.7, 1+2+4 17.1,
            # 1+6 16.8, 3+4 16.6)
            its = [0, 2, n_iter]
        return its

    def feature_launches(self, B, N, edges, dev, loops=None):
        """The projector launches of ``features_persistent``: (first row, end row) in the FLAT (B * N) row space + what each
        makes visible, [(slide, rows)].  One slide, or positional encodings (a table per slide position): a slide's parts.
        Several slides without them: the slides are one stream of rows cut into full launches wherever a slide ends (the
        patch tensor is contiguous).  A full launch: the free units of the fullest XCD less one per XCD (measured on 256
        units at 2 / 16 slides: 208 workgroups 36.3 / 43.1 M patches/s, 224: 36.5 / 45.9, 240: 30.4 / 37.8 - now and then a
        workgroup of a fuller launch waits for a second round)."""
        I = self.net.I
        P = len(edges) - 1
        if B == 1 or self.net.use_pos:
            return [(b_ * N + edges[k], b_ * N + edges[k + 1], [(b_, edges[k + 1])]) for b_ in range(B) for k in range(P)]
        g = hip.device_geometry(dev)
        cap = max(I, min(g.cus - 4 * g.xcds, self.free_units(dev, loops or B)) * 64 // I * I)
        launches, r0 = [], 0
        while r0 < B * N:
            # the first launch of the call stays short: the first loop starts after M + I rows' worth of projector
            r1 = min(B * N, r0 + (cap if r0 > 0 else min(cap, edges[1])))
            pubs = [(b_, min(N, r1 - b_ * N)) for b_ in range(r0 // N, (r1 - 1) // N + 1)]
            launches.append((r0, r1, pubs))
            r0 = r1
        return launches

    # ------------------------------------------------------------------ pipeline: feature slides, persistent loops
    def features_persistent(self, patches, pos_enc):
        """Feature inputs, up to IPSX_PERSIST_MAX_B slides: every slide's loop is resident from the start of the call and
        follows its own progress word; the projector works through the slides one after the other, so the loop of slide b
        runs beside the projector of slide b + 1.  Without positional encoding and with fp32 logits the projector is ONE
        persistent launch (ipsx_projector_stream: moments + Linear + logits per tile, tiles published as they complete,
        across the slides' ends); otherwise launch by launch - per part the GEMM (LayerNorm in its operand load; its first
        thread publishes what was enqueued before it) and the logits of the part together with the row moments of the next."""
        net, plan = self.net, self.plan()
        B, N = patches.shape[:2]
        M, I, dev = net.M, net.I, patches.device
        ca = net.transf.crs_attn
        vq, R = ca.folded_query(), ca.H * ca.n_token
        n_iter = self.n_iter(N)
        self.streams(dev)
        logits, mem_idx_buf, zeroed, stats, emb_buf, scan_ws = self.buffers(
            "features", (B, N, M, I, R, net.D, str(dev)),
            lambda: (torch.empty((B, N, R), dtype=torch.float32, device=dev),
                     torch.empty((B, M), dtype=torch.int64, device=dev),
                     torch.zeros((2 * B + 1 + plan.stream_ctl_words(B * N),), dtype=torch.int32, device=dev),
                     torch.empty((B * N, 2), dtype=torch.float32, device=dev),      # LayerNorm moments
                     torch.empty((B, N, net.D), dtype=torch.float32, device=dev),
                     hip.scan_workspace(B, M, I, ca.H, ca.n_token, dev)))            # (candidate sets beyond the LDS; else None)
        # Resident loops: the projector goes through the slides in order and needs longer for a slide than its loop does
        # (65,536 x 2048 rows: 1.2 ms against 0.94), so TWO loop workgroups, each taking its slides one after the other,
        # keep up with any number of slides - and the compute units of the other loops stay the projector's
        # (16 slides: 240 -> 254 units, 52.5 -> [DESIGN 6] M patches/s).
        loops = self.feature_loops(B)
        plan._refresh()
        fused2 = vq.dtype == torch.float32         # (bf16 logits: a launch of their own, plain statistics and publication)
        xf, ef, lf = patches.view(B * N, -1), emb_buf.view(B * N, -1), logits.view(1, B * N, R)
        streamed = (not net.use_pos and fused2 and _env_on("IPSX_CAM_STREAM") and (B == 1 or N % 32 == 0)
                    and plan.stream_supported(B * N, R))
        # (candidate sets beyond the LDS - the shipped M = I = 5000 - run as a TEAM of workgroups per slide, csrc/scan_large_team.h:
        #  each of them keeps a compute unit)
        team = hip.scan_workgroups_per_image(B, M, I, ca.H, ca.n_token)
        # (a shuffle index rides inside the library's one call, which composes its own flat index, under IPSX_NATIVE_ORDER=1;
        #  by default such a call stays on the launches one by one: the one call measured no faster)
        ordered = self._order is not None
        if streamed and patches.dtype == torch.float32 and (not ordered or _native_order_on()) and self.native_ok(patches, None):
            free = hip.device_geometry(dev).cus - loops * team
            wgs = int(os.environ.get("IPSX_CAM_WGS", "0")) or free
            # (a team's iteration is ~55 us and the last TWO of them run behind the producer - the rows of the last chunk all
            #  complete in its last round - so a finer end of the stream pays: the last 2 x workgroups units as 32-row tiles,
            #  38,000 rows at M = I = 5000: 39.3 -> 39.6 M patches/s)
            short = int(os.environ.get("IPSX_CAM_SHORT", "0")) or ((-19 if team > 1 else -11) if B == 1 else -1)
            return self.native_call("features", patches, None, logits, mem_idx_buf, zeroed, emb_buf, scan_ws, loops, wgs,
                                    short_first=short)
        fidx = self._flat.view(-1) if ordered else None       # (composed here: in front of the loop's launch)
        with _no_gc_pause():                       # from the loop's launch to its producers': no host stall
            tie, ready, status, ctl = self.persistent_begin(logits, mem_idx_buf, zeroed, B, dev, loops, scan_ws,
                                                            zero_words=2 * B + 1 + plan.stream_ctl_zero_words(B * N))
            if streamed:
                # one workgroup per compute unit the loops leave free (with dynamic pulls one that is placed late just starts
                # late).  Round 4: the loop (3.7 us per iteration) is no longer the bound of a lone slide, the projector is:
                # 64-row tiles at full rate, the last round handed out as 32-row tiles and what is left over then as column
                # quarters, so that the launch ends evenly (short_first = -11: half the workgroups start with a 32-row tile, one round of single units;
                # M patches/s per slide synced / back to back: all tiles 32 rows 39.9 / 41.1, this 41.6 / 43.4; without the
                # quarters the leftover 8-16 units were a round of their own: stream 1.38 -> 1.30 ms)
                free = hip.device_geometry(dev).cus - loops * team
                wgs = int(os.environ.get("IPSX_CAM_WGS", "0")) or free
                short = int(os.environ.get("IPSX_CAM_SHORT", "0")) or (-11 if B == 1 else -1)
                plan.stream(xf, vq, R, ef, logits.view(B * N, R), ctl, ready, workgroups=wgs, slide_rows=N, short_first=short,
                            index=fidx)
                # (whatever two simultaneous finishers leave to each other is published by the last workgroup out: round 5 -
                #  it was one publish_rows launch per slide behind the stream)
            else:
                its = self.feature_parts(loops * team, N, dev, True)
                edges = [0] + [min(N, M + it * I) for it in its[1:]]
                edges[-1] = N
                launches = self.feature_launches(B, N, edges, dev, loops * team)
                # (through a shuffle index the launches read the whole tensor xf through their rows of the index)
                src_of = (lambda r0, r1: (xf, fidx[r0:r1])) if fidx is not None else (lambda r0, r1: (xf[r0:r1], None))
                if fused2:
                    x0, i0 = src_of(launches[0][0], launches[0][1])
                    plan.row_stats(x0, out=stats[launches[0][0]:launches[0][1]], index=i0)
                published = None                       # (slide, rows) whose publication rides on the next GEMM launch
                for n_step, (r0, r1, pubs) in enumerate(launches):
                    xk, ik = src_of(r0, r1)
                    if not fused2:
                        plan.row_stats(xk, out=stats[r0:r1], index=ik)
                    emb = plan.encode(xk, stats=stats[r0:r1], out=ef[r0:r1], index=ik,
                                      publish=(ready[published[0]:published[0] + 1], published[1]) if published else None)
                    published = None
                    emb = emb.view(1, r1 - r0, -1)
                    pos = pos_enc[r0 // N:r0 // N + 1, r0 % N:r0 % N + (r1 - r0)] if net.use_pos else None
                    nxt = launches[n_step + 1] if n_step + 1 < len(launches) else None
                    if fused2 and nxt is not None:
                        if fidx is not None:           # the next part's moments as a launch of their own, through the index
                            hip.logits(emb, pos, vq, R, out=lf[:, r0:r1])
                            plan.row_stats(xf, out=stats[nxt[0]:nxt[1]], index=fidx[nxt[0]:nxt[1]])
                        else:
                            hip.logits_stats(emb, pos, vq, R, lf[:, r0:r1], xf[nxt[0]:nxt[1]], stats[nxt[0]:nxt[1]], plan.ln_eps)
                        for b_, rows in pubs[:-1]:     # (a launch across a slide's end: the finished slide is published at once)
                            hip.publish_rows(ready[b_:b_ + 1], rows)
                        published = pubs[-1]
                    else:
                        hip.logits(emb, pos, vq, R, out=lf[:, r0:r1])
                        for b_, rows in pubs:          # after the kernels that wrote those rows
                            hip.publish_rows(ready[b_:b_ + 1], rows)
        net._emb_parts = [emb_buf]
        return self.persistent_end(logits, mem_idx_buf, tie, status, n_iter, dev, scan_ws)

    # ------------------------------------------------------------------ pipeline: one image, persistent trunk stream
    def image_stream(self, patches, pos_enc):
        """One image (the reference's eager-sequential mode, B_seq = 1): the loop is resident on a compute unit of its own;
        the trunk's workgroups - one per remaining unit - pull four, later two patches at a time, encode them, compute their
        logits and publish them (ipsx_trunk_stream).  No parts, no launch between trunk and logits, no loop workgroup looking
        for a free unit beside a trunk launch; what is exposed of the loop is the iteration after the last patch."""
        net, plan = self.net, self.plan()
        N = patches.shape[1]
        M, I, dev = net.M, net.I, patches.device
        ca = net.transf.crs_attn
        vq, R = ca.folded_query(), ca.H * ca.n_token
        self.streams(dev)
        logits, mem_idx_buf, emb_buf, zeroed = self.buffers(
            "image", (N, M, I, R, net.D, str(dev)),
            lambda: (torch.empty((1, N, R), dtype=torch.float32, device=dev),
                     torch.empty((1, M), dtype=torch.int64, device=dev),
                     torch.empty((1, N, net.D), dtype=torch.float32, device=dev),
                     torch.zeros((3 + plan.image_stream_ctl_words(N),), dtype=torch.int32, device=dev)))
        ordered = self._order is not None           # (a shuffle index: the tiles read patch index[j] where they read patch j)
        if patches.dtype == torch.float32 and self.native_ok(patches, pos_enc if net.use_pos else None):
            tp = (pos_enc[0] if pos_enc[0].is_contiguous() else pos_enc[0].contiguous()) if net.use_pos else None
            return self.native_call("image", patches, pos_enc if net.use_pos else None, logits, mem_idx_buf, zeroed, emb_buf, None, 0, 0,
                                    trunk_pos=tp, quad_pulls=-1)
        fidx = self._flat.view(-1) if ordered else None       # (composed here: in front of the loop's launch)
        with _no_gc_pause():                       # from the loop's launch to its producer's: no host stall
            tie, ready, status, ctl = self.persistent_begin(logits, mem_idx_buf, zeroed, 1, dev)
            plan.image_stream(patches[0], pos_enc[0] if net.use_pos else None, vq, R, emb_buf[0], logits[0], ctl, ready,
                              index=fidx)
        # (whatever two simultaneous finishers leave to each other is published by the last workgroup out: no launch for it)
        net._emb_parts = [emb_buf]
        return self.persistent_end(logits, mem_idx_buf, tie, status, self.n_iter(N), dev)

    # ------------------------------------------------------------------ the parts' index lists
    @staticmethod
    def part_lists(B, N, edges, dev):
        """int32 patch numbers b * N + j of every part: part k is rows edges[k] .. edges[k + 1] of every image, image-major."""
        rows = torch.arange(B, device=dev, dtype=torch.int32).unsqueeze(1) * N
        return [(rows + torch.arange(edges[k], edges[k + 1], device=dev, dtype=torch.int32)).reshape(-1)
                for k in range(len(edges) - 1)]

    @staticmethod
    def part_map(B, N, edges, dev):
        """Where the parts' lists lie in a flat (B, N) index: part k's (B, rows) block, one after the other."""
        pos = torch.arange(B * N, device=dev).view(B, N)
        return torch.cat([pos[:, edges[k]:edges[k + 1]].reshape(-1) for k in range(len(edges) - 1)])

    @staticmethod
    def part_ends(B, edges):
        """Exclusive prefix ends of the parts in entries of the joined list."""
        return [B * e for e in edges[1:]]

    def one_launch_ok(self, src, fused, small, vq, P):
        """Every part of the call as ONE launch of the fused fp32 trunk (``ipsx_trunk_encode_parts`` and its ``_u8`` /
        ``_view`` / ``_view_u8`` twins), the parts' logits and iterations let go by wait kernels on the side stream: the
        exact fp32 trunk (a view's lists serve layered trunks too) on float32 patches or images, or - under
        ``IPSX_ONE_LAUNCH_U8=1`` (``ONE_LAUNCH_U8_DEFAULT``) - on uint8 ones with their table (``hip.PatchSource`` has checked
        it), cut by the loop's chunk boundaries (not the small-batch split), where kernels of different streams have been
        SEEN to run side by side."""
        if src is not None and src.dtype == torch.uint8 and os.environ.get("IPSX_ONE_LAUNCH_U8", ONE_LAUNCH_U8_DEFAULT) == "0":
            return False
        return (src is not None and fused and not small and 2 <= P <= 16 and src.dtype in (torch.float32, torch.uint8)
                and hip.precision() == "fp32"
                and vq.dtype == torch.float32 and src.count < (1 << 31) - 16
                and _env_on("IPSX_ONE_LAUNCH") and hip.persistent_ok(src.device))

    @staticmethod
    def one_launch_dedup(src):
        """Exact blank-patch dedup inside the counted launch of ``parts_one_launch``: with ``IPSX_DEDUP_BLANK`` unset (or
        ``auto``), for every source that route takes - float32 or uint8 patches, a view of float32 or uint8 images (a blank
        byte patch is all bytes 0: ``EncoderPlan.blank_embedding``).  ``0``: nowhere; ``1``: the explicit route's business
        (``hip.dedup_blank``), which this route is not.  A function of the source's kind and the environment only."""
        return (hip.dedup_auto() and src.dtype in (torch.float32, torch.uint8)
                and (src.table is not None) == (src.dtype == torch.uint8))

    def parts_one_launch(self, src, every, edges, its, pos_enc, vq, R):
        """``parts_with_ranges`` without the trunk's launch boundaries: ``every`` is the parts' index lists
        joined.  The trunk launch goes to the main stream FIRST - a runtime that runs the two streams one after the other
        then finds every counter full - and for each part but the last the side stream gets a wait on the part's counter,
        the part's logits and its iterations.  A wait that gave up (no progress for hip.persistent_wait_ms) sets the status
        word; the conditional launches at the end then redo the early parts' logits and the whole loop in this call, and
        the host, which reads the word one call later, counts the event as the persistent pipelines do.
        At ``scan_mnist_kernel``'s shape (``scan_logits_ok``) what follows the trunk launch is ``parts_loop_logits`` instead:
        the same launches per part, the redo inside the last part's launch, the end of the call in one launch."""
        net, plan = self.net, self.plan()
        N = edges[-1]
        B = every.numel() // N
        M, I, dev = net.M, net.I, src.device
        ca = net.transf.crs_attn
        P = len(its) - 1
        hip._PERSIST_CALLS += 1                    # (the window of hip.persistent_timed_out is counted in such calls)
        self.check_strike(dev)
        side, main = self.streams(dev)
        logits, mem_idx_buf, words, scan_ws = self.buffers(
            "parts1", (B, N, M, I, R, P, str(dev)),
            lambda: (torch.empty((B, N, R), dtype=torch.float32, device=dev),
                     torch.empty((B, M), dtype=torch.int64, device=dev),
                     torch.zeros((-(-(2 * B + P + 1) // 4) * 4,), dtype=torch.int32, device=dev),   # tie flags | counters | status | gate
                     hip.scan_workspace(B, M, I, ca.H, ca.n_token, dev)))
        tie, done, status, gate = words[:B], words[B:B + P], words[B + P:B + P + 1], words[B + P + 1:2 * B + P + 1]
        if self._side_pending is not None:
            # the last call's final launch did not wait for the side stream (``parts_loop_logits``: a device-side gate instead):
            # its side-stream kernels come in front of this fill.  They are long done when the caller has synchronised in
            # between - the host sees that, and no hand-over between the two queues (measured: 20 - 30 us in front of the fill)
            # is enqueued; calls back to back wait for the event, beside the last call's end
            if not self._side_pending.query():
                main.wait_event(self._side_pending)
            self._side_pending = None
        words.zero_()
        zeroed = torch.cuda.Event()
        zeroed.record(main)
        ends = self.part_ends(B, edges)
        # blank entries are found, written and counted in front of the trunk launch, which encodes the others only (same
        # bits; the waits below see done[k] fill as before)
        emb_all = plan.encode_source(src, index=every, parts=(ends, done), dedup=self.one_launch_dedup(src))
        emb_all.record_stream(side)
        starts = [0] + ends[:-1]
        net._emb_parts = parts = [emb_all[starts[k]:ends[k]].view(B, edges[k + 1] - edges[k], -1) for k in range(P)]
        if self.scan_logits_ok(vq, M, I, ca, net.D):
            return self.parts_loop_logits(src, parts, its, pos_enc if net.use_pos else None, vq, logits, mem_idx_buf, tie, done, status,
                                          [ends[k] - starts[k] for k in range(P)], zeroed, scan_ws, gate)
        pos = [pos_enc[:, edges[k]:edges[k + 1]] if net.use_pos else None for k in range(P)]
        with torch.cuda.stream(side):
            side.wait_event(zeroed)                # (previous readers of the buffers are done, the counters are zero)
            for k in range(P - 1):
                hip.part_wait(done[k:k + 1], ends[k] - starts[k], status)
                hip.logits(parts[k], pos[k], vq, R, out=logits[:, edges[k]:edges[k + 1]])
                hip.scan_range(logits, M, I, ca.H, ca.n_token, its[k], its[k + 1], mem_idx_buf, tie, scan_ws)
        main.wait_stream(side)
        k = P - 1
        hip.logits(parts[k], pos[k], vq, R, out=logits[:, edges[k]:edges[k + 1]])
        hip.scan_range(logits, M, I, ca.H, ca.n_token, its[k], its[k + 1], mem_idx_buf, tie, scan_ws)
        # recovery, no-ops unless a wait gave up: behind the trunk launch every embedding is there
        for k in range(P - 1):
            hip.logits(parts[k], pos[k], vq, R, out=logits[:, edges[k]:edges[k + 1]], cond=status)
        hip.scan_range_if(logits, M, I, ca.H, ca.n_token, 0, its[P], mem_idx_buf, tie, status, 1, workspace=scan_ws)
        self._mirror_pending = status              # (copied to the host by after_call: behind the call's gathers)
        hip.scan.last_tie = tie
        return mem_idx_buf.clone()                 # the buffer is overwritten by the next call

    @staticmethod
    def scan_logits_ok(vq, M, I, ca, D):
        """The counted route without logits launches (``parts_loop_logits``): ``scan_mnist_kernel``'s shape on float32 logits,
        embeddings of whole 8-float groups, and not switched off (``hip.dbg_scan_logits``, ``IPSX_SCAN_LOGITS=0``)."""
        return (vq.dtype == torch.float32 and D % 8 == 0 and hip.scan_mnist_shape(M, I, ca.H, ca.n_token) and hip.scan_logits_on())

    def parts_loop_logits(self, src, parts, its, pos, vq, logits, mem_idx_buf, tie, done, status, counts, zeroed, scan_ws=None, gate=None):
        """What ``parts_one_launch`` enqueues behind the trunk launch at ``scan_mnist_kernel``'s shape: per part
        a wait, the part's logits and its iterations on the side stream, as before - a part of at most ``SCAN_LOGITS_ROWS``
        rows per image without a logits launch: workgroup b of the loop's launch writes image b's logits of the part itself
        (``hip.LogitsParts.scan_range``).  The last part's launch, on the main stream, takes the status word: clear, it does the
        last part; set by a wait that gave up, every workgroup recomputes every row of its image and runs the whole loop -
        the redo of the call, in the launch that was due anyway, so no launch does nothing on the clean path.  The call's
        end is ``finish``'s one launch where ``IPSNet._call`` asks for it and the patches are a tensor it takes."""
        net = self.net
        M, I = net.M, net.I
        ca = net.transf.crs_attn
        P = len(its) - 1
        side, main = self.streams(logits.device)
        table = hip.LogitsParts(parts)
        limit = self.SCAN_LOGITS_ROWS
        R = ca.H * ca.n_token

        def part(k, redo=None, publish=None):
            if table.rows[k] <= limit:
                table.scan_range(logits, M, I, ca.H, ca.n_token, its[k], its[k + 1], mem_idx_buf, tie, k, k + 1, pos, vq, redo=redo,
                                 gate_publish=publish)
                return
            # a long part: its logits on the whole device, then the loop's launch - the plain one (the kernels of the chain
            # this replaces), or, where it carries the redo, the prologue's instance with no rows of its own
            lo = table.first[k]
            hip.logits(parts[k], pos[:, lo:lo + table.rows[k]] if pos is not None else None, vq, R, out=logits[:, lo:lo + table.rows[k]])
            if redo is None and publish is None:
                hip.scan_range(logits, M, I, ca.H, ca.n_token, its[k], its[k + 1], mem_idx_buf, tie, scan_ws)
            else:
                table.scan_range(logits, M, I, ca.H, ca.n_token, its[k], its[k + 1], mem_idx_buf, tie, k + 1, k + 1, pos, vq, redo=redo,
                                 gate_publish=publish)

        k_tail = P
        if gate is not None and self.scan_tail_on(logits.shape[0] * logits.shape[1], logits.device):
            k_tail = self.tail_parts(table.rows, int(os.environ.get("IPSX_SCAN_TAIL_ROWS", SCAN_TAIL_ROWS_DEFAULT)))
        with torch.cuda.stream(side):
            side.wait_event(zeroed)                # (previous readers of the buffers are done, the counters are zero)
            for k in range(min(k_tail, P - 1)):
                hip.part_wait(done[k:k + 1], counts[k], status)
                part(k, publish=gate if k == k_tail - 1 else None)
        result = mem_idx_buf
        if k_tail < P:
            # The trailing parts [k_tail, P) as ONE launch directly behind the trunk's, no stream wait in front of it (enqueued
            # AFTER the side stream's launches all the same: a runtime that runs kernels in submission order meets the side's
            # work first): rows first - every embedding is there behind the trunk -, then the device-side gate lets the
            # iterations go when image b's side-stream loop has published its[k_tail], and the result goes to a buffer of its
            # own.  The next call's fill is ordered behind this call's side-stream kernels in ``parts_one_launch``.
            result = self.buffers("parts1_out", (tuple(mem_idx_buf.shape), str(mem_idx_buf.device)), lambda: (torch.empty_like(mem_idx_buf),))[0]
            table.scan_range(logits, M, I, ca.H, ca.n_token, its[k_tail], its[P], mem_idx_buf, tie, k_tail, P, pos, vq, redo=status,
                             gate=gate, status=status, out=result)
            if self._side_event is None:
                self._side_event = torch.cuda.Event()
            self._side_event.record(side)
            self._side_pending = self._side_event
        else:
            main.wait_stream(side)
            # behind the trunk launch every embedding is there: what the redo reads
            part(P - 1, redo=status)
        self._mirror_pending = status              # (copied to the host by finish's launch, or by after_call behind the gathers)
        hip.scan.last_tie = tie
        # (whole images: the patches are gathered through the view; a caller that does not end in ``finish`` / ``take_unfinished``
        #  - dist.py - gets its own copy, as before)
        if src.is_view or not self.caller_finishes:
            return result.clone()
        self._unfinished = result                  # ``finish`` - one launch - or ``take_unfinished`` + the gathers is the caller's next step
        return result

    def scan_tail_on(self, patches, dev):
        """The gated last launch of ``parts_loop_logits``: ``IPSX_SCAN_TAIL=0`` nowhere, ``=1`` on every call of the route, unset
        on calls of at least ``small_batch_limit`` patches.  That is every image batch the route gets by itself - a smaller
        one comes here only with 100 iterations or more per image (not measured with the gate), or from a test that lifts the
        limit to look at the route's launches one by one (tests/test_scan_logits.py counts them).  The limit is written out
        below and NOT asked of ``small_batch_limit``, deliberately and in this one place: that test lifts the method itself,
        and the launches it counts are the chain's."""
        mode = os.environ.get("IPSX_SCAN_TAIL", "auto")
        return mode != "0" and (mode == "1" or patches >= 16 * self.round_patches(dev))

    @staticmethod
    def tail_parts(rows, limit):
        """``k_tail`` of ``parts_loop_logits``: the first part such that the parts ``k_tail .. P - 1`` together hold at most
        ``limit`` rows per image - those go into the call's last launch.  At least one part stays on the side stream (there
        is nothing to gate on otherwise); ``P``: no trailing part fits, the chain as it was."""
        P, k, held = len(rows), len(rows), 0
        while k > 1 and held + rows[k - 1] <= limit:
            k -= 1
            held += rows[k]
        return k

    # ------------------------------------------------------------------ pipeline: parts, the loop in ranges beside them
    def parts_with_ranges(self, patches, pos_enc):
        """The patch axis in parts cut at chunk boundaries; part k is encoded (the fused trunk through an index list -
        nothing is copied - every other encoder through a slice) and scored, and the loop iterations that part makes
        possible run on the side stream (ipsx_scan_range resumes from the memory indices) while the encoder is already
        working on part k + 1.  Only the last part's iterations are exposed - what keeps the loop off the critical path when
        the image (and with it the iteration count) grows across GPUs.  Image encoders: parts shrinking towards the end;
        a small batch: small_batch_split; feature inputs without persistent loops: equal parts."""
        net, plan = self.net, self.plan()
        B, N = patches.shape[:2]
        M, I, dev = net.M, net.I, patches.device
        ca = net.transf.crs_attn
        vq, R = ca.folded_query(), ca.H * ca.n_token
        n_iter = self.n_iter(N)
        from .dist import part_iterations
        # parts as index lists into the call's source: the fused trunk, and - whole images - every encoder that reads a view
        src = self.source(patches)
        fused = src is not None and bool(plan.fused(src.shape))
        indexed = fused or (src is not None and src.is_view)
        edges, small = None, False
        if net.is_image and B * N < self.small_batch_limit(dev) and n_iter < 100:
            edges, its = self.small_batch_split(B, N, dev)
            small = True
        elif net.is_image and indexed and hip.precision() == "bf16":
            # the bf16 trunk's workgroups take EIGHT patches (fused_trunk_bf16.h): a round is 16 patches per unit, and the
            # fixed 50 / 30 / 15 / 5 % cut of a 40,000-patch batch is 12 rounds of work for 9.8 - every part a whole number of
            # rounds instead (dist.plan_iterations: the sharded path's planner, one rank)
            from .dist import launch_model, plan_iterations
            its = plan_iterations(N, M, I, 1, B, launch_model(net, tuple(patches.shape[2:]), hip.device_geometry(dev).cus),
                                  self.OVERLAP_PARTS)
        elif net.is_image:
            its = part_iterations(n_iter, self.OVERLAP_PARTS)
        else:
            its = self.feature_parts(B, N, dev, False)
        P = len(its) - 1
        if edges is None:                                      # parts cut at the loop's chunk boundaries
            edges = [0] + [min(N, M + it * I) for it in its[1:]]
            edges[-1] = N
        key = (B, N, tuple(edges), str(dev))
        if indexed and (self._part_index is None or self._part_index[0] != key):      # int32 patch indices of every part, cached
            lists = self.part_lists(B, N, edges, dev)
            self._part_index = (key, lists, torch.cat(lists))                         # (and joined: the one-launch route)
        side, main = self.streams(dev)
        flat = patches.reshape(B * N, *patches.shape[2:]) if self._flat is not None and not indexed else None   # (feature rows)
        part_index = self._part_index[1] if indexed else None
        every = self._part_index[2] if indexed else None
        if self._flat is not None:
            # a shuffle index: composed into the parts' index lists, per call, by ONE gather (the map - part k's (B, rows)
            # block of the (B, N) index, one after the other - is kept with the parts)
            if self._part_map is None or self._part_map[0] != key:
                self._part_map = (key, self.part_map(B, N, edges, dev))
            every = torch.index_select(self._flat.reshape(-1), 0, self._part_map[1])
            part_index = [every[B * edges[k]:B * edges[k + 1]] for k in range(P)]
        if self.one_launch_ok(src, fused, small, vq, P):
            return self.parts_one_launch(src, every, edges, its, pos_enc, vq, R)
        logits, mem_idx_buf, tie, scan_ws = self.buffers(
            "parts", (B, N, M, I, R, str(dev)),
            lambda: (torch.empty((B, N, R), dtype=torch.float32, device=dev),
                     torch.empty((B, M), dtype=torch.int64, device=dev),
                     torch.zeros((B,), dtype=torch.int32, device=dev),
                     hip.scan_workspace(B, M, I, ca.H, ca.n_token, dev)))   # None unless M + I exceeds the LDS
        tie.zero_()
        net._emb_parts = parts = []
        side.wait_stream(main)
        for k in range(P):
            lo, hi = edges[k], edges[k + 1]
            if indexed:
                emb = plan.encode_source(src, index=part_index[k]).view(B, hi - lo, -1)
            elif self._flat is not None:           # feature rows through the shuffle index
                emb = plan.encode(flat, index=part_index[k]).view(B, hi - lo, -1)
            else:
                emb = net._embed(patches[:, lo:hi].reshape(-1, *patches.shape[2:])).view(B, hi - lo, -1)
            parts.append(emb)
            pos = pos_enc[:, lo:hi] if net.use_pos else None
            if k == P - 1:
                # the last part has nothing to run beside: its logits and iterations stay on the main stream (one
                # cross-stream hand-over less on the critical path; it only has to follow the side stream's earlier parts)
                main.wait_stream(side)
                hip.logits(emb, pos, vq, R, out=logits[:, lo:hi])
                hip.scan_range(logits, M, I, ca.H, ca.n_token, its[k], its[k + 1], mem_idx_buf, tie, scan_ws)
                continue
            done = torch.cuda.Event()
            done.record(main)
            emb.record_stream(side)
            with torch.cuda.stream(side):
                side.wait_event(done)
                hip.logits(emb, pos, vq, R, out=logits[:, lo:hi])
                hip.scan_range(logits, M, I, ca.H, ca.n_token, its[k], its[k + 1], mem_idx_buf, tie, scan_ws)
        main.wait_stream(side)
        hip.scan.last_tie = tie
        return mem_idx_buf.clone()                 # the buffer is overwritten by the next call

    # ------------------------------------------------------------------ pipeline: everything else (one piece, or lazy slabs)
    def slabs(self, patches, pos_enc):
        """Encode -> logits -> one scan; patches on the host (lazy loading, reference ips_net.py:204-206,223) arrive in a few
        large slabs on a copy stream while the previous slab is being encoded, and the loop runs on the side stream over the
        iterations whose rows have arrived - only the last slab's iterations are exposed."""
        net = self.net
        B, N = patches.shape[:2]
        M, I, dev = net.M, net.I, net.device
        ca = net.transf.crs_attn
        vq, R = ca.folded_query(), ca.H * ca.n_token
        logits = torch.empty((B, N, R), dtype=torch.float32, device=dev)
        viewed = not torch.is_tensor(patches)                    # a hip.PatchSource (select_view: whole images), one span
        if viewed or patches.is_cuda:
            spans, fetch, prefetch = [(0, N)], lambda k: patches, lambda k: None
        else:
            spans, fetch, prefetch = self.lazy_slabs(patches)
        n_iter = self.n_iter(N)
        beside = len(spans) > 1 and _env_on("IPSX_OVERLAP_SCAN") and not hip.dedup_blank()
        if beside:
            side, main = self.streams(dev)
            mem_idx = torch.empty((B, M), dtype=torch.int64, device=dev)
            tie = torch.zeros((B,), dtype=torch.int32, device=dev)
            scan_ws = hip.scan_workspace(B, M, I, ca.H, ca.n_token, dev)     # None unless M + I exceeds the LDS
            for t in (logits, mem_idx, tie) + ((scan_ws,) if scan_ws is not None else ()):
                t.record_stream(side)
            side.wait_stream(main)
            it_prev = 0
        parts = []
        for k, (lo, hi) in enumerate(spans):
            part = fetch(k)
            if viewed:                             # every grid patch, or those the shuffle index names
                emb = self.plan().encode_source(part, index=self._flat.reshape(-1) if self._flat is not None else None).view(B, N, -1)
            elif self._order is not None and net.is_image:       # (device-resident patches of a layered trunk, one span: the stem reads the list)
                emb = self.plan().encode_source(self.source(part), index=self._flat.view(-1)).view(B, N, -1)
            elif self._order is not None:          # (device-resident feature rows, one span) through the shuffle index
                emb = self.plan().encode(part.reshape(B * N, -1), index=self._flat.view(-1)).view(B, N, -1)
            else:
                emb = net._embed(part.reshape(-1, *patches.shape[2:])).view(B, hi - lo, -1)
            hip.logits(emb, pos_enc[:, lo:hi] if net.use_pos else None, vq, R, out=logits[:, lo:hi])
            prefetch(k + 1)          # after the encoder is enqueued: a pageable-memory copy blocks the host, not the GPU
            parts.append(emb)
            if beside:
                it_k = n_iter if hi >= N else max(it_prev, (hi - M) // I)
                if it_k > it_prev:
                    done = torch.cuda.Event()
                    done.record(main)
                    with torch.cuda.stream(side):
                        side.wait_event(done)
                        hip.scan_range(logits, M, I, ca.H, ca.n_token, it_prev, it_k, mem_idx, tie, scan_ws)
                    it_prev = it_k
        net._emb_parts = parts
        if beside:
            main.wait_stream(side)
            hip.scan.last_tie = tie
            return mem_idx
        return hip.scan(logits, M, I, ca.H, ca.n_token)

    def lazy_slabs(self, patches):
        """Host tensor -> (spans, fetch, prefetch): slab k travels on the copy stream while slab k - 1 is encoded.  The first
        slab is the only copy nothing hides, so the slabs GROW (1/6, 1/2, then full slabs of IPSX_LAZY_SLAB_MB: the copy
        engine moves patches ~3x faster than the fp32 encoder consumes them).  With 288 GB of HBM the slabs are kept (up to
        IPSX_LAZY_KEEP_MB, default 16 GiB) so that the M winners are gathered on the device; beyond that a two-slot ring is
        recycled and the final gather happens on the host exactly as in the reference."""
        net = self.net
        B, N = patches.shape[:2]
        row_bytes = patches[0, 0].numel() * patches.element_size()
        slab_bytes = int(os.environ.get("IPSX_LAZY_SLAB_MB", "0")) << 20 or self.LAZY_SLAB_BYTES
        per = max(1, min(N, slab_bytes // max(1, B * row_bytes)))
        spans, lo = [], 0
        for size in (max(1, per // 6), max(1, per // 2)):
            if N - lo > per:
                spans.append((lo, lo + size))
                lo += size
        spans += [(a, min(a + per, N)) for a in range(lo, N, per)]
        keep = patches.numel() * patches.element_size() <= int(os.environ.get("IPSX_LAZY_KEEP_MB", "16384")) << 20
        dev = net.device
        bufs = self.buffers("lazy", (keep, tuple(patches.shape), per, patches.dtype, str(dev)),
                            lambda: [torch.empty(patches.shape, dtype=patches.dtype, device=dev)] if keep else
                            [torch.empty((B, per) + tuple(patches.shape[2:]), dtype=patches.dtype, device=dev) for _ in range(2)])
        if keep:
            store = bufs[0]
            net._device_patches = store
            dst = lambda k, lo, hi: store[:, lo:hi]
        else:
            dst = lambda k, lo, hi: bufs[k % 2][:, :hi - lo]
        if self._copy is None or self._copy.device != torch.device(dev):
            self._copy = torch.cuda.Stream(device=dev)
        copy_stream, main = self._copy, torch.cuda.current_stream(dev)
        # the buffers come from the main stream's allocator pool: a block freed in Python a moment ago may still be read by
        # kernels queued on the main stream (the previous step's backward / optimizer), so the copy stream must not write
        # it before the main stream got that far - and the allocator must know the copy stream uses it
        copy_stream.wait_stream(main)
        for buf in bufs:
            buf.record_stream(copy_stream)
        ready, freed = {}, {}

        def issue(k):
            lo, hi = spans[k]
            with torch.cuda.stream(copy_stream):
                if not keep and k - 2 in freed:
                    copy_stream.wait_event(freed[k - 2])          # ring slot must have been consumed
                d = dst(k, lo, hi)
                for b in range(B):                                  # per image: contiguous on both sides
                    d[b].copy_(patches[b, lo:hi], non_blocking=True)
                ready[k] = torch.cuda.Event()
                ready[k].record(copy_stream)

        issue(0)

        def fetch(k):
            main.wait_event(ready[k])
            part = dst(k, *spans[k])
            if not keep:
                part = part.clone()
                freed[k] = torch.cuda.Event()
                freed[k].record(main)
            return part

        def prefetch(k):
            if k < len(spans):
                issue(k)                                            # travels while slab k-1 is being encoded

        return spans, fetch, prefetch
