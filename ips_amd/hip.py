"""ctypes binding of libipsx.so (include/ipsx.h) for torch tensors on a ROCm device.

PyTorch is plumbing here: it owns device memory and the stream; every function
below hands raw device pointers to the C ABI, which launches the hand-written
gfx950 kernels of ips_amd/csrc on ``torch.cuda.current_stream()``.

There is NO fallback in this module: if the shared library cannot be loaded, or a
call returns an error code, a RuntimeError is raised.  ``IPSX_BACKEND=aten``
(explicit opt-out, e.g. to time stock PyTorch-ROCm ops on the same GPU) makes
``on_device`` report False so callers keep to ATen; the default is ``hip``.
"""

import collections
import ctypes as C
import operator
import os
import subprocess

import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_PKG, "lib", "libipsx.so")
_LIB = None

f32p = C.c_void_p  # device pointers travel as integers
ABI_MAJOR = 3       # include/ipsx.h IPSX_VERSION / 100: the signatures in _EXPORTS below are those of this major version


def backend():
    b = os.environ.get("IPSX_BACKEND", "hip").lower()
    if b not in ("hip", "aten"):
        raise ValueError("IPSX_BACKEND must be 'hip' or 'aten', got {!r}".format(b))
    return b


def precision():
    """'fp32' (default: exact, reference parity), 'fp32x3' (every fp32 operand of the residual stages split exactly
    into three bf16 terms, six products on the bf16 matrix pipe, fp32 accumulation: fp32-grade accuracy but not
    bit-identical to the fp32 kernel) or 'bf16' (bf16 operands with fp32 accumulation; no reference behaviour
    to match).  'fp32x3' exists for the fused 1x32x32 trunk only.  'bf16' runs on every image encoder: the fused trunk
    for 1x32x32 patches, and for every other trunk the stem and max-pool in fp32, then bf16 activations in memory and
    every convolution on the bf16 matrix pipe ("bf16 layered trunk").  A feature net under 'bf16' runs its projector on the
    bf16 matrix pipe too (rows centred in fp32, then rounded) and reads feature rows stored as float16 /
    bfloat16; under 'fp32x3' it keeps the fp32 projector and float32 features."""
    p = os.environ.get("IPSX_PRECISION", "fp32").lower()
    if p not in ("fp32", "fp32x3", "bf16"):
        raise ValueError("IPSX_PRECISION must be 'fp32', 'fp32x3' or 'bf16', got {!r}".format(p))
    return p


_TIE_MODES = {"canonical": 0, "torch": 1, "torch_all": 2}


def tie_order():
    """How equal scores are ordered (``IPSX_TIE_ORDER``).
    'torch' (default): the order torch.topk returns on CPU (the reference's), replayed on the device - in the selection
    loops only where the tie is between bit-IDENTICAL candidates (duplicated patches: they tie in the reference's own
    arithmetic too); two different candidates whose scores collide in the last bit of this arithmetic keep the canonical
    order (in the reference's arithmetic they are an ulp apart: a replay reproduces nothing of it, and costs 100+ us per
    iteration at 10,000 candidates).  ``ipsx_topm`` - scores only - replays on every tie.
    'torch_all': replay wherever scores tie (rounds 1-4).  'canonical': earlier candidate position first, never a replay."""
    t = os.environ.get("IPSX_TIE_ORDER", "torch").lower()
    if t not in _TIE_MODES:
        raise ValueError("IPSX_TIE_ORDER must be 'torch', 'torch_all' or 'canonical', got {!r}".format(t))
    return t


def set_tie_order(mode):
    """Switch the tie order at run time ('torch' | 'torch_all' | 'canonical'); returns the previous one."""
    prev = lib().ipsx_set_tie_order(_TIE_MODES[mode])
    return {v: k for k, v in _TIE_MODES.items()}[prev]


def dedup_blank():
    """The explicit exact blank-patch deduplication in front of the fused encoder (IPSX_DEDUP_BLANK=1): every image-encoder
    call through ``ipsx_trunk_encode_dedup``, and the routes that cannot take it refuse."""
    return os.environ.get("IPSX_DEDUP_BLANK") == "1"


def dedup_auto():
    """IPSX_DEDUP_BLANK unset (or ``auto``): exact blank-patch dedup inside the one counted launch, wherever that route runs -
    float32 or uint8 patches, float32 or uint8 images (``selection.parts_one_launch``, ``ipsx_trunk_encode_parts_dedup`` and
    its ``_u8`` / ``_view`` / ``_view_u8`` twins), and in the packed encoder pass of ``ips_image_ragged`` on the fused trunk
    (``ragged_image.ragged_dedup``, ``ipsx_trunk_encode_ragged_view_dedup``, uint8 images: ``_dedup_u8``); every other route runs as under ``0`` and
    refuses nothing.  ``0``: no dedup anywhere."""
    return os.environ.get("IPSX_DEDUP_BLANK", "auto") == "auto"


# Graph replays (training/graphed.py) update parameters and BatchNorm statistics without bumping tensor._version or
# changing storage pointers, so every cache keyed on (data_ptr, _version) also carries this counter; whoever mutates
# weights behind autograd's back calls weights_changed().
_WEIGHTS_GENERATION = 0


def weights_generation():
    return _WEIGHTS_GENERATION


def weights_changed():
    """Invalidate every packed-weight cache (EncoderPlan, folded query): call after a HIP-graph replay or any other
    update of parameters / buffers that bypasses ``_version``."""
    global _WEIGHTS_GENERATION
    _WEIGHTS_GENERATION += 1


def _optimizer_stepped(optimizer, args, kwargs):
    weights_changed()


# Not every in-place update bumps ``_version``: torch's FUSED optimizers (AdamW(fused=True), ...) move the parameters
# without touching it (checked: version 0 -> 0 across a step), so every optimizer step invalidates the packed weights.
# The hook is process-global in torch (there is no per-module form), so it is installed when the first IPSNet is BUILT
# (``IPSNet.__init__`` calls ``install_optimizer_hook``), not when this module is imported: a process that merely imports
# the package keeps its optimizers untouched.  (Manual updates through ``.data`` or raw pointers still need an explicit
# ``weights_changed()``.)
_HOOK_INSTALLED = False


def install_optimizer_hook():
    global _HOOK_INSTALLED
    if _HOOK_INSTALLED:
        return True
    try:
        from torch.optim.optimizer import register_optimizer_step_post_hook
    except ImportError:      # older torch: per-optimizer hooks only; ips_amd.training registers them itself
        return False
    register_optimizer_step_post_hook(_optimizer_stepped)
    _HOOK_INSTALLED = True
    return True


def on_device(x):
    """True when ``x`` (tensor / device / str) is a GPU and the HIP backend is selected."""
    if torch.is_tensor(x):
        dev = x.device
    else:
        dev = torch.device(x)
    return _gpu_device(dev) and backend() == "hip"


def _gpu_device(dev):
    """Is ``dev`` a GPU?  THE device test of ``on_device`` and of every wrapper's arguments (``_one_gpu``): a test without
    a GPU switches it here."""
    return dev.type == "cuda"


# ------------------------------------------------------------------ C structs
class Conv(C.Structure):
    _fields_ = [("c_in", C.c_int), ("c_out", C.c_int), ("kh", C.c_int), ("kw", C.c_int),
                ("stride", C.c_int), ("pad", C.c_int),
                ("w_packed", C.c_void_p), ("alpha", C.c_void_p), ("shift", C.c_void_p),
                ("w_packed_bf16", C.c_void_p), ("colsum", C.c_void_p)]


class Block(C.Structure):
    _fields_ = [("n_conv", C.c_int), ("conv", Conv * 3), ("has_down", C.c_int), ("down", Conv)]


class Trunk(C.Structure):
    _fields_ = [("c_in", C.c_int), ("h", C.c_int), ("w", C.c_int), ("stem", Conv),
                ("n_block", C.c_int), ("blocks", C.POINTER(Block)), ("precision", C.c_int), ("patch_dtype", C.c_int)]


class PatchViewStruct(C.Structure):
    """``ipsx_patch_view``: float32 images (b, c, h, w) and the patch grid laid over them."""
    _fields_ = [("b", C.c_int), ("c", C.c_int), ("h", C.c_int), ("w", C.c_int),
                ("ph", C.c_int), ("pw", C.c_int), ("sh", C.c_int), ("sw", C.c_int)]


class ImageEntry(C.Structure):
    """``ipsx_image_entry``: one image of a ragged view - where it lies in the packed buffer, its first packed patch, its grid."""
    _fields_ = [("elem_off", C.c_int64), ("first", C.c_int64), ("h", C.c_int32), ("w", C.c_int32), ("ny", C.c_int32), ("nx", C.c_int32)]


class RaggedViewStruct(C.Structure):
    """``ipsx_ragged_view``: float32 images of different sizes in one packed buffer and the patch grids laid over them;
    ``images`` the table on the device, ``host`` the same table on the host."""
    _fields_ = [("b", C.c_int), ("c", C.c_int), ("ph", C.c_int), ("pw", C.c_int), ("sh", C.c_int), ("sw", C.c_int),
                ("images", C.c_void_p), ("host", C.POINTER(ImageEntry))]


class IpsCall(C.Structure):
    """include/ipsx.h ``ipsx_ips_call``: one ips() call with a resident loop, enqueued by ONE library call."""
    _fields_ = [("b", C.c_int), ("n", C.c_int64), ("m", C.c_int), ("i", C.c_int), ("h", C.c_int), ("n_token", C.c_int),
                ("logits", C.c_void_p), ("mem_idx", C.c_void_p), ("words", C.c_void_p), ("words_total", C.c_int64),
                ("loops", C.c_int), ("scan_workspace", C.c_void_p), ("scan_workspace_bytes", C.c_size_t),
                ("trunk", C.POINTER(Trunk)), ("pos", C.c_void_p), ("quad_pulls", C.c_int),
                ("lin", C.POINTER(Conv)), ("ln_eps", C.c_float), ("short_first", C.c_int),
                ("x", C.c_void_p), ("emb", C.c_void_p), ("v_packed", C.c_void_p), ("r", C.c_int), ("workgroups", C.c_int),
                ("src", C.c_void_p), ("src_row_bytes", C.c_int64), ("src_bstride_rows", C.c_int64),
                ("pos_table", C.c_void_p), ("pos_row_bytes", C.c_int64), ("pos_bstride_rows", C.c_int64),
                ("mem_patch", C.c_void_p), ("mem_pos", C.c_void_p), ("mem_idx_out", C.c_void_p), ("status_host", C.c_void_p),
                ("timing_slot", C.c_int), ("stream", C.c_void_p), ("side_stream", C.c_void_p)]


class IpsCallOrder(C.Structure):
    """include/ipsx.h ``ipsx_call_order``: the permutation an ``ipsx_ips_call_run_ordered`` selects through, and the
    workspace the call composes its flat row index in."""
    _fields_ = [("order", C.c_void_p), ("order_bstride", C.c_int64), ("index", C.c_void_p)]


class StreamTable(C.Structure):
    """include/ipsx.h ``ipsx_stream_table``: one table of a stream's state as ``ipsx_stream_commit`` moves it."""
    _fields_ = [("held", C.c_void_p), ("held_rows", C.c_int64), ("held_bstride_rows", C.c_int64),
                ("piece", C.c_void_p), ("piece_bstride_bytes", C.c_int64),
                ("dst", C.c_void_p), ("dst_rows", C.c_int64), ("dst_bstride_rows", C.c_int64), ("row_bytes", C.c_int64)]


class Transf(C.Structure):
    _fields_ = [("n_token", C.c_int), ("h", C.c_int), ("d", C.c_int), ("dk", C.c_int),
                ("dv", C.c_int), ("d_inner", C.c_int)] + \
               [(n, C.c_void_p) for n in ("q", "wq", "wk", "wv", "fc", "ln1_g", "ln1_b", "w1", "b1",
                                          "w2", "b2", "ln2_g", "ln2_b")] + \
               [("temperature", C.c_float), ("ln_eps", C.c_float)]


_EXPORTS = {
    # name: (restype, argtypes)
    "ipsx_version": (C.c_int, []),
    "ipsx_last_error": (C.c_char_p, []),
    "ipsx_device_count": (C.c_int, []),
    "ipsx_device_is_gfx950": (C.c_int, [C.c_int]),
    "ipsx_packed_conv_weight_elems": (C.c_size_t, [C.c_int] * 4),
    "ipsx_pack_conv_weight": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "ipsx_pack_conv_weight_strided": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                                C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "ipsx_pack_conv_weights_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "ipsx_packed_conv_weight_bf16_bytes": (C.c_size_t, [C.c_int] * 4),
    "ipsx_pack_conv_weight_bf16": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "ipsx_packed_conv_weight_tile16_elems": (C.c_size_t, [C.c_int] * 4),
    "ipsx_pack_conv_weight_tile16": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "ipsx_packed_conv_weight_x3_bytes": (C.c_size_t, [C.c_int] * 4),
    "ipsx_pack_conv_weight_x3": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "ipsx_packed_stem_weight_split_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "ipsx_pack_stem_weight_split": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "ipsx_bn_affine": (C.c_int, [C.c_void_p] * 5 + [C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ipsx_conv2d_affine": (C.c_int, [C.POINTER(Conv), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                     C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "ipsx_conv2d_affine_to_nhwc": (C.c_int, [C.POINTER(Conv), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                             C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "ipsx_conv2d_affine_nhwc": (C.c_int, [C.POINTER(Conv), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                          C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "ipsx_conv2d_affine_nhwc_bf16_supported": (C.c_int, [C.POINTER(Conv)]),
    "ipsx_conv2d_affine_nhwc_bf16": (C.c_int, [C.POINTER(Conv), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                               C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "ipsx_conv2d_lds_nhwc_supported": (C.c_int, [C.c_int] * 7),
    "ipsx_conv2d_lds_nhwc": (C.c_int, [C.POINTER(Conv), C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "ipsx_conv2d_lds_nhwc_stats_slabs": (C.c_int64, [C.c_int64]),
    "ipsx_conv2d_lds_nhwc_stats": (C.c_int, [C.POINTER(Conv), C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p,
                                             C.c_void_p, C.c_void_p]),
    "ipsx_bn_train_forward_partials": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p,
                                                 C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_int,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "ipsx_conv2d_dgrad_s2_lds_nhwc_supported": (C.c_int, [C.c_int] * 7),
    "ipsx_conv2d_dgrad_s2_lds_nhwc": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "ipsx_stem7x7s2_nhwc_supported": (C.c_int, [C.c_int] * 8),
    "ipsx_stem7x7s2_nhwc": (C.c_int, [C.POINTER(Conv), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ipsx_conv2d_wgrad_nhwc_supported": (C.c_int, [C.c_int] * 6),
    "ipsx_conv2d_wgrad_nhwc_workspace_bytes": (C.c_size_t, [C.c_int64] + [C.c_int] * 4),
    "ipsx_conv2d_wgrad_nhwc": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64] + [C.c_int] * 8 + [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ipsx_maxpool_3x3s2_nhwc": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "ipsx_maxpool_3x3s2_bwd_nhwc_supported": (C.c_int, [C.c_int] * 3),
    "ipsx_maxpool_3x3s2_bwd_nhwc": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "ipsx_avgpool_nhwc": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "ipsx_avgpool_nhwc_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "ipsx_maxpool_3x3s2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "ipsx_avgpool": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "ipsx_trunk_workspace_bytes": (C.c_size_t, [C.POINTER(Trunk), C.c_int64]),
    "ipsx_trunk_kernel": (C.c_char_p, [C.POINTER(Trunk)]),
    "ipsx_trunk_encode": (C.c_int, [C.POINTER(Trunk), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                    C.c_size_t, C.c_void_p]),
    "ipsx_patch_view_offset": (C.c_int64, [C.POINTER(PatchViewStruct), C.c_int64]),
    "ipsx_trunk_view_supported": (C.c_int, [C.POINTER(Trunk), C.POINTER(PatchViewStruct)]),
    "ipsx_trunk_encode_view": (C.c_int, [C.POINTER(Trunk), C.c_void_p, C.POINTER(PatchViewStruct), C.c_void_p, C.c_int64,
                                         C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ipsx_trunk_encode_parts_view": (C.c_int, [C.POINTER(Trunk), C.c_void_p, C.POINTER(PatchViewStruct), C.c_void_p, C.c_int64,
                                               C.c_void_p, C.POINTER(C.c_int64), C.c_int, C.c_void_p, C.c_void_p]),
    "ipsx_gather_patches_view": (C.c_int, [C.c_void_p, C.POINTER(PatchViewStruct), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "ipsx_trunk_encode_view_u8": (C.c_int, [C.POINTER(Trunk), C.c_void_p, C.c_void_p, C.POINTER(PatchViewStruct), C.c_void_p,
                                            C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ipsx_trunk_encode_parts_u8": (C.c_int, [C.POINTER(Trunk), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                             C.POINTER(C.c_int64), C.c_int, C.c_void_p, C.c_void_p]),
    "ipsx_trunk_encode_parts_view_u8": (C.c_int, [C.POINTER(Trunk), C.c_void_p, C.c_void_p, C.POINTER(PatchViewStruct), C.c_void_p,
                                                  C.c_int64, C.c_void_p, C.POINTER(C.c_int64), C.c_int, C.c_void_p, C.c_void_p]),
    "ipsx_gather_patches_view_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(PatchViewStruct), C.c_void_p, C.c_int, C.c_void_p,
                                              C.c_void_p]),
    "ipsx_trunk_dedup_workspace_bytes": (C.c_size_t, [C.POINTER(Trunk), C.c_int64]),
    "ipsx_trunk_encode_dedup": (C.c_int, [C.POINTER(Trunk), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                          C.c_size_t, C.c_void_p, C.c_void_p]),
    "ipsx_trunk_encode_dedup_flagged": (C.c_int, [C.POINTER(Trunk), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "ipsx_patchify_count": (C.c_int64, [C.c_int] * 6),
    "ipsx_patchify": (C.c_int, [C.c_void_p] + [C.c_int] * 8 + [C.c_void_p, C.c_void_p]),
    "ipsx_patchify_sparse": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_int] * 8 +
                             [C.c_void_p, C.c_void_p, C.c_void_p]),
    "ipsx_projector": (C.c_int, [C.POINTER(Conv), C.c_void_p, C.c_int64, C.c_float, C.c_void_p,
                                 C.c_void_p, C.c_size_t, C.c_void_p]),
    "ipsx_projector_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "ipsx_weight_colsum": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "ipsx_projector_stats": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "ipsx_projector_apply": (C.c_int, [C.POINTER(Conv), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ipsx_projector_apply_publish": (C.c_int, [C.POINTER(Conv), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_int32, C.c_void_p]),
    "ipsx_projector_stats_typed": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "ipsx_projector_bf16_supported": (C.c_int, [C.POINTER(Conv)]),
    "ipsx_projector_apply_bf16": (C.c_int, [C.POINTER(Conv), C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_int32, C.c_void_p]),
    "ipsx_projector_stats_indexed": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_float, C.c_void_p,
                                               C.c_void_p]),
    "ipsx_projector_apply_indexed": (C.c_int, [C.POINTER(Conv), C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_int32, C.c_void_p]),
    "ipsx_projector_apply_bf16_indexed": (C.c_int, [C.POINTER(Conv), C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "ipsx_projector_stream_indexed": (C.c_int, [C.POINTER(Conv), C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_float,
                                                C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                C.c_void_p]),
    "ipsx_trunk_stream_ctl_words": (C.c_size_t, [C.c_int64]),
    "ipsx_trunk_stream_supported": (C.c_int, [C.POINTER(Trunk), C.c_int, C.c_int]),
    "ipsx_trunk_stream": (C.c_int, [C.POINTER(Trunk), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "ipsx_projector_stream_ctl_words": (C.c_size_t, [C.c_int64]),
    "ipsx_projector_stream_ctl_zero_words": (C.c_size_t, [C.c_int64]),
    "ipsx_projector_stream_supported": (C.c_int, [C.POINTER(Conv), C.c_int64, C.c_int]),
    "ipsx_projector_stream": (C.c_int, [C.POINTER(Conv), C.c_void_p, C.c_int64, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_int,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "ipsx_logits_stats": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                    C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int64,
                                    C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "ipsx_query_proj": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_int,
                                  C.c_void_p, C.c_void_p]),
    "ipsx_folded_query_elems": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "ipsx_fold_query": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "ipsx_logits": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                              C.c_int, C.c_int64, C.c_int, C.c_int,
                              C.c_void_p, C.c_int64, C.c_void_p]),
    "ipsx_folded_query_bf16_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "ipsx_fold_query_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "ipsx_logits_bf16": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                   C.c_int, C.c_int64, C.c_int, C.c_int,
                                   C.c_void_p, C.c_int64, C.c_void_p]),
    "ipsx_set_tie_order": (C.c_int, [C.c_int]),
    "ipsx_scan": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ipsx_scan_workspace_bytes": (C.c_size_t, [C.c_int] * 5),
    "ipsx_scan_workgroups_per_image": (C.c_int, [C.c_int] * 5),
    "ipsx_scan_range": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ipsx_scan_range_strided": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64,
                                          C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ipsx_scan_ragged": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ipsx_stream_commit": (C.c_int, [C.POINTER(StreamTable), C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                     C.c_void_p]),
    "ipsx_stream_commit_view": (C.c_int, [C.POINTER(StreamTable), C.c_int, C.c_void_p, C.POINTER(PatchViewStruct), C.c_int,
                                          C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int64, C.POINTER(C.c_int), C.c_void_p]),
    "ipsx_scan_range_if": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "ipsx_scan_persistent_supported": (C.c_int, [C.c_int] * 4),
    "ipsx_scan_persistent_groupable": (C.c_int, [C.c_int] * 4),
    "ipsx_scan_persistent_on": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int,
                                          C.c_void_p]),
    "ipsx_scan_persistent_ws": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int,
                                          C.c_void_p, C.c_size_t, C.c_void_p]),
    "ipsx_scan_range_if_ws": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t,
                                        C.c_void_p]),
    "ipsx_scan_persistent": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "ipsx_publish_rows": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "ipsx_set_persistent_wait_ms": (C.c_int, [C.c_int]),
    "ipsx_scan_gate": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ipsx_trunk_encode_indexed": (C.c_int, [C.POINTER(Trunk), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "ipsx_trunk_encode_parts": (C.c_int, [C.POINTER(Trunk), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                          C.POINTER(C.c_int64), C.c_int, C.c_void_p, C.c_void_p]),
    "ipsx_trunk_parts_dedup_workspace_bytes": (C.c_size_t, [C.POINTER(Trunk), C.c_int64]),
    "ipsx_trunk_encode_parts_dedup": (C.c_int, [C.POINTER(Trunk), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                                C.POINTER(C.c_int64), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                                C.c_void_p, C.c_void_p]),
    "ipsx_trunk_encode_parts_dedup_u8": (C.c_int, [C.POINTER(Trunk), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                                   C.POINTER(C.c_int64), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                                   C.c_void_p, C.c_void_p]),
    "ipsx_trunk_encode_parts_dedup_view": (C.c_int, [C.POINTER(Trunk), C.c_void_p, C.POINTER(PatchViewStruct), C.c_void_p, C.c_int64,
                                                     C.c_void_p, C.POINTER(C.c_int64), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_size_t, C.c_void_p, C.c_void_p]),
    "ipsx_trunk_encode_parts_dedup_view_u8": (C.c_int, [C.POINTER(Trunk), C.c_void_p, C.c_void_p, C.POINTER(PatchViewStruct),
                                                        C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_int64), C.c_int, C.c_void_p,
                                                        C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "ipsx_part_wait": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "ipsx_scan_logits_check": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_int64]),
    "ipsx_scan_range_logits": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                         C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "ipsx_scan_range_logits_gate": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                              C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                              C.c_int32, C.c_void_p, C.c_void_p]),
    "ipsx_logits_if": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int,
                                 C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p]),
    "ipsx_trunk_encode_u8": (C.c_int, [C.POINTER(Trunk), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                       C.c_size_t, C.c_void_p]),
    "ipsx_trunk_encode_indexed_u8": (C.c_int, [C.POINTER(Trunk), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                               C.c_void_p]),
    "ipsx_dequant_patches": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "ipsx_scores_workspace_bytes": (C.c_size_t, [C.c_int] * 5),
    "ipsx_scores": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 6 +
                    [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ipsx_topm": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ipsx_topm_workspace_bytes": (C.c_size_t, [C.c_int] * 3),
    "ipsx_gather_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int,
                                   C.c_int64, C.c_int64, C.c_void_p]),
    "ipsx_ips_call_run": (C.c_int, [C.POINTER(IpsCall)]),
    "ipsx_ips_call_elapsed": (C.c_int, [C.c_int, C.POINTER(C.c_float)]),
    "ipsx_ips_call_run_ordered": (C.c_int, [C.POINTER(IpsCall), C.POINTER(IpsCallOrder)]),
    "ipsx_order_index": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]),
    "ipsx_trunk_stream_indexed": (C.c_int, [C.POINTER(Trunk), C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "ipsx_ips_finish": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int,
                                  C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ipsx_ips_finish_indexed": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                                          C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p]),
    "ipsx_ragged_finish": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                     C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ipsx_ragged_view_fill": (C.c_int64, [C.POINTER(ImageEntry)] + [C.c_int] * 6 + [C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                          C.POINTER(C.c_int64)]),
    "ipsx_ragged_view_offset": (C.c_int64, [C.POINTER(ImageEntry), C.c_int, C.POINTER(RaggedViewStruct), C.c_int64,
                                            C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "ipsx_trunk_ragged_view_supported": (C.c_int, [C.POINTER(Trunk), C.POINTER(RaggedViewStruct)]),
    "ipsx_trunk_encode_ragged_view": (C.c_int, [C.POINTER(Trunk), C.c_void_p, C.POINTER(RaggedViewStruct), C.c_void_p, C.c_int64,
                                                C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ipsx_ragged_finish_view": (C.c_int, [C.c_void_p, C.POINTER(RaggedViewStruct), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                          C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ipsx_ragged_view_blank_flags": (C.c_int, [C.c_void_p, C.POINTER(RaggedViewStruct), C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                                               C.c_void_p]),
    "ipsx_trunk_ragged_view_dedup_workspace_bytes": (C.c_size_t, [C.POINTER(Trunk), C.c_int64]),
    "ipsx_trunk_encode_ragged_view_dedup": (C.c_int, [C.POINTER(Trunk), C.c_void_p, C.POINTER(RaggedViewStruct), C.c_void_p, C.c_int64,
                                                      C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "ipsx_trunk_encode_ragged_view_u8": (C.c_int, [C.POINTER(Trunk), C.c_void_p, C.c_void_p, C.POINTER(RaggedViewStruct), C.c_void_p,
                                                   C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ipsx_ragged_finish_view_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(RaggedViewStruct), C.c_void_p, C.c_void_p, C.c_int,
                                             C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p]),
    "ipsx_ragged_view_blank_flags_u8": (C.c_int, [C.c_void_p, C.POINTER(RaggedViewStruct), C.c_void_p, C.c_int64, C.c_int64,
                                                  C.c_void_p, C.c_void_p]),
    "ipsx_trunk_encode_ragged_view_dedup_u8": (C.c_int, [C.POINTER(Trunk), C.c_void_p, C.c_void_p, C.POINTER(RaggedViewStruct),
                                                         C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t,
                                                         C.c_void_p, C.c_void_p]),
    "ipsx_scan_ragged_spans": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ipsx_stream_commit_ragged": (C.c_int, [C.POINTER(StreamTable), C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64,
                                            C.c_int64, C.c_void_p]),
    "ipsx_stream_commit_ragged_view": (C.c_int, [C.POINTER(StreamTable), C.c_int, C.c_void_p, C.POINTER(RaggedViewStruct), C.c_int,
                                                 C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int64, C.POINTER(C.c_int),
                                                 C.c_void_p]),
    "ipsx_aggregate_workspace_bytes": (C.c_size_t, [C.POINTER(Transf), C.c_int, C.c_int]),
    "ipsx_aggregate": (C.c_int, [C.POINTER(Transf), C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                 C.c_void_p, C.c_size_t, C.c_void_p]),
    "ipsx_aggregate_packed": (C.c_int, [C.POINTER(Transf), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                        C.c_void_p, C.c_size_t, C.c_void_p]),
    "ipsx_aggregate_counted": (C.c_int, [C.POINTER(Transf), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ipsx_head": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                            C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "ipsx_bn_train_supported": (C.c_int, [C.c_int64, C.c_int]),
    "ipsx_bn_train_workspace_floats": (C.c_size_t, [C.c_int64, C.c_int]),
    "ipsx_bn_train_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_int,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ipsx_bn_train_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "ipsx_projector_train_supported": (C.c_int, [C.c_int, C.c_int]),
    "ipsx_projector_train_slabs": (C.c_int64, [C.c_int64]),
    "ipsx_projector_train_forward": (C.c_int, [C.POINTER(Conv), C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p]),
    "ipsx_projector_wgrad_chunk_rows": (C.c_int64, []),
    "ipsx_projector_wgrad_max_rows": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "ipsx_projector_wgrad_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int]),
    "ipsx_projector_wgrad": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ipsx_projector_train_forward_indexed": (C.c_int, [C.POINTER(Conv), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int64,
                                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ipsx_projector_wgrad_indexed": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int,
                                               C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ipsx_attn_pool_supported": (C.c_int, [C.c_int, C.c_int]),
    "ipsx_attn_pool_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int, C.c_int]),
    "ipsx_attn_pool_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ipsx_attn_pool_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                          C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ipsx_attn_pool_forward_counted": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ipsx_attn_pool_backward_counted": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                                  C.c_void_p]),
}


def library_path():
    return _SO


def build(verbose=False):
    """Compile ips_amd/csrc for gfx950 into ips_amd/lib/libipsx.so (in-tree)."""
    cmd = ["make", "-C", os.path.join(_PKG, "csrc")] + ([] if verbose else ["-s"])
    subprocess.check_call(cmd)
    return _SO


def lib():
    """The loaded library.  Raises (never falls back) when it is missing."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(_SO):
            raise RuntimeError(
                "libipsx.so not found at {} - build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` or `make -C ips_amd/csrc`; the HIP backend has no fallback".format(_SO))
        L = C.CDLL(_SO)
        for name, (res, args) in _EXPORTS.items():
            fn = getattr(L, name)          # AttributeError here = header/library mismatch
            fn.restype, fn.argtypes = res, args
        if L.ipsx_version() // 100 != ABI_MAJOR:
            raise RuntimeError("libipsx.so ABI version {} != {}.x (include/ipsx.h: the major number changes with every "
                               "incompatible change of an exported signature)".format(L.ipsx_version(), ABI_MAJOR))
        L.ipsx_set_tie_order(_TIE_MODES[tie_order()])
        if os.environ.get("IPSX_CAM_HEAD"):        # diagnostic: units a lone slide's projector stream hands out as column quarters first
            L.ipsx_dbg_stream_head.restype, L.ipsx_dbg_stream_head.argtypes = None, [C.c_int]
            L.ipsx_dbg_stream_head(int(os.environ["IPSX_CAM_HEAD"]))
        if os.environ.get("IPSX_SCAN_R8", "1") == "0":      # diagnostic: the 8-row loop shapes through scan_fast_kernel
            L.ipsx_dbg_scan_r8.argtypes = [C.c_int]
            L.ipsx_dbg_scan_r8(0)
        if os.environ.get("IPSX_SCAN_LOGITS", "1") == "0":  # diagnostic: logits launches in front of scan_mnist_kernel's ranges
            L.ipsx_dbg_scan_logits.restype, L.ipsx_dbg_scan_logits.argtypes = C.c_int, [C.c_int]
            L.ipsx_dbg_scan_logits(0)
        _LIB = L
    return _LIB


def _ck(rc, what):
    if rc != 0:
        raise RuntimeError("{} failed ({}): {}".format(what, rc, lib().ipsx_last_error().decode()))


def _stream():
    """The current stream's handle.  (The raw getter: ``torch.cuda.current_stream()`` builds a Stream object through three
    Python layers - ~4 us, ten times per ips() call, most of them between the first and the last launch of the call.)"""
    return C.c_void_p(_raw_stream(_cur_device()))


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)
if _raw_stream is None or _cur_device is None:          # (another torch build: the documented way)
    def _stream():                                      # noqa: F811
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _f32(t):
    if t.dtype != torch.float32:
        raise TypeError("expected float32, got {}".format(t.dtype))
    return t if t.is_contiguous() else t.contiguous()


# The argument contract of every wrapper below and in hip_train.py: three helpers, attribute comparisons
# only - nothing that synchronises, allocates or launches while the arguments are valid.
def _same_gpu(what, names, *tensors):
    """Every tensor of a call (None: absent) lies on ONE GPU -> that device.  (``names``: of ``tensors``, for the message - the
    positional form of ``_one_gpu`` for the wrappers a selection calls many times.)"""
    dev = None
    for t in tensors:
        if t is not None:
            d = t.device
            if dev is None:
                if not _gpu_device(d):
                    raise ValueError("{}: {} lies on {}, the kernels read and write GPU memory".format(
                        what, [n for n, u in zip(names, tensors) if u is t][0], d))
                dev = d
            elif d != dev:
                raise ValueError("{}: {} lies on {}, the call's other tensors on {}".format(
                    what, [n for n, u in zip(names, tensors) if u is t][0], d, dev))
    return dev


def _one_gpu(what, **tensors):
    """Every tensor of a call (None: absent) lies on ONE GPU -> that device."""
    return _same_gpu(what, tuple(tensors), *tensors.values())


def _rd(what, name, t, dtype=torch.float32, dim=None, align=16, cl=False):
    """A tensor the kernel only READS, as the kernel takes it.  Another dtype or rank is refused (an index tensor is never
    converted); another layout - transposed, strided, sliced, expanded, channels-first where ``cl`` asks for channels-last -
    is copied, and so is a tensor whose address is no multiple of ``align`` (a fresh allocation is)."""
    if t.dtype != dtype:
        raise TypeError("{}: {} must be {}, got {}".format(what, name, dtype, t.dtype))
    if dim is not None and t.dim() != dim:
        raise ValueError("{}: {} must have {} dimensions, got {}".format(what, name, dim, tuple(t.shape)))
    if cl:
        if not t.is_contiguous(memory_format=torch.channels_last):
            return t.contiguous(memory_format=torch.channels_last)
    elif not t.is_contiguous():
        return t.contiguous()
    return t.clone() if t.data_ptr() % align else t


def _wr(what, name, t, dtype, shape=None, align=1, cl=False):
    """A tensor the kernel WRITES (outputs, loop state, workspaces, flags): handed over where it lies, never copied - so
    another dtype, shape, layout or an address that is no multiple of ``align`` is refused."""
    if t.dtype != dtype or (shape is not None and tuple(t.shape) != tuple(shape)) or t.data_ptr() % align or \
            not (t.is_contiguous(memory_format=torch.channels_last) if cl else t.is_contiguous()):
        raise ValueError("{}: {} must be a {}{} {} tensor{}, got {} {} with strides {} at an address {} mod 16".format(
            what, name, "channels-last" if cl else "contiguous", " " + str(tuple(shape)) if shape is not None else "", dtype,
            " at a {}-byte address".format(align) if align > 1 else "", t.dtype, tuple(t.shape), t.stride(), t.data_ptr() % 16))
    return t


def _workspace(what, ws):
    """A caller's workspace: contiguous uint8 bytes (None: the wrapper allocates)."""
    return _wr(what, "workspace", ws, torch.uint8, align=16) if ws is not None else None


def slot_counts(what, count, B, M, device):
    """The filled slots of a zero-padded batch (``IPSNet.last_mem_count``) as the masked aggregator takes them: -> ONE int32
    tensor of shape (B,) on ``device``.  ``count``: a sequence of B ints, or an integer tensor of shape (B,) on any device.
    What lies on the host is checked here, before anything is launched or allocated: a wrong length or an entry outside
    1 .. M raises ValueError.  A tensor that already lies on a GPU is NOT read back (that would synchronise): its shape and
    dtype are checked, its entries are not - the kernels clamp them into 1 .. M."""
    if torch.is_tensor(count):
        if count.is_floating_point() or count.is_complex() or count.dtype == torch.bool:
            raise TypeError("{}: count must hold integers, got {}".format(what, count.dtype))
        if tuple(count.shape) != (B,):
            raise ValueError("{}: count must have shape ({},) - one entry per image - got {}".format(what, B, tuple(count.shape)))
        if count.device.type != "cpu":
            return count.to(device=device, dtype=torch.int32).contiguous()
        count = count.tolist()
    try:
        seq = [operator.index(c) for c in count]
    except TypeError:
        raise TypeError("{}: count must be a sequence of ints or an integer tensor, got {!r}".format(what, count)) from None
    if len(seq) != B:
        raise ValueError("{}: count has {} entries for a batch of {}".format(what, len(seq), B))
    bad = [c for c in seq if not 1 <= c <= M]
    if bad:
        raise ValueError("{}: count entries must lie in 1 .. M = {}, got {}".format(what, M, bad[0]))
    return torch.tensor(seq, dtype=torch.int32, device=device)


_PATCH_DTYPES = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}


def _patch_table(table, n_chan, device):
    """A dequantisation table as the uint8 entry points take it: (n_chan, 256) float32, contiguous, on ``device``."""
    from .quant import check_table
    check_table(table, n_chan)
    if table.device != device:
        raise ValueError("the patch table lies on {}, the patches on {}".format(table.device, device))
    return table if table.is_contiguous() else table.contiguous()


def _call_twin(name, head, table, tail, u8=None):
    """The one rule of the float32 / uint8 twin exports: ``name(*head, *tail)`` on float32 storage, and on uint8 storage
    (``u8``; default: there is a ``table``) the ``_u8`` twin, whose ``table`` - where it takes one - stands behind the base
    pointer, the last of ``head``."""
    if (table is not None) if u8 is None else u8:
        name, head = name + "_u8", head + ((_p(table),) if table is not None else ())
    _ck(getattr(lib(), name)(*head, *tail), name)


def _patches(t, table=None):
    """Patch tensors may be stored in bfloat16 / float16 (BASELINE configs[4]); only the reduced-precision fused trunks
    read those (the exact path's contract is float32 in).  uint8 patches go with a ``table`` (n_chan, 256) on the exact
    path only: its stems look every byte up (``ips_amd.quant``); everything is checked here, before the first launch."""
    if t.dtype == torch.uint8:
        if table is None:
            raise TypeError("uint8 patches need a dequantisation table: IPSNet.set_patch_table(ips_amd.quant.patch_table(...)) "
                            "(EncoderPlan.encode(..., table=))")
        if precision() != "fp32":
            raise TypeError("uint8 patches go with the exact trunk (IPSX_PRECISION=fp32), not {}".format(precision()))
        if dedup_blank():
            raise TypeError("blank-patch dedup reads float32 patches (IPSX_DEDUP_BLANK=1 with uint8 patches)")
        _patch_table(table, t.shape[-3], t.device)
        return t if t.is_contiguous() else t.contiguous()
    if table is not None:
        raise TypeError("a patch table goes with uint8 patches, got {}".format(t.dtype))
    if t.dtype not in _PATCH_DTYPES:
        raise TypeError("patches must be float32, bfloat16 or float16, got {}".format(t.dtype))
    if t.dtype != torch.float32 and precision() == "fp32":
        raise TypeError("{} patch storage needs IPSX_PRECISION=bf16 or fp32x3 (the exact trunk reads float32)".format(t.dtype))
    return t if t.is_contiguous() else t.contiguous()


# ------------------------------------------------------------------ scorer
def query_proj(q, wq, temperature):
    """(T, D) queries, (H*Dk, D) weight -> (T, H*Dk) = (q @ wq.T) / temperature."""
    _one_gpu("query_proj", q=q, wq=wq)
    q, wq = _rd("query_proj", "q", q.detach(), dim=2, align=4), _rd("query_proj", "wq", wq.detach(), dim=2, align=4)
    if q.shape[1] != wq.shape[1]:
        raise ValueError("query_proj: q has {} features, wq takes {}".format(q.shape[1], wq.shape[1]))
    out = torch.empty((q.shape[0], wq.shape[0]), dtype=torch.float32, device=q.device)
    _ck(lib().ipsx_query_proj(_p(q), _p(wq), C.c_float(temperature), q.shape[0], q.shape[1],
                              wq.shape[0], _p(out), _stream()), "ipsx_query_proj")
    return out


def pack_linear(weight):
    """nn.Linear weight (out, in) -> MFMA B-operand stream (a 1x1 convolution)."""
    w = weight.detach()
    if w.dim() != 2:
        raise ValueError("pack_linear: weight must be (out, in), got {}".format(tuple(w.shape)))
    return _pack_conv(w.reshape(w.shape[0], w.shape[1], 1, 1))


def _fold_args(what, qs, wk_weight, H, Dk, T):
    """(T, H*Dk) scaled query and (H*Dk, D) key weight on one GPU -> qs as the kernel reads it, D."""
    _one_gpu(what, qs=qs, wk_weight=wk_weight)
    qs = _rd(what, "qs", qs.detach(), dim=2, align=4)          # (fold_query_kernel: 4-byte loads)
    if wk_weight.dtype != torch.float32 or wk_weight.dim() != 2:
        raise TypeError("{}: wk_weight must be a float32 (H*Dk, D) matrix, got {} {}".format(what, wk_weight.dtype, tuple(wk_weight.shape)))
    if tuple(qs.shape) != (T, H * Dk) or wk_weight.shape[0] != H * Dk:
        raise ValueError("{}: qs must be ({}, {}) and wk_weight ({}, D), got {} and {}".format(
            what, T, H * Dk, H * Dk, tuple(qs.shape), tuple(wk_weight.shape)))
    return qs, wk_weight.shape[1]


def fold_query(qs, wk_weight, H, Dk, T):
    """Scaled query (T, H*Dk) folded into the key weights k_w.weight (H*Dk, D) -> packed (H*T, D) operand of
    ``logits`` (ipsx_fold_query): logit = x . V[h*T + t],  V[h*T + t] = sum_j qs[t][h, j] k_w[h*Dk + j]."""
    qs, D = _fold_args("fold_query", qs, wk_weight, H, Dk, T)
    out = torch.empty(lib().ipsx_folded_query_elems(H, T, D), dtype=torch.float32, device=qs.device)
    _ck(lib().ipsx_fold_query(_p(qs), _p(pack_linear(wk_weight)), H, Dk, T, D, _p(out), _stream()), "ipsx_fold_query")
    return out


def fold_query_bf16(qs, wk_weight, H, Dk, T):
    """The folded query rounded to bfloat16 in the operand layout of ``ipsx_logits_bf16`` (a uint8 tensor: that dtype is
    how ``logits`` tells the two apart)."""
    qs, D = _fold_args("fold_query_bf16", qs, wk_weight, H, Dk, T)
    out = torch.empty(lib().ipsx_folded_query_bf16_bytes(H, T, D), dtype=torch.uint8, device=qs.device)
    _ck(lib().ipsx_fold_query_bf16(_p(qs), _p(pack_linear(wk_weight)), H, Dk, T, D, _p(out), _stream()),
        "ipsx_fold_query_bf16")
    return out


def logits(emb, pos, vq, R, out=None, cond=None, mask=1):
    """Per-patch attention logits (B, n, R = H*T) from the folded query ``vq``; ``out`` may be a column slice of
    (B, N, R).  A bfloat16 folded query (``fold_query_bf16``) selects the bf16 matrix pipe.  ``cond`` (int32 device
    scalar; fp32 folded query only): a conditional launch that does nothing unless a bit of ``mask`` is set in it."""
    emb, pos, pos_bs, out = _logits_args("logits", emb, pos, vq, R, out, cond)
    B, n, D = emb.shape
    if vq.dtype == torch.uint8:
        if cond is not None:
            raise ValueError("conditional logits: fp32 folded query only")
        _ck(lib().ipsx_logits_bf16(_p(emb), n * D, _p(pos), pos_bs, _p(vq), B, n, D, R, _p(out), out.stride(0), _stream()),
            "ipsx_logits_bf16")
        return out
    if cond is not None:
        _ck(lib().ipsx_logits_if(_p(emb), n * D, _p(pos), pos_bs, _p(vq), B, n, D, R, _p(out), out.stride(0), _p(cond), mask,
                                 _stream()), "ipsx_logits_if")
        return out
    _ck(lib().ipsx_logits(_p(emb), n * D, _p(pos), pos_bs, _p(vq), B, n, D, R, _p(out), out.stride(0), _stream()),
        "ipsx_logits")
    return out


_VQ_SIZE = {}


def _logits_args(what, emb, pos, vq, R, out, cond):
    """The arguments of the logits kernels, checked -> (emb, pos, pos_bstride, out) as the kernel takes them.  ``emb`` /
    ``pos`` are read with 16-byte loads when D % 8 == 0 (csrc/logits.hip ``logits_wave``: no scalar route at that D), so a
    view at another address or with rows that are not D apart is copied; ``out`` is written with 4-byte stores, row by row.
    (Called ten times per ``ips()``: plain comparisons, written out.)"""
    _same_gpu(what, _LOGITS_NAMES, emb, pos, vq, out, cond)
    shape = emb.shape
    if emb.dtype != torch.float32:
        raise TypeError("{}: emb must be float32, got {}".format(what, emb.dtype))
    if len(shape) != 3:
        raise ValueError("{}: emb must be (B, n, D), got {}".format(what, tuple(shape)))
    B, n, D = shape
    align = 4 if D & 7 else 16
    if not emb.is_contiguous():
        emb = emb.contiguous()
    elif emb.data_ptr() % align:
        emb = emb.clone()
    size = _VQ_SIZE.get((vq.dtype, R, D))
    if size is None:
        if vq.dtype == torch.float32:
            size = lib().ipsx_folded_query_elems(R, 1, D)
        elif vq.dtype == torch.uint8:
            size = lib().ipsx_folded_query_bf16_bytes(R, 1, D)
        else:
            raise TypeError("{}: vq must be a folded query (float32, or uint8 bytes of bfloat16), got {}".format(what, vq.dtype))
        _VQ_SIZE[(vq.dtype, R, D)] = size
    if vq.numel() != size or vq.data_ptr() & 15 or not vq.is_contiguous():
        raise ValueError("{}: vq must be the contiguous folded query of R = {}, D = {} ({} elements at a 16-byte address), got {}".format(
            what, R, D, size, tuple(vq.shape)))
    if out is None:
        out = torch.empty((B, n, R), dtype=torch.float32, device=emb.device)
    else:
        st = out.stride()
        if out.dtype != torch.float32 or out.shape != (B, n, R) or st[2] != 1 or st[1] != R or (B > 1 and st[0] < n * R):
            raise ValueError("{}: out must be float32 ({}, {}, {}) with contiguous rows (a row range of a longer table), got {} {} "
                             "with strides {}".format(what, B, n, R, out.dtype, tuple(out.shape), st))
    pos_bs = 0
    if pos is not None:
        ps = pos.shape
        if pos.dtype != torch.float32:
            raise TypeError("{}: pos must be float32, got {}".format(what, pos.dtype))
        if len(ps) != 3 or ps[1] != n or ps[2] != D or (ps[0] != B and ps[0] != 1):
            raise ValueError("{}: pos must be ({} or 1, {}, {}), got {}".format(what, B, n, D, tuple(ps)))
        st = pos.stride()
        pos_bs = st[0] if ps[0] > 1 else 0
        if st[2] != 1 or st[1] != D or pos_bs < 0 or pos.data_ptr() % align or (pos_bs * 4) % align:
            pos = pos.clone() if pos.is_contiguous() else pos.contiguous()
            pos_bs = pos.stride(0) if ps[0] > 1 else 0
    if cond is not None:
        _word(what, "cond", cond)
    return emb, pos, pos_bs, out


_LOGITS_NAMES = ("emb", "pos", "vq", "out", "cond")


def _word(what, name, t, n=1):
    """An int32 flag / counter the kernels poll or set: ``n`` contiguous words on the GPU."""
    if t.dtype != torch.int32 or t.numel() != n or not t.is_contiguous():
        raise ValueError("{}: {} must hold {} contiguous int32 word(s), got {} {}".format(what, name, n, t.dtype, tuple(t.shape)))
    return t


def part_wait(done, want, status, bit=1):
    """Hold the current stream until the counter ``done`` (int32 device scalar, a part of ``EncoderPlan.encode_indexed``'s
    one launch) has reached ``want``; a wait without progress for ``persistent_wait_ms`` sets ``bit`` in ``status``."""
    _same_gpu("part_wait", ("done", "status"), done, status)
    _word("part_wait", "done", done)
    _word("part_wait", "status", status)
    _ck(lib().ipsx_part_wait(_p(done), int(want), _p(status), int(bit), _stream()), "ipsx_part_wait")


def logits_stats(emb, pos, vq, R, out, stats_x, stats_out, ln_eps):
    """``logits(emb, pos, vq, R, out)`` and, in the same launch, the LayerNorm row moments of ``stats_x`` (P, F) into
    ``stats_out`` (P, 2).  fp32 folded query only."""
    _same_gpu("logits_stats", ("emb", "stats_x", "stats_out"), emb, stats_x, stats_out)
    if vq.dtype != torch.float32:
        raise TypeError("logits_stats: vq must be the float32 folded query, got {}".format(vq.dtype))
    if out is None:
        raise ValueError("logits_stats: out must be given")
    stats_x = _rd("logits_stats", "stats_x", stats_x, dim=2)
    sn, sf = stats_x.shape
    _wr("logits_stats", "stats_out", stats_out, torch.float32, (sn, 2), align=8)
    emb, pos, pos_bs, out = _logits_args("logits_stats", emb, pos, vq, R, out, None)
    B, n, D = emb.shape
    _ck(lib().ipsx_logits_stats(_p(emb), n * D, _p(pos), pos_bs, _p(vq), B, n, D, R, _p(out), out.stride(0),
                                _p(stats_x), sn, sf, C.c_float(ln_eps), _p(stats_out), _stream()), "ipsx_logits_stats")
    return out


def scan_workspace(B, M, I, H, T, device):
    """Device workspace of the selection loop for candidate sets beyond the LDS (M + I above ~4,000: the reference's
    shipped CAMELYON configuration is M = I = 5000), or ``None`` when the shape needs none.  A caller that runs the loop on
    a side stream keeps it between calls (like its other per-call buffers) instead of allocating it there."""
    nb = lib().ipsx_scan_workspace_bytes(B, M, I, H, T)
    return torch.empty(nb, dtype=torch.uint8, device=device) if nb else None


def scan_workgroups_per_image(B, M, I, H, T):
    """Compute units the loop of ONE image occupies in a call of B images (1, or the team of csrc/scan_large_team.h)."""
    return max(1, int(lib().ipsx_scan_workgroups_per_image(B, M, I, H, T)))


def _scan_args(what, lg, M, I, H, T, mem_idx=None, tie=None, workspace=None, copy=True, words=()):
    """The arguments of a selection loop on a (B, N, H*T) float32 logits table, checked -> (lg, B, N).  The loops read
    ``lg`` rows with 16-byte loads (csrc/scan_large.hip, scan_cam.hip): a view is copied where the loop only reads a
    finished table (``copy``) and refused where producers still write it; ``mem_idx`` (B, M) int64 and ``tie`` (B,) int32
    are loop state, ``words`` int32 flags: handed over where they lie."""
    _same_gpu(what, _SCAN_NAMES, lg, mem_idx, tie, workspace, *words)
    shape = lg.shape
    if len(shape) != 3 or shape[2] != H * T:
        raise ValueError("{}: lg must be (B, N, H*T = {}), got {}".format(what, H * T, tuple(shape)))
    B, N = shape[0], shape[1]
    if N <= M:
        raise ValueError("{}: lg has N = {} rows per image, the loop needs more than M = {}".format(what, N, M))
    if lg.dtype != torch.float32:
        raise TypeError("{}: lg must be float32, got {}".format(what, lg.dtype))
    if not lg.is_contiguous() or lg.data_ptr() & 15:
        if not copy:
            raise ValueError("{}: lg must be the whole contiguous (B, N, H*T) table at a 16-byte address (it is read where it "
                             "lies), got strides {}".format(what, lg.stride()))
        lg = lg.clone() if lg.is_contiguous() else lg.contiguous()
    if mem_idx is not None and (mem_idx.dtype != torch.int64 or mem_idx.shape != (B, M) or not mem_idx.is_contiguous()):
        raise ValueError("{}: mem_idx must be a contiguous ({}, {}) int64 tensor, got {} {}".format(what, B, M, mem_idx.dtype, tuple(mem_idx.shape)))
    if tie is not None and (tie.dtype != torch.int32 or tie.shape != (B,) or not tie.is_contiguous()):
        raise ValueError("{}: tie must be a contiguous ({},) int32 tensor, got {} {}".format(what, B, tie.dtype, tuple(tie.shape)))
    if workspace is not None:
        _workspace(what, workspace)
    return lg, B, N


_SCAN_NAMES = ("lg", "mem_idx", "tie", "workspace", "cond / ready", "status")


def scan(lg, M, I, H, T, want_scores=False):
    """The IPS chunk loop on cached logits (B, N, H*T) -> mem_idx (B, M) int64."""
    lg, B, N = _scan_args("scan", lg, M, I, H, T)
    mem_idx = torch.empty((B, M), dtype=torch.int64, device=lg.device)
    sc = torch.empty((B, M), dtype=torch.float32, device=lg.device) if want_scores else None
    tie = torch.zeros((B,), dtype=torch.int32, device=lg.device)
    ws = scan_workspace(B, M, I, H, T, lg.device)
    _ck(lib().ipsx_scan(_p(lg), B, N, M, I, H, T, _p(mem_idx), _p(sc), _p(tie), _p(ws), ws.numel() if ws is not None else 0,
                        _stream()), "ipsx_scan")
    scan.last_tie = tie
    return (mem_idx, sc) if want_scores else mem_idx


def scan_range(lg, M, I, H, T, it_begin, it_end, mem_idx, tie, workspace=None):
    """Iterations [it_begin, it_end) of the loop, state carried in ``mem_idx`` (B, M) int64 / ``tie`` (B,) int32.
    ``workspace``: ``scan_workspace(...)`` kept by the caller; allocated here (on the current stream) when missing."""
    lg, B, N = _scan_args("scan_range", lg, M, I, H, T, mem_idx, tie, workspace)
    ws = workspace if workspace is not None else scan_workspace(B, M, I, H, T, lg.device)
    _ck(lib().ipsx_scan_range(_p(lg), B, N, M, I, H, T, it_begin, it_end, _p(mem_idx), None, _p(tie),
                              _p(ws), ws.numel() if ws is not None else 0, _stream()), "ipsx_scan_range")
    return mem_idx


class LogitsPartStruct(C.Structure):
    """``ipsx_logits_part`` (include/ipsx.h): a part's (B, rows, D) embeddings, its rows per image, its first row in an image."""
    _fields_ = [("emb", C.c_void_p), ("rows", C.c_int64), ("first", C.c_int64)]


class LogitsParts:
    """The part table of ``ipsx_scan_range_logits`` and its launch (``scan_range``): the parts' embeddings ``embs[k]``
    (B, rows_k, D) float32, one after the other along the patch axis - part k holds the rows ``first[k] = rows_0 + ... + rows_(k-1)`` onwards of every image.  Made once
    per call; keeps the tensors it points to.  ``rows`` alone (ints) makes the table's arithmetic without tensors."""

    def __init__(self, embs=None, rows=None):
        if embs is not None:
            rows = [int(e.shape[1]) for e in embs]
        self.embs, self.rows = embs, [int(r) for r in rows]
        self.first = [sum(self.rows[:k]) for k in range(len(self.rows))]
        self.n = sum(self.rows)
        self.array = (LogitsPartStruct * max(1, len(self.rows)))()
        for k, r in enumerate(self.rows):
            self.array[k].emb = embs[k].data_ptr() if embs is not None else None
            self.array[k].rows, self.array[k].first = r, self.first[k]

    def __len__(self):
        return len(self.rows)

    def check(self, part_begin, part_end, M, I, it_begin, it_end):
        """The host-side check of ``ipsx_scan_range_logits`` on this table (``ipsx_scan_logits_check``; no device needed):
        raises RuntimeError with the library's message when the ranges do not fit the parts."""
        _ck(lib().ipsx_scan_logits_check(self.array, len(self), part_begin, part_end, self.n, M, I, it_begin, it_end),
            "ipsx_scan_logits_check")

    def scan_range(self, logits, M, I, H, T, it_begin, it_end, mem_idx, tie, part_begin, part_end, pos, vq, redo=None, mask=1,
                   gate=None, gate_publish=None, status=None, out=None):
        """``logits(self.embs[k], pos rows of part k, vq)`` for k in [part_begin, part_end) into the (B, N, H*T) table ``logits``
        and ``scan_range(logits, ..., it_begin, it_end, ...)`` as ONE launch, bit for bit (``ipsx_scan_range_logits``:
        ``scan_mnist_kernel``'s shape only - ``scan_mnist_shape`` - and D % 8 == 0).  ``pos``: (B or 1, >= N, D) positional rows of
        WHOLE images, or None.  ``redo`` (int32 device scalar): with a bit of ``mask`` set in it, all parts and the iterations
        [0, it_end) - the call's conditional redo inside this launch.  ``dbg_scan_logits(False)`` makes the library enqueue the
        launches this replaces instead.

        The hand-over between two such launches on different streams (``ipsx_scan_range_logits_gate``), each on its own or
        together: ``gate_publish`` (B int32 words): workgroup b stores ``it_end`` there at its end; ``gate`` (the same words,
        zeroed before either launch) with ``status`` (int32 device scalar): behind its prologue workgroup b waits on the device
        until ``gate[b] >= it_begin`` - a wait without progress for ``persistent_wait_ms`` sets bit ``mask`` in ``status`` and
        redoes the call in that workgroup; ``out`` (B, M) int64: the final indices go there, ``mem_idx`` is only read."""
        _same_gpu("scan_range_logits", ("logits", "mem_idx", "tie", "pos", "vq", "redo", "gate", "gate_publish", "status", "out") +
                  ("emb",) * len(self), logits, mem_idx, tie, pos, vq, redo, gate, gate_publish, status, out, *self.embs)
        lg, B, N = _scan_args("scan_range_logits", logits, M, I, H, T, mem_idx, tie, None, False)
        D = self.embs[0].shape[2]
        for k, e in enumerate(self.embs):
            if e.dtype != torch.float32 or e.dim() != 3 or tuple(e.shape) != (B, self.rows[k], D) or not e.is_contiguous() or e.data_ptr() & 15:
                raise ValueError("scan_range_logits: part {} must be a contiguous float32 ({}, {}, {}) block at a 16-byte address, got {} {}".format(
                    k, B, self.rows[k], D, e.dtype, tuple(e.shape)))
        if self.n != N:
            raise ValueError("scan_range_logits: the parts hold {} rows per image, the logits table {}".format(self.n, N))
        size = lib().ipsx_folded_query_elems(H * T, 1, D)
        if vq.dtype != torch.float32 or vq.numel() != size or vq.data_ptr() & 15 or not vq.is_contiguous():
            raise ValueError("scan_range_logits: vq must be the contiguous float32 folded query of R = {}, D = {} at a 16-byte address".format(H * T, D))
        pos_bs = 0
        if pos is not None:
            ps, st = pos.shape, pos.stride()
            if pos.dtype != torch.float32 or len(ps) != 3 or ps[1] < N or ps[2] != D or ps[0] not in (1, B):
                raise ValueError("scan_range_logits: pos must be float32 ({} or 1, >= {}, {}), got {} {}".format(B, N, D, pos.dtype, tuple(ps)))
            pos_bs = st[0] if ps[0] > 1 else 0
            if st[2] != 1 or st[1] != D or pos_bs < 0 or pos.data_ptr() & 15 or pos_bs & 3:
                pos = pos.contiguous()
                pos_bs = pos.stride(0) if ps[0] > 1 else 0
        if redo is not None:
            _word("scan_range_logits", "redo", redo)
        if gate is None and gate_publish is None and status is None and out is None:
            _ck(lib().ipsx_scan_range_logits(_p(lg), B, N, M, I, H, T, it_begin, it_end, _p(mem_idx), None, _p(tie), self.array, len(self),
                                             part_begin, part_end, D, _p(pos), pos_bs, _p(vq), _p(redo), mask if redo is not None else 0,
                                             _stream()), "ipsx_scan_range_logits")
            return mem_idx
        for name, t in (("gate", gate), ("gate_publish", gate_publish)):
            if t is not None:
                _word("scan_range_logits", name, t, B)
        if status is not None:
            _word("scan_range_logits", "status", status)
        if out is not None and (out.dtype != torch.int64 or out.shape != (B, M) or not out.is_contiguous() or out.data_ptr() == mem_idx.data_ptr()):
            raise ValueError("scan_range_logits: out must be a contiguous ({}, {}) int64 tensor other than mem_idx, got {} {}".format(
                B, M, out.dtype, tuple(out.shape)))
        _ck(lib().ipsx_scan_range_logits_gate(_p(lg), B, N, M, I, H, T, it_begin, it_end, _p(mem_idx), None, _p(tie), self.array, len(self),
                                              part_begin, part_end, D, _p(pos), pos_bs, _p(vq), _p(redo), mask if redo is not None else 0,
                                              _p(gate), it_begin if gate is not None else 0, _p(gate_publish), _p(status),
                                              mask if status is not None else 0, _p(out), _stream()), "ipsx_scan_range_logits_gate")
        return mem_idx if out is None else out


def scan_range_strided(lg, n, M, I, H, T, it_begin, it_end, mem_idx, tie, workspace=None):
    """``scan_range`` on the first ``n`` rows per image of a (B, cap, H*T) logits table (``ipsx_scan_range_strided``): the
    candidate table of ``IPSNet.ips_stream``, whose capacity stays while ``n`` changes from feed to feed.  From
    ``it_begin = 0`` the memory is rows 0 .. M-1 and ``mem_idx`` comes back as row numbers of the table."""
    B, cap = lg.shape[:2]
    if lg.dtype != torch.float32 or lg.dim() != 3 or lg.stride(2) != 1 or lg.stride(1) != lg.shape[2] or (B > 1 and lg.stride(0) != cap * lg.shape[2]):
        raise ValueError("scan_range_strided needs a row-contiguous float32 (B, cap, H*T) logits table")
    if lg.shape[2] != H * T or lg.data_ptr() % 16:
        raise ValueError("scan_range_strided: lg must have H*T = {} columns and lie at a 16-byte address, got {}".format(H * T, tuple(lg.shape)))
    if not 0 < n <= cap:
        raise ValueError("{} candidates in a table of {} rows".format(n, cap))
    _one_gpu("scan_range_strided", lg=lg, mem_idx=mem_idx, tie=tie, workspace=workspace)
    _wr("scan_range_strided", "mem_idx", mem_idx, torch.int64, (B, M))
    _wr("scan_range_strided", "tie", tie, torch.int32, (B,))
    _workspace("scan_range_strided", workspace)
    ws = workspace if workspace is not None else scan_workspace(B, M, I, H, T, lg.device)
    _ck(lib().ipsx_scan_range_strided(_p(lg), cap, B, n, M, I, H, T, it_begin, it_end, _p(mem_idx), None, _p(tie),
                                      _p(ws), ws.numel() if ws is not None else 0, _stream()), "ipsx_scan_range_strided")
    return mem_idx


def scan_ragged(lg, offsets, lengths, M, I, H, T, want_scores=False, workspace=None, short_ok=False):
    """The IPS chunk loop on slides of different lengths in ONE launch (``ipsx_scan_ragged``): ``lg`` the packed
    (sum N_b, H*T) float32 logits, ``offsets`` the (B + 1,) int64 prefix sum of ``lengths`` on ``lg``'s device, ``lengths``
    the host ints -> mem_idx (B, M) int64, slide-local (and the scores with ``want_scores``); the tie flags are left in
    ``scan_ragged.last_tie``.  Every slide must have more than ``M`` rows: checked here, on the host lengths.
    ``short_ok``: that check is skipped - the workgroup of a slide with no more than ``M`` rows returns before its first
    read, so the ``mem_idx`` (and score) rows of such slides come back UNWRITTEN (``ragged_finish`` never reads them); one
    slide must still be longer than ``M``."""
    lengths = [int(n) for n in lengths]
    B, total = len(lengths), sum(lengths)
    if B == 0:
        raise ValueError("scan_ragged: no slides")
    _one_gpu("scan_ragged", lg=lg, offsets=offsets, workspace=workspace)
    _workspace("scan_ragged", workspace)
    if lg.data_ptr() % 16:
        raise ValueError("scan_ragged: lg must lie at a 16-byte address")
    if lg.dtype != torch.float32 or lg.dim() != 2 or not lg.is_contiguous() or lg.shape != (total, H * T):
        raise ValueError("scan_ragged needs a contiguous float32 ({}, {}) logits table, got {} {}".format(
            total, H * T, lg.dtype, tuple(lg.shape)))
    if offsets.dtype != torch.int64 or tuple(offsets.shape) != (B + 1,) or not offsets.is_contiguous() or offsets.device != lg.device:
        raise ValueError("scan_ragged needs the ({},) int64 row offsets on the logits' device".format(B + 1))
    for k, n in enumerate(lengths):
        if n <= M and not short_ok:
            raise ValueError("slide {} has {} rows: the loop needs more than M = {}".format(k, n, M))
    if max(lengths) <= M:
        raise ValueError("scan_ragged: no slide has more than M = {} rows".format(M))
    mem_idx = torch.empty((B, M), dtype=torch.int64, device=lg.device)
    sc = torch.empty((B, M), dtype=torch.float32, device=lg.device) if want_scores else None
    tie = torch.empty((B,), dtype=torch.int32, device=lg.device)
    ws = workspace
    if ws is None:
        nb = lib().ipsx_scan_workspace_bytes(1, M, I, H, T)
        ws = torch.empty(B * nb, dtype=torch.uint8, device=lg.device) if nb else None
    _ck(lib().ipsx_scan_ragged(_p(lg), _p(offsets), B, max(lengths), total, M, I, H, T, _p(mem_idx), _p(sc), _p(tie), _p(ws),
                               ws.numel() if ws is not None else 0, _stream()), "ipsx_scan_ragged")
    scan_ragged.last_tie = tie
    return (mem_idx, sc) if want_scores else mem_idx


def _on_gpu(what, *tensors):
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not _gpu_device(t.device) or (dev is not None and t.device != dev):
            raise ValueError("{}: every tensor lies on the GPU, all on the same one (got one on {})".format(what, t.device))
        dev = t.device


def scan_ragged_spans(lg, spans, n_max, M, I, H, T, mem_idx, tie, mem_score=None, workspace=None):
    """``scan_ragged`` on slides that lie anywhere in ONE (rows_total, H*T) float32 table (``ipsx_scan_ragged_spans``):
    ``spans`` (B, 2) int64 on ``lg``'s device, first row and row count per slide; ``n_max`` the caller's host-side bound on
    the counts.  ``mem_idx`` (B, M) int64 - row numbers inside the span -, ``mem_score`` (B, M) float32 or None and ``tie``
    (B,) int32 are the caller's: a slide whose count is not above ``M``, or whose span leaves the table, is left untouched
    in all three, and ``tie`` is only ever set (the caller clears it)."""
    _on_gpu("scan_ragged_spans", lg, spans, mem_idx, tie, mem_score, workspace)
    if lg.dtype != torch.float32 or lg.dim() != 2 or not lg.is_contiguous() or lg.shape[1] != H * T or lg.data_ptr() % 16:
        raise ValueError("scan_ragged_spans needs a contiguous float32 (rows, {}) logits table at a 16-byte address, got {} {}".format(
            H * T, lg.dtype, tuple(lg.shape)))
    _workspace("scan_ragged_spans", workspace)
    B = spans.shape[0] if spans.dim() == 2 else 0
    if spans.dtype != torch.int64 or tuple(spans.shape) != (B, 2) or B == 0 or not spans.is_contiguous() or spans.device != lg.device:
        raise ValueError("scan_ragged_spans needs (B, 2) int64 spans on the logits' device")
    if mem_idx.dtype != torch.int64 or tuple(mem_idx.shape) != (B, M) or not mem_idx.is_contiguous():
        raise ValueError("mem_idx must be a contiguous ({}, {}) int64 tensor".format(B, M))
    if tie.dtype != torch.int32 or tuple(tie.shape) != (B,) or not tie.is_contiguous():
        raise ValueError("tie must be a contiguous ({},) int32 tensor".format(B))
    if mem_score is not None and (mem_score.dtype != torch.float32 or tuple(mem_score.shape) != (B, M) or not mem_score.is_contiguous()):
        raise ValueError("mem_score must be a contiguous ({}, {}) float32 tensor".format(B, M))
    ws = workspace
    if ws is None:
        nb = lib().ipsx_scan_workspace_bytes(1, M, I, H, T)
        ws = torch.empty(B * nb, dtype=torch.uint8, device=lg.device) if nb else None
    _ck(lib().ipsx_scan_ragged_spans(_p(lg), _p(spans), B, int(n_max), lg.shape[0], M, I, H, T, _p(mem_idx), _p(mem_score), _p(tie),
                                     _p(ws), ws.numel() if ws is not None else 0, _stream()), "ipsx_scan_ragged_spans")
    return mem_idx


COMMIT_IDLE, COMMIT_APPEND, COMMIT_SELECT, COMMIT_MOVE = 0, 1, 2, 3


def stream_commit_ragged(tables, sel, slides, M, rows_max, pixels=None, view=None):
    """The state update of a ragged stream, ONE launch (``ipsx_stream_commit_ragged``).  ``tables``: up to four ``(held, piece,
    dst)`` - ``held`` (B, cap, ...) or None, all of whose rows may be read; ``piece`` (rows, ...) ONE packed tensor for all
    slides, or None for a table that holds all candidates itself; ``dst`` (B, cap', ...) contiguous (``held`` itself: append in
    place).  ``slides`` (B, 6) int64 on the device, per slide: held rows, candidates, tail_first, first row in the packed
    piece, the mode (``COMMIT_IDLE / _APPEND / _SELECT / _MOVE``), 0.  ``sel`` (B, M) int64 candidate rows of the slides that
    select, or None.  ``rows_max``: the most rows any slide writes (the grid).

    ``pixels`` and ``view`` (both, or neither): the stream is fed pixel-row bands (``ipsx_stream_commit_ragged_view``, DESIGN
    2.10).  ``tables[0]`` is the patch table ``(held, None, dst)`` with rows (C, ph, pw) of the pixels' dtype: candidate
    held + r of slide k is packed patch first_k + r of ``view`` (a ``RaggedView``) over ``pixels``, the packed 1-d float32 |
    uint8 buffer of the feed's windows, copied where it lies - bytes as bytes.  A strided ``pixels`` is copied, another dtype or
    rank refused.  -> the bytes per lane the patch table was copied with (16, 4 or 1); None without a view."""
    what = "stream_commit_ragged"
    if (pixels is None) != (view is None):
        raise ValueError("{}: pixels and view go together".format(what))
    flat = [t for tab in tables for t in tab]
    _on_gpu(what, sel, slides, pixels, *flat)
    if view is not None:
        if pixels.dtype not in (torch.float32, torch.uint8):
            raise TypeError("{}: a ragged view reads float32 or uint8 pixels, got {}".format(what, pixels.dtype))
        pixels = _rd(what, "pixels", pixels, dtype=pixels.dtype, dim=1, align=1)
        if not tables or tables[0][1] is not None:
            raise ValueError("{}: table 0 is the patch table: its piece is the view (pass None)".format(what))
        dst0 = tables[0][2]
        if dst0.dtype != pixels.dtype or tuple(dst0.shape[2:]) != view.patch_shape:
            raise ValueError("{}: table 0: rows of {} {}, the view's patches are {} {}".format(
                what, dst0.dtype, tuple(dst0.shape[2:]), pixels.dtype, view.patch_shape))
        e = view.table[len(view.sizes) - 1]
        if e.elem_off + view.patch_shape[0] * e.h * e.w > pixels.numel():
            raise ValueError("{}: the view's images end at element {}, the pixels hold {}".format(
                what, e.elem_off + view.patch_shape[0] * e.h * e.w, pixels.numel()))
    arr, B, piece_rows = _stream_tables(tables, packed=True)
    if tuple(slides.shape) != (B, 6) or slides.dtype != torch.int64 or not slides.is_contiguous():
        raise ValueError("slides must be a contiguous (B, 6) int64 tensor")
    _check_sel(sel, B, M)
    if view is None:
        _ck(lib().ipsx_stream_commit_ragged(arr, len(tables), _p(sel), _p(slides), B or 0, M, int(rows_max), piece_rows, _stream()),
            "ipsx_stream_commit_ragged")
        return None
    unit = C.c_int(0)
    _ck(lib().ipsx_stream_commit_ragged_view(arr, len(tables), _p(pixels), C.byref(view.on(pixels.device).struct), pixels.element_size(),
                                             _p(sel), _p(slides), B or 0, M, int(rows_max), piece_rows, C.byref(unit), _stream()),
        "ipsx_stream_commit_ragged_view")
    return unit.value


def _stream_tables(tables, n_cand=None, packed=False):
    """The tables of a commit -> (the ``ipsx_stream_table`` array, B, rows of the packed pieces); the checks a tensor allows
    before the library's own.  ``tables``: ``(held, held_rows, piece, dst)`` with ``piece`` (B or 1, n_cand - held_rows, ...)
    read where it lies, at most four; or, ``packed`` (the ragged call form): ``(held, piece, dst)`` - all rows of ``held`` may
    be read, and ``piece`` is ONE packed (rows, ...) tensor for all slides, of as many rows in every table."""
    if not packed and len(tables) > 4:
        raise ValueError("{} tables: a commit moves at most four".format(len(tables)))
    arr = (StreamTable * max(1, len(tables)))()
    B, piece_rows = None, 0
    for k, tab in enumerate(tables[:len(arr)]):
        held, held_rows, piece, dst = (tab[0], None, tab[1], tab[2]) if packed else tab
        if (packed and dst.dim() < 2) or not dst.is_contiguous():
            raise ValueError("table {}: the destination must be {}".format(k, "a contiguous (B, cap, ...) tensor" if packed else "contiguous"))
        B = dst.shape[0] if B is None else B
        if dst.shape[0] != B:
            raise ValueError("table {}: {} {}, the first table has {}".format(k, dst.shape[0], "slides" if packed else "images", B))
        t = arr[k]
        t.dst, t.dst_rows, t.dst_bstride_rows = dst.data_ptr(), dst.shape[1], dst.shape[1]
        t.row_bytes = dst[0, 0].numel() * dst.element_size()
        if held is not None:
            if not held.is_contiguous() or held.dtype != dst.dtype or held.shape[2:] != dst.shape[2:] or held.shape[0] != B \
                    or held.device != dst.device:
                raise ValueError("table {}: held rows must be a contiguous (B, cap, ...) tensor of the destination's kind".format(k))
            if packed:
                held_rows = held.shape[1]
            elif held_rows > held.shape[1]:
                raise ValueError("table {}: {} held rows in a buffer of {}".format(k, held_rows, held.shape[1]))
            t.held, t.held_bstride_rows = held.data_ptr(), held.shape[1]
        elif held_rows:
            raise ValueError("table {}: {} held rows but no buffer".format(k, held_rows))
        t.held_rows = held_rows or 0
        if piece is None:
            continue
        if packed:
            if piece.dtype != dst.dtype or piece.shape[1:] != dst.shape[2:] or piece.device != dst.device or not piece.is_contiguous():
                raise ValueError("table {}: the piece must be a contiguous packed (rows, ...) tensor of the destination's kind".format(k))
            if piece_rows and piece.shape[0] != piece_rows:
                raise ValueError("table {}: a piece of {} rows, another table's has {}".format(k, piece.shape[0], piece_rows))
            piece_rows = piece.shape[0]
            t.piece = piece.data_ptr()
            continue
        if piece.dtype != dst.dtype or piece.shape[2:] != dst.shape[2:] or piece.shape[0] not in (1, B) or piece.device != dst.device:
            raise ValueError("table {}: the piece must be a (B or 1, n, ...) tensor of the destination's kind".format(k))
        if piece.shape[1] != n_cand - held_rows:
            raise ValueError("table {}: a piece of {} rows behind {} held rows, {} candidates".format(k, piece.shape[1], held_rows, n_cand))
        if piece.shape[1] and not piece[0].is_contiguous():
            raise ValueError("table {}: the piece's rows must be contiguous inside an image".format(k))
        bs = piece.stride(0) if piece.shape[0] > 1 else 0
        if bs < 0:
            raise ValueError("table {}: negative batch stride".format(k))
        t.piece, t.piece_bstride_bytes = piece.data_ptr(), bs * piece.element_size()
    return arr, B, piece_rows


def _check_sel(sel, B, M):
    if sel is not None and (sel.dtype != torch.int64 or tuple(sel.shape) != (B, M) or not sel.is_contiguous()):
        raise ValueError("sel must be a contiguous (B, M) int64 tensor")


def stream_commit(tables, sel, M, n_cand, tail_first=0):
    """The state update of a stream, ONE launch (``ipsx_stream_commit``).  ``tables``: up to four ``(held, held_rows, piece,
    dst)`` - ``held`` (B, cap, ...) or None, of which the first ``held_rows`` rows per image are candidates; ``piece``
    (B or 1, n_cand - held_rows, ...) the candidates behind them (or None), read where it lies: any batch stride, rows
    contiguous; ``dst`` (B, cap', ...) contiguous.  ``sel`` (B, M) int64 candidate rows: ``dst[b, j] = cand[b, sel[b, j]]``,
    ``dst[b, M + r] = cand[b, tail_first + r]``.  ``sel`` None: ``dst[b, held_rows + r] = piece[b, r]`` (append; the rows in
    front stay as they are).  Everything is checked before the launch."""
    if tables is None:
        _ck(lib().ipsx_stream_commit(None, 0, None, 0, M, n_cand, tail_first, None), "ipsx_stream_commit")
    arr, B, _ = _stream_tables(tables, n_cand)
    _check_sel(sel, B, M)
    _on_gpu("stream_commit", sel, *[t for tab in tables for t in (tab[0], tab[2], tab[3])])
    st = _stream() if len(tables) else None
    _ck(lib().ipsx_stream_commit(arr, len(tables), _p(sel), B or 0, M, n_cand, tail_first, st), "ipsx_stream_commit")


def stream_commit_view(tables, images, view, sel, M, n_cand, tail_first=0):
    """``stream_commit`` for a stream fed pixel-row bands, ONE launch (``ipsx_stream_commit_view``).
    ``tables[0]`` is the patch table ``(held, held_rows, None, dst)`` with rows (C, ph, pw) of the images' dtype: its
    candidates behind the held rows are the first ``n_cand - held_rows`` patches per image of ``images`` (B, C, H, W)
    float32 | uint8 on the GPU, read through ``view`` (a ``PatchView``) where they lie - bytes are copied as bytes.  The other
    tables are those of ``stream_commit``.  -> the bytes per lane the patch table was copied with (16, 4 or 1)."""
    if tables is None:
        _ck(lib().ipsx_stream_commit_view(None, 0, _p(images), C.byref(view.struct), images.element_size(), None, 0, M, n_cand,
                                          tail_first, None, None), "ipsx_stream_commit_view")
    if images.dtype not in (torch.float32, torch.uint8):
        raise TypeError("a patch view reads float32 or uint8 images, got {}".format(images.dtype))
    if tuple(images.shape) != view.image_shape or not images.is_contiguous():
        raise ValueError("images are {}{}, the view was made for {}".format(tuple(images.shape), "" if images.is_contiguous() else
                                                                            " (not contiguous)", view.image_shape))
    if len(tables):
        held, held_rows, piece, dst = tables[0]
        if piece is not None:
            raise ValueError("table 0 is the patch table: its piece is the view (pass None)")
        if dst.dtype != images.dtype or tuple(dst.shape[2:]) != view.patch_shape or dst.device != images.device:
            raise ValueError("table 0: rows of {} {}, the view's patches are {} {}".format(
                dst.dtype, tuple(dst.shape[2:]), images.dtype, view.patch_shape))
    arr, B, _ = _stream_tables(tables, n_cand)
    _check_sel(sel, B, M)
    unit = C.c_int(0)
    _on_gpu("stream_commit_view", images, sel, *[t for tab in tables for t in (tab[0], tab[2], tab[3])])
    st = _stream()
    _ck(lib().ipsx_stream_commit_view(arr, len(tables), _p(images), C.byref(view.struct), images.element_size(), _p(sel), B or 0,
                                      M, n_cand, tail_first, C.byref(unit), st), "ipsx_stream_commit_view")
    return unit.value


def scan_range_if(lg, M, I, H, T, it_begin, it_end, mem_idx, tie, cond, mask=1, workspace=None):
    """``scan_range`` that every workgroup abandons at once unless ``cond`` (int32 device scalar) has a bit of ``mask``
    set: the in-call recovery of a persistent loop that gave up waiting (its status word, bit 0)."""
    lg, B, N = _scan_args("scan_range_if", lg, M, I, H, T, mem_idx, tie, workspace, False, (cond,))
    _word("scan_range_if", "cond", cond)
    if workspace is not None:
        _ck(lib().ipsx_scan_range_if_ws(_p(lg), B, N, M, I, H, T, it_begin, it_end, _p(mem_idx), None, _p(tie), _p(cond), mask,
                                        _p(workspace), workspace.numel(), _stream()), "ipsx_scan_range_if_ws")
        return mem_idx
    _ck(lib().ipsx_scan_range_if(_p(lg), B, N, M, I, H, T, it_begin, it_end, _p(mem_idx), None, _p(tie), _p(cond), mask,
                                 _stream()), "ipsx_scan_range_if")
    return mem_idx


Geometry = collections.namedtuple("Geometry", "cus xcds cus_per_xcd")
_GEOMETRY = {}


def device_geometry(dev):
    """(compute units, XCDs, compute units per XCD) of a device as this process sees it.  gfx950 / gfx942 chiplets have 32
    units each - SPX 256 units = 8 XCDs, DPX / QPX / CPX partitions 4 / 2 / 1 - and deal workgroups to their XCDs
    round-robin; anything else counts as one XCD.  Launch sizes of the selection pipelines are derived from this."""
    dev = torch.device(dev)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    g = _GEOMETRY.get(idx)
    if g is None:
        props = torch.cuda.get_device_properties(idx)
        cus = int(props.multi_processor_count)
        arch = str(getattr(props, "gcnArchName", ""))
        xcds = cus // 32 if (arch.startswith("gfx95") or arch.startswith("gfx94")) and cus % 32 == 0 and cus >= 32 else 1
        g = _GEOMETRY[idx] = Geometry(cus, xcds, cus // xcds)
    return g


# Persistent kernels (a selection loop that waits for rows its producers publish while both run) need kernels of
# different streams to actually run side by side.  Under rocprofv3's counter collection, thread traces or a serialising
# debug switch they do not - the loop could only time out.  Instead of guessing from environment variables this is
# established ONCE per device by doing it: a four-iteration loop is launched before its rows are published.  And it is
# revoked for the whole process when a loop ever times out in production (IPSNet mirrors the status word to the host).
_PERSIST_OK = {}
_PERSIST_OFF = None


def persistent_wait_ms(ms=0):
    """Longest wait of a persistent loop (and its gate) without any progress, in ms (default 50); ms > 0 sets it.
    ``IPSX_PERSIST_WAIT_MS`` sets it once per process, when the first device is asked about (``persistent_ok``)."""
    return lib().ipsx_set_persistent_wait_ms(int(ms))


_PERSIST_STRIKES = 0
_PERSIST_WAIT_SET = False


def persistent_ok(dev):
    global _PERSIST_WAIT_SET
    if _PERSIST_OFF is not None:
        return False
    if not _PERSIST_WAIT_SET:
        _PERSIST_WAIT_SET = True
        ms = int(os.environ.get("IPSX_PERSIST_WAIT_MS", "0") or 0)
        if ms > 0:
            persistent_wait_ms(ms)
    dev = torch.device(dev)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    ok = _PERSIST_OK.get(idx)
    if ok is None:
        ok = _PERSIST_OK[idx] = _persistent_selftest(torch.device("cuda", idx))
    return ok


def persistent_disable(reason):
    """Switch the persistent pipelines off for the rest of the process (per-part launches take over) and say so once."""
    global _PERSIST_OFF
    if _PERSIST_OFF is None:
        import warnings
        _PERSIST_OFF = reason
        warnings.warn("ips_amd: persistent selection loops are switched off for this process: " + reason +
                      " (IPSX_SCAN_PERSIST=0 avoids the attempt)")


_PERSIST_CALLS = 0            # calls that launched a resident loop (Selection.persistent_begin counts them)
_PERSIST_RECENT = []          # _PERSIST_CALLS at the time of every recent timeout


def persistent_timed_out(dev):
    """A persistent loop gave up waiting (its call was redone by the conditional launch: results valid).  ONE such event
    on healthy hardware is a stalled host between the loop's launch and its producer's - the soak run
    (tools/soak.py, profiles/r05_soak.txt) saw one in ~5,000 calls while the cyclic garbage collector could land there
    (40-60 ms per full collection; it is held off across those lines now) and one in ~19,000 since: it does not cost a
    long-running job its pipelines.  The device's self-test is run again (a device synchronisation, once per event), and
    the pipelines stay on while it passes and fewer than ``IPSX_PERSIST_STRIKES`` (default 3) loops have timed out within
    the last ``IPSX_PERSIST_WINDOW`` (default 1,000) calls that launched one.  -> True when they stay on."""
    global _PERSIST_STRIKES
    import warnings
    _PERSIST_STRIKES += 1
    limit = max(1, int(os.environ.get("IPSX_PERSIST_STRIKES", "3") or 3))
    window = max(1, int(os.environ.get("IPSX_PERSIST_WINDOW", "1000") or 1000))
    _PERSIST_RECENT[:] = [c for c in _PERSIST_RECENT if _PERSIST_CALLS - c < window] + [_PERSIST_CALLS]
    what = "a persistent selection loop timed out waiting for rows (its call was redone with per-part launches: results valid)"
    if len(_PERSIST_RECENT) >= limit:
        persistent_disable("%s - %d such events within %d calls" % (what, len(_PERSIST_RECENT), window))
        return False
    dev = torch.device(dev)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    ok = _PERSIST_OK[idx] = _persistent_selftest(torch.device("cuda", idx))
    if not ok:
        persistent_disable(what + "; a loop beside its producer no longer passes the device's self-test")
        return False
    warnings.warn("ips_amd: %s; the device's self-test passes, the persistent pipelines stay on (event %d of %d allowed within "
                  "%d calls; IPSX_PERSIST_WAIT_MS raises the wait, IPSX_PERSIST_STRIKES the allowance)"
                  % (what, len(_PERSIST_RECENT), limit, window))
    return True


def _persistent_selftest(dev):
    M = I = 16
    H, T = 8, 1
    if not scan_persistent_supported(M, I, H, T):
        return False
    N = M + 4 * I
    with torch.cuda.device(dev):
        lg = torch.zeros((1, N, H * T), dtype=torch.float32, device=dev)
        mem = torch.empty((1, M), dtype=torch.int64, device=dev)
        words = torch.zeros((3,), dtype=torch.int32, device=dev)            # tie | progress | status
        side, main = side_stream(dev), torch.cuda.current_stream(dev)
        side.wait_stream(main)
        with torch.cuda.stream(side):
            scan_persistent(lg, M, I, H, T, mem, words[0:1], words[1:2], words[2:3])
        scan_gate(words[2:3])
        publish_rows(words[1:2], N)
        main.wait_stream(side)
        torch.cuda.synchronize(dev)
        status = int(words[2].item())
    return (status & 1) == 0 and (status & 2) == 2


_SIDE_STREAMS = {}


def side_stream(dev):
    """THE side stream of a device (high priority: the few workgroups of a selection loop must not queue behind an encoder
    grid), shared by every net of the process: the runtime maps streams onto a handful of hardware queues in creation
    order, and a net whose fresh side stream lands on its main stream's queue runs loop and encoder one after the other
    (measured: the CAMELYON M = I = 5000 leg of bench.py 12 % slower when a leg before it had created streams)."""
    dev = torch.device(dev)
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    st = _SIDE_STREAMS.get(key)
    if st is None:
        st = _SIDE_STREAMS[key] = torch.cuda.Stream(device=dev, priority=-1)
    return st


def scan_persistent_supported(M, I, H, T):
    return bool(lib().ipsx_scan_persistent_supported(M, I, H, T))


def scan_persistent_large(M, I, H, T):
    """Does this shape run its persistent loop on ``scan_large_kernel`` (a candidate set beyond the LDS: the caller hands
    ``scan_workspace`` to ``scan_persistent`` / ``scan_range_if``)?"""
    return (not scan_persistent_supported(M, I, H, T) and lib().ipsx_scan_workspace_bytes(1, M, I, H, T) > 0
            and M + I <= 16384 and H * T <= 256)


def scan_mnist_shape(M, I, H, T):
    """Is this the shape of ``scan_mnist_kernel`` (8 heads x 4 tokens, M = I = 64: the dispatcher's predicate)?"""
    fn = lib().ipsx_dbg_scan_mnist_shape           # (diagnostic export, not in include/ipsx.h: bound here, not in _EXPORTS)
    fn.restype, fn.argtypes = C.c_int, [C.c_int] * 4
    return bool(fn(M, I, H, T))


def dbg_scan_mnist(on):
    """Diagnostic: ``False`` sends ``scan_mnist_kernel``'s shape through ``scan_fast_kernel`` (comparisons, A/B timing);
    the default is on.  Process-wide: restore it in a ``finally``."""
    fn = lib().ipsx_dbg_scan_mnist
    fn.restype, fn.argtypes = None, [C.c_int]
    fn(1 if on else 0)


def dbg_scan_logits(on):
    """Diagnostic: ``False`` makes ``LogitsParts.scan_range`` enqueue the launches it replaces - ``logits_kernel<1>`` per part, the
    loop's range, the conditional redo - and ``Selection.parts_one_launch`` take its earlier launch chain (comparisons, A/B
    timing); ``None`` only asks.  The default is on; ``IPSX_SCAN_LOGITS=0`` in the environment switches it off when the
    library is loaded.  Process-wide: restore it in a ``finally``.  -> the previous setting"""
    fn = lib().ipsx_dbg_scan_logits                # (diagnostic export, not in include/ipsx.h: bound here, not in _EXPORTS)
    fn.restype, fn.argtypes = C.c_int, [C.c_int]
    return bool(fn(-1 if on is None else (1 if on else 0)))


def scan_logits_on():
    """Does ``LogitsParts.scan_range`` run as one launch (``dbg_scan_logits``, ``IPSX_SCAN_LOGITS``)?"""
    return dbg_scan_logits(None)


def scan_persistent_groupable(M, I, H, T):
    """Can fewer resident workgroups than images run this shape's persistent loops (``scan_persistent(workgroups=)``)?"""
    return bool(lib().ipsx_scan_persistent_groupable(M, I, H, T))


def scan_persistent(lg, M, I, H, T, mem_idx, tie, ready, status, workgroups=0, workspace=None, stream=None):
    """The whole loop as one launch on the CURRENT stream that waits for ``ready`` (int32 device scalar, advanced with
    ``publish_rows`` on the producing stream; or one word per image - ``ready.numel() == B`` > 1 - when the producer works
    through the images one after the other) before it reads rows; see include/ipsx.h.  ``workgroups`` in (0, B): that
    many resident loops, each taking its images one after the other (``scan_persistent_groupable`` shapes)."""
    lg, B, N = _scan_args("scan_persistent", lg, M, I, H, T, mem_idx, tie, workspace, False, (ready, status))
    _wr("scan_persistent", "ready", ready, torch.int32)
    if ready.numel() not in (1, B):
        raise ValueError("ready: one word, or one per image")
    _word("scan_persistent", "status", status)
    st = C.c_void_p(stream.cuda_stream) if stream is not None else _stream()     # (``stream``: launch there without
    if workspace is not None:          # a candidate set beyond the LDS             #  making it the current stream)
        _ck(lib().ipsx_scan_persistent_ws(_p(lg), B, N, M, I, H, T, _p(mem_idx), None, _p(tie), _p(ready),
                                          1 if (ready.numel() == B and B > 1) else 0, _p(status), int(workgroups),
                                          _p(workspace), workspace.numel(), st), "ipsx_scan_persistent_ws")
        return mem_idx
    _ck(lib().ipsx_scan_persistent_on(_p(lg), B, N, M, I, H, T, _p(mem_idx), None, _p(tie), _p(ready),
                                      1 if (ready.numel() == B and B > 1) else 0, _p(status), int(workgroups), st),
        "ipsx_scan_persistent_on")
    return mem_idx


def scan_gate(status):
    """Hold the current stream until the persistent scan owning ``status`` is resident (bounded wait)."""
    _same_gpu("scan_gate", ("status",), status)
    _word("scan_gate", "status", status)
    _ck(lib().ipsx_scan_gate(_p(status), _stream()), "ipsx_scan_gate")


def publish_rows(ready, n_rows):
    """Advance the progress word ``ready`` (one int32 on the GPU) to ``n_rows`` on the current stream."""
    _same_gpu("publish_rows", ("ready",), ready)
    _word("publish_rows", "ready", ready)
    _ck(lib().ipsx_publish_rows(_p(ready), int(n_rows), _stream()), "ipsx_publish_rows")


def _scores_impl(x, qs, wk, H, Dk, T, want_attn):
    what = "attn_map" if want_attn else "scores"
    _one_gpu(what, x=x, qs=qs, wk=wk)
    x = _rd(what, "x", x, dim=3)           # (read by the logits kernel: 16-byte loads when D % 8 == 0)
    B, L, D = x.shape
    qs, Dw = _fold_args(what, qs, wk, H, Dk, T)
    if Dw != D:
        raise ValueError("{}: x has {} features, wk takes {}".format(what, D, Dw))
    sc = torch.empty((B, L), dtype=torch.float32, device=x.device)
    attn = torch.empty((B, H, T, L), dtype=torch.float32, device=x.device) if want_attn else None
    nb = lib().ipsx_scores_workspace_bytes(B, L, D, H, T)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=x.device)
    wkp = pack_linear(wk)
    _ck(lib().ipsx_scores(_p(x), _p(wkp), _p(qs), B, L, D, H, Dk, T, _p(sc), _p(attn),
                          _p(ws), nb, _stream()), "ipsx_scores")
    return sc, attn


def scores(x, qs, wk, H, Dk, T):
    return _scores_impl(x, qs, wk, H, Dk, T, False)[0]


def attn_map(x, qs, wk, H, Dk, T):
    return _scores_impl(x, qs, wk, H, Dk, T, True)[1]


def topm(sc, M):
    _one_gpu("topm", sc=sc)
    sc = _rd("topm", "sc", sc, dim=2, align=4)
    B, L = sc.shape
    if not 0 < M <= L:
        raise ValueError("topm: M = {} of L = {} candidates".format(M, L))
    top = torch.empty((B, M), dtype=torch.int64, device=sc.device)
    tie = torch.zeros((B,), dtype=torch.int32, device=sc.device)
    nb = lib().ipsx_topm_workspace_bytes(B, L, M)
    ws = torch.empty(nb, dtype=torch.uint8, device=sc.device) if nb else None
    _ck(lib().ipsx_topm(_p(sc), B, L, M, _p(top), _p(tie), _p(ws), nb, _stream()), "ipsx_topm")
    return top


def gather_rows(src, idx):
    """src (B|1, N, ...) on the GPU, idx (B, M) int64 -> (B, M, ...)."""
    _same_gpu("gather_rows", ("src", "idx"), src, idx)
    if idx.dtype != torch.int64 or idx.dim() != 2:
        raise TypeError("gather_rows: idx must be a (B, M) int64 tensor, got {} {}".format(idx.dtype, tuple(idx.shape)))
    B, M = idx.shape
    if src.dim() < 2 or src.shape[0] not in (1, B):
        raise ValueError("gather_rows: src must be ({} or 1, N, ...) for idx {}, got {}".format(B, tuple(idx.shape), tuple(src.shape)))
    if src.stride(0) == 0 and src.shape[0] > 1:      # expanded broadcast table
        src = src[:1]
    src = src if src.is_contiguous() else src.contiguous()
    idx = idx if idx.is_contiguous() else idx.contiguous()
    N = src.shape[1]
    row_bytes = src[0, 0].numel() * src.element_size()       # (no multiple of 4: uint8 rows of an odd size, copied by bytes)
    out = torch.empty((B, M) + tuple(src.shape[2:]), dtype=src.dtype, device=src.device)
    bstride = N if src.shape[0] > 1 else 0
    _ck(lib().ipsx_gather_rows(_p(src), _p(idx), _p(out), B, N, M, row_bytes, bstride, _stream()),
        "ipsx_gather_rows")
    return out


def dequant_patches(q, table):
    """uint8 patches (..., C, h, w) on the GPU -> float32 of the same shape, ``table[c][q]`` (``table``: (C, 256) float32,
    ``ips_amd.quant.patch_table``).  For the M patches a selection keeps: what leaves ``ips()`` is float32."""
    if q.dtype != torch.uint8 or q.dim() < 3:
        raise TypeError("expected uint8 (..., C, h, w) patches, got {} {}".format(q.dtype, tuple(q.shape)))
    _one_gpu("dequant_patches", q=q, table=table)
    table = _patch_table(table, q.shape[-3], q.device)
    q = q if q.is_contiguous() else q.contiguous()
    out = torch.empty(q.shape, dtype=torch.float32, device=q.device)
    c, hw = q.shape[-3], q.shape[-2] * q.shape[-1]
    _ck(lib().ipsx_dequant_patches(_p(q), _p(table), _p(out), q.numel() // max(1, c * hw), c, hw, _stream()),
        "ipsx_dequant_patches")
    return out


def ips_finish_supported(src, pos):
    """Can ``ips_finish`` end the call: device tensors whose rows are whole 16-byte units at 16-byte addresses?"""
    if not (on_device(src) and src.is_contiguous() and src.dim() >= 3):
        return False
    if (src[0, 0].numel() * src.element_size()) % 16 or src.data_ptr() % 16:
        return False
    if pos is None:
        return True
    if not on_device(pos) or pos.dim() != 3:
        return False
    p1 = pos[:1] if pos.stride(0) == 0 else pos
    return p1.is_contiguous() and (pos.shape[2] * pos.element_size()) % 16 == 0 and pos.data_ptr() % 16 == 0


def ips_finish(src, pos, idx_buf, status, status_host, order=None):
    """The end of an ``ips()`` call whose loop ran resident, ONE launch: ``src[b, idx[b, m]]``, ``pos[b, idx[b, m]]`` (or None),
    a fresh copy of the loop's index buffer, the loop's status word to its pinned host mirror (``ipsx_ips_finish``).
    ``order`` ((B or 1, N) int64, contiguous, on the device): the loop ran on shuffled numbering - the patch rows are
    ``src[b, order[b, idx[b, m]]]`` of the UNSHUFFLED ``src`` (``ipsx_ips_finish_indexed``), ``pos`` and the indices as before.
    -> (mem_idx, mem_patch, mem_pos)"""
    _same_gpu("ips_finish", ("src", "pos", "idx_buf", "status", "order"), src, pos, idx_buf, status, order)
    if idx_buf.dim() != 2:
        raise ValueError("ips_finish: idx_buf must be (B, M), got {}".format(tuple(idx_buf.shape)))
    B, M = idx_buf.shape
    _wr("ips_finish", "idx_buf", idx_buf, torch.int64)
    _word("ips_finish", "status", status)
    # status_host is THE host argument of this module: the pinned mirror the kernel writes the status word to
    if status_host.device.type != "cpu" or status_host.dtype != torch.int32 or status_host.numel() < 1:
        raise ValueError("ips_finish: status_host must be the pinned host mirror (int32, on the CPU), got {} on {}".format(
            status_host.dtype, status_host.device))
    if not ips_finish_supported(src, pos) or src.shape[0] not in (1, B):
        raise ValueError("ips_finish: src ({} or 1, N, ...) / pos must be contiguous device rows of whole 16-byte units at 16-byte "
                         "addresses (ips_finish_supported)".format(B))
    N = src.shape[1]
    if pos is not None and (pos.shape[0] not in (1, B) or pos.shape[1] < N):         # (a longer table: its first N rows)
        raise ValueError("ips_finish: pos must be ({} or 1, >= {}, D), got {}".format(B, N, tuple(pos.shape)))
    row_bytes = src[0, 0].numel() * src.element_size()
    out = torch.empty((B, M) + tuple(src.shape[2:]), dtype=src.dtype, device=src.device)
    idx = torch.empty_like(idx_buf)
    out_pos = None
    pos_bytes = pos_bs = 0
    if pos is not None:
        pos_bs = 0 if (pos.stride(0) == 0 or pos.shape[0] == 1) else pos.shape[1]
        pos_bytes = pos.shape[2] * pos.element_size()
        out_pos = torch.empty((B, M, pos.shape[2]), dtype=pos.dtype, device=pos.device)
    if order is not None:
        if order.dtype != torch.int64 or order.dim() != 2 or order.shape[1] != N or order.shape[0] not in (1, B) or \
                not order.is_contiguous() or order.device != src.device:
            raise ValueError("order must be a contiguous (B or 1, N) int64 tensor on the patches' device")
        _ck(lib().ipsx_ips_finish_indexed(_p(src), row_bytes, N if src.shape[0] > 1 else 0, N, _p(pos), pos_bytes, pos_bs, _p(idx_buf),
                                          _p(order), N if order.shape[0] > 1 else 0, B, M, _p(out), _p(out_pos), _p(idx), _p(status),
                                          _p(status_host), _stream()), "ipsx_ips_finish_indexed")
        return idx, out, out_pos
    _ck(lib().ipsx_ips_finish(_p(src), row_bytes, N if src.shape[0] > 1 else 0, N, _p(pos), pos_bytes, pos_bs, _p(idx_buf), B, M,
                              _p(out), _p(out_pos), _p(idx), _p(status), _p(status_host), _stream()), "ipsx_ips_finish")
    return idx, out, out_pos


def ragged_finish_supported(rows, pos):
    """Can ``ragged_finish`` end a padded ragged call: packed device rows (total, ...) - and positional rows (total, D) -
    that are whole 16-byte units at 16-byte addresses?"""
    for t in (rows, pos):
        if t is None:
            continue
        if not (on_device(t) and t.is_contiguous() and t.dim() >= 2 and t.shape[0] > 0):
            return False
        if (t[0].numel() * t.element_size()) % 16 or t.data_ptr() % 16:
            return False
    return rows is not None and (pos is None or (pos.dim() == 2 and pos.shape[0] == rows.shape[0] and pos.device == rows.device))


def _finish_args(name, what, unit, dev, offsets, B, M, total, mem_idx, flat, pos, pos_refusal, patch, out):
    """What ``ragged_finish`` and ``ragged_finish_view`` (``name``) ask alike of the (B + 1,) ``offsets`` (``unit``: "row",
    "patch"), ``mem_idx``, ``flat`` and ``out`` on the device ``dev`` of the ``what`` ("rows", "pixels"); ``pos_refusal``: what
    the caller has against ``pos``, said in its place; ``patch`` = (shape, dtype) of ``mem_patch`` -> the four result
    tensors, ``out`` or fresh ones."""
    if offsets.dtype != torch.int64 or tuple(offsets.shape) != (B + 1,) or B < 1 or not offsets.is_contiguous() or offsets.device != dev:
        raise ValueError("{} needs the (B + 1,) int64 {} offsets on the {}' device".format(name, unit, what))
    if mem_idx is not None and (mem_idx.dtype != torch.int64 or tuple(mem_idx.shape) != (B, M) or not mem_idx.is_contiguous()
                                or mem_idx.device != dev):
        raise ValueError("mem_idx must be a contiguous ({}, {}) int64 tensor on the {}' device".format(B, M, what))
    if flat is not None and (flat.dtype != torch.int32 or tuple(flat.shape) != (total,) or not flat.is_contiguous() or flat.device != dev):
        raise ValueError("flat must be a contiguous ({},) int32 tensor on the {}' device".format(total, what))
    if pos_refusal is not None:
        raise ValueError(pos_refusal)
    shapes = patch, ((B, M, pos.shape[1]), pos.dtype) if pos is not None else None, ((B, M), torch.int64), ((B, M), torch.int64)
    if out is None:
        return tuple(torch.empty(s[0], dtype=s[1], device=dev) if s is not None else None for s in shapes)
    for t, s in zip(out, shapes):
        if (t is None) != (s is None) or (t is not None and (tuple(t.shape) != s[0] or t.dtype != s[1] or not t.is_contiguous()
                                                              or t.device != dev)):
            raise ValueError("{}: out must be the four contiguous result tensors on the {}' device".format(name, what))
    return out


def ragged_finish(rows, offsets, mem_idx, M, flat=None, pos=None, out=None):
    """The end of ``IPSNet.ips_ragged(pad=True)``, ONE launch (``ipsx_ragged_finish``).  ``rows`` (total, ...) the packed rows
    of the B slides, ``offsets`` (B + 1,) int64 on their device, ``mem_idx`` (B, M) int64 slide-local as ``scan_ragged``
    leaves it (rows of slides with at most ``M`` rows are never read; None when no slide is longer), ``flat`` (total,) int32:
    packed row g is source row ``flat[g]`` of ``rows``, ``pos`` (total, D) the packed positional rows.  A slide with more
    than ``M`` rows gets its selected rows, a shorter one its rows in the order given and zeros behind them (written by the
    kernel: nothing depends on what the buffers held) -> (mem_patch (B, M, ...), mem_pos (B, M, D) | None, mem_idx (B, M)
    with -1 in the padding, rows (B, M): the packed row of every slot or -1).  ``out``: those four tensors (``mem_pos`` None
    without ``pos``), written in place of fresh ones."""
    if not ragged_finish_supported(rows, pos):
        raise ValueError("ragged_finish needs packed device rows of whole 16-byte units at 16-byte addresses")
    total, B = rows.shape[0], offsets.numel() - 1
    out, out_pos, idx, grow = _finish_args("ragged_finish", "rows", "row", rows.device, offsets, B, M, total, mem_idx, flat, pos, None,
                                           ((B, M) + tuple(rows.shape[1:]), rows.dtype), out)
    _ck(lib().ipsx_ragged_finish(_p(rows), rows[0].numel() * rows.element_size(), total, _p(offsets), _p(mem_idx), _p(flat), _p(pos),
                                 pos.shape[1] * pos.element_size() if pos is not None else 0, B, M, _p(out), _p(out_pos), _p(idx),
                                 _p(grow), _stream()), "ipsx_ragged_finish")
    return out, out_pos, idx, grow


def ragged_finish_view(pixels, rview, offsets, mem_idx, M, flat=None, pos=None, out=None, table=None):
    """The end of ``IPSNet.ips_image_ragged``, ONE launch (``ipsx_ragged_finish_view``): ``ragged_finish`` with the source
    row replaced by a grid patch copied out of its image.  ``pixels`` the packed 1-d float32 buffer, ``rview`` its
    ``RaggedView``, ``offsets`` (B + 1,) int64 packed patch numbers on the device, ``mem_idx`` / ``flat`` / ``pos`` as there
    -> (mem_patch (B, M, C, ph, pw), mem_pos | None, mem_idx with -1 in the padding, packed patch of every slot or -1).
    ``out``: those four tensors (``mem_pos`` None without ``pos``), written in place of fresh ones - every slot is written,
    nothing depends on what they held.  ``table`` (C, 256): ``pixels`` is the packed uint8 buffer and ``mem_patch`` comes
    back float32, ``table[c][byte]``, its padding float +0.0 (``ipsx_ragged_finish_view_u8``), as ``gather_patches_view``
    dispatches on its table."""
    B, total, dev = len(rview.sizes), rview.count, pixels.device
    if table is not None:
        if pixels.dtype != torch.uint8 or pixels.dim() != 1 or not pixels.is_contiguous() or not on_device(pixels):
            raise ValueError("ragged_finish_view with a table needs the packed 1-d uint8 buffer on the GPU")
        table = _patch_table(table, rview.patch_shape[0], dev)
    elif pixels.dtype != torch.float32 or pixels.dim() != 1 or not pixels.is_contiguous() or not on_device(pixels):
        raise ValueError("ragged_finish_view needs the packed 1-d float32 buffer on the GPU")
    bad_pos = pos is not None and (pos.dim() != 2 or pos.shape[0] != total or not pos.is_contiguous() or pos.device != dev
                                   or (pos.shape[1] * pos.element_size()) % 16 or pos.data_ptr() % 16)
    out, out_pos, idx, grow = _finish_args(
        "ragged_finish_view", "pixels", "patch", dev, offsets, B, M, total, mem_idx, flat, pos,
        "pos must be ({}, D) contiguous rows of whole 16-byte units on the pixels' device".format(total) if bad_pos else None,
        ((B, M) + rview.patch_shape, torch.float32), out)
    rview.on(dev)
    _call_twin("ipsx_ragged_finish_view", (_p(pixels),), table,
               (C.byref(rview.struct), _p(offsets), _p(mem_idx), M, _p(flat), _p(pos),
                pos.shape[1] * pos.element_size() if pos is not None else 0, _p(out), _p(out_pos), _p(idx), _p(grow), _stream()))
    return out, out_pos, idx, grow


def ragged_blank_flags(pixels, rview, index=None, first=0, n=None):
    """Which entries of a list of packed patches of a ragged view hold a non-zero pixel (``ipsx_ragged_view_blank_flags``)?
    ``pixels`` the packed 1-d float32 buffer on the GPU, ``rview`` its ``RaggedView`` (1x32x32 patches); the entries are
    packed patches ``index`` ((n,) int32 on the device; a number that is no packed patch reads packed patch 0) or
    ``first .. first + n - 1`` (default: all from ``first`` on) -> (n,) int32, 1 = non-blank (-0.0 is zero, a denormal is
    not): the rule of the exact blank-patch dedup, read where the patches lie.  A packed uint8 buffer: non-blank is any
    byte of the window other than 0 (``ipsx_ragged_view_blank_flags_u8``; no table: the rule reads bytes)."""
    u8 = pixels.dtype == torch.uint8
    if not (u8 or pixels.dtype == torch.float32) or pixels.dim() != 1 or not pixels.is_contiguous() or not on_device(pixels):
        raise ValueError("ragged_blank_flags needs the packed 1-d float32 (or uint8) buffer on the GPU")
    if index is not None:
        if index.dtype != torch.int32 or index.dim() != 1 or not index.is_contiguous() or index.device != pixels.device:
            raise ValueError("index must be a contiguous 1-d int32 tensor on the pixels' device")
        first, n = 0, index.numel()
    elif n is None:
        n = rview.count - first
    if first < 0 or n < 0 or (index is None and first + n > rview.count):
        raise ValueError("patches {} .. {} of a view of {}".format(first, first + n, rview.count))
    rview.on(pixels.device)
    out = torch.empty((n,), dtype=torch.int32, device=pixels.device)
    _call_twin("ipsx_ragged_view_blank_flags", (_p(pixels),), None, (C.byref(rview.struct), _p(index), first, n, _p(out), _stream()),
               u8=u8)                                   # (no table: the rule reads bytes)
    return out


def order_index(order, B, N, out=None):
    """``order`` ((B or 1, N) int64, contiguous, on the device) -> (B, N) int32 flat row numbers
    ``b * N + clamp(order[b, j], 0, N - 1)`` - what the row-indexed producers read through - in ONE launch
    (``ipsx_order_index``); ``out``: B * N int32 on the same device."""
    if order.dtype != torch.int64 or order.dim() != 2 or order.shape[1] != N or order.shape[0] not in (1, B) or \
            not order.is_contiguous() or not _gpu_device(order.device):
        raise ValueError("order must be a contiguous (B or 1, N) int64 tensor on the device")
    if out is None:
        out = torch.empty((B, N), dtype=torch.int32, device=order.device)
    elif out.dtype != torch.int32 or out.numel() != B * N or not out.is_contiguous() or out.device != order.device:
        raise ValueError("out must be B * N contiguous int32 on the order's device")
    _ck(lib().ipsx_order_index(_p(order), N if order.shape[0] > 1 else 0, B, N, _p(out), _stream()), "ipsx_order_index")
    return out.view(B, N)


# ------------------------------------------------------------------ image -> patches
def patchify(img, patch_size, patch_stride):
    """img (B, C, H, W) float32 on the GPU -> (B, N, C, ph, pw): unfold + permute + reshape of the reference's
    datasets (data/megapixel_mnist/mnist_dataset.py:44-51, data/traffic/traffic_dataset.py:336-343), batched."""
    _one_gpu("patchify", img=img)
    img = _rd("patchify", "img", img, dim=4, align=4)      # (ipsx_patchify takes its scalar route off 16-byte addresses)
    B, Cc, H, W = img.shape
    (ph, pw), (sh, sw) = patch_size, patch_stride
    n = lib().ipsx_patchify_count(H, W, ph, pw, sh, sw)
    if n <= 0:
        raise ValueError("patch {}x{} / stride {}x{} does not fit a {}x{} image".format(ph, pw, sh, sw, H, W))
    out = torch.empty((B, n, Cc, ph, pw), dtype=torch.float32, device=img.device)
    _ck(lib().ipsx_patchify(_p(img), B, Cc, H, W, ph, pw, sh, sw, _p(out), _stream()), "ipsx_patchify")
    return out


class PatchView:
    """The patch grid of a batch of whole images, as addresses (``ipsx_patch_view``): what
    ``patchify(images, patch_size, patch_stride)`` would copy out, patch ``p = (b * ny + py) * nx + px`` in the order of the
    reference's ``unfold`` - never materialised.  ``image_shape`` = (B, C, H, W)."""

    def __init__(self, image_shape, patch_size, patch_stride):
        B, Cc, H, W = (int(v) for v in image_shape)
        (ph, pw), (sh, sw) = (int(v) for v in patch_size), (int(v) for v in patch_stride)
        self.struct = PatchViewStruct(B, Cc, H, W, ph, pw, sh, sw)
        if min(B, Cc, H, W, ph, pw, sh, sw) <= 0 or ph > H or pw > W:
            raise ValueError("patch {}x{} / stride {}x{} does not fit {} images of {}x{}x{}".format(ph, pw, sh, sw, B, Cc, H, W))
        self.ny, self.nx = (H - ph) // sh + 1, (W - pw) // sw + 1
        if B * self.ny * self.nx >= 1 << 31:
            raise ValueError("a view of {} patches (the limit is 2^31 - 1)".format(B * self.ny * self.nx))
        self.image_shape, self.patch_size, self.patch_stride = (B, Cc, H, W), (ph, pw), (sh, sw)
        self.per_image = self.ny * self.nx         # N of the (B, N, C, ph, pw) tensor that does not exist
        self.count = B * self.per_image
        self.patch_shape = (Cc, ph, pw)

    def origin(self, p):
        """Element offset of patch ``p``'s (channel 0, row 0, column 0) inside the contiguous images, or -1 when ``p`` is
        no patch of the grid.  Element (c, y, x) of the patch lies ``(c * H + y) * W + x`` further."""
        _, Cc, H, W = self.image_shape
        if not 0 <= p < self.count:
            return -1
        r, px = divmod(int(p), self.nx)
        b, py = divmod(r, self.ny)
        return ((b * Cc) * H + py * self.patch_stride[0]) * W + px * self.patch_stride[1]

    def check(self, images, table=None):
        """``images`` as the view kernels read them: float32, or uint8 with their ``table`` (C, 256) - refused where uint8
        patches are (``_patches``) -, this view's shape, contiguous."""
        if images.dtype == torch.uint8 or table is not None:
            if tuple(images.shape) != self.image_shape:
                raise ValueError("images are {}, the view was made for {}".format(tuple(images.shape), self.image_shape))
            return _patches(images, table)
        if images.dtype != torch.float32:
            raise TypeError("a patch view reads float32 or uint8 images, got {}".format(images.dtype))
        if tuple(images.shape) != self.image_shape:
            raise ValueError("images are {}, the view was made for {}".format(tuple(images.shape), self.image_shape))
        return images if images.is_contiguous() else images.contiguous()

    def load_bytes(self, images, widths):
        """The launcher's rule for a view kernel's load width (``view_args``, csrc/ipsx_internal.h): the first of ``widths``
        (bytes, widest first) of which the images' address, their row pitch and the patches' column stride in bytes are
        all multiples; 0 when none is.  fused 1x32x32: float32 (16,), uint8 (16, 4, 1), its pair kernel (8, 4, 1); 1x50x50:
        (8,) / (2, 1); 3x100x100: (16,) / (4, 1)."""
        e = images.element_size()
        for wd in widths:
            if images.data_ptr() % wd == 0 and self.image_shape[3] * e % wd == 0 and self.patch_stride[1] * e % wd == 0:
                return wd
        return 0


class RaggedView:
    """The patch grids of whole images of DIFFERENT sizes that lie in one packed buffer, as addresses (``ipsx_ragged_view``,
    DESIGN 2.8): packed patch ``p`` is grid patch ``p - first_b`` (``py * nx_b + px``, the order of the reference's
    ``unfold``) of the image ``b`` with the largest ``first_b <= p``.  ``sizes`` the (H_b, W_b) pairs, ``elem_offsets`` the
    element offset of every image inside the buffer - the pixels are float32, or uint8 read through a table
    (``PatchSource(images=, ragged=, table=)``), for which an element is a byte.  The table is built and checked on the host
    (``ipsx_ragged_view_fill``: a geometry it refuses raises ValueError) and uploaded by ``on(device)``, once per device."""

    def __init__(self, channels, sizes, elem_offsets, patch_size, patch_stride):
        sizes = [(int(h), int(w)) for h, w in sizes]
        (ph, pw), (sh, sw) = (int(v) for v in patch_size), (int(v) for v in patch_stride)
        B, Cc = len(sizes), int(channels)
        self.table = (ImageEntry * max(B, 1))()
        total = lib().ipsx_ragged_view_fill(self.table, B, Cc, ph, pw, sh, sw, (C.c_int32 * max(B, 1))(*[s[0] for s in sizes]),
                                            (C.c_int32 * max(B, 1))(*[s[1] for s in sizes]),
                                            (C.c_int64 * max(B, 1))(*[int(o) for o in elem_offsets]))
        if total < 0:
            raise ValueError("patch {}x{} / stride {}x{} on images {}: {}".format(ph, pw, sh, sw, sizes, lib().ipsx_last_error().decode()))
        self.struct = RaggedViewStruct(B, Cc, ph, pw, sh, sw, None, self.table)
        self.sizes, self.patch_size, self.patch_stride, self.patch_shape = tuple(sizes), (ph, pw), (sh, sw), (Cc, ph, pw)
        self.grids = tuple((e.ny, e.nx) for e in self.table[:B])
        self.lengths = tuple(ny * nx for ny, nx in self.grids)       # patches per image
        self.firsts = tuple(e.first for e in self.table[:B])
        self.elem_offsets = tuple(e.elem_off for e in self.table[:B])
        self.count = int(total)
        self._device = {}                                             # device -> the uploaded table (kept alive here)

    def on(self, device, uploaded=None):
        """This view with its table on ``device`` (uploaded on first use) -> self.  ``uploaded``: the caller's own upload of
        ``bytes(self.table)`` to that device - a stream that makes a view per feed sends it with its other numbers."""
        device = torch.device(device)
        if uploaded is not None:
            if uploaded.device != device or uploaded.numel() * uploaded.element_size() < C.sizeof(ImageEntry) * len(self.sizes):
                raise ValueError("the uploaded table lies on {} with {} bytes".format(uploaded.device, uploaded.numel() * uploaded.element_size()))
            self._device[device] = uploaded
        dev = self._device.get(device)
        if dev is None:
            host = torch.frombuffer(bytearray(bytes(self.table)), dtype=torch.uint8)
            dev = self._device[device] = host.to(device)
        self.struct.images = dev.data_ptr()
        return self

    def load_width(self, pixels, widths):
        """The launcher's rule for a ragged view kernel's load width (``ragged_view_args``, csrc/ipsx_internal.h), a pure host
        function: the first of ``widths`` (bytes, widest first) of which the address of ``pixels`` (the packed 1-d buffer,
        float32 or uint8), every image's byte offset, every row pitch ``W_b`` in bytes and the patches' column stride in
        bytes are all multiples; 0 when none is.  The lists are ``PatchView.load_bytes``': fused 1x32x32 float32 (16,),
        uint8 (16, 4, 1), its pair kernel (8, 4, 1); 1x50x50 (8,) / (2, 1); 3x100x100 (16,) / (4, 1)."""
        e = pixels.element_size()
        for wd in widths:
            if pixels.data_ptr() % wd == 0 and self.patch_stride[1] * e % wd == 0 and \
                    all(o * e % wd == 0 and w * e % wd == 0 for o, (_, w) in zip(self.elem_offsets, self.sizes)):
                return wd
        return 0

    def origin(self, p):
        """(element offset of packed patch ``p``'s (0, 0, 0) inside the buffer, row pitch, channel pitch) - or (-1, 0, 0)
        when ``p`` is no packed patch (``ipsx_ragged_view_offset``: the function the kernels address by)."""
        pitch, chan = C.c_int64(0), C.c_int64(0)
        off = lib().ipsx_ragged_view_offset(self.table, len(self.sizes), C.byref(self.struct), int(p), C.byref(pitch), C.byref(chan))
        return int(off), int(pitch.value), int(chan.value)


class PatchSource:
    """Where the patches of an image-encoder call lie - what ``EncoderPlan.encode_source`` reads.  Either a patch tensor
    ``PatchSource(patches, table=None)``: (P, C, h, w) or (B, N, C, h, w) on the GPU, float32, float16 / bfloat16 under
    IPSX_PRECISION=bf16 / fp32x3, or uint8 with its ``table`` (C, 256); or whole images read through a patch grid
    ``PatchSource(images=..., view=..., table=None)`` (``PatchView``, DESIGN 2.3: float32 images, or uint8 images with
    their ``table``), whose patch tensor is never made; or images of different sizes in ONE packed 1-d buffer read
    through their grids ``PatchSource(images=pixels, ragged=..., table=None)`` (``RaggedView``, DESIGN 2.8: float32 pixels,
    or uint8 pixels with their ``table``).  Everything that
    refuses a storage kind does so here, once, before the first launch; what is kept is contiguous.  ``shape`` is that of
    the patch tensor (for a view: the one ``patchify`` would make), ``count`` its number of patches."""

    __slots__ = ("patches", "table", "images", "view", "shape", "dtype", "device", "count", "ragged")

    def __init__(self, patches=None, table=None, images=None, view=None, ragged=None):
        self.patches = self.table = self.images = self.view = self.ragged = None
        if ragged is not None:
            # images of different sizes in one packed 1-d buffer, read through a ``RaggedView``: float32, or
            # uint8 with their table - refused where uint8 patches are (``_patches``)
            if images.dim() != 1 or not on_device(images) or (images.dtype != torch.uint8 and (table is not None or
                                                                                               images.dtype != torch.float32)):
                raise TypeError("a ragged view reads a packed 1-d float32 buffer on the GPU, or a uint8 one with its table")
            if images.dtype == torch.uint8:
                if table is None:
                    raise TypeError("uint8 images need a dequantisation table: IPSNet.set_patch_table(ips_amd.quant.patch_table(...))")
                if precision() != "fp32":
                    raise TypeError("uint8 images go with the exact trunk (IPSX_PRECISION=fp32), not {}".format(precision()))
                if dedup_blank():
                    raise TypeError("blank-patch dedup reads float32 patches (IPSX_DEDUP_BLANK=1 with uint8 images)")
                self.table = _patch_table(table, ragged.patch_shape[0], images.device)
            self.images, self.ragged = images if images.is_contiguous() else images.contiguous(), ragged.on(images.device)
            self.shape = torch.Size((ragged.count,) + ragged.patch_shape)
            self.dtype, self.device, self.count = images.dtype, images.device, ragged.count
            return
        if view is not None:
            self.images, self.view = view.check(images, table), view
            if table is not None:
                self.table = _patch_table(table, images.shape[-3], images.device)
            self.shape = torch.Size((view.image_shape[0], view.per_image) + view.patch_shape)
            self.dtype, self.device, self.count = images.dtype, images.device, view.count
            return
        self.patches = patches = _patches(patches, table)
        if table is not None:
            self.table = _patch_table(table, patches.shape[-3], patches.device)
        self.shape, self.dtype, self.device = patches.shape, patches.dtype, patches.device
        self.count = patches.shape[:-3].numel()

    @property
    def is_view(self):
        return self.view is not None

    @property
    def base(self):
        """The tensor the kernels' base pointer points into."""
        return self.images if self.view is not None or self.ragged is not None else self.patches


def gather_patches_view(images, view, idx, table=None):
    """images (B, C, H, W) float32 on the GPU, idx (B, M) int64 patch numbers inside each image (py * nx + px) ->
    (B, M, C, ph, pw): ``patchify(images, ...)[b, idx[b, m]]`` copied straight out of the images.  uint8 images with
    their ``table`` (C, 256): float32 all the same, ``table[c][byte]``."""
    _one_gpu("gather_patches_view", images=images, idx=idx, table=table)
    images = view.check(images, table)
    if idx.dtype != torch.int64 or idx.dim() != 2 or idx.shape[0] != view.image_shape[0] or idx.device != images.device:
        raise ValueError("idx must be a (B, M) int64 tensor on the images' device")
    idx = idx if idx.is_contiguous() else idx.contiguous()
    M = idx.shape[1]
    out = torch.empty((idx.shape[0], M) + view.patch_shape, dtype=torch.float32, device=images.device)
    if table is not None:
        table = _patch_table(table, images.shape[-3], images.device)
    _call_twin("ipsx_gather_patches_view", (_p(images),), table, (C.byref(view.struct), _p(idx), M, _p(out), _stream()))
    return out


def patchify_sparse(index, value, offsets, canvas, patch_size, patch_stride, flags=False):
    """Sparse (H, W, C) canvases -> (B, N, C, ph, pw) patches on the GPU (mnist_dataset.py:34-51).

    ``index`` (nnz int64 flat positions), ``value`` (nnz float32), ``offsets`` (B+1 int64, image i owns
    [offsets[i], offsets[i+1])) - all on the GPU; ``canvas`` = (H, W, C).  With ``flags`` also returns the
    per-patch int32 non-blank flags (B*N)."""
    H, W, Cc = canvas
    (ph, pw), (sh, sw) = patch_size, patch_stride
    B = offsets.numel() - 1
    if index.dtype != torch.int64 or offsets.dtype != torch.int64 or value.dtype != torch.float32:
        raise TypeError("index / offsets must be int64 and value float32")
    _one_gpu("patchify_sparse", index=index, value=value, offsets=offsets)
    if index.dim() != 1 or value.dim() != 1 or offsets.dim() != 1 or index.numel() != value.numel():
        raise ValueError("patchify_sparse: index and value must be 1-d of one length, offsets 1-d, got {}, {} and {} (the kernel "
                         "reads no entry past that length, whatever offsets[-1] says)".format(
                             tuple(index.shape), tuple(value.shape), tuple(offsets.shape)))
    n = lib().ipsx_patchify_count(H, W, ph, pw, sh, sw)
    if n <= 0 or B <= 0:
        raise ValueError("bad geometry")
    index, value, offsets = index.contiguous(), value.contiguous(), offsets.contiguous()
    out = torch.empty((B, n, Cc, ph, pw), dtype=torch.float32, device=offsets.device)
    nb = torch.empty((B * n,), dtype=torch.int32, device=offsets.device) if flags else None
    _ck(lib().ipsx_patchify_sparse(_p(index), _p(value), _p(offsets), index.numel(), B, Cc, H, W, ph, pw, sh, sw,
                                   _p(out), _p(nb), _stream()), "ipsx_patchify_sparse")
    return (out, nb) if flags else out


# ------------------------------------------------------------------ bf16 layer kernels (the layered trunk under IPSX_PRECISION=bf16)
def conv2d_nhwc_bf16(x, weight, alpha, shift, stride, pad, residual=None, relu=True, out=None):
    """One convolution of the bf16 layer-by-layer trunk (conv_nhwc_bf16_kernel): ``x`` (n, h, w, C_in) bfloat16, OIHW float32
    ``weight`` (rounded to bf16 by the packing), float32 ``alpha`` / ``shift`` (C_out,) or None, ``residual``
    (n, ho, wo, C_out) bfloat16 or None  ->  (n, ho, wo, C_out) bfloat16 (written into ``out`` where one is given)."""
    _one_gpu("conv2d_nhwc_bf16", x=x, weight=weight, alpha=alpha, shift=shift, residual=residual, out=out)
    if x.dim() != 4 or x.dtype != torch.bfloat16 or not x.is_contiguous():
        raise ValueError("expected a contiguous bfloat16 (n, h, w, C) tensor")
    w = _f32(weight.detach())
    co, ci, kh, kw = w.shape
    n, h, wd, _ = x.shape
    alpha, shift = (_f32(alpha) if alpha is not None else None), (_f32(shift) if shift is not None else None)
    for name, t in (("alpha", alpha), ("shift", shift)):
        if t is not None and tuple(t.shape) != (co,):
            raise ValueError("conv2d_nhwc_bf16: {} must be ({},), got {}".format(name, co, tuple(t.shape)))
    cv = Conv(ci, co, kh, kw, stride, pad, None, _p(alpha), _p(shift), None)
    if x.shape[3] != ci or not lib().ipsx_conv2d_affine_nhwc_bf16_supported(C.byref(cv)):
        raise ValueError("the bf16 convolution needs C_in % 16 == 0 and C_out % 8 == 0, got {} -> {}".format(ci, co))
    ho, wo = (h + 2 * pad - kh) // stride + 1, (wd + 2 * pad - kw) // stride + 1
    if residual is not None and (residual.dtype != torch.bfloat16 or tuple(residual.shape) != (n, ho, wo, co) or
                                 not residual.is_contiguous()):
        raise ValueError("residual must be a contiguous bfloat16 (n, ho, wo, C_out) tensor")
    if out is not None and (out.dtype != torch.bfloat16 or tuple(out.shape) != (n, ho, wo, co) or not out.is_contiguous() or
                            out.device != x.device):
        raise ValueError("out must be a contiguous bfloat16 (n, ho, wo, C_out) tensor on the device of x")
    # (every refusal stands in front of the packing launch)
    half = torch.empty(lib().ipsx_packed_conv_weight_bf16_bytes(co, ci, kh, kw), dtype=torch.uint8, device=x.device)
    _ck(lib().ipsx_pack_conv_weight_bf16(_p(w), co, ci, kh, kw, _p(half), _stream()), "ipsx_pack_conv_weight_bf16")
    cv.w_packed_bf16 = half.data_ptr()
    y = out if out is not None else torch.empty((n, ho, wo, co), dtype=torch.bfloat16, device=x.device)
    _ck(lib().ipsx_conv2d_affine_nhwc_bf16(C.byref(cv), _p(x), _p(residual), _p(y), n, h, wd, int(bool(relu)), _stream()),
        "ipsx_conv2d_affine_nhwc_bf16")
    return y


def avgpool_nhwc_bf16(x):
    """(n, h, w, C) bfloat16 -> (n, C) float32: the fp32 sum over the pixels in memory order, divided by their number."""
    if x.dim() != 4 or x.dtype != torch.bfloat16 or not x.is_contiguous():
        raise ValueError("expected a contiguous bfloat16 (n, h, w, C) tensor")
    _one_gpu("avgpool_nhwc_bf16", x=x)
    n, h, w, c = x.shape
    y = torch.empty((n, c), dtype=torch.float32, device=x.device)
    _ck(lib().ipsx_avgpool_nhwc_bf16(_p(x), _p(y), n, c, h * w, _stream()), "ipsx_avgpool_nhwc_bf16")
    return y


# ------------------------------------------------------------------ aggregation
def aggregate(transf, x, count=None):
    """Transformer.forward in eval / no-grad mode: x (B, M, D) -> (B, n_token, D).  ``count`` (``slot_counts``: B ints or an
    integer tensor (B,); None = every slot): image b attends to its slots 0 .. count[b] - 1 only (ipsx_aggregate_counted) -
    out[b] has the bits of ``aggregate(transf, x[b:b + 1, :count[b]])``.  Host counts are checked here; a tensor on the GPU
    is not read back, the kernel clamps its entries into 1 .. M."""
    ca, mlp = transf.crs_attn, transf.mlp
    _one_gpu("aggregate", x=x, weights=ca.k_w.weight)
    if count is not None and x.dim() == 3:          # (in front of every allocation and launch)
        count = slot_counts("aggregate", count, x.shape[0], x.shape[1], x.device)
    x = _rd("aggregate", "x", x, dim=3)          # (its logits pass reads rows with 16-byte loads)
    B, M, D = x.shape
    if ca.k_w.weight.shape[1] != D or ca.v_w.weight.shape[1] != D:
        raise ValueError("aggregate: x has {} features, the attention's weights take {}".format(D, ca.k_w.weight.shape[1]))
    t = Transf()
    t.n_token, t.h, t.d, t.dk, t.dv, t.d_inner = ca.n_token, ca.H, D, ca.D_k, ca.D_v, mlp.w_1.out_features
    keep = []
    for name, src in (("q", ca.q[0]), ("wq", ca.q_w.weight), ("wk", ca.k_w.weight), ("wv", ca.v_w.weight),
                      ("fc", ca.fc.weight), ("ln1_g", ca.layer_norm.weight), ("ln1_b", ca.layer_norm.bias),
                      ("w1", mlp.w_1.weight), ("b1", mlp.w_1.bias), ("w2", mlp.w_2.weight),
                      ("b2", mlp.w_2.bias), ("ln2_g", mlp.layer_norm.weight), ("ln2_b", mlp.layer_norm.bias)):
        s = _f32(src.detach())
        keep.append(s)
        setattr(t, name, s.data_ptr())
    t.temperature = float(ca.attention.temperature)
    t.ln_eps = float(ca.layer_norm.eps)
    out = torch.empty((B, ca.n_token, D), dtype=torch.float32, device=x.device)
    nb = lib().ipsx_aggregate_workspace_bytes(C.byref(t), B, M)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=x.device)
    # the folded query and the packed V weights depend on the parameters only: kept by the attention module between calls
    vq = ca.folded_query() if hasattr(ca, "folded_query") else None
    if vq is not None and vq.dtype != torch.float32:       # (bf16 logits operand: the aggregation folds its own fp32 one)
        vq = None
    wvp = ca.packed_v() if hasattr(ca, "packed_v") else None
    if count is not None:
        _ck(lib().ipsx_aggregate_counted(C.byref(t), _p(vq), _p(wvp), _p(x), _p(count), B, M, _p(out), _p(ws), nb, _stream()),
            "ipsx_aggregate_counted")
        return out
    _ck(lib().ipsx_aggregate_packed(C.byref(t), _p(vq), _p(wvp), _p(x), B, M, _p(out), _p(ws), nb, _stream()),
        "ipsx_aggregate_packed")
    return out


def head(emb, token, linear, act):
    """act(Linear(emb[:, token])) with act in {'softmax', 'sigmoid'}: (B, T, D) -> (B, n_class)."""
    _one_gpu("head", emb=emb, weight=linear.weight, bias=linear.bias)
    emb = _rd("head", "emb", emb, dim=3, align=4)          # (head_kernel: 4-byte loads only)
    B, T, D = emb.shape
    w, b = _rd("head", "linear.weight", linear.weight.detach(), dim=2, align=4), _rd("head", "linear.bias", linear.bias.detach(), dim=1, align=4)
    if w.shape[1] != D or b.shape[0] != w.shape[0] or not 0 <= token < T or act not in ("softmax", "sigmoid"):
        raise ValueError("head: emb {} with token {}, act {!r} and a Linear of weight {} / bias {}".format(
            tuple(emb.shape), token, act, tuple(w.shape), tuple(b.shape)))
    out = torch.empty((B, w.shape[0]), dtype=torch.float32, device=emb.device)
    _ck(lib().ipsx_head(_p(emb), B, T, D, token, _p(w), _p(b), w.shape[0],
                        {"softmax": 0, "sigmoid": 1}[act], _p(out), _stream()), "ipsx_head")
    return out


# ------------------------------------------------------------------ the encoder plan and the training step's kernels
# (modules of their own since round 6; every name stays reachable as ``hip.<name>``)
from .hip_encoder import (EncoderPlan, _PlanHold, _bn_affine, _pack_conv, encoder_kernel_name)          # noqa: E402,F401
from .hip_train import (attn_pool_backward, attn_pool_forward, attn_pool_supported, PackJob, _BN_MAX_SLABS, _BN_WS_FLOATS, _CL, _PACK_BATCH_MAX, _WGRAD_MAX_BYTES, _bn_workspace_floats, _pack_conv_view, _rows_cl, bn_train_backward, bn_train_forward, bn_train_forward_partials, bn_train_supported, conv2d_nhwc, conv2d_nhwc_dgrad, conv2d_nhwc_wgrad, conv_lds_supported, conv_train_supported, maxpool_3x3s2_bwd_nhwc, maxpool_3x3s2_nhwc, maxpool_train_supported, pack_conv_views, projector_train_forward, projector_train_index_supported, projector_train_supported, projector_wgrad)          # noqa: E402,F401
