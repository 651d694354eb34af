"""What the ``ipsx_trunk_encode*`` family - all twenty exports - and the float32 / uint8 twins ``ipsx_ragged_finish_view*``,
``ipsx_ragged_view_blank_flags*`` and ``ipsx_gather_patches_view*`` say when they refuse a call: the return code and the
whole ``ipsx_last_error()`` text, the export's own name included, for the first refusal of every export and for later ones.
Every case ends in a host-side refusal in front of any launch, so no GPU is needed.

The texts are part of the behaviour.  EXPECTED was recorded from the library of the commit BEFORE the exports were routed
through shared implementations (``python tests/test_export_refusals_cpu.py`` prints the table of whatever library is built),
so the siblings' accidental differences - "bad arguments" against "null pointer", the view exports' longer text, a twin that
answers under its sibling's name - are held as they were."""

import ctypes as C

import pytest

from ips_amd import hip

EINVAL, EWORKSPACE = -1, -3


def _aligned(nbytes, align=256):
    raw = (C.c_ubyte * (nbytes + align))()
    return raw, (C.addressof(raw) + align - 1) // align * align


_KEEP, A = _aligned(4096)                  # a buffer that is never read: every case is refused in front of any launch
ODD = A + 1
ENDS = (C.c_int64 * 1)(4)


def _conv(c_in, c_out, k, stride, pad):
    return hip.Conv(c_in, c_out, k, k, stride, pad, A, A, A, None, None)       # (weights that are never read; no tile16 packing)


def _fused_trunk(precision=0):
    """A trunk of the fused 1x32x32 shape whose weights are never read: enough for every check in front of a launch."""
    blocks = (hip.Block * 4)()
    for k, (ci, co, s) in enumerate([(64, 64, 1), (64, 64, 1), (64, 128, 2), (128, 128, 1)]):
        blocks[k].n_conv = 2
        blocks[k].conv[0], blocks[k].conv[1] = _conv(ci, co, 3, s, 1), _conv(co, co, 3, 1, 1)
    blocks[2].has_down, blocks[2].down = 1, _conv(64, 128, 1, 2, 0)
    t = hip.Trunk(1, 32, 32, _conv(1, 64, 7, 2, 3), 4, blocks, precision, 0)
    t._blocks = blocks
    return t


T0, TF, TF3 = hip.Trunk(), _fused_trunk(), _fused_trunk(precision=3)
PV = hip.PatchView((2, 1, 64, 64), (32, 32), (32, 32)).struct                 # 8 grid patches
PV_BAD = hip.PatchViewStruct(2, 1, 16, 64, 32, 32, 32, 32)                    # the patch is taller than the images


def _ragged(channels, device_table):
    rv = hip.RaggedView(channels, [(64, 64), (32, 96)], [0, channels * 4096], (32, 32), (32, 32))     # 4 + 3 packed patches
    if device_table:
        rv.struct.images = A               # (never read)
    return rv


_RV, _RVD, _RVD3 = _ragged(1, False), _ragged(1, True), _ragged(3, True)
RV, RVD, RVD3 = _RV.struct, _RVD.struct, _RVD3.struct
RV_EMPTY = hip.RaggedViewStruct(0, 1, 32, 32, 32, 32, None, None)

# (case, export, arguments)
CASES = [
    ("encode-null", "ipsx_trunk_encode", (None, None, 0, None, None, 0, None)),
    ("encode-args", "ipsx_trunk_encode", (TF, None, 4, A, None, 0, None)),
    ("encode-precision", "ipsx_trunk_encode", (TF3, A, 4, A, None, 0, None)),
    ("encode_u8-null", "ipsx_trunk_encode_u8", (None, None, None, 0, None, None, 0, None)),
    ("encode_u8-args", "ipsx_trunk_encode_u8", (TF, None, A, 4, A, None, 0, None)),
    ("encode_u8-precision", "ipsx_trunk_encode_u8", (TF3, A, A, 4, A, None, 0, None)),
    ("encode_u8-address", "ipsx_trunk_encode_u8", (TF, ODD, A, 4, A, None, 0, None)),
    ("encode_view-null", "ipsx_trunk_encode_view", (None, None, None, None, 0, 0, None, None, 0, None)),
    ("encode_view-first", "ipsx_trunk_encode_view", (TF, A, PV, None, -1, 4, A, None, 0, None)),
    ("encode_view-precision", "ipsx_trunk_encode_view", (TF3, A, PV, None, 0, 4, A, None, 0, None)),
    ("encode_view-range", "ipsx_trunk_encode_view", (TF, A, PV, None, 6, 4, A, None, 0, None)),
    ("encode_view-address", "ipsx_trunk_encode_view", (TF, ODD, PV, None, 0, 4, A, None, 0, None)),
    ("encode_view_u8-null", "ipsx_trunk_encode_view_u8", (None, None, None, None, None, 0, 0, None, None, 0, None)),
    ("encode_view_u8-table", "ipsx_trunk_encode_view_u8", (TF, A, None, PV, None, 0, 4, A, None, 0, None)),
    ("encode_view_u8-table-address", "ipsx_trunk_encode_view_u8", (TF, A, A + 4, PV, None, 0, 4, A, None, 0, None)),
    ("encode_view_u8-range", "ipsx_trunk_encode_view_u8", (TF, A, A, PV, None, 6, 4, A, None, 0, None)),
    ("encode_ragged_view-null", "ipsx_trunk_encode_ragged_view", (None, None, None, None, 0, 0, None, None, 0, None)),
    ("encode_ragged_view-precision", "ipsx_trunk_encode_ragged_view", (TF3, A, RV, None, 0, 4, A, None, 0, None)),
    ("encode_ragged_view-host-table", "ipsx_trunk_encode_ragged_view", (TF, A, RV_EMPTY, None, 0, 4, A, None, 0, None)),
    ("encode_ragged_view-device-table", "ipsx_trunk_encode_ragged_view", (TF, A, RV, None, 0, 4, A, None, 0, None)),
    ("encode_ragged_view-shape", "ipsx_trunk_encode_ragged_view", (TF, A, RVD3, None, 0, 4, A, None, 0, None)),
    ("encode_ragged_view-range", "ipsx_trunk_encode_ragged_view", (TF, A, RVD, None, 5, 4, A, None, 0, None)),
    ("encode_ragged_view_u8-null", "ipsx_trunk_encode_ragged_view_u8", (None, None, None, None, None, 0, 0, None, None, 0, None)),
    ("encode_ragged_view_u8-table", "ipsx_trunk_encode_ragged_view_u8", (TF, A, None, RVD, None, 0, 4, A, None, 0, None)),
    ("encode_ragged_view_u8-device-table", "ipsx_trunk_encode_ragged_view_u8", (TF, A, A, RV, None, 0, 4, A, None, 0, None)),
    ("encode_ragged_view_u8-range", "ipsx_trunk_encode_ragged_view_u8", (TF, A, A, RVD, None, 5, 4, A, None, 0, None)),
    ("indexed-null", "ipsx_trunk_encode_indexed", (None, None, None, 0, None, None)),
    ("indexed-count", "ipsx_trunk_encode_indexed", (TF, A, A, -1, A, None)),
    ("indexed-trunk", "ipsx_trunk_encode_indexed", (T0, A, A, 4, A, None)),
    ("indexed-precision", "ipsx_trunk_encode_indexed", (TF3, A, A, 4, A, None)),
    ("indexed_u8-null", "ipsx_trunk_encode_indexed_u8", (None, None, None, None, 0, None, None)),
    ("indexed_u8-table", "ipsx_trunk_encode_indexed_u8", (TF, A, None, A, 4, A, None)),
    ("indexed_u8-trunk", "ipsx_trunk_encode_indexed_u8", (T0, A, A, A, 4, A, None)),
    ("indexed_u8-precision", "ipsx_trunk_encode_indexed_u8", (TF3, A, A, A, 4, A, None)),
    ("indexed_u8-address", "ipsx_trunk_encode_indexed_u8", (TF, A + 4, A, A, 4, A, None)),
    ("parts-null", "ipsx_trunk_encode_parts", (None, None, None, 0, None, None, 0, None, None)),
    ("parts-trunk", "ipsx_trunk_encode_parts", (T0, A, A, 4, A, ENDS, 1, A, None)),
    ("parts-precision", "ipsx_trunk_encode_parts", (TF3, A, A, 4, A, ENDS, 1, A, None)),
    ("parts-count", "ipsx_trunk_encode_parts", (TF, A, A, 4, A, ENDS, 0, A, None)),
    ("parts-ends", "ipsx_trunk_encode_parts", (TF, A, A, 5, A, ENDS, 1, A, None)),
    ("parts-weights", "ipsx_trunk_encode_parts", (TF, A, A, 4, A, ENDS, 1, A, None)),
    ("parts_u8-null", "ipsx_trunk_encode_parts_u8", (None, None, None, None, 0, None, None, 0, None, None)),
    ("parts_u8-table", "ipsx_trunk_encode_parts_u8", (TF, A, None, A, 4, A, ENDS, 1, A, None)),
    ("parts_u8-trunk", "ipsx_trunk_encode_parts_u8", (T0, A, A, A, 4, A, ENDS, 1, A, None)),
    ("parts_u8-precision", "ipsx_trunk_encode_parts_u8", (TF3, A, A, A, 4, A, ENDS, 1, A, None)),
    ("parts_u8-address", "ipsx_trunk_encode_parts_u8", (TF, A, A + 4, A, 4, A, ENDS, 1, A, None)),
    ("parts_u8-count", "ipsx_trunk_encode_parts_u8", (TF, A, A, A, 4, A, ENDS, 0, A, None)),
    ("parts_view-null", "ipsx_trunk_encode_parts_view", (None, None, None, None, 0, None, None, 0, None, None)),
    ("parts_view-view", "ipsx_trunk_encode_parts_view", (TF, A, None, A, 4, A, ENDS, 1, A, None)),
    ("parts_view-trunk", "ipsx_trunk_encode_parts_view", (T0, A, PV, A, 4, A, ENDS, 1, A, None)),
    ("parts_view-precision", "ipsx_trunk_encode_parts_view", (TF3, A, PV, A, 4, A, ENDS, 1, A, None)),
    ("parts_view-geometry", "ipsx_trunk_encode_parts_view", (TF, A, PV_BAD, A, 4, A, ENDS, 1, A, None)),
    ("parts_view-count", "ipsx_trunk_encode_parts_view", (TF, A, PV, A, 4, A, ENDS, 17, A, None)),
    ("parts_view_u8-null", "ipsx_trunk_encode_parts_view_u8", (None, None, None, None, None, 0, None, None, 0, None, None)),
    ("parts_view_u8-table", "ipsx_trunk_encode_parts_view_u8", (TF, A, None, PV, A, 4, A, ENDS, 1, A, None)),
    ("parts_view_u8-trunk", "ipsx_trunk_encode_parts_view_u8", (T0, A, A, PV, A, 4, A, ENDS, 1, A, None)),
    ("parts_view_u8-table-address", "ipsx_trunk_encode_parts_view_u8", (TF, A, A + 4, PV, A, 4, A, ENDS, 1, A, None)),
    ("parts_view_u8-count", "ipsx_trunk_encode_parts_view_u8", (TF, A, A, PV, A, 4, A, ENDS, 0, A, None)),
    ("parts_dedup-null", "ipsx_trunk_encode_parts_dedup", (None, None, None, 0, None, None, 0, None, None, None, 0, None, None)),
    ("parts_dedup-blank", "ipsx_trunk_encode_parts_dedup", (TF, A, A, 4, A, ENDS, 1, A, None, A, 1 << 20, None, None)),
    ("parts_dedup-trunk", "ipsx_trunk_encode_parts_dedup", (T0, A, A, 4, A, ENDS, 1, A, A, A, 1 << 20, None, None)),
    ("parts_dedup-precision", "ipsx_trunk_encode_parts_dedup", (TF3, A, A, 4, A, ENDS, 1, A, A, A, 1 << 20, None, None)),
    ("parts_dedup-count", "ipsx_trunk_encode_parts_dedup", (TF, A, A, 4, A, ENDS, 0, A, A, A, 1 << 20, None, None)),
    ("parts_dedup-weights", "ipsx_trunk_encode_parts_dedup", (TF, A, A, 4, A, ENDS, 1, A, A, A, 1 << 20, None, None)),
    ("parts_dedup_u8-null", "ipsx_trunk_encode_parts_dedup_u8",
     (None, None, None, None, 0, None, None, 0, None, None, None, 0, None, None)),
    ("parts_dedup_u8-table", "ipsx_trunk_encode_parts_dedup_u8", (TF, A, None, A, 4, A, ENDS, 1, A, A, A, 1 << 20, None, None)),
    ("parts_dedup_u8-trunk", "ipsx_trunk_encode_parts_dedup_u8", (T0, A, A, A, 4, A, ENDS, 1, A, A, A, 1 << 20, None, None)),
    ("parts_dedup_u8-ends", "ipsx_trunk_encode_parts_dedup_u8", (TF, A, A, A, 5, A, ENDS, 1, A, A, A, 1 << 20, None, None)),
    ("parts_dedup_view-null", "ipsx_trunk_encode_parts_dedup_view",
     (None, None, None, None, 0, None, None, 0, None, None, None, 0, None, None)),
    ("parts_dedup_view-view", "ipsx_trunk_encode_parts_dedup_view", (TF, A, None, A, 4, A, ENDS, 1, A, A, A, 1 << 20, None, None)),
    ("parts_dedup_view-trunk", "ipsx_trunk_encode_parts_dedup_view", (T0, A, PV, A, 4, A, ENDS, 1, A, A, A, 1 << 20, None, None)),
    ("parts_dedup_view-count", "ipsx_trunk_encode_parts_dedup_view", (TF, A, PV, A, 4, A, ENDS, 17, A, A, A, 1 << 20, None, None)),
    ("parts_dedup_view_u8-null", "ipsx_trunk_encode_parts_dedup_view_u8",
     (None, None, None, None, None, 0, None, None, 0, None, None, None, 0, None, None)),
    ("parts_dedup_view_u8-table", "ipsx_trunk_encode_parts_dedup_view_u8",
     (TF, A, None, PV, A, 4, A, ENDS, 1, A, A, A, 1 << 20, None, None)),
    ("parts_dedup_view_u8-trunk", "ipsx_trunk_encode_parts_dedup_view_u8",
     (T0, A, A, PV, A, 4, A, ENDS, 1, A, A, A, 1 << 20, None, None)),
    ("parts_dedup_view_u8-precision", "ipsx_trunk_encode_parts_dedup_view_u8",
     (TF3, A, A, PV, A, 4, A, ENDS, 1, A, A, A, 1 << 20, None, None)),
    ("dedup-null", "ipsx_trunk_encode_dedup", (None, None, 0, None, None, 0, None, None)),
    ("dedup-args", "ipsx_trunk_encode_dedup", (TF, None, 4, A, None, 0, None, None)),
    ("dedup-trunk", "ipsx_trunk_encode_dedup", (T0, A, 4, A, None, 0, None, None)),
    ("dedup-many", "ipsx_trunk_encode_dedup", (TF, A, 1 << 31, A, None, 0, None, None)),
    ("dedup-precision", "ipsx_trunk_encode_dedup", (TF3, A, 4, A, None, 0, None, None)),
    ("dedup-workspace", "ipsx_trunk_encode_dedup", (TF, A, 4, A, A, 64, None, None)),
    ("dedup_flagged-null", "ipsx_trunk_encode_dedup_flagged", (None, None, 0, None, None, None, 0, None, None)),
    ("dedup_flagged-trunk-null", "ipsx_trunk_encode_dedup_flagged", (None, A, 4, A, A, None, 0, None, None)),
    ("dedup_flagged-args", "ipsx_trunk_encode_dedup_flagged", (TF, A, 4, A, None, None, 0, None, None)),
    ("dedup_flagged-workspace", "ipsx_trunk_encode_dedup_flagged", (TF, A, 4, A, A, None, 0, None, None)),
    ("ragged_view_dedup-null", "ipsx_trunk_encode_ragged_view_dedup", (None, None, None, None, 0, 0, None, None, 0, None, None)),
    ("ragged_view_dedup-args", "ipsx_trunk_encode_ragged_view_dedup", (TF, None, RVD, None, 0, 4, A, None, 0, None, None)),
    ("ragged_view_dedup-first", "ipsx_trunk_encode_ragged_view_dedup", (TF, A, RVD, A, -1, 4, A, None, 0, None, None)),
    ("ragged_view_dedup-many", "ipsx_trunk_encode_ragged_view_dedup", (TF, A, RVD, None, 0, 1 << 31, A, None, 0, None, None)),
    ("ragged_view_dedup-device-table", "ipsx_trunk_encode_ragged_view_dedup", (TF, A, RV, None, 0, 4, A, None, 0, None, None)),
    ("ragged_view_dedup-shape", "ipsx_trunk_encode_ragged_view_dedup", (TF, A, RVD3, None, 0, 4, A, None, 0, None, None)),
    ("ragged_view_dedup-range", "ipsx_trunk_encode_ragged_view_dedup", (TF, A, RVD, None, 5, 4, A, None, 0, None, None)),
    ("ragged_view_dedup-trunk", "ipsx_trunk_encode_ragged_view_dedup", (T0, A, RVD, None, 0, 4, A, None, 0, None, None)),
    ("ragged_view_dedup-weights", "ipsx_trunk_encode_ragged_view_dedup", (TF, A, RVD, None, 0, 4, A, None, 0, None, None)),
    ("ragged_view_dedup_u8-null", "ipsx_trunk_encode_ragged_view_dedup_u8",
     (None, None, None, None, None, 0, 0, None, None, 0, None, None)),
    ("ragged_view_dedup_u8-trunk-null", "ipsx_trunk_encode_ragged_view_dedup_u8", (None, A, A, RVD, None, 0, 4, A, None, 0, None, None)),
    ("ragged_view_dedup_u8-device-table", "ipsx_trunk_encode_ragged_view_dedup_u8", (TF, A, A, RV, None, 0, 4, A, None, 0, None, None)),
    ("ragged_view_dedup_u8-trunk", "ipsx_trunk_encode_ragged_view_dedup_u8", (T0, A, A, RVD, None, 0, 4, A, None, 0, None, None)),
    ("ragged_view_dedup_u8-table-address", "ipsx_trunk_encode_ragged_view_dedup_u8",
     (TF, A, A + 4, RVD, None, 0, 4, A, None, 0, None, None)),
    ("finish_view-null", "ipsx_ragged_finish_view", (None, None, None, None, 0, None, None, 0, None, None, None, None, None)),
    ("finish_view-host-table", "ipsx_ragged_finish_view", (A, RV_EMPTY, A, None, 4, None, None, 0, A, None, A, A, None)),
    ("finish_view-device-table", "ipsx_ragged_finish_view", (A, RV, A, None, 4, None, None, 0, A, None, A, A, None)),
    ("finish_view-address", "ipsx_ragged_finish_view", (ODD, RVD, A, None, 4, None, None, 0, A, None, A, A, None)),
    ("finish_view-pos", "ipsx_ragged_finish_view", (A, RVD, A, None, 4, None, A, 24, A, A, A, A, None)),
    ("finish_view_u8-null", "ipsx_ragged_finish_view_u8", (None, None, None, None, None, 0, None, None, 0, None, None, None, None, None)),
    ("finish_view_u8-args", "ipsx_ragged_finish_view_u8", (None, A, RVD, A, None, 4, None, None, 0, A, None, A, A, None)),
    ("finish_view_u8-device-table", "ipsx_ragged_finish_view_u8", (A, A, RV, A, None, 4, None, None, 0, A, None, A, A, None)),
    ("finish_view_u8-address", "ipsx_ragged_finish_view_u8", (ODD, A, RVD, A, None, 4, None, None, 0, ODD, None, A, A, None)),
    ("finish_view_u8-pos", "ipsx_ragged_finish_view_u8", (ODD, A, RVD, A, None, 4, None, A, 16, A, None, A, A, None)),
    ("blank_flags-null", "ipsx_ragged_view_blank_flags", (None, None, None, 0, 0, None, None)),
    ("blank_flags-many", "ipsx_ragged_view_blank_flags", (A, RVD, None, 0, 1 << 31, A, None)),
    ("blank_flags-device-table", "ipsx_ragged_view_blank_flags", (A, RV, None, 0, 4, A, None)),
    ("blank_flags-shape", "ipsx_ragged_view_blank_flags", (A, RVD3, None, 0, 4, A, None)),
    ("blank_flags-address", "ipsx_ragged_view_blank_flags", (ODD, RVD, None, 0, 4, A, None)),
    ("blank_flags-range", "ipsx_ragged_view_blank_flags", (A, RVD, None, 5, 4, A, None)),
    ("blank_flags-flags", "ipsx_ragged_view_blank_flags", (A, RVD, None, 0, 4, None, None)),
    ("blank_flags_u8-null", "ipsx_ragged_view_blank_flags_u8", (None, None, None, 0, 0, None, None)),
    ("blank_flags_u8-host-table", "ipsx_ragged_view_blank_flags_u8", (ODD, RV_EMPTY, None, 0, 4, A, None)),
    ("blank_flags_u8-range", "ipsx_ragged_view_blank_flags_u8", (ODD, RVD, None, 5, 4, A, None)),
    ("blank_flags_u8-flags", "ipsx_ragged_view_blank_flags_u8", (ODD, RVD, None, 0, 4, None, None)),
    ("gather_view-null", "ipsx_gather_patches_view", (None, None, None, 0, None, None)),
    ("gather_view-count", "ipsx_gather_patches_view", (A, PV, A, -1, A, None)),
    ("gather_view-geometry", "ipsx_gather_patches_view", (A, PV_BAD, A, 4, A, None)),
    ("gather_view-address", "ipsx_gather_patches_view", (ODD, PV, A, 4, A, None)),
    ("gather_view_u8-null", "ipsx_gather_patches_view_u8", (None, None, None, None, 0, None, None)),
    ("gather_view_u8-table", "ipsx_gather_patches_view_u8", (A, None, PV, A, 4, A, None)),
    ("gather_view_u8-geometry", "ipsx_gather_patches_view_u8", (ODD, A, PV_BAD, A, 4, A, None)),
    ("gather_view_u8-address", "ipsx_gather_patches_view_u8", (ODD, ODD, PV, A, 4, A, None)),
]

FAMILY = sorted(n for n in hip._EXPORTS if n.startswith("ipsx_trunk_encode")) + [
    "ipsx_ragged_finish_view", "ipsx_ragged_finish_view_u8", "ipsx_ragged_view_blank_flags", "ipsx_ragged_view_blank_flags_u8",
    "ipsx_gather_patches_view", "ipsx_gather_patches_view_u8"]

# case -> (return code, ipsx_last_error()), recorded from the commit in front of the shared implementations
EXPECTED = {
    'encode-null': (-1, 'trunk: missing blocks'),
    'encode-args': (-1, 'trunk_encode: bad arguments'),
    'encode-precision': (-1, 'trunk_encode: precision 3'),
    'encode_u8-null': (-1, 'trunk_encode_u8: no table'),
    'encode_u8-args': (-1, 'trunk_encode_u8: bad arguments'),
    'encode_u8-precision': (-1, 'trunk_encode_u8: precision 3'),
    'encode_u8-address': (-1, 'fused trunk: uint8 patches and their table must lie at 16-byte addresses'),
    'encode_view-null': (-1, 'trunk_encode_view: bad arguments'),
    'encode_view-first': (-1, 'trunk_encode_view: bad arguments'),
    'encode_view-precision': (-1, 'trunk_encode_view: precision 3'),
    'encode_view-range': (-1, 'trunk_encode_view: patches 6 .. 10 of a grid of 8'),
    'encode_view-address': (-1, 'trunk_encode_view: images must lie at a 4-byte address'),
    'encode_view_u8-null': (-1, 'trunk_encode_view_u8: bad arguments'),
    'encode_view_u8-table': (-1, 'trunk_encode_view_u8: bad arguments'),
    'encode_view_u8-table-address': (-1, 'trunk_encode_view_u8: the table of uint8 images must lie at a 16-byte address'),
    'encode_view_u8-range': (-1, 'trunk_encode_view_u8: patches 6 .. 10 of a grid of 8'),
    'encode_ragged_view-null': (-1, 'trunk_encode_ragged_view: bad arguments'),
    'encode_ragged_view-precision': (-1, 'trunk_encode_ragged_view: precision 3'),
    'encode_ragged_view-host-table': (-1,
        'trunk_encode_ragged_view: a ragged view needs a host table and positive b, c, patch and '
        'stride'),
    'encode_ragged_view-device-table': (-1, 'trunk_encode_ragged_view: no device table'),
    'encode_ragged_view-shape': (-1,
        'trunk_encode_ragged_view: the exact fp32 trunks whose stem stages its patch into LDS (1x32x32 fused, '
        '1x50x50, 3x100x100) on a ragged view of their patch shape (ipsx_trunk_ragged_view_supported)'),
    'encode_ragged_view-range': (-1, 'trunk_encode_ragged_view: packed patches 5 .. 9 of 7'),
    'encode_ragged_view_u8-null': (-1, 'trunk_encode_ragged_view_u8: bad arguments'),
    'encode_ragged_view_u8-table': (-1, 'trunk_encode_ragged_view_u8: bad arguments'),
    'encode_ragged_view_u8-device-table': (-1, 'trunk_encode_ragged_view_u8: no device table'),
    'encode_ragged_view_u8-range': (-1, 'trunk_encode_ragged_view_u8: packed patches 5 .. 9 of 7'),
    'indexed-null': (-1, 'trunk_encode_indexed: bad arguments'),
    'indexed-count': (-1, 'trunk_encode_indexed: bad arguments'),
    'indexed-trunk': (-1, 'trunk_encode_indexed: only the fused 1x32x32 trunk is supported'),
    'indexed-precision': (-1, 'trunk_encode_indexed: precision 3'),
    'indexed_u8-null': (-1, 'trunk_encode_indexed_u8: bad arguments'),
    'indexed_u8-table': (-1, 'trunk_encode_indexed_u8: bad arguments'),
    'indexed_u8-trunk': (-1, 'trunk_encode_indexed_u8: only the fused 1x32x32 trunk is supported'),
    'indexed_u8-precision': (-1, 'trunk_encode_indexed_u8: precision 3'),
    'indexed_u8-address': (-1, 'fused trunk: uint8 patches and their table must lie at 16-byte addresses'),
    'parts-null': (-1, 'trunk_encode_parts: null pointer'),
    'parts-trunk': (-1, 'trunk_encode_parts: only the fused 1x32x32 trunk is supported'),
    'parts-precision': (-1,
        'trunk_encode_parts: the exact fp32 trunk on float32 or uint8 patches only (precision 3, patch_dtype '
        '0)'),
    'parts-count': (-1, 'trunk_encode_parts: 0 parts (1 .. 16)'),
    'parts-ends': (-1, "trunk_encode_parts: part_end must increase and end on the list's length"),
    'parts-weights': (-1,
        'trunk_encode_parts: the exact fp32 trunk needs ipsx_pack_conv_weight_tile16 of its three 128 -> 128 '
        'convolutions in their w_packed_bf16'),
    'parts_u8-null': (-1, 'trunk_encode_parts_u8: null pointer'),
    'parts_u8-table': (-1, 'trunk_encode_parts_u8: null pointer'),
    'parts_u8-trunk': (-1, 'trunk_encode_parts_u8: only the fused 1x32x32 trunk is supported'),
    'parts_u8-precision': (-1, 'trunk_encode_parts_u8: precision 3'),
    'parts_u8-address': (-1, 'fused trunk: uint8 patches and their table must lie at 16-byte addresses'),
    'parts_u8-count': (-1, 'trunk_encode_parts: 0 parts (1 .. 16)'),
    'parts_view-null': (-1, 'trunk_encode_parts_view: null pointer'),
    'parts_view-view': (-1, 'trunk_encode_parts_view: null pointer'),
    'parts_view-trunk': (-1, 'trunk_encode_parts_view: the fused fp32 1x32x32 trunk on a valid view of 1x32x32 patches only'),
    'parts_view-precision': (-1, 'trunk_encode_parts_view: precision 3'),
    'parts_view-geometry': (-1,
        'trunk_encode_parts_view: the exact fp32 trunks whose stem stages its patch into LDS (1x32x32 fused, '
        '1x50x50, 3x100x100) on a valid view of their patch shape (ipsx_trunk_view_supported)'),
    'parts_view-count': (-1, 'trunk_encode_parts: 17 parts (1 .. 16)'),
    'parts_view_u8-null': (-1, 'trunk_encode_parts_view_u8: null pointer'),
    'parts_view_u8-table': (-1, 'trunk_encode_parts_view_u8: null pointer'),
    'parts_view_u8-trunk': (-1,
        'trunk_encode_parts_view_u8: the fused fp32 1x32x32 trunk on a valid view of 1x32x32 patches '
        'only'),
    'parts_view_u8-table-address': (-1, 'trunk_encode_parts_view_u8: the table of uint8 images must lie at a 16-byte address'),
    'parts_view_u8-count': (-1, 'trunk_encode_parts: 0 parts (1 .. 16)'),
    'parts_dedup-null': (-1, 'trunk_encode_parts_dedup: null pointer'),
    'parts_dedup-blank': (-1, 'trunk_encode_parts_dedup: null pointer'),
    'parts_dedup-trunk': (-1, 'trunk_encode_parts_dedup: only the fused 1x32x32 trunk is supported'),
    'parts_dedup-precision': (-1,
        'trunk_encode_parts_dedup: blank-patch detection reads float32 or uint8 patches, on the exact fp32 '
        'trunk'),
    'parts_dedup-count': (-1, 'trunk_encode_parts_dedup: 0 parts (1 .. 16)'),
    'parts_dedup-weights': (-1,
        'trunk_encode_parts_dedup: the exact fp32 trunk needs ipsx_pack_conv_weight_tile16 of its three 128 -> '
        '128 convolutions in their w_packed_bf16'),
    'parts_dedup_u8-null': (-1, 'trunk_encode_parts_dedup_u8: null pointer'),
    'parts_dedup_u8-table': (-1, 'trunk_encode_parts_dedup_u8: null pointer'),
    'parts_dedup_u8-trunk': (-1, 'trunk_encode_parts_dedup_u8: only the fused 1x32x32 trunk is supported'),
    'parts_dedup_u8-ends': (-1, "trunk_encode_parts_dedup_u8: part_end must increase and end on the list's length"),
    'parts_dedup_view-null': (-1, 'trunk_encode_parts_dedup_view: null pointer'),
    'parts_dedup_view-view': (-1, 'trunk_encode_parts_dedup_view: null pointer'),
    'parts_dedup_view-trunk': (-1, 'trunk_encode_parts_dedup_view: only the fused 1x32x32 trunk is supported'),
    'parts_dedup_view-count': (-1, 'trunk_encode_parts_dedup_view: 17 parts (1 .. 16)'),
    'parts_dedup_view_u8-null': (-1, 'trunk_encode_parts_dedup_view_u8: null pointer'),
    'parts_dedup_view_u8-table': (-1, 'trunk_encode_parts_dedup_view_u8: null pointer'),
    'parts_dedup_view_u8-trunk': (-1, 'trunk_encode_parts_dedup_view_u8: only the fused 1x32x32 trunk is supported'),
    'parts_dedup_view_u8-precision': (-1,
        'trunk_encode_parts_dedup_view_u8: blank-patch detection reads float32 or uint8 patches, on the exact '
        'fp32 trunk'),
    'dedup-null': (-1, 'trunk_encode_dedup: blank-patch detection reads float32 patches'),
    'dedup-args': (-1, 'trunk_encode_dedup: bad arguments'),
    'dedup-trunk': (-1, 'trunk_encode_dedup: only the fused 1x32x32 trunk is supported'),
    'dedup-many': (-1, 'trunk_encode_dedup: too many patches'),
    'dedup-precision': (-1, 'trunk_encode_dedup: precision 3'),
    'dedup-workspace': (-3, 'trunk_encode_dedup: workspace 64 B < 3120 B'),
    'dedup_flagged-null': (-1, 'trunk_encode_dedup_flagged: no flags'),
    'dedup_flagged-trunk-null': (-1, 'trunk_encode_dedup: blank-patch detection reads float32 patches'),
    'dedup_flagged-args': (-1, 'trunk_encode_dedup: bad arguments'),
    'dedup_flagged-workspace': (-3, 'trunk_encode_dedup: workspace 0 B < 3120 B'),
    'ragged_view_dedup-null': (-1, 'trunk_encode_ragged_view_dedup: null pointer'),
    'ragged_view_dedup-args': (-1, 'trunk_encode_ragged_view_dedup: bad arguments'),
    'ragged_view_dedup-first': (-1, 'trunk_encode_ragged_view_dedup: bad arguments'),
    'ragged_view_dedup-many': (-1, 'trunk_encode_ragged_view_dedup: too many entries'),
    'ragged_view_dedup-device-table': (-1, 'trunk_encode_ragged_view_dedup: no device table'),
    'ragged_view_dedup-shape': (-1,
        "trunk_encode_ragged_view_dedup: blank-patch detection reads the 1x32x32 patches of the fused trunk, the "
        "view's are 3x32x32"),
    'ragged_view_dedup-range': (-1, 'trunk_encode_ragged_view_dedup: packed patches 5 .. 9 of 7'),
    'ragged_view_dedup-trunk': (-1, 'trunk_encode_ragged_view_dedup: the exact fp32 fused 1x32x32 trunk only'),
    'ragged_view_dedup-weights': (-1,
        'trunk_encode_ragged_view_dedup: the exact fp32 trunk needs ipsx_pack_conv_weight_tile16 of its three 128 '
        '-> 128 convolutions in their w_packed_bf16'),
    'ragged_view_dedup_u8-null': (-1, 'trunk_encode_ragged_view_dedup_u8: no table'),
    'ragged_view_dedup_u8-trunk-null': (-1, 'trunk_encode_ragged_view_dedup_u8: null pointer'),
    'ragged_view_dedup_u8-device-table': (-1, 'trunk_encode_ragged_view_dedup_u8: no device table'),
    'ragged_view_dedup_u8-trunk': (-1, 'trunk_encode_ragged_view_dedup_u8: the exact fp32 fused 1x32x32 trunk only'),
    'ragged_view_dedup_u8-table-address': (-1,
        'trunk_encode_ragged_view_dedup_u8: the table of uint8 images must lie at a 16-byte '
        'address'),
    'finish_view-null': (-1, 'ragged_finish_view: bad arguments'),
    'finish_view-host-table': (-1, 'ragged_finish_view: a ragged view needs a host table and positive b, c, patch and stride'),
    'finish_view-device-table': (-1, 'ragged_finish_view: a device table of at most 65535 images'),
    'finish_view-address': (-1, 'ragged_finish_view: pixels and mem_patch at 4-byte addresses'),
    'finish_view-pos': (-1, 'ragged_finish_view: positional rows of 16-byte units'),
    'finish_view_u8-null': (-1, 'ragged_finish_view_u8: no table'),
    'finish_view_u8-args': (-1, 'ragged_finish_view: bad arguments'),
    'finish_view_u8-device-table': (-1, 'ragged_finish_view: a device table of at most 65535 images'),
    'finish_view_u8-address': (-1, 'ragged_finish_view: pixels and mem_patch at 4-byte addresses'),
    'finish_view_u8-pos': (-1, 'ragged_finish_view: positional rows of 16-byte units'),
    'blank_flags-null': (-1, 'ragged_view_blank_flags: bad arguments'),
    'blank_flags-many': (-1, 'ragged_view_blank_flags: too many entries'),
    'blank_flags-device-table': (-1, 'ragged_view_blank_flags: no device table'),
    'blank_flags-shape': (-1,
        "ragged_view_blank_flags: blank-patch detection reads the 1x32x32 patches of the fused trunk, the view's "
        "are 3x32x32"),
    'blank_flags-address': (-1, 'ragged_view_blank_flags: images must lie at a 4-byte address'),
    'blank_flags-range': (-1, 'ragged_view_blank_flags: packed patches 5 .. 9 of 7'),
    'blank_flags-flags': (-1, 'ragged_view_blank_flags: no flags'),
    'blank_flags_u8-null': (-1, 'ragged_view_blank_flags_u8: bad arguments'),
    'blank_flags_u8-host-table': (-1,
        'ragged_view_blank_flags_u8: a ragged view needs a host table and positive b, c, patch and '
        'stride'),
    'blank_flags_u8-range': (-1, 'ragged_view_blank_flags_u8: packed patches 5 .. 9 of 7'),
    'blank_flags_u8-flags': (-1, 'ragged_view_blank_flags_u8: no flags'),
    'gather_view-null': (-1, 'gather_patches_view: bad arguments'),
    'gather_view-count': (-1, 'gather_patches_view: bad arguments'),
    'gather_view-geometry': (-1, 'gather_patches_view: images 2x1x16x64, patch 32x32, stride 32x32'),
    'gather_view-address': (-1, 'gather_patches_view: images and out must lie at 4-byte addresses'),
    'gather_view_u8-null': (-1, 'gather_patches_view_u8: bad arguments'),
    'gather_view_u8-table': (-1, 'gather_patches_view_u8: bad arguments'),
    'gather_view_u8-geometry': (-1, 'gather_patches_view_u8: images 2x1x16x64, patch 32x32, stride 32x32'),
    'gather_view_u8-address': (-1, 'gather_patches_view_u8: table and out must lie at 4-byte addresses'),
}


def refusal(export, args):
    lib = hip.lib()
    fn = getattr(lib, export)
    args = [C.byref(a) if isinstance(a, C.Structure) else a for a in args]
    rc = fn(*args)
    return rc, lib.ipsx_last_error().decode()


def test_the_table_covers_the_family_first_refusal_and_a_later_one():
    assert len(FAMILY) == 26 and len([n for n in FAMILY if n.startswith("ipsx_trunk_encode")]) == 20
    assert sorted(EXPECTED) == sorted(c for c, _, _ in CASES) and len(EXPECTED) == len(CASES)
    for name in FAMILY:
        cases = [c for c, n, _ in CASES if n == name]
        assert len(cases) >= 2 and cases[0].endswith("-null"), name
        assert len({EXPECTED[c][1] for c in cases}) >= 2, name                # (a later refusal: another text)


@pytest.mark.parametrize("case,export,args", CASES, ids=[c for c, _, _ in CASES])
def test_refusal_code_and_text(case, export, args):
    assert refusal(export, args) == EXPECTED[case]


if __name__ == "__main__":
    print("EXPECTED = {")
    for case, export, args in CASES:
        print("    %r: %r," % (case, refusal(export, args)))
    print("}")
