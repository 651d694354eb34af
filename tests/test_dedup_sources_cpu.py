"""Blank-patch dedup on every source of the counted launch, the part that needs no device: ``ips_amd.hip`` binds
``ipsx_trunk_encode_parts_dedup_u8`` / ``_view`` / ``_view_u8`` argument for argument as ``include/ipsx.h`` declares them, a
call with null pointers is refused under the entry's own name, and ``Selection.one_launch_dedup`` decides by
``IPSX_DEDUP_BLANK`` alone for each of the four kinds of source."""

import ctypes as C
import os
import re
import types

import pytest
import torch

from ips_amd import hip
from ips_amd.selection import Selection

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ipsx.h")
TAIL = [("const float*", "blank_emb"), ("void*", "workspace"), ("size_t", "workspace_bytes"), ("int32_t*", "n_encoded"),
        ("void*", "stream")]
# the export, its twin without dedup, its float32-tensor twin with dedup
NEW = [("ipsx_trunk_encode_parts_dedup_u8", "ipsx_trunk_encode_parts_u8"),
       ("ipsx_trunk_encode_parts_dedup_view", "ipsx_trunk_encode_parts_view"),
       ("ipsx_trunk_encode_parts_dedup_view_u8", "ipsx_trunk_encode_parts_view_u8")]

_CTYPES = {"const ipsx_trunk*": C.POINTER(hip.Trunk), "const ipsx_patch_view*": C.POINTER(hip.PatchViewStruct),
           "const int64_t*": C.POINTER(C.c_int64), "int64_t": C.c_int64, "int": C.c_int, "size_t": C.c_size_t,
           "const uint8_t*": C.c_void_p, "const float*": C.c_void_p, "const int32_t*": C.c_void_p, "float*": C.c_void_p,
           "int32_t*": C.c_void_p, "void*": C.c_void_p}


def declared(name):
    """(return type, [(type, name)]) of ``name`` in the header, comments stripped (the way tests/test_abi.py reads it)."""
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b(\w+)\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S)
    assert m, name
    args = []
    for a in m.group(2).split(","):
        typ, arg = re.match(r"\s*(.*?)\s*(\w+)\s*$", a, flags=re.S).groups()
        args.append((re.sub(r"\s+", " ", typ).replace(" *", "*"), arg))
    return m.group(1), args


@pytest.mark.parametrize("name,twin", NEW)
def test_binding_declares_the_new_exports_as_the_header_does(name, twin):
    ret, args = declared(name)
    assert ret == "int" and name in hip._EXPORTS
    restype, argtypes = hip._EXPORTS[name]
    assert restype is C.c_int
    assert [_CTYPES[t] for t, _ in args] == list(argtypes), args
    # the twin's list up to `done`, then the tail of ipsx_trunk_encode_parts_dedup
    _, twin_args = declared(twin)
    assert twin_args[-1] == ("void*", "stream")
    assert args == twin_args[:-1] + TAIL
    assert declared("ipsx_trunk_encode_parts_dedup")[1][-5:] == TAIL
    text = open(HEADER).read()
    assert re.search(name + r"\b", text[text.index(" *   3.06 "):text.index("#define IPSX_VERSION")])   # in the history block
    lib = hip.lib()
    assert lib.ipsx_version() == 306 and len(getattr(lib, name).argtypes) == len(args)


def test_the_existing_export_keeps_its_thirteen_arguments():
    _, args = declared("ipsx_trunk_encode_parts_dedup")
    assert len(args) == 13 and len(hip._EXPORTS["ipsx_trunk_encode_parts_dedup"][1]) == 13
    assert [a for _, a in args[:4]] == ["t", "patches", "index", "n_index"]


@pytest.mark.parametrize("name", [n for n, _ in NEW] + ["ipsx_trunk_encode_parts_dedup"])
def test_null_pointers_are_refused_under_the_entrys_name(name):
    """No device is touched: the null check is the entry's first."""
    lib = hip.lib()
    fn = getattr(lib, name)
    args = [0 if t in (C.c_int, C.c_int64, C.c_size_t) else None for t in fn.argtypes]
    assert fn(*args) != 0
    message = lib.ipsx_last_error().decode()
    assert message.startswith(name[len("ipsx_"):] + ":"), message


# ---------------------------------------------------------------- the switch
def source(dtype, view):
    """What ``one_launch_dedup`` reads of a ``hip.PatchSource``."""
    return types.SimpleNamespace(dtype=dtype, is_view=view, table=object() if dtype == torch.uint8 else None)


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8], ids=["float32", "uint8"])
@pytest.mark.parametrize("view", [False, True], ids=["patches", "view"])
def test_the_switch_decides_for_every_kind_of_source(view, dtype, monkeypatch):
    src = source(dtype, view)
    monkeypatch.delenv("IPSX_DEDUP_BLANK", raising=False)
    assert Selection.one_launch_dedup(src) is True                        # unset: dedup wherever the counted launch runs
    monkeypatch.setenv("IPSX_DEDUP_BLANK", "auto")
    assert Selection.one_launch_dedup(src) is True
    monkeypatch.setenv("IPSX_DEDUP_BLANK", "0")
    assert Selection.one_launch_dedup(src) is False                       # no dedup anywhere
    monkeypatch.setenv("IPSX_DEDUP_BLANK", "1")
    assert Selection.one_launch_dedup(src) is False                       # the explicit route's, which refuses bytes and views
    assert hip.dedup_blank()
