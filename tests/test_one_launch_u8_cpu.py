"""uint8 sources on the fused trunk's one counted launch, the part that needs no device: ``Selection.one_launch_ok``
answers for a uint8 source (patch tensor or view) what it answers for a float32 one under ``IPSX_ONE_LAUNCH_U8=1`` - the
route for bytes ships behind that switch - and keeps every refusal, and
``ips_amd.hip`` binds ``ipsx_trunk_encode_parts_u8`` / ``ipsx_trunk_encode_parts_view_u8`` argument for argument as
``include/ipsx.h`` declares them."""

import ctypes as C
import os
import re
import types

import pytest
import torch

from ips_amd import hip
from ips_amd.selection import Selection

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ipsx.h")


def source(dtype, view=False, count=16 * 2500):
    """What ``one_launch_ok`` reads of a ``hip.PatchSource``."""
    return types.SimpleNamespace(dtype=dtype, count=count, device=torch.device("cpu"), is_view=view,
                                 table=object() if dtype == torch.uint8 else None)


VQ = types.SimpleNamespace(dtype=torch.float32)


@pytest.fixture
def sel(monkeypatch):
    monkeypatch.setattr(hip, "persistent_ok", lambda dev: True)
    monkeypatch.setenv("IPSX_PRECISION", "fp32")
    monkeypatch.delenv("IPSX_ONE_LAUNCH", raising=False)
    monkeypatch.setenv("IPSX_ONE_LAUNCH_U8", "1")            # (the route for bytes sits behind it: DESIGN 2.3)
    return Selection.__new__(Selection)                      # (the answer reads its arguments and the environment only)


def ok(sel, src, fused=True, small=False, vq=VQ, P=4):
    return bool(sel.one_launch_ok(src, fused, small, vq, P))


@pytest.mark.parametrize("view", [False, True], ids=["patches", "view"])
def test_uint8_sources_are_admitted_where_float32_sources_are(sel, view):
    f32, u8 = source(torch.float32, view), source(torch.uint8, view)
    assert ok(sel, f32)
    assert ok(sel, u8)
    for P in (2, 16):
        assert ok(sel, u8, P=P) and ok(sel, f32, P=P)
    for kw in (dict(P=1), dict(P=17), dict(small=True), dict(fused=False), dict(vq=types.SimpleNamespace(dtype=torch.float16))):
        assert not ok(sel, u8, **kw) and not ok(sel, f32, **kw), kw
    assert not ok(sel, source(torch.float16, view))
    assert not ok(sel, source(torch.uint8, view, count=(1 << 31) - 16))
    assert not ok(sel, None)


def test_the_switch_and_the_precision_hold_for_bytes(sel, monkeypatch):
    u8 = source(torch.uint8)
    for off in ("0", None):                                  # the new switch, and what ships without it: off for bytes only
        monkeypatch.setenv("IPSX_ONE_LAUNCH_U8", off) if off else monkeypatch.delenv("IPSX_ONE_LAUNCH_U8")
        assert not ok(sel, u8) and not ok(sel, source(torch.uint8, view=True)) and ok(sel, source(torch.float32))
    monkeypatch.setenv("IPSX_ONE_LAUNCH_U8", "1")
    monkeypatch.setenv("IPSX_ONE_LAUNCH", "0")
    assert not ok(sel, u8) and not ok(sel, source(torch.float32))
    monkeypatch.setenv("IPSX_ONE_LAUNCH", "1")
    assert ok(sel, u8)
    for precision in ("bf16", "fp32x3"):
        monkeypatch.setenv("IPSX_PRECISION", precision)
        assert not ok(sel, u8), precision
    monkeypatch.setenv("IPSX_PRECISION", "fp32")
    monkeypatch.setattr(hip, "persistent_ok", lambda dev: False)
    assert not ok(sel, u8)


# ---------------------------------------------------------------- the two exports, header against binding
_CTYPES = {"const ipsx_trunk*": C.POINTER(hip.Trunk), "const ipsx_patch_view*": C.POINTER(hip.PatchViewStruct),
           "const int64_t*": C.POINTER(C.c_int64), "int64_t": C.c_int64, "int": C.c_int,
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


@pytest.mark.parametrize("name,twin,extra", [("ipsx_trunk_encode_parts_u8", "ipsx_trunk_encode_parts", {2: ("const float*", "table")}),
                                             ("ipsx_trunk_encode_parts_view_u8", "ipsx_trunk_encode_parts_view", {2: ("const float*", "table")})])
def test_binding_declares_the_new_exports_as_the_header_does(name, twin, extra):
    ret, args = declared(name)
    assert ret == "int" and name in hip._EXPORTS
    restype, argtypes = hip._EXPORTS[name]
    assert restype is C.c_int
    assert [_CTYPES[t] for t, _ in args] == list(argtypes), args
    # the float32 twin's list with the bytes and their table: (t, patches | images, table, ...)
    _, twin_args = declared(twin)
    for at, what in extra.items():
        twin_args.insert(at, what)
    twin_args[1] = ("const uint8_t*", twin_args[1][1])
    assert args == twin_args
    text = open(HEADER).read()
    assert name in text[text.index(" *   3.06 "):text.index("#define IPSX_VERSION")]       # listed in the history block
    lib = hip.lib()
    assert lib.ipsx_version() == 306 and len(getattr(lib, name).argtypes) == len(args)
