"""ABI 3.06: the row-indexed projector entry points and the indexed end of a call are declared in include/ipsx.h, exported
by libipsx.so and bound by ips_amd.hip with matching argument counts (no compute)."""

import ctypes
import os
import re

from ips_amd import hip

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ipsx.h")
NEW = ("ipsx_projector_stats_indexed", "ipsx_projector_apply_indexed", "ipsx_projector_apply_bf16_indexed",
       "ipsx_projector_stream_indexed", "ipsx_ips_finish_indexed")


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_version_is_3_06():
    assert re.search(r"#define\s+IPSX_VERSION\s+306\b", open(HEADER).read())
    lib = ctypes.CDLL(hip.library_path())
    assert lib.ipsx_version() == 306
    assert hip.lib().ipsx_version() // 100 == hip.ABI_MAJOR


def test_new_symbols_are_declared_exported_and_bound():
    text = header_text()
    lib = ctypes.CDLL(hip.library_path())
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name), name
        assert name in hip._EXPORTS, name


def test_header_and_ctypes_table_agree_on_the_new_signatures():
    """Argument count, and which arguments are pointers / 64-bit / 32-bit / float, per declaration."""
    text = header_text()
    kinds = {ctypes.c_void_p: "ptr", ctypes.c_int64: "i64", ctypes.c_int: "i32", ctypes.c_int32: "i32", ctypes.c_float: "f32",
             ctypes.c_size_t: "size"}
    for name in NEW:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name
        want = []
        for arg in m.group(1).split(","):
            arg = " ".join(arg.split())
            if "*" in arg:
                want.append("ptr")
            elif arg.startswith("int64_t"):
                want.append("i64")
            elif arg.startswith(("int32_t", "int ")):
                want.append("i32")
            elif arg.startswith("float"):
                want.append("f32")
            else:
                raise AssertionError("unexpected argument %r of %s" % (arg, name))
        res, args = hip._EXPORTS[name]
        got = ["ptr" if (a in (ctypes.c_void_p,) or hasattr(a, "contents")) else kinds[a] for a in args]
        assert res is ctypes.c_int and got == want, (name, got, want)


def test_existing_signatures_are_untouched():
    text = header_text()
    for name, n_args in (("ipsx_projector_stats_typed", 7), ("ipsx_projector_apply", 6), ("ipsx_projector_apply_publish", 8),
                         ("ipsx_projector_apply_bf16", 9), ("ipsx_projector_stream", 14), ("ipsx_ips_finish", 16)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m and len(m.group(1).split(",")) == n_args == len(hip._EXPORTS[name][1]), name
