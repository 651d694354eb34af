"""uint8 images for ``ips_image`` without a GPU: the CPU path (stock ops on the unfolded bytes) against the float32 images the
table stands for, the two 3.06 exports of the view over bytes, and the refusals that need no device."""

import ctypes
import os
import re

import pytest
import torch

from ips_amd import hip, quant, synth
from ips_amd.architecture import IPSNet
from view_cases import FUSED, POOL50, POOL100, grid
from view_u8_cases import TIERS, expected_tier, guarded_images_u8, plain_table

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ipsx.h")
NEW = ("ipsx_trunk_encode_view_u8", "ipsx_gather_patches_view_u8")


def _cpu_net(**over):
    conf = synth.mnist_conf(N=24, M=4, I=6, **over)
    return synth.fill_weights(IPSNet(torch.device("cpu"), conf), 3).eval()


def _bytes(seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (2, 1, 80, 112), dtype=torch.uint8, generator=g)   # 32-px patches at stride 16: 24 per image


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and torch.equal(a, b))


@pytest.mark.parametrize("style", [None, "batch", "instance"])
def test_cpu_ips_image_on_bytes_equals_ips_image_on_the_dequantised_images(style):
    over = {} if style is None else dict(shuffle=True, shuffle_style=style)
    net = _cpu_net(**over)
    table = plain_table(1)
    net.set_patch_table(table)
    x = _bytes()
    torch.manual_seed(11)
    want = net.ips_image(quant.dequant(x, table), (32, 32), (16, 16))
    want_left = (net.last_mem_idx, net.last_mem_emb, net.last_shuffle)
    torch.manual_seed(11)
    got = net.ips_image(x, (32, 32), (16, 16))
    assert got[0].shape == (2, 4, 1, 32, 32) and got[0].dtype == torch.float32
    for a, b in zip(got + (net.last_mem_idx, net.last_mem_emb, net.last_shuffle), want + want_left):
        assert _same(a, b)
    assert (net.last_shuffle is not None) == (style is not None)


def test_cpu_nothing_to_select_returns_the_dequantised_patches():
    net = _cpu_net()
    table = plain_table(1)
    net.set_patch_table(table)
    x = _bytes()[:, :, :64, :64]                                 # 2 x 2 = 4 patches: M >= N
    got, want = net.ips_image(x, (32, 32), (32, 32)), net.ips_image(quant.dequant(x, table), (32, 32), (32, 32))
    assert got[0].dtype == torch.float32 and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_refusals_need_no_device(monkeypatch):
    x = _bytes()
    view = hip.PatchView(x.shape, (32, 32), (16, 16))
    table = plain_table(1)
    src = hip.PatchSource(images=x, view=view, table=table)
    assert src.dtype == torch.uint8 and src.shape == (2, 24, 1, 32, 32) and src.count == 48 and src.is_view
    with pytest.raises(TypeError, match="dequantisation table"):
        hip.PatchSource(images=x, view=view)
    with pytest.raises(TypeError, match="dequantisation table"):
        _cpu_net().ips_image(x, (32, 32), (16, 16))
    with pytest.raises(TypeError, match="patch table goes with uint8"):
        hip.PatchSource(images=quant.dequant(x, table), view=view, table=table)      # a table with float32 images
    with pytest.raises(TypeError, match="patch table goes with uint8"):
        view.check(quant.dequant(x, table), table)
    with pytest.raises(ValueError):
        hip.PatchSource(images=x, view=view, table=plain_table(3))                   # channel count
    with pytest.raises(ValueError):
        hip.PatchSource(images=x[:1], view=view, table=table)                        # another shape than the view's
    monkeypatch.setenv("IPSX_DEDUP_BLANK", "1")
    with pytest.raises(TypeError, match="dedup"):
        hip.PatchSource(images=x, view=view, table=table)
    monkeypatch.delenv("IPSX_DEDUP_BLANK")
    monkeypatch.setenv("IPSX_PRECISION", "bf16")
    with pytest.raises(TypeError, match="IPSX_PRECISION"):
        hip.PatchSource(images=x, view=view, table=table)


@pytest.mark.parametrize("kind,cases", [("fused", FUSED), ("pair", FUSED), ("pool50", POOL50), ("pool100", POOL100)])
def test_load_width_rule_on_host_pointers(kind, cases):
    """``PatchView.load_bytes`` (the launchers' rule, view_args) on real addresses k bytes past a 16-byte boundary."""
    for g in cases:
        for k in (0, 1, 2, 4, 8):
            images = guarded_images_u8(g, k)
            assert images.data_ptr() % 16 == k % 16
            view = hip.PatchView(images.shape, g[4], g[5])
            assert view.load_bytes(images, TIERS[kind]) == expected_tier(kind, g, k)
            assert view.per_image == grid(g)[0] * grid(g)[1]
    # float32 images: the one wide load, or 0 = dwords
    f = torch.zeros((1, 1, 96, 128))
    view = hip.PatchView(f.shape, (32, 32), (32, 32))
    assert view.load_bytes(f, (16,)) == (16 if f.data_ptr() % 16 == 0 else 0)
    assert hip.PatchView((1, 1, 100, 117), (32, 32), (24, 20)).load_bytes(torch.zeros((1, 1, 100, 117)), (16,)) == 0


# ---------------------------------------------------------------- ABI 3.06
def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_version_stays_3_06():
    assert re.search(r"#define\s+IPSX_VERSION\s+306\b", open(HEADER).read())
    assert ctypes.CDLL(hip.library_path()).ipsx_version() == 306
    assert hip.lib().ipsx_version() == 306


def test_new_symbols_are_declared_exported_and_bound_alike():
    """Argument count, and which arguments are pointers / 64-bit / 32-bit / size_t, per declaration."""
    text = header_text()
    lib = ctypes.CDLL(hip.library_path())
    kinds = {ctypes.c_int64: "i64", ctypes.c_int: "i32", ctypes.c_int32: "i32", ctypes.c_float: "f32", ctypes.c_size_t: "size"}
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in hip._EXPORTS, name
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
            elif arg.startswith("size_t"):
                want.append("size")
            else:
                raise AssertionError("unexpected argument %r of %s" % (arg, name))
        res, args = hip._EXPORTS[name]
        got = ["ptr" if (a is ctypes.c_void_p or hasattr(a, "contents")) else kinds[a] for a in args]
        assert res is ctypes.c_int and got == want, (name, got, want)
    # the struct keeps its layout: the element type travels in which export is called
    assert ctypes.sizeof(hip.PatchViewStruct) == 32
    m = re.search(r"typedef struct ipsx_patch_view \{(.*?)\} ipsx_patch_view;", text, re.S)
    assert m and "".join(m.group(1).split()) == "intb,c,h,w;intph,pw,sh,sw;"
