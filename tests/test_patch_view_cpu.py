"""The patch-grid view without a GPU: the address arithmetic every view kernel uses (ipsx_patch_view_offset is the host
export of the inline the kernels share), the ABI additions, and ``IPSNet.ips_image`` / ``SparseImages.image`` on the CPU."""

import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from ips_amd import hip, synth
from ips_amd.architecture import IPSNet
from view_cases import ALL, geom_id, grid, unfold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ipsx.h")
NEW = ("ipsx_patch_view_offset", "ipsx_trunk_view_supported", "ipsx_trunk_encode_view", "ipsx_trunk_encode_parts_view",
       "ipsx_gather_patches_view")


@pytest.mark.parametrize("g", ALL, ids=geom_id)
def test_offsets_agree_with_unfold_and_stay_inside_the_images(g):
    """Every patch of every geometry: the C export and PatchView.origin name the element where unfold puts the patch's
    first pixel, and every element of the patch lies inside [0, b c h w)."""
    b, c, h, w, (ph, pw), (sh, sw) = g
    view = hip.PatchView((b, c, h, w), (ph, pw), (sh, sw))
    ny, nx = grid(g)
    assert (view.ny, view.nx, view.count) == (ny, nx, b * ny * nx)
    total = b * c * h * w
    # an image whose every element holds its own flat offset: unfold then SHOWS where each patch element comes from
    # (float64: exact for every offset of these sizes)
    where = unfold(torch.arange(total, dtype=torch.float64).view(b, c, h, w), (ph, pw), (sh, sw)).reshape(-1, c, ph, pw)
    assert where.shape[0] == view.count
    off = hip.lib().ipsx_patch_view_offset
    ch, yy, xx = np.meshgrid(np.arange(c), np.arange(ph), np.arange(pw), indexing="ij")
    rel = (ch * h + yy) * w + xx
    for p in range(view.count):
        o = off(C.byref(view.struct), p)
        assert o == view.origin(p) == int(where[p, 0, 0, 0])
        assert 0 <= o and o + int(rel.max()) < total
        if p % 97 == 0 or p == view.count - 1:                 # the whole patch, element by element
            assert np.array_equal(where[p].numpy(), (o + rel).astype(np.float64))
    for bad in (-1, view.count, view.count + 5, 1 << 40):
        assert off(C.byref(view.struct), bad) == -1 and view.origin(bad) == -1


def test_invalid_geometries_have_no_patches():
    off = hip.lib().ipsx_patch_view_offset
    ok = dict(b=1, c=1, h=64, w=64, ph=32, pw=32, sh=32, sw=32)
    assert off(C.byref(hip.PatchViewStruct(**ok)), 3) == 64 * 32 + 32
    for k, v in (("b", 0), ("c", 0), ("ph", 0), ("pw", -1), ("sh", 0), ("sw", 0), ("ph", 65), ("pw", 65), ("h", 0)):
        assert off(C.byref(hip.PatchViewStruct(**dict(ok, **{k: v}))), 0) == -1, (k, v)
    # 2^31 patches and more: int32 index lists cannot name them
    assert off(C.byref(hip.PatchViewStruct(b=1 << 20, c=1, h=1500, w=1500, ph=32, pw=32, sh=32, sw=32)), 0) == -1
    assert off(None, 0) == -1
    with pytest.raises(ValueError):
        hip.PatchView((1, 1, 20, 64), (32, 32), (32, 32))
    with pytest.raises(ValueError):
        hip.PatchView((1, 1, 64, 64), (32, 32), (0, 32))


def test_view_supported_is_zero_for_a_null_or_mismatched_view():
    L = hip.lib()
    assert L.ipsx_trunk_view_supported(None, None) == 0
    t = hip.Trunk()
    t.c_in, t.h, t.w = 1, 32, 32
    assert L.ipsx_trunk_view_supported(C.byref(t), C.byref(hip.PatchViewStruct(1, 1, 64, 64, 50, 50, 7, 7))) == 0


# ---------------------------------------------------------------- ABI
def _header():
    return open(HEADER).read()


def test_new_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(ipsx_[a-z0-9_]+)\s*\(", text))
    lib = C.CDLL(hip.library_path())
    for s in NEW:
        assert s in declared and hasattr(lib, s) and s in hip._EXPORTS, s
    assert "typedef struct ipsx_patch_view" in text
    assert C.sizeof(hip.PatchViewStruct) == 8 * C.sizeof(C.c_int)
    assert [f[0] for f in hip.PatchViewStruct._fields_] == ["b", "c", "h", "w", "ph", "pw", "sh", "sw"]


def test_version_stays_306_and_the_history_lists_the_new_names():
    text = _header()
    assert re.search(r"#define IPSX_VERSION 306\b", text)
    assert hip.lib().ipsx_version() == 306
    block = text[text.index(" *   3.06 "):text.index("#define IPSX_VERSION")]
    for s in NEW + ("ipsx_patch_view (struct)",):
        assert s in block, s


def test_a_c_program_with_the_new_struct_links(tmp_path):
    """include/ipsx.h through gcc -std=c11 -pedantic, the new struct and its host entry point called from C."""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "abi_view.c"
    src.write_text(r'''
#include <stdio.h>
#include "ipsx.h"
int main(void) {
    ipsx_patch_view v = {2, 3, 200, 301, 100, 100, 100, 67};
    ipsx_trunk tr = {0};
    if (ipsx_version() != IPSX_VERSION) return 1;
    if (ipsx_patch_view_offset(&v, 0) != 0) return 2;
    if (ipsx_patch_view_offset(&v, 6) != (int64_t)100 * 301 + 2 * 67) return 3;              /* py = 1, px = 2 of 2 x 4 */
    if (ipsx_patch_view_offset(&v, 8) != (int64_t)3 * 200 * 301) return 4;                   /* the second image */
    if (ipsx_patch_view_offset(&v, 16) != -1 || ipsx_patch_view_offset(&v, -1) != -1) return 5;
    if (ipsx_patchify_count(200, 301, 100, 100, 100, 67) != 8) return 6;
    if (ipsx_trunk_view_supported(&tr, &v) != 0) return 7;
    printf("abi ok %d\n", ipsx_version());
    return 0;
}
''')
    exe = tmp_path / "abi_view"
    libdir = os.path.dirname(hip.library_path())
    subprocess.check_call(["gcc", "-std=c11", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe), "-L", libdir, "-lipsx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("abi ok"), (out.returncode, out.stdout, out.stderr)


# ---------------------------------------------------------------- the CPU path of ips_image
def _cpu_net(**over):
    conf = synth.mnist_conf(N=24, M=4, I=6, **over)
    return synth.fill_weights(IPSNet(torch.device("cpu"), conf), 3).eval()


def _images(seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((2, 1, 80, 112), generator=g)            # 32-px patches at stride 16: 4 x 6 = 24 per image


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and torch.equal(a, b))


@pytest.mark.parametrize("style", [None, "batch", "instance"])
def test_cpu_ips_image_equals_ips_of_the_unfolded_images(style):
    over = {} if style is None else dict(shuffle=True, shuffle_style=style)
    net = _cpu_net(**over)
    x = _images()
    torch.manual_seed(11)
    want = net.ips(unfold(x, (32, 32), (16, 16)))
    want_left = (net.last_mem_idx, net.last_mem_emb, net.last_shuffle)
    torch.manual_seed(11)
    got = net.ips_image(x, (32, 32), (16, 16))
    assert want[0].shape == (2, 4, 1, 32, 32)
    for a, b in zip(got + (net.last_mem_idx, net.last_mem_emb, net.last_shuffle), want + want_left):
        assert _same(a, b)
    assert (net.last_shuffle is not None) == (style is not None)


def test_cpu_ips_image_shortcut_and_refusals():
    net = _cpu_net()
    x = _images()[:, :, :64, :64]                                # 2 x 2 = 4 patches: M >= N, nothing to select
    got, want = net.ips_image(x, (32, 32), (32, 32)), net.ips(unfold(x, (32, 32), (32, 32)))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and net.last_mem_idx is None
    with pytest.raises(TypeError, match="dequantisation table"):
        net.ips_image(torch.zeros((1, 1, 80, 112), dtype=torch.uint8), (32, 32), (16, 16))
    with pytest.raises(TypeError):
        net.ips_image(torch.zeros((2, 24, 1, 32, 32)), (32, 32), (16, 16))


def test_sparse_images_image_is_the_dense_canvas():
    from ips_amd.data.megapixel_mnist import SparseImages
    H, W = 37, 53
    g = np.random.default_rng(2)
    dense = np.zeros((3, H, W, 1), dtype=np.float32)
    index, value, offsets = [], [], [0]
    for i in range(3):
        flat = np.sort(g.choice(H * W, 40, replace=False))
        vals = g.random(40).astype(np.float32) + 0.1
        dense[i].reshape(-1)[flat] = vals
        index.append(flat)
        value.append(vals)
        offsets.append(offsets[-1] + 40)
    batch = SparseImages(torch.from_numpy(np.concatenate(index)), torch.from_numpy(np.concatenate(value)),
                         torch.tensor(offsets, dtype=torch.int64), (H, W, 1))
    img = batch.image()
    assert img.shape == (3, 1, H, W)
    assert torch.equal(img, torch.from_numpy(dense).permute(0, 3, 1, 2))
    # and its patches are the patches of the sparse form
    assert torch.equal(unfold(img, (16, 16), (7, 9)), batch.patches((16, 16), (7, 9)))
