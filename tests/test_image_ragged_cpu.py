"""ips_image_ragged() without a GPU: the ragged view's host table and address arithmetic - ONE function shared
with the kernels -, the RaggedImages container, the call on a CPU device against the loop of solo ips_image() calls, every
refusal before the RNG moves, and the new exports."""

import ctypes as C
import os
import re

import pytest
import torch
from torch.utils.data import DataLoader

import image_ragged_cases as ic
import ragged_cases as rc
from ips_amd import hip
from ips_amd.ragged_image import RaggedImages, collate_ragged_images
from view_cases import unfold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ipsx.h")
NEW = ("ipsx_ragged_view_fill", "ipsx_ragged_view_offset", "ipsx_trunk_ragged_view_supported", "ipsx_trunk_encode_ragged_view",
       "ipsx_ragged_finish_view")


# ---------------------------------------------------------------- the table and the address arithmetic
@pytest.mark.parametrize("name", sorted(ic.HOST_LISTS))
def test_every_packed_patch_lies_where_its_own_one_image_view_puts_it(name):
    """Every packed patch p of every list (the first and the last patch of every image among them): offset, pitch and channel
    pitch are elem_off_b + ipsx_patch_view_offset of image b's own one-image view, w_b and h_b * w_b; p = -1 and p = total
    give -1."""
    case = ic.HOST_LISTS[name]
    c, sizes, (ph, pw), (sh, sw) = case
    offs, _ = ic.offsets16(case, shift=3)                      # (any increasing offsets: the arithmetic does not ask for alignment)
    rv = hip.RaggedView(c, sizes, offs, (ph, pw), (sh, sw))
    grids = ic.grids(case)
    assert rv.grids == tuple(grids) and rv.count == sum(ny * nx for ny, nx in grids) and len(rv.sizes) == len(sizes)
    one = hip.lib().ipsx_patch_view_offset
    p = 0
    for b, ((h, w), (ny, nx)) in enumerate(zip(sizes, grids)):
        assert rv.firsts[b] == p
        own = hip.PatchViewStruct(1, c, h, w, ph, pw, sh, sw)
        for q in range(ny * nx):
            assert rv.origin(p) == (offs[b] + one(C.byref(own), q), w, h * w), (b, q)
            p += 1
    assert p == rv.count
    for bad in (-1, rv.count, rv.count + 7, 1 << 40):
        assert rv.origin(bad) == (-1, 0, 0)


def test_the_offsets_name_the_pixels_unfold_copies():
    """An image list whose every element holds its own offset inside the packed buffer: unfold SHOWS where each patch element
    comes from, and offset + (ch * h + y) * w + x names it."""
    case = ic.TWO
    c, sizes, (ph, pw), (sh, sw) = case
    offs, end = ic.offsets16(case)
    rv = hip.RaggedView(c, sizes, offs, (ph, pw), (sh, sw))
    where = torch.arange(end, dtype=torch.float64)
    p = 0
    for (h, w), o in zip(sizes, offs):
        patches = unfold(where[o:o + c * h * w].view(1, c, h, w), (ph, pw), (sh, sw))[0]
        ch, yy, xx = torch.meshgrid(torch.arange(c), torch.arange(ph), torch.arange(pw), indexing="ij")
        for q in range(patches.shape[0]):
            off, pitch, chan = rv.origin(p)
            assert torch.equal(patches[q], (off + ch * chan + yy * pitch + xx).to(torch.float64))
            p += 1


def test_fill_refuses_what_no_kernel_may_read():
    L = hip.lib()
    table = (hip.ImageEntry * 2)()

    def fill(h, w, off, c=1, ph=32, pw=32, sh=32, sw=32, b=2):
        return L.ipsx_ragged_view_fill(table, b, c, ph, pw, sh, sw, (C.c_int32 * 2)(*h), (C.c_int32 * 2)(*w), (C.c_int64 * 2)(*off))

    assert fill((64, 96), (64, 32), (0, 4096)) == 4 + 3
    assert fill((64, 31), (64, 32), (0, 4096)) == -1                       # a patch larger than an image
    assert fill((64, 96), (64, 31), (0, 4096)) == -1
    for bad in (dict(c=0), dict(ph=0), dict(pw=-1), dict(sh=0), dict(sw=0), dict(b=0)):
        assert fill((64, 96), (64, 32), (0, 4096), **bad) == -1, bad       # a non-positive field
    assert fill((0, 96), (64, 32), (0, 4096)) == -1
    assert fill((64, 96), (64, 32), (-4, 4096)) == -1
    assert fill((64, 96), (64, 32), (0, 4095)) == -1                       # overlapping images
    assert fill((64, 96), (64, 32), (4096, 0)) == -1                       # decreasing offsets
    assert fill((64, 96), (64, 32), (0, 2 * 4096), c=2) == 7 and fill((64, 96), (64, 32), (0, 2 * 4096 - 1), c=2) == -1
    assert L.ipsx_ragged_view_fill(None, 2, 1, 32, 32, 32, 32, None, None, None) == -1
    with pytest.raises(ValueError):
        hip.RaggedView(1, [(64, 64), (20, 64)], [0, 4096], (32, 32), (32, 32))
    # an entry that is not the geometry's own is no table: offset and supported say so
    assert fill((64, 96), (64, 32), (0, 4096)) == 7
    geo = hip.RaggedViewStruct(2, 1, 32, 32, 32, 32, None, table)
    assert L.ipsx_ragged_view_offset(table, 2, C.byref(geo), 4, None, None) == 4096
    table[1].first = 3
    assert L.ipsx_ragged_view_offset(table, 2, C.byref(geo), 4, None, None) == -1
    assert L.ipsx_trunk_ragged_view_supported(None, None) == 0
    t = hip.Trunk()
    t.c_in, t.h, t.w = 1, 32, 32
    assert L.ipsx_trunk_ragged_view_supported(C.byref(t), C.byref(geo)) == 0


# ---------------------------------------------------------------- the container
def test_ragged_images_round_trip_and_move():
    imgs = ic.make_images([(40, 51), (33, 37), (64, 32)], c=3)
    r = RaggedImages.from_list(imgs)
    assert len(r) == 3 and r.device == imgs[0].device and r.dtype == torch.float32 and r.pixels.dim() == 1
    assert r.sizes == ((40, 51), (33, 37), (64, 32)) and r.channels == 3
    for b, im in enumerate(imgs):
        assert r[b].shape == im.shape and ic.same_bits(r[b], im)
        assert (r.elem_offsets[b] * r.pixels.element_size()) % 16 == 0
    assert ic.same_bits(r[-1], imgs[-1]) and [tuple(v.shape) for v in r] == [tuple(im.shape) for im in imgs]
    half = r.to(torch.float64)
    assert half.sizes == r.sizes and half.elem_offsets == r.elem_offsets and half.dtype == torch.float64
    assert torch.equal(half[1], imgs[1].double()) and r.to(torch.float32) is r
    u8 = RaggedImages.from_list([torch.zeros((1, 5, 7), dtype=torch.uint8), torch.ones((1, 3, 3), dtype=torch.uint8)])
    assert u8.elem_offsets == (0, 48) and int(u8[1].sum()) == 9
    with pytest.raises(TypeError):
        RaggedImages.from_list([imgs[0], imgs[1][0]])
    with pytest.raises(ValueError):
        RaggedImages.from_list([imgs[0], imgs[1][:2]])
    with pytest.raises(ValueError):
        RaggedImages(torch.zeros(100), 1, [(5, 5), (5, 5)], [0, 24])


def test_pin_memory_keeps_shapes_and_offsets():
    r = RaggedImages.from_list(ic.make_images([(40, 51), (33, 37)]), pad=True)
    if torch.cuda.is_available():
        p = r.pin_memory()
        assert p.pixels.is_pinned()
    else:
        p = r._like(r.pixels.clone())              # (what to() and pin_memory() build their result with; pinning needs a GPU runtime)
    assert p is not r and p.sizes == r.sizes and p.elem_offsets == r.elem_offsets and p.channels == r.channels and p.pad
    assert ic.same_bits(p[1], r[1]) and p.view((32, 32), (32, 32)) is r.view((32, 32), (32, 32))


def test_collate_ragged_images_on_dataset_samples():
    imgs = ic.make_images([(40, 51), (33, 37), (64, 32), (50, 50)])
    data = [{"input": im, "majority": k % 3, "max": float(k)} for k, im in enumerate(imgs)]
    batches = list(DataLoader(data, batch_size=2, collate_fn=collate_ragged_images))
    assert len(batches) == 2
    for k, batch in enumerate(batches):
        r = batch["input"]
        assert isinstance(r, RaggedImages) and len(r) == 2 and not r.pad
        assert ic.same_bits(r[0], imgs[2 * k]) and ic.same_bits(r[1], imgs[2 * k + 1])
        assert batch["majority"].tolist() == [(2 * k) % 3, (2 * k + 1) % 3]


# ---------------------------------------------------------------- the call on a CPU device
SIZES = [(160, 192), (192, 224), (128, 416)]                   # 30, 42, 52 patches at stride 32: all longer than M = 16
PATCH, STRIDE = (32, 32), (32, 32)


@pytest.mark.parametrize("shuffle,style,use_pos", [(False, "batch", True), (True, "batch", True), (True, "instance", False)])
def test_cpu_call_equals_the_solo_ips_image_loop(shuffle, style, use_pos):
    net = rc.make_net(rc.image_conf(M=16, shuffle=shuffle, shuffle_style=style, use_pos=use_pos), "cpu")
    imgs = ic.make_images(SIZES)
    want = ic.solo_loop(net, imgs, PATCH, STRIDE)
    got = ic.image_call(net, imgs, PATCH, STRIDE)
    rc.assert_same_record(got, want)
    assert got["count"] is None
    if shuffle:
        assert [tuple(s.shape) for s in got["shuffle"]] == [(1, 30), (1, 42), (1, 52)]
    # ... and the ragged call on the materialised patch tensors
    slides = [unfold(im[None], PATCH, STRIDE)[0] for im in imgs]
    rc.assert_same_record(ic.patch_call(net, slides), want)
    # net.ips_image(RaggedImages) hands over
    rc.assert_same_record(ic.image_call(net, imgs, PATCH, STRIDE, through_ips_image=True), want)


@pytest.mark.parametrize("shuffle", [False, True])
def test_cpu_padded_call_with_a_short_image_and_one_of_exactly_m(shuffle):
    net = rc.make_net(rc.image_conf(M=16, shuffle=shuffle, shuffle_style="batch"), "cpu")
    sizes = SIZES + [(128, 128), (64, 96)]                     # 16 = M and 6 patches
    imgs = ic.make_images(sizes)
    slides = [unfold(im[None], PATCH, STRIDE)[0] for im in imgs]
    want = ic.patch_call(net, slides, pad=True)
    got = ic.image_call(net, imgs, PATCH, STRIDE, pad=True)
    ic.assert_same_padded(got, want)
    assert got["count"] == (16, 16, 16, 16, 6) == net.last_mem_count
    # the long images are the solo loop's, the short ones DESIGN 2.6's table
    solo = ic.solo_loop(net, imgs[:3], PATCH, STRIDE)
    for key in ("mem_patch", "mem_pos", "mem_idx", "mem_emb"):
        assert ic.same_bits(got[key][:3], solo[key]), key
    assert ic.same_bits(got["mem_patch"][3], slides[3]) and ic.same_bits(got["mem_patch"][4, :6], slides[4])
    assert not got["mem_patch"][4, 6:].any() and not got["mem_pos"][4, 6:].any()
    assert got["mem_idx"][4].tolist() == list(range(6)) + [-1] * 10 and got["mem_idx"][3].tolist() == list(range(16))
    assert ic.same_bits(got["mem_pos"][4, :6], net.pos_enc[0, :6])
    through = ic.image_call(net, imgs, PATCH, STRIDE, pad=True, through_ips_image=True)
    ic.assert_same_padded(through, want)


def test_every_refusal_comes_before_the_rng_moves(monkeypatch):
    net = rc.make_net(rc.image_conf(M=16, shuffle=True, shuffle_style="batch"), "cpu")
    imgs = ic.make_images(SIZES)
    short = ic.make_images([(64, 96)])[0]

    def refused(exc, images, patch=PATCH, stride=STRIDE, who=net, **kw):
        torch.manual_seed(5)
        before = torch.get_rng_state()
        who.last_mem_idx = "untouched"
        with pytest.raises(exc):
            who.ips_image_ragged(images, patch, stride, **kw)
        assert torch.equal(torch.get_rng_state(), before) and who.last_mem_idx == "untouched"

    refused(ValueError, [])                                                       # an empty batch
    refused(ValueError, imgs + [short])                                           # an image with no more than M patches, no pad
    refused(ValueError, imgs + [torch.zeros((1, 31, 40))], pad=True)              # the patch does not fit an image
    refused(ValueError, imgs, stride=(0, 32))
    refused(ValueError, imgs + [torch.zeros((2, 160, 192))])                      # channel counts differ from each other
    refused(ValueError, [torch.zeros((3, 160, 192)), torch.zeros((3, 192, 192))])  # ... and from the encoder's
    refused(TypeError, [im.mul(255).to(torch.uint8) for im in imgs])             # uint8 images
    refused(TypeError, [imgs[0], imgs[1][0]])                                     # no (C, H, W) tensor
    refused(ValueError, imgs + [torch.zeros((1, 32 * 12, 32 * 11))])              # 132 patches, the positional table conf.N = 128
    monkeypatch.setenv("IPSX_DEDUP_BLANK", "1")
    refused(TypeError, imgs)
    monkeypatch.delenv("IPSX_DEDUP_BLANK")
    inst = rc.make_net(rc.image_conf(M=16, shuffle=True, shuffle_style="instance"), "cpu")
    refused(ValueError, imgs, who=inst)                                           # 'instance' with positions needs conf.N patches
    feat = rc.make_net(rc.feature_conf(M=16), "cpu")
    refused(TypeError, imgs, who=feat)                                            # a feature net


# ---------------------------------------------------------------- ABI
def test_new_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(ipsx_[a-z0-9_]+)\s*\(", text))
    lib = C.CDLL(hip.library_path())
    for s in NEW:
        assert s in declared and hasattr(lib, s) and s in hip._EXPORTS, s
    assert "typedef struct ipsx_image_entry" in text and "typedef struct ipsx_ragged_view" in text
    assert C.sizeof(hip.ImageEntry) == 32
    assert [f[0] for f in hip.ImageEntry._fields_] == ["elem_off", "first", "h", "w", "ny", "nx"]
    assert [f[0] for f in hip.RaggedViewStruct._fields_][:7] == ["b", "c", "ph", "pw", "sh", "sw", "images"]
    assert hip.lib().ipsx_version() == 306
