"""Row streams (``IPSNet.ips_stream(patch_size, patch_stride)``) without a GPU: the integer bookkeeping of the
bands swept against ``unfold``'s patch rows, ``feed_rows`` on the CPU device against ``ips_image`` on the concatenation,
the caller's buffer, the refusals, and the header / export surface of ``ipsx_stream_commit_view`` with the argument checks
that need no device."""

import ctypes as C
import os
import re

import pytest
import torch

from ips_amd import hip, synth
from ips_amd.architecture import IPSNet
from ips_amd.stream import BandGeometry, IPSStream
from tests.stream_rows_cases import band_patterns, bands_of

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ipsx.h")
PATCH, STRIDE = (32, 32), (16, 16)
H, W = 149, 80                      # 8 x 4 = 32 patches, 5 trailing rows that complete nothing
PATTERNS = ["ones", "stride", "straddle", "irregular", "whole"]


# ------------------------------------------------------------------ 1. the geometry alone
@pytest.mark.parametrize("sh", [1, 2, 5, 7])
@pytest.mark.parametrize("ph", [3, 5])
def test_geometry_completes_unfolds_patch_rows(ph, sh):
    for total in range(1, 41):
        ny = (total - ph) // sh + 1 if total >= ph else 0
        for name, heights in band_patterns(total, ph, sh, irregular=[1, 2 * ph + 3, 3, ph, 1, 1, sh + 1, 2]).items():
            g = BandGeometry(ph, sh)
            starts, taken = [], 0
            for h in heights:
                first, carry_before, skip_before = g.first_row, g.carry, g.skip
                assert carry_before < ph and (skip_before == 0 or carry_before == 0)
                plan = g.plan(h)
                assert g.rows == taken and plan == g.take(h)              # plan() takes nothing
                drop, rows, ny_w, carry, skip = plan
                taken += h
                assert g.rows == taken and drop == min(skip_before, h) and rows == carry_before + h - drop
                assert g.carry == carry and g.skip == skip and carry < ph
                if ny_w:
                    assert (ny_w - 1) * sh + ph <= rows                  # every completed patch row lies inside the window
                    assert first == len(starts) * sh
                starts += [first + i * sh for i in range(ny_w)]
                # the rows kept are those from the next patch row's first row on, and only rows that exist
                assert g.first_row == len(starts) * sh
            assert starts == [py * sh for py in range(ny)], (total, name)
            assert g.patch_rows == ny


def test_geometry_refuses_nonsense():
    with pytest.raises(ValueError):
        BandGeometry(0, 1)
    with pytest.raises(ValueError):
        BandGeometry(3, 1).plan(0)


# ------------------------------------------------------------------ 2. the CPU device
def small_net(**kw):
    conf = synth.mnist_conf(N=40, M=8, I=8, **kw)
    net = synth.fill_weights(IPSNet(torch.device("cpu"), conf), 5).eval()
    net.shuffle = False
    return net


def results(net, out):
    return out[0], out[1], net.last_mem_idx, net.last_mem_emb


def same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def f32():
    net = small_net(use_pos=True)
    images = torch.randn((2, 1, H, W), generator=torch.Generator().manual_seed(3))
    want = results(net, net.ips_image(images, PATCH, STRIDE))
    assert want[2] is not None and want[0].shape == (2, 8, 1, 32, 32)
    return net, images, want


@pytest.fixture(scope="module")
def u8():
    net = small_net()
    table = torch.randn((1, 256), generator=torch.Generator().manual_seed(4))
    table[0, 0] = 0.5
    net.set_patch_table(table)
    images = torch.randint(0, 256, (2, 1, H, W), dtype=torch.uint8, generator=torch.Generator().manual_seed(5))
    want = results(net, net.ips_image(images, PATCH, STRIDE))
    assert want[0].dtype == torch.float32
    return net, images, want


def run(net, bands, after=None):
    s = net.ips_stream(patch_size=PATCH, patch_stride=STRIDE)
    rows = 0
    for band in bands:
        assert s.feed_rows(band) is s
        rows += band.shape[2]
        assert s.rows == rows and s.fed == (max(0, rows - PATCH[0]) // STRIDE[0] + (rows >= PATCH[0])) * 4
        assert s.iterations == max(0, s.fed - net.M) // net.I
        assert (s.mem_idx is None) == (s.fed < net.M)
        if after is not None:
            after(band)
    return results(net, s.finish())


@pytest.mark.parametrize("pattern", PATTERNS)
def test_feed_rows_equals_ips_image_on_the_cpu_device(pattern, f32):
    net, images, want = f32
    assert same(run(net, bands_of(images, band_patterns(H, 32, 16)[pattern])), want)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_uint8_bands_on_the_cpu_device(pattern, u8):
    net, images, want = u8
    got = run(net, bands_of(images, band_patterns(H, 32, 16)[pattern]))
    assert got[0].dtype == torch.float32 and same(got, want)


def test_a_stride_above_the_patch_skips_rows():
    net = small_net()
    images = torch.randn((2, 1, 150, 80), generator=torch.Generator().manual_seed(6))
    want = results(net, net.ips_image(images, PATCH, (40, 16)))              # patch rows at 0, 40, 80: 8 rows between them unused
    for heights in ([7] * 21 + [3], [33, 1, 5, 40, 71], [150]):
        s = net.ips_stream(PATCH, (40, 16))
        for band in bands_of(images, heights):
            s.feed_rows(band)
        assert s.fed == 12 and same(results(net, s.finish()), want)


def test_a_total_of_at_most_m_returns_the_patches_in_arrival_order():
    net = small_net(use_pos=True)
    images = torch.randn((2, 1, 50, 80), generator=torch.Generator().manual_seed(7))        # 2 x 4 = 8 patches = M
    s = net.ips_stream(PATCH, STRIDE)
    for band in bands_of(images, [20, 20, 10]):
        s.feed_rows(band)
    mem_patch, mem_pos = s.finish()
    p = images.unfold(2, 32, 16).unfold(3, 32, 16).permute(0, 2, 3, 1, 4, 5).reshape(2, 8, 1, 32, 32)
    assert torch.equal(mem_patch, p) and net.last_mem_idx is None and tuple(mem_pos.shape) == (2, 8, net.D)
    s = net.ips_stream(PATCH, STRIDE)
    s.feed_rows(images[:, :, :20])
    with pytest.raises(RuntimeError, match="complete no patch row"):
        s.finish()


# ------------------------------------------------------------------ 3. the caller's buffer
@pytest.mark.parametrize("kind", ["f32", "u8"])
def test_the_caller_may_overwrite_the_band_after_every_feed(kind, f32, u8):
    net, images, want = f32 if kind == "f32" else u8
    buf = torch.empty((2, 1, 37, W), dtype=images.dtype)

    def bands():
        for lo in range(0, H, 37):
            n = min(37, H - lo)
            buf[:, :, :n] = images[:, :, lo:lo + n]
            yield buf[:, :, :n]

    assert same(run(net, bands(), after=lambda band: buf.fill_(float("nan") if kind == "f32" else 255)), want)


# ------------------------------------------------------------------ 4. refusals
def test_refusals(monkeypatch, f32):
    net, images, _ = f32
    assert type(net.ips_stream()) is IPSStream and net.ips_stream().rows is None            # still a patch stream
    with pytest.raises(TypeError, match="patch stream"):
        net.ips_stream().feed_rows(images[:, :, :40])
    with pytest.raises(ValueError, match="both"):
        net.ips_stream(patch_size=PATCH)
    s = net.ips_stream(patch_size=PATCH, patch_stride=STRIDE)
    with pytest.raises(TypeError, match="row stream"):
        s.feed(torch.zeros((2, 4, 1, 32, 32)))
    with pytest.raises(ValueError, match="do not fit"):
        s.feed_rows(images[:, :, :40, :31])                      # pw > W
    with pytest.raises(ValueError):
        s.feed_rows(images[0, :, :40])                           # not 4-D
    with pytest.raises(TypeError):
        s.feed_rows(images[:, :, :40].double())
    with pytest.raises(TypeError, match="dequantisation table"):
        s.feed_rows(torch.zeros((2, 1, 40, W), dtype=torch.uint8))          # uint8 without a table
    with pytest.raises(ValueError, match="channels"):
        s.feed_rows(images[:, :, :40].expand(2, 3, 40, W))
    assert s.rows == 0 and s.fed == 0
    s.feed_rows(images[:, :, :40])
    state = (s.rows, s.fed, s._carry.clone())
    with pytest.raises(ValueError):
        s.feed_rows(images[:1, :, 40:60])                        # another B
    with pytest.raises(ValueError):
        s.feed_rows(images[:, :, 40:60, :64])                    # another W
    with pytest.raises(ValueError):
        s.feed_rows(images[:, :, 40:60].expand(2, 2, 20, W))     # another C
    with pytest.raises(TypeError):
        s.feed_rows(images[:, :, 40:60].to(torch.uint8))         # another dtype
    with pytest.raises(ValueError):
        s.feed_rows(images[:, :, 40:40])                         # no rows
    with pytest.raises(ValueError, match="positional"):
        s.feed_rows(torch.zeros((2, 1, 16 * 10, W)))             # 11 patch rows: 44 patches, a table of 40 rows
    monkeypatch.setenv("IPSX_DEDUP_BLANK", "1")
    with pytest.raises(TypeError, match="dedup"):
        s.feed_rows(images[:, :, 40:60])
    monkeypatch.delenv("IPSX_DEDUP_BLANK")
    assert (s.rows, s.fed) == state[:2] and torch.equal(s._carry, state[2])          # a refused band leaves the stream as it was
    hip.weights_changed()
    with pytest.raises(RuntimeError, match="weights changed"):
        s.feed_rows(images[:, :, 40:60])
    s = net.ips_stream(PATCH, STRIDE)
    s.feed_rows(images)
    s.finish()
    with pytest.raises(RuntimeError, match="finished"):
        s.feed_rows(images[:, :, :8])
    with pytest.raises(TypeError):
        synth.fill_weights(IPSNet(torch.device("cpu"), synth.camelyon_conf(N=40, M=8, I=8, n_chan_in=64)), 5).ips_stream(PATCH, STRIDE)


def test_a_table_of_another_channel_count_is_refused():
    net = small_net()
    net.patch_table = torch.zeros((3, 256))                     # (set_patch_table itself refuses it: put there by hand)
    with pytest.raises(ValueError, match="channels"):
        net.ips_stream(PATCH, STRIDE).feed_rows(torch.zeros((2, 1, 40, W), dtype=torch.uint8))


def test_a_training_mode_net_is_restored_after_every_feed(f32):
    net, images, want = f32
    net.train()
    try:
        s = net.ips_stream(PATCH, STRIDE)
        for band in bands_of(images, band_patterns(H, 32, 16)["straddle"]):
            s.feed_rows(band)
            assert net.training and net.encoder.training and net.transf.training
        got = results(net, s.finish())
    finally:
        net.eval()
    assert same(got, want)


# ------------------------------------------------------------------ 5. header and export
def test_header_declares_the_export_inside_the_306_block():
    text = open(HEADER).read()
    assert re.search(r"#define\s+IPSX_VERSION\s+306\b", text)
    block = text[text.index("3.06  (additions only)"):text.index("#define IPSX_VERSION")]
    assert "ipsx_stream_commit_view" in block
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+ipsx_stream_commit_view\s*\(", plain)
    assert "ipsx_stream_commit_view" in hip._EXPORTS
    lib = hip.lib()
    assert lib.ipsx_version() == 306 and len(lib.ipsx_stream_commit_view.argtypes) == 12
    assert C.sizeof(hip.PatchViewStruct) == 32                  # the view keeps its layout


def test_stream_commit_view_refuses_bad_arguments_before_any_launch():
    lib = hip.lib()
    images = (C.c_char * (2 * 40 * 48 * 4))()
    state = (C.c_char * (2 * 8 * 4096))()
    other = (C.c_char * (2 * 8 * 4096))()
    view = hip.PatchViewStruct(2, 1, 40, 48, 32, 32, 8, 16)     # 2 x 2 patches per image
    one = hip.StreamTable()
    one.held, one.dst = C.addressof(state), C.addressof(other)
    one.held_rows, one.held_bstride_rows, one.dst_rows, one.dst_bstride_rows, one.row_bytes = 2, 8, 8, 8, 4096
    tabs = (hip.StreamTable * 1)(one)
    sel = (C.c_int64 * 8)(*range(4), *range(4))

    def call(tables=tabs, img=C.addressof(images), v=view, elem=4, s=C.addressof(sel), n_cand=6, tail=6):
        return lib.ipsx_stream_commit_view(tables, 1, img, C.byref(v) if v is not None else None, elem, s, 2, 4, n_cand, tail,
                                           None, None)

    def refused(rc, what):
        assert rc == -1 and what in lib.ipsx_last_error().decode(), lib.ipsx_last_error()      # IPSX_EINVAL

    refused(call(img=None), "null images")
    refused(call(v=None), "null images or view")
    refused(call(tables=None), "null tables")
    refused(call(elem=3), "element of 3 bytes")
    refused(call(elem=1), "rows of 4096 bytes")                 # the rows are not byte patches
    refused(call(v=hip.PatchViewStruct(2, 1, 31, 48, 32, 32, 8, 16)), "does not fit")       # ph > h
    refused(call(v=hip.PatchViewStruct(3, 1, 40, 48, 32, 32, 8, 16)), "a view of 3 images")
    refused(call(n_cand=7, tail=7), "4 patches per image")      # 5 candidates behind the held rows
    refused(call(tail=1), "do not fit")                         # 4 + 5 rows into room for 8
    small = hip.StreamTable.from_buffer_copy(one)
    small.dst_rows = small.dst_bstride_rows = 3
    refused(call(tables=(hip.StreamTable * 1)(small)), "do not fit")
    inplace = hip.StreamTable.from_buffer_copy(one)
    inplace.dst = C.addressof(state)
    refused(call(tables=(hip.StreamTable * 1)(inplace)), "in place")
    over = hip.StreamTable.from_buffer_copy(one)
    over.dst = C.addressof(images) + 64
    over.dst_rows = over.dst_bstride_rows = 1
    refused(lib.ipsx_stream_commit_view((hip.StreamTable * 1)(over), 1, C.addressof(images), C.byref(view), 4, None, 1, 4, 1, 0,
                                        None, None), "a view of 2 images")
    v1 = hip.PatchViewStruct(1, 1, 40, 48, 32, 32, 8, 16)
    over.held, over.held_rows = None, 0
    refused(lib.ipsx_stream_commit_view((hip.StreamTable * 1)(over), 1, C.addressof(images), C.byref(v1), 4, None, 1, 4, 1, 0,
                                        None, None), "overlaps the images")
    piece = hip.StreamTable.from_buffer_copy(one)
    piece.piece = C.addressof(other)
    refused(call(tables=(hip.StreamTable * 1)(piece)), "its piece is the patch view")
    with pytest.raises(RuntimeError, match="null tables"):
        hip.stream_commit_view(None, torch.zeros((2, 1, 40, 48)), hip.PatchView((2, 1, 40, 48), (32, 32), (8, 16)), None, 4, 4)
    t = torch.zeros((2, 8, 1, 32, 32))
    with pytest.raises(ValueError, match="piece is the view"):
        hip.stream_commit_view([(t, 2, t[:, :2], t)], torch.zeros((2, 1, 40, 48)), hip.PatchView((2, 1, 40, 48), (32, 32), (8, 16)),
                               None, 4, 4)
    with pytest.raises(ValueError, match="made for"):
        hip.stream_commit_view([(t, 2, None, t)], torch.zeros((2, 1, 41, 48)), hip.PatchView((2, 1, 40, 48), (32, 32), (8, 16)),
                               None, 4, 4)
