"""The patch-grid view over uint8 images on the GPU: the stems stage ``table[c][byte]`` straight off the image grid
("uint8 images").

Two yardsticks everywhere, both compared with ``torch.equal`` - behind the staged image the ``_view_u8`` kernels run the code
of their twins, so there is no tolerance: the float32 view on ``table[c][images]``, and the uint8 patch path on the unfolded
bytes.  Inputs are guarded: every pixel no patch covers and a margin around the images is byte 255, ``table[c][255]`` is 1e30
and ``table[c][0] != 0`` - a read outside a patch row, a dequantised pad or a wrong channel row changes bits.  The images lie
k bytes past a 16-byte boundary, k in {0, 1, 2, 4}: every load width of every kernel is taken, and asserted."""

import pytest
import torch

from ips_amd import hip, quant, synth
from ips_amd.architecture import IPSNet
from view_cases import FUSED, FUSED_ROUND, GENERIC, POOL50, POOL50_CUT, POOL100, geom_id, grid, unfold
from view_u8_cases import (FUSED_AT_0, POOL50_AT_0, POOL100_AT_0, TIERS, expected_tier, guard_table, guarded_images_u8,
                           plain_table)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
_NETS = {}
# 2,116 patches at a row pitch and a stride of whole 16-byte units: the eight-patch kernel's 16-byte tier on a whole round
# (view_cases.FUSED_ROUND has w = 392 = 24.5 x 16: dwords there, 8-byte loads in the pair kernel)
FUSED_ROUND16 = (1, 1, 752, 752, (32, 32), (16, 16))


def net_for(kind, **over):
    """One net per configuration for the whole module (weights packed once)."""
    key = (kind, tuple(sorted(over.items())))
    if key not in _NETS:
        conf = {"mnist": lambda: synth.mnist_conf(**over),
                "mnist50": lambda: synth.mnist_conf(patch=50, **over),
                "traffic": lambda: synth.traffic_conf(**over),
                "generic": lambda: synth.traffic_conf(patch=37, **over)}[kind]()
        if kind == "generic":
            conf = conf.clone(patch_size=[37, 45], patch_stride=[37, 45])
        _NETS[key] = synth.fill_weights(IPSNet(DEV, conf), 5).to(DEV).eval()
    return _NETS[key]


def plan_of(net):
    return net.selection.plan()


def check_tiers(kinds, view, images, g, k, at_0=None):
    """The launcher's choice (``PatchView.load_bytes``: view_args' rule on the very pointer) against the width worked out
    from the numbers - and, at k = 0, against the table written out by hand."""
    for kind in kinds:
        got = view.load_bytes(images, TIERS[kind])
        assert got == expected_tier(kind, g, k), (kind, geom_id(g), k, got)
        if k == 0 and at_0 is not None and kind != "pair":
            assert got == at_0[(g[3], g[5][1])], (kind, geom_id(g), got)


def check_geometry(net, g, name, kinds, ks, firsts=(), at_0=None):
    b, c, h, w, patch, stride = g
    plan = plan_of(net)
    ny, nx = grid(g)
    table = guard_table(c).to(DEV)
    for k in ks:
        images = guarded_images_u8(g, k, device=DEV)
        assert images.data_ptr() % 16 == k and images.dtype == torch.uint8
        view = hip.PatchView(images.shape, patch, stride)
        assert plan.view_supported(view) and plan.view_kernel_name(view, u8=True) == name
        check_tiers(kinds, view, images, g, k, at_0)
        src = hip.PatchSource(images=images, view=view, table=table)
        patches = unfold(images, patch, stride)
        assert src.dtype == torch.uint8 and src.shape == patches.shape and int(patches.max()) < 255
        flat = patches.reshape(-1, *patches.shape[2:])
        floats = quant.dequant(images, table)
        want = plan.encode_view(floats, view)                          # the float32 view
        assert bool(torch.isfinite(want).all()) and float(want.abs().max()) < 1e20
        assert torch.equal(plan.encode(flat, table=table), want)       # the uint8 patches
        got = plan.encode_view(images, view, table=table)
        assert torch.equal(got, want)
        perm = torch.randperm(view.count, generator=torch.Generator().manual_seed(3 + k)).to(DEV)
        assert torch.equal(plan.encode_view(images, view, index=perm.to(torch.int32), table=table), want[perm])
        for first, n in firsts:
            assert torch.equal(plan.encode_view(images, view, first=first, n=n, table=table), want[first:first + n])
        # the M winners, written as float32 through the table
        m = min(7, view.per_image)
        idx = torch.stack([torch.randperm(view.per_image, generator=torch.Generator().manual_seed(9 + i))[:m] for i in range(b)]).to(DEV)
        rows = hip.gather_patches_view(images, view, idx, table)
        assert rows.dtype == torch.float32
        assert torch.equal(rows, hip.dequant_patches(hip.gather_rows(patches, idx), table))
        for bi in range(b):
            for j in range(m):
                py, px = divmod(int(idx[bi, j]), nx)
                y0, x0 = py * stride[0], px * stride[1]
                assert torch.equal(rows[bi, j], quant.dequant(images[bi, :, y0:y0 + patch[0], x0:x0 + patch[1]], table))
    torch.cuda.synchronize()


KS = (0, 1, 2, 4)


@pytest.mark.parametrize("g", FUSED, ids=geom_id)
def test_fused_trunk_reads_bytes_off_the_grid(g):
    check_geometry(net_for("mnist", N=64, M=8, I=8), g, "fused_trunk_view_u8_kernel", ("fused", "pair"), KS, at_0=FUSED_AT_0)


@pytest.mark.parametrize("g", [FUSED_ROUND, FUSED_ROUND16], ids=geom_id)
def test_fused_trunk_a_whole_round_and_the_pair_remainder(g):
    """A whole round of the eight-patch ``_view_u8`` kernel plus the remainder, which is the pair ``_view_u8`` kernel."""
    cus = hip.device_geometry(DEV).cus
    ny, nx = grid(g)
    assert ny * nx >= 8 * cus + 5, "the shape is meant to fill one whole round of the eight-patch kernel and leave a remainder"
    ks = (0, 1) if g is FUSED_ROUND else (0, 4)                 # 4 / bytes (pair: 8 / bytes), and 16 / 4 (pair: 8 / 4)
    check_geometry(net_for("mnist", N=64, M=8, I=8), g, "fused_trunk_view_u8_kernel", ("fused", "pair"), ks,
                   firsts=[(3, 1), (8 * cus - 3, 11)])


@pytest.mark.parametrize("g", POOL50, ids=geom_id)
def test_stem_pool50_reads_bytes_off_the_grid(g):
    check_geometry(net_for("mnist50", N=64, M=8, I=8), g, "stem_pool50_view_u8_kernel", ("pool50",), KS,
                   firsts=[(0, 1), (1, 4), (2, 5), (3, 9)], at_0=POOL50_AT_0)


def test_stem_pool50_across_the_two_stream_cut():
    check_geometry(net_for("mnist50", N=64, M=8, I=8), POOL50_CUT, "stem_pool50_view_u8_kernel", ("pool50",), (0, 1),
                   firsts=[(1023, 9)])


@pytest.mark.parametrize("g", POOL100, ids=geom_id)
def test_stem_pool100x3_reads_bytes_off_the_grid(g):
    check_geometry(net_for("traffic", N=48, M=16, I=32), g, "stem_pool100x3_view_u8_kernel", ("pool100",), KS, firsts=[(1, 3)],
                   at_0=POOL100_AT_0)


def test_the_lattice_takes_every_load_width():
    """No tier of any kernel's list goes untested: the widths expected over the cases above (each asserted against the
    launcher's choice where the case runs) are all of the list - the eight-patch kernel's on the whole rounds, which alone
    reach it (a remainder of up to a quarter round is the pair kernel's)."""
    lattice = {"fused": [(FUSED_ROUND, (0, 1)), (FUSED_ROUND16, (0, 4))],
               "pair": [(g, KS) for g in FUSED],
               "pool50": [(g, KS) for g in POOL50],
               "pool100": [(g, KS) for g in POOL100]}
    for kind, cases in lattice.items():
        assert {expected_tier(kind, g, k) for g, ks in cases for k in ks} == set(TIERS[kind]), kind


# ---------------------------------------------------------------- ips_image(uint8) against ips_image(float32) and ips(uint8 patches)
NAMES = ("mem_patch", "mem_pos", "last_mem_idx", "last_mem_emb", "last_shuffle")


def left_behind(net, out):
    return [None if t is None else t.clone() for t in tuple(out) + (net.last_mem_idx, net.last_mem_emb, net.last_shuffle)]


def same(got, want, what):
    for name, a, b in zip(NAMES, got, want):
        assert (a is None) == (b is None), (what, name)
        if a is not None:
            assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.cpu(), b.cpu()), (what, name)


def run_all(net, images, table, patch, stride, seed=None, view_expected=True, host=False):
    """-> by how much ``index_calls`` went up in the ``ips_image(uint8)`` call."""
    sel = net.selection
    net.set_patch_table(table)
    table = net.patch_table

    def seeded():
        if seed is not None:
            torch.manual_seed(seed)

    seeded()
    want_float = left_behind(net, net.ips_image(quant.dequant(images, table), patch, stride))
    seeded()
    want_patch = left_behind(net, net.ips(unfold(images, patch, stride)))
    before = (sel.view_calls, sel.index_calls)
    seeded()
    got = left_behind(net, net.ips_image(images.cpu() if host else images, patch, stride))
    torch.cuda.synchronize()
    assert sel.view_calls - before[0] == (1 if view_expected else 0)
    assert got[0].dtype == torch.float32 and got[0].device.type == "cuda"
    same(got, want_float, "ips_image(float32 images)")
    same(got, want_patch, "ips(uint8 patches)")
    return sel.index_calls - before[1]


def byte_images(shape, seed):
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed)).to(DEV)


def test_ips_image_mnist_small_batch():
    run_all(net_for("mnist", N=300, M=16, I=16), byte_images((2, 1, 480, 640), 3), plain_table(1), (32, 32), (32, 32))


@pytest.mark.parametrize("style", ["batch", "instance"])
def test_ips_image_shuffled_through_the_index(style):
    net = net_for("mnist", N=2500, shuffle=True, shuffle_style=style)
    assert run_all(net, byte_images((16, 1, 1600, 1600), 2), plain_table(1), (32, 32), (32, 32), seed=21) == 1
    assert net.last_shuffle is not None


def test_ips_image_one_image_at_stride_8():
    run_all(net_for("mnist", N=2116), byte_images((1, 1, 392, 392), 5), plain_table(1), (32, 32), (8, 8))


def test_ips_image_mnist50_long_loop_parts_through_index_lists():
    """961 overlapping 50-px patches, M = I = 8: 120 iterations - a layer-by-layer trunk whose parts are index lists."""
    images = byte_images((1, 1, 800, 800), 7)
    run_all(net_for("mnist50", N=961, M=8, I=8), images, plain_table(1), (50, 50), (25, 25))
    run_all(net_for("mnist50", N=961, M=8, I=8, shuffle=True, shuffle_style="instance"), images, plain_table(1), (50, 50), (25, 25),
            seed=5)


def test_ips_image_traffic_padding_does_not_go_through_the_table():
    """``patch_table(3, mean, std)``: table[c][0] = -mean / std != 0, so a padded pixel looked up would change bits."""
    table = quant.patch_table(3, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    assert bool((table[:, 0] != 0).all())
    run_all(net_for("traffic", N=48, M=16, I=32), byte_images((2, 3, 600, 800), 8), table, (100, 100), (100, 100))


def test_ips_image_host_images_give_the_device_result():
    run_all(net_for("mnist", N=300, M=16, I=16), byte_images((2, 1, 480, 640), 9), plain_table(1), (32, 32), (32, 32), host=True)


# ---------------------------------------------------------------- fallbacks and refusals
def test_generic_stem_materialises_uint8_patches():
    net = net_for("generic", N=9, M=4, I=2)
    b, c, h, w, patch, stride = GENERIC
    images = guarded_images_u8(GENERIC, 0, device=DEV)
    assert not plan_of(net).view_supported(hip.PatchView(images.shape, patch, stride))
    assert plan_of(net).view_kernel_name(hip.PatchView(images.shape, patch, stride), u8=True) is None
    run_all(net, images, guard_table(3), patch, stride, view_expected=False)


def test_bf16_precision_raises(monkeypatch):
    monkeypatch.setenv("IPSX_PRECISION", "bf16")
    net = synth.fill_weights(IPSNet(DEV, synth.mnist_conf(N=300, M=16, I=16)), 5).to(DEV).eval()
    net.set_patch_table(plain_table(1))
    with pytest.raises(TypeError, match="IPSX_PRECISION"):
        net.ips_image(byte_images((2, 1, 480, 640), 11), (32, 32), (32, 32))


def test_blank_patch_dedup_raises(monkeypatch):
    monkeypatch.setenv("IPSX_DEDUP_BLANK", "1")
    net = synth.fill_weights(IPSNet(DEV, synth.mnist_conf(N=300, M=16, I=16)), 5).to(DEV).eval()
    net.set_patch_table(plain_table(1))
    images = byte_images((2, 1, 480, 640), 12)
    with pytest.raises(TypeError, match="dedup"):
        net.ips_image(images, (32, 32), (32, 32))
    with pytest.raises(TypeError, match="dedup"):
        hip.PatchSource(images=images, view=hip.PatchView(images.shape, (32, 32), (32, 32)), table=net.patch_table)


def test_no_table_raises():
    net = synth.fill_weights(IPSNet(DEV, synth.mnist_conf(N=300, M=16, I=16)), 5).to(DEV).eval()
    images = byte_images((2, 1, 480, 640), 13)
    with pytest.raises(TypeError, match="dequantisation table"):
        net.ips_image(images, (32, 32), (32, 32))
    with pytest.raises(TypeError, match="dequantisation table"):
        hip.PatchSource(images=images, view=hip.PatchView(images.shape, (32, 32), (32, 32)))


# ---------------------------------------------------------------- memory
def test_neither_float_images_nor_patches_are_allocated():
    """B = 4 images of 392x392 at stride 8, warm net: the uint8 call's peak above its input is at most the float32 call's
    peak above ITS input plus 64 KiB (the only extra allocation is the table's use, at most 3 KB, plus allocator rounding) -
    float32 images would be 2.46 MB on top, the patch tensor 34.7 MB."""
    net = net_for("mnist", N=2116)
    net.set_patch_table(plain_table(1))
    bytes_ = byte_images((4, 1, 392, 392), 10)
    floats = quant.dequant(bytes_, net.patch_table)
    peaks = {}
    for name, images in (("uint8", bytes_), ("float32", floats)):
        net.ips_image(images, (32, 32), (8, 8))                # warmed: weights packed, the pipelines' buffers exist
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(DEV)
        base = torch.cuda.max_memory_allocated(DEV)
        out = net.ips_image(images, (32, 32), (8, 8))
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated(DEV) - base
        assert out[0].shape == (4, 64, 1, 32, 32) and out[0].dtype == torch.float32
        del out
    print("peak above the input: uint8 %d B, float32 %d B (input %d / %d B)" % (peaks["uint8"], peaks["float32"], bytes_.numel(),
                                                                               4 * floats.numel()))
    assert peaks["uint8"] <= peaks["float32"] + 64 * 1024
