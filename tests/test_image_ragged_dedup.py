"""Exact blank-patch dedup on the ragged view ("Dedup"): the blank scan that reads grid patches where they lie in
images of different sizes, the encoder pass over the non-blank entries and ONE blank one, and ips_image_ragged() on top.

Every comparison is bit for bit: the same kernel encodes the same inputs with and without dedup.  Inputs carry NaN in every
pixel no patch covers, between the images and around the buffer, and are mostly zero: a read outside a patch window turns a
blank patch into a non-blank one, a stray read of the encoder breaks finiteness."""

import pytest
import torch

import image_ragged_cases as ic
import image_ragged_dedup_cases as dc
import ragged_cases as rc
from ips_amd import hip, synth
from ips_amd.architecture import IPSNet

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
_NETS = {}


def net_for(kind, **over):
    """One net per configuration for the whole module (weights packed once)."""
    key = (kind, tuple(sorted(over.items())))
    if key not in _NETS:
        conf = {"mnist": lambda: synth.mnist_conf(**over), "mnist50": lambda: synth.mnist_conf(patch=50, **over)}[kind]()
        _NETS[key] = synth.fill_weights(IPSNet(DEV, conf), 5).to(DEV).eval()
    return _NETS[key]


# ---------------------------------------------------------------- the flags
def planted(case):
    """All-zero images of ``case`` (every first image at least 96 x 128, every second at least 100 x 116) with, at window
    origins that are multiples of 32 - grid patches at stride 32 and at stride 16 alike:
      image 0: ONE non-zero pixel at each of the four corners of four windows, (0, 0) (0, 64) (64, 0) (64, 64); the window at
               (32, 32) stays zero, with a non-zero pixel one column to its right and one one row below it;
      image 1: the window at (0, 0) all -0.0 (blank), the window at (32, 32) zero but for one denormal in its row 20 (not
               blank: read behind the first KiB), the window at (64, 64) full of content.
    -> the host images"""
    imgs = dc.zero_images(case)
    a, b = imgs[0][0], imgs[1][0]
    a[0, 0] = 1.0                     # top left of the window at (0, 0)
    a[0, 64 + 31] = 2.0               # top right of the window at (0, 64)
    a[64 + 31, 0] = -3.0              # bottom left of the window at (64, 0)
    a[64 + 31, 64 + 31] = 4.0         # bottom right of the window at (64, 64)
    a[32 + 5, 64] = 5.0               # one column right of the window at (32, 32)
    a[64, 32 + 7] = 6.0               # one row below it
    b[0:32, 0:32] = -0.0
    b[32 + 20, 32 + 9] = 1e-45        # the smallest denormal
    b[64:96, 64:96] = torch.randn((32, 32), generator=torch.Generator().manual_seed(1)) + 3.0
    return imgs


def patch_at(case, b, y0, x0):
    """The packed number of image b's grid patch whose window starts at (y0, x0)."""
    grids = ic.grids(case)
    return sum(ny * nx for ny, nx in grids[:b]) + (y0 // case[3][0]) * grids[b][1] + x0 // case[3][1]


@pytest.mark.parametrize("case,k", [(ic.FUSED_MIXED, 0), (ic.FUSED_ALIGNED, 0), (ic.FUSED_ALIGNED, 1), (dc.STRIDE16, 0)],
                         ids=["dword", "wide", "wide_four_bytes_off", "stride16"])
def test_flags_equal_the_host_rule_on_planted_content(case, k):
    c, sizes, patch, stride = case
    images, imgs = dc.pack(case, planted(case), k, device=DEV)
    assert images.pixels.data_ptr() % 16 == 4 * k
    rview = images.view(patch, stride)
    want = dc.host_flags(dc.flat_patches([im.cpu() for im in imgs], patch, stride))
    assert want.numel() == rview.count and 0 < int(want.sum()) < rview.count // 2            # mostly blank
    # what the planted content means, whatever the stride: the patch at (32, 32) of image 0 sees neither neighbour pixel,
    # -0.0 is blank, a denormal is not
    assert want[patch_at(case, 0, 32, 32)] == 0 and want[patch_at(case, 1, 0, 0)] == 0 and want[patch_at(case, 1, 32, 32)] == 1
    for y0, x0 in ((0, 0), (0, 64), (64, 0), (64, 64)):
        assert want[patch_at(case, 0, y0, x0)] == 1
    got = hip.ragged_blank_flags(images.pixels, rview)
    assert got.dtype == torch.int32 and torch.equal(got.cpu(), want)
    # an index list with a repeated entry and one that is no packed patch: it is flagged as packed patch 0
    listed = torch.randperm(rview.count, generator=torch.Generator().manual_seed(3 + k))
    listed[-1] = listed[0]
    take = listed.clone()
    listed[1], take[1] = rview.count + 5, 0
    got = hip.ragged_blank_flags(images.pixels, rview, index=listed.to(torch.int32).to(DEV))
    assert torch.equal(got.cpu(), want[take])
    # first > 0 lands inside the second image
    first = rview.firsts[1] + 1
    assert torch.equal(hip.ragged_blank_flags(images.pixels, rview, first=first, n=6).cpu(), want[first:first + 6])
    assert torch.equal(hip.ragged_blank_flags(images.pixels, rview, first=first).cpu(), want[first:])
    assert hip.ragged_blank_flags(images.pixels, rview, first=3, n=0).numel() == 0


def test_flags_refuse_another_patch_shape_and_a_range_outside_the_view():
    images, _ = ic.guarded_ragged(ic.POOL50, 0, device=DEV)
    with pytest.raises(RuntimeError):
        hip.ragged_blank_flags(images.pixels, images.view((50, 50), (25, 25)))
    images, _ = ic.guarded_ragged(ic.FUSED_MIXED, 0, device=DEV)
    rview = images.view((32, 32), (32, 32))
    with pytest.raises(ValueError):
        hip.ragged_blank_flags(images.pixels, rview, first=rview.count - 2, n=3)


# ---------------------------------------------------------------- the encoder pass
def check_encoder(case, imgs, k=0, listed=None, ranges=()):
    """``encode_source(dedup=True)`` of the packed ``imgs`` against ``encode_plain`` of their patches, and ``n_encoded``
    against the host's count: the whole view, ``listed`` (packed patch numbers, every one a packed patch), ``ranges``."""
    c, sizes, patch, stride = case
    plan = net_for("mnist", N=64, M=8, I=8).selection.plan()
    images, imgs = dc.pack(case, imgs, k, device=DEV)
    rview = images.view(patch, stride)
    patches = dc.flat_patches(imgs, patch, stride)
    assert patches.shape[0] == rview.count and bool(torch.isfinite(patches).all())
    flags = dc.host_flags(patches.cpu())
    want = plan.encode_plain(patches)
    src = hip.PatchSource(images=images.pixels, ragged=rview)
    plan.n_encoded = None
    got = plan.encode_source(src, dedup=True)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)
    assert int(plan.n_encoded) == dc.host_count(flags)
    if listed is not None:
        got = plan.encode_source(src, index=listed.to(torch.int32).to(DEV), dedup=True)
        assert torch.equal(got, want[listed.to(DEV)]) and int(plan.n_encoded) == dc.host_count(flags[listed])
    for first, n in ranges:
        got = plan.encode_source(src, first=first, n=n, dedup=True)
        assert torch.equal(got, want[first:first + n]) and int(plan.n_encoded) == dc.host_count(flags[first:first + n])
    torch.cuda.synchronize()
    return flags


def total_of(case):
    return sum(ny * nx for ny, nx in ic.grids(case))


def test_no_blank_patch_encodes_every_entry():
    case = ic.FUSED_MIXED
    flags = check_encoder(case, dc.fill_windows(case, dc.zero_images(case), range(total_of(case))))
    assert int(flags.sum()) == total_of(case)                             # n_encoded == n


def test_all_blank_encodes_one_entry():
    flags = check_encoder(ic.FUSED_MIXED, dc.zero_images(ic.FUSED_MIXED))
    assert int(flags.sum()) == 0                                          # n_encoded == 1


def test_exactly_one_blank_patch():
    case = ic.FUSED_ALIGNED
    n = total_of(case)
    flags = check_encoder(case, dc.fill_windows(case, dc.zero_images(case), [p for p in range(n) if p != 17]), k=1)
    assert int(flags.sum()) == n - 1 and flags[17] == 0


@pytest.mark.parametrize("nonblank", [7, 8, 9])
def test_the_count_just_before_on_and_after_a_workgroups_edge(nonblank):
    """The trunk's list is the non-blank entries and one blank one: 8, 9 and 10 entries for eight-patch workgroups."""
    case = ic.FUSED_MIXED                                                 # 12 + 9 + 1 + 10 windows that do not overlap
    keep = [1, 4, 11, 12, 13, 20, 21, 22, 31][:nonblank]                  # (the lone patch of image 2 among them, and the last one)
    flags = check_encoder(case, dc.fill_windows(case, dc.zero_images(case), keep), ranges=[(13, 6), (2, 30)])
    assert int(flags.sum()) == nonblank and total_of(case) == 32


def half_blank_round():
    """FUSED_ROUND's images with content in their upper rows only: the patches that reach below are part blank, those that
    start below all blank - about half of every image."""
    case = ic.FUSED_ROUND
    imgs = dc.zero_images(case)
    for b, im in enumerate(imgs):
        gen = torch.Generator().manual_seed(40 + b)
        rows = im.shape[1] // 2
        im[:, :rows] = torch.where(torch.isnan(im[:, :rows]), im[:, :rows], torch.randn(im[:, :rows].shape, generator=gen) + 0.5)
    return case, imgs


def test_a_whole_round_about_half_blank():
    cus = hip.device_geometry(DEV).cus
    case, imgs = half_blank_round()
    total = total_of(case)
    assert total >= 8 * cus + 5, "the shape is meant to fill one whole round of the eight-patch kernel and leave a remainder"
    flags = check_encoder(case, imgs, ranges=[(2110, 100)])
    nb = int(flags.sum())
    assert total // 3 < nb < 2 * total // 3
    # an image's last non-blank patch and the next image's first share a workgroup of the compacted list
    firsts = [0, 2116, 2296]
    assert int(flags[:firsts[1]].sum()) % 8 != 0 and int(flags[:firsts[2]].sum()) % 8 != 0


def test_an_index_list_permuted_with_a_repeated_entry():
    case, imgs = half_blank_round()
    listed = torch.randperm(total_of(case), generator=torch.Generator().manual_seed(9))[:700]
    listed[-1] = listed[0]
    check_encoder(case, imgs, listed=listed)


def test_a_list_entry_that_is_no_packed_patch_reads_packed_patch_zero():
    case = ic.FUSED_MIXED
    plan = net_for("mnist", N=64, M=8, I=8).selection.plan()
    for keep, blank0 in (([0, 5], False), ([5, 9], True)):               # packed patch 0 non-blank (9 blank), and blank
        images, imgs = dc.pack(case, dc.fill_windows(case, dc.zero_images(case), keep), device=DEV)
        rview = images.view(case[2], case[3])
        want = plan.encode_plain(dc.flat_patches(imgs, case[2], case[3]))
        listed = torch.tensor([9, total_of(case) + 5, 5, -3], dtype=torch.int32, device=DEV)
        got = plan.encode_source(hip.PatchSource(images=images.pixels, ragged=rview), index=listed, dedup=True)
        assert torch.equal(got, want[torch.tensor([9, 0, 5, 0], device=DEV)])
        flags = dc.host_flags(dc.flat_patches(imgs, case[2], case[3]).cpu())
        assert int(flags[0]) == (0 if blank0 else 1)
        assert int(plan.n_encoded) == dc.host_count(flags[torch.tensor([9, 0, 5, 0])]) == (3 if blank0 else 4)


def test_dedup_on_a_trunk_that_is_not_fused_is_refused():
    net = net_for("mnist50", N=64, M=8, I=8)
    plan = net.selection.plan()
    images, _ = ic.guarded_ragged(ic.POOL50, 0, device=DEV)
    src = hip.PatchSource(images=images.pixels, ragged=images.view((50, 50), (25, 25)))
    with pytest.raises(ValueError):
        plan.encode_source(src, dedup=True)
    assert plan.encode_source(src).shape[0] == src.count                  # (plain launches go on)


def test_entry_refusals_launch_nothing():
    import ctypes as C
    plan = net_for("mnist", N=64, M=8, I=8).selection.plan()
    images, _ = dc.pack(ic.FUSED_MIXED, dc.zero_images(ic.FUSED_MIXED), device=DEV)
    rview = images.view((32, 32), (32, 32)).on(DEV)
    L, n = hip.lib(), rview.count
    plan._refresh()
    tr = C.byref(plan._describe((1, 32, 32)))
    need = L.ipsx_trunk_ragged_view_dedup_workspace_bytes(tr, n)
    ws = torch.zeros((need,), dtype=torch.uint8, device=DEV)
    emb = torch.full((n, 128), 7.0, device=DEV)
    px, rv = images.pixels.data_ptr(), C.byref(rview.struct)

    def call(t=tr, pixels=px, view=rv, first=0, count=n, out=emb.data_ptr(), w=ws.data_ptr(), wb=need):
        return L.ipsx_trunk_encode_ragged_view_dedup(t, pixels, view, None, first, count, out, w, wb, None, None)

    assert call(count=0) == 0                                             # IPSX_OK
    small = call(wb=need - 1)
    assert small == -3 and call(w=None) == small                          # IPSX_EWORKSPACE
    bad = call(count=1 << 31)
    assert bad == -1                                                      # IPSX_EINVAL
    for kw in (dict(t=None), dict(pixels=None), dict(view=None), dict(out=None), dict(first=-1), dict(first=2, count=n - 1)):
        assert call(**kw) == bad, kw
    assert L.ipsx_ragged_view_blank_flags(px, rv, None, 0, n, None, None) == bad
    assert L.ipsx_ragged_view_blank_flags(px, rv, None, 0, 1 << 31, ws.data_ptr(), None) == bad
    torch.cuda.synchronize()
    assert bool((emb == 7.0).all()) and not bool(ws.any())                # no launch wrote anything


# ---------------------------------------------------------------- end to end on the 32-px net
SIZES = [(160, 192), (192, 224), (128, 416), (128, 128), (64, 96)]        # 30, 42, 52, 16 = M and 6 patches at stride 32
PATCH, STRIDE = (32, 32), (32, 32)


def _call(net, imgs, pad):
    """``ips_image_ragged`` from the seed -> (record, n_encoded right behind the call | None)."""
    plan = net.plan
    plan.n_encoded = None
    ic._seed(11)
    out = net.ips_image_ragged(imgs, PATCH, STRIDE, pad=pad)
    n_enc = None if plan.n_encoded is None else int(plan.n_encoded)
    return ic.record(net, out), n_enc


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("pad", [False, True])
def test_call_with_dedup_equals_the_plain_call_and_the_solo_loop(shuffle, pad, monkeypatch):
    net = rc.make_net(rc.image_conf(M=16, shuffle=shuffle, shuffle_style="batch"), DEV)
    host = dc.planted_images(SIZES if pad else SIZES[:3])
    imgs = [im.to(DEV) for im in host]
    flags = dc.host_flags(dc.flat_patches(host, PATCH, STRIDE))
    assert 0 < int(flags.sum()) < flags.numel() // 2
    solo = ic.solo_loop(net, imgs[:3], PATCH, STRIDE)
    monkeypatch.setenv("IPSX_DEDUP_BLANK", "0")
    plain, none = _call(net, imgs, pad)
    assert none is None                                                   # plain launches: nothing counted
    monkeypatch.delenv("IPSX_DEDUP_BLANK")                                # the default: dedup on the fused trunk
    calls = []
    real = type(net.plan).encode_source

    def counted(self, *a, **kw):
        calls.append(kw.get("dedup"))
        return real(self, *a, **kw)
    monkeypatch.setattr(type(net.plan), "encode_source", counted)
    got, n_enc = _call(net, imgs, pad)
    assert calls[:1] == [True] and calls.count(True) == 1                 # exactly one encoder pass, with dedup
    assert n_enc == dc.host_count(flags)
    if pad:
        ic.assert_same_padded(got, plain)
        assert got["count"] == (16, 16, 16, 16, 6)
        for key in ("mem_patch", "mem_pos", "mem_idx", "mem_emb"):
            assert ic.same_bits(got[key][:3], solo[key]), key
        if shuffle:
            for g, w in zip(got["shuffle"][:3], solo["shuffle"]):
                assert torch.equal(g, w)
    else:
        rc.assert_same_record(got, plain)
        rc.assert_same_record(got, solo)
        assert got["count"] is None
