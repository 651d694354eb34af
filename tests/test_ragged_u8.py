"""uint8 on the ragged routes on the GPU: the stems, the blank scan and the finish launch read the BYTES of
images of different sizes where they lie, through the patch table.

Yardstick everywhere: the same entry on the float32 expansion ``table[c][byte]`` (and the existing uint8 routes on the same
patches copied out), compared bit for bit - behind the staged patch the kernels are the float32 ones, so there is no
tolerance.  The byte buffers carry 255 in every pixel no patch covers, between the images and around the buffer, and the
table maps 255 to 1e30: a read outside a patch window blows the embedding up."""

import ctypes as C

import pytest
import torch

import image_ragged_cases as ic
import image_ragged_dedup_cases as dc
import ragged_cases as rc
import ragged_u8_cases as uc
import view_u8_cases as vu
from ips_amd import hip, synth
from ips_amd.architecture import IPSNet
from ips_amd.quant import dequant
from view_cases import unfold

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
_NETS = {}


def net_for(kind, **over):
    """One net per configuration for the whole module (weights packed once)."""
    key = (kind, tuple(sorted(over.items())))
    if key not in _NETS:
        conf = {"mnist": lambda: synth.mnist_conf(**over), "mnist50": lambda: synth.mnist_conf(patch=50, **over),
                "traffic": lambda: synth.traffic_conf(**over)}[kind]()
        _NETS[key] = synth.fill_weights(IPSNet(DEV, conf), 5).to(DEV).eval()
    return _NETS[key]


@pytest.fixture(params=[0, 1], ids=["split_rule", "eight_patch_kernel"])
def trunk_mode(request):
    """The fused trunk's kernel choice (ipsx_dbg_fused_trunk_pair): 0 the product's rule - these small lists go through the
    pair kernel -, 1 every patch through the eight-patch kernel."""
    fn = hip.lib().ipsx_dbg_fused_trunk_pair
    fn.restype, fn.argtypes = None, [C.c_int]
    fn(request.param)
    yield request.param
    fn(0)


def flat_patches(imgs, patch, stride):
    return torch.cat([unfold(im[None], patch, stride)[0] for im in imgs]).contiguous()


def packed(case, k=0, shifts=None, seed=0, imgs=None):
    """-> (uint8 RaggedImages on the device, its host images, the guard table on the device)"""
    imgs = uc.guarded_images_u8(case, seed=seed) if imgs is None else imgs
    images, _ = uc.pack_u8(case, imgs, k, shifts, device=DEV)
    assert images.pixels.data_ptr() % 16 == k
    return images, imgs, vu.guard_table(case[0]).to(DEV)


# ---------------------------------------------------------------- 6. the encoder pass, per stem
def check_encoder(net, case, bases=(0,), shifts=None, firsts=()):
    c, sizes, patch, stride = case
    plan = net.selection.plan()
    for k in bases:
        images, imgs, table = packed(case, k, shifts)
        rview = images.view(patch, stride)
        assert plan.ragged_view_supported(rview)
        # the float32 ragged view of the expanded buffer, and the trunk on the materialised uint8 patches
        wide = uc.expanded(images, table)
        want = plan.encode_source(hip.PatchSource(images=wide.pixels, ragged=wide.view(patch, stride)))
        patches = flat_patches([im.to(DEV) for im in imgs], patch, stride)
        assert patches.dtype == torch.uint8 and patches.shape[0] == rview.count and int(patches.max()) < 255
        assert torch.equal(plan.encode_plain(patches, table=table), want)
        src = hip.PatchSource(images=images.pixels, ragged=rview, table=table)
        assert src.dtype == torch.uint8 and src.count == rview.count
        got = plan.encode_source(src)
        assert bool(torch.isfinite(got).all()) and float(got.abs().max()) < 1e20 and torch.equal(got, want)
        # a permutation with a repeated entry and one that is no packed patch: it reads packed patch 0
        perm = torch.randperm(rview.count, generator=torch.Generator().manual_seed(3 + k))
        listed = perm.clone()
        listed[-1] = listed[0]
        take = listed.clone()
        if rview.count > 2:
            listed[1], take[1] = rview.count + 5, 0
        got = plan.encode_source(src, index=listed.to(torch.int32).to(DEV))
        assert torch.equal(got, want[take.to(DEV)])
        for first, n in firsts:
            assert torch.equal(plan.encode_source(src, first=first, n=n), want[first:first + n]), (first, n)
    torch.cuda.synchronize()


# (ALL16: 12 + 9 + 1 + 10 patches; n = 7, 8, 9 around a workgroup's edge, (10, 6) and (20, 9) cross image boundaries)
RANGES = [(0, 7), (3, 8), (5, 9), (10, 6), (20, 9)]


def test_fused_trunk_tiers_16_4_1_by_the_base(trunk_mode):
    check_encoder(net_for("mnist", N=64, M=8, I=8), uc.ALL16, bases=(0, 4, 1), firsts=RANGES)


def test_fused_trunk_second_image_four_bytes_past_a_16_byte_boundary(trunk_mode):
    check_encoder(net_for("mnist", N=64, M=8, I=8), uc.ALL16, shifts=[0, 4, 0, 0], firsts=[(10, 6)])


def test_fused_trunk_pair_kernel_eight_byte_loads():
    check_encoder(net_for("mnist", N=64, M=8, I=8), uc.ALL16, bases=(8,), firsts=[(13, 6)])


def test_fused_trunk_odd_widths(trunk_mode):
    check_encoder(net_for("mnist", N=64, M=8, I=8), ic.FUSED_MIXED, firsts=[(13, 6)])


def test_fused_trunk_a_whole_round_and_the_pair_remainder():
    cus = hip.device_geometry(DEV).cus
    total = sum(ny * nx for ny, nx in ic.grids(ic.FUSED_ROUND))
    assert total >= 8 * cus + 5, "the shape is meant to fill one whole round of the eight-patch kernel and leave a remainder"
    check_encoder(net_for("mnist", N=64, M=8, I=8), ic.FUSED_ROUND, firsts=[(2110, 100)])


@pytest.mark.parametrize("case,bases,firsts", [(ic.POOL50, (0, 1), [(35, 9)]), (ic.POOL50_EVEN, (0, 1), [(28, 6)]),
                                               (ic.POOL50_CUT, (0,), [(1023, 9), (1050, 12)])], ids=["odd", "even", "cut"])
def test_stem_pool50(case, bases, firsts):
    check_encoder(net_for("mnist50", N=64, M=8, I=8), case, bases=bases, firsts=firsts)


@pytest.mark.parametrize("case", [ic.POOL100, ic.POOL100_HALF, ic.POOL100_WIDE], ids=["stride100", "stride50", "wide"])
def test_stem_pool100x3(case):
    total = sum(ny * nx for ny, nx in ic.grids(case))
    check_encoder(net_for("traffic", N=48, M=16, I=32), case, bases=(0, 2), firsts=[(5, min(4, total - 5))])


def test_a_byte_source_refuses_what_uint8_patches_refuse(monkeypatch):
    images, _, table = packed(uc.ALL16)
    rview = images.view((32, 32), (32, 32))
    with pytest.raises(TypeError):
        hip.PatchSource(images=images.pixels, ragged=rview)                        # bytes without a table
    with pytest.raises(ValueError):
        hip.PatchSource(images=images.pixels, ragged=rview, table=vu.guard_table(3).to(DEV))
    monkeypatch.setenv("IPSX_PRECISION", "bf16")
    with pytest.raises(TypeError):
        hip.PatchSource(images=images.pixels, ragged=rview, table=table)


# ---------------------------------------------------------------- 7. the finish launch
@pytest.mark.parametrize("case,k,M", [(uc.ALL16, 0, 10), (ic.FUSED_ALIGNED, 0, 10), (ic.FUSED_MIXED, 0, 10), (uc.ALL16, 1, 10),
                                      (ic.POOL100_HALF, 0, 8), (ic.FUSED_ROUND, 0, 4)],
                         ids=["sixteen", "dword", "byte", "odd_base", "three_channels", "no_short_image"])
@pytest.mark.parametrize("with_flat", [False, True])
@pytest.mark.parametrize("with_pos", [False, True])
def test_finish_view_with_a_table_equals_the_per_image_gather_plus_the_padding_rule(case, k, M, with_flat, with_pos):
    c, sizes, patch, stride = case
    images, imgs, table = packed(case, k)
    rview = images.view(patch, stride)
    B, total, lengths = len(sizes), rview.count, rview.lengths
    assert any(n > M for n in lengths)
    g = torch.Generator().manual_seed(17)
    mem_idx = torch.stack([torch.randperm(max(n, M), generator=g)[:M] % n for n in lengths]).to(DEV)
    offsets = torch.tensor(rview.firsts + (total,), dtype=torch.int64, device=DEV)
    flat = None
    if with_flat:                                             # a permutation inside every image
        flat = torch.cat([f + torch.randperm(n, generator=g) for f, n in zip(rview.firsts, lengths)]).to(torch.int32).to(DEV)
    pos = torch.randn((total, 32), generator=g).to(DEV) if with_pos else None
    nan = float("nan")                                        # the launch writes every slot, the padding too
    bufs = (torch.full((B, M, c) + tuple(patch), nan, device=DEV), torch.full((B, M, 32), nan, device=DEV) if with_pos else None,
            torch.full((B, M), -7, dtype=torch.int64, device=DEV), torch.full((B, M), -7, dtype=torch.int64, device=DEV))
    out, out_pos, idx, grow = hip.ragged_finish_view(images.pixels, rview, offsets, mem_idx, M, flat, pos, out=bufs, table=table)
    assert out is bufs[0] and out.dtype == torch.float32
    torch.cuda.synchronize()
    for b, (im, n, f) in enumerate(zip(imgs, lengths, rview.firsts)):
        view = hip.PatchView((1,) + tuple(im.shape), patch, stride)
        local = mem_idx[b] if n > M else torch.arange(M, device=DEV).clamp(max=n - 1)
        src = local if flat is None else flat[f + local].to(torch.int64) - f
        want = hip.gather_patches_view(im[None].to(DEV).contiguous(), view, src[None], table)[0]
        valid = min(n, M)
        assert ic.same_bits(out[b, :valid], want[:valid]), b
        assert idx[b, :valid].tolist() == local[:valid].tolist() and grow[b, :valid].tolist() == (f + local[:valid]).tolist()
        if with_pos:
            assert ic.same_bits(out_pos[b, :valid], pos[f + local[:valid]])
        if valid < M:                                         # float +0.0 behind the rows - not table[c][0] -, index and row -1
            assert ic.same_bits(out[b, valid:], torch.zeros_like(out[b, valid:]))
            assert idx[b, valid:].tolist() == [-1] * (M - valid) == grow[b, valid:].tolist()
            if with_pos:
                assert ic.same_bits(out_pos[b, valid:], torch.zeros_like(out_pos[b, valid:]))
    assert bool(torch.isfinite(out).all()) and float(out.abs().max()) < 1e20


# ---------------------------------------------------------------- 8. the byte blank flags
def planted_bytes(case):
    """All-zero byte windows (255 elsewhere) with, in image 0, ONE non-zero byte at a corner of the windows at (0, 0), (0, 64),
    (64, 0), (64, 64); its window at (32, 32) stays zero although the 255s of no-patch pixels and planted bytes one column to
    its right and one row below touch it from outside; image 1: a lone byte in row 20 of the window at (32, 32), the window
    at (64, 64) full."""
    imgs = uc.guarded_images_u8(case, zero=True)
    a, b = imgs[0][0], imgs[1][0]
    a[0, 0] = 1
    a[0, 64 + 31] = 2
    a[64 + 31, 0] = 254
    a[64 + 31, 64 + 31] = 4
    a[32 + 5, 64] = 5                 # one column right of the window at (32, 32)
    a[64, 32 + 7] = 6                 # one row below it
    b[32 + 20, 32 + 9] = 1
    b[64:96, 64:96] = torch.randint(1, 255, (32, 32), generator=torch.Generator().manual_seed(1), dtype=torch.uint8)
    return imgs


def host_byte_flags(patches):
    """The host rule on bytes: 1 where any byte of the window is not 0."""
    return (patches.reshape(patches.shape[0], -1) != 0).any(dim=1).to(torch.int32)


def patch_at(case, b, y0, x0):
    grids = ic.grids(case)
    return sum(ny * nx for ny, nx in grids[:b]) + (y0 // case[3][0]) * grids[b][1] + x0 // case[3][1]


@pytest.mark.parametrize("case,k", [(uc.ALL16, 0), (ic.FUSED_ALIGNED, 0), (ic.FUSED_MIXED, 0), (uc.ALL16, 1), (dc.STRIDE16, 0)],
                         ids=["sixteen", "dword", "byte", "odd_base", "stride16"])
def test_byte_flags_equal_the_host_rule_on_planted_content(case, k):
    c, sizes, patch, stride = case
    images, imgs, _ = packed(case, k, imgs=planted_bytes(case))
    rview = images.view(patch, stride)
    want = host_byte_flags(flat_patches(imgs, patch, stride))
    assert want.numel() == rview.count and 0 < int(want.sum()) < rview.count // 2            # mostly blank
    assert want[patch_at(case, 0, 32, 32)] == 0 and want[patch_at(case, 1, 32, 32)] == 1
    for y0, x0 in ((0, 0), (0, 64), (64, 0), (64, 64)):
        assert want[patch_at(case, 0, y0, x0)] == 1
    got = hip.ragged_blank_flags(images.pixels, rview)
    assert got.dtype == torch.int32 and torch.equal(got.cpu(), want)
    listed = torch.randperm(rview.count, generator=torch.Generator().manual_seed(3 + k))
    listed[-1] = listed[0]
    take = listed.clone()
    listed[1], take[1] = rview.count + 5, 0                  # no packed patch: flagged as packed patch 0
    got = hip.ragged_blank_flags(images.pixels, rview, index=listed.to(torch.int32).to(DEV))
    assert torch.equal(got.cpu(), want[take])
    first = rview.firsts[1] + 1
    assert torch.equal(hip.ragged_blank_flags(images.pixels, rview, first=first, n=6).cpu(), want[first:first + 6])
    assert hip.ragged_blank_flags(images.pixels, rview, first=3, n=0).numel() == 0


# ---------------------------------------------------------------- 9. dedup encode equals plain encode
def byte_windows(case, keep, seed=0):
    """Host byte images of ``case``: bytes 1..254 in the windows of the packed patches ``keep``, 0 in the other windows, 255
    where no window lies."""
    imgs = uc.guarded_images_u8(case, zero=True)
    firsts = [0]
    for ny, nx in ic.grids(case):
        firsts.append(firsts[-1] + ny * nx)
    g = torch.Generator().manual_seed(seed)
    (ph, pw) = case[2]
    for p in keep:
        b = max(i for i in range(len(firsts) - 1) if firsts[i] <= p)
        y0, x0 = dc.window(case, b, p - firsts[b])
        imgs[b][:, y0:y0 + ph, x0:x0 + pw] = torch.randint(1, 255, (case[0], ph, pw), generator=g, dtype=torch.uint8)
    return imgs


def check_dedup(case, imgs, k=0, listed=None, ranges=()):
    c, sizes, patch, stride = case
    plan = net_for("mnist", N=64, M=8, I=8).selection.plan()
    images, imgs, table = packed(case, k, imgs=imgs)
    rview = images.view(patch, stride)
    flags = host_byte_flags(flat_patches(imgs, patch, stride))
    src = hip.PatchSource(images=images.pixels, ragged=rview, table=table)
    want = plan.encode_source(src)                            # the plain launches (held to the float32 expansion above)
    plan.n_encoded = None
    got = plan.encode_source(src, dedup=True)
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) < 1e20 and torch.equal(got, want)
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


def test_dedup_no_blank_patch_encodes_every_entry():
    flags = check_dedup(uc.ALL16, byte_windows(uc.ALL16, range(total_of(uc.ALL16))))
    assert int(flags.sum()) == total_of(uc.ALL16)


def test_dedup_all_blank_encodes_one_entry():
    """The one blank entry is read from its image: every pixel table[0] = 0.5, not 0.0f."""
    flags = check_dedup(ic.FUSED_MIXED, byte_windows(ic.FUSED_MIXED, []))
    assert int(flags.sum()) == 0


def test_dedup_exactly_one_blank_patch():
    n = total_of(ic.FUSED_ALIGNED)
    flags = check_dedup(ic.FUSED_ALIGNED, byte_windows(ic.FUSED_ALIGNED, [p for p in range(n) if p != 17]), k=1)
    assert int(flags.sum()) == n - 1 and flags[17] == 0


@pytest.mark.parametrize("nonblank", [7, 8, 9])
def test_dedup_count_just_before_on_and_after_a_workgroups_edge(nonblank):
    case = uc.ALL16                                           # 12 + 9 + 1 + 10 windows that do not overlap
    keep = [1, 4, 11, 12, 13, 20, 21, 22, 31][:nonblank]
    listed = torch.randperm(32, generator=torch.Generator().manual_seed(9))
    listed[-1] = listed[0]
    flags = check_dedup(case, byte_windows(case, keep), listed=listed, ranges=[(13, 6), (2, 30)])
    assert int(flags.sum()) == nonblank and total_of(case) == 32


def test_dedup_a_whole_round_about_half_blank():
    cus = hip.device_geometry(DEV).cus
    case = ic.FUSED_ROUND
    total = total_of(case)
    assert total >= 8 * cus + 5
    imgs = uc.guarded_images_u8(case, seed=4)
    for im in imgs:                                           # content in the upper half only; 255 stays where no window lies
        lower = im[:, im.shape[1] // 2:]
        lower[lower != 255] = 0
    flags = check_dedup(case, imgs, ranges=[(2110, 100)])
    assert total // 3 < int(flags.sum()) < 2 * total // 3


def test_dedup_on_a_trunk_that_is_not_fused_is_refused():
    plan = net_for("mnist50", N=64, M=8, I=8).selection.plan()
    images, _, table = packed(ic.POOL50)
    src = hip.PatchSource(images=images.pixels, ragged=images.view((50, 50), (25, 25)), table=table)
    with pytest.raises(ValueError):
        plan.encode_source(src, dedup=True)
    assert plan.encode_source(src).shape[0] == src.count      # (plain launches go on)


# ---------------------------------------------------------------- 10. end to end
SIZES = [(160, 192), (192, 224), (128, 416), (128, 128), (64, 96)]        # 30, 42, 52, 16 = M and 6 patches at stride 32
PATCH, STRIDE = (32, 32), (32, 32)


def _counted(monkeypatch, net):
    seen = []

    def counted(name, real):
        def call(*a, **k):
            seen.append(name)
            return real(*a, **k)
        return call
    for name in ("scan_ragged", "ragged_finish_view", "ragged_finish", "patchify", "gather_rows", "logits", "scan", "scan_range",
                 "gather_patches_view", "dequant_patches"):
        monkeypatch.setattr(hip, name, counted(name, getattr(hip, name)))
    plan = type(net.plan)
    for name in ("encode", "encode_source"):
        monkeypatch.setattr(plan, name, counted("encode", getattr(plan, name)))
    real = hip.lib().ipsx_ragged_finish_view_u8
    monkeypatch.setattr(hip.lib(), "ipsx_ragged_finish_view_u8", counted("ipsx_ragged_finish_view_u8", real))
    return seen


@pytest.mark.parametrize("dedup", [None, "0"], ids=["dedup_auto", "dedup_off"])
@pytest.mark.parametrize("pad", [False, True])
@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("resident", ["device", "host"])
def test_image_call_on_bytes_equals_the_call_on_the_expansion(resident, shuffle, pad, dedup, monkeypatch):
    if dedup is None:
        monkeypatch.delenv("IPSX_DEDUP_BLANK", raising=False)
    else:
        monkeypatch.setenv("IPSX_DEDUP_BLANK", dedup)
    net = rc.make_net(rc.image_conf(M=16, shuffle=shuffle, shuffle_style="batch"), DEV)
    table = vu.plain_table(1)
    net.set_patch_table(table)
    host = uc.byte_images(SIZES if pad else SIZES[:3])
    imgs = [im.to(DEV) for im in host] if resident == "device" else host
    wide = [dequant(im, table.to(im.device)) for im in imgs]
    want = ic.image_call(net, wide, PATCH, STRIDE, pad=pad)
    solo = ic.solo_loop(net, imgs[:3], PATCH, STRIDE)
    seen = _counted(monkeypatch, net)
    got = ic.image_call(net, imgs, PATCH, STRIDE, pad=pad)
    # one encoder pass, one logits table, ONE loop launch, ONE finish launch on the bytes, no patch tensor, nothing dequantised
    # (reading last_mem_emb gathers; with a short image it also embeds one all-zero patch)
    assert sorted(n for n in seen if n not in ("gather_rows", "encode")) == \
        ["ipsx_ragged_finish_view_u8", "logits", "ragged_finish_view", "scan_ragged"]
    # (the zero patch goes through encode() and, inside it, encode_source(): both are counted)
    finish = seen.index("ragged_finish_view")
    assert seen[0] == "encode" and "encode" not in seen[1:finish] and seen[finish:].count("encode") == (2 if pad else 0)
    assert seen.index("gather_rows") > finish
    ic.assert_same_padded(got, want)
    assert got["mem_patch"].dtype == torch.float32
    for key in ("mem_patch", "mem_pos", "mem_idx", "mem_emb"):
        assert ic.same_bits(got[key][:3], solo[key]), key
    if shuffle:
        for g, w in zip(got["shuffle"][:3], solo["shuffle"]):
            assert torch.equal(g, w)
    if not pad:                                               # the solo loop ends where the call ends: RNG states included
        assert torch.equal(got["rng"], solo["rng"]) and torch.equal(got["rng_cuda"], solo["rng_cuda"])


def test_bytes_take_the_dedup_route_on_the_fused_trunk(monkeypatch):
    monkeypatch.delenv("IPSX_DEDUP_BLANK", raising=False)
    net = rc.make_net(rc.image_conf(M=16), DEV)
    net.set_patch_table(vu.plain_table(1))
    imgs = [im.mul(50).clamp(0, 255).to(torch.uint8).to(DEV) for im in dc.planted_images(SIZES[:3])]
    net.plan.n_encoded = None
    net.ips_image_ragged(imgs, PATCH, STRIDE)
    flags = host_byte_flags(flat_patches(imgs, PATCH, STRIDE).cpu())
    assert 0 < int(flags.sum()) < flags.numel() and int(net.plan.n_encoded) == dc.host_count(flags)


def test_peak_memory_stays_below_the_patch_tensor_that_was_not_made():
    """An overlapping stride (8): the uint8 patch tensor would be 16 x the images, 1,024 B per patch.  What the call does
    allocate per patch: the embedding (128 floats, 512 B), the logits (32 floats, 128 B) and a few index words - about 670 B;
    a positional row would be another 512 B, so the net has none.  The plan's workspace is kept between calls like the packed
    weights and is allocated by the warm-up call."""
    net = rc.make_net(synth.mnist_conf(N=4096, M=16, I=16, use_pos=False), DEV)
    net.set_patch_table(vu.plain_table(1))
    imgs = [im.to(DEV) for im in uc.byte_images([(320, 352), (288, 416), (352, 320)])]
    stride = (8, 8)
    n_patches = sum(((h - 32) // 8 + 1) * ((w - 32) // 8 + 1) for _, h, w in (im.shape for im in imgs))
    net.ips_image_ragged(imgs, PATCH, stride)                 # (warm: weights packed, workspaces sized)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.memory_allocated(DEV)
    net.ips_image_ragged(imgs, PATCH, stride)
    torch.cuda.synchronize()
    above = torch.cuda.max_memory_allocated(DEV) - base
    print("peak above the input: {} B, the uint8 patch tensor: {} B".format(above, n_patches * 1024))
    assert above < n_patches * 1024


# ---------------------------------------------------------------- 11. ips_ragged on uint8 slides
def byte_slides(lengths, c, h, w, seed=5):
    out = []
    for k, n in enumerate(lengths):
        g = torch.Generator().manual_seed(seed + 7 * k)
        s = torch.randint(0, 256, (n, c, h, w), dtype=torch.uint8, generator=g)
        s[torch.rand(n, generator=g) < 0.5] = 0
        out.append(s.to(DEV))
    return out


@pytest.mark.parametrize("kind,shape,pad", [("mnist", (1, 32, 32), False), ("mnist", (1, 32, 32), True), ("mnist50", (1, 50, 50), True),
                                            ("traffic", (3, 100, 100), True)],
                         ids=["fused", "fused_short_slide", "pool50_aten_finish", "pool100_short_slide"])
@pytest.mark.parametrize("shuffle", [False, True])
def test_ips_ragged_on_byte_slides_equals_the_float32_call(kind, shape, pad, shuffle, monkeypatch):
    over = dict(N=64, M=16, I=16, shuffle=shuffle, shuffle_style="batch")
    conf = synth.mnist_conf(**over) if kind == "mnist" else synth.mnist_conf(patch=50, **over) if kind == "mnist50" \
        else synth.traffic_conf(**over)
    net = synth.fill_weights(IPSNet(DEV, conf), 5).to(DEV).eval()
    table = vu.plain_table(shape[0])
    net.set_patch_table(table)
    slides = byte_slides((40, 23) + ((5, 16) if pad else ()), *shape)
    want = ic.patch_call(net, [dequant(s, table.to(DEV)) for s in slides], pad=pad)
    seen = _counted(monkeypatch, net)
    got = ic.patch_call(net, slides, pad=pad)
    ic.assert_same_padded(got, want)                          # last_shuffle: what the float32 call keeps
    assert got["mem_patch"].dtype == torch.float32 and seen.count("dequant_patches") == 1
    # rows of 2,500 bytes are no whole 16-byte units: the gather launches; 1,024 and 30,000 are: the one finish launch
    assert ("ragged_finish" in seen) == (shape != (1, 50, 50)) and seen.count("scan_ragged") == 1
    if pad:
        assert ic.same_bits(got["mem_patch"][2, 5:], torch.zeros((11,) + shape)) and got["count"] == (16, 16, 5, 16)
        assert ic.same_bits(got["mem_patch"][2, :5], dequant(slides[2], table.to(DEV)).cpu())
    else:
        rc.assert_same_record(got, rc.solo_loop(net, slides))
