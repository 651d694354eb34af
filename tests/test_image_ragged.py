"""ips_image_ragged() on the GPU: the stems read the patches of images of DIFFERENT sizes where they lie.

Yardstick everywhere: the existing routes on the same patches copied out of the images, compared bit for bit - behind the
staged patch the ragged view kernels run the code of the view kernels, so there is no tolerance.  Inputs carry NaN in every
pixel no patch covers, between the images and around the buffer: a stray read changes bits or breaks finiteness."""

import pytest
import torch

import image_ragged_cases as ic
import ragged_cases as rc
from ips_amd import hip, synth
from ips_amd.architecture import IPSNet
from ips_amd.ragged_image import RaggedImages
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


def flat_patches(imgs, patch, stride):
    """The patches of every image in unfold order, one image after the other: (total, C, ph, pw)."""
    return torch.cat([unfold(im[None], patch, stride)[0] for im in imgs]).contiguous()


def check_encoder(net, case, bases=(0,), firsts=()):
    c, sizes, patch, stride = case
    plan = net.selection.plan()
    for k in bases:
        images, imgs = ic.guarded_ragged(case, k, device=DEV)
        assert images.pixels.data_ptr() % 16 == 4 * k
        rview = images.view(patch, stride)
        assert plan.ragged_view_supported(rview)
        patches = flat_patches(imgs, patch, stride)
        assert patches.shape[0] == rview.count and bool(torch.isfinite(patches).all())
        want = plan.encode_plain(patches)
        src = hip.PatchSource(images=images.pixels, ragged=rview)
        got = plan.encode_source(src)
        assert bool(torch.isfinite(got).all()) and torch.equal(got, want)
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
            assert torch.equal(plan.encode_source(src, first=first, n=n), want[first:first + n])
    torch.cuda.synchronize()


def test_fused_trunk_dword_loads():
    check_encoder(net_for("mnist", N=64, M=8, I=8), ic.FUSED_MIXED, firsts=[(13, 6)])     # (first > 0 lands inside the second image)


def test_fused_trunk_wide_loads_and_a_base_four_bytes_off():
    check_encoder(net_for("mnist", N=64, M=8, I=8), ic.FUSED_ALIGNED, bases=(0, 1), firsts=[(13, 6)])


def test_fused_trunk_a_whole_round_and_the_pair_remainder():
    cus = hip.device_geometry(DEV).cus
    total = sum(ny * nx for ny, nx in ic.grids(ic.FUSED_ROUND))
    assert total >= 8 * cus + 5, "the shape is meant to fill one whole round of the eight-patch kernel and leave a remainder"
    check_encoder(net_for("mnist", N=64, M=8, I=8), ic.FUSED_ROUND, firsts=[(2110, 100)])


def test_stem_pool50():
    check_encoder(net_for("mnist50", N=64, M=8, I=8), ic.POOL50, bases=(0, 1), firsts=[(35, 9)])


def test_stem_pool50_float2_loads():
    check_encoder(net_for("mnist50", N=64, M=8, I=8), ic.POOL50_EVEN, firsts=[(28, 6)])


def test_stem_pool50_across_the_two_stream_cut():
    check_encoder(net_for("mnist50", N=64, M=8, I=8), ic.POOL50_CUT, firsts=[(1023, 9), (1050, 12)])


@pytest.mark.parametrize("case", [ic.POOL100, ic.POOL100_HALF, ic.POOL100_WIDE], ids=["stride100", "stride50", "wide"])
def test_stem_pool100x3(case):
    total = sum(ny * nx for ny, nx in ic.grids(case))
    check_encoder(net_for("traffic", N=48, M=16, I=32), case, bases=(0, 1), firsts=[(5, min(4, total - 5))])


# ---------------------------------------------------------------- the finish launch
@pytest.mark.parametrize("case,k,M", [(ic.FUSED_ALIGNED, 0, 10), (ic.FUSED_MIXED, 0, 10), (ic.FUSED_ALIGNED, 1, 10), (ic.POOL100_HALF, 0, 8)],
                         ids=["wide", "dword", "off_base", "three_channels"])       # (M = 10: 12 long, 10 exactly M, 9 and 1 short)
@pytest.mark.parametrize("with_flat", [False, True])
@pytest.mark.parametrize("with_pos", [False, True])
def test_finish_view_equals_the_per_image_gather_plus_the_padding_rule(case, k, M, with_flat, with_pos):
    c, sizes, patch, stride = case
    images, imgs = ic.guarded_ragged(case, k, device=DEV)
    rview = images.view(patch, stride)
    B, total, lengths = len(sizes), rview.count, rview.lengths
    assert any(n > M for n in lengths) and any(n < M for n in lengths)        # long and short images
    g = torch.Generator().manual_seed(17)
    mem_idx = torch.stack([torch.randperm(max(n, M), generator=g)[:M] % n for n in lengths]).to(DEV)
    offsets = torch.tensor(rview.firsts + (total,), dtype=torch.int64, device=DEV)
    flat = None
    if with_flat:                                             # a permutation inside every image
        flat = torch.cat([f + torch.randperm(n, generator=g) for f, n in zip(rview.firsts, lengths)]).to(torch.int32).to(DEV)
    pos = torch.randn((total, 32), generator=g).to(DEV) if with_pos else None
    # the output buffers are NaN (indices: -7) beforehand: the launch writes every slot, the padding too
    nan = float("nan")
    bufs = (torch.full((B, M, c) + tuple(patch), nan, device=DEV), torch.full((B, M, 32), nan, device=DEV) if with_pos else None,
            torch.full((B, M), -7, dtype=torch.int64, device=DEV), torch.full((B, M), -7, dtype=torch.int64, device=DEV))
    out, out_pos, idx, grow = hip.ragged_finish_view(images.pixels, rview, offsets, mem_idx, M, flat, pos, out=bufs)
    assert out is bufs[0] and idx is bufs[2]
    torch.cuda.synchronize()
    for b, (im, n, f) in enumerate(zip(imgs, lengths, rview.firsts)):
        view = hip.PatchView((1,) + tuple(im.shape), patch, stride)
        local = mem_idx[b] if n > M else torch.arange(M, device=DEV).clamp(max=n - 1)
        src = local if flat is None else flat[f + local].to(torch.int64) - f
        want = hip.gather_patches_view(im[None].contiguous(), view, src[None])[0]
        valid = min(n, M)
        assert ic.same_bits(out[b, :valid], want[:valid]), b
        assert idx[b, :valid].tolist() == local[:valid].tolist() and grow[b, :valid].tolist() == (f + local[:valid]).tolist()
        if with_pos:
            assert ic.same_bits(out_pos[b, :valid], pos[f + local[:valid]])
        if valid < M:                                         # +0.0 behind the rows, index and row -1
            assert ic.same_bits(out[b, valid:], torch.zeros_like(out[b, valid:]))
            assert idx[b, valid:].tolist() == [-1] * (M - valid) == grow[b, valid:].tolist()
            if with_pos:
                assert ic.same_bits(out_pos[b, valid:], torch.zeros_like(out_pos[b, valid:]))
    assert bool(torch.isfinite(out).all())


# ---------------------------------------------------------------- end to end on the 32-px net
SIZES = [(160, 192), (192, 224), (128, 416), (128, 128), (64, 96)]        # 30, 42, 52, 16 = M and 6 patches at stride 32
PATCH, STRIDE = (32, 32), (32, 32)


def _on_device(imgs):
    return [im.to(DEV) for im in imgs]


def _counted(monkeypatch, net):
    seen = []

    def counted(name, real):
        def call(*a, **k):
            seen.append(name)
            return real(*a, **k)
        return call
    for name in ("scan_ragged", "ragged_finish_view", "ragged_finish", "patchify", "gather_rows", "logits", "scan", "scan_range",
                 "gather_patches_view"):
        monkeypatch.setattr(hip, name, counted(name, getattr(hip, name)))
    plan = type(net.plan)
    for name in ("encode", "encode_source"):
        monkeypatch.setattr(plan, name, counted("encode", getattr(plan, name)))
    return seen


@pytest.mark.parametrize("shuffle", [False, True])
def test_padded_call_equals_the_ragged_call_on_patches_and_the_solo_loop(shuffle, monkeypatch):
    net = rc.make_net(rc.image_conf(M=16, shuffle=shuffle, shuffle_style="batch"), DEV)
    imgs = _on_device(ic.make_images(SIZES))
    slides = [hip.patchify(im[None], PATCH, STRIDE)[0] for im in imgs]
    want = ic.patch_call(net, slides, pad=True)
    solo = ic.solo_loop(net, imgs[:3], PATCH, STRIDE)
    seen = _counted(monkeypatch, net)
    got = ic.image_call(net, imgs, PATCH, STRIDE, pad=True)
    # the viewed route: one encoder pass, one logits table, ONE loop launch, ONE finish launch, no patch tensor
    # (reading last_mem_emb gathers; with a short image it also embeds one all-zero patch)
    assert sorted(n for n in seen if n not in ("gather_rows", "encode")) == ["logits", "ragged_finish_view", "scan_ragged"]
    assert seen[0] == "encode" and seen.index("gather_rows") > seen.index("ragged_finish_view")
    ic.assert_same_padded(got, want)
    assert got["count"] == (16, 16, 16, 16, 6)
    for key in ("mem_patch", "mem_pos", "mem_idx", "mem_emb"):
        assert ic.same_bits(got[key][:3], solo[key]), key
    if shuffle:
        for g, w in zip(got["shuffle"][:3], solo["shuffle"]):
            assert torch.equal(g, w)
        assert got["shuffle"][3] is None and got["shuffle"][4] is None


@pytest.mark.parametrize("shuffle", [False, True])
def test_call_without_pad_on_the_long_images(shuffle, monkeypatch):
    net = rc.make_net(rc.image_conf(M=16, shuffle=shuffle, shuffle_style="batch"), DEV)
    imgs = _on_device(ic.make_images(SIZES[:3]))
    want = ic.solo_loop(net, imgs, PATCH, STRIDE)
    seen = _counted(monkeypatch, net)
    p, q = net.ips_image_ragged(imgs, PATCH, STRIDE)
    assert sorted(seen) == ["encode", "logits", "ragged_finish_view", "scan_ragged"]
    got = ic.image_call(net, imgs, PATCH, STRIDE)
    rc.assert_same_record(got, want)
    assert got["count"] is None
    rc.assert_same_record(ic.patch_call(net, [hip.patchify(im[None], PATCH, STRIDE)[0] for im in imgs]), want)


def test_a_host_resident_list_and_the_container():
    net = rc.make_net(rc.image_conf(M=16), DEV)
    host = ic.make_images(SIZES)
    on_dev = ic.image_call(net, _on_device(host), PATCH, STRIDE, pad=True)
    ic.assert_same_padded(ic.image_call(net, host, PATCH, STRIDE, pad=True), on_dev)
    ic.assert_same_padded(ic.image_call(net, host, PATCH, STRIDE, pad=True, through_ips_image=True), on_dev)
    r = RaggedImages.from_list(host, pad=True).pin_memory()
    assert r.pixels.is_pinned() and r.to(DEV).sizes == r.sizes
    ic.assert_same_padded(ic.record(net, net.ips_image(r, PATCH, STRIDE)), on_dev)


def test_a_trunk_without_the_ragged_view_materialises(monkeypatch):
    """IPSX_PRECISION=bf16: the trunk reads no view, the patch tensors are made and ips_ragged runs unchanged."""
    monkeypatch.setenv("IPSX_PRECISION", "bf16")
    net = rc.make_net(rc.image_conf(M=16), DEV)
    imgs = _on_device(ic.make_images(SIZES))
    want = ic.patch_call(net, [hip.patchify(im[None], PATCH, STRIDE)[0] for im in imgs], pad=True)
    seen = _counted(monkeypatch, net)
    got = ic.image_call(net, imgs, PATCH, STRIDE, pad=True)
    assert seen.count("patchify") == len(imgs) and "ragged_finish_view" not in seen and seen.count("scan_ragged") == 1
    ic.assert_same_padded(got, want)
