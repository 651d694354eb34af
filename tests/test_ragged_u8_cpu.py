"""uint8 on the ragged routes without a GPU: ``ips_ragged`` and ``ips_image_ragged`` on bytes with a patch
table equal, bit for bit, the same call on the float32 expansion ``table[c][byte]`` - everything returned and left behind, the
RNG included; every refusal comes before the RNG moves; the byte load-width rule of the ragged launchers against tiers worked
out from the numbers; and the new exports."""

import ctypes as C
import os
import re
import subprocess

import pytest
import torch
from torch.utils.data import DataLoader

import image_ragged_cases as ic
import ragged_cases as rc
import ragged_u8_cases as uc
import view_u8_cases as vu
from ips_amd import hip, synth
from ips_amd.architecture import IPSNet
from ips_amd.quant import dequant
from ips_amd.ragged import Ragged, collate_ragged, collate_ragged_padded
from ips_amd.ragged_image import RaggedImages, collate_ragged_images

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ipsx.h")
NEW = ("ipsx_trunk_encode_ragged_view_u8", "ipsx_ragged_finish_view_u8", "ipsx_ragged_view_blank_flags_u8",
       "ipsx_trunk_encode_ragged_view_dedup_u8")


def byte_slides(lengths, c=1, hw=32, seed=5):
    """One (N_b, C, h, w) uint8 tensor per length: all 256 byte values, half of the patches all-zero bytes."""
    out = []
    for k, n in enumerate(lengths):
        g = torch.Generator().manual_seed(seed + 7 * k)
        s = torch.randint(0, 256, (n, c, hw, hw), dtype=torch.uint8, generator=g)
        s[torch.rand(n, generator=g) < 0.5] = 0
        out.append(s)
    return out


# ---------------------------------------------------------------- 1. ips_ragged on uint8 slides, CPU device
@pytest.mark.parametrize("pad", [False, True])
@pytest.mark.parametrize("shuffle,style", [(False, "batch"), (True, "batch"), (True, "instance")])
def test_ips_ragged_on_bytes_equals_the_call_on_the_expansion(shuffle, style, pad):
    conf = rc.image_conf(M=16, shuffle=shuffle, shuffle_style=style)
    net = rc.make_net(conf, "cpu")
    table = vu.plain_table(1)                                  # table[c][0] = 0.5: a dequantised pad would change bits
    assert float(table[0, 0]) != 0.0
    net.set_patch_table(table)
    # ('instance' with positions: long slides have exactly conf.N rows, as ips() asks)
    lengths = ((conf.N, conf.N) if style == "instance" and shuffle else (20, 40)) + ((5, 16) if pad else ())
    slides = byte_slides(lengths)
    want = ic.patch_call(net, [dequant(s, table) for s in slides], pad=pad)
    got = ic.patch_call(net, slides, pad=pad)
    ic.assert_same_padded(got, want)
    assert got["mem_patch"].dtype == torch.float32 and got["mem_patch"].shape == (len(lengths), 16, 1, 32, 32)
    assert (got["shuffle"] is not None) == shuffle
    # ... and through net.ips(Ragged), and a loader's collate
    r = Ragged.from_list(slides, pad)
    torch.manual_seed(11)
    ic.assert_same_padded(ic.record(net, net.ips(r)), want)
    data = [{"input": s, "label": k} for k, s in enumerate(slides)]
    batch = next(iter(DataLoader(data, batch_size=len(slides), collate_fn=collate_ragged_padded if pad else collate_ragged)))
    assert batch["input"].dtype == torch.uint8
    torch.manual_seed(11)
    ic.assert_same_padded(ic.record(net, net.ips(batch["input"])), want)
    if pad:
        # the short slide: its own rows dequantised, +0.0 behind them (not table[c][0]), the padding's embedding that of ONE
        # all-zero FLOAT patch - what forward() computes from that padding
        assert ic.same_bits(got["mem_patch"][2, :5], dequant(slides[2], table))
        assert ic.same_bits(got["mem_patch"][2, 5:], torch.zeros((11, 1, 32, 32)))
        assert ic.same_bits(got["mem_patch"][3], dequant(slides[3], table))
        with torch.no_grad():
            zero = net._embed(torch.zeros((1, 1, 32, 32)))
        assert ic.same_bits(got["mem_emb"][2, 5:], zero.expand(11, -1).contiguous())
        assert got["mem_idx"][2].tolist() == list(range(5)) + [-1] * 11 and got["count"] == (16, 16, 5, 16)
    else:
        # slide by slide the solo calls on bytes
        rc.assert_same_record(got, rc.solo_loop(net, slides))


# ---------------------------------------------------------------- 2. ips_image_ragged on uint8 images, CPU device
def _image_net(c, shuffle=True):
    over = dict(N=64, M=8, I=8, shuffle=shuffle, shuffle_style="batch")
    conf = synth.mnist_conf(**over) if c == 1 else synth.traffic_conf(**over)
    return synth.fill_weights(IPSNet(torch.device("cpu"), conf), 3).eval()


@pytest.mark.parametrize("name", sorted(ic.HOST_LISTS))
def test_ips_image_ragged_on_bytes_equals_the_call_on_the_expansion(name):
    c, sizes, patch, stride = ic.HOST_LISTS[name]
    net = _image_net(c)
    table = vu.plain_table(c)
    net.set_patch_table(table)
    imgs = uc.byte_images(sizes, c=c)
    want = ic.image_call(net, [dequant(im, table) for im in imgs], patch, stride, pad=True)
    got = ic.image_call(net, imgs, patch, stride, pad=True)
    ic.assert_same_padded(got, want)
    assert got["mem_patch"].dtype == torch.float32
    ic.assert_same_padded(ic.image_call(net, imgs, patch, stride, pad=True, through_ips_image=True), want)
    data = [{"input": im, "label": k} for k, im in enumerate(imgs)]
    batch = next(iter(DataLoader(data, batch_size=len(imgs), collate_fn=lambda s: collate_ragged_images(s, pad=True))))
    assert isinstance(batch["input"], RaggedImages) and batch["input"].dtype == torch.uint8
    assert all(o % 16 == 0 for o in batch["input"].elem_offsets)               # bytes: every image at a 16-byte offset
    torch.manual_seed(11)
    ic.assert_same_padded(ic.record(net, net.ips_image(batch["input"], patch, stride)), want)


def test_long_byte_images_equal_the_solo_ips_image_loop_on_bytes():
    net = rc.make_net(rc.image_conf(M=16, shuffle=True, shuffle_style="batch"), "cpu")
    net.set_patch_table(vu.plain_table(1))
    imgs = uc.byte_images([(160, 192), (192, 224), (128, 416)])
    want = ic.solo_loop(net, imgs, (32, 32), (32, 32))
    rc.assert_same_record(ic.image_call(net, imgs, (32, 32), (32, 32)), want)


# ---------------------------------------------------------------- 3. the refusals
def _refused(net, exc, call, match=None):
    torch.manual_seed(5)
    before = torch.get_rng_state()
    net.last_mem_idx = "untouched"
    with pytest.raises(exc, match=match):
        call()
    assert torch.equal(torch.get_rng_state(), before) and net.last_mem_idx == "untouched"


def test_every_refusal_leaves_the_rng_and_the_last_selection_untouched(monkeypatch):
    net = rc.make_net(rc.image_conf(M=16, shuffle=True, shuffle_style="batch"), "cpu")
    slides = byte_slides((20, 40))
    imgs = uc.byte_images([(160, 192), (192, 224)])
    ragged = lambda: net.ips_ragged(slides)                                          # noqa: E731
    image = lambda: net.ips_image_ragged(imgs, (32, 32), (32, 32))                   # noqa: E731
    for call in (ragged, image):
        _refused(net, TypeError, call, "table")                                      # uint8 without a table
    net.patch_table = vu.plain_table(3)                 # (set_patch_table itself refuses a table the encoder's stem cannot use)
    for call in (ragged, image):
        _refused(net, ValueError, call, "3 rows")                                    # table rows != channels
    net.set_patch_table(vu.plain_table(1))
    monkeypatch.setenv("IPSX_DEDUP_BLANK", "1")
    for call in (ragged, image):
        _refused(net, TypeError, call, "IPSX_DEDUP_BLANK")
    monkeypatch.delenv("IPSX_DEDUP_BLANK")
    # a feature net handed bytes: a TypeError that names them; streams and sharded calls are as they were
    feat = rc.make_net(rc.feature_conf(M=16), "cpu")
    rows = [s.to(torch.uint8) for s in rc.make_slides(rc.feature_conf(M=16), (20, 40))]
    _refused(feat, TypeError, lambda: feat.ips_ragged(rows), "uint8")
    _refused(net, TypeError, lambda: net.ips_ragged_stream().feed([s[:3] for s in slides]), "uint8")
    _refused(net, TypeError, lambda: net.ips_stream().feed(Ragged.from_list(slides)), "Ragged")
    ragged(), image()                                                                # ... and with the table both run


def test_bytes_on_a_device_need_the_exact_trunk(monkeypatch):
    """IPSX_PRECISION=bf16 / fp32x3 refuse uint8 rows on a ROCm device - asked of ``_check`` with the device test answered
    yes, so that the refusal is held without a GPU."""
    from ips_amd import ragged
    net = rc.make_net(rc.image_conf(M=16, shuffle=True, shuffle_style="batch"), "cpu")
    net.set_patch_table(vu.plain_table(1))
    slides = Ragged.from_list(byte_slides((20, 40)))
    monkeypatch.setattr(ragged.hip, "on_device", lambda x: True)
    ragged._check(net, slides)
    for prec in ("bf16", "fp32x3"):
        monkeypatch.setenv("IPSX_PRECISION", prec)
        _refused(net, TypeError, lambda: ragged._check(net, slides), "IPSX_PRECISION=fp32")


# ---------------------------------------------------------------- 4. the byte load-width rule
def _load_width(case, kind, k=0, shifts=None, zero=True):
    """``RaggedView.load_width`` of the packed byte buffer against the tier from the numbers -> the tier."""
    c, sizes, patch, stride = case
    images, offs = uc.pack_u8(case, uc.guarded_images_u8(case, zero=zero), k, shifts)
    assert images.pixels.data_ptr() % 16 == k
    rview = images.view(patch, stride)
    got = rview.load_width(images.pixels, vu.TIERS[kind])
    assert got == uc.expected_tier(kind, k, offs, case), (kind, k, offs)
    return got


def test_load_width_on_bytes_is_the_tier_the_numbers_give():
    # the fused trunk's list (16, 4, 1)
    assert _load_width(uc.ALL16, "fused") == 16                       # all widths multiples of 16
    assert _load_width(uc.ALL16, "fused", k=4) == 4                   # ... a base 4 bytes off
    assert _load_width(uc.ALL16, "fused", k=1) == 1                   # ... an odd base
    assert _load_width(uc.ALL16, "fused", k=8) == 4                   # (8 is no entry of this list)
    assert _load_width(ic.FUSED_ALIGNED, "fused") == 4                # 116 is a multiple of 4 and not of 16
    assert _load_width(ic.FUSED_MIXED, "fused") == 1                  # 117
    assert _load_width(uc.ALL16, "fused", shifts=[0, 4, 0, 0]) == 4   # the second image at a byte offset 4 mod 16
    assert _load_width(uc.ALL16, "fused", shifts=[0, 0, 3, 0]) == 1   # an odd image offset
    # the pair kernel's (8, 4, 1)
    assert _load_width(uc.ALL16, "pair") == 8 and _load_width(uc.ALL16, "pair", k=8) == 8
    assert _load_width(uc.ALL16, "pair", shifts=[0, 8, 0, 0]) == 8 and _load_width(uc.ALL16, "pair", k=4) == 4
    assert _load_width(ic.FUSED_ALIGNED, "pair") == 4 and _load_width(ic.FUSED_MIXED, "pair") == 1
    # 1x50x50: (2, 1)
    assert _load_width(ic.POOL50_EVEN, "pool50") == 2 and _load_width(ic.POOL50_EVEN, "pool50", k=1) == 1
    assert _load_width(ic.POOL50, "pool50") == 1                      # 175, 203 and the stride 25 are odd
    # 3x100x100: (4, 1)
    assert _load_width(ic.POOL100_WIDE, "pool100") == 4 and _load_width(ic.POOL100_WIDE, "pool100", k=2) == 1
    assert _load_width(ic.POOL100, "pool100") == 1                    # 301
    assert _load_width(ic.POOL100_HALF, "pool100") == 1               # the stride 50 is no multiple of 4


def test_load_width_on_floats_is_the_float_launchers_rule():
    """float32 buffers: the kernel's ONE wide load where base, offsets, pitches and stride in BYTES allow it, else 0 (dwords)."""
    for case, k, want in ((ic.FUSED_ALIGNED, 0, 16), (ic.FUSED_ALIGNED, 1, 0), (ic.FUSED_MIXED, 0, 0)):
        images, _ = ic.guarded_ragged(case, k)
        assert images.pixels.data_ptr() % 16 == 4 * k
        assert images.view(case[2], case[3]).load_width(images.pixels, (16,)) == want
    images, _ = ic.guarded_ragged(ic.POOL50_EVEN, 0)
    assert images.view(ic.POOL50_EVEN[2], ic.POOL50_EVEN[3]).load_width(images.pixels, (8,)) == 8


# ---------------------------------------------------------------- 5. ABI
def test_new_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(ipsx_[a-z0-9_]+)\s*\(", text))
    lib = C.CDLL(hip.library_path())
    for s in NEW:
        assert s in declared and hasattr(lib, s) and s in hip._EXPORTS, s
        twin = s[:-3]                                          # the float32 entry beside it: the table follows the pixels
        assert len(hip._EXPORTS[s][1]) == len(hip._EXPORTS[twin][1]) + (0 if s == "ipsx_ragged_view_blank_flags_u8" else 1)
    assert hip.lib().ipsx_version() == 306


def test_the_library_builds_for_gfx950_only():
    make = ["make", "-C", os.path.join(ROOT, "ips_amd", "csrc"), "-n"]
    other = subprocess.run(make + ["ARCH=gfx942"], capture_output=True, text=True, timeout=60)
    assert other.returncode != 0 and "gfx950 (MI355X) only" in other.stderr
    assert subprocess.run(make, capture_output=True, text=True, timeout=60).returncode == 0
    flags = open(os.path.join(ROOT, "ips_amd", "csrc", "Makefile")).read()
    assert "ARCH     ?= gfx950" in flags and flags.count("--offload-arch=$(ARCH)") == 2


def test_a_byte_source_on_the_host_is_refused():
    """``PatchSource(images=bytes, ragged=, table=)`` reads GPU memory; a float table without bytes stays refused."""
    images, _ = uc.pack_u8(uc.ALL16, uc.guarded_images_u8(uc.ALL16))
    rview = images.view((32, 32), (32, 32))
    with pytest.raises(TypeError):
        hip.PatchSource(images=images.pixels, ragged=rview, table=vu.guard_table(1))
    with pytest.raises(TypeError):
        hip.PatchSource(images=images.pixels.float(), ragged=rview, table=vu.guard_table(1))
