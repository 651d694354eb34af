"""fused_trunk_kernel's 4x4 stage on 16-row tiles (v_mfma_f32_16x16x4_f32, csrc/fused_trunk.hip: conv_t16):
the embeddings of the eight-patch kernel stay bit for bit those of the oracle and of fused_trunk_pair_kernel, which keeps the
32-row tiles and the ipsx_pack_conv_weight stream.  Compared through int32 views at every remainder of a workgroup of eight
and at the clamped tail, on dense N(0,1) patches (sparse ones hide order errors) with an all-zero patch and a patch of -0.0
among them, random weights with negative BatchNorm scales, through every storage kind the kernel's eight instances read."""

import ctypes as C

import numpy as np
import pytest
import torch

from ips_amd import hip, quant, synth
from ips_amd.architecture import IPSNet
from oracle import oracle as orc
from view_u8_cases import plain_table

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
COUNTS = [1, 7, 8, 9, 15, 16, 17, 24]
P = 24
GRID = (1, 1, 4 * 32, 6 * 32)                  # the 24 patches as ONE image of 4 x 6 grid patches

_SHARED = {}


def pair_mode(mode):
    fn = hip.lib().ipsx_dbg_fused_trunk_pair
    fn.restype, fn.argtypes = None, [C.c_int]
    fn(mode)


@pytest.fixture
def eight_patch_kernel():
    """Every patch through the eight-patch kernel, not the pair kernel's remainder rule (the references are made first:
    the pair kernel's needs the other mode)."""
    shared()
    pair_mode(1)
    yield
    pair_mode(0)


def bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


def as_image(x):
    """(24, 1, 32, 32) patches -> the (1, 1, 128, 192) image whose grid patch p (stride 32) is patch p."""
    return x.view(4, 6, 32, 32).permute(0, 2, 1, 3).reshape(GRID).contiguous()


def shared():
    """The net (random weights, every third BatchNorm scale negative), 24 float32 patches, 24 uint8 patches with a table, and
    the reference embeddings of both - the oracle's and the pair kernel's - made once and left unchanged."""
    if not _SHARED:
        conf = synth.mnist_conf(N=64, M=8, I=8)
        cpu = synth.fill_weights(IPSNet(torch.device("cpu"), conf), 9).eval()
        sd = cpu.state_dict()
        flipped = 0
        for k, v in sd.items():
            if k.startswith("encoder.") and v.dim() == 1 and k.endswith(".weight"):          # BatchNorm scales
                v[::3] = -v[::3]
                flipped += 1
        assert flipped >= 9
        cpu.load_state_dict(sd)
        net = IPSNet(DEV, conf)
        net.load_state_dict(cpu.state_dict())
        net = net.to(DEV).eval()
        gen = torch.Generator().manual_seed(16)
        x = torch.randn((P, 1, 32, 32), generator=gen)
        x[3] = 0.0
        x[5] = -0.0
        assert bool((x[5].view(torch.int32) == -2 ** 31).all())
        q = torch.randint(0, 256, (P, 1, 32, 32), dtype=torch.uint8, generator=gen)
        table = plain_table(1)
        xq = quant.dequant(q, table)
        oracle = orc.Oracle(cpu)
        plan = hip.EncoderPlan(net.encoder, True)
        xd, qd, td = x.to(DEV), q.to(DEV), table.to(DEV)
        assert plan.fused(xd.shape)
        pair_mode(2)
        try:
            pair = {"f32": bits(plan.encode_plain(xd)), "u8": bits(plan.encode_plain(qd, table=td))}
        finally:
            pair_mode(0)
        want = {"f32": bits(torch.from_numpy(oracle.encode(x.numpy()))), "u8": bits(torch.from_numpy(oracle.encode(xq.numpy())))}
        order = torch.randperm(P, generator=gen).to(torch.int32)
        _SHARED.update(net=net, plan=plan, x=xd, q=qd, table=td, want=want, pair=pair, order=order)
    return _SHARED


def same(got, kind, rows):
    s = shared()
    got = bits(got)
    rows = np.asarray(rows)
    assert got.shape == (len(rows), 128)
    assert np.array_equal(got, s["want"][kind][rows]), "against the oracle: %d of %d words differ" % (
        np.count_nonzero(got != s["want"][kind][rows]), got.size)
    assert np.array_equal(got, s["pair"][kind][rows]), "against the pair kernel"


def test_references_agree_and_are_not_trivial():
    s = shared()
    for kind in ("f32", "u8"):
        assert np.array_equal(s["want"][kind], s["pair"][kind])
        emb = s["want"][kind].view(np.float32)
        assert np.isfinite(emb).all() and np.count_nonzero(emb) > emb.size // 4
    assert np.array_equal(s["want"]["f32"][3], s["want"]["f32"][5])       # the zero patch and the patch of -0.0


@pytest.mark.parametrize("n", COUNTS)
def test_plain_tensor(n, eight_patch_kernel):
    s = shared()
    same(s["plan"].encode_plain(s["x"][:n]), "f32", range(n))
    assert hip.encoder_kernel_name(s["plan"]) == "fused_trunk_kernel"


@pytest.mark.parametrize("n", COUNTS)
def test_index_list(n, eight_patch_kernel):
    s = shared()
    index = s["order"][:n]
    same(s["plan"].encode_indexed(s["x"], index.to(DEV)), "f32", index.long().numpy())


@pytest.mark.parametrize("n", COUNTS)
def test_uint8_with_a_table(n, eight_patch_kernel):
    s = shared()
    same(s["plan"].encode_plain(s["q"][:n], table=s["table"]), "u8", range(n))
    index = s["order"][:n]
    same(s["plan"].encode_indexed(s["q"], index.to(DEV), table=s["table"]), "u8", index.long().numpy())


@pytest.mark.parametrize("n", COUNTS)
def test_patch_view(n, eight_patch_kernel):
    s = shared()
    view = hip.PatchView(GRID, (32, 32), (32, 32))
    assert view.count == P and s["plan"].view_kernel_name(view) == "fused_trunk_view_kernel"
    same(s["plan"].encode_view(as_image(s["x"]), view, n=n), "f32", range(n))
    same(s["plan"].encode_view(as_image(s["q"]), view, first=P - n, n=n, table=s["table"]), "u8", range(P - n, P))


def test_parts_of_9_and_15():
    s = shared()
    every = s["order"].to(DEV)
    done = torch.zeros((2,), dtype=torch.int32, device=DEV)
    got = s["plan"].encode_indexed(s["x"], every, parts=([9, 24], done))
    torch.cuda.synchronize()
    assert done.tolist() == [9, 15]
    same(got, "f32", s["order"].long().numpy())
    done.zero_()
    got = s["plan"].encode_indexed(s["q"], every, table=s["table"], parts=([9, 24], done))
    torch.cuda.synchronize()
    assert done.tolist() == [9, 15]
    same(got, "u8", s["order"].long().numpy())
    view = hip.PatchView(GRID, (32, 32), (32, 32))
    done.zero_()
    got = s["plan"].encode_view(as_image(s["x"]), view, index=every, parts=([9, 24], done))
    torch.cuda.synchronize()
    assert done.tolist() == [9, 15]
    same(got, "f32", s["order"].long().numpy())
    done.zero_()
    got = s["plan"].encode_view(as_image(s["q"]), view, index=every, table=s["table"], parts=([9, 24], done))
    torch.cuda.synchronize()
    assert done.tolist() == [9, 15]
    same(got, "u8", s["order"].long().numpy())


def test_repacking_after_an_in_place_weight_update(eight_patch_kernel):
    """The plan's signature sees the update and packs BOTH streams again: the 16-row tiles' (the eight-patch kernel) and
    ipsx_pack_conv_weight's (the pair kernel) agree on the new weights, and the output moved."""
    conf = synth.mnist_conf(N=64, M=8, I=8)
    net = synth.fill_weights(IPSNet(DEV, conf), 4).to(DEV).eval()
    plan = hip.EncoderPlan(net.encoder, True)
    x = shared()["x"]
    before = bits(plan.encode_plain(x))
    for blk, name in ((0, "conv2"), (1, "conv1"), (1, "conv2")):
        with torch.no_grad():
            w = getattr(net.encoder[5][blk], name).weight
            w[:, 1::2] *= -1.25
        after = bits(plan.encode_plain(x))
        assert not np.array_equal(after, before), (blk, name)
        pair_mode(2)
        pair = bits(plan.encode_plain(x))
        pair_mode(1)
        assert np.array_equal(after, pair), (blk, name)
        assert np.array_equal(after, bits(hip.EncoderPlan(net.encoder, True).encode_plain(x))), (blk, name)
        before = after
