"""IPSX_PRECISION=bf16 on the layer-by-layer trunks (csrc/conv_nhwc_bf16.hip, csrc/trunk.hip; DESIGN 4, "bf16 layered
trunk"): 50-px Megapixel-MNIST patches, the traffic-sign model, ResNet-50 bottlenecks.

There is no reference behaviour at this precision.  The oracle is a float64 emulation that rounds exactly where the
kernels round: stem, BatchNorm, ReLU and max-pool in float32, the pooled map rounded once to bf16, every weight behind
the stem rounded to bf16, every block convolution summed in float64, then (float64) affine, + the bf16 identity, ReLU,
and one rounding to bf16; the average pool sums the bf16 map.  The kernels differ from it by their fp32 accumulation
and fp32 epilogue only.

Bounds.  One convolution (a): with e the emulation BEFORE its last rounding and s = max |e|, every element within
2^-8 |e| + 1e-5 s, and at most 1e-3 of the elements different from bf16(e) - fp32 accumulation moves a result across
a rounding boundary only when float64 puts it within ~1e-6 relative of one (ATen's fp32 convolution in the kernel's
place differs on 7e-6 .. 4.5e-5 of the elements).  Whole trunk (c): max |got - emu| / max |emu| < 3e-3 and row-wise
||got - fp32|| / ||fp32|| < 3e-2, the bounds tests/test_hip_kernels.py::test_bf16_trunk_tracks_fp32_within_tolerance holds
the fused bf16 trunk to (a bf16 rounding flip of one activation is 4e-3 of that activation).  Every test prints what it
measured.  Measured on one MI355X: (a) 0 .. 7.7e-5 of the elements differ from bf16(e); (c) native50 7.2e-4 / 2.9e-3,
traffic_full 1.7e-3 / 3.1e-3, ResNet-50 1.6e-3 / 3.3e-3 (the emulation with fp32 accumulation lies 1.2e-5 / 1.6e-3 /
1.4e-3 from the float64 one); (d) 100 % / 100 % / 87.5 % of the fp32 selection's patches, predictions within 8.2e-3."""

import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from ips_amd import hip, synth
from ips_amd.architecture import IPSNet
from tests.util import Golden, bf16_conv_emulation, r16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = hip.C

EMU_BOUND = 3e-3
FP32_BOUND = 3e-2
FLIP_CAP = 1e-3


def bf16_env(monkeypatch):
    monkeypatch.setenv("IPSX_PRECISION", "bf16")


# ---------------------------------------------------------------------------------------------- (a) one convolution
CONV_SHAPES = [
    # c_in, c_out, k, stride, pad, h, w, n, residual, relu
    (64, 64, 3, 1, 1, 13, 13, 3, True, True),        # 50-px patches, layer1
    (64, 64, 3, 1, 1, 13, 13, 70, False, True),      # ... many patches, ragged M tiles
    (64, 128, 3, 2, 1, 13, 13, 3, False, True),      # strided, odd map
    (64, 128, 1, 2, 0, 25, 25, 1, False, False),     # 1x1 strided projection (traffic layer2 shortcut)
    (256, 512, 3, 2, 1, 7, 7, 3, False, True),
    (512, 512, 3, 1, 1, 4, 4, 70, True, True),       # small map: M runs over the patches
    (512, 512, 3, 1, 1, 4, 4, 1, True, True),        # 16 pixels in all
    (256, 64, 1, 1, 0, 12, 12, 3, False, True),      # bottleneck reduce
    (64, 256, 1, 1, 0, 12, 12, 3, True, True),       # bottleneck expand, shortcut
    (64, 96, 3, 1, 1, 9, 11, 3, True, False),        # C_out not a multiple of 64, not square, residual without ReLU
    (16, 32, 3, 1, 1, 5, 7, 1, False, True),         # smallest: one k-step per tap, one n-tile
]


@pytest.mark.parametrize("c_in,c_out,k,stride,pad,h,w,n,res,relu", CONV_SHAPES)
def test_one_convolution_against_the_emulation(c_in, c_out, k, stride, pad, h, w, n, res, relu):
    g = torch.Generator().manual_seed(1000 * c_in + c_out + 7 * k + n)
    x = torch.relu(torch.randn(n, h, w, c_in, generator=g)).to(torch.bfloat16)
    wt = torch.randn(c_out, c_in, k, k, generator=g) * (2.0 / (c_in * k * k)) ** 0.5
    alpha, shift = 1 + 0.2 * torch.randn(c_out, generator=g), 0.1 * torch.randn(c_out, generator=g)
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    r = torch.relu(torch.randn(n, ho, wo, c_out, generator=g)).to(torch.bfloat16) if res else None
    got = hip.conv2d_nhwc_bf16(x.to(DEV), wt.to(DEV), alpha.to(DEV), shift.to(DEV), stride, pad,
                               r.to(DEV) if res else None, relu)
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == (n, ho, wo, c_out)
    got = got.cpu().double()
    e = bf16_conv_emulation(x, wt, alpha, shift, stride, pad, r, relu)
    s = float(e.abs().max())
    assert torch.isfinite(got).all()
    excess = float(((got - e).abs() - (2.0 ** -8 * e.abs() + 1e-5 * s)).max())
    flips = float((got != r16(e)).double().mean())
    print("\n  conv %d -> %d %dx%d/%d on %dx%d n=%d: share of elements != bf16(emulation) %.2e, worst |got - e| - bound %.3e"
          % (c_in, c_out, k, k, stride, h, w, n, flips, excess))
    assert excess <= 0.0, excess
    assert flips <= FLIP_CAP, flips


def test_average_pool_of_a_bf16_map():
    g = torch.Generator().manual_seed(3)
    x = torch.relu(torch.randn(5, 4, 4, 96, generator=g)).to(torch.bfloat16)
    got = hip.avgpool_nhwc_bf16(x.to(DEV)).cpu()
    s = torch.zeros(5, 96)
    for j in range(16):                                  # the fp32 sum in memory order, then one division
        s = s + x.reshape(5, 16, 96)[:, j].float()
    assert torch.equal(got, s / 16.0)


# ---------------------------------------------------------------------------------------------- the emulation
def emulate_trunk(net, x, acc=torch.float64):
    """The contract of DESIGN 4 on the CPU.  acc = float64: the oracle; float32: the same with ATen's fp32 convolutions
    (a reference-only figure: how far two correct accumulations lie apart)."""
    mods = list(net.encoder.children())
    xc = x.detach().float().cpu()

    def aff(bn):      # the fp32 (alpha, shift) the kernels apply
        a = hip._bn_affine(bn).cpu().double()
        return a[0][None, :, None, None], a[1][None, :, None, None]

    def cpu(t):
        return t.detach().float().cpu()

    with torch.no_grad():                               # stem, BN, ReLU, max-pool: float32, as torch computes them
        bn = mods[1]
        y = F.conv2d(xc, cpu(mods[0].weight), None, mods[0].stride, mods[0].padding)
        y = F.batch_norm(y, cpu(bn.running_mean), cpu(bn.running_var), cpu(bn.weight), cpu(bn.bias), False, 0.0, bn.eps)
        y = F.max_pool2d(F.relu(y), 3, 2, 1)
    y = r16(y)

    def cba(t, cv, bn, relu, idt=None):
        al, sh = aff(bn)
        z = F.conv2d(t.to(acc), r16(cpu(cv.weight)).to(acc), None, cv.stride, cv.padding).double() * al + sh
        if idt is not None:
            z = z + idt
        return r16(F.relu(z) if relu else z)

    for stage in mods[4:-1]:
        for blk in stage.children():
            pairs = [(getattr(blk, "conv%d" % i), getattr(blk, "bn%d" % i)) for i in (1, 2, 3) if hasattr(blk, "conv%d" % i)]
            idt = y if blk.downsample is None else cba(y, blk.downsample[0], blk.downsample[1], False)
            z = y
            for cv, bn in pairs[:-1]:
                z = cba(z, cv, bn, True)
            y = cba(z, pairs[-1][0], pairs[-1][1], True, idt)
    n, c = y.shape[:2]
    flat = y.permute(0, 2, 3, 1).reshape(n, -1, c)
    s = torch.zeros(n, c)
    for j in range(flat.shape[1]):                      # the fp32 sum in memory order, then one division
        s = s + flat[:, j].float()
    return (s / float(flat.shape[1])).double()


def resnet50_case():
    conf = synth.traffic_conf(N=12, M=4, I=4, patch=48, enc_type='resnet50', n_res_blocks=2, D=512)
    net = synth.fill_weights(IPSNet(torch.device(DEV), conf), 3).to(DEV).eval()
    return net, synth.make_patches(conf, 1, seed=4)[0]


def trunk_case(name):
    if name == "resnet50":
        return resnet50_case()
    g = Golden(name)
    return g.net(DEV), g.patches()[0]


# ---------------------------------------------------------------------------------------------- (c) whole trunk
@pytest.mark.parametrize("name,n", [("mnist_native50", 24), ("traffic_full", 6), ("resnet50", 12)])
def test_whole_trunk_against_the_emulation_and_the_fp32_kernels(name, n, monkeypatch):
    net, x = trunk_case(name)
    x = x[:n].to(DEV)
    plan = hip.EncoderPlan(net.encoder, True)
    ref = plan.encode(x).double()
    assert "bf16" not in hip.encoder_kernel_name(plan)
    bf16_env(monkeypatch)
    got = plan.encode(x)
    kernel = hip.encoder_kernel_name(plan)
    monkeypatch.delenv("IPSX_PRECISION")
    assert "conv_nhwc_bf16_kernel (layer by layer, bf16)" in kernel, kernel
    assert got.dtype == torch.float32 and torch.isfinite(got).all()
    emu = emulate_trunk(net, x)
    emu32 = emulate_trunk(net, x, torch.float32)
    err = float((got.double().cpu() - emu).abs().max() / emu.abs().max())
    gap = float((emu32 - emu).abs().max() / emu.abs().max())
    rel = float(((got.double() - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(1e-12)).max())
    print("\n  %s (%s): |got - emu| / max|emu| = %.3e (fp32-accumulating emulation vs float64 emulation: %.3e), "
          "row-wise ||got - fp32|| / ||fp32|| = %.3e" % (name, kernel, err, gap, rel))
    assert err < EMU_BOUND, err
    assert rel < FP32_BOUND, rel


# ---------------------------------------------------------------------------------------------- (b) determinism, independence
@pytest.mark.parametrize("name", ["mnist_native50", "traffic_full"])
def test_embeddings_do_not_depend_on_batch_chunk_or_stream(name, monkeypatch):
    net, x = trunk_case(name)
    n_all = 1100 if name == "mnist_native50" else 64
    reps = -(-n_all // x.shape[0])
    x = torch.cat([x] * reps)[:n_all].to(DEV)
    if reps > 1:                                        # not the same patches over and over
        x = x * torch.linspace(0.5, 1.5, n_all, device=DEV).view(-1, 1, 1, 1)
    plan = hip.EncoderPlan(net.encoder, True)
    bf16_env(monkeypatch)
    full = plan.encode(x)
    assert "bf16" in hip.encoder_kernel_name(plan)
    assert torch.isfinite(full).all()
    assert torch.equal(full, plan.encode(x)), "two calls differ"
    for k0, k1 in ((0, 1), (1, 4), (5, 42), (n_all - 37, n_all)):
        assert torch.equal(full[k0:k1], plan.encode(x[k0:k1].contiguous())), (k0, k1)
    monkeypatch.setenv("IPSX_LAYERED_STREAMS", "1")
    assert torch.equal(full, plan.encode(x)), "one stream differs from two halves on two streams"
    monkeypatch.delenv("IPSX_LAYERED_STREAMS")
    # a workspace that holds a handful of patches: many chunks, a ragged last one
    one = hip.lib().ipsx_trunk_workspace_bytes(C.byref(plan.trunk), 1)
    monkeypatch.setenv("IPSX_TRUNK_WORKSPACE_MB", str(max(1, (7 * one) >> 20)))
    assert hip.lib().ipsx_trunk_workspace_bytes(C.byref(plan.trunk), n_all) < n_all * one
    assert torch.equal(full[:50], plan.encode(x[:50].contiguous())), "chunked call differs"
    monkeypatch.delenv("IPSX_TRUNK_WORKSPACE_MB")


def test_blank_patch_dedup_is_exact_under_bf16(monkeypatch):
    g = Golden("mnist_native50")
    net = g.net(DEV)
    x = synth.make_patches(g.conf, 1, seed=5, blank_frac=0.85, N=333)[0].to(DEV)
    plan = hip.EncoderPlan(net.encoder, True)
    bf16_env(monkeypatch)
    full = plan.encode(x)
    assert "bf16" in hip.encoder_kernel_name(plan)
    monkeypatch.setenv("IPSX_DEDUP_BLANK", "1")
    dd = plan.encode(x)
    monkeypatch.delenv("IPSX_DEDUP_BLANK")
    nonblank = int((x.reshape(x.shape[0], -1) != 0).any(1).sum().item())
    assert int(plan.n_encoded.item()) == nonblank + 1 and nonblank < 100
    assert torch.equal(full, dd)


def test_trunk_equals_the_kernels_applied_to_the_rounded_fp32_pooled_map(monkeypatch):
    """Where a probe reaches the pooled map: the fp32 library kernels' stem + max-pool output, rounded to bf16 here, then
    every block by hand through hip.conv2d_nhwc_bf16 and hip.avgpool_nhwc_bf16 - ipsx_trunk_encode under bf16 must give
    the same bits (its stem is the fp32 path's, its pooled map is rounded once, the shortcut is the stored bf16 map)."""
    g = Golden("mnist_native50")
    net = g.net(DEV)
    x = g.patches()[0, :9].to(DEV)
    plan = hip.EncoderPlan(net.encoder, True)
    mods = list(net.encoder.children())
    plan._refresh()
    n = x.shape[0]
    s_out = torch.empty((n, 25, 25, 64), device=DEV)
    hip._ck(hip.lib().ipsx_conv2d_affine_to_nhwc(C.byref(plan.trunk.stem), hip._p(x), None, hip._p(s_out), n, 50, 50, 1,
                                                 hip._stream()), "stem")
    pooled = torch.empty((n, 13, 13, 64), device=DEV)
    hip._ck(hip.lib().ipsx_maxpool_3x3s2_nhwc(hip._p(s_out), hip._p(pooled), n, 64, 25, 25, hip._stream()), "pool")
    y = pooled.to(torch.bfloat16)

    def cba(t, cv, bn, relu, idt=None):
        a = hip._bn_affine(bn)
        return hip.conv2d_nhwc_bf16(t, cv.weight, a[0], a[1], cv.stride[0], cv.padding[0], idt, relu)

    for stage in mods[4:-1]:
        for blk in stage.children():
            idt = y if blk.downsample is None else cba(y, blk.downsample[0], blk.downsample[1], False)
            y = cba(cba(y, blk.conv1, blk.bn1, True), blk.conv2, blk.bn2, True, idt)
    want = hip.avgpool_nhwc_bf16(y)
    bf16_env(monkeypatch)
    got = plan.encode(x)
    assert "bf16" in hip.encoder_kernel_name(plan)
    assert torch.equal(got, want)


# ---------------------------------------------------------------------------------------------- (d) end to end
@pytest.mark.parametrize("name", ["mnist_native50", "traffic_tiny", "traffic_full"])
def test_ips_and_forward_under_bf16(name, monkeypatch):
    g = Golden(name)
    net = g.net(DEV)
    x = g.patches().to(DEV)
    mp32, pos32 = net.ips(x)
    idx32 = net.last_mem_idx.clone()
    with torch.no_grad():
        p32 = net(mp32, pos32)
    bf16_env(monkeypatch)
    mp16, pos16 = net.ips(x)
    idx16 = net.last_mem_idx.clone()
    with torch.no_grad():
        p16 = net(mp16, pos16)
    monkeypatch.setenv("IPSX_OVERLAP_SCAN", "0")            # the other schedule selection.py can choose
    net.ips(x)
    idx16_plain = net.last_mem_idx.clone()
    monkeypatch.delenv("IPSX_OVERLAP_SCAN")
    monkeypatch.delenv("IPSX_PRECISION")
    assert torch.equal(idx16, idx16_plain), "the schedules select different patches"
    shares = [len(set(idx32[b].tolist()) & set(idx16[b].tolist())) / float(g.conf.M) for b in range(idx32.shape[0])]
    worst = max(float((p16[k] - p32[k]).abs().max()) for k in p32)
    print("\n  %s: share of the fp32 selection's patches per image %s, predictions within %.3e of fp32"
          % (name, ["%.3f" % s for s in shares], worst))
    assert min(shares) >= 0.85, shares
    for k in p32:
        assert torch.isfinite(p16[k]).all() and float((p16[k] - p32[k]).abs().max()) < 0.1


def test_sharded_path_equals_the_single_gpu_call_under_bf16():
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", "29571", os.path.join(repo, "tools", "dist_check.py"),
           "--backend", "gloo", "--share-gpu", "--precision", "bf16", "--cases", "mnist_native50,traffic_tiny"]
    out = subprocess.run(cmd, cwd=repo, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert out.stdout.count(" ok") == 4 and "MISMATCH" not in out.stdout, out.stdout[-2000:]
    assert "bf16 f32" in out.stdout


# ---------------------------------------------------------------------------------------------- (e) refusals
def test_refusals(monkeypatch):
    g = Golden("mnist_native50")
    net = g.net(DEV)
    x = g.patches()[0, :4].to(DEV)
    monkeypatch.setenv("IPSX_PRECISION", "fp32x3")
    with pytest.raises(RuntimeError) as e:
        hip.EncoderPlan(net.encoder, True).encode(x)
    assert "fp32x3 exists for the fused 1x32x32 trunk only" in str(e.value) and "bf16" not in str(e.value)
    monkeypatch.setenv("IPSX_PRECISION", "bf16")
    plan = hip.EncoderPlan(net.encoder, True)
    assert torch.isfinite(plan.encode(x)).all()
    with pytest.raises((TypeError, RuntimeError)) as e:
        plan.encode(x.to(torch.float16))
    assert "stem" in str(e.value)
    assert torch.isfinite(plan.encode(x)).all()             # (the refused call left the plan usable)
    monkeypatch.delenv("IPSX_PRECISION")
    lib = hip.lib()
    assert lib.ipsx_conv2d_affine_nhwc_bf16_supported(C.byref(hip.Conv(24, 64, 3, 3, 1, 1))) == 0
    assert lib.ipsx_conv2d_affine_nhwc_bf16_supported(C.byref(hip.Conv(64, 60, 3, 3, 1, 1))) == 0
    assert lib.ipsx_conv2d_affine_nhwc_bf16_supported(C.byref(hip.Conv(16, 96, 3, 3, 2, 1))) == 1
    with pytest.raises(ValueError):
        hip.conv2d_nhwc_bf16(torch.zeros(1, 5, 5, 24, dtype=torch.bfloat16, device=DEV), torch.zeros(64, 24, 3, 3, device=DEV),
                             None, None, 1, 1)
