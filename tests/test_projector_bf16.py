"""The feature projector on the bf16 matrix pipe (IPSX_PRECISION=bf16, csrc/projector_bf16.hip) and feature
rows stored as float16 / bfloat16.

There is no reference behaviour at this precision.  The oracle is a float64 emulation that rounds exactly where the
kernel rounds: the fp32 row moments, x - mean in fp32 then rounded to bf16, W rounded to bf16, the products summed in
float64, then |rstd|, the BatchNorm affine and the ReLU.  The kernel differs from it by its fp32 accumulation only.
Measured worst cases (relative to the output's scale) are printed; the bounds below are those plus margin."""

import re

import pytest
import torch
from torch import nn

from ips_amd import hip, synth
from ips_amd.architecture import IPSNet
from ips_amd.hip_encoder import EncoderPlan, _bn_affine, encoder_kernel_name

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

EMU_BOUND = 2e-6        # measured worst 7.5e-7 (F = 2048); against the float64 emulation of the kernel's roundings
FP32_BOUND = 1e-2       # measured worst 4.4e-3; against the fp32 projector
LN64_BOUND = 1e-2       # measured worst 3.4e-3; rows whose mean dwarfs their spread, against float64 LayerNorm etc.
ROW_COUNTS = (1, 31, 65, 1000, 4099)


def projector(F, D, seed):
    """IPSNet.get_projector with non-trivial parameters."""
    g = torch.Generator().manual_seed(seed)
    enc = nn.Sequential(nn.LayerNorm(F, eps=1e-05, elementwise_affine=False), nn.Linear(F, D), nn.BatchNorm1d(D), nn.ReLU())
    with torch.no_grad():
        enc[1].weight.copy_(torch.randn(D, F, generator=g) * (2.0 / F) ** 0.5)
        enc[1].bias.copy_(0.1 * torch.randn(D, generator=g))
        enc[2].weight.copy_(0.5 + torch.rand(D, generator=g))
        enc[2].bias.copy_(0.1 * torch.randn(D, generator=g))
        enc[2].running_mean.copy_(0.1 * torch.randn(D, generator=g))
        enc[2].running_var.copy_(0.5 + torch.rand(D, generator=g))
    return enc.to(DEV).eval()


def rows(n, F, seed):
    """ReLU-Gaussian rows (post-ReLU CNN features); every 7th row instead 10 + 0.5 N(0, 1): mean^2 / var = 400."""
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn(n, F, generator=g))
    big = torch.arange(n) % 7 == 3
    x[big] = 10.0 + 0.5 * torch.randn(int(big.sum()), F, generator=g)
    return x.to(DEV), big.to(DEV)


def emulate(enc, x, stats):
    a = (x.float() - stats[:, :1]).to(torch.bfloat16).double()
    w = enc[1].weight.detach().float().to(torch.bfloat16).double()
    aff = _bn_affine(enc[2], bias=enc[1].bias).double()
    t = stats[:, 1:].abs().double() * (a @ w.T)
    return torch.relu(t * aff[0] + aff[1])


def layernorm64(enc, x):
    xd = x.double()
    y = (xd - xd.mean(1, keepdim=True)) / torch.sqrt(xd.var(1, unbiased=False, keepdim=True) + enc[0].eps)
    y = y @ enc[1].weight.detach().double().T + enc[1].bias.detach().double()
    bn = enc[2]
    y = (y - bn.running_mean.double()) / torch.sqrt(bn.running_var.double() + bn.eps) * bn.weight.detach().double() \
        + bn.bias.detach().double()
    return torch.relu(y)


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("F,D", [(2048, 512), (96, 128), (64, 96), (96, 64)])
def test_bf16_projector_against_float64_emulation(F, D, monkeypatch):
    """Every row count (one, a partial 32-row half, a partial 64-row tile, thousands) and every output-tile split (4, 2 and
    1 tiles of 32 columns per wavefront): within EMU_BOUND of the emulation, within FP32_BOUND of the fp32 projector, and
    the rows whose mean dwarfs their spread within LN64_BOUND of a float64 LayerNorm (a folded, uncentred bf16 design
    cancels there)."""
    enc = projector(F, D, seed=F + D)
    worst = [0.0, 0.0, 0.0]
    for n in ROW_COUNTS:
        x, big = rows(n, F, seed=n)
        monkeypatch.setenv("IPSX_PRECISION", "fp32")
        want32 = EncoderPlan(enc, False).encode(x)
        monkeypatch.setenv("IPSX_PRECISION", "bf16")
        plan = EncoderPlan(enc, False)
        stats = plan.row_stats(x)
        got = plan.encode(x, stats=stats)
        assert encoder_kernel_name(plan).startswith("row_moments_typed_kernel + projector_bf16_kernel")
        assert torch.isfinite(got).all()
        e = (rel(got, emulate(enc, x, stats)), rel(got, want32),
             rel(got[big], layernorm64(enc, x[big])) if bool(big.any()) else 0.0)
        worst = [max(w, v) for w, v in zip(worst, e)]
    print("F={} D={}: emulation {:.3g}, fp32 projector {:.3g}, float64 LayerNorm on large-mean rows {:.3g}".format(F, D, *worst))
    assert worst[0] <= EMU_BOUND and worst[1] <= FP32_BOUND and worst[2] <= LN64_BOUND, worst


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_storage_is_bit_identical_to_float32(dtype, monkeypatch):
    """Moments and outputs of half-stored rows are those of the same values passed as float32; the plain, stats-given and
    publish forms agree bitwise; rows k0:k1 of a call on x are a call on x[k0:k1]."""
    monkeypatch.setenv("IPSX_PRECISION", "bf16")
    enc = projector(2048, 512, seed=3)
    plan = EncoderPlan(enc, False)
    x, _ = rows(3000, 2048, seed=9)
    xs = x.to(dtype)
    xw = xs.float()
    stats = plan.row_stats(xs)
    assert torch.equal(stats, plan.row_stats(xw))
    plain = plan.encode(xs).clone()
    assert torch.equal(plain, plan.encode(xw))
    assert torch.equal(plain, plan.encode(xs, stats=stats))
    ready = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert torch.equal(plain, plan.encode(xs, stats=stats, publish=(ready, 77)))
    assert int(ready.item()) == 77
    for k0, k1 in ((0, 1), (5, 38), (64, 129), (1000, 3000), (2999, 3000)):
        assert torch.equal(plain[k0:k1], plan.encode(xs[k0:k1])), (k0, k1)


@pytest.mark.parametrize("B,N,M", [(1, 8192, 256), (3, 4096, 256), (16, 4096, 256), (1, 20000, 5000)])
def test_every_schedule_selects_the_same_patches_under_bf16(B, N, M, monkeypatch):
    """The feature pipeline's schedules (the default - persistent loops, the projector launch by launch -, per-part
    launches, the loop after the projector, lazy loading from pinned host memory) run half-stored slides under bf16 and
    select the same indices as each other and as float32 storage of the same values; mem_patch keeps the storage dtype
    and holds the gathered rows.  M = I = 5000: a candidate set beyond the LDS."""
    monkeypatch.setenv("IPSX_PRECISION", "bf16")
    conf = synth.camelyon_conf(N=N, M=M, I=M)
    net = synth.fill_weights(IPSNet(torch.device(DEV), conf), 7).to(DEV).eval()
    x16 = synth.make_patches(conf, B, seed=3).half()
    xd = x16.to(DEV)
    res = {}
    for name, env, x in (("default", {}, xd), ("per-part launches", {"IPSX_SCAN_PERSIST": "0"}, xd),
                         ("after", {"IPSX_OVERLAP_SCAN": "0"}, xd), ("lazy", {}, x16.pin_memory()),
                         ("float32 storage", {}, xd.float())):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        net.ips(x)
        mem_patch, _ = net.ips(x)                   # (a second call: cached buffers, the status mirror of the first)
        idx = net.last_mem_idx.clone()
        res[name] = idx
        assert mem_patch.dtype == x.dtype and mem_patch.device == torch.device(DEV)
        assert torch.equal(mem_patch, torch.gather(x.to(DEV), 1, idx.unsqueeze(-1).expand(-1, -1, x.shape[2]))), name
        for k in env:
            monkeypatch.delenv(k)
    for name, idx in res.items():
        assert torch.equal(idx, res["after"]), name


def test_end_to_end_against_the_fp32_path(monkeypatch):
    """A camelyon_conf shape: the bf16 selection of f16-stored slides shares most patches with the fp32 selection of the
    float32 slides; eval forward is finite, close to the fp32 forward on the same patches, and the same bits with the
    embeddings ips() kept; the training-mode forward on half input is the forward on its float32 widening."""
    conf = synth.camelyon_conf(N=8192, M=256, I=256, dropout=0.0, attn_dropout=0.0)
    net = synth.fill_weights(IPSNet(torch.device(DEV), conf), 7).to(DEV).eval()
    x32 = synth.make_patches(conf, 2, seed=5).to(DEV)
    x16 = x32.half()
    monkeypatch.setenv("IPSX_PRECISION", "fp32")
    net.ips(x32)
    idx32 = net.last_mem_idx.clone()
    monkeypatch.setenv("IPSX_PRECISION", "bf16")
    mem_patch, _ = net.ips(x16)
    idx16 = net.last_mem_idx.clone()
    shares = [len(set(idx16[b].tolist()) & set(idx32[b].tolist())) / conf.M for b in range(2)]
    print("patches in common with the fp32 selection:", shares)
    assert min(shares) >= 0.95, shares                # measured 0.988 / 0.996
    assert mem_patch.dtype == torch.float16
    assert torch.equal(mem_patch, torch.gather(x16, 1, idx16.unsqueeze(-1).expand(-1, -1, x16.shape[2])))
    with torch.no_grad():
        kept = net.last_mem_emb
        p16 = net(mem_patch)["metastases"]
        p_kept = net(mem_patch, mem_emb=kept)["metastases"]
        monkeypatch.setenv("IPSX_PRECISION", "fp32")
        p32 = net(mem_patch.float())["metastases"]
    print("eval predictions, bf16 - fp32: {:.3g}".format(float((p16 - p32).abs().max())))
    assert torch.isfinite(p16).all()
    assert torch.equal(p16, p_kept)
    assert float((p16 - p32).abs().max()) <= 2e-3     # measured 2.9e-4
    monkeypatch.setenv("IPSX_PRECISION", "bf16")
    net.train()
    torch.manual_seed(0)
    t16 = net(mem_patch)["metastases"]
    t32 = net(mem_patch.float())["metastases"]
    assert torch.equal(t16, t32)


@pytest.mark.parametrize("prec", ["fp32", "fp32x3"])
def test_half_features_are_refused_outside_bf16(prec, monkeypatch):
    monkeypatch.setenv("IPSX_PRECISION", prec)
    conf = synth.camelyon_conf(N=1024, M=64, I=64)
    net = synth.fill_weights(IPSNet(torch.device(DEV), conf), 7).to(DEV).eval()
    x16 = synth.make_patches(conf, 1, seed=1).half().to(DEV)
    with pytest.raises(TypeError, match="IPSX_PRECISION=bf16"):
        net.ips(x16)
    plan = EncoderPlan(net.encoder, False)
    for call in (plan.encode, plan.row_stats):
        with pytest.raises(TypeError, match="IPSX_PRECISION=bf16"):
            call(x16[0])


def test_shapes_outside_the_bf16_projector_raise(monkeypatch):
    """F % 16 and D % 32 are checked before the first launch - in the binding and in the library - naming the limit."""
    monkeypatch.setenv("IPSX_PRECISION", "bf16")
    for F, D, limit in ((72, 128, "F % 16 == 0"), (64, 48, "D % 32 == 0")):
        plan = EncoderPlan(projector(F, D, seed=1), False)
        x, _ = rows(100, F, seed=2)
        for call in (plan.encode, plan.row_stats):
            with pytest.raises(ValueError, match=re.escape(limit)):
                call(x)
        stats = torch.zeros((100, 2), dtype=torch.float32, device=DEV)
        out = torch.empty((100, D), dtype=torch.float32, device=DEV)
        lib = hip.lib()
        assert lib.ipsx_projector_bf16_supported(hip.C.byref(plan.lin)) == 0
        with pytest.raises(RuntimeError, match=re.escape(limit)):
            hip._ck(lib.ipsx_projector_apply_bf16(hip.C.byref(plan.lin), hip._p(x), 0, 100, hip._p(stats), hip._p(out), None, 0,
                                                  hip._stream()), "ipsx_projector_apply_bf16")


def test_projector_stream_refuses_the_bf16_projector_and_half_rows(monkeypatch):
    """``EncoderPlan.stream`` is the fp32 projector's persistent kernel (it reads 4 bytes per feature): under bf16 it is
    not offered (``stream_supported``) and refuses float32 and half rows alike; under fp32 it refuses half rows - all
    with TypeError before any launch (the output buffers are never touched)."""
    enc = projector(2048, 512, seed=5)
    x, _ = rows(256, 2048, seed=4)
    for prec, inputs in (("bf16", (x, x.half(), x.bfloat16())), ("fp32", (x.half(), x.bfloat16()))):
        monkeypatch.setenv("IPSX_PRECISION", prec)
        plan = EncoderPlan(enc, False)
        if prec == "bf16":
            assert not plan.stream_supported(256, 8)
        for xi in inputs:
            with pytest.raises(TypeError, match="IPSX_PRECISION=bf16"):
                plan.stream(xi, None, 8, None, None, None, None)
    monkeypatch.setenv("IPSX_PRECISION", "fp32")
    assert EncoderPlan(enc, False).stream_supported(256, 8)
