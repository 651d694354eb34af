"""The with-grad cross-attention aggregator on folded queries (training/fused_aggregator.py): what can be checked without a
GPU - the algebra of the fold on both sides of the pool and the row order r = h * T + t, in float64 against the stock
modules; which Transformers ``supported`` takes; the switch."""

import copy

import pytest
import torch
from torch import nn

from ips_amd import synth
from ips_amd.architecture import IPSNet
from ips_amd.architecture.transformer import MultiHeadCrossAttention, Transformer
from ips_amd.training import fused_aggregator

SHAPES = [((1, 8, 512, 64, 64, 2048), 2, 300), ((4, 8, 128, 16, 16, 512), 3, 100)]


def _transf(args, seed):
    torch.manual_seed(seed)
    t = Transformer(*args, attn_dropout=0.0, dropout=0.0).double()
    with torch.no_grad():
        t.crs_attn.q.mul_(8.0)          # (attention that is not flat)
    return t


@pytest.mark.parametrize("args,B,M", SHAPES)
def test_fold_equals_the_stock_modules_in_float64(args, B, M):
    """fused_aggregator.forward with the ATen pool equals transf.mlp(transf.crs_attn(x)) to 1e-12 relative: output, x.grad
    and every parameter's gradient."""
    a = _transf(args, 3)
    s = copy.deepcopy(a)
    g = torch.Generator().manual_seed(5)
    x = torch.randn((B, M, args[2]), generator=g, dtype=torch.float64)
    w = torch.randn((B, args[0], args[2]), generator=g, dtype=torch.float64)
    xa, xs = x.clone().requires_grad_(), x.clone().requires_grad_()
    ya = fused_aggregator.forward(a, xa, pool=fused_aggregator.aten_pool)
    ys = s.mlp(s.crs_attn(xs))
    (ya * w).sum().backward()
    (ys * w).sum().backward()

    def rel(u, v):
        return float((u - v).abs().max() / v.abs().max())
    assert ya.shape == ys.shape and rel(ya.detach(), ys.detach()) < 1e-12
    assert rel(xa.grad, xs.grad) < 1e-12
    for (n, p), (_, q) in zip(a.named_parameters(), s.named_parameters()):
        assert p.grad is not None and rel(p.grad, q.grad) < 1e-12, n


def test_keep_scales_the_attention_weights():
    """keep = the mask stock attention dropout would draw: the same value as masking the attention map by hand."""
    args = (4, 8, 128, 16, 16, 512)
    t = _transf(args, 4)
    x = torch.randn((2, 50, 128), dtype=torch.float64)
    keep = (torch.rand((2, 32, 50)) > 0.1).double() / 0.9
    with torch.no_grad():
        got = fused_aggregator.forward(t, x, keep=keep, pool=fused_aggregator.aten_pool)
        want = _by_hand(t, x, keep)
    assert float((got - want).abs().max() / want.abs().max()) < 1e-12


def _by_hand(t, x, keep):
    ca = t.crs_attn
    attn = ca.get_attn(x) * keep.view(2, 8, 4, 50)                    # (B, H, T, M): row h * T + t of keep
    ctx = torch.matmul(attn, ca._heads(ca.v_w, x, ca.D_v)).transpose(1, 2).contiguous().view(2, 4, -1)
    return t.mlp(ca.layer_norm(ca.fc(ctx) + ca.q))


def test_supported():
    cpu = torch.device("cpu")
    for conf in (synth.mnist_conf(N=64, M=8, I=8), synth.traffic_conf(N=64, M=8, I=8), synth.camelyon_conf(N=64, M=8, I=8)):
        assert fused_aggregator.supported(IPSNet(cpu, conf).transf)
    args = (1, 8, 512, 64, 64, 2048)
    assert fused_aggregator.supported(Transformer(*args))
    biased = Transformer(*args)
    biased.crs_attn.k_w = nn.Linear(512, 512, bias=True)
    assert not fused_aggregator.supported(biased)

    class Other(MultiHeadCrossAttention):
        pass
    sub = Transformer(*args)
    sub.crs_attn = Other(1, 8, 512, 64, 64)
    assert not fused_aggregator.supported(sub)
    assert not fused_aggregator.supported(Transformer(3, 11, 64, 8, 8, 96))          # R = 33
    assert fused_aggregator.supported(Transformer(4, 8, 64, 8, 8, 96))               # R = 32
    assert not fused_aggregator.supported(Transformer(1, 8, 40, 8, 8, 96))           # D = 40
    assert not fused_aggregator.supported(Transformer(*args).double())


def test_enabled_follows_the_environment(monkeypatch):
    monkeypatch.delenv("IPSX_TRAIN_AGGREGATOR", raising=False)
    assert fused_aggregator.enabled()
    monkeypatch.setenv("IPSX_TRAIN_AGGREGATOR", "0")
    assert not fused_aggregator.enabled()
    monkeypatch.setenv("IPSX_TRAIN_AGGREGATOR", "1")
    assert fused_aggregator.enabled()


def test_library_sizes():
    from ips_amd import hip
    L = hip.lib()
    assert L.ipsx_version() % 100 >= 5
    for R, D, ok in ((8, 512, 1), (32, 128, 1), (1, 32, 1), (32, 1024, 1), (33, 64, 0), (0, 64, 0), (8, 40, 0), (8, 1056, 0)):
        assert L.ipsx_attn_pool_supported(R, D) == ok, (R, D)
    assert L.ipsx_attn_pool_workspace_bytes(16, 5000, 8, 512) == (16 * 40 * 8 * 512 + 16 * 32) * 4
    assert L.ipsx_attn_pool_workspace_bytes(1, 1, 1, 32) == 128 + 128
    assert L.ipsx_attn_pool_workspace_bytes(16, 5000, 33, 512) == 0
