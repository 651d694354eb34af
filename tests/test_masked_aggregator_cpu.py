"""The masked aggregator's DEFINITION, on the CPU in float64: ``Transformer.forward(x, count=)`` on the stock
modules with the ATen mask against the call that never sees padding - ``transf(x[b:b + 1, :count[b]])`` - output and
gradients; ``count=None`` untouched; the refusals of host counts; and the way from ``IPSNet.forward(mem_count=)`` and from
the training loop's ``conf.mask_padding`` down to the transformer.  No GPU, no library call."""

import copy

import pytest
import torch

from ips_amd import hip, synth
from ips_amd.architecture import IPSNet
from ips_amd.architecture.transformer import Transformer
from ips_amd.training import fused_aggregator, iterative

D, H, T, B, M = 32, 2, 2, 3, 9
COUNTS = (1, 4, 9)
TOL = dict(rtol=1e-12, atol=1e-14)          # float64, the same work up to summation order


def _transf(seed=3):
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        return Transformer(T, H, D, 8, 8, 64, attn_dropout=0.0, dropout=0.0).double()


def _x(seed=4):
    return torch.randn((B, M, D), dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


def _weights(seed=5):
    return torch.randn((B, T, D), dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


def test_masked_call_is_the_solo_call_on_the_filled_slots():
    transf, x, w = _transf(), _x(), _weights()
    xm = x.clone().requires_grad_()
    out = transf(xm, count=COUNTS)
    assert out.shape == (B, T, D)
    (out * w).sum().backward()
    masked_grads = {n: p.grad.clone() for n, p in transf.named_parameters()}
    solo_sum = {n: torch.zeros_like(p) for n, p in transf.named_parameters()}
    for b, c in enumerate(COUNTS):
        solo = copy.deepcopy(transf)
        solo.zero_grad()
        xs = x[b:b + 1, :c].clone().requires_grad_()
        ys = solo(xs)
        assert torch.allclose(out[b], ys[0], **TOL), b
        (ys * w[b:b + 1]).sum().backward()
        assert torch.allclose(xm.grad[b, :c], xs.grad[0], **TOL), b
        assert torch.equal(xm.grad[b, c:], torch.zeros_like(xm.grad[b, c:])), b          # exactly zero beyond the count
        for n, p in solo.named_parameters():
            solo_sum[n] += p.grad
    for n in masked_grads:
        assert torch.allclose(masked_grads[n], solo_sum[n], **TOL), n


def test_padding_content_cannot_reach_the_output():
    transf, x = _transf(), _x()
    ref = transf(x, count=COUNTS)
    y = x.clone()
    for b, c in enumerate(COUNTS):
        y[b, c:] = 1e30
    assert torch.equal(transf(y, count=COUNTS), ref)


def test_count_none_and_full_counts_are_the_unmasked_call():
    transf, x = _transf(), _x()
    base = transf.mlp(transf.crs_attn(x))
    assert torch.equal(transf(x), base) and torch.equal(transf(x, count=None), base)
    assert torch.equal(transf(x, count=(M,) * B), base)
    assert torch.equal(transf(x, count=torch.full((B,), M)), base)


def test_attention_definition_and_aten_pool():
    """compute_attn's probabilities are exactly +0.0 beyond the count and sum to 1 within it; ``aten_pool(count=)`` is the
    solo pool on the filled rows."""
    transf, x = _transf(), _x()
    ca = transf.crs_attn
    count = torch.tensor(COUNTS)
    attn = ca.attention.compute_attn(ca._heads(ca.q_w, ca.q, ca.D_k), ca._heads(ca.k_w, x, ca.D_k), count)
    A = torch.randn((H * T, D), dtype=torch.float64, generator=torch.Generator().manual_seed(6))
    Z = fused_aggregator.aten_pool(x, A, None, COUNTS)
    for b, c in enumerate(COUNTS):
        assert torch.equal(attn[b, :, :, c:], torch.zeros_like(attn[b, :, :, c:])) and not bool(torch.signbit(attn[b, :, :, c:]).any())
        assert torch.allclose(attn[b, :, :, :c].sum(-1), torch.ones((H, T), dtype=torch.float64), **TOL)
        assert torch.allclose(Z[b], fused_aggregator.aten_pool(x[b:b + 1, :c], A)[0], **TOL)
    got = fused_aggregator.forward(transf, x, pool=fused_aggregator.aten_pool, count=count)
    assert torch.allclose(got, transf(x, count=count), **TOL)


@pytest.mark.parametrize("count", [(1, 4), (1, 4, 9, 9), (0, 4, 9), (1, 4, M + 1), torch.tensor([1, 4]), torch.tensor([1, 0, 9])],
                         ids=["short", "long", "zero", "M+1", "tensor short", "tensor zero"])
def test_host_counts_are_checked(count):
    transf, x = _transf(), _x()
    with pytest.raises(ValueError):
        transf(x, count=count)
    with pytest.raises(ValueError):
        hip.slot_counts("test", count, B, M, torch.device("cpu"))


def test_counts_must_be_integers():
    with pytest.raises(TypeError):
        hip.slot_counts("test", torch.tensor([1.0, 4.0, 9.0]), B, M, torch.device("cpu"))
    with pytest.raises(TypeError):
        hip.slot_counts("test", (1.5, 4, 9), B, M, torch.device("cpu"))
    out = hip.slot_counts("test", COUNTS, B, M, torch.device("cpu"))
    assert out.dtype == torch.int32 and out.tolist() == list(COUNTS)


def _net():
    conf = synth.camelyon_conf(N=32, M=8, I=8, D=64, D_k=8, D_v=8, D_inner=128, n_chan_in=64, B=3)
    return conf, synth.fill_weights(IPSNet(torch.device("cpu"), conf), 7).eval()


def test_ipsnet_forward_hands_mem_count_to_the_transformer(monkeypatch):
    conf, net = _net()
    seen = []
    real = net.transf.forward

    def recording(x, count=None):
        seen.append(count)
        return real(x, count=count)
    monkeypatch.setattr(net.transf, "forward", recording)
    mem = torch.randn((3, 8, conf.n_chan_in), generator=torch.Generator().manual_seed(8)).relu()
    counts = (2, 8, 5)
    with torch.no_grad():
        masked = net(mem, None, mem_count=counts)
        plain = net(mem, None)
        assert seen == [counts, None]
        net._mem_count = counts                       # forward never reads last_mem_count by itself
        again = net(mem, None)
        assert seen[-1] is None
        # slide 1 is full: its prediction does not move; the others are the solo calls' (eval BatchNorm: rows independent)
        for k in plain:
            assert torch.equal(again[k], plain[k])
            assert torch.allclose(masked[k][1], plain[k][1], rtol=1e-5, atol=1e-7)
            for b in (0, 2):
                solo = net(mem[b:b + 1, :counts[b]], None)
                assert torch.allclose(masked[k][b], solo[k][0], rtol=1e-5, atol=1e-7)
                assert not torch.allclose(plain[k][b], solo[k][0], rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("flag,left,want", [(None, (2, 8, 5), None), (False, (2, 8, 5), None), (True, None, None), (True, (2, 8, 5), (2, 8, 5))],
                         ids=["no field", "off", "on, no count", "on"])
def test_training_loop_passes_the_count_only_under_mask_padding(flag, left, want, monkeypatch):
    conf, net = _net()
    if flag is not None:
        conf = conf.clone(mask_padding=flag)
    net._mem_count = left
    seen = []

    def recording(*args, **kwargs):
        seen.append((len(args), dict(kwargs)))
        return {"metastases": torch.full((3, 1), 0.5)}
    monkeypatch.setattr(net, "forward", recording)
    labels = {"metastases": torch.tensor([0, 1, 1])}
    crit = {"metastases": torch.nn.BCELoss()}
    mem = torch.zeros((3, 8, conf.n_chan_in))
    iterative.compute_loss(net, mem, None, crit, labels, conf)
    emb = torch.zeros((3, 8, conf.D))
    iterative.compute_loss(net, mem, None, crit, labels, conf, mem_emb=emb)
    assert [n for n, _ in seen] == [2, 2]
    assert seen[0][1] == ({} if want is None else {"mem_count": want})
    assert set(seen[1][1]) == ({"mem_emb"} if want is None else {"mem_emb", "mem_count"})
    assert seen[1][1]["mem_emb"] is emb and seen[1][1].get("mem_count") == want
