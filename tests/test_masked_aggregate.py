"""The masked EVAL aggregator (csrc/aggregate.hip attn_ctx_kernel<true>, ipsx_aggregate_counted): a slide of
a zero-padded batch aggregated from its filled slots only has the BITS of the unmasked call on those slots alone - through
``hip.aggregate``, through ``net(..., mem_count=)`` and after ``ips_ragged(pad=True)``.  M = 130 with one slide per count
1, 63, 64, 65, 129, 130: the context kernel's 64-lane stride and its seams."""

import pytest
import torch

from ips_amd import hip, synth
from ips_amd.architecture import IPSNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M = 130
COUNTS = (1, 63, 64, 65, 129, 130)
B = len(COUNTS)

CASES = {
    "cam T=1": lambda: synth.camelyon_conf(N=512, M=M, I=M, D=128, D_k=16, D_v=16, D_inner=256, n_chan_in=64, n_token=1),
    "cam T=4": lambda: synth.camelyon_conf(N=512, M=M, I=M, D=128, D_k=16, D_v=16, D_inner=256, n_chan_in=64, n_token=4),
    "mnist T=1": lambda: synth.mnist_conf(N=512, M=M, I=M, n_token=1),
    "mnist T=4": lambda: synth.mnist_conf(N=512, M=M, I=M, n_token=4),
}


def _net(conf):
    conf.tasks = {k: t for k, t in conf.tasks.items() if t["id"] < conf.n_token}          # (a task reads the token of its id)
    return synth.fill_weights(IPSNet(torch.device(DEV), conf), 7).to(DEV).eval()


def _emb(conf, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, M, conf.D), generator=g)
    for b, c in enumerate(COUNTS):          # what pad=True leaves behind a short slide: the same made-up row in every padded slot
        x[b, c:] = x[b, -1]
    return x.to(DEV)


@pytest.mark.parametrize("case", list(CASES))
def test_counted_aggregate_has_the_bits_of_the_solo_call(case):
    conf = CASES[case]()
    net = _net(conf)
    x = _emb(conf)
    with torch.no_grad():
        got = hip.aggregate(net.transf, x, COUNTS)
        on_device = hip.aggregate(net.transf, x, torch.tensor(COUNTS, device=DEV))          # (not read back: the same kernel)
        through_module = net.transf(x, count=COUNTS)
        plain = hip.aggregate(net.transf, x)
        for b, c in enumerate(COUNTS):
            solo = hip.aggregate(net.transf, x[b:b + 1, :c].contiguous())
            assert torch.equal(got[b], solo[0]), (case, c)
            if c < M:
                assert not torch.equal(plain[b], solo[0]), (case, c)          # (the padding does move the unmasked call)
    assert torch.equal(on_device, got) and torch.equal(through_module, got)
    assert bool(torch.isfinite(got).all())


@pytest.mark.parametrize("case", list(CASES))
def test_padding_content_cannot_reach_the_output(case):
    conf = CASES[case]()
    net = _net(conf)
    x = _emb(conf)
    y = x.clone()
    for b, c in enumerate(COUNTS):
        y[b, c:] = float("nan")          # (the context kernel reads neither the logits nor the V rows of a padded slot)
    with torch.no_grad():
        assert torch.equal(hip.aggregate(net.transf, y, COUNTS), hip.aggregate(net.transf, x, COUNTS))


@pytest.mark.parametrize("case", list(CASES))
def test_forward_with_mem_count(case):
    """``net(mem_patch, mem_pos, mem_emb=, mem_count=)`` in eval mode against the solo calls on the filled slots."""
    conf = CASES[case]()
    net = _net(conf)
    emb = _emb(conf, 5)
    g = torch.Generator().manual_seed(6)
    if conf.is_image:
        mem_patch = torch.zeros((B, M, conf.n_chan_in, *conf.patch_size), device=DEV)          # (mem_emb stands for them in eval mode)
        mem_pos = torch.randn((B, M, conf.D), generator=g).to(DEV)
    else:
        mem_patch, mem_pos = torch.zeros((B, M, conf.n_chan_in), device=DEV), None
    with torch.no_grad():
        got = net(mem_patch, mem_pos, mem_emb=emb, mem_count=COUNTS)
        plain = net(mem_patch, mem_pos, mem_emb=emb)
        for b, c in enumerate(COUNTS):
            solo = net(mem_patch[b:b + 1, :c], mem_pos[b:b + 1, :c] if mem_pos is not None else None, mem_emb=emb[b:b + 1, :c])
            for k in solo:
                assert torch.equal(got[k][b], solo[k][0]), (case, k, c)
        for k in plain:
            assert torch.equal(got[k][B - 1], plain[k][B - 1])          # the full slide: the mask changes nothing


def test_count_none_is_the_unmasked_export(monkeypatch):
    """``count=None`` reaches ipsx_aggregate_packed - the export and the kernel instantiation of before - and never the
    counted one; counts of M everywhere give the same bits through the counted kernel."""
    conf = CASES["cam T=4"]()
    net = _net(conf)
    x = _emb(conf)
    real = hip.lib()
    names = []

    class Spy:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if name.startswith("ipsx_aggregate") and not name.endswith("_bytes"):
                names.append(name)
            return fn
    with torch.no_grad():
        before = hip.aggregate(net.transf, x)
        monkeypatch.setattr(hip, "lib", lambda: Spy())
        none = hip.aggregate(net.transf, x, None)
        default = net.transf(x)
        assert names == ["ipsx_aggregate_packed"] * 2
        full = hip.aggregate(net.transf, x, (M,) * B)
        assert names[2:] == ["ipsx_aggregate_counted"]
    assert torch.equal(none, before) and torch.equal(default, before) and torch.equal(full, before)


def test_refusals():
    conf = CASES["cam T=1"]()
    net = _net(conf)
    x = _emb(conf)
    for bad in ((1,) * (B - 1), (0,) + COUNTS[1:], COUNTS[:-1] + (M + 1,), torch.tensor(COUNTS[:-1], device=DEV)):
        with pytest.raises(ValueError):
            hip.aggregate(net.transf, x, bad)
    with pytest.raises(TypeError):
        hip.aggregate(net.transf, x, torch.ones(B, device=DEV))
    t = hip.Transf()          # the C entry point refuses a null count before it reads anything else
    assert hip.lib().ipsx_aggregate_counted(hip.C.byref(t), None, None, None, None, B, M, None, None, 0, None) != 0


def test_after_a_padded_ragged_selection():
    """ips_ragged(pad=True) on slides of 3, 8 and 20 rows at M = I = 8, then the masked forward: the short slides are
    classified as the loop of solo calls classifies them, bit for bit; the long slide as without the mask."""
    conf = synth.camelyon_conf(N=64, M=8, I=8, D=128, D_k=16, D_v=16, D_inner=256, n_chan_in=64)
    net = _net(conf)
    lengths = (3, 8, 20)
    g = torch.Generator().manual_seed(9)
    slides = [torch.randn((n, conf.n_chan_in), generator=g).relu().to(DEV) for n in lengths]
    with torch.no_grad():
        mem_patch, mem_pos = net.ips_ragged(slides, pad=True)
        count, emb = net.last_mem_count, net.last_mem_emb
        assert count == (3, 8, 8) and mem_patch.shape[:2] == (3, 8)
        masked = net(mem_patch, mem_pos, mem_emb=emb, mem_count=count)
        plain = net(mem_patch, mem_pos, mem_emb=emb)
        for b in (0, 1):
            p, pos = net.ips(slides[b][None])
            assert p.shape[1] == lengths[b] and torch.equal(p[0], mem_patch[b, :lengths[b]])
            solo = net(p, pos)
            for k in solo:
                assert torch.equal(masked[k][b], solo[k][0]), (k, b)
        for k in plain:
            assert torch.equal(masked[k][2], plain[k][2])
            assert not torch.equal(masked[k][0], plain[k][0])          # 3 real rows and 5 made-up ones are another slide
