"""The masked encoder pass's DEFINITION on the CPU: ``net(mem, pos, mem_count=c, mask_encoder=True)`` is

    rows = cat_b(range(b * M, b * M + c[b]));  emb = zeros(B * M, D);  emb[rows] = net._embed(flat[rows])

followed by ``forward(mem_count=c)``'s aggregation - predictions, parameter gradients, BatchNorm buffers -, for a feature net
and a small image net; what lies in the padding cannot reach anything; the default is today's call; the refusals; the way
from the training loop's ``mask_padding: 'encoder'``.  No GPU, no library call."""

import copy

import pytest
import torch

from ips_amd import synth
from ips_amd.architecture import IPSNet
from ips_amd.training import iterative

B, M = 3, 8
COUNTS = (2, 8, 5)
ROWS = torch.cat([torch.arange(b * M, b * M + c) for b, c in enumerate(COUNTS)])


def _feature_net():
    conf = synth.camelyon_conf(N=32, M=M, I=8, D=64, D_k=8, D_v=8, D_inner=128, n_chan_in=64, B=B, attn_dropout=0.0, dropout=0.0)
    return conf, synth.fill_weights(IPSNet(torch.device("cpu"), conf), 7)


def _image_net():
    conf = synth.mnist_conf(N=32, M=M, I=8, patch=32, B=B, attn_dropout=0.0, dropout=0.0)
    return conf, synth.fill_weights(IPSNet(torch.device("cpu"), conf), 7)


NETS = {"features": _feature_net, "images": _image_net}


def _mem(conf, seed=8):
    g = torch.Generator().manual_seed(seed)
    shape = (B, M, conf.n_chan_in, *conf.patch_size) if conf.is_image else (B, M, conf.n_chan_in)
    mem = torch.randn(shape, generator=g).relu()
    for b, c in enumerate(COUNTS):
        mem[b, c:] = 0.0                       # what pad=True leaves behind a short slide
    return mem


def _poisoned(mem, value):
    out = mem.clone()
    for b, c in enumerate(COUNTS):
        out[b, c:] = value
    return out


def _loss(preds):
    return sum((p * torch.arange(1, p.numel() + 1, dtype=p.dtype).view_as(p)).sum() for p in preds.values())


def _by_hand(net, mem):
    """The definition written out: the encoder on the gathered filled rows, scattered into zeros, then forward(mem_count=)'s
    aggregation on that embedding."""
    flat = mem.reshape(B * M, *mem.shape[2:])
    packed = net._embed(flat[ROWS])
    emb = torch.zeros((B * M, packed.shape[1])).index_copy(0, ROWS, packed)
    return net.get_preds(net.transf(emb.view(B, M, -1), count=COUNTS)), emb


def _buffers(net):
    return {n: b.clone() for n, b in net.encoder.named_buffers()}


def _record_transf(net, monkeypatch):
    seen, real = [], net.transf.forward

    def recording(x, count=None):
        seen.append(x.detach().clone())
        return real(x, count=count)
    monkeypatch.setattr(net.transf, "forward", recording)
    return seen


@pytest.mark.parametrize("kind", list(NETS))
def test_train_mode_is_the_definition(kind, monkeypatch):
    conf, net = NETS[kind]()
    net.train()
    hand = copy.deepcopy(net)
    mem = _mem(conf)
    seen = _record_transf(net, monkeypatch)
    preds = net(mem, None, mem_count=COUNTS, mask_encoder=True)
    want, emb = _by_hand(hand, mem)
    for k in want:
        assert torch.equal(preds[k], want[k]), k
    # the transformer received exactly +0.0 in the padding slots
    got = seen[0].view(B, M, -1)
    assert torch.equal(got, emb.detach().view(B, M, -1))
    for b, c in enumerate(COUNTS):
        assert torch.equal(got[b, c:], torch.zeros_like(got[b, c:])) and not bool(torch.signbit(got[b, c:]).any()), b
    _loss(preds).backward()
    _loss(want).backward()
    for (n, p), (_, q) in zip(net.named_parameters(), hand.named_parameters()):
        assert q.grad is not None and torch.equal(p.grad, q.grad), n
    bufs, hand_bufs = _buffers(net), _buffers(hand)
    assert any(n.endswith("num_batches_tracked") for n in bufs)
    for n in bufs:
        assert torch.equal(bufs[n], hand_bufs[n]), n
        if n.endswith("num_batches_tracked"):
            assert int(bufs[n]) == 1, n


def test_running_statistics_are_those_of_the_filled_rows():
    """The projector's BatchNorm1d: momentum * (batch mean | unbiased variance over n_fill = 15 rows) of Linear(LN(x[rows]))."""
    conf, net = _feature_net()
    net.train()
    mem = _mem(conf)
    ln, lin, bn, _ = net.encoder.children()
    before_mean, before_var = bn.running_mean.clone(), bn.running_var.clone()
    net(mem, None, mem_count=COUNTS, mask_encoder=True)
    with torch.no_grad():
        z = lin(ln(mem.reshape(B * M, -1)[ROWS])).double()
    n_fill = sum(COUNTS)
    assert z.shape[0] == n_fill == 15
    want_mean = (1 - bn.momentum) * before_mean.double() + bn.momentum * z.mean(0)
    want_var = (1 - bn.momentum) * before_var.double() + bn.momentum * z.var(0, unbiased=False) * n_fill / (n_fill - 1)
    assert torch.allclose(bn.running_mean.double(), want_mean, rtol=1e-5, atol=1e-6)
    assert torch.allclose(bn.running_var.double(), want_var, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("kind", list(NETS))
@pytest.mark.parametrize("value", [float("nan"), 1e30], ids=["nan", "1e30"])
def test_padding_content_changes_nothing(kind, value):
    conf, net = NETS[kind]()
    net.train()
    other = copy.deepcopy(net)
    mem = _mem(conf)
    a = net(mem, None, mem_count=COUNTS, mask_encoder=True)
    b = other(_poisoned(mem, value), None, mem_count=COUNTS, mask_encoder=True)
    _loss(a).backward()
    _loss(b).backward()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for (n, p), (_, q) in zip(net.named_parameters(), other.named_parameters()):
        assert torch.equal(p.grad, q.grad), n
    for (n, p), (_, q) in zip(net.encoder.named_buffers(), other.encoder.named_buffers()):
        assert torch.equal(p, q), n


@pytest.mark.parametrize("kind", list(NETS))
def test_without_the_flag_the_padding_shapes_the_encoder(kind):
    conf, net = NETS[kind]()
    net.train()
    plain, poisoned = copy.deepcopy(net), copy.deepcopy(net)
    mem = _mem(conf)
    masked = net(mem, None, mem_count=COUNTS, mask_encoder=True)
    unmasked = plain(mem, None, mem_count=COUNTS)
    nan = poisoned(_poisoned(mem, float("nan")), None, mem_count=COUNTS)
    for k in masked:
        assert not torch.equal(masked[k], unmasked[k]), k
        assert bool(torch.isnan(nan[k]).all()), k
    bn = [m for m in net.encoder.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)][0]
    bn_plain = [m for m in plain.encoder.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)][0]
    assert not torch.equal(bn.running_mean, bn_plain.running_mean)


@pytest.mark.parametrize("kind", list(NETS))
def test_eval_mode_keeps_the_filled_rows_and_zeroes_the_padding(kind, monkeypatch):
    conf, net = NETS[kind]()
    net.eval()
    mem = _mem(conf)
    seen = _record_transf(net, monkeypatch)
    before = _buffers(net)
    with torch.no_grad():
        net(mem, None, mem_count=COUNTS, mask_encoder=True)
        net(mem, None, mem_count=COUNTS)
        packed = net._embed(mem.reshape(B * M, *mem.shape[2:])[ROWS])
    masked, plain = seen[0].view(B, M, -1), seen[1].view(B, M, -1)
    assert torch.equal(masked.reshape(B * M, -1)[ROWS], packed)
    for b, c in enumerate(COUNTS):
        # eval mode: rows are independent - the filled rows' embeddings are the bits of today's pass over all B * M rows
        assert torch.equal(masked[b, :c], plain[b, :c]), b
        assert torch.equal(masked[b, c:], torch.zeros_like(masked[b, c:])), b
        if c < M:
            assert bool((plain[b, c:] != 0).any()), b           # (today: the blank row's embedding)
    for n, buf in net.encoder.named_buffers():
        assert torch.equal(buf, before[n]), n


def test_mem_emb_in_eval_mode_leaves_the_flag_nothing_to_do(monkeypatch):
    conf, net = _feature_net()
    net.eval()
    mem = _mem(conf)
    emb = torch.randn((B, M, conf.D), generator=torch.Generator().manual_seed(9))
    monkeypatch.setattr(net, "_embed", lambda *a, **k: pytest.fail("an encoder pass"))
    with torch.no_grad():
        a = net(mem, None, mem_emb=emb, mem_count=COUNTS, mask_encoder=True)
        b = net(mem, None, mem_emb=emb, mem_count=COUNTS)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("kind", list(NETS))
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_the_default_is_todays_call(kind, mode, monkeypatch):
    conf, net = NETS[kind]()
    getattr(net, mode)()
    mem = _mem(conf)
    nets = [copy.deepcopy(net) for _ in range(4)]
    calls = []
    for n in nets:                                   # (no call may reach the masked pass)
        monkeypatch.setattr(n, "_embed_filled", lambda *a, **k: calls.append(a))
    with torch.set_grad_enabled(mode == "train"):
        flat = mem.reshape(B * M, *mem.shape[2:])
        want = nets[0].get_preds(nets[0].transf(nets[0]._embed(flat).view(B, M, -1)))
        want_counted = nets[1].get_preds(nets[1].transf(nets[1]._embed(flat).view(B, M, -1), count=COUNTS))
        nets[2]._mem_count = COUNTS                  # forward never reads last_mem_count by itself
        got = nets[2](mem, None, mask_encoder=False)
        got_counted = nets[3](mem, None, mem_count=COUNTS, mask_encoder=False)
    assert not calls
    for k in want:
        assert torch.equal(got[k], want[k]), k
        assert torch.equal(got_counted[k], want_counted[k]), k
    for a, b in ((nets[2], nets[0]), (nets[3], nets[1])):
        for (n, p), (_, q) in zip(a.encoder.named_buffers(), b.encoder.named_buffers()):
            assert torch.equal(p, q), n


def test_full_counts_are_the_unmasked_encoder():
    conf, net = _feature_net()
    net.train()
    other = copy.deepcopy(net)
    mem = _mem(conf)
    a = net(mem, None, mem_count=(M,) * B, mask_encoder=True)
    b = other(mem, None, mem_count=(M,) * B)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for (n, p), (_, q) in zip(net.encoder.named_buffers(), other.encoder.named_buffers()):
        assert torch.equal(p, q), n


REFUSED = {
    "no count": None,
    "short": (2, 8),
    "long": (2, 8, 5, 5),
    "zero": (0, 8, 5),
    "M+1": (2, M + 1, 5),
    "tensor short": torch.tensor([2, 8]),
    "tensor zero": torch.tensor([2, 0, 5]),
    "meta tensor (not on the host)": torch.empty((3,), dtype=torch.int64, device="meta"),
}


@pytest.mark.parametrize("kind", list(NETS))
@pytest.mark.parametrize("count", list(REFUSED.values()), ids=list(REFUSED))
def test_refusals_touch_nothing(kind, count):
    conf, net = NETS[kind]()
    net.train()
    mem = _mem(conf)
    before, rng = _buffers(net), torch.get_rng_state()
    with pytest.raises(ValueError):
        net(mem, None, mem_count=count, mask_encoder=True)
    assert torch.equal(torch.get_rng_state(), rng)
    for n, buf in net.encoder.named_buffers():
        assert torch.equal(buf, before[n]), n


@pytest.mark.parametrize("kind", list(NETS))
def test_one_filled_row_in_training_mode_is_refused(kind):
    conf, net = NETS[kind]()
    mem = _mem(conf)[:1]
    net.train()
    before = _buffers(net)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        net(mem, None, mem_count=(1,), mask_encoder=True)
    for n, buf in net.encoder.named_buffers():
        assert torch.equal(buf, before[n]), n
    net.eval()                                       # (eval mode: rows are independent, one row is a batch like any other)
    with torch.no_grad():
        net(mem, None, mem_count=(1,), mask_encoder=True)


def test_a_cpu_count_tensor_is_read():
    conf, net = _feature_net()
    net.eval()
    mem = _mem(conf)
    with torch.no_grad():
        a = net(mem, None, mem_count=torch.tensor(COUNTS), mask_encoder=True)
        b = net(mem, None, mem_count=COUNTS, mask_encoder=True)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("flag,left,want", [
    (None, COUNTS, {}), (False, COUNTS, {}), (True, None, {}), (True, COUNTS, {"mem_count": COUNTS}),
    ("encoder", None, {}), ("encoder", COUNTS, {"mem_count": COUNTS, "mask_encoder": True})],
    ids=["no field", "off", "on, no count", "on", "encoder, no count", "encoder"])
def test_training_loop_passes_mask_encoder_only_under_encoder(flag, left, want, monkeypatch):
    conf, net = _feature_net()
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
    assert seen[0][1] == want
    assert seen[1][1] == dict(want, mem_emb=emb) and seen[1][1]["mem_emb"] is emb
