"""The masked encoder pass on the feature projector's row-indexed kernels (csrc/projector_train.hip's INDEXED
instantiations, ``hip.projector_train_forward(index=)``, ``hip.projector_wgrad(index=)``, ``fused_projector.encode(rows=)``,
``IPSNet.forward(mask_encoder=True)``).

The indexed kernels do the plain kernels' arithmetic in the plain kernels' slab, chunk and k order on the packed rows, so
everything is held to ``torch.equal`` against the plain calls on the gathered copy ``x[rows]`` - exports that
tests/test_train_projector.py holds to float64.  At the net level the fused route is another summation order than the
generic route (ATen gather + the stock modules): there the yardstick of that file applies - per tensor, the error against
float64 autograd of the definition at most 4 x the stock float32 route's."""

import copy

import pytest
import torch
from torch import nn

from ips_amd import hip, hip_train, synth
from ips_amd.architecture import IPSNet
from ips_amd.training import fused_projector

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LN_EPS = 1e-5


def _rows(counts, M):
    return torch.cat([torch.arange(b * M, b * M + c, dtype=torch.int32) for b, c in enumerate(counts)]).to(DEV)


def _inputs(n_src, f, d, seed, dtype=torch.float32):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn((n_src, f), generator=g) * (0.5 + torch.rand((1, f), generator=g)) + 0.5 * torch.randn((1, f), generator=g)
    w = torch.randn((d, f), generator=g) / f ** 0.5
    b = 0.1 * torch.randn(d, generator=g)
    return x.to(DEV).to(dtype), w.to(DEV), b.to(DEV)


def _poison(x, rows):
    """NaN in every row of ``x`` outside ``rows``"""
    keep = torch.zeros(x.shape[0], dtype=torch.bool, device=x.device)
    keep[rows.long()] = True
    out = x.clone()
    out[~keep] = float("nan")
    return out


# ---------------------------------------------------------------- forward
F_B, F_M, F_COUNTS = 6, 70, (1, 63, 64, 65, 70, 7)          # n_fill = 270: five slabs, seams inside a slab and on a slab's
                                                            # edge (rows 64, 128), the last slab partial, the shift's eight
                                                            # rows over two slides


@pytest.mark.parametrize("f,d,dtype", [(32, 32, torch.float32), (96, 64, torch.float32), (64, 512, torch.float32),
                                       (96, 64, torch.float16), (96, 64, torch.bfloat16)],
                         ids=["32x32", "96x64", "64x512", "96x64 f16", "96x64 bf16"])
def test_forward_is_the_plain_call_on_the_gathered_rows(f, d, dtype):
    rows = _rows(F_COUNTS, F_M)
    assert rows.numel() == 270
    x, w, b = _inputs(F_B * F_M, f, d, seed=f + d, dtype=dtype)
    want = hip.projector_train_forward(x[rows.long()].contiguous(), w, b, LN_EPS)
    got = hip.projector_train_forward(x, w, b, LN_EPS, index=rows)
    names = ("z", "stats", "partial", "slabs", "shift")
    assert got[3] == want[3] == 5
    for name, a, r in zip(names, got, want):
        if name != "slabs":
            assert a.shape == r.shape and torch.equal(a, r), name
    assert bool(torch.isfinite(got[0]).all())
    if (f, d, dtype) == (32, 32, torch.float32):            # nothing outside the index is read
        poisoned = hip.projector_train_forward(_poison(x, rows), w, b, LN_EPS, index=rows)
        for name, a, r in zip(names, poisoned, want):
            if name != "slabs":
                assert torch.equal(a, r), name


# ---------------------------------------------------------------- weight gradient
W_B, W_M, W_COUNTS = 3, 3000, (2999, 1, 3000)               # n_fill = 6000: a seam at the odd packed row 2999 inside chunk 0, a
                                                            # seam on a row pair (3000), a partial second chunk (1904 rows)


def _wgrad_case(f, d):
    rows = _rows(W_COUNTS, W_M)
    x, w, b = _inputs(W_B * W_M, f, d, seed=f * d)
    dz = torch.randn((rows.numel(), d), generator=torch.Generator().manual_seed(f + d)).to(DEV)
    xg = x[rows.long()].contiguous()
    _, stats, _, _, _ = hip.projector_train_forward(xg, w, b, LN_EPS)
    dw, db = hip.projector_wgrad(xg, dz, stats)
    return x, rows, dz, stats, dw, db


# (288, 256): across the 256-column and the 128-row edge of a workgroup's region of dW.  D is a power of two for these
# kernels and the BatchNorm behind them (ipsx_projector_train_supported), so 256 is the smallest D beyond one 128-row region.
@pytest.mark.parametrize("f,d", [(32, 32), (288, 256)], ids=["32x32", "288x256"])
def test_wgrad_is_the_plain_call_on_the_gathered_rows(f, d, monkeypatch):
    x, rows, dz, stats, dw, db = _wgrad_case(f, d)
    got_w, got_b = hip.projector_wgrad(x, dz, stats, index=rows)
    assert torch.equal(got_w, dw) and torch.equal(got_b, db)
    assert bool(torch.isfinite(got_w).all()) and float(got_w.abs().max()) > 0.0
    monkeypatch.setenv("IPSX_TRAIN_PROJECTOR_SLICE_ROWS", "4096")          # two calls, the second adding onto the first
    assert hip_train._projector_wgrad_slice_rows(f, d, torch.float32) == 4096
    sl_w, sl_b = hip.projector_wgrad(x, dz, stats, index=rows)
    assert torch.equal(sl_w, dw) and torch.equal(sl_b, db)
    monkeypatch.undo()
    if (f, d) == (32, 32):                                   # nothing outside the index is read, and a row pair beyond the
        po_w, po_b = hip.projector_wgrad(_poison(x, rows), dz, stats, index=rows)        # chunk adds exact zeros
        assert torch.equal(po_w, dw) and torch.equal(po_b, db)


# ---------------------------------------------------------------- the node
def _encoder(f, d, seed):
    torch.manual_seed(seed)
    enc = nn.Sequential(nn.LayerNorm(f, eps=LN_EPS, elementwise_affine=False), nn.Linear(f, d), nn.BatchNorm1d(d), nn.ReLU())
    with torch.no_grad():
        enc[2].weight.uniform_(0.5, 1.5)
        enc[2].bias.normal_(0.0, 0.2)
        enc[2].running_mean.normal_(0.0, 0.1)
        enc[2].running_var.uniform_(0.5, 1.5)
    return enc.to(DEV).train()


def test_node_is_the_uncounted_node_on_the_gathered_rows():
    f, d = 96, 64
    rows = _rows(F_COUNTS, F_M)
    x, _, _ = _inputs(F_B * F_M, f, d, seed=11)
    enc = _encoder(f, d, 5)
    other = copy.deepcopy(enc)
    dy = torch.randn((rows.numel(), d), generator=torch.Generator().manual_seed(12)).to(DEV)
    y = fused_projector.encode(enc, _poison(x, rows), rows=rows)
    want = fused_projector.encode(other, x[rows.long()].contiguous())
    assert y.shape == (270, d) and torch.equal(y, want)
    y.backward(dy)
    want.backward(dy)
    for (n, p), (_, q) in zip(enc.named_parameters(), other.named_parameters()):
        assert p.grad is not None and torch.equal(p.grad, q.grad), n
        assert bool(torch.isfinite(p.grad).all()), n
    for (n, p), (_, q) in zip(enc.named_buffers(), other.named_buffers()):
        assert torch.equal(p, q), n
    assert int(enc[2].num_batches_tracked) == 1


# ---------------------------------------------------------------- the net
N_B, N_M, N_COUNTS = 6, 70, (1, 63, 64, 65, 70, 7)


def _conf():
    return synth.camelyon_conf(N=256, M=N_M, I=N_M, D=64, D_k=8, D_v=8, D_inner=128, n_chan_in=64, B=N_B, attn_dropout=0.0, dropout=0.0)


def _mem(seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    mem = torch.randn((N_B, N_M, 64), generator=g) * (0.5 + torch.rand((1, 1, 64), generator=g)) + 0.5 * torch.randn((1, 1, 64), generator=g)
    for b, c in enumerate(N_COUNTS):
        mem[b, c:] = 0.0
    return mem


def _net_step(net, mem, **kw):
    """One forward + backward -> the embedding the transformer received, predictions, every gradient, the encoder's buffers"""
    seen = []
    hook = net.transf.register_forward_pre_hook(lambda mod, args: seen.append(args[0].detach().clone()))
    try:
        preds = net(mem, None, **kw)
    finally:
        hook.remove()
    loss = sum((p * torch.arange(1, p.numel() + 1, dtype=p.dtype, device=p.device).view_as(p)).sum() for p in preds.values())
    net.zero_grad()
    loss.backward()
    out = {"emb": seen[0]}
    for k, p in preds.items():
        out["prediction " + k] = p.detach()
    for n, p in net.named_parameters():
        out["grad " + n] = p.grad.clone()
    for n, bf in net.encoder.named_buffers():
        out["buffer " + n] = bf.clone()
    return out


def _err(t, ref):
    ref = ref.double().cpu()
    return float((t.double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def test_net_fused_route_against_the_generic_route_and_float64(monkeypatch):
    """Train mode, dropout off: ``net(mem, None, mem_count=, mask_encoder=True)`` on the fused route, on the generic route
    (``IPSX_TRAIN_PROJECTOR=0``: ATen gather + the stock modules) and as float64 autograd of the definition on the CPU.  The
    yardstick and the ReLU rule of tests/test_train_projector.py: per tensor the fused error is at most 4 x the generic
    route's; a seed on which either float32 route has an activation on the other side of zero than float64 is held on
    embeddings, predictions and buffers only, and one seed of at most ten must be free of such flips."""
    conf = _conf()
    clean = 0
    for seed in range(10):
        net = synth.fill_weights(IPSNet(torch.device(DEV), conf), 7 + seed).to(DEV).train()
        generic = copy.deepcopy(net)
        ref = IPSNet(torch.device("cpu"), conf)
        ref.load_state_dict({k: v.cpu() for k, v in net.state_dict().items()})
        ref = ref.double().train()
        mem = _mem(20 + seed)
        calls = []
        real = fused_projector.encode
        monkeypatch.setattr(fused_projector, "encode", lambda enc, x, rows=None: (calls.append(rows), real(enc, x, rows=rows))[1])
        a = _net_step(net, mem.to(DEV), mem_count=N_COUNTS, mask_encoder=True)
        assert len(calls) == 1 and calls[0] is not None and calls[0].numel() == 270          # (the indexed node ran)
        monkeypatch.setenv("IPSX_TRAIN_PROJECTOR", "0")
        s = _net_step(generic, mem.to(DEV), mem_count=N_COUNTS, mask_encoder=True)
        assert len(calls) == 1
        monkeypatch.undo()
        r = _net_step(ref, mem.double(), mem_count=N_COUNTS, mask_encoder=True)
        pad = torch.ones((N_B, N_M), dtype=torch.bool)
        for b, c in enumerate(N_COUNTS):
            pad[b, :c] = False
        for out in (a, s, r):
            e = out["emb"].cpu()[pad]
            assert torch.equal(e, torch.zeros_like(e)) and not bool(torch.signbit(e).any())
        assert int(a["buffer 2.num_batches_tracked"]) == int(s["buffer 2.num_batches_tracked"]) == int(r["buffer 2.num_batches_tracked"]) == 1
        flips_a = int(((a["emb"].cpu() > 0) != (r["emb"] > 0)).sum())
        flips_s = int(((s["emb"].cpu() > 0) != (r["emb"] > 0)).sum())
        print("seed %d, ReLU flips against float64: fused %d, generic %d" % (seed, flips_a, flips_s))
        assert flips_a <= 8 and flips_s <= 8
        bad = []
        for k in r:
            if k.endswith("num_batches_tracked"):
                continue
            if (flips_a or flips_s) and not k.startswith(("emb", "prediction", "buffer")):
                continue
            ef, es = _err(a[k], r[k]), _err(s[k], r[k])
            print("%-44s fused %.3e   generic %.3e" % (k, ef, es))
            if not ef <= 4.0 * es:
                bad.append((k, ef, es))
        assert not bad, bad
        if not (flips_a or flips_s):
            clean += 1
            break
    assert clean == 1


def test_net_full_counts_are_the_unmasked_call():
    conf = _conf()
    net = synth.fill_weights(IPSNet(torch.device(DEV), conf), 7).to(DEV).train()
    other = copy.deepcopy(net)
    mem = torch.randn((N_B, N_M, 64), generator=torch.Generator().manual_seed(3)).to(DEV)
    a = _net_step(net, mem, mem_count=(N_M,) * N_B, mask_encoder=True)
    b = _net_step(other, mem, mem_count=(N_M,) * N_B, mask_encoder=False)
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_net_eval_mode_keeps_the_bits_of_todays_pass():
    """Eval mode, no grad (the eval projector's kernels; rows are independent): the filled rows' embeddings are the bits of the
    pass over all B * M rows, the padding slots exactly +0.0 instead of the blank row's embedding, no buffer moves."""
    conf = _conf()
    net = synth.fill_weights(IPSNet(torch.device(DEV), conf), 7).to(DEV).eval()
    mem = _mem(4).to(DEV)
    before = {n: b.clone() for n, b in net.encoder.named_buffers()}
    seen = []
    hook = net.transf.register_forward_pre_hook(lambda mod, args: seen.append(args[0].detach().clone()))
    with torch.no_grad():
        masked_preds = net(mem, None, mem_count=N_COUNTS, mask_encoder=True)
        plain_preds = net(mem, None, mem_count=N_COUNTS)
    hook.remove()
    masked, plain = seen[0].view(N_B, N_M, -1), seen[1].view(N_B, N_M, -1)
    for b, c in enumerate(N_COUNTS):
        assert torch.equal(masked[b, :c], plain[b, :c]), b
        assert torch.equal(masked[b, c:], torch.zeros_like(masked[b, c:])) and not bool(torch.signbit(masked[b, c:]).any()), b
        if c < N_M:
            assert bool((plain[b, c:] != 0).any()), b
    for k in plain_preds:                                    # (the masked aggregator never reads the padding)
        assert torch.equal(masked_preds[k], plain_preds[k]), k
    for n, buf in net.encoder.named_buffers():
        assert torch.equal(buf, before[n]), n


def test_step_after_a_padded_selection_sees_the_filled_rows_only():
    """ips_ragged(pad=True) on slides of 3, 8 and 20 rows at M = 8, then a training-mode step with the count it left: the
    BatchNorm's running mean is the one the encoder leaves on the 3 + 8 + 8 filled rows alone."""
    conf = synth.camelyon_conf(N=32, M=8, I=8, D=64, D_k=8, D_v=8, D_inner=128, n_chan_in=64, B=3, attn_dropout=0.0, dropout=0.0)
    net = synth.fill_weights(IPSNet(torch.device(DEV), conf), 7).to(DEV).train()
    padded = synth.fill_weights(IPSNet(torch.device(DEV), conf), 7).to(DEV).train()
    g = torch.Generator().manual_seed(5)
    slides = [torch.randn((n, 64), generator=g).to(DEV) for n in (3, 8, 20)]
    mem_patch, mem_pos = net.ips_ragged(slides, pad=True)
    assert net.last_mem_count == (3, 8, 8)
    alone = copy.deepcopy(net.encoder)
    rows = _rows(net.last_mem_count, 8)
    fused_projector.encode(alone, mem_patch.reshape(-1, 64)[rows.long()].contiguous())
    preds = net(mem_patch, mem_pos, mem_count=net.last_mem_count, mask_encoder=True)
    sum(p.sum() for p in preds.values()).backward()
    assert torch.equal(net.encoder[2].running_mean, alone[2].running_mean)
    assert torch.equal(net.encoder[2].running_var, alone[2].running_var)
    assert int(net.encoder[2].num_batches_tracked) == 1
    padded(mem_patch, mem_pos, mem_count=net.last_mem_count)                # (without the flag the 5 blank rows take part)
    assert not torch.equal(padded.encoder[2].running_mean, alone[2].running_mean)


# ---------------------------------------------------------------- the wrappers' refusals
class _NoLaunch:
    """libipsx with every export but the ``_supported`` queries failing the test"""

    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        if name.endswith("_supported"):
            return getattr(self._real, name)
        pytest.fail("{} called behind an argument that had to be refused".format(name))


def test_wrappers_refuse_a_bad_index_before_any_launch(monkeypatch):
    x, w, b = _inputs(64, 32, 32, seed=1)
    good = torch.arange(0, 64, 2, dtype=torch.int32)
    z, stats, _, _, _ = hip.projector_train_forward(x, w, b, LN_EPS, index=good)          # (a host-built index is taken)
    assert z.shape == (32, 32)
    dz = torch.randn((32, 32), device=DEV)
    real = hip.lib()
    monkeypatch.setattr(hip_train, "lib", lambda: _NoLaunch(real))
    monkeypatch.setattr(hip_train, "_pack_conv", lambda *a, **k: pytest.fail("a packing launch"))
    bad = {
        "float": good.float(),
        "int64": good.long().to(DEV),
        "2-d": good.view(4, 8).to(DEV),
        "empty": good[:0].to(DEV),
        "host entry = src_rows": torch.tensor([0, 64], dtype=torch.int32),
        "host entry < 0": torch.tensor([-1, 3], dtype=torch.int32),
    }
    for name, index in bad.items():
        with pytest.raises((TypeError, ValueError)):
            hip.projector_train_forward(x, w, b, LN_EPS, index=index)
        with pytest.raises((TypeError, ValueError)):
            hip.projector_wgrad(x, dz[:max(index.numel(), 1)].contiguous(), stats[:max(index.numel(), 1)].contiguous(), index=index)
    with pytest.raises(ValueError):                           # statistics and dz are packed: as many rows as the index
        hip.projector_wgrad(x, dz[:16].contiguous(), stats[:16].contiguous(), index=good.to(DEV))
