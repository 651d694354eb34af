"""The with-grad cross-attention aggregator of the training step on libipsx's kernels (csrc/attn_pool_train.hip,
training/fused_aggregator.py) against float64 autograd of the same formulas and of the stock modules.

The yardstick throughout is tests/test_train_projector.py's: per tensor, err(t) = max |t - t64| / max |t64|, and the fused
path's error must be at most 4 x the error of the stock float32 ATen path on the same inputs.  Both errors are printed."""

import copy

import numpy as np
import pytest
import torch
from torch import nn

from ips_amd import hip, synth
from ips_amd.architecture import IPSNet
from ips_amd.training import fused_aggregator
from oracle import oracle as orc
from util import Golden, ulp_diff

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _err(t, ref):
    ref = ref.double()
    return float((t.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def _check(name, fused, stock, ref, log):
    ef, es = _err(fused, ref), _err(stock, ref)
    print("%-34s fused %.3e   stock %.3e" % (name, ef, es))
    log.append((name, ef, es))


def _assert_log(log):
    bad = [(n, ef, es) for n, ef, es in log if not ef <= 4.0 * es]
    assert not bad, bad


def _inputs(B, M, D, R, seed, logit_std=2.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn((B, M, D), generator=g)
    A = torch.randn((R, D), generator=g) * (logit_std / D ** 0.5)
    dZ = torch.randn((B, R, D), generator=g)
    return x.to(DEV), A.to(DEV), dZ.to(DEV)


def _keep(B, R, M, p=0.1, seed=0):
    """Attention-dropout factors from the first seed that leaves no (b, r) row fully dropped."""
    for s in range(seed, seed + 100):
        g = torch.Generator(device="cpu").manual_seed(1000 + s)
        keep = (torch.rand((B, R, M), generator=g) >= p).float() / (1.0 - p)
        if bool((keep.sum(-1) > 0).all()):
            return keep.to(DEV)
    raise AssertionError("no seed keeps every row")


def _formulas(x, A, keep, dZ, dtype):
    """Z, P, dx, dA by autograd of the formulas in ATen ops in ``dtype``"""
    xt, At = x.to(dtype).clone().requires_grad_(), A.to(dtype).clone().requires_grad_()
    P = torch.softmax(torch.matmul(xt, At.t()), dim=1).transpose(1, 2)
    Pk = P if keep is None else P * keep.to(dtype)
    Z = torch.matmul(Pk, xt)
    Z.backward(dZ.to(dtype))
    return Z.detach(), P.detach(), xt.grad, At.grad


def _fused(x, A, keep, dZ):
    Z, P = hip.attn_pool_forward(x, A, keep)
    dx, dA = hip.attn_pool_backward(x, A, keep, P, Z, dZ)
    return Z, P, dx, dA


NAMES = ("Z", "P", "dx", "dA")
SHAPES = [(2, 10, 512, 8, 1), (3, 100, 128, 8, 4), (2, 5000, 512, 8, 1), (1, 1, 64, 1, 1), (2, 333, 96, 4, 3), (1, 4097, 256, 8, 4)]


@pytest.mark.parametrize("dropped", [False, True])
@pytest.mark.parametrize("B,M,D,H,T", SHAPES)
def test_kernels_against_float64(B, M, D, H, T, dropped):
    """Z, P, dx, dA of attn_pool_forward / attn_pool_backward against float64 autograd of the formulas, the float32 ATen
    evaluation of the same formulas as the second column; without keep and with a seeded keep of p = 0.1.
    Measured on an MI355X, fused | stock error (keep absent):
      (2, 10, 512, 8, 1)    Z 2.1e-7 | 3.2e-7, P 2.5e-7 | 2.9e-7, dx 3.7e-7 | 3.9e-7, dA 4.1e-7 | 3.1e-7
      (3, 100, 128, 8, 4)   Z 3.7e-7 | 8.5e-7, P 2.0e-7 | 6.8e-7, dx 5.3e-7 | 7.4e-7, dA 4.5e-7 | 1.3e-6
      (2, 5000, 512, 8, 1)  Z 4.7e-7 | 7.7e-7, P 5.6e-7 | 5.2e-7, dx 7.4e-7 | 8.6e-7, dA 9.3e-7 | 1.8e-6
    (with keep the same within 30 %; one patch: every tensor exact without keep, dA 2.2e-6 absolute with keep.  With ONE
    accumulation chain over D the kernels measured 3 - 9 x the stock error at D = 512 and missed this bound: ap_dot_tile.)"""
    R = H * T
    x, A, dZ = _inputs(B, M, D, R, seed=M + D)
    keep = _keep(B, R, M) if dropped else None
    if dropped:
        assert bool((keep.sum(-1) > 0).all())
    got = _fused(x, A, keep, dZ)
    stock = _formulas(x, A, keep, dZ, torch.float32)
    ref = _formulas(x, A, keep, dZ, torch.float64)
    log = []
    for name, a, s, r in zip(NAMES, got, stock, ref):
        assert a.shape == r.shape and bool(torch.isfinite(a).all())
        _check("%s %s%s" % (name, (B, M, D, H, T), " keep" if dropped else ""), a, s, r, log)
    if M == 1 and not dropped:
        assert torch.equal(got[0], x.expand(B, R, D)) and torch.equal(got[1], torch.ones_like(got[1]))
    # One patch: dL = P (keep dP' - c) is zero in exact arithmetic, so the float64 dA is identically zero and the relative
    # yardstick has no denominator.  Such a tensor is held to the rounding of the terms that cancel: two float32 dot
    # products of length D (at most D 2^-24 of sum |dZ x| each, Higham's gamma_D), times P <= keep, times |x|.
    zero_ref = [k for k, r in enumerate(ref) if float(r.abs().max()) == 0.0]
    assert zero_ref == ([3] if M == 1 else [])
    for k in zero_ref:
        kmax = 1.0 if keep is None else float(keep.max())
        bound = 4.0 * D * 2.0 ** -24 * kmax * float((dZ.double().abs() * x.double().abs()).sum(-1).max()) * float(x.abs().max())
        print("%s: float64 is zero; |fused| %.3e, |stock| %.3e, bound %.3e" % (NAMES[k], float(got[k].abs().max()),
                                                                              float(stock[k].abs().max()), bound))
        assert float(got[k].abs().max()) <= bound
    _assert_log([e for k, e in enumerate(log) if k not in zero_ref])


def test_keep():
    """keep = None and keep = ones give equal bits; a keep that zeroes patch m0 in every row gives Z of the float64 softmax
    with that patch's weight removed, and dx[:, m0] = sum_r dL[b, m0, r] A[r]: the patch still shapes the denominator.
    Measured on an MI355X, fused | stock error: Z 2.9e-7 | 9.3e-7, dx[:, m0] 7.6e-7 | 1.1e-6."""
    B, M, D, R, m0 = 2, 333, 96, 12, 130
    x, A, dZ = _inputs(B, M, D, R, seed=21)
    ones = torch.ones((B, R, M), device=DEV)
    for u, v in zip(_fused(x, A, None, dZ), _fused(x, A, ones, dZ)):
        assert torch.equal(u, v)
    keep = ones.clone()
    keep[:, :, m0] = 0.0
    got = _fused(x, A, keep, dZ)
    stock = _formulas(x, A, keep, dZ, torch.float32)
    x64, A64, dZ64 = x.double(), A.double(), dZ.double()
    P64 = torch.softmax(torch.matmul(x64, A64.t()), dim=1).transpose(1, 2)           # the FULL softmax
    Pcut = P64.clone()
    Pcut[:, :, m0] = 0.0
    Z64 = torch.matmul(Pcut, x64)
    c = (dZ64 * Z64).sum(-1)                                                          # (B, R)
    dL_m0 = P64[:, :, m0] * (0.0 - c)                                                 # keep = 0 there
    dx_m0 = torch.matmul(dL_m0, A64)                                                  # (B, D)
    log = []
    _check("Z, patch m0 dropped", got[0], stock[0], Z64, log)
    _check("dx[:, m0]", got[2][:, m0], stock[2][:, m0], dx_m0, log)
    _assert_log(log)
    assert float(got[2][:, m0].abs().max()) > 0.0


def test_range():
    """Logits up to +-1e4, and a slide of identical patches (uniform softmax): finite, within the yardstick; for the
    identical patches P within 2 ulp of 1 / M and Z within 1e-6 relative of x[b, 0].  (M = 100, the shipped Megapixel-MNIST
    memory: Z is a float32 chain over the patches, whose rounding grows with sqrt(M) * 2^-24.)
    Measured on an MI355X, fused | stock error: logits to 1e4: Z 0 | 0, P 1.1e-24 | 5.1e-25, dx 5.3e-8 |
    5.3e-8, dA 6.7e-4 | 3.1e-4; identical patches: Z 6.4e-7 | 1.1e-6 (the stock chain over 100 equal terms is past 1e-6), P 0 ulp,
    dx 9.0e-7 | 3.5e-7, |dA| 3.6e-5 | 6.8e-6 against a bound of 8.5e-3."""
    B, M, D, R = 2, 333, 128, 8
    x, A, dZ = _inputs(B, M, D, R, seed=31)
    top = float(torch.matmul(x.double(), A.double().t()).abs().max())
    x = x * (1e4 / top)
    assert 0.99e4 < float(torch.matmul(x.double(), A.double().t()).abs().max()) < 1.01e4
    got = _fused(x, A, None, dZ)
    stock, ref = _formulas(x, A, None, dZ, torch.float32), _formulas(x, A, None, dZ, torch.float64)
    log = []
    for name, a, s, r in zip(NAMES, got, stock, ref):
        assert bool(torch.isfinite(a).all())
        _check("%s, logits to 1e4" % name, a, s, r, log)
    B, M, D, R = 2, 100, 128, 32
    x, A, dZ = _inputs(B, M, D, R, seed=32)
    x = x[:, :1].expand(B, M, D).contiguous()
    got = _fused(x, A, None, dZ)
    stock, ref = _formulas(x, A, None, dZ, torch.float32), _formulas(x, A, None, dZ, torch.float64)
    for name, a, s, r in zip(NAMES, got, stock, ref):
        assert bool(torch.isfinite(a).all())
        if name == "dA":
            # every patch the same: dP' = c, so dA is zero in exact arithmetic (float64 returns ~1e-16 of the terms' scale) and
            # the relative yardstick compares two roundings of nothing.  Held, as for one patch, to the rounding of the two
            # float32 dot products of length D that cancel (D 2^-24 of sum |dZ x| each), the weights P summing to 1, times |x|.
            bound = 4.0 * D * 2.0 ** -24 * float((dZ.double().abs() * x[:, :1].double().abs()).sum(-1).max()) * float(x.abs().max())
            print("dA, identical patches: |float64| %.3e, |fused| %.3e, |stock| %.3e, bound %.3e" % (
                float(r.abs().max()), float(a.abs().max()), float(s.abs().max()), bound))
            assert float(r.abs().max()) < 1e-12 and float(a.abs().max()) <= bound
            continue
        _check("%s, identical patches" % name, a, s, r, log)
    ulps = ulp_diff(got[1].cpu().numpy(), np.full((B, R, M), np.float32(1.0) / np.float32(M), dtype=np.float32))
    zrel = _err(got[0], x[:, :1].expand(B, R, D))
    print("identical patches: P %d ulp from 1 / M, Z %.3e from x[b, 0]" % (ulps, zrel))
    assert ulps <= 2 and zrel <= 1e-6
    _assert_log(log)


def test_determinism_and_batch_independence():
    """Two calls give equal bits; Z, P, dx of an image in a batch of 3 equal those computed for it alone, bit for bit; dA of
    the batch equals the float64 sum of the per-image dA.  Measured on an MI355X, fused | stock error: 9.7e-8 | 1.2e-6 and 1.6e-7 | 1.2e-6."""
    for B, M, D, R in ((3, 333, 96, 12), (3, 1300, 512, 8)):
        x, A, dZ = _inputs(B, M, D, R, seed=41)
        keep = _keep(B, R, M)
        one, two = _fused(x, A, keep, dZ), _fused(x, A, keep, dZ)
        for u, v in zip(one, two):
            assert torch.equal(u, v)
        total = torch.zeros((R, D), dtype=torch.float64, device=DEV)
        for b in range(B):
            alone = _fused(x[b:b + 1].contiguous(), A, keep[b:b + 1].contiguous(), dZ[b:b + 1].contiguous())
            for k in range(3):
                assert torch.equal(alone[k][0], one[k][b]), (NAMES[k], b)
            total += alone[3].double()
        stock, ref = _formulas(x, A, keep, dZ, torch.float32), _formulas(x, A, keep, dZ, torch.float64)
        ef, es = _err(one[3], total), _err(stock[3], ref[3])
        print("dA of the batch against the per-image sum %.3e   stock against float64 %.3e" % (ef, es))
        assert ef <= 4.0 * es


def _transf(conf, seed):
    net = synth.fill_weights(IPSNet(torch.device(DEV), conf), seed).to(DEV)
    return net.transf.eval()


def _node_step(transf, x, w, fused):
    opt = torch.optim.AdamW(transf.parameters(), lr=1e-3, weight_decay=0.1)
    xr = x.clone().requires_grad_()
    out = transf(xr) if fused else transf.mlp(transf.crs_attn(xr))
    # (x 100: AdamW's first step is lr g / (|g| + 1e-8) - gradients near 1e-8 would turn their rounding into the step's sign)
    loss = 100.0 * ((out * w.to(out.dtype)).sum() + 0.1 * out.sum(1).sin().sum())
    opt.zero_grad()
    loss.backward()
    res = {"out": out.detach(), "x.grad": xr.grad.clone()}
    for n, p in transf.named_parameters():
        res["grad " + n] = p.grad.clone()
    opt.step()
    for n, p in transf.named_parameters():
        res["stepped " + n] = p.detach().clone()
    return res


@pytest.mark.parametrize("conf,B,M", [(synth.camelyon_conf(N=64, M=8, I=8), 2, 300), (synth.mnist_conf(N=64, M=8, I=8), 3, 100)])
def test_whole_node_against_the_stock_modules(conf, B, M, monkeypatch):
    """Transformer.forward under autograd (dropout off) at the CAMELYON / traffic-sign and the Megapixel-MNIST module sizes:
    output, x.grad, every parameter's gradient and the parameters after one AdamW step against a float64 copy, the stock
    float32 modules as the yardstick.  Measured on an MI355X, worst fused / stock ratio: 2.0 (x.grad at the larger
    shape, 2.2e-6 | 1.6e-6 before the D contraction ran as eight chains)."""
    calls = _counting(monkeypatch)
    a = _transf(conf, 11)
    s, r = copy.deepcopy(a), copy.deepcopy(a).double()
    g = torch.Generator(device="cpu").manual_seed(12)
    x = torch.randn((B, M, conf.D), generator=g).to(DEV)
    w = torch.randn((B, conf.n_token, conf.D), generator=g).to(DEV)
    fa, fs, fr = _node_step(a, x, w, True), _node_step(s, x, w, False), _node_step(r, x.double(), w.double(), False)
    assert len(calls) == 1
    log = []
    for k in fr:
        _check(k, fa[k], fs[k], fr[k], log)
    _assert_log(log)


def test_dropout_on(monkeypatch):
    """transf.train() with p = 0.1: the fused route is taken, the output differs from the p = 0 output, the same seed gives
    the same bits, and the mean over 64 seeds is closer to the p = 0 output than any single seed's (1 / (1 - p) is there)."""
    calls = _counting(monkeypatch)
    transf = _transf(synth.mnist_conf(N=64, M=8, I=8), 13)
    x = torch.randn((2, 100, 128), generator=torch.Generator().manual_seed(14)).to(DEV).requires_grad_()
    base = transf(x).detach()
    assert len(calls) == 1
    transf.train()
    assert transf.crs_attn.attention.dropout.p == pytest.approx(0.1)
    outs = []
    for seed in range(64):
        torch.manual_seed(seed)
        outs.append(transf(x).detach())
    assert len(calls) == 65
    torch.manual_seed(5)
    again = transf(x)
    assert torch.equal(again.detach(), outs[5]) and not torch.equal(outs[5], base)
    again.sum().backward()
    assert bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0.0
    single = min(float((o - base).abs().max()) for o in outs)
    mean = float((torch.stack(outs).mean(0) - base).abs().max())
    print("distance to the p = 0 output: mean of 64 seeds %.3e, closest single seed %.3e" % (mean, single))
    assert mean < single


def _counting(monkeypatch):
    calls = []
    real = fused_aggregator.forward

    def counted(transf, x, keep=None, pool=None):
        calls.append(tuple(x.shape))
        return real(transf, x, keep, pool)
    monkeypatch.setattr(fused_aggregator, "forward", counted)
    return calls


@pytest.mark.parametrize("name", ["cam_small", "mnist_mini"])
def test_routing(name, monkeypatch):
    """net.train(); net(mem_patch, mem_pos) takes the fused aggregator - once - on a feature net and on an image net with
    positional encoding; not when switched off, without grad, in eval mode without grad or for a Transformer ``supported``
    refuses.  With the switch off Transformer.forward is the stock modules, bit for bit.  On the feature net the two
    routes' predictions are held against float64.  Measured on an MI355X, fused | stock error: 1.3e-8 | 1.3e-8."""
    g = Golden(name)
    net = g.net(DEV)
    x = g.patches().to(DEV)
    mem_patch, mem_pos = net.ips(x)
    assert torch.is_tensor(mem_pos) == (name == "mnist_mini")
    calls = _counting(monkeypatch)
    net.train()
    for m in (net.transf, net.output_layers):      # (dropout off: the two routes and float64 see the same function)
        m.eval()
    preds = net(mem_patch, mem_pos)
    assert len(calls) == 1 and calls[0] == (mem_patch.shape[0], mem_patch.shape[1], g.conf.D)
    assert all(p.requires_grad and bool(torch.isfinite(p).all()) for p in preds.values())
    monkeypatch.setenv("IPSX_TRAIN_AGGREGATOR", "0")
    stock = net(mem_patch, mem_pos)
    emb = torch.randn((2, 37, g.conf.D), device=DEV, requires_grad=True)
    assert torch.equal(net.transf(emb), net.transf.mlp(net.transf.crs_attn(emb)))
    assert len(calls) == 1
    monkeypatch.delenv("IPSX_TRAIN_AGGREGATOR")
    with torch.no_grad():
        net(mem_patch, mem_pos)
    assert len(calls) == 1
    net.eval()
    with torch.no_grad():
        net(mem_patch, mem_pos)
    assert len(calls) == 1
    if name == "cam_small":
        net64 = g.net(DEV).double().eval()
        net64.encoder.train()                      # the projector in batch-statistics mode, the rest in eval mode
        ref = net64(mem_patch.double(), mem_pos)
        log = []
        for k in ref:
            _check("prediction " + k, preds[k].detach(), stock[k].detach(), ref[k].detach(), log)
        _assert_log(log)
    other = IPSNet(torch.device(DEV), g.conf)
    ca = other.transf.crs_attn
    ca.k_w = nn.Linear(g.conf.D, ca.H * ca.D_k, bias=True)          # not what Transformer(...) builds
    other = other.to(DEV).train()
    assert not fused_aggregator.supported(other.transf)
    out = other(mem_patch, mem_pos)
    assert len(calls) == 1 and all(p.requires_grad for p in out.values())


def test_training_step_between_ips_calls():
    """ips() in train mode -> forward with grad (fused projector and aggregator) -> backward -> AdamW step -> ips() again:
    every parameter of the Transformer has a non-zero gradient, and the second selection equals the oracle's on the
    updated state dict."""
    g = Golden("cam_small")
    net = g.net(DEV)
    net.train()
    x = g.patches().to(DEV)
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3, weight_decay=0.1)
    mem_patch, mem_pos = net.ips(x)
    assert np.array_equal(net.last_mem_idx.cpu().numpy(), g.mem_idx)
    assert fused_aggregator.supported(net.transf) and fused_aggregator.enabled()
    preds = net(mem_patch, mem_pos)
    loss = sum((p ** 2).mean() for p in preds.values())
    opt.zero_grad()
    loss.backward()
    for n, p in net.transf.named_parameters():
        assert p.grad is not None and float(p.grad.abs().max()) > 0.0, n
    opt.step()
    net.ips(x)
    after = net.last_mem_idx.cpu().numpy()
    cpu = IPSNet(torch.device("cpu"), g.conf)
    cpu.load_state_dict({k: v.cpu() for k, v in net.state_dict().items()})
    cpu.eval()
    want = orc.Oracle(cpu).ips(g.patches().numpy(), None)
    assert np.array_equal(after, want["mem_idx"])


def _peak_delta(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def test_memory():
    """Peak memory of forward + backward at B = 4, M = 5000, D = 512, H = 8, D_k = D_v = 64, dropout off: below the stock
    path's by at least 0.9 x B M (H D_k + H D_v) 4 bytes - K and V, which no longer exist.
    Measured on an MI355X: fused 54.9 MB, stock 167.5 MB, K + V = 81.9 MB."""
    B, M = 4, 5000
    conf = synth.camelyon_conf(N=64, M=8, I=8)
    transf = _transf(conf, 15)
    x = torch.randn((B, M, conf.D), device=DEV).requires_grad_()
    gout = torch.randn((B, conf.n_token, conf.D), device=DEV)

    def run(fused, xs):
        def go():
            (transf(xs) if fused else transf.mlp(transf.crs_attn(xs))).backward(gout[:xs.shape[0]])
        return go
    small = x[:1, :64].detach().clone().requires_grad_()
    run(True, small)()                              # (first-use allocations of the library and the runtime)
    run(False, small)()
    transf.zero_grad(set_to_none=True)
    x.grad = None
    fused = _peak_delta(run(True, x))
    transf.zero_grad(set_to_none=True)
    x.grad = None
    stock = _peak_delta(run(False, x))
    kv = B * M * (conf.H * conf.D_k + conf.H * conf.D_v) * 4
    print("peak delta: fused %.1f MB, stock %.1f MB, K + V = %.1f MB" % (fused / 1e6, stock / 1e6, kv / 1e6))
    assert stock - fused >= 0.9 * kv


def test_captured_step(monkeypatch):
    """GraphedStep (conf.hip_graph) on the cam_small feature net captures the step with the fused aggregator in it and
    replays it twice: finite losses, and the parameters of the Transformer moved."""
    from ips_amd.training.graphed import GraphedStep
    g = Golden("cam_small")
    conf = g.conf.clone(B=g.B, B_seq=g.B, hip_graph=True)
    net = g.net(DEV)
    net.train()
    calls = _counting(monkeypatch)
    crit = {t['name']: (nn.NLLLoss() if t['act_fn'] == 'softmax' else nn.BCELoss()) for t in conf.tasks.values()}
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3, weight_decay=0.1)
    step = GraphedStep(net, crit, opt, conf)
    mem_patch, mem_pos = net.ips(g.patches().to(DEV))
    labels = {t['name']: torch.ones((g.B,), dtype=torch.int64, device=DEV) for t in conf.tasks.values()}
    before = {n: p.detach().clone() for n, p in net.transf.named_parameters()}
    losses = []
    for _ in range(2):
        loss, _ = step(mem_patch, mem_pos, labels)
        losses.append(float(loss))
    assert step.graph is not None and len(calls) == 4            # three warm-up steps and the capture
    assert all(np.isfinite(v) for v in losses), losses
    moved = [n for n, p in net.transf.named_parameters() if not torch.equal(p.detach(), before[n])]
    assert len(moved) == len(before), sorted(set(before) - set(moved))


def test_wrappers_raise_on_what_the_kernels_do_not_take():
    x, A, dZ = _inputs(2, 50, 64, 8, seed=1)
    Z, P = hip.attn_pool_forward(x, A)
    with pytest.raises(ValueError):
        hip.attn_pool_forward(x[:, :, :40].contiguous(), A[:, :40].contiguous())                   # D = 40
    with pytest.raises(ValueError):
        hip.attn_pool_forward(x, torch.randn((33, 64), device=DEV))                                # R = 33
    with pytest.raises(ValueError):
        hip.attn_pool_forward(x.double(), A)
    with pytest.raises(ValueError):
        hip.attn_pool_forward(x.transpose(0, 1), A)                                                # not contiguous
    with pytest.raises(ValueError):
        hip.attn_pool_forward(x, A, torch.ones((2, 8, 49), device=DEV))                            # keep of another M
    with pytest.raises(ValueError):
        hip.attn_pool_backward(x, A, None, P[:, :, :49].contiguous(), Z, dZ)                       # P of another shape
    assert not hip.attn_pool_supported(33, 64) and not hip.attn_pool_supported(8, 40) and hip.attn_pool_supported(32, 1024)
