"""The masked attention pool of the training step (csrc/attn_pool_train.hip, the COUNTED instantiations behind
ipsx_attn_pool_forward_counted / ipsx_attn_pool_backward_counted).

The mask is a row BOUND: image b's kernels run over its first count[b] rows where the unmasked ones run over M.  The
unmasked kernels' trees of additions depend on the row count alone (header comment of attn_pool_train.hip), so Z[b],
P[b, :, :count[b]] and dx[b, :count[b]] must have the BITS of the unmasked node on x[b:b + 1, :count[b]] - which holds the
implementation to a bound and rules out a zero weight multiplied in.  dA is a sum over the batch in (b, chunk) order that
no solo call has; it is held to float64 autograd of ``aten_pool(count=)`` under the yardstick of
tests/test_train_aggregator.py: err = max |t - t64| / max |t64|, fused at most 4 x the float32 ATen evaluation's.

Counts from {1, 31, 32, 33, 127, 128, 129, 256, 257, 300} clipped to M: the 32-row wave tile, the 128-row chunk and the
256-thread softmax stride, each from both sides.  D = 128 takes the GPW = 1 kernels, D = 640 the GPW = 2 ones."""

import copy

import pytest
import torch

from ips_amd import hip, synth
from ips_amd.architecture import IPSNet
from ips_amd.training import fused_aggregator

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("Z", "P", "dx", "dA")

# B, M, D, R, counts
CASES = [
    (6, 300, 128, 8, (1, 31, 32, 33, 127, 128)),
    (6, 300, 128, 8, (129, 256, 257, 300, 1, 32)),
    (3, 300, 640, 4, (33, 129, 257)),
    (3, 300, 640, 4, (128, 256, 300)),
    (2, 40, 64, 32, (31, 40)),          # (127 .. 300 clip to M = 40)
    (2, 40, 64, 32, (32, 33)),
    (2, 40, 64, 1, (1, 40)),
    (2, 40, 64, 1, (33, 32)),
]
IDS = ["B%d-M%d-D%d-R%d-%s" % (c[0], c[1], c[2], c[3], "_".join(map(str, c[4]))) for c in CASES]


def _err(t, ref):
    ref = ref.double()
    return float((t.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def _inputs(B, M, D, R, seed, logit_std=2.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn((B, M, D), generator=g)
    A = torch.randn((R, D), generator=g) * (logit_std / D ** 0.5)
    dZ = torch.randn((B, R, D), generator=g)
    return x.to(DEV), A.to(DEV), dZ.to(DEV)


def _keep(B, R, M, counts, p=0.1, seed=0):
    """Attention-dropout factors from the first seed that leaves no (b, r) row fully dropped WITHIN its count."""
    within = torch.arange(M)[None, None, :] < torch.tensor(counts)[:, None, None]
    for s in range(seed, seed + 1000):
        g = torch.Generator(device="cpu").manual_seed(1000 + s)
        keep = (torch.rand((B, R, M), generator=g) >= p).float() / (1.0 - p)
        if bool(((keep * within).sum(-1) > 0).all()):
            return keep.to(DEV)
    raise AssertionError("no seed keeps every row")


def _fused(x, A, keep, dZ, count=None):
    Z, P = hip.attn_pool_forward(x, A, keep, count)
    dx, dA = hip.attn_pool_backward(x, A, keep, P, Z, dZ, count=count)
    return Z, P, dx, dA


def _formulas(x, A, keep, dZ, counts, dtype):
    """Z, dx, dA by autograd of ``aten_pool(count=)`` in ``dtype``"""
    xt, At = x.to(dtype).clone().requires_grad_(), A.to(dtype).clone().requires_grad_()
    Z = fused_aggregator.aten_pool(xt, At, None if keep is None else keep.to(dtype), counts)
    Z.backward(dZ.to(dtype))
    return Z.detach(), xt.grad, At.grad


@pytest.mark.parametrize("dropped", [False, True], ids=["", "keep"])
@pytest.mark.parametrize("B,M,D,R,counts", CASES, ids=IDS)
def test_counted_kernels(B, M, D, R, counts, dropped):
    """Per image the bits of the unmasked node on the filled rows; exact zeros beyond; dA against float64; and the same
    bits again with 1e30 in every padded row of x (finite, every product with it overflows).
    Measured on an MI355X: see the printed dA errors (fused | float32 ATen)."""
    assert len(counts) == B and all(1 <= c <= M for c in counts)
    x, A, dZ = _inputs(B, M, D, R, seed=M + D + R)
    for b, c in enumerate(counts):
        x[b, c:] = 0.0                                   # what pad=True writes
    keep = _keep(B, R, M, counts) if dropped else None
    Z, P, dx, dA = got = _fused(x, A, keep, dZ, counts)
    assert all(bool(torch.isfinite(t).all()) for t in got)
    for b, c in enumerate(counts):
        kb = keep[b:b + 1, :, :c].contiguous() if dropped else None
        sZ, sP, sdx, _ = _fused(x[b:b + 1, :c].contiguous(), A, kb, dZ[b:b + 1].contiguous())
        # (torch.equal compares values: a -0.0 sum that a trailing zero block turned into +0.0 is equal)
        assert torch.equal(Z[b], sZ[0]), ("Z", b, c)
        assert torch.equal(P[b, :, :c], sP[0]), ("P", b, c)
        assert torch.equal(dx[b, :c], sdx[0]), ("dx", b, c)
        assert torch.equal(P[b, :, c:], torch.zeros((R, M - c), device=DEV)), ("P beyond", b, c)
        assert not bool(torch.signbit(P[b, :, c:]).any())
        assert torch.equal(dx[b, c:], torch.zeros((M - c, D), device=DEV)), ("dx beyond", b, c)
    r64 = _formulas(x, A, keep, dZ, counts, torch.float64)
    r32 = _formulas(x, A, keep, dZ, counts, torch.float32)
    ef, es = _err(dA, r64[2]), _err(r32[2], r64[2])
    print("dA %s%s   fused %.3e   float32 ATen %.3e" % ((B, M, D, R, counts), " keep" if dropped else "", ef, es))
    print("Z  fused %.3e | %.3e   dx fused %.3e | %.3e" % (_err(Z, r64[0]), _err(r32[0], r64[0]), _err(dx, r64[1]), _err(r32[1], r64[1])))
    assert float(r64[2].abs().max()) > 0.0
    assert ef <= 4.0 * es
    # garbage in the padding
    y = x.clone()
    for b, c in enumerate(counts):
        y[b, c:] = 1e30 * (1.0 - 2.0 * (torch.arange(M - c, device=DEV)[:, None] % 2))
    gZ, gP, gdx, gdA = _fused(y, A, keep, dZ, counts)
    assert torch.equal(gZ, Z) and torch.equal(gP, P) and torch.equal(gdA, dA)
    for b, c in enumerate(counts):
        assert torch.equal(gdx[b, :c], dx[b, :c]), ("dx with garbage", b, c)
        assert torch.equal(gdx[b, c:], torch.zeros((M - c, D), device=DEV)), ("dx beyond, garbage", b, c)


@pytest.mark.parametrize("dropped", [False, True], ids=["", "keep"])
@pytest.mark.parametrize("B,M,D,R", [(6, 300, 128, 8), (3, 300, 640, 4), (2, 40, 64, 32), (2, 40, 64, 1)])
def test_full_counts_are_the_unmasked_node(B, M, D, R, dropped):
    x, A, dZ = _inputs(B, M, D, R, seed=7)
    keep = _keep(B, R, M, (M,) * B) if dropped else None
    plain = _fused(x, A, keep, dZ)
    for count in ((M,) * B, torch.full((B,), M, device=DEV), torch.full((B,), M, dtype=torch.int32)):
        for name, u, v in zip(NAMES, _fused(x, A, keep, dZ, count), plain):
            assert torch.equal(u, v), name


def test_without_dx():
    B, M, D, R, counts = 3, 300, 128, 8, (5, 130, 300)
    x, A, dZ = _inputs(B, M, D, R, seed=8)
    Z, P = hip.attn_pool_forward(x, A, None, counts)
    dx, dA = hip.attn_pool_backward(x, A, None, P, Z, dZ, want_dx=False, count=counts)
    assert dx is None and torch.equal(dA, hip.attn_pool_backward(x, A, None, P, Z, dZ, count=counts)[1])


def test_wrapper_refusals():
    B, M, D, R = 2, 40, 64, 8
    x, A, dZ = _inputs(B, M, D, R, seed=9)
    Z, P = hip.attn_pool_forward(x, A)
    for bad in ((1,), (1, 2, 3), (0, 5), (5, M + 1), torch.tensor([1, 2, 3], device=DEV), torch.tensor([[1, 2]], device=DEV)):
        with pytest.raises(ValueError):
            hip.attn_pool_forward(x, A, None, bad)
        with pytest.raises(ValueError):
            hip.attn_pool_backward(x, A, None, P, Z, dZ, count=bad)
    with pytest.raises(TypeError):
        hip.attn_pool_forward(x, A, None, torch.tensor([1.0, 2.0], device=DEV))
    L = hip.lib()          # the C entry points refuse a null count
    assert L.ipsx_attn_pool_forward_counted(None, None, None, None, B, M, R, D, None, None, None, 0, None) != 0
    assert L.ipsx_attn_pool_backward_counted(None, None, None, None, None, None, None, B, M, R, D, None, None, None, 0, None) != 0


def _node(transf, x, w, count, fused):
    xr = x.clone().requires_grad_()
    if fused:
        out = fused_aggregator.forward(transf, xr, count=count)
    else:
        out = transf.mlp(transf.crs_attn(xr, count))          # the stock modules with the ATen mask
    transf.zero_grad()
    ((out * w.to(out.dtype)).sum() + 0.1 * out.sum(1).sin().sum()).backward()
    res = {"out": out.detach(), "x.grad": xr.grad.clone()}
    for n, p in transf.named_parameters():
        res["grad " + n] = p.grad.clone()
    return res


@pytest.mark.parametrize("conf,B,M,counts", [(synth.camelyon_conf(N=64, M=8, I=8), 3, 300, (40, 300, 129)),
                                             (synth.mnist_conf(N=64, M=8, I=8), 3, 100, (1, 100, 33))], ids=["cam", "mnist"])
def test_whole_node_against_the_stock_modules(conf, B, M, counts):
    """fused_aggregator.forward(transf, x, count=) and Transformer.forward under autograd against the stock float32 modules
    with the ATen mask, both against a float64 copy: output and every parameter's gradient, fused <= 4 x stock.
    x.grad as well, and exactly zero beyond the counts."""
    a = synth.fill_weights(IPSNet(torch.device(DEV), conf), 11).to(DEV).transf.eval()
    s, r = copy.deepcopy(a), copy.deepcopy(a).double()
    g = torch.Generator(device="cpu").manual_seed(12)
    x = torch.randn((B, M, conf.D), generator=g).to(DEV)
    for b, c in enumerate(counts):
        x[b, c:] = 0.0
    w = torch.randn((B, conf.n_token, conf.D), generator=g).to(DEV)
    count = torch.tensor(counts, device=DEV)
    fa, fs, fr = _node(a, x, w, count, True), _node(s, x, w, count, False), _node(r, x.double(), w.double(), count, False)
    bad = []
    for k in fr:
        ef, es = _err(fa[k], fr[k]), _err(fs[k], fr[k])
        print("%-34s fused %.3e   stock %.3e" % (k, ef, es))
        if not ef <= 4.0 * es:
            bad.append((k, ef, es))
    assert not bad, bad
    for b, c in enumerate(counts):
        assert torch.equal(fa["x.grad"][b, c:], torch.zeros((M - c, conf.D), device=DEV))
    # the module's own route under autograd is this node
    xr = x.clone().requires_grad_()
    assert torch.equal(a(xr, count=counts).detach(), fa["out"])
