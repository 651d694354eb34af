"""The with-grad cross-attention aggregator (csrc/attn_pool_train.hip, training/fused_aggregator.py) at the kernel paths and
seams tests/test_train_aggregator.py does not reach: the two-column-group kernels (D > 512, whole and partly live), one live
wavefront (D = 32) and partial ones, odd R and R = 1 with more than one patch, R = 32 across chunks, M around the 8-row trip,
the 32-row wavefront tile and the 128-row chunk, want_dx = False, poisoned neighbours, guarded outputs and workspace, and the
whole node at head layouts no configuration uses (D_k != D_v, odd H * T, H = 1, T > 4, an explicit keep, non-contiguous x).

The yardstick is that file's: per tensor, err(t) = max |t - t64| / max |t64| against float64 autograd of the same formulas,
and the fused error at most 4 x the error of the stock float32 ATen path on the same inputs.  At the tiny shapes of the
lattice the stock error can be 0 or a fraction of an ulp, so there each tensor kind is held to 4 x max(stock error of the
case, E_KIND[kind]), E_KIND the largest STOCK error of that kind over the lattice (a property of the ATen path, measured
once on an MI355X).  A dropped, doubled or misplaced row, column or r shows at 1 / M or 1 / R of the scale (>= 3e-3 at
M <= 300, 1 / 9 for a lost chunk at M = 1153): three orders of magnitude above either bound.  Both errors are printed."""

import copy

import pytest
import torch
from torch import nn

from ips_amd import hip
from ips_amd.architecture.transformer import Transformer
from ips_amd.training import fused_aggregator

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P_DROP = 0.1
NAMES = ("Z", "P", "dx", "dA")

# the largest stock float32 error per tensor kind over LATTICE x {no keep, keep}, measured on an MI355X (see the table in
# test_lattice_against_float64): Z at (3, 33, 544, 3) with keep, P at (2, 135, 512, 1), dx and dA at (2, 32, 640, 31) - all
# below 3e-6, the input scale of tests/test_train_aggregator.py kept
E_KIND = {"Z": 1.580e-6, "P": 1.850e-6, "dx": 1.868e-6, "dA": 2.240e-6}


def _err(t, ref):
    ref = ref.double()
    return float((t.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def _check(name, fused, stock, ref, log):
    ef, es = _err(fused, ref), _err(stock, ref)
    print("%-40s fused %.3e   stock %.3e" % (name, ef, es))
    log.append((name, ef, es))


def _assert_log(log, floor=0.0):
    bad = [(n, ef, es) for n, ef, es in log if not ef <= 4.0 * max(es, floor)]
    assert not bad, bad


def _worst(log):
    return max(ef / es if es > 0.0 else float("inf") for _, ef, es in log)


def _inputs(B, M, D, R, seed, logit_std=2.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn((B, M, D), generator=g)
    A = torch.randn((R, D), generator=g) * (logit_std / D ** 0.5)
    dZ = torch.randn((B, R, D), generator=g)
    return x.to(DEV), A.to(DEV), dZ.to(DEV)


def _keep(B, R, M):
    """Attention-dropout factors of p = 0.1 by rule, not by seed: keep[b, r, m] = 0 where (m + r + b) % 5 == 0.  Two
    neighbouring m are never both dropped, so no (b, r) row is empty from M = 2 on; one patch keeps its only weight."""
    b, r, m = torch.meshgrid(torch.arange(B), torch.arange(R), torch.arange(M), indexing="ij")
    keep = torch.full((B, R, M), 1.0 / (1.0 - P_DROP))
    if M >= 2:
        keep[(m + r + b) % 5 == 0] = 0.0
    assert bool((keep.sum(-1) > 0).all())
    assert M < 5 or bool((keep == 0).any())
    return keep.to(DEV)


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


# (B, M, D, R).  D: 32 one live wavefront with 8 lanes of columns, 96 / 160 a partial wavefront, 512 the one-group kernel
# full, 544 / 640 the two-group kernel with a partly live second group, 1024 the two-group kernel full.  R: 1, 2, odd (3, 31:
# ksteps reads one padded column of the LDS images), 32.  M: 1, 2, around the 8-row trip (7, 8, 9), the 32-row wavefront tile
# (31, 32, 33) and the 128-row chunk (127, 128, 129), 135 (a last chunk of 7 rows), 256 / 257, and 1153 = nine chunks and one
# row (the eight-at-a-time loop of attn_pool_sum_kernel and its tail).  Every value of every axis appears at least twice.
LATTICE = [
    (2, 257, 1024, 32), (2, 129, 544, 31), (2, 135, 640, 3), (2, 33, 32, 32), (1, 1153, 32, 1), (2, 128, 160, 2),
    (2, 127, 96, 31), (3, 9, 1024, 1), (2, 1153, 1024, 32),
    (2, 1, 512, 3), (3, 1, 32, 32), (3, 1, 1024, 31), (2, 2, 544, 32), (3, 2, 96, 1), (2, 7, 640, 2), (2, 7, 160, 31),
    (2, 8, 512, 32), (3, 8, 96, 3), (2, 9, 160, 2), (2, 31, 544, 1), (3, 31, 1024, 3), (2, 32, 640, 31), (2, 32, 512, 2),
    (3, 33, 544, 3), (2, 33, 640, 1), (2, 127, 1024, 2), (3, 128, 640, 32), (2, 128, 32, 3), (2, 129, 32, 31),
    (2, 135, 512, 1), (2, 256, 96, 32), (3, 256, 544, 31), (2, 257, 160, 3), (2, 257, 512, 31),
]


def test_the_lattice_covers_every_axis_value_twice():
    for axis, values in ((2, (32, 96, 160, 512, 544, 640, 1024)), (3, (1, 2, 3, 31, 32)),
                         (1, (1, 2, 7, 8, 9, 31, 32, 33, 127, 128, 129, 135, 256, 257, 1153))):
        seen = [case[axis] for case in LATTICE]
        assert set(seen) == set(values)
        assert all(seen.count(v) >= 2 for v in values), (axis, seen)
    assert len(set(LATTICE)) == len(LATTICE) and all(M <= 300 or M == 1153 for _, M, _, _ in LATTICE)


@pytest.mark.parametrize("dropped", [False, True])
@pytest.mark.parametrize("B,M,D,R", LATTICE)
def test_lattice_against_float64(B, M, D, R, dropped):
    """Z, P, dx, dA of attn_pool_forward / attn_pool_backward against float64 autograd of the formulas, the float32 ATen
    evaluation as the second column, without keep and with the keep of ``_keep``; each kind held to
    4 x max(stock error of the case, E_KIND[kind]).  dA of one patch is identically zero in float64 and is held to the
    absolute rounding bound tests/test_train_aggregator.py derives for that case.
    Measured on an MI355X, fused | stock error (keep absent; with keep the same within a factor 2):
      (2, 257, 1024, 32)   Z 7.0e-7 | 1.1e-6, P 6.4e-7 | 7.3e-7, dx 5.3e-7 | 6.6e-7, dA 4.6e-7 | 9.6e-7
      (2, 129, 544, 31)    Z 3.7e-7 | 5.3e-7, P 2.7e-7 | 3.7e-7, dx 4.7e-7 | 7.2e-7, dA 4.4e-7 | 5.4e-7
      (2, 135, 640, 3)     Z 3.2e-7 | 4.7e-7, P 1.0e-7 | 1.4e-7, dx 2.4e-7 | 6.8e-7, dA 4.0e-7 | 7.0e-7
      (2, 33, 32, 32)      Z 2.1e-7 | 3.0e-7, P 2.0e-7 | 2.8e-7, dx 1.9e-7 | 3.1e-7, dA 3.0e-7 | 6.4e-7
      (1, 1153, 32, 1)     Z 1.5e-7 | 2.8e-7, P 1.6e-7 | 7.7e-7, dx 1.5e-7 | 7.7e-7, dA 1.9e-7 | 5.9e-7
      (2, 128, 160, 2)     Z 1.4e-7 | 9.2e-7, P 8.0e-8 | 7.4e-7, dx 1.5e-7 | 8.8e-7, dA 2.3e-7 | 6.7e-7
      (2, 127, 96, 31)     Z 2.6e-7 | 4.6e-7, P 2.4e-7 | 7.1e-7, dx 3.8e-7 | 6.7e-7, dA 4.5e-7 | 6.5e-7
      (3, 9, 1024, 1)      Z 3.2e-7 | 1.8e-7, P 2.8e-7 | 1.7e-7, dx 5.2e-7 | 4.2e-7, dA 8.6e-7 | 5.8e-7
      (2, 1153, 1024, 32)  Z 6.6e-7 | 1.1e-6, P 4.4e-7 | 9.0e-7, dx 4.1e-7 | 6.6e-7, dA 4.1e-7 | 1.8e-6
      (2, 1, 512, 3)       Z 0 | 0, P 0 | 0, dx 6.1e-8 | 6.1e-8, dA 0 | 0
      (3, 1, 32, 32)       Z 0 | 0, P 0 | 0, dx 1.1e-7 | 8.0e-8, dA 0 | 0
      (3, 1, 1024, 31)     Z 0 | 0, P 0 | 0, dx 1.3e-7 | 1.1e-7, dA 0 | 0
      (2, 2, 544, 32)      Z 2.5e-7 | 3.5e-7, P 2.3e-7 | 2.8e-7, dx 5.9e-7 | 2.4e-7, dA 7.4e-7 | 3.3e-7
      (3, 2, 96, 1)        Z 4.5e-8 | 4.5e-8, P 2.5e-8 | 2.5e-8, dx 1.8e-7 | 1.1e-7, dA 2.5e-6 | 1.2e-6
      (2, 7, 640, 2)       Z 2.6e-7 | 9.0e-7, P 2.3e-7 | 8.9e-7, dx 1.8e-7 | 4.0e-7, dA 1.7e-7 | 3.1e-7
      (2, 7, 160, 31)      Z 2.1e-7 | 2.7e-7, P 2.0e-7 | 2.2e-7, dx 3.6e-7 | 2.4e-7, dA 3.4e-7 | 4.1e-7
      (2, 8, 512, 32)      Z 3.2e-7 | 7.5e-7, P 2.8e-7 | 6.9e-7, dx 4.8e-7 | 7.2e-7, dA 4.9e-7 | 7.7e-7
      (3, 8, 96, 3)        Z 9.5e-8 | 2.0e-7, P 7.7e-8 | 2.1e-7, dx 3.8e-7 | 2.3e-7, dA 2.3e-7 | 1.8e-7
      (2, 9, 160, 2)       Z 2.0e-7 | 1.8e-7, P 1.6e-7 | 9.8e-8, dx 3.9e-7 | 1.6e-7, dA 4.6e-7 | 2.2e-7
      (2, 31, 544, 1)      Z 2.8e-7 | 8.8e-7, P 1.7e-7 | 7.9e-7, dx 7.4e-7 | 9.5e-7, dA 8.2e-7 | 1.0e-6
      (3, 31, 1024, 3)     Z 6.5e-7 | 5.0e-7, P 5.4e-7 | 4.2e-7, dx 4.9e-7 | 2.7e-7, dA 6.5e-7 | 3.9e-7
      (2, 32, 640, 31)     Z 5.1e-7 | 1.5e-6, P 3.2e-7 | 1.6e-6, dx 4.3e-7 | 1.9e-6, dA 4.2e-7 | 2.2e-6
      (2, 32, 512, 2)      Z 1.2e-7 | 2.1e-7, P 7.3e-8 | 1.8e-7, dx 3.1e-7 | 3.8e-7, dA 8.3e-7 | 5.7e-7
      (3, 33, 544, 3)      Z 2.5e-7 | 1.4e-6, P 1.8e-7 | 1.5e-6, dx 2.3e-7 | 1.2e-6, dA 2.9e-7 | 6.4e-7
      (2, 33, 640, 1)      Z 3.0e-7 | 8.2e-7, P 2.4e-7 | 8.2e-7, dx 2.9e-7 | 6.4e-7, dA 3.8e-7 | 5.5e-7
      (2, 127, 1024, 2)    Z 4.8e-7 | 4.2e-7, P 3.1e-7 | 2.5e-7, dx 5.4e-7 | 4.6e-7, dA 5.1e-7 | 5.6e-7
      (3, 128, 640, 32)    Z 4.0e-7 | 5.3e-7, P 4.1e-7 | 4.8e-7, dx 6.5e-7 | 7.0e-7, dA 5.7e-7 | 8.5e-7
      (2, 128, 32, 3)      Z 1.3e-7 | 2.5e-7, P 9.4e-8 | 2.0e-7, dx 4.2e-7 | 5.0e-7, dA 2.5e-7 | 3.8e-7
      (2, 129, 32, 31)     Z 4.5e-7 | 9.5e-7, P 2.2e-7 | 3.8e-7, dx 4.5e-7 | 4.6e-7, dA 3.4e-7 | 4.5e-7
      (2, 135, 512, 1)     Z 3.0e-7 | 1.0e-6, P 2.7e-7 | 1.9e-6, dx 3.8e-7 | 1.6e-6, dA 3.5e-7 | 1.1e-6
      (2, 256, 96, 32)     Z 3.9e-7 | 9.8e-7, P 3.2e-7 | 8.0e-7, dx 2.6e-7 | 5.8e-7, dA 2.2e-7 | 6.3e-7
      (3, 256, 544, 31)    Z 3.4e-7 | 1.5e-6, P 2.9e-7 | 4.3e-7, dx 1.1e-6 | 9.8e-7, dA 6.2e-7 | 1.3e-6
      (2, 257, 160, 3)     Z 3.4e-7 | 5.6e-7, P 4.7e-7 | 5.6e-7, dx 3.1e-7 | 3.6e-7, dA 2.8e-7 | 4.1e-7
      (2, 257, 512, 31)    Z 5.1e-7 | 7.5e-7, P 3.1e-7 | 4.1e-7, dx 7.1e-7 | 5.3e-7, dA 9.3e-7 | 1.1e-6
    Worst fused / max(stock, E_KIND) over the 68 cases: 1.66 (dA of (3, 2, 96, 1) with keep); the largest fused error of a
    kind: Z 7.0e-7, P 6.4e-7, dx 1.1e-6, dA 3.7e-6.  One patch with keep: |dA| up to 6.5e-6 against a bound of 8.2e-4.
    With the one-group kernels dispatched for D <= 1024 (a scratch build: columns from 512 on are never written) all 32 cases
    of D > 512 fail and the 36 others pass."""
    x, A, dZ = _inputs(B, M, D, R, seed=1000 * R + M + D)
    keep = _keep(B, R, M) if dropped else None
    got = _fused(x, A, keep, dZ)
    stock = _formulas(x, A, keep, dZ, torch.float32)
    ref = _formulas(x, A, keep, dZ, torch.float64)
    zero_ref = [k for k, r in enumerate(ref) if float(r.abs().max()) == 0.0]
    assert zero_ref == ([3] if M == 1 else [])
    tag = "%s%s" % ((B, M, D, R), " keep" if dropped else "")
    log = []
    for k, (name, a, s, r) in enumerate(zip(NAMES, got, stock, ref)):       # (every figure printed before the first assertion)
        assert a.shape == r.shape
        if k in zero_ref:
            log.append(None)
        else:
            _check("%s %s" % (name, tag), a, s, r, log)
    for k, (name, a, s) in enumerate(zip(NAMES, got, stock)):
        assert bool(torch.isfinite(a).all()), name
        if k in zero_ref:
            # dL = P (keep dP' - c) is zero in exact arithmetic; what is left is the rounding of the two float32 dot products
            # of length D that cancel (at most D 2^-24 of sum |dZ x| each), times P <= keep, times |x|
            kmax = 1.0 if keep is None else float(keep.max())
            bound = 4.0 * D * 2.0 ** -24 * kmax * float((dZ.double().abs() * x.double().abs()).sum(-1).max()) * float(x.abs().max())
            print("%s %s: float64 is zero; |fused| %.3e, |stock| %.3e, bound %.3e" % (
                name, tag, float(a.abs().max()), float(s.abs().max()), bound))
            assert float(a.abs().max()) <= bound
        else:
            _assert_log(log[k:k + 1], E_KIND[name])
    if M == 1 and not dropped:
        assert torch.equal(got[0], x.expand(B, R, D)) and torch.equal(got[1], torch.ones_like(got[1]))


@pytest.mark.parametrize("dropped", [False, True])
@pytest.mark.parametrize("B,M,D,R", [(2, 135, 640, 3), (2, 257, 1024, 32), (3, 100, 128, 8)])
def test_backward_without_dx(B, M, D, R, dropped):
    """want_dx = False (the embeddings need no gradient: the kernel leaves after dA's block) returns no dx and the bits of
    dA of the want_dx = True call - directly, and through autograd with x detached."""
    x, A, dZ = _inputs(B, M, D, R, seed=51)
    keep = _keep(B, R, M) if dropped else None
    Z, P = hip.attn_pool_forward(x, A, keep)
    dx, dA = hip.attn_pool_backward(x, A, keep, P, Z, dZ)
    none, dA_only = hip.attn_pool_backward(x, A, keep, P, Z, dZ, want_dx=False)
    assert none is None and dx is not None
    assert bool(torch.isfinite(dA).all()) and float(dA.abs().max()) > 0.0
    assert torch.equal(dA_only, dA)
    Ag = A.clone().requires_grad_()
    Zg = fused_aggregator.hip_pool(x.detach(), Ag, keep)
    assert torch.equal(Zg.detach(), Z)
    Zg.backward(dZ)
    assert torch.equal(Ag.grad, dA)


@pytest.mark.parametrize("R", [3, 32])
@pytest.mark.parametrize("D", [32, 640])
@pytest.mark.parametrize("M", [1, 7, 129, 135])
def test_poisoned_neighbour_image(M, D, R):
    """B = 3 with the x, dZ and keep rows of image 1 NaN: Z, P, dx of images 0 and 2 are finite and the bits of the same
    images computed alone.  (A row read past an image's end carries weight 0 - harmless unless it is NaN; every read stays
    inside the three live tensors.)  dA sums over the images and is NaN by construction."""
    B = 3
    x, A, dZ = _inputs(B, M, D, R, seed=61)
    keep = _keep(B, R, M)
    x[1], dZ[1], keep[1] = float("nan"), float("nan"), float("nan")
    got = _fused(x, A, keep, dZ)
    for b in (0, 2):
        alone = _fused(x[b:b + 1].contiguous(), A, keep[b:b + 1].contiguous(), dZ[b:b + 1].contiguous())
        for k in range(3):
            assert bool(torch.isfinite(got[k][b]).all()), (NAMES[k], b)
            assert torch.equal(got[k][b], alone[k][0]), (NAMES[k], b)
        assert bool(torch.isfinite(alone[3]).all())


@pytest.mark.parametrize("dropped", [False, True])
@pytest.mark.parametrize("B,M,D,R", [(2, 33, 96, 1), (2, 135, 640, 3), (2, 129, 544, 31)])
def test_operands_followed_by_nan_rows(B, M, D, R, dropped):
    """A (R, D), dZ (B, R, D) and x (B, M, D) as the leading rows of larger buffers whose following rows are NaN (the views
    are contiguous and start on the allocation): every output is finite and has the bits of the call on tight tensors.
    The rows of A and dZ beyond R are zero operands of the kernels, not reads."""
    x, A, dZ = _inputs(B, M, D, R, seed=71)
    keep = _keep(B, R, M) if dropped else None

    def padded(t):
        rows = t.numel() // D
        big = torch.full((rows + 40, D), float("nan"), device=DEV)
        big[:rows] = t.reshape(rows, D)
        view = big[:rows].view(t.shape)
        assert view.is_contiguous() and view.data_ptr() % 16 == 0 and bool(torch.isnan(big[rows:]).all())
        return view
    want = _fused(x, A, keep, dZ)
    got = _fused(padded(x), padded(A), keep, padded(dZ))
    for name, u, v in zip(NAMES, got, want):
        assert bool(torch.isfinite(u).all()), name
        assert torch.equal(u, v), name


SENTINEL = 0x7FA5C3D2          # a NaN's bits: a sentinel word that is read, not only one that is written, shows as well
GUARD = 2048                   # words in front of and behind every slice: 8 KiB, so the slice starts 16-byte aligned
EWORKSPACE = -3                # include/ipsx.h IPSX_EWORKSPACE


class _Guarded:
    """``words`` float32 in the middle of a larger tensor filled with SENTINEL."""

    def __init__(self, *shape):
        self.words = 1
        for s in shape:
            self.words *= s
        self.big = torch.full((GUARD + self.words + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
        self.t = self.big[GUARD:GUARD + self.words].view(torch.float32).view(*shape)
        assert self.t.data_ptr() % 16 == 0 and self.t.is_contiguous()

    def guards_untouched(self):
        return bool((self.big[:GUARD] == SENTINEL).all()) and bool((self.big[GUARD + self.words:] == SENTINEL).all())

    def untouched(self):
        return bool((self.big == SENTINEL).all())


@pytest.mark.parametrize("B,M,D,R", [(2, 1, 32, 1), (2, 129, 544, 31), (3, 33, 1024, 32), (2, 135, 96, 3)])
def test_guarded_outputs_and_workspace(B, M, D, R):
    """ipsx_attn_pool_forward / ipsx_attn_pool_backward through the C entry points with the wrappers' argument lists, Z, P,
    dx, dA and a workspace of exactly ipsx_attn_pool_workspace_bytes each a slice between two 8 KiB guards of a sentinel:
    no guard word changes, and the slices hold the bits the wrappers return.  With a workspace one float short either call
    returns IPSX_EWORKSPACE and launches nothing: every output still holds the sentinel."""
    L = hip.lib()
    p, stream = hip._p, hip._stream
    x, A, dZ = _inputs(B, M, D, R, seed=81)
    keep = _keep(B, R, M)
    want = _fused(x, A, keep, dZ)
    nb = int(L.ipsx_attn_pool_workspace_bytes(B, M, R, D))
    assert nb > 0 and nb % 4 == 0
    Z, P, dx, dA = _Guarded(B, R, D), _Guarded(B, R, M), _Guarded(B, M, D), _Guarded(R, D)
    ws = _Guarded(nb // 4)
    outs = (Z, P, dx, dA)
    # one float short: refused before any launch
    assert L.ipsx_attn_pool_forward(p(x), p(A), p(keep), B, M, R, D, p(Z.t), p(P.t), p(ws.t), nb - 4, stream()) == EWORKSPACE
    assert L.ipsx_attn_pool_backward(p(x), p(A), p(keep), p(want[1]), p(want[0]), p(dZ), B, M, R, D, p(dx.t), p(dA.t), p(ws.t),
                                     nb - 4, stream()) == EWORKSPACE
    torch.cuda.synchronize()
    assert all(g.untouched() for g in outs + (ws,))
    assert L.ipsx_attn_pool_forward(p(x), p(A), p(keep), B, M, R, D, p(Z.t), p(P.t), p(ws.t), nb, stream()) == 0
    torch.cuda.synchronize()
    assert all(g.guards_untouched() for g in outs + (ws,)) and dx.untouched() and dA.untouched()
    assert torch.equal(Z.t, want[0]) and torch.equal(P.t, want[1])
    ws.big.fill_(SENTINEL)
    assert L.ipsx_attn_pool_backward(p(x), p(A), p(keep), p(P.t), p(Z.t), p(dZ), B, M, R, D, p(dx.t), p(dA.t), p(ws.t), nb,
                                     stream()) == 0
    torch.cuda.synchronize()
    assert all(g.guards_untouched() for g in outs + (ws,))
    assert torch.equal(dx.t, want[2]) and torch.equal(dA.t, want[3])
    assert torch.equal(Z.t, want[0]) and torch.equal(P.t, want[1])          # (inputs of the backward: read only)


# ------------------------------------------------------------------ the whole node
def _transformer(T, H, D, D_k, D_v, D_inner, seed):
    """Transformer(...) with seeded normals of 1 / sqrt(fan_in) (q: 1 / sqrt(D_k), the scale of its own initialisation;
    LayerNorm weights around 1, biases around 0)."""
    transf = Transformer(T, H, D, D_k, D_v, D_inner, attn_dropout=0, dropout=0)
    g = torch.Generator(device="cpu").manual_seed(seed)
    with torch.no_grad():
        for n, p in transf.named_parameters():
            v = torch.randn(p.shape, generator=g)
            if n == "crs_attn.q":
                v = v / D_k ** 0.5
            elif n.endswith("layer_norm.weight"):
                v = 1.0 + 0.1 * v
            elif p.dim() == 1:
                v = 0.1 * v
            else:
                v = v / p.shape[-1] ** 0.5
            p.copy_(v)
    return transf.to(DEV).train()


def _loss(out, w):
    """the loss of tests/test_train_aggregator.py::_node_step"""
    return 100.0 * ((out * w.to(out.dtype)).sum() + 0.1 * out.sum(1).sin().sum())


def _node_grads(transf, x, w, forward):
    xr = x.clone().requires_grad_()
    out = forward(transf, xr)
    transf.zero_grad(set_to_none=True)
    _loss(out, w).backward()
    res = {"out": out.detach(), "x.grad": xr.grad.clone()}
    for n, p in transf.named_parameters():
        res["grad " + n] = p.grad.clone()
    return res


def _counting(monkeypatch):
    calls = []
    real = fused_aggregator.forward

    def counted(transf, x, keep=None, pool=None):
        calls.append(tuple(x.shape))
        return real(transf, x, keep, pool)
    monkeypatch.setattr(fused_aggregator, "forward", counted)
    return calls


def _stock(transf, x):
    return transf.mlp(transf.crs_attn(x))


def _node_inputs(B, M, T, D, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn((B, M, D), generator=g).to(DEV), torch.randn((B, T, D), generator=g).to(DEV)


# (T, H, D, D_k, D_v, D_inner, M): D_k != D_v in four of the five, odd R = H T (15, 3), H = 1, T > 4, R = 1, R = 32
LAYOUTS = [(8, 4, 96, 24, 8, 64, 129), (1, 1, 32, 8, 40, 32, 7), (5, 3, 640, 32, 16, 128, 135), (2, 16, 1024, 64, 64, 256, 257),
           (3, 1, 160, 16, 48, 64, 33)]


@pytest.mark.parametrize("T,H,D,D_k,D_v,D_inner,M", LAYOUTS)
def test_whole_node_at_other_head_layouts(T, H, D, D_k, D_v, D_inner, M, monkeypatch):
    """Transformer.forward under autograd at head layouts no configuration has (A folded with view(H, D_k, D), ctx built with
    view(H, D_v, D)): output, x.grad and every parameter's gradient against a float64 copy, the stock float32 modules as
    the yardstick (fused <= 4 x stock); the fused route is taken exactly once.
    Measured on an MI355X, worst fused / stock ratio over the 10 to 12 tensors, in the order of LAYOUTS: 1.31, 1.41, 1.65, 1.17,
    1.36."""
    calls = _counting(monkeypatch)
    a = _transformer(T, H, D, D_k, D_v, D_inner, seed=91)
    s, r = copy.deepcopy(a), copy.deepcopy(a).double()
    assert fused_aggregator.supported(a)
    x, w = _node_inputs(2, M, T, D, seed=92)
    fa = _node_grads(a, x, w, lambda t, xs: t(xs))
    assert calls == [(2, M, D)]
    fs, fr = _node_grads(s, x, w, _stock), _node_grads(r, x.double(), w.double(), _stock)
    assert len(calls) == 1
    log = []
    for k in fr:
        _check("%s %s" % (k, (T, H, D, D_k, D_v)), fa[k], fs[k], fr[k], log)
    print("worst fused / stock ratio %.2f" % _worst(log))
    _assert_log(log)


class _Keep(nn.Module):
    """In the place of the attention dropout: the (B, H, T, M) attention times fixed factors."""

    def __init__(self, keep):
        super().__init__()
        self.keep = keep

    def forward(self, attn):
        return attn * self.keep.to(attn.dtype)


def test_whole_node_with_an_explicit_keep():
    """fused_aggregator.forward(transf, x, keep=keep) with the (B, H * n_token, M) keep of ``_keep`` against float64 and
    float32 stock copies whose attention dropout multiplies the (B, H, T, M) attention by keep.view(B, H, T, M): the
    documented row order h * T + t (a keep taken as t * H + h is another function: the rule depends on m + r + b).
    Measured on an MI355X, worst fused / stock ratio: 1.84."""
    T, H, D, D_k, D_v, D_inner, M = LAYOUTS[0]
    B = 2
    a = _transformer(T, H, D, D_k, D_v, D_inner, seed=93)
    s, r = copy.deepcopy(a), copy.deepcopy(a).double()
    keep = _keep(B, H * T, M)
    assert not torch.equal(keep.view(B, H, T, M), keep.view(B, T, H, M).transpose(1, 2))
    for m in (s, r):
        m.crs_attn.attention.dropout = _Keep(keep.view(B, H, T, M))
    x, w = _node_inputs(B, M, T, D, seed=94)
    fa = _node_grads(a, x, w, lambda t, xs: fused_aggregator.forward(t, xs, keep=keep))
    fs, fr = _node_grads(s, x, w, _stock), _node_grads(r, x.double(), w.double(), _stock)
    log = []
    for k in fr:
        _check("%s, explicit keep" % k, fa[k], fs[k], fr[k], log)
    print("worst fused / stock ratio %.2f" % _worst(log))
    _assert_log(log)


@pytest.mark.parametrize("T,H,D,D_k,D_v,D_inner", [(3, 11, 64, 8, 8, 32), (2, 2, 1056, 16, 16, 64)])
def test_refused_layouts_run_the_stock_modules(T, H, D, D_k, D_v, D_inner, monkeypatch):
    """H * n_token = 33 and D = 1056 are beyond the kernels: ``supported`` refuses, fused_aggregator.forward is not reached,
    and Transformer.forward under autograd is the stock modules, bit for bit."""
    calls = _counting(monkeypatch)
    transf = _transformer(T, H, D, D_k, D_v, D_inner, seed=95)
    assert not fused_aggregator.supported(transf)
    x = _node_inputs(2, 37, T, D, seed=96)[0].requires_grad_()
    out = transf(x)
    assert out.requires_grad and calls == []
    assert torch.equal(out, _stock(transf, x))
    out.sum().backward()
    assert bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0.0


def test_non_contiguous_embeddings_and_gradient(monkeypatch):
    """x = big[:, ::2] of a leaf ``big`` and a loss that consumes Z.transpose(1, 2): big.grad is zero on the skipped rows
    and matches float64 on the used ones within the yardstick.
    Measured on an MI355X, fused | stock error: the output 3.1e-7 | 2.9e-7, big.grad on the used rows 3.5e-7 | 4.3e-7."""
    T, H, D, D_k, D_v, D_inner, M = LAYOUTS[2]
    B = 2
    calls = _counting(monkeypatch)
    a = _transformer(T, H, D, D_k, D_v, D_inner, seed=97)
    s, r = copy.deepcopy(a), copy.deepcopy(a).double()
    big0, w = _node_inputs(B, 2 * M, T, D, seed=98)

    def run(transf, big, w, forward):
        big = big.clone().requires_grad_()
        x = big[:, ::2]
        assert not x.is_contiguous()
        zt = forward(transf, x).transpose(1, 2)                                   # (B, D, T)
        loss = 100.0 * ((zt * w.to(zt.dtype).transpose(1, 2)).sum() + 0.1 * zt.sum(2).sin().sum())
        loss.backward()
        return zt.detach(), big.grad
    za, ga = run(a, big0, w, lambda t, xs: t(xs))
    assert calls == [(B, M, D)]
    zs, gs = run(s, big0, w, _stock)
    zr, gr = run(r, big0.double(), w.double(), _stock)
    assert ga.shape == (B, 2 * M, D)
    assert torch.equal(ga[:, 1::2], torch.zeros_like(ga[:, 1::2])) and float(ga[:, ::2].abs().max()) > 0.0
    log = []
    _check("out, x = big[:, ::2]", za, zs, zr, log)
    _check("big.grad[:, ::2]", ga[:, ::2], gs[:, ::2], gr[:, ::2], log)
    _assert_log(log)
