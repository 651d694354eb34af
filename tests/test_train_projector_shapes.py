"""The with-grad feature projector (csrc/projector_train.hip) at the seams tests/test_train_projector.py does not reach: fewer
rows than one 64-row tile (1, 63) and one more (65), the 4096-row chunk of the weight gradient from below (4095, 4096),
D = 256 (the NTW = 2 forward kernel with grid.y = 1 and all 256 columns live), F = 32 (one k-group of 8 times four, the
minimum), and outputs between guards.

The yardstick is that file's: per tensor, err(t) = max |t - t64| / max |t64| against float64 autograd of nn.LayerNorm +
Linear, the fused error at most 4 x the stock float32 error on the same inputs.  At these small shapes the stock error can be
0 or a fraction of an ulp, so each tensor kind is held to 4 x max(stock error of the case, E_KIND[kind]), E_KIND the largest
STOCK error of that kind over CASES (a property of the ATen path, measured once on an MI355X).  A dropped row or k-group
shows at 1 / rows or 1 / F of the scale, orders of magnitude above either.  Both errors are printed."""

import ctypes as C

import pytest
import torch
from torch import nn

from ips_amd import hip
from ips_amd.hip_encoder import _pack_conv

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LN_EPS, BN_EPS = 1e-5, 1e-5
NAMES = ("z", "column mean", "column invstd", "dW", "db")

# the largest stock float32 error per tensor kind over CASES, measured on an MI355X (the table in
# test_seams_against_float64): z at (4096, 288, 32), the four others at (4095, 32, 256)
E_KIND = {"z": 6.569e-7, "column mean": 1.905e-7, "column invstd": 1.533e-7, "dW": 1.955e-6, "db": 2.045e-7}


def _err(t, ref):
    ref = ref.double()
    return float((t.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def _check(name, fused, stock, ref, log):
    ef, es = _err(fused, ref), _err(stock, ref)
    print("%-36s fused %.3e   stock %.3e" % (name, ef, es))
    log.append((name, ef, es))


def _assert_log(log, floor=0.0):
    bad = [(n, ef, es) for n, ef, es in log if not ef <= 4.0 * max(es, floor)]
    assert not bad, bad


def _inputs(rows, f, d, seed, offset=True):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn((rows, f), generator=g)
    if offset:                                  # features with a per-feature pattern, as extracted features have
        x = x * (0.5 + torch.rand((1, f), generator=g)) + 0.5 * torch.randn((1, f), generator=g)
    w = torch.randn((d, f), generator=g) / f ** 0.5
    b = 0.1 * torch.randn(d, generator=g)
    dz = torch.randn((rows, d), generator=g)
    return x.to(DEV), w.to(DEV), b.to(DEV), dz.to(DEV)


def _reference(x, w, b, dz, dtype):
    """z, column mean / invstd of z, dW, db by autograd of nn.LayerNorm + nn.Linear in ``dtype``"""
    ln = nn.LayerNorm(x.shape[1], eps=LN_EPS, elementwise_affine=False)
    wt, bt = w.detach().to(dtype).clone().requires_grad_(), b.detach().to(dtype).clone().requires_grad_()
    z = torch.nn.functional.linear(ln(x.to(dtype)), wt, bt)
    z.backward(dz.to(dtype))
    zd = z.detach()
    return zd, zd.mean(0), 1.0 / torch.sqrt(zd.var(0, unbiased=False) + BN_EPS), wt.grad, bt.grad


def _fused(x, w, b, dz):
    z, stats, partial, slabs, shift = hip.projector_train_forward(x, w, b, LN_EPS)
    d = w.shape[0]
    gamma, beta = torch.ones(d, device=DEV), torch.zeros(d, device=DEV)
    rm, rv = torch.zeros(d, device=DEV), torch.ones(d, device=DEV)
    _, mean, invstd = hip.bn_train_forward_partials(z, None, gamma, beta, BN_EPS, 0.1, rm, rv, True, partial, slabs, shift)
    dw, db = hip.projector_wgrad(x, dz, stats)
    return z, mean, invstd, dw, db


# (rows, F, D): one row; one row short of a 64-row tile at the minimum F; one row past a tile at D = 256; the weight
# gradient's 4096-row chunk from below (4095: an odd last row pair) and exactly, at F = 32 / D = 256 and at the F = 288
# (a partial 256-column region) / D = 32 (no second tile) corner; 130 rows (two tiles and two rows) at F = D = 256
CASES = [(1, 64, 32), (63, 32, 64), (65, 96, 256), (4095, 32, 256), (4096, 288, 32), (130, 256, 256)]


@pytest.mark.parametrize("rows,f,d", CASES)
def test_seams_against_float64(rows, f, d):
    """z, the column mean and invstd the BatchNorm takes off the forward kernel's sums, dW and db against float64, each kind
    held to 4 x max(stock error of the case, E_KIND[kind]).  One row: the column variance is 0, the column mean is the row
    itself and invstd = 1 / sqrt(eps).
    Measured on an MI355X, fused | stock error:
      (1, 64, 32)          z 1.9e-7 | 1.0e-7, mean 1.9e-7 | 1.0e-7, invstd 5.4e-8 | 5.4e-8, dW 3.9e-8 | 7.3e-8, db 0 | 0
      (63, 32, 64)         z 2.3e-7 | 2.1e-7, mean 7.2e-8 | 1.2e-7, invstd 1.3e-7 | 9.7e-8, dW 2.7e-7 | 4.0e-7, db 6.8e-8 | 1.2e-7
      (65, 96, 256)        z 3.8e-7 | 3.5e-7, mean 8.5e-8 | 1.3e-7, invstd 1.7e-7 | 1.3e-7, dW 2.8e-7 | 3.7e-7, db 6.5e-8 | 6.5e-8
      (4095, 32, 256)      z 3.1e-7 | 2.4e-7, mean 5.1e-8 | 1.9e-7, invstd 7.4e-8 | 1.5e-7, dW 1.9e-6 | 2.0e-6, db 3.2e-7 | 2.0e-7
      (4096, 288, 32)      z 7.5e-7 | 6.6e-7, mean 2.8e-8 | 1.1e-7, invstd 7.8e-8 | 1.2e-7, dW 1.9e-6 | 1.9e-6, db 5.5e-7 | 9.0e-8
      (130, 256, 256)      z 6.4e-7 | 7.9e-7, mean 8.9e-8 | 1.8e-7, invstd 1.4e-7 | 1.5e-7, dW 4.5e-7 | 5.0e-7, db 1.2e-7 | 9.6e-8
    Worst fused / max(stock, E_KIND): 2.7 (db at 4,096 rows: 512 sequential additions per lane and slot, ATen's sum is a tree).
    With the column sums taken around row 0 of z alone, as they were, invstd measured 6.5e-7 | 9.7e-8 at (63, 32, 64) and
    8.8e-7 | 1.3e-7 at (65, 96, 256) - past 4 x max(stock, E_KIND) = 6.1e-7: var = q / n - (s / n)^2 cancels where row 0 lies
    3 sigma off the column mean, and one slab has no second one to average the fp32 rounding of s and q out.  The shift is
    now the mean of the first eight rows (projector_train_shift_kernel)."""
    x, w, b, dz = _inputs(rows, f, d, seed=rows + f)
    got = _fused(x, w, b, dz)
    stock = _reference(x, w, b, dz, torch.float32)
    ref = _reference(x, w, b, dz, torch.float64)
    log = []
    for name, a, s, r in zip(NAMES, got, stock, ref):
        assert a.shape == r.shape and bool(torch.isfinite(a).all())
        _check("%s (%d, %d, %d)" % (name, rows, f, d), a, s, r, log)
    if rows == 1:                               # (the float64 reference itself: no spread, the mean is the row)
        assert _err(ref[2], torch.full_like(ref[2], BN_EPS ** -0.5)) < 1e-12 and torch.equal(ref[1], ref[0][0])
    for k, name in enumerate(NAMES):
        _assert_log(log[k:k + 1], E_KIND[name])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("rows,f,d", [(63, 32, 64), (65, 96, 256)])
def test_half_stored_rows_at_the_tile_seam(rows, f, d, dtype):
    """float16 / bfloat16 rows give the bits of the same values passed as float32 - z, the column statistics, dW, db - below
    and past one 64-row tile (tests/test_train_projector.py asserts it at (2500, 512, 128))."""
    x, w, b, dz = _inputs(rows, f, d, seed=7)
    xh = x.to(dtype)
    assert not torch.equal(xh.float(), x)
    for name, u, v in zip(NAMES, _fused(xh, w, b, dz), _fused(xh.float(), w, b, dz)):
        assert bool(torch.isfinite(u).all()) and torch.equal(u, v), name


SENTINEL = 0x7FA5C3D2          # a NaN's bits
GUARD = 2048                   # words in front of and behind every slice: 8 KiB, so the slice starts 16-byte aligned


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


def test_guarded_outputs():
    """Both of the two: ipsx_projector_train_forward through the C entry point with the wrapper's argument list, z, the
    column-sum partials and the shift each a slice between two 8 KiB guards of a sentinel; and ipsx_projector_wgrad with
    dW, db and a workspace of exactly ipsx_projector_wgrad_workspace_bytes guarded in the same way - at (65, 96, 256), one row
    past a tile.  No guard word changes, and the slices hold the bits the wrappers return."""
    rows, f, d = 65, 96, 256
    L = hip.lib()
    p, stream = hip._p, hip._stream
    x, w, b, dz = _inputs(rows, f, d, seed=11)
    z_w, stats_w, partial_w, slabs, shift_w = hip.projector_train_forward(x, w, b, LN_EPS)
    dw_w, db_w = hip.projector_wgrad(x, dz, stats_w)
    packed = _pack_conv(w.view(d, f, 1, 1))
    lin = hip.Conv(f, d, 1, 1, 1, 0, p(packed), None, p(b), None, None)
    stats = torch.empty((rows, 2), dtype=torch.float32, device=DEV)
    assert L.ipsx_projector_stats_typed(p(x), 0, rows, f, C.c_float(LN_EPS), p(stats), stream()) == 0
    assert torch.equal(stats, stats_w)
    assert slabs == int(L.ipsx_projector_train_slabs(rows)) == 2
    z, partial, shift = _Guarded(rows, d), _Guarded(slabs, 2, d), _Guarded(d)
    assert L.ipsx_projector_train_forward(C.byref(lin), p(w), p(x), 0, rows, p(stats), p(z.t), p(shift.t), p(partial.t), stream()) == 0
    torch.cuda.synchronize()
    assert all(g.guards_untouched() for g in (z, partial, shift))
    assert torch.equal(z.t, z_w) and torch.equal(partial.t, partial_w) and torch.equal(shift.t, shift_w)
    nb = int(L.ipsx_projector_wgrad_workspace_bytes(rows, f, d))
    assert nb == (d * f + d) * 4
    dw, db, ws = _Guarded(d, f), _Guarded(d), _Guarded(nb // 4)
    assert L.ipsx_projector_wgrad(p(x), 0, p(dz), p(stats), rows, f, d, p(dw.t), p(db.t), 0, p(ws.t), nb, stream()) == 0
    torch.cuda.synchronize()
    assert all(g.guards_untouched() for g in (dw, db, ws))
    assert torch.equal(dw.t, dw_w) and torch.equal(db.t, db_w)
