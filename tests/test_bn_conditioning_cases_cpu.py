"""CPU: the cases of tests/bn_conditioning_cases.py are what they declare, and stock float32 ``F.batch_norm`` handles every
one of them inside the floors that tests/test_hip_train.py asserts of the kernels (y 2e-6, gradients 2e-5, relative to the
tensor's largest entry, against float64 autograd).  The second half is what keeps the bounds of
tests/test_bn_train_conditioning.py - max(floor, 4 x stock error) - from being vacuous: on these inputs a correct
float32 BatchNorm IS that accurate, so a kernel that is not has lost it in its own arithmetic.  ``tight`` is the
exception by construction (float32 cannot store its mean to better than 6e-3 sigma), and says so."""
import pytest
import torch
import torch.nn.functional as F

import bn_conditioning_cases as K

EPS = 1e-5
FLOOR_Y, FLOOR_GRAD = 2e-6, 2e-5
SHAPES = [(64, 8, 8), (1025, 4, 1), (32769, 64, 1)]              # >= 1025 rows: an outlier row CAN be 30 batch-sigma off


def _rel(a, b):
    return float((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _stock_errors(x, seed=0, y_channels=slice(None)):
    """float32 F.batch_norm (training mode) with autograd on the CPU against the same in float64 -> {tensor: error}.
    On the values, laid out channel by channel as ONE image (1, C, rows, 1) - the same BatchNorm: ATen's CPU kernel for
    rows-major memory adds a channel's rows up one by one in float32 and comes to 2.3e-6 on the 65,536 rows of ``patch0``
    where its kernel for contiguous channels gives 1.0e-7, and what is asked here is what float32 CAN do on these inputs."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    C = x.shape[1]
    x = K.rows(x).t().contiguous().view(1, C, -1, 1)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    dy = torch.randn(x.shape, generator=g)
    out = {}
    for dt in (torch.float64, torch.float32):
        xs, gs, bs = (t.detach().to(dt).clone().requires_grad_() for t in (x, gamma, beta))
        y = F.batch_norm(xs, None, None, gs, bs, True, 0.1, EPS)
        y.backward(dy.to(dt))
        out[dt] = {"y": y.detach()[:, y_channels], "dx": xs.grad, "dgamma": gs.grad, "dbeta": bs.grad}
    return {k: _rel(out[torch.float32][k], out[torch.float64][k]) for k in out[torch.float64]}


def _inside_floors(x, name, y_channels=slice(None)):
    err = _stock_errors(x, y_channels=y_channels)
    print(name, " ".join("%s %.2e" % kv for kv in err.items()))
    assert err["y"] <= FLOOR_Y, (name, err)
    for k in ("dx", "dgamma", "dbeta"):
        assert err[k] <= FLOOR_GRAD, (name, k, err)


@pytest.mark.parametrize("shape", SHAPES)
def test_single_outlier_rows_are_far_out_and_stock_float32_does_not_mind(shape):
    n = shape[0] * shape[2] * shape[2]
    for name, case, floor in (("row0 +50", K.row0(*shape), 40.0), ("row0 -200", K.row0(*shape, value=-200.0), 160.0),
                              ("last", K.last(*shape), 40.0)):
        assert case.prop["rest"] >= floor, (name, case.prop)              # delta / sigma of the N(0, 1) bulk
        assert case.prop["batch"] >= 0.5 * min(floor, n ** 0.5), (name, case.prop)   # .. of the batch: at most sqrt(rows)
        _inside_floors(case.x, name)
    a, b = K.row0(*shape).x, K.last(*shape).x
    assert torch.equal(K.rows(a)[1:-1], K.rows(b)[1:-1]) and torch.equal(K.rows(a)[0], K.rows(b)[-1])   # the same outlier, moved


@pytest.mark.parametrize("shape", SHAPES)
def test_head8_well_tight_const(shape):
    n = shape[0] * shape[2] * shape[2]
    c = K.head8(*shape)
    assert c.prop["rest"] >= 40.0, c.prop
    if n >= 4096:
        assert c.prop["batch"] >= 15.0, c.prop
    assert bool((K.rows(c.x)[:8] == K.OUTLIER).all())
    _inside_floors(c.x, "head8")

    c = K.well(*shape)
    assert c.prop["mean_over_sigma"] <= 2.0, c.prop
    _inside_floors(c.x, "well")

    c = K.const(*shape)
    assert c.prop["var0"] == 0.0 and bool((c.x[:, 0] == K.CONST).all())
    y = F.batch_norm(c.x.double(), None, None, None, None, True, 0.1, EPS)
    # reference invstd = 1 / sqrt(eps) = 316 there, on a numerator that is zero up to the float64 rounding of the mean
    assert float(y[:, 0].abs().max()) <= 1e-9
    # channel 0 of y is the exception to the floor, in any float32 BatchNorm: a mean that is a fraction of an ulp of 3.25 off - as
    # ATen's is - times that invstd is 1.2e-7 * 316 = 3.8e-5 next to beta; the channel is held to exactly that instead
    _inside_floors(c.x, "const", y_channels=slice(1, None))
    y32 = F.batch_norm(c.x.contiguous(), None, None, None, None, True, 0.1, EPS)
    assert float(y32[:, 0].abs().max()) <= 2.0 ** -22 / EPS ** 0.5                  # (an ulp of 3.25, to be safe)

    c = K.tight(*shape)
    assert c.prop["mean_over_sigma"] >= 5e4 and c.prop["row0"] <= 4.5, c.prop     # row 0 is typical; the mean is what is far
    err = _stock_errors(c.x)
    print("tight", " ".join("%s %.2e" % kv for kv in err.items()))
    # the exception: x - mean carries 2^-24 * 1000 / 0.01 = 6e-3 sigma of rounding in float32 whatever the kernel does
    assert err["y"] > FLOOR_Y


@pytest.mark.parametrize("shape", SHAPES + [(16, 1024, 2)])
@pytest.mark.parametrize("which", ["row0", "slabs", "lanes"])
def test_sampled_puts_the_outliers_on_the_shift_rows(shape, which):
    P, C, H = shape
    n = P * H * H
    nrl, slab, slabs = K.bn_slab_cut(n, C)
    idx = K.sampled_rows(n, C, which)
    assert slabs <= 512 and slab * (slabs - 1) < n <= slab * slabs
    want = {"row0": 1, "slabs": slabs, "lanes": sum(min(nrl, min(slab, n - g * slab)) for g in range(slabs))}[which]
    assert len(idx) == len(set(idx)) == want and idx[0] == 0 and max(idx) < n
    c = K.sampled(P, C, H, which)
    lad = K.ladder(C)
    assert bool((K.rows(c.x)[idx] == lad).all())
    if C >= len(K.LADDER):                       # every rung present: channels below, near and far above the 2-sigma line
        assert set(lad.abs().tolist()) == set(torch.tensor(K.LADDER).tolist())
        assert c.prop["rest_max"] >= 250.0 and c.prop["rest"] <= 1.2, c.prop
    _inside_floors(c.x, "sampled " + which)


def test_patch0_and_jump():
    c = K.patch0(1024, 64, 8)
    assert c.x.numel() * 4 == 16 << 20
    assert c.prop["rest"] >= 40.0 and c.prop["batch"] >= 25.0, c.prop   # delta / sigma_batch <= sqrt(1024) = 32
    assert bool((c.x[0] == K.OUTLIER).all())
    _inside_floors(c.x, "patch0")

    c = K.jump(64, 64, 8)
    assert c.prop["stale"] >= 49.0, c.prop
    _inside_floors(c.x[0], "jump, first")
    _inside_floors(c.x[1], "jump, second")

    c = K.jump_const(64, 64, 8)
    assert c.prop["var0"] == 0.0 and c.prop["stale0"] >= 2.0, c.prop
    _inside_floors(c.x[1], "jump, then const", y_channels=slice(1, None))


@pytest.mark.parametrize("n,f", [(4096, 64), (130, 256)])
def test_projector_rows_have_tight_columns_behind_a_far_head(n, f):
    x = K.projector_rows(n, f).double()
    assert bool((x[:8] == x[0]).all())
    g = torch.Generator(device="cpu").manual_seed(1)
    w = (torch.randn((f, f), generator=g) / f ** 0.5).double()
    z = F.layer_norm(x, (f,), None, None, 1e-5) @ w.t()
    off = (z[:8].mean(0) - z.mean(0)).abs() / z.std(0, unbiased=False)
    print("projector rows: shift rows are %.1f .. %.1f column sigma from the column mean" % (float(off.min()), float(off.max())))
    assert float(off.median()) >= 0.95 * (n / 8) ** 0.5       # (sqrt(n / 8) = 22.6 and 4.0 is the most 8 rows of n can be off)
