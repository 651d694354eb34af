"""GPU: the three producers of training-mode BatchNorm batch statistics on batches whose SHIFT ROWS are atypical
(tests/bn_conditioning_cases.py; tests/test_bn_conditioning_cases_cpu.py shows that stock float32 handles every case).

Every producer sums d = x - shift and d^2 in float32; var = E[d^2] - E[d]^2 is as good as the shift is near the mean.
``bn_reduce_kernel<false>`` (csrc/bn_train.hip) took row 0 of the activation, the convolutions' epilogues the previous
step's batch mean (the first patch's at a layer's first step), the projector the mean of z's first 8 rows: the suite had
only well-spread random data, where such a sample is 1 - 3 sigma off, and all of it passed at 1e-6.

Yardstick (tests/test_train_aggregator_shapes.py): float64 autograd of the same BatchNorm (+ residual, + ReLU) on the same
inputs is the reference, float32 ``torch.native_batch_norm`` on the same device (what ``F.batch_norm`` runs) the stock path;
per tensor ``fused <= max(B, 4 x stock)``, B what tests/test_hip_train.py asserts of that tensor already (B_FWD behind
``bn_train_forward``, B_PART behind ``bn_train_forward_partials``).  Errors: mean |mean - mean64| / sqrt(var64 + eps) per
channel (means may be near zero), invstd |invstd / invstd64 - 1| per channel, anything else max |t - t64| / max |t64|.
Under ReLU ``dy`` is 0 wherever the float64 pre-activation lies within 1e-3 gamma (= 1e-3 sigma of the normalised term)
of zero, so that no mask flip decides a gradient, and the masks must agree everywhere else (``tight``: within 2^-22 |mean|
invstd gamma = 2.4e-2 gamma, which is what a float32 mean costs x - mean there).  Both errors are printed.
dx at one and two rows: there xhat is 0 resp. +-1 whatever the data, dx64 is what eps / var leaves of terms of order
dy gamma invstd, and an error relative to max |dx64| measures float32 rounding against 1e-4 of itself (1.2e+1 for the
kernel and for ATen alike).  At those shapes dx is held to max |dx - dx64| / max |dy gamma invstd64| instead, the size of
the terms that cancel - same floor, same 4 x.

Measured on an MI355X: in each test's docstring, fused | stock, and what the same test gave on the commit before the
per-thread shifts (bn_reduce_kernel) and the checked shift (bn_finalize_kernel), where 24 of 66 failed (the 66 that leave out ``sampled`` at one and two rows and the overflowing shift).  No
constant here is tuned: the floors are the existing tests', the 4 is the yardstick's; the dead zone of 1e-3 sigma is a
thousand times the 1e-6 sigma that the statistics may be off by, and far too thin to hide a wrong gradient (0.1 % of the
elements).
"""
import copy

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import bn_conditioning_cases as K
from ips_amd import hip
from ips_amd.training import fused_encoder

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS, MOM = 1e-5, 0.1

B_FWD = {"mean": 1e-6, "invstd": 1e-6, "y": 2e-6, "running_mean": 1e-6, "running_var": 1e-6,
         "dx": 2e-5, "dres": 2e-5, "dgamma": 2e-5, "dbeta": 2e-5}
B_PART = dict(B_FWD, invstd=2e-6, y=5e-6, running_var=2e-6)


def _err(kind, t, ref, var64=None, scale=None):
    t, ref = t.detach().double(), ref.detach().double()
    if kind == "mean":
        return float(((t - ref).abs() / torch.sqrt(var64 + EPS)).max())
    if kind == "invstd":
        return float((t / ref - 1).abs().max())
    return float((t - ref).abs().max() / (ref.abs().max().clamp_min(1e-300) if scale is None else scale))


class _Log:
    def __init__(self, floors):
        self.floors, self.rows = floors, []

    def check(self, what, kind, fused, stock, ref, var64=None, scale=None):
        ef, es = _err(kind, fused, ref, var64, scale), _err(kind, stock, ref, var64, scale)
        print("%-46s %-12s fused %.3e   stock %.3e   floor %.0e" % (what, kind, ef, es, self.floors[kind]))
        self.rows.append((what, kind, ef, es))

    def assert_all(self):
        bad = [r for r in self.rows if not r[2] <= max(self.floors[r[1]], 4.0 * r[3])]
        assert not bad, bad


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _bn(c, res, gamma, beta, rm, rv, relu, dy, dtype, dead=None):
    """[relu](batch_norm(c) [+ res]) and its gradients by ATen's op and autograd in ``dtype``; rm / rv are updated in place.
    -> dict; ``dead``: where dy is zeroed (the float64 run returns it, the others are given it)."""
    ct = c.detach().to(dtype).clone().requires_grad_()
    gt, bt = gamma.detach().to(dtype).clone().requires_grad_(), beta.detach().to(dtype).clone().requires_grad_()
    rt = res.detach().to(dtype).clone().requires_grad_() if res is not None else None
    rmt, rvt = rm.to(dtype), rv.to(dtype)
    pre, mean, invstd = torch.native_batch_norm(ct, gt, bt, rmt, rvt, True, MOM, EPS)
    if rt is not None:
        pre = pre + rt
    y = torch.relu(pre) if relu else pre
    if dead is None:
        # 1e-3 sigma of the normalised term - or, where that is more, what storing the mean in float32 costs it (2^-22 |mean|
        # invstd: the one case where it is more is ``tight``, 2.4e-2)
        zone = torch.maximum(torch.full_like(mean, 1e-3), 2.0 ** -22 * mean.detach().abs() * invstd.detach()) * gt.detach().abs()
        dead = (pre.detach().abs() < zone.view(1, -1, 1, 1)) if relu else torch.zeros_like(pre, dtype=torch.bool)
    dyt = dy.to(dtype).masked_fill(dead, 0.0)
    y.backward(dyt)
    rm.copy_(rmt)
    rv.copy_(rvt)
    return {"y": y.detach(), "pre": pre.detach(), "mean": mean, "invstd": invstd, "running_mean": rmt, "running_var": rvt,
            "dx": ct.grad, "dres": rt.grad if rt is not None else None, "dgamma": gt.grad, "dbeta": bt.grad, "dead": dead}


def _params(C, shape, seed, res):
    g = torch.Generator(device="cpu").manual_seed(seed)
    gamma, beta = (torch.rand(C, generator=g) + 0.5).to(DEV), torch.randn(C, generator=g).to(DEV)
    dy = _cl(torch.randn(shape, generator=g)).to(DEV)
    r = _cl(torch.randn(shape, generator=g)).to(DEV) if res else None
    rm, rv = torch.randn(C, generator=g).to(DEV), (torch.rand(C, generator=g) + 0.5).to(DEV)
    return gamma, beta, dy, r, rm, rv


def _masks_agree(y, ref):
    live = ~ref["dead"]
    assert torch.equal((y > 0)[live], (ref["pre"] > 0)[live])


# ---------------------------------------------------------------- bn_reduce_kernel<false>: the standalone kernel
# (P, C, H): cg = 2 | cg = 1, 256 row lanes, a second slab of one row | cg = 256, one row lane | one row beyond the
# 512-slab cap | one row | two rows
SHAPES = [(64, 8, 8), (1025, 4, 1), (16, 1024, 2), (32769, 64, 1), (1, 64, 1), (2, 64, 1)]
CASES = {
    "well": lambda s: K.well(*s), "row0 +50": lambda s: K.row0(*s), "row0 -200": lambda s: K.row0(*s, value=-200.0),
    "head8": lambda s: K.head8(*s), "last": lambda s: K.last(*s), "tight": lambda s: K.tight(*s), "const": lambda s: K.const(*s),
    "sampled row0": lambda s: K.sampled(*s, "row0"), "sampled slabs": lambda s: K.sampled(*s, "slabs"),
    "sampled lanes": lambda s: K.sampled(*s, "lanes"),
}


def _standalone(x, what, log):
    C = x.shape[1]
    var64 = K.rows(x).double().var(0, unbiased=False) if x.shape[0] * x.shape[2] * x.shape[3] > 1 else torch.zeros(C, dtype=torch.float64, device=x.device)
    for relu in (True, False):
        for res in (False, True):
            tag = "%s relu %d res %d" % (what, relu, res)
            gamma, beta, dy, r, rm0, rv0 = _params(C, x.shape, 7 + 2 * relu + res, res)
            rm64, rv64, rm32, rv32, rmf, rvf = (t.clone() for t in (rm0.double(), rv0.double(), rm0, rv0, rm0, rv0))
            ref = _bn(x, r, gamma, beta, rm64, rv64, relu, dy, torch.float64)
            stock = _bn(x, r, gamma, beta, rm32, rv32, relu, dy, torch.float32, ref["dead"])
            y, mean, invstd = hip.bn_train_forward(x, r, gamma, beta, EPS, MOM, rmf, rvf, relu)
            dyf = _cl(dy.masked_fill(ref["dead"], 0.0))
            dx, dres, dgamma, dbeta = hip.bn_train_backward(dyf, y if relu else None, x, gamma, mean, invstd, relu, res)
            got = {"y": y, "mean": mean, "invstd": invstd, "running_mean": rmf, "running_var": rvf, "dx": dx, "dres": dres,
                   "dgamma": dgamma, "dbeta": dbeta}
            # (dx at one and two rows: relative to the terms that cancel in it, see the module's docstring)
            terms = float((dyf.double() * (gamma.double() * ref["invstd"]).view(1, -1, 1, 1)).abs().max())
            for kind in ("mean", "invstd", "y", "running_mean", "running_var", "dx", "dres", "dgamma", "dbeta"):
                if kind == "running_var" and K.rows(x).shape[0] == 1:
                    # one row: ATen's unbiased variance is 0 / 0; the kernel keeps the biased one, 0
                    assert _err("running_var", rvf, 0.9 * rv0.double()) <= B_FWD["running_var"]
                elif got[kind] is not None:
                    log.check(tag, kind, got[kind], stock[kind], ref[kind], var64,
                              terms if kind == "dx" and K.rows(x).shape[0] <= 2 else None)
            if relu:
                _masks_agree(y, ref)
            y2, mean2, invstd2 = hip.bn_train_forward(x, r, gamma, beta, EPS, MOM, rm0.clone(), rv0.clone(), relu)
            assert torch.equal(y, y2) and torch.equal(mean, mean2) and torch.equal(invstd, invstd2)      # deterministic


def _combinations():
    """Every case at every shape.  (``sampled`` at one row, and ``sampled lanes`` at two, put every row on the ladder: no
    row is left for the sample to be atypical of, and the kernels are held to the same bounds there all the same.)"""
    for case in CASES:
        for shape in SHAPES:
            yield pytest.param(case, shape, id="%s-%dx%dx%d" % ((case.replace(" ", "_"),) + shape))


@pytest.mark.parametrize("case,shape", list(_combinations()))
def test_standalone_kernel_on_atypical_shift_rows(case, shape):
    """``hip.bn_train_forward`` + ``hip.bn_train_backward`` (with the forward's own saved statistics) across relu x res.
    Measured, worst over the six shapes and relu x res, fused | stock (before: fused):
      case            invstd                          y                               dgamma
      well            1.2e-7 | 1.3e-7 (3.8e-7)        1.8e-6 | 1.8e-6 (1.8e-6)        2.2e-6 | 2.1e-6 (2.2e-6)
      row0 +50        3.7e-7 | 1.6e-7 (2.9e-4)        3.1e-7 | 1.7e-7 (2.8e-4)        8.5e-7 | 1.1e-7 (2.1e-4)
      row0 -200       3.9e-7 | 1.6e-7 (6.4e-4)        3.0e-7 | 1.3e-7 (5.0e-4)        2.0e-6 | 1.0e-7 (6.4e-4)
      head8           1.2e-7 | 1.3e-7 (5.1e-5)        2.0e-7 | 1.3e-7 (4.8e-5)        6.8e-7 | 2.1e-7 (5.4e-5)
      last            1.6e-7 | 1.6e-7 (1.7e-7)        2.0e-7 | 1.7e-7 (1.7e-7)        4.3e-7 | 1.7e-7 (2.8e-7)
      tight           1.0e-7 | 3.3e-4 (2.0e-6)        4.3e-3 | 4.3e-3 (4.3e-3)        1.1e-2 | 1.1e-2 (1.1e-2)
      const           1.2e-7 | 1.3e-7 (2.3e-7)        3.2e-7 | 3.2e-7 (3.2e-7)        9.2e-7 | 9.2e-7 (9.2e-7)
      sampled row0    3.0e-7 | 1.4e-7 (1.7e-4)        2.7e-7 | 1.2e-7 (1.7e-4)        1.1e-6 | 1.2e-7 (5.8e-5)
      sampled slabs   1.6e-7 | 1.4e-7 (8.7e-7)        1.3e-7 | 8.2e-8 (8.5e-7)        3.0e-7 | 1.4e-7 (9.5e-7)
      sampled lanes   1.6e-7 | 1.4e-7 (3.5e-7)        1.3e-7 | 8.0e-8 (2.0e-7)        3.9e-7 | 5.7e-8 (7.0e-7)
    mean: 4.6e-7 | 9.8e-9 (5.6e-6) at row0 +50 - the slab's sum is handed on in float32 around its first row, the outlier -
    6.8e-6 | 6.8e-6 at two rows and 9.6e-3 | 9.6e-3 on ``tight``: float32 storage of the mean, the same in both.
    At (1, 64, 1) and (2, 64, 1), where ``sampled`` leaves one row or none outside the sample (row0 and slabs are the
    same rows there): invstd 1.1e-7 | 1.2e-7, y 5.9e-8 | 5.9e-8, running_var 1.6e-7 | 1.3e-7, dgamma 6.7e-8 | 8.9e-8.  dx
    at those two shapes, relative to max |dy gamma invstd64| (the module's docstring): 0 | 0 at one row; at two rows
    sampled row0 2.0e-7 | 8.4e-8, sampled lanes 1.3e-7 | 5.9e-8, row0 +50 / -200 1.3e-7 | 1.3e-7 and 1.5e-7 | 1.8e-7, well
    6.5e-6 | 6.4e-6, tight 4.6e-3 | 4.6e-3.  (Relative to max |dx64|, sampled row0 at two rows is 2.6e-4 | 1.8e-5 and
    row0 1.2e+1 | 1.2e+1: rounding measured against what eps / var leaves of the terms.)
    """
    x = CASES[case](shape).x.to(DEV)
    log = _Log(B_FWD)
    _standalone(x, "%s %s" % (case, shape), log)
    if case == "const":
        y, mean, invstd = hip.bn_train_forward(x, None, torch.ones(shape[1], device=DEV), torch.zeros(shape[1], device=DEV), EPS, MOM, None, None, False)
        assert float(mean[0]) == K.CONST and abs(float(invstd[0]) * EPS ** 0.5 - 1.0) <= B_FWD["invstd"]
        assert float(y[:, 0].abs().max()) == 0.0
    log.assert_all()


# ---------------------------------------------------------------- the convolutions' epilogues: the conv + BN node
# the four LDS-resident layer shapes of test_hip_train.py::test_conv_epilogue_statistics_feed_the_batch_norm
LAYERS = [(64, 64, 3, 1, 8), (128, 128, 3, 1, 4), (64, 128, 3, 2, 8), (64, 128, 1, 2, 8)]


def _selection_conv(ci, co, k, s):
    """A convolution whose centre tap is a 0 / 1 selection matrix and whose other taps are 0: its output IS the input,
    channel co reading ci = co % C_in (at every s-th pixel) - exactly, so that the crafted batch reaches the BatchNorm."""
    conv = nn.Conv2d(ci, co, k, s, k // 2, bias=False).to(DEV)
    with torch.no_grad():
        conv.weight.zero_()
        conv.weight[torch.arange(co), torch.arange(co) % ci, k // 2, k // 2] = 1.0
    return conv


def _fresh_bn(co, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    bn = nn.BatchNorm2d(co, eps=EPS, momentum=MOM).to(DEV).train()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(co, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(co, generator=g))
        bn.running_mean.copy_(torch.randn(co, generator=g))
        bn.running_var.copy_(torch.rand(co, generator=g) + 0.5)
    return bn


def _node_step(conv, bn, x, what, log, twins, relu=True, res=True, seed=3, expect=None):
    """One training step of ``fused_encoder.conv_bn_act`` on ``x`` against the same BatchNorm, in float64 and in stock
    float32, of the convolution's output (the node's own, bit for bit: ``hip.conv2d_nhwc``).  ``twins`` = (rm64, rv64, rm32,
    rv32): the running statistics of the two references, carried from step to step like the module's."""
    assert hip.conv_lds_supported(conv, x.shape[2], x.shape[3])
    c = hip.conv2d_nhwc(x, conv.weight.detach(), conv.stride[0], conv.padding[0])
    if expect is not None:
        assert torch.equal(c, expect)
    gamma, beta = bn.weight.detach(), bn.bias.detach()
    _, _, dy, r, _, _ = _params(c.shape[1], c.shape, seed, res)
    ref = _bn(c, r, gamma, beta, twins[0], twins[1], relu, dy, torch.float64)
    stock = _bn(c, r, gamma, beta, twins[2], twins[3], relu, dy, torch.float32, ref["dead"])
    for p in (conv.weight, bn.weight, bn.bias):
        p.grad = None
    xs = x.clone().requires_grad_(x.shape[1] > 1)
    rs = r.clone().requires_grad_() if res else None
    y = fused_encoder.conv_bn_act(conv, bn, xs, None, rs, relu)
    y.backward(_cl(dy.masked_fill(ref["dead"], 0.0)))
    var64 = K.rows(c).double().var(0, unbiased=False)
    got = {"y": y, "mean": bn._ipsx_batch_mean, "running_mean": bn.running_mean, "running_var": bn.running_var,
           "dres": rs.grad if res else None, "dgamma": bn.weight.grad, "dbeta": bn.bias.grad}
    for kind in ("mean", "y", "running_mean", "running_var", "dres", "dgamma", "dbeta"):
        if got[kind] is not None:
            log.check(what, kind, got[kind], stock[kind], ref[kind], var64)
    # invstd is not handed out by the node: running_var = 0.9 rv + 0.1 var n / (n - 1) holds it, and y
    if xs.requires_grad:                                  # the node's dx = the data gradient of the BatchNorm's dx
        def dgrad(dc, dtype):
            xt = x.detach().to(dtype).clone().requires_grad_()
            F.conv2d(xt, conv.weight.detach().to(dtype), None, conv.stride, conv.padding).backward(dc.to(dtype))
            return xt.grad
        log.check(what, "dx", xs.grad, dgrad(stock["dx"], torch.float32), dgrad(ref["dx"], torch.float64))
    if relu:
        _masks_agree(y, ref)
    assert bool(torch.isfinite(y).all())
    return y


def _twins(bn):
    return bn.running_mean.double().clone(), bn.running_var.double().clone(), bn.running_mean.clone(), bn.running_var.clone()


def _selected(x, conv):
    co, ci, s = conv.out_channels, conv.in_channels, conv.stride[0]
    return _cl(x[:, torch.arange(co, device=x.device) % ci][:, :, ::s, ::s])


@pytest.mark.parametrize("ci,co,k,s,H", LAYERS)
def test_conv_bn_node_first_step_behind_a_bright_first_patch(ci, co, k, s, H):
    """``patch0`` at a fresh module: the first-step shift is the channel means of the convolution of the FIRST patch, here
    50 sigma above the rest (1,024 patches: only there does that reach ~30 batch-sigma).  And ``well`` as the control.
    Measured, worst of the four layers, fused | stock (before: fused): patch0 y 1.7e-7 | 1.7e-7 (8.1e-6), running_var
    7.1e-8 | 9.7e-8 (3.9e-6), dx 1.7e-7 | 1.7e-7 (7.8e-6), dgamma 1.4e-7 | 2.2e-7 (5.5e-6), mean 1.8e-9 | 5.0e-9 (3.4e-7);
    well y 1.5e-7 | 1.3e-7, running_var 7.2e-8 | 8.5e-8.
    """
    for name, case in (("patch0", K.patch0(1024, ci, H)), ("well", K.well(1024, ci, H))):
        x = case.x.to(DEV)
        conv, bn = _selection_conv(ci, co, k, s), _fresh_bn(co, 11)
        assert not hasattr(bn, "_ipsx_batch_mean")
        log = _Log(B_PART)
        _node_step(conv, bn, x, "%s %d->%d %dx%d/%d" % (name, ci, co, k, k, s), log, _twins(bn), expect=_selected(x, conv))
        log.assert_all()


@pytest.mark.parametrize("ci,co,k,s,H", LAYERS)
def test_conv_bn_node_over_a_jump_between_two_steps(ci, co, k, s, H):
    """``jump``: the second step's shift is the first step's batch mean, 50 sigma from the second batch; then ``const`` as
    the second step of a ``jump`` (behind the stale shift a channel of variance 0, where invstd = 1 / sqrt(eps) multiplies
    whatever is left of the mean's error).
    Measured at the second step, worst of the four layers, fused | stock (before: fused): jump y 5.1e-7 | 1.2e-6 (7.0e-5),
    running_var 1.3e-7 | 1.9e-7 (3.9e-5), dx 1.3e-7 | 3.7e-7 (9.2e-5), dgamma 2.0e-6 | 3.1e-6 (9.9e-5), mean 2.6e-6 | 6.5e-6
    (5.4e-6: float32 storage of a mean 50 sigma from zero); jump, const y 1.2e-7 | 1.2e-7, running_var 1.5e-7 | 1.5e-7,
    mean 2.5e-8 | 1.0e-8.
    """
    for name, case in (("jump", K.jump(64, ci, H)), ("jump, const", K.jump_const(64, ci, H))):
        conv, bn = _selection_conv(ci, co, k, s), _fresh_bn(co, 12)
        twins = _twins(bn)
        log = _Log(B_PART)
        for step, xb in enumerate(case.x):
            x = xb.to(DEV)
            _node_step(conv, bn, x, "%s step %d %d->%d %dx%d/%d" % (name, step, ci, co, k, k, s), log, twins, seed=3 + step,
                       expect=_selected(x, conv))
        log.assert_all()


def test_stem_node_behind_an_offset_first_patch_over_two_steps():
    """The 1 -> 64, 7 x 7 / 2 stem on 32-px patches with patch 0 of the input offset by a constant (every channel of the
    first patch's output moves by that constant times the channel's weight sum), two steps: the first-patch shift, then
    the previous step's mean against a batch whose bright patch has gone.
    Measured, fused | stock (before: fused): step 0 y 1.4e-7 | 1.4e-7 (4.6e-6), running_var 4.0e-8 | 6.3e-8 (4.7e-6), dgamma
    1.2e-7 | 1.3e-7 (3.9e-6); step 1 y 1.0e-7 | 9.9e-8 (1.2e-7), running_var 7.2e-8 | 7.2e-8 (4.7e-6).
    """
    g = torch.Generator(device="cpu").manual_seed(21)
    conv = nn.Conv2d(1, 64, 7, 2, 3, bias=False).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / 7.0 + 0.05)
    bn = _fresh_bn(64, 13)
    twins = _twins(bn)
    log = _Log(B_PART)
    for step in range(2):
        x = torch.randn((256, 1, 32, 32), generator=g)
        x[0] += 50.0 if step == 0 else 0.0
        x = x.to(DEV)
        x = x.as_strided(x.shape, (32 * 32, 1, 32, 1))               # (one channel: the channels-last strides spelled out)
        _node_step(conv, bn, x, "stem step %d" % step, log, twins, res=False, seed=5 + step)
    log.assert_all()


# ---------------------------------------------------------------- a non-finite step must not outlive its cause
def _restorable_layer():
    ci, co, k, s, H = LAYERS[0]
    g = torch.Generator(device="cpu").manual_seed(31)
    conv = nn.Conv2d(ci, co, k, s, k // 2, bias=False).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / (ci * k * k)) ** 0.5)
    layer = nn.Sequential(conv, _fresh_bn(co, 14))
    x = _cl(torch.randn((32, ci, H, H), generator=g) + 0.5).to(DEV)
    return layer, x


def _nan_step(layer, x):
    bad = x.clone()
    bad[3, 5, 2, 2] = float("nan")
    fused_encoder.conv_bn_act(layer[0], layer[1], bad, None, None, True)
    # (the 3 x 3 convolution spreads the NaN over every channel: every batch mean is NaN, and the running statistics with it)
    assert bool(torch.isnan(layer[1]._ipsx_batch_mean).all()) and bool(torch.isnan(layer[1].running_mean).all())


def test_a_non_finite_step_is_over_once_the_state_is_restored():
    """Save the state dict, run one step on a batch that holds a NaN, load the state dict back, run a clean batch: finite and
    inside the bounds - the previous step's batch mean, which the layer keeps as the next shift, is NaN then and must not
    be used.  The same after ``copy.deepcopy`` of a module that has seen the NaN step.
    Measured, fused | stock, the same for the module and for its deep copy: y 9.5e-8 | 1.0e-7, mean 4.2e-8 | 7.0e-8,
    running_var 9.3e-8 | 7.1e-8, dx 7.8e-7 | 3.6e-7, dgamma 9.0e-8 | 2.0e-7.  Before: mean NaN, y 1.0 (all of it), dx NaN.
    """
    layer, x = _restorable_layer()
    saved = copy.deepcopy(layer.state_dict())
    _nan_step(layer, x)
    clone = copy.deepcopy(layer)
    for what, mod in (("restored", layer), ("deep copy, restored", clone)):
        mod.load_state_dict(saved)
        log = _Log(B_PART)
        _node_step(mod[0], mod[1], x, what, log, _twins(mod[1]))
        log.assert_all()
        assert bool(torch.isfinite(mod[1].running_mean).all()) and bool(torch.isfinite(mod[1].running_var).all())
        _node_step(mod[0], mod[1], x, what + ", next step", log, _twins(mod[1]))      # (and the shift it left is a good one)
        log.assert_all()


def test_a_finite_shift_whose_square_overflows_is_not_used():
    """A shift that is finite but so far out that d^2 = (x - shift)^2 overflows float32 (3e19): the epilogue's sum of
    squares is inf, var = inf would satisfy E[d]^2 <= 4 var, and invstd would come out 0 without a word.  The channel is
    summed again, around row 0 - the mean found behind such a shift is rounding debris of the shift's size (1e12).
    Measured, fused | stock: y 9.5e-8 | 1.0e-7, mean 4.2e-8 | 7.0e-8, running_var 8.6e-8 | 6.3e-8, dx 7.8e-7 | 3.4e-7,
    dgamma 9.0e-8 | 2.0e-7.
    """
    layer, x = _restorable_layer()
    log = _Log(B_PART)
    _node_step(layer[0], layer[1], x, "first step", log, _twins(layer[1]))
    layer[1]._ipsx_batch_mean = torch.full_like(layer[1].running_mean, 3e19)
    _node_step(layer[0], layer[1], x, "behind a shift of 3e19", log, _twins(layer[1]))
    log.assert_all()


# ---------------------------------------------------------------- the projector's column sums
@pytest.mark.parametrize("rows,f,d", [(4096, 64, 64), (130, 256, 256)])
def test_projector_columns_behind_eight_far_rows(rows, f, d):
    """``hip.projector_train_forward`` + ``bn_train_forward_partials`` on rows whose first eight are one repeated row and the
    rest near-duplicates of another (``K.projector_rows``): the columns of z have a small sigma and the shift - the mean
    of those eight rows - lies sqrt(rows / 8) sigma off.  Column mean and invstd against float64 LayerNorm + Linear (stock:
    the same in float32, then ATen's batch norm), and against the float64 statistics of the z the kernel wrote (stock:
    ATen's float32 batch norm of that z) - the second is the BatchNorm's own share, at the floors.
    Measured, worst of the two shapes, fused | stock (before: fused): of its own z invstd 1.3e-7 | 1.8e-6 (2.7e-5), y 1.9e-6 |
    2.0e-6 (1.9e-5), mean 1.4e-5 | 1.4e-5 (1.4e-5: float32 storage, |mean| / sigma = 500); against LayerNorm + Linear
    invstd 1.4e-5 | 1.1e-5 (2.7e-5), mean 3.6e-5 | 1.3e-5 (3.6e-5) - the float32 GEMM's error over a column sigma of 1e-3.
    """
    g = torch.Generator(device="cpu").manual_seed(41)
    x = K.projector_rows(rows, f).to(DEV)
    w, b = (torch.randn((d, f), generator=g) / f ** 0.5).to(DEV), (0.1 * torch.randn(d, generator=g)).to(DEV)
    gamma, beta = (torch.rand(d, generator=g) + 0.5).to(DEV), torch.randn(d, generator=g).to(DEV)

    def stock_path(dtype):
        z = F.linear(F.layer_norm(x.to(dtype), (f,), None, None, 1e-5), w.to(dtype), b.to(dtype))
        _, mean, invstd = torch.native_batch_norm(z, gamma.to(dtype), beta.to(dtype), None, None, True, MOM, EPS)
        return z, mean, invstd

    z64, mean64, inv64 = stock_path(torch.float64)
    z32, mean32, inv32 = stock_path(torch.float32)
    z, stats, partial, slabs, shift = hip.projector_train_forward(x, w, b, 1e-5)
    rm, rv = torch.zeros(d, device=DEV), torch.ones(d, device=DEV)
    y, mean, invstd = hip.bn_train_forward_partials(z, None, gamma, beta, EPS, MOM, rm, rv, False, partial, slabs, shift)
    off = ((shift.double() - mean64).abs() * inv64)
    print("shift rows: %.1f .. %.1f column sigma from the column mean" % (float(off.min()), float(off.max())))
    assert float(off.median()) >= 0.9 * (rows / 8) ** 0.5
    log = _Log(B_PART)
    var64 = z64.var(0, unbiased=False)
    what = "projector (%d, %d, %d)" % (rows, f, d)
    log.check(what + " vs LayerNorm + Linear", "mean", mean, mean32, mean64, var64)
    log.check(what + " vs LayerNorm + Linear", "invstd", invstd, inv32, inv64)
    zd = z.double()
    y_own, mean_own, inv_own = torch.native_batch_norm(zd, gamma.double(), beta.double(), None, None, True, MOM, EPS)
    y_st, mean_st, inv_st = torch.native_batch_norm(z, gamma, beta, None, None, True, MOM, EPS)
    log.check(what + " vs float64 of its own z", "mean", mean, mean_st, mean_own, zd.var(0, unbiased=False))
    log.check(what + " vs float64 of its own z", "invstd", invstd, inv_st, inv_own)
    log.check(what + " vs float64 of its own z", "y", y, y_st, y_own)
    log.assert_all()
