"""Seeded activations on which a training-mode BatchNorm's batch statistics are hard to get right, shared by
tests/test_bn_conditioning_cases_cpu.py (the cases are what they claim to be, and stock float32 handles them) and
tests/test_bn_train_conditioning.py (libipsx's kernels handle them).

Every producer of batch statistics here (csrc/bn_train.hip bn_reduce_kernel, the convolutions' epilogues, the projector)
sums d = x - shift and d^2 in float32 and forms var = E[d^2] - E[d]^2; that loses (E[d]^2 / var) * 2^-24 of the variance
per rounding, so it is as good as the shift is near the channel mean.  The shifts are SAMPLES of the data - row 0, the
first 8 rows, the first patch, the previous batch - and each case below makes exactly such a sample atypical.

A builder returns ``Case(x, prop)``: ``x`` a float32 channels-last (P, C, H, H) tensor on the CPU (``jump``: a tuple of
two), ``prop`` the declared property as a dict of float64 numbers, which the CPU test asserts.  "Rows" are the (P * H * H)
pixels in memory order, as the kernels see them: row = (p * H + h) * H + w.
"""
from collections import namedtuple

import torch

Case = namedtuple("Case", "x prop")

OUTLIER = 50.0            # sigma units of the N(0, 1) bulk


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _cl(x):
    return x.contiguous(memory_format=torch.channels_last)


def rows(x):
    """(P, C, H, H) -> the (P * H * H, C) rows in memory order (a view of a channels-last tensor)."""
    r = x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])
    assert r.data_ptr() == x.data_ptr(), "not channels-last: the rows would be a copy"
    return r


def _bulk(P, C, H, seed):
    return _cl(torch.randn((P, C, H, H), generator=_gen(seed)))


def offset_in_sigmas(x, idx):
    """How atypical the rows ``idx`` are, per channel, in float64: (their mean - the mean of the other rows) in units of
    the other rows' sigma (``rest``) and of the whole batch's sigma (``batch``: at most sqrt(rows / len(idx))).  Worst
    (smallest) channel of each."""
    r = rows(x).double()
    pick = torch.zeros(r.shape[0], dtype=torch.bool)
    pick[idx] = True
    sample, rest = r[pick], r[~pick]
    delta = (sample.mean(0) - rest.mean(0)).abs()
    return {"rest": float((delta / rest.std(0, unbiased=False)).min()),
            "batch": float((delta / r.std(0, unbiased=False)).min())}


def well(P, C, H, seed=1):
    x = _cl(torch.randn((P, C, H, H), generator=_gen(seed)) * 2 + 3)
    r = rows(x).double()
    return Case(x, {"mean_over_sigma": float((r.mean(0) / r.std(0, unbiased=False)).abs().max()) if r.shape[0] > 1 else 0.0})


def row0(P, C, H, value=OUTLIER, seed=2):
    """N(0, 1); the first pixel of the first patch at ``value`` in every channel."""
    x = _bulk(P, C, H, seed)
    x[0, :, 0, 0] = value
    return Case(x, offset_in_sigmas(x, [0]) if P * H * H > 1 else {})


def head8(P, C, H, value=OUTLIER, seed=3):
    """N(0, 1); the first 8 rows at ``value`` (what the projector's shift is the mean of)."""
    x = _bulk(P, C, H, seed)
    k = min(8, P * H * H)
    rows(x)[:k] = value
    return Case(x, offset_in_sigmas(x, list(range(k))) if P * H * H > k else {})


def patch0(P, C, H, value=OUTLIER, seed=4):
    """N(0, 1); every pixel of patch 0 at ``value`` (what a convolution's first-step shift is the mean of)."""
    x = _bulk(P, C, H, seed)
    x[0] = value
    return Case(x, offset_in_sigmas(x, list(range(H * H))) if P > 1 else {})


def last(P, C, H, value=OUTLIER, seed=2):
    """The ``row0`` outlier at the last row instead: no shift is taken there, it must not matter."""
    x = _bulk(P, C, H, seed)
    x[-1, :, -1, -1] = value
    return Case(x, offset_in_sigmas(x, [P * H * H - 1]) if P * H * H > 1 else {})


def jump(P, C, H, sigmas=OUTLIER, seed=5):
    """Two batches, the second the first plus ``sigmas`` of its channel's sigma: the previous batch's mean is a stale shift."""
    a = _bulk(P, C, H, seed) * 1.5 + 0.25
    sd = rows(a).double().std(0, unbiased=False)
    b = _cl((a.double() + (sigmas * sd).view(1, -1, 1, 1)).float())
    d = (rows(b).double().mean(0) - rows(a).double().mean(0)).abs() / rows(b).double().std(0, unbiased=False)
    return Case((a, b), {"stale": float(d.min())})


def tight(P, C, H, seed=6):
    """1000 + 0.01 N(0, 1): row 0 is typical, the MEAN is 10^5 sigma from zero.  float32 cannot even store the mean to
    better than 2^-24 * 1000 = 6e-3 sigma, so stock float32 is far outside the floors here too: the case pins that a
    shifted sum does no worse than that (the bound's 4 x stock term is what it is held to)."""
    x = _cl(1000 + 0.01 * torch.randn((P, C, H, H), generator=_gen(seed)))
    r = rows(x).double()
    out = {"mean_over_sigma": float((r.mean(0) / r.std(0, unbiased=False).clamp_min(1e-30)).abs().min()) if r.shape[0] > 1 else 0.0}
    if r.shape[0] > 1:
        out["row0"] = float(((r[0] - r.mean(0)).abs() / r.std(0, unbiased=False)).max())
    return Case(x, out)


CONST = 3.25


def const(P, C, H, seed=7):
    """Channel 0 constant 3.25 (variance 0: invstd = 1 / sqrt(eps) exactly), the others N(0, 1)."""
    x = _bulk(P, C, H, seed)
    x[:, 0] = CONST
    return Case(x, {"var0": float(rows(x).double().var(0, unbiased=False)[0])})


def jump_const(P, C, H, seed=5):
    """``jump`` whose second batch is ``const``: behind a stale shift a channel of variance 0."""
    a = jump(P, C, H, seed=seed).x[0]
    b = const(P, C, H).x
    return Case((a, b), {"var0": float(rows(b).double().var(0, unbiased=False)[0]),
                         "stale0": float((rows(a).double().mean(0)[0] - CONST).abs())})


LADDER = (1, 1.5, 1.9, 2.1, 2.5, 3, 3.9, 4.1, 6, 10, 30, 100, 300)


def ladder(C):
    """A different distance per channel, in sigma of the bulk: LADDER cycled, the sign alternating from cycle to cycle -
    channels on both sides of the 2 sigma at which bn_finalize_kernel sums a channel again, close to it, and far out."""
    i = torch.arange(C)
    return torch.tensor(LADDER)[i % len(LADDER)] * (1 - 2 * ((i // len(LADDER)) % 2)).float()


def bn_slab_cut(n, C):
    """csrc/bn_train.hip bn_shape(): (row lanes, rows per slab, slabs) of bn_reduce_kernel at ``n`` rows of ``C`` channels -
    written out here, not asked of the library, so that the ``sampled`` cases are what they say on a machine without it."""
    nrl = 256 // (C // 4)
    slabs = min(-(-n // (nrl * 4)), 512)
    slab = -(-n // slabs)
    return nrl, slab, -(-n // slab)


def sampled_rows(n, C, which):
    """The rows bn_reduce_kernel<false> / bn_finalize_slabs_kernel shift by after this work.  ``lanes``: the first row
    every THREAD reads (row lane j of slab g starts at g * slab + j) - its own shift.  ``slabs``: the first row of every
    slab, around which the slab's sum is handed on in float32.  ``row0``: row 0, around which the slabs are combined."""
    nrl, slab, slabs = bn_slab_cut(n, C)
    if which == "row0":
        return [0]
    if which == "slabs":
        return [g * slab for g in range(slabs)]
    return [g * slab + j for g in range(slabs) for j in range(min(nrl, min(slab, n - g * slab)))]


def sampled(P, C, H, which, seed=8):
    """Whatever rows a shift is taken from, this case puts the outliers on exactly those: ``sampled_rows(.., which)`` of
    the standalone kernel, each at ``ladder(C)`` sigma (``lanes`` is a quarter of all rows or less: the batch turns
    bimodal and the sample is at most 2 batch-sigma off - a sample that large cannot be far from the batch).  For the
    other producers the sample rows are what ``head8`` (projector), ``patch0`` and ``jump`` (convolutions) already hit."""
    x = _bulk(P, C, H, seed)
    idx = sampled_rows(P * H * H, C, which)
    rows(x)[idx] = ladder(C)
    out = {"rows": len(idx), "of": P * H * H}
    if len(idx) < P * H * H:
        out.update(offset_in_sigmas(x, idx))
        pick = torch.zeros(P * H * H, dtype=torch.bool)
        pick[idx] = True
        d = (rows(x)[pick].double().mean(0) - rows(x)[~pick].double().mean(0)).abs() / rows(x)[~pick].double().std(0, unbiased=False)
        out["rest_max"] = float(d.max())
    return Case(x, out)


def projector_rows(n, f, seed=9, head=8, spread=1e-3):
    """(n, f) feature rows for LayerNorm + Linear + BatchNorm1d: the first ``head`` rows are ONE repeated row, the others
    near-duplicates of ANOTHER row (a perturbation of ``spread`` of that row's spread).  The columns of z then have a
    small sigma, and the shift rows sit far from their mean."""
    g = _gen(seed)
    a, b = torch.randn(f, generator=g) * 2 + 0.5, torch.randn(f, generator=g) * 2 + 0.5
    x = b.repeat(n, 1) + spread * float(b.std()) * torch.randn((n, f), generator=g)
    x[:min(head, n)] = a
    return x.contiguous()
