"""scan_mnist_kernel (csrc/scan_mnist.hip): the selection loop specialised for 8 heads x 4 query tokens, M = I = 64, against
the oracle's loop (orc_scores_from_logits + orc_topm / orc_topm_loop) and against scan_fast_kernel (through the diagnostic
switch ipsx_dbg_scan_mnist): indices exactly, scores bit for bit, tie flags, in both tie orders, as one launch and cut
into resumed ranges; conditional and persistent launches.

The kernel has no survivor cap: every iteration ranks all of its (at most 128) candidates on their 64-bit keys."""

import numpy as np
import pytest
import torch

from ips_amd import hip
from oracle import oracle as orc
from tests.util import ulp_diff

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M = I = 64
H, T = 8, 4
R = H * T
MODES = (("torch", True), ("canonical", False))


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)          # (a copy: the cached logits are read-only)


def _continuous(B, N):
    return (np.random.default_rng(7000 + 10 * N + B).standard_normal((B, N, R)) * 3.0).astype(np.float32)


def _quantised(levels, same):
    if same:
        B, N = 2, M + 5 * I + 17
        g = np.random.default_rng(8001 + 2 * levels)
        lg = (g.integers(0, levels, (B, N, R)).astype(np.float32) - 1.0) * np.float32(0.75)
        lg[:, :, 1:] = lg[:, :, :1]                       # every row equal across (h, t): whole candidates tie
        return lg
    # 32 independent levels per row: no two rows are equal, and two DIFFERENT rows whose scores collide in the last bit at the
    # boundary of the memory are rare - seeds found with the oracle on the CPU (one tied iteration among 23 of one image)
    B, N = 2, 1500
    g = np.random.default_rng(80000 + 10000 * levels + {2: 15, 3: 671, 5: 120, 17: 480}[levels])
    return (g.integers(0, levels, (B, N, R)).astype(np.float32) - 1.0) * np.float32(0.75)


def _survivors():
    B, N = 2, 1500
    lg = (np.random.default_rng(9001).standard_normal((B, N, R)) * 3.0).astype(np.float32)
    return lg + (np.arange(N, dtype=np.float32) * np.float32(0.01)).reshape(1, N, 1)      # scores grow along the scan


def _duplicates():
    lg = _continuous(2, M + 6 * I + 40)
    lg[:, 230:300] = lg[:, 90:160]                        # a stretch of rows again, across the chunk boundary at 256
    return lg


def _special():
    lg = _continuous(3, M + 5 * I + 30)
    lg[0, 40, 3] = np.nan
    lg[1, 7, 0] = np.inf
    lg[2, 100:110, 5] = -np.inf
    return lg


CONT_N = (65, 127, 128, 129, 64 + 5 * 64, 64 + 5 * 64 + 1, 64 + 5 * 64 + 63, 1500)
CASES = {}
for _b in (1, 3):
    for _n in CONT_N:
        CASES["cont-%d-%d" % (_b, _n)] = (_continuous, (_b, _n))
for _lv in (2, 3, 5, 17):
    for _same in (True, False):
        CASES["quant-%d-%s" % (_lv, "same" if _same else "free")] = (_quantised, (_lv, _same))
CASES["survivors"] = (_survivors, ())
CASES["duplicates"] = (_duplicates, ())
CASES["special"] = (_special, ())

_LOGITS, _ORACLE, _GPU = {}, {}, {}


def logits(name):
    if name not in _LOGITS:
        fn, args = CASES[name]
        _LOGITS[name] = fn(*args)
        _LOGITS[name].setflags(write=False)
    return _LOGITS[name]


def oracle_scan(name, aten):
    """The oracle's loop, image by image: final indices, final scores, tie flag of every iteration, and how many chunk
    candidates every iteration admitted into the memory.  Computed once per (case, tie order)."""
    if (name, aten) not in _ORACLE:
        lg = logits(name)
        L = orc.lib()
        out = []
        for b in range(lg.shape[0]):
            N = lg.shape[1]
            cur = np.arange(M, dtype=np.int64)
            ties, admitted, last = [], [], None
            for lo in range(M, N, I):
                cand = np.concatenate([cur, np.arange(lo, min(lo + I, N), dtype=np.int64)])
                s = np.empty(len(cand), dtype=np.float32)
                L.orc_scores_from_logits(orc._f(lg[b][cand])[1], len(cand), H, T, s.ctypes.data_as(orc.f32p), None)
                top, tie = orc.topm(s, M, aten_ties=aten, rows=lg[b][cand])
                ties.append(tie)
                admitted.append(int((top >= M).sum()))
                cur, last = cand[top], s[top]
            out.append((cur, last, ties, admitted))
        _ORACLE[(name, aten)] = out
    return _ORACLE[(name, aten)]


def gpu_scan(name, mode, kernel):
    """(indices, scores, tie flags, indices of the scan cut into two resumed ranges) of the default kernel ("mnist") or of
    scan_fast_kernel ("fast": the switch off).  Computed once per (case, tie order, kernel)."""
    key = (name, mode, kernel)
    if key not in _GPU:
        lg = dev(logits(name))
        B, N = lg.shape[:2]
        n_iter = -(-(N - M) // I)
        hip.set_tie_order(mode)
        hip.dbg_scan_mnist(kernel == "mnist")
        try:
            idx, sc = hip.scan(lg, M, I, H, T, want_scores=True)
            tie = hip.scan.last_tie
            cut = max(1, n_iter // 2)
            mem = torch.empty((B, M), dtype=torch.int64, device=DEV)
            tie2 = torch.zeros((B,), dtype=torch.int32, device=DEV)
            hip.scan_range(lg, M, I, H, T, 0, cut, mem, tie2)
            hip.scan_range(lg, M, I, H, T, cut, n_iter, mem, tie2)
            _GPU[key] = (idx.cpu().numpy(), sc.cpu().numpy(), tie.cpu().numpy(), mem.cpu().numpy(), tie2.cpu().numpy())
        finally:
            hip.dbg_scan_mnist(True)
            hip.set_tie_order("torch")
    return _GPU[key]


def _check_against_oracle(name, scores):
    for mode, aten in MODES:
        idx, sc, tie, mem2, tie2 = gpu_scan(name, mode, "mnist")
        want = oracle_scan(name, aten)
        for b, (cur, last, ties, _) in enumerate(want):
            assert np.array_equal(idx[b], cur), (name, mode, b)
            if scores:
                # (a NaN score has no bits to compare: the host's inf - inf is a negative NaN, the kernels return the canonical one)
                nan = np.isnan(last)
                assert np.array_equal(np.isnan(sc[b]), nan), (name, mode, b)
                assert nan.all() or ulp_diff(sc[b][~nan], last[~nan]) == 0, (name, mode, b)
            assert int(tie[b]) == int(any(ties)), (name, mode, b, ties)
        assert np.array_equal(mem2, idx), (name, mode, "resumed ranges")
        assert np.array_equal(tie2, tie), (name, mode, "tie flags of the resumed ranges")


def test_dispatch_takes_the_specialised_shape_only():
    assert hip.scan_mnist_shape(M, I, H, T)
    assert not hip.scan_mnist_shape(256, 256, 8, 1)


@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("N", CONT_N)
def test_continuous_logits_match_oracle(B, N):
    """One candidate in the only chunk (65), a chunk ending on the boundary (128, 64 + 5 * 64), ragged ends of 1 and 63 rows,
    one image and several: indices equal, scores bit for bit, and - asserted from the oracle - no iteration ties."""
    name = "cont-%d-%d" % (B, N)
    for _, aten in MODES:
        assert not any(any(ties) for _, _, ties, _ in oracle_scan(name, aten)), "continuous case with a tie: pick another seed"
    _check_against_oracle(name, scores=True)


@pytest.mark.parametrize("same", (True, False))
@pytest.mark.parametrize("levels", (2, 3, 5, 17))
def test_quantised_logits_match_oracle(levels, same):
    """Exact ties in most iterations: the ranking must hand over to the replay of torch.topk's order.  The oracle's own tie
    output shows that at least one iteration of every image's case ties; the kernel's flag is "some iteration tied"."""
    name = "quant-%d-%s" % (levels, "same" if same else "free")
    for _, aten in MODES:
        assert any(any(ties) for _, _, ties, _ in oracle_scan(name, aten)), "quantised case without a tie: pick another seed"
    # (the scores of tied candidates belong to whichever of them was kept: compared bit for bit in both orders as well)
    _check_against_oracle(name, scores=True)


def test_many_survivors_match_oracle():
    """Scores growing along the scan: most of every chunk enters the memory.  There is no survivor cap in this kernel (all
    128 candidates are ranked every time); the oracle shows an iteration after the first that admits more than 32."""
    for _, aten in MODES:
        assert any(max(adm[1:]) > 32 for _, _, _, adm in oracle_scan("survivors", aten))
    _check_against_oracle("survivors", scores=True)


def test_duplicated_rows_and_special_values_match_oracle():
    """A duplicated stretch of rows across a chunk boundary (exact ties between memory and chunk); NaN in one row, +inf in one
    row, -inf over ten rows."""
    _check_against_oracle("duplicates", scores=True)
    _check_against_oracle("special", scores=True)


def test_resumed_ranges_at_every_boundary_and_conditional_launch():
    N = M + 6 * I + 17
    n_iter = 7
    q = (np.random.default_rng(8500).integers(0, 3, (2, N, 1)).astype(np.float32) - 1.0) * np.float32(0.75)
    lg = dev(np.concatenate([_continuous(2, N), np.repeat(q, R, axis=2)]))               # two tie-free images, two that tie
    B = lg.shape[0]
    for mode, _ in MODES:
        hip.set_tie_order(mode)
        try:
            def ranges(cuts):
                mem = torch.full((B, M), -7, dtype=torch.int64, device=DEV)
                tie = torch.zeros((B,), dtype=torch.int32, device=DEV)
                for lo, hi in zip(cuts[:-1], cuts[1:]):
                    hip.scan_range(lg, M, I, H, T, lo, hi, mem, tie)
                return mem, tie
            prefix = [ranges([0, k]) for k in range(1, n_iter + 1)]                       # one launch over [0, k)
            whole, whole_tie = prefix[-1]
            assert torch.equal(whole, hip.scan(lg, M, I, H, T)) and torch.equal(whole_tie, hip.scan.last_tie)
            mem = torch.full((B, M), -7, dtype=torch.int64, device=DEV)
            tie = torch.zeros((B,), dtype=torch.int32, device=DEV)
            for k in range(n_iter):                                                       # seven launches of one iteration
                hip.scan_range(lg, M, I, H, T, k, k + 1, mem, tie)
                assert torch.equal(mem, prefix[k][0]) and torch.equal(tie, prefix[k][1]), (mode, k)
            for cut in range(1, n_iter):                                                  # every two-way cut
                m2, t2 = ranges([0, cut, n_iter])
                assert torch.equal(m2, whole) and torch.equal(t2, whole_tie), (mode, cut)
            # conditional launch: a zero condition word leaves everything untouched, a set bit is the plain launch
            L = hip.lib()
            cond = torch.tensor([0, 4], dtype=torch.int32, device=DEV)
            mem = torch.full((B, M), -7, dtype=torch.int64, device=DEV)
            sc = torch.full((B, M), -3.0, dtype=torch.float32, device=DEV)
            tie = torch.zeros((B,), dtype=torch.int32, device=DEV)
            for word, ran in ((cond[0:1], False), (cond[1:2], True)):
                rc = L.ipsx_scan_range_if(hip._p(lg), B, N, M, I, H, T, 0, n_iter, hip._p(mem), hip._p(sc), hip._p(tie), hip._p(word), 4,
                                          hip._stream())
                assert rc == 0
                if not ran:
                    assert bool((mem == -7).all()) and bool((sc == -3.0).all()) and int(tie.sum()) == 0, mode
            _, want_sc = hip.scan(lg, M, I, H, T, want_scores=True)
            assert torch.equal(mem, whole) and torch.equal(tie, whole_tie) and torch.equal(sc.view(torch.int32), want_sc.view(torch.int32))
        finally:
            hip.set_tie_order("torch")


@pytest.mark.parametrize("name", sorted(CASES))
def test_bit_identical_to_scan_fast_kernel(name):
    """Every input above through scan_fast_kernel (the switch off): indices, score bits and tie flags equal, as one launch
    and as resumed ranges.  (gpu_scan restores the switch in a finally.)"""
    for mode, _ in MODES:
        a, b = gpu_scan(name, mode, "mnist"), gpu_scan(name, mode, "fast")
        assert np.array_equal(a[0], b[0]), (name, mode, "indices")
        assert np.array_equal(a[1].view(np.int32), b[1].view(np.int32)), (name, mode, "score bits")
        assert np.array_equal(a[2], b[2]) and np.array_equal(a[4], b[4]), (name, mode, "tie flags")
        assert np.array_equal(a[3], b[3]), (name, mode, "resumed ranges")


@pytest.mark.parametrize("name", ("cont-3-1500", "quant-3-same"))
def test_persistent_instantiation_matches_plain_launch(name):
    """ipsx_scan_persistent with every row published BEFORE the launch (the bounded wait is never exercised) against the plain
    launch."""
    lg = dev(logits(name))
    B, N = lg.shape[:2]
    assert hip.scan_persistent_supported(M, I, H, T)
    for mode, _ in MODES:
        plain, _, plain_tie, _, _ = gpu_scan(name, mode, "mnist")
        hip.set_tie_order(mode)
        try:
            words = torch.tensor([N, 0], dtype=torch.int32, device=DEV)                   # [rows published, status]
            mem = torch.full((B, M), -7, dtype=torch.int64, device=DEV)
            tie = torch.zeros((B,), dtype=torch.int32, device=DEV)
            hip.scan_persistent(lg, M, I, H, T, mem, tie, words[0:1], words[1:2])
            torch.cuda.synchronize()
        finally:
            hip.set_tie_order("torch")
        assert int(words[1].item()) & 1 == 0 and int(words[1].item()) & 2 == 2, mode       # never gave up; was resident
        assert np.array_equal(mem.cpu().numpy(), plain) and np.array_equal(tie.cpu().numpy(), plain_tie), (name, mode)
