"""What the lattice tests of ``ipsx_scan_ragged`` share (tests/test_ragged_lattice_cpu.py on the host,
tests/test_ragged_scan_lattice.py on the device): one shape per instantiation class of the ragged selection loop with
I != M, six slide lengths per shape, five kinds of packed logits tables, and the oracle's loop for one slide.

No GPU code is imported here: the module serves the CPU test as well."""

import numpy as np

from oracle import oracle as orc

# name -> (M, I, heads, tokens, class).  The class of scan_fast_kernel is (EPT, LCH); of scan_large_kernel its staging
# path; "cam" is scan_cam_kernel.  "-lt": I < M, "-gt": I > M; I divides neither M nor is divided by it (cam's shape is fixed).
CASES = {
    "f8-e1-lt": (24, 10, 8, 1, (1, 2)), "f8-e1-gt": (16, 24, 8, 1, (1, 2)),
    "f8-e2-lt": (100, 60, 8, 1, (2, 8)), "f8-e2-gt": (48, 100, 8, 1, (2, 8)),
    "f8-e4-lt": (200, 150, 8, 1, (4, 8)), "f8-e4-gt": (80, 200, 8, 1, (4, 8)),
    "f8-e8-lt": (400, 130, 8, 1, (8, 16)), "f8-e8-gt": (200, 340, 8, 1, (8, 16)),
    "f32-e1-lt": (20, 12, 8, 4, (1, 2)), "f32-e1-gt": (12, 20, 8, 4, (1, 2)),
    "f32-e2-lt": (40, 24, 8, 4, (2, 2)), "f32-e2-gt": (24, 40, 8, 4, (2, 2)),
    "f32-e4-lt": (80, 48, 8, 4, (4, 2)), "f32-e4-gt": (40, 88, 8, 4, (4, 2)),
    "f32-e8-lt": (100, 60, 8, 4, (8, 8)), "f32-e8-gt": (60, 100, 8, 4, (8, 8)),
    "l-direct": (16, 400, 8, 1, "direct"), "l-direct-lt": (700, 400, 8, 1, "direct"),
    "l-r4": (24, 40, 4, 1, "float4"),           # R = 4, 12: the last group of the float4 staging is half filled
    "l-r12": (40, 24, 3, 4, "float4"),
    "l-r32": (150, 120, 8, 4, "float4"),        # R = 32 beyond the LDS plan
    # R = 20: a multiple of 4, so the float4 staging (two whole groups and a half-filled one), and no fewer rows than the
    # 16 wavefronts that take the row maxima
    "l-r20": (30, 50, 5, 4, "float4"),
    "l-r3": (16, 24, 3, 1, "scalar"), "l-r9": (20, 12, 3, 3, "scalar"), "l-r1": (16, 40, 1, 1, "scalar"),
    "l-r18": (30, 50, 6, 3, "scalar"),          # R = 18: the scalar staging with no fewer rows than the 16 wavefronts
    "cam": (256, 256, 8, 1, "cam"),
}
KINDS = ("cont", "quant", "dup", "ramp", "special")
MODES = (("torch", True), ("canonical", False))          # (hip.set_tie_order's name, the oracle's aten_ties)
CLEAN = (1, 3, 4)                                        # the slides the `special` table leaves as `cont` has them


def fast_class(M, I, R):
    """The (EPT, LCH) class rule of scan_fast_plan (csrc/scan_fast.hip): elements per thread of the 1,024 that stage the
    candidates' logits, and the chunk of the ranking.  Says which class a shape CLAIMS; whether the shape is LDS-resident
    at all is the library's answer (``ipsx_scan_workspace_bytes``), asked on the device."""
    ept = 1
    while ept * 1024 < (M + I) * R:
        ept *= 2
    return ept, (2 if M + I <= 128 else 8 if M + I <= 512 else 16)


def lengths(M, I):
    """A ragged last chunk; one candidate in the only chunk; a chunk that ends on the boundary; a second chunk of one row;
    exactly one full chunk; a last chunk one row short.  The shortest slide is not first."""
    return (M + 2 * I + I // 2 + 1, M + 1, M + 3 * I, M + I + 1, M + I, M + 4 * I - 1)


def starts(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def seed_of(M, I, R):
    return 4100 + 31 * M + I + R


def table(kind, lens, M, I, R, seed):
    """The packed (sum lens, R) float32 logits of ``kind``; every kind but ``quant`` starts from the same ``cont`` draw."""
    g = np.random.default_rng(seed)
    total = int(sum(lens))
    if kind == "quant":       # whole candidates tie and their rows are bit-identical
        q = (g.integers(0, 5, (total, 1)).astype(np.float32) - 1.0) * np.float32(0.75)
        return np.ascontiguousarray(np.repeat(q, R, axis=1))
    lg = (g.standard_normal((total, R)) * 3.0).astype(np.float32)
    st = starts(lens)
    if kind == "dup":         # every slide's last rows are its first rows again
        for lo, n in zip(st, lens):
            k = min(I, n - M)
            lg[lo + n - k:lo + n] = lg[lo:lo + k]
    elif kind == "ramp":      # scores grow along the scan: most of every chunk enters the memory
        for lo, n in zip(st, lens):
            lg[lo:lo + n] += (np.arange(n, dtype=np.float32) * np.float32(0.05))[:, None]
    elif kind == "special":
        lg[st[0] + M + 3, 1 % R] = np.nan
        lg[st[2] + 5, 0] = np.inf
        lg[st[5] + M - 2:st[5] + M + 4, R - 1] = -np.inf
    else:
        assert kind == "cont", kind
    return np.ascontiguousarray(lg)


def oracle_loop(lg, M, I, H, T, aten):
    """The oracle's loop over ONE slide's (N, H*T) logits (the loop of tests/test_scan_mnist.py::oracle_scan): the final
    indices, the final scores, the tie flag of every iteration, and how many chunk candidates every iteration admitted."""
    L = orc.lib()
    N = lg.shape[0]
    cur = np.arange(M, dtype=np.int64)
    ties, admitted, last = [], [], None
    for lo in range(M, N, I):
        cand = np.concatenate([cur, np.arange(lo, min(lo + I, N), dtype=np.int64)])
        s = np.empty(len(cand), dtype=np.float32)
        L.orc_scores_from_logits(orc._f(lg[cand])[1], len(cand), H, T, s.ctypes.data_as(orc.f32p), None)
        top, tie = orc.topm(s, M, aten_ties=aten, rows=lg[cand])
        ties.append(tie)
        admitted.append(int((top >= M).sum()))
        cur, last = cand[top], s[top]
    return cur, last, ties, admitted


_TABLES, _ORACLE = {}, {}


def case_table(name, kind):
    """(lengths, the read-only packed table) of a case; made once."""
    if (name, kind) not in _TABLES:
        M, I, H, T, _ = CASES[name]
        lens = lengths(M, I)
        lg = table(kind, lens, M, I, H * T, seed_of(M, I, H * T))
        lg.setflags(write=False)
        _TABLES[(name, kind)] = (lens, lg)
    return _TABLES[(name, kind)]


def case_oracle(name, kind, aten, chunk=None):
    """``oracle_loop`` of every slide of a case (``chunk``: another chunk size than the case's I); computed once."""
    key = (name, kind, aten, chunk)
    if key not in _ORACLE:
        M, I, H, T, _ = CASES[name]
        lens, lg = case_table(name, kind)
        st = starts(lens)
        _ORACLE[key] = [oracle_loop(lg[st[b]:st[b] + n], M, I if chunk is None else chunk, H, T, aten)
                        for b, n in enumerate(lens)]
    return _ORACLE[key]
