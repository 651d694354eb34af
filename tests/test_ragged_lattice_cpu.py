"""The inputs of tests/test_ragged_scan_lattice.py can tell right from wrong - shown from the oracle alone, on the host:
the continuous tables never tie, the quantised ones do, the ramp fills the memory from the chunk, a loop that mistook M
for I selects something else, and every ``f*`` shape claims the class its name states (tests/ragged_lattice_cases.py)."""

import numpy as np
import pytest

import ragged_lattice_cases as lc

NAMES = list(lc.CASES)


def test_the_table_is_the_lattice():
    """Eight scan_fast_kernel classes from both sides of I = M, three staging paths of scan_large_kernel, scan_cam_kernel."""
    fast = {(n.split("-")[0], lc.CASES[n][4]) for n in NAMES if n.startswith("f")}
    assert fast == {("f8", c) for c in ((1, 2), (2, 8), (4, 8), (8, 16))} | {("f32", c) for c in ((1, 2), (2, 2), (4, 2), (8, 8))}
    assert {lc.CASES[n][4] for n in NAMES if n.startswith("l-")} == {"direct", "float4", "scalar"}
    assert len(NAMES) == 27
    for name, (M, I, H, T, _) in lc.CASES.items():
        if name != "cam":
            assert I != M and (not name.startswith("f") or (M % I and I % M)), name
        assert (name.endswith("-lt") and I < M) or (name.endswith("-gt") and I > M) or name[-2:] not in ("lt", "gt"), name
        lens = lc.lengths(M, I)
        assert min(lens) == M + 1 and lens[0] != min(lens) and len(set(lens)) == 6
        assert [(n - M) % I for n in lens] == [(I // 2 + 1) % I, 1 % I, 0, 1 % I, 0, I - 1]


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("f")])
def test_fast_cases_claim_the_class_of_their_name(name):
    M, I, H, T, cls = lc.CASES[name]
    R = H * T
    assert name.startswith("f%d-e%d-" % (R, cls[0]))
    assert lc.fast_class(M, I, R) == cls
    assert (H, T) in ((8, 1), (8, 4)) and M + I <= 1024              # the instantiated (R, T) pairs; one key per thread


def test_large_cases_claim_the_path_of_their_name():
    for name, (M, I, H, T, cls) in lc.CASES.items():
        R = H * T
        if cls == "direct":
            assert (H, T) == (8, 1), name                            # (that the LDS plan refuses the shape: asked on the device)
        elif cls == "float4":
            assert R % 4 == 0 and (R, T) != (8, 1), name
            assert name != "l-r32" or (R == 32 and lc.fast_class(M, I, R)[0] > 8), name
        elif cls == "scalar":
            assert R % 4 != 0, name
        if name.startswith("l-r"):
            assert R == int(name[3:]), name
    rows = lambda path: sorted(H * T for M, I, H, T, cls in lc.CASES.values() if cls == path)
    assert rows("float4") == [4, 12, 20, 32]                  # R % 8 == 4: the last group of eight is half filled; R % 8 == 0
    assert rows("scalar") == [1, 3, 9, 18]                    # fewer rows than the 16 wavefronts, and more


@pytest.mark.parametrize("name", NAMES)
def test_continuous_and_ramp_tables_never_tie(name):
    for kind in ("cont", "ramp"):
        for _, aten in lc.MODES:
            for b, (_, _, ties, _) in enumerate(lc.case_oracle(name, kind, aten)):
                assert not any(ties), (name, kind, aten, b)


@pytest.mark.parametrize("name", NAMES)
def test_quantised_tables_tie_in_most_slides(name):
    for _, aten in lc.MODES:
        tied = sum(1 for _, _, ties, _ in lc.case_oracle(name, "quant", aten) if any(ties))
        assert tied >= 4, (name, aten, tied)


@pytest.mark.parametrize("name", [n for n in NAMES if n.endswith("-lt") or n == "cam"])
def test_the_ramp_admits_most_of_a_chunk(name):
    """Some iteration after the first takes at least 80 % of its chunk into the memory: scan_cam_kernel then exceeds its
    survivor limit."""
    M, I = lc.CASES[name][:2]
    for _, aten in lc.MODES:
        best = 0.0
        for (_, _, _, adm), n in zip(lc.case_oracle(name, "ramp", aten), lc.lengths(M, I)):
            for k, a in enumerate(adm):
                if k > 0:
                    best = max(best, a / min(I, n - M - k * I))
        assert best >= 0.8, (name, aten, best)


@pytest.mark.parametrize("name", [n for n in NAMES if lc.CASES[n][0] != lc.CASES[n][1]])
def test_a_loop_that_took_m_for_i_selects_something_else(name):
    """The oracle with the chunk size replaced by M: at least 3 of the 6 slides differ on ``cont`` or on ``quant``, in either
    tie order.  One exception that no seed can lift: with ONE logit per patch (``l-r1``) a candidate's score is monotone
    in that logit, so the top M of a slide do not depend on how it is cut into chunks - unless equal scores are broken in
    torch.topk's order, which does.  ``l-r1`` is sensitive on ``quant`` in the torch order only."""
    M = lc.CASES[name][0]
    for mode, aten in lc.MODES:
        differ = {}
        for kind in ("cont", "quant"):
            right, wrong = lc.case_oracle(name, kind, aten), lc.case_oracle(name, kind, aten, chunk=M)
            differ[kind] = sum(1 for r, w in zip(right, wrong) if not np.array_equal(r[0], w[0]))
        if name == "l-r1":
            assert differ["cont"] == 0 and (differ["quant"] >= 3 if aten else differ["quant"] == 0), (name, mode, differ)
        else:
            assert max(differ.values()) >= 3, (name, mode, differ)


def test_special_is_cont_plus_its_entries():
    """What the isolation test on the device rests on: slides 1, 3 and 4 of ``special`` are those of ``cont``, bit for bit."""
    for name in ("f8-e2-gt", "f32-e8-lt", "l-r12", "cam"):
        M, I, H, T, _ = lc.CASES[name]
        R = H * T
        (lens, cont), (_, spec) = lc.case_table(name, "cont"), lc.case_table(name, "special")
        st = lc.starts(lens)
        diff = np.argwhere(cont.view(np.int32) != spec.view(np.int32))
        want = [(st[0] + M + 3, 1 % R), (st[2] + 5, 0)] + [(st[5] + r, R - 1) for r in range(M - 2, M + 4)]
        assert sorted(map(tuple, diff.tolist())) == sorted((int(a), int(b)) for a, b in want)
        assert np.isnan(spec[st[0] + M + 3, 1 % R]) and np.isposinf(spec[st[2] + 5, 0])
        for b in lc.CLEAN:
            assert np.isfinite(spec[st[b]:st[b + 1]]).all()
