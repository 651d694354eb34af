"""The hand-over between two launches of ``scan_mnist_kernel`` on different streams (``hip.LogitsParts.scan_range`` with
``gate_publish=`` / ``gate=`` / ``out=``, ``ipsx_scan_range_logits_gate``, csrc/scan_mnist.hip): the side stream's last loop
launch publishes, per image, the iteration it reached; the call's last launch writes the rows of the trailing parts first,
waits on the device for its image's word, runs the remaining iterations and leaves the indices in a buffer of its own.
Against the launches it replaces - ``hip.logits`` over the parts and ONE ``hip.scan_range`` over the whole loop - bit for
bit: every logits row, the final ``mem_idx``, the tie flags.  (``mem_score`` is not handed through by the wrapper.)

B = 3, D = 16, H = 8, 4 tokens, M = I = 64; N = 64 + 64 k + r for k in {1, 4}, r in {0, 1, 17}: a ragged last chunk.
N = 128 is ONE iteration - nothing to hand over between two launches: its launch only publishes and writes to ``out``."""

import pytest
import torch

from ips_amd import hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M = I = 64
H, T, D, DK = 8, 4, 16, 2
R = H * T
B = 3
SIZES = [64 + 64 * k + r for k in (1, 4) for r in (0, 1, 17)]
# rows per image of the trailing parts that go into the last launch: 1 or 2 parts of 1, 64, 65 and 200 rows
TAILS = [(1,), (64,), (65,), (200,), (64, 1), (1, 65), (65, 64)]
_CACHE = {}


def folded_query():
    if "vq" not in _CACHE:
        g = torch.Generator().manual_seed(11)
        qs = (torch.randn((T, H * DK), generator=g) * 0.5).to(DEV)
        wk = (torch.randn((H * DK, D), generator=g) * 0.3).to(DEV)
        _CACHE["vq"] = hip.fold_query(qs, wk, H, DK, T)
    return _CACHE["vq"]


def n_iter(N):
    return -(-(N - M) // I)


def reference(N):
    """(embeddings, positional rows, logits table, mem_idx, tie flags) of the plain launches - once per N, never written again."""
    if N not in _CACHE:
        g = torch.Generator().manual_seed(1000 + N)
        emb = torch.randn((B, N, D), generator=g).to(DEV)
        pos = (torch.randn((B, N, D), generator=g) * 0.5).to(DEV)
        logits = torch.empty((B, N, R), device=DEV)
        hip.logits(emb, pos, folded_query(), R, out=logits)
        mem = torch.full((B, M), -7, dtype=torch.int64, device=DEV)
        tie = torch.zeros((B,), dtype=torch.int32, device=DEV)
        hip.scan_range(logits, M, I, H, T, 0, n_iter(N), mem, tie)
        torch.cuda.synchronize()
        _CACHE[N] = (emb, pos, logits, mem, tie)
    return _CACHE[N]


def cut(N, tail):
    """-> (rows of every part, k_tail, iterations its[0 .. P]) or None: the side stream keeps at least M + I rows - one iteration -
    in one part, or in two where the second adds an iteration; the tail's parts follow; its[k] = the iterations whose rows end
    inside the parts in front of part k."""
    side = N - sum(tail)
    if side < M + I or (side - M) // I >= n_iter(N):
        return None
    rows = [M + I, side - M - I] if side - M - I >= I else [side]
    k_tail = len(rows)
    rows += list(tail)
    its, at = [0], 0
    for r in rows[:k_tail]:
        at += r
        its.append((at - M) // I)
    its += [n_iter(N)] * len(tail)
    return rows, k_tail, its


CHAINS = [(N, tail) for N in SIZES for tail in TAILS if cut(N, tail) is not None]


def state(N):
    return (torch.full((B, N, R), float("nan"), device=DEV), torch.full((B, M), -7, dtype=torch.int64, device=DEV),
            torch.zeros((B,), dtype=torch.int32, device=DEV), torch.zeros((B + 1,), dtype=torch.int32, device=DEV),
            torch.full((B, M), -9, dtype=torch.int64, device=DEV))


def parts_of(emb, rows):
    at, out = 0, []
    for r in rows:
        out.append(emb[:, at:at + r].contiguous())
        at += r
    return hip.LogitsParts(out)


def side_launches(table, k_tail, its, logits, mem, tie, pos, publish):
    for k in range(k_tail):
        table.scan_range(logits, M, I, H, T, its[k], its[k + 1], mem, tie, k, k + 1, pos, folded_query(),
                         gate_publish=publish if k == k_tail - 1 else None)


def same(N, logits, out, tie, what):
    _, _, want_lg, want_mem, want_tie = reference(N)
    assert torch.equal(logits.view(torch.int32), want_lg.view(torch.int32)), what + ": the logits table"
    assert torch.equal(out, want_mem), what + ": mem_idx"
    assert torch.equal(tie, want_tie), what + ": tie flags"


def test_one_iteration_publishes_and_writes_to_its_own_buffer():
    N = 128
    emb, pos = reference(N)[:2]
    logits, mem, tie, words, out = state(N)
    parts_of(emb, [N]).scan_range(logits, M, I, H, T, 0, 1, mem, tie, 0, 1, pos, folded_query(), gate_publish=words[:B], out=out)
    torch.cuda.synchronize()
    same(N, logits, out, tie, "N = 128")
    assert words[:B].tolist() == [1] * B and int(words[B]) == 0
    assert bool((mem == -7).all()), "the working buffer is only read"


@pytest.mark.parametrize("N, tail", CHAINS, ids=["%d-%s" % (n, "+".join(map(str, t))) for n, t in CHAINS])
def test_gate_words_at_their_target_when_the_launch_starts(N, tail):
    """(i) everything on one stream: the side's launches have ended - and published - when the last launch starts."""
    rows, k_tail, its = cut(N, tail)
    emb, pos = reference(N)[:2]
    table = parts_of(emb, rows)
    logits, mem, tie, words, out = state(N)
    gate, status = words[:B], words[B:]
    side_launches(table, k_tail, its, logits, mem, tie, pos, gate)
    table.scan_range(logits, M, I, H, T, its[k_tail], its[-1], mem, tie, k_tail, len(rows), pos, folded_query(), redo=status,
                     gate=gate, status=status, out=out)
    torch.cuda.synchronize()
    same(N, logits, out, tie, "one stream")
    assert gate.tolist() == [its[k_tail]] * B and int(status) == 0


@pytest.mark.parametrize("N, tail", CHAINS, ids=["%d-%s" % (n, "+".join(map(str, t))) for n, t in CHAINS])
def test_the_chain_on_two_streams_without_a_stream_wait(N, tail):
    """(ii) the side's launches on a stream of their own, the last launch on the current one, enqueued behind them by the host
    and ordered by the gate alone."""
    rows, k_tail, its = cut(N, tail)
    emb, pos = reference(N)[:2]
    table = parts_of(emb, rows)
    logits, mem, tie, words, out = state(N)
    gate, status = words[:B], words[B:]
    side = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        side_launches(table, k_tail, its, logits, mem, tie, pos, gate)
    table.scan_range(logits, M, I, H, T, its[k_tail], its[-1], mem, tie, k_tail, len(rows), pos, folded_query(), redo=status,
                     gate=gate, status=status, out=out)
    torch.cuda.synchronize()
    same(N, logits, out, tie, "two streams")
    assert gate.tolist() == [its[k_tail]] * B and int(status) == 0


@pytest.mark.parametrize("N, tail", [(337, (65, 64)), (145, (17,))])
def test_a_word_never_published_is_given_up_on_and_the_image_redone(N, tail):
    """(iii) image 1's word stays 0 under a bound of 1 ms, and what the side left for that image is spoilt - its rows, its working
    indices - so that only the redo (every row again, the loop from iteration 0) gives the clean call's result."""
    rows, k_tail, its = cut(N, tail)
    emb, pos = reference(N)[:2]
    table = parts_of(emb, rows)
    logits, mem, tie, words, out = state(N)
    gate, status = words[:B], words[B:]
    side_launches(table, k_tail, its, logits, mem, tie, pos, None)
    gate.fill_(its[k_tail])
    gate[1] = 0
    logits[1, :N - sum(tail)] = 3.0
    mem[1] = torch.arange(M, device=DEV).flip(0)
    before = mem.clone()
    was = hip.persistent_wait_ms(1)
    try:
        table.scan_range(logits, M, I, H, T, its[k_tail], its[-1], mem, tie, k_tail, len(rows), pos, folded_query(), redo=status,
                         gate=gate, status=status, out=out)
        torch.cuda.synchronize()
    finally:
        hip.persistent_wait_ms(was)
    assert hip.persistent_wait_ms(0) == was
    assert int(status) & 1, "the wait that gave up sets the status bit"
    kept = out.clone()
    same(N, logits, out, tie, "gave up on image 1")
    assert torch.equal(mem, before), "the last launch leaves the working buffer alone"
    mem.fill_(-1)                                                       # a late side-stream launch writing the working buffer
    torch.cuda.synchronize()
    assert torch.equal(out, kept)


@pytest.mark.parametrize("N, tail", [(337, (65, 64)), (321, (1,))])
def test_the_status_word_set_in_front_redoes_the_call_behind_the_gate(N, tail):
    """(iv) a part wait gave up: the side's launches read OTHER embeddings, the word is set when the last launch starts - it waits
    for its gate all the same, then computes every row and runs the whole loop."""
    rows, k_tail, its = cut(N, tail)
    emb, pos = reference(N)[:2]
    g = torch.Generator().manual_seed(5)
    early = parts_of(torch.randn((B, N, D), generator=g).to(DEV), rows)
    table = parts_of(emb, rows)
    logits, mem, tie, words, out = state(N)
    gate, status = words[:B], words[B:]
    status.fill_(1)
    side = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        side_launches(early, k_tail, its, logits, mem, tie, pos, gate)
    table.scan_range(logits, M, I, H, T, its[k_tail], its[-1], mem, tie, k_tail, len(rows), pos, folded_query(), redo=status,
                     gate=gate, status=status, out=out)
    torch.cuda.synchronize()
    same(N, logits, out, tie, "redo in front")
    assert gate.tolist() == [its[k_tail]] * B


@pytest.mark.parametrize("N, tail", [(337, (65, 64)), (321, (1,)), (145, (17,))])
def test_a_long_side_part_publishes_from_a_launch_with_no_rows_of_its_own(N, tail):
    """The side's parts as ``Selection.parts_loop_logits`` enqueues a long one: ``hip.logits`` over the part, then the loop's
    launch with part_begin == part_end - the plain instance with the gate's parameter - publishing at its end; two streams."""
    rows, k_tail, its = cut(N, tail)
    emb, pos = reference(N)[:2]
    table = parts_of(emb, rows)
    logits, mem, tie, words, out = state(N)
    gate, status = words[:B], words[B:]
    side = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for k in range(k_tail):
            lo = table.first[k]
            hip.logits(table.embs[k], pos[:, lo:lo + rows[k]], folded_query(), R, out=logits[:, lo:lo + rows[k]])
            table.scan_range(logits, M, I, H, T, its[k], its[k + 1], mem, tie, k + 1, k + 1, pos, folded_query(),
                             gate_publish=gate if k == k_tail - 1 else None)
    table.scan_range(logits, M, I, H, T, its[k_tail], its[-1], mem, tie, k_tail, len(rows), pos, folded_query(), redo=status,
                     gate=gate, status=status, out=out)
    torch.cuda.synchronize()
    same(N, logits, out, tie, "long side parts")
    assert gate.tolist() == [its[k_tail]] * B and int(status) == 0


# ---------------------------------------------------------------------------------------------------- mem_score, through the export
def raw(table, logits, it0, it1, mem, score, tie, p0, p1, pos, redo=None, gate=None, publish=None, status=None, out=None):
    """``ipsx_scan_range_logits_gate`` itself, with a ``mem_score`` buffer (``LogitsParts.scan_range`` passes none)."""
    p = hip._p
    N = logits.shape[1]
    rc = hip.lib().ipsx_scan_range_logits_gate(p(logits), B, N, M, I, H, T, it0, it1, p(mem), p(score), p(tie), table.array, len(table), p0, p1, D,
                                               p(pos), pos.stride(0), p(folded_query()), p(redo), 1 if redo is not None else 0, p(gate),
                                               it0 if gate is not None else 0, p(publish), p(status), 1 if status is not None else 0, p(out),
                                               hip._stream())
    assert rc == 0, hip.lib().ipsx_last_error().decode()


@pytest.mark.parametrize("give_up", [False, True], ids=["clean", "image 1 gives up"])
@pytest.mark.parametrize("N, tail", [(337, (65, 64)), (145, (17,))])
def test_mem_score_of_the_gated_launch_is_the_whole_loops(N, tail, give_up):
    """The scores of the selected patches as ONE ``hip.scan`` over the table leaves them, on the clean path and for an image whose
    wait gave up (its rows and working indices spoilt, as in (iii)); the scores go where ``mem_score`` says, not to ``out``."""
    rows, k_tail, its = cut(N, tail)
    emb, pos, want_lg = reference(N)[:3]
    want_mem, want_score = hip.scan(want_lg, M, I, H, T, want_scores=True)
    table = parts_of(emb, rows)
    logits, mem, tie, words, out = state(N)
    gate, status = words[:B], words[B:]
    score = torch.full((B, M), float("nan"), device=DEV)
    for k in range(k_tail):
        raw(table, logits, its[k], its[k + 1], mem, score, tie, k, k + 1, pos, publish=gate if k == k_tail - 1 else None)
    if give_up:
        torch.cuda.synchronize()
        gate[1] = 0
        logits[1, :N - sum(tail)] = 3.0
        mem[1] = torch.arange(M, device=DEV).flip(0)
        score[1] = -1.0
    was = hip.persistent_wait_ms(1) if give_up else None
    try:
        raw(table, logits, its[k_tail], its[-1], mem, score, tie, k_tail, len(rows), pos, redo=status, gate=gate, status=status, out=out)
        torch.cuda.synchronize()
    finally:
        if was is not None:
            hip.persistent_wait_ms(was)
    assert (int(status) & 1) == int(give_up)
    assert torch.equal(out, want_mem)
    assert torch.equal(score.view(torch.int32), want_score.view(torch.int32))
