"""``ipsx_stream_commit_ragged`` (the state update of ``IPSNet.ips_ragged_stream``) against a restatement in
torch on the host: four tables in one launch with rows of 48, 20, 7 and 32 bytes (lanes of 16, 4, 1 and 16 bytes; the last
table has no piece and holds all candidates), one slide in each of the four modes, a ``sel`` with entries below 0 and
beyond the candidates, sentinels behind what a slide writes, and slides whose device numbers contradict the capacities."""

import pytest
import torch

from ips_amd import hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M, CAP = 4, 12
SENTINEL = 113
IDLE, APPEND, SELECT, MOVE = hip.COMMIT_IDLE, hip.COMMIT_APPEND, hip.COMMIT_SELECT, hip.COMMIT_MOVE
#          held cand tail first mode
SLIDES = [[2, 5, 0, 0, IDLE, 0],
          [3, 6, 0, 0, APPEND, 0],
          [5, 10, 8, 3, SELECT, 0],
          [2, 4, 0, 8, MOVE, 0],
          [11, 13, 0, 0, MOVE, 0],         # 13 rows into tables of 12: not touched
          [1, 3, 0, 10, APPEND, 0]]        # rows 10, 11 of a piece of 11 rows: not touched
UNTOUCHED = (0, 4, 5)
PIECE_ROWS = 11
SEL = [[0, 0, 0, 0], [0, 0, 0, 0], [-3, 9, 17, 2], [0, 0, 0, 0], [0, 1, 2, 3], [0, 0, 0, 0]]       # slide 2: clamped to 0, 9, 9, 2
WIDTHS = ((torch.float32, 12, True), (torch.uint8, 20, True), (torch.uint8, 7, True), (torch.float32, 8, False))   # 48, 20, 7, 32 bytes


def make_tables(seed, in_place=False):
    """-> [(held, piece | None, dst)] on the host: random held rows and pieces, destinations full of the sentinel (in place:
    the held buffer itself)."""
    g = torch.Generator().manual_seed(seed)
    B = len(SLIDES)
    out = []
    for dtype, width, has_piece in WIDTHS:
        held = torch.randint(0, 100, (B, CAP, width), generator=g).to(dtype)
        piece = torch.randint(0, 100, (PIECE_ROWS, width), generator=g).to(dtype) if has_piece else None
        dst = held if in_place else torch.full((B, CAP, width), SENTINEL, dtype=dtype)
        out.append((held, piece, dst))
    return out


def restate(tables, slides, sel, untouched):
    """What the launch leaves in every destination, slide by slide."""
    want = []
    for held, piece, dst in tables:
        d = dst.clone()
        for b, (n_held, n_cand, tail, first, mode, _) in enumerate(slides):
            if b in untouched or mode == IDLE:
                continue
            if piece is not None:
                cand = torch.cat((held[b, :n_held], piece[first:first + n_cand - n_held]))
            else:
                cand = held[b, :n_cand]
            assert cand.shape[0] == n_cand
            if mode == APPEND:
                if piece is not None:
                    d[b, n_held:n_cand] = cand[n_held:]
            elif mode == SELECT:
                rows = torch.tensor(sel[b]).clamp(0, n_cand - 1)
                d[b, :M] = cand[rows]
                d[b, M:M + n_cand - tail] = cand[tail:]
            else:
                d[b, :n_cand] = cand
        want.append(d)
    return want


def launch(tables, slides, sel, rows_max, in_place=False):
    dev = []
    for held, piece, dst in tables:
        h = held.to(DEV)
        dev.append((h, piece.to(DEV) if piece is not None else None, h if in_place else dst.to(DEV)))
    hip.stream_commit_ragged(dev, torch.tensor(sel, dtype=torch.int64, device=DEV) if sel is not None else None,
                             torch.tensor(slides, dtype=torch.int64, device=DEV), M, rows_max)
    torch.cuda.synchronize()
    return [(h.cpu(), d.cpu()) for h, _, d in dev]


@pytest.mark.parametrize("rows_max", [6, 9])
def test_four_tables_four_modes_in_one_launch(rows_max):
    """(6 rows: what the select slide writes; 9: workgroups beyond every slide's rows return at once)"""
    tables = make_tables(3)
    want = restate(tables, SLIDES, SEL, UNTOUCHED)
    got = launch(tables, SLIDES, SEL, rows_max)
    for k, ((held, _, _), (held_after, dst), w) in enumerate(zip(tables, got, want)):
        assert torch.equal(held_after, held), ("table", k, "the held rows were written")
        assert torch.equal(dst, w), ("table", k)
    # what the restatement implies, said once more: the clamped selection, the sentinel behind the written rows, the
    # untouched rows in front of an append, the untouched slides
    held, piece, _ = tables[0]
    dst = got[0][1]
    cand2 = torch.cat((held[2, :5], piece[3:8]))
    assert torch.equal(dst[2, :6], cand2[[0, 9, 9, 2, 8, 9]]) and (dst[2, 6:] == SENTINEL).all()
    assert (dst[1, :3] == SENTINEL).all() and torch.equal(dst[1, 3:6], piece[0:3]) and (dst[1, 6:] == SENTINEL).all()
    assert torch.equal(dst[3, :4], torch.cat((held[3, :2], piece[8:10]))) and (dst[3, 4:] == SENTINEL).all()
    for b in UNTOUCHED:
        assert all((d[b] == SENTINEL).all() for _, d in got), b
    # the table without a piece: nothing to append, all candidates from its held rows
    assert (got[3][1][1] == SENTINEL).all() and torch.equal(got[3][1][2, :4], tables[3][0][2, [0, 9, 9, 2]])


def test_append_in_place_leaves_the_held_rows():
    """dst is the held buffer: the append slides write rows [held, cand) alone; a slide that selects or moves in place
    contradicts the launch and is not touched."""
    tables = make_tables(4, in_place=True)
    slides = [[2, 5, 0, 0, IDLE, 0], [3, 6, 0, 0, APPEND, 0], [5, 10, 8, 3, SELECT, 0], [2, 4, 0, 8, MOVE, 0], [4, 7, 0, 6, APPEND, 0],
              [0, 2, 0, 9, APPEND, 0]]
    before = [held.clone() for held, _, _ in tables]
    want = restate([(h, p, h) for h, p, _ in tables], slides, SEL, untouched=(0, 2, 3))
    got = launch(tables, slides, SEL, 3, in_place=True)
    for k, ((_, dst), w) in enumerate(zip(got, want)):
        assert torch.equal(dst, w), ("table", k)
    assert torch.equal(got[0][1][1, :3], before[0][1, :3]) and torch.equal(got[0][1][1, 3:6], tables[0][1][0:3])
    assert torch.equal(got[0][1][5, :2], tables[0][1][9:11])
    assert torch.equal(got[3][1], before[3])                       # (the table without a piece appends nothing)


def test_select_without_sel_and_numbers_out_of_range_write_nothing():
    tables = make_tables(5)
    big = 1 << 62
    slides = [[5, 10, 8, 3, SELECT, 0],          # selects, the launch has no sel
              [-1, 4, 0, 0, MOVE, 0],            # negative held rows
              [3, 2, 0, 0, MOVE, 0],             # fewer candidates than held rows
              [2, 4, 0, -1, MOVE, 0],            # the piece starts in front of the tensor
              [2, big, 0, 0, MOVE, 0],           # sums that would overflow
              [2, 4, 0, 8, 7, 0]]                # an unknown mode
    got = launch(tables, slides, None, 8)
    for k, (_, dst) in enumerate(got):
        assert (dst == SENTINEL).all(), ("table", k)
    slides[0] = [5, 10, 11, 3, SELECT, 0]        # the tail starts behind the candidates
    got = launch(tables, slides, SEL, 8)
    assert all((dst == SENTINEL).all() for _, dst in got)


@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("dtype,width", [(torch.float32, 4), (torch.float32, 3), (torch.uint8, 3)])        # rows of 16, 12, 3 bytes
def test_uniform_and_ragged_commit_write_the_same_bytes(dtype, width, clamp):
    """Where the contracts of ``hip.stream_commit`` and ``hip.stream_commit_ragged`` overlap - every slide has the uniform
    call's numbers, the pieces are contiguous - the two kernel families share their body and must write byte-identical
    destinations: an append, then a selection with a tail.  B = 2, M = 4, 5 held rows, a piece of 3 rows (the uniform call
    takes it as (B, 3, ...), the ragged one the same rows packed as (6, ...)), tail_first = 6; ``clamp``: one ``sel`` entry
    of -1 and one of n_cand.  Sources and destinations are filled with distinct values, and the bytes neither call may
    touch - the rows in front of an append, the rows behind what is written - are compared with the rest."""
    B, held_rows, piece_rows, tail_first, cap = 2, 5, 3, 6, 12
    n_cand = held_rows + piece_rows
    numel = B * cap * width

    def values(first, shape):           # first, first + 1, ...: no value twice in held and piece together, none is the filler
        return torch.arange(first, first + torch.Size(shape).numel()).to(dtype).view(shape).to(DEV)

    held = values(1, (B, cap, width))
    piece = values(1 + numel, (B, piece_rows, width))
    assert numel + piece.numel() < 251       # (a uint8 holds them)
    sel = torch.tensor([[7, 0, 5, 2], [3, 3, 6, 1]], dtype=torch.int64, device=DEV)
    if clamp:
        sel[0, 1], sel[1, 2] = -1, n_cand

    def fresh():
        return torch.full((B, cap, width), 251, dtype=dtype, device=DEV) if dtype == torch.uint8 else \
            torch.full((B, cap, width), -7.0, dtype=dtype, device=DEV)

    # append: the piece's rows go behind the held ones; the uniform call needs no candidates in front of them in dst
    dst_u, dst_r = fresh(), fresh()
    hip.stream_commit([(held, held_rows, piece, dst_u)], None, M, n_cand)
    slides = torch.tensor([[held_rows, n_cand, 0, b * piece_rows, APPEND, 0] for b in range(B)], dtype=torch.int64, device=DEV)
    hip.stream_commit_ragged([(held, piece.reshape(B * piece_rows, width), dst_r)], None, slides, M, piece_rows)
    torch.cuda.synchronize()
    assert torch.equal(dst_u.view(torch.uint8), dst_r.view(torch.uint8))
    assert torch.equal(dst_u[:, held_rows:n_cand], piece) and torch.equal(dst_u[:, :held_rows], fresh()[:, :held_rows]) \
        and torch.equal(dst_u[:, n_cand:], fresh()[:, n_cand:])

    # select with a tail: M winners, then candidates [tail_first, n_cand)
    dst_u, dst_r = fresh(), fresh()
    hip.stream_commit([(held, held_rows, piece, dst_u)], sel, M, n_cand, tail_first)
    slides = torch.tensor([[held_rows, n_cand, tail_first, b * piece_rows, SELECT, 0] for b in range(B)], dtype=torch.int64, device=DEV)
    hip.stream_commit_ragged([(held, piece.reshape(B * piece_rows, width), dst_r)], sel, slides, M, M + n_cand - tail_first)
    torch.cuda.synchronize()
    assert torch.equal(dst_u.view(torch.uint8), dst_r.view(torch.uint8))
    cand = torch.cat((held[:, :held_rows], piece), dim=1)
    rows = torch.cat((sel.clamp(0, n_cand - 1), torch.arange(tail_first, n_cand, device=DEV).expand(B, -1)), dim=1)
    want = fresh()
    want[:, :rows.shape[1]] = torch.gather(cand, 1, rows.unsqueeze(-1).expand(-1, -1, width))
    assert torch.equal(dst_u, want)
    assert torch.equal(held, values(1, (B, cap, width))) and torch.equal(piece, values(1 + numel, (B, piece_rows, width)))
