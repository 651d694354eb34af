"""``hip.stream_commit_ragged(..., pixels=, view=)`` (``ipsx_stream_commit_ragged_view``) against its sibling on
the unfolded packed patches: every load tier at shifted buffer bases for float32 and uint8, poisoned pixels between and
around the patches and the images, sentinel-filled destinations, more slides than view entries in all four modes, a
selection that leaves the candidates, slides that contradict a table, and the host refusals."""

import ctypes as C
import gc

import pytest
import torch

from ips_amd import hip
from view_cases import guarded_images, unfold
from view_u8_cases import guarded_images_u8

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32_SENTINEL, U8_SENTINEL = 7e30, 254
M, TAIL = 6, 2

# name: (C, window sizes (rows_b, W_b), patch, stride)
SETS = {
    "p32_s16": (1, [(64, 160), (48, 96), (32, 128)], (32, 32), (16, 16)),          # the 16-byte tier
    "p32_s16_w161": (1, [(64, 161), (48, 96), (32, 128)], (32, 32), (16, 16)),     # a row pitch that is no multiple of 4 pixels
    "p32_s16x6": (1, [(64, 160), (48, 96), (32, 128)], (32, 32), (16, 6)),         # a column stride that is no multiple of 4 pixels
    "p50_s25": (1, [(75, 125), (50, 100)], (50, 50), (25, 25)),
    "p100x3": (3, [(150, 212), (100, 200)], (100, 100), (50, 100)),
}


def tier(case, elem, k_bytes):
    """The width the launch must take, from the numbers: the widest of 16 / 4 / 1 bytes that divides the buffer's address,
    every image's byte offset (multiples of 16 elements here) and every w, sw and pw in bytes (the tables come from the
    allocator: 256-byte aligned)."""
    _, sizes, (_, pw), (_, sw) = case
    for u in (16, 4, 1):
        if all(v % u == 0 for v in [k_bytes, 16 * elem, sw * elem, pw * elem] + [w * elem for _, w in sizes]):
            return u


def test_the_tiers_of_the_sets_written_out():
    got = {(n, e): tier(c, e, 0) for n, c in SETS.items() for e in (4, 1)}
    assert got == {("p32_s16", 4): 16, ("p32_s16", 1): 16, ("p32_s16_w161", 4): 4, ("p32_s16_w161", 1): 1,
                   ("p32_s16x6", 4): 4, ("p32_s16x6", 1): 1, ("p50_s25", 4): 4, ("p50_s25", 1): 1,
                   ("p100x3", 4): 16, ("p100x3", 1): 4}
    assert tier(SETS["p32_s16"], 4, 4) == 4 and tier(SETS["p100x3"], 1, 4) == 4
    assert [tier(SETS["p32_s16"], 1, k) for k in (1, 2, 4)] == [1, 1, 4]


def packed_windows(case, u8, k):
    """The packed 1-d pixel buffer of a feed -> (pixels, element offsets, packed patches).  Pixels no patch covers are NaN /
    255 and so is everything between and around the images; the buffer starts k elements past a 16-byte boundary."""
    c, sizes, patch, stride = case
    guard, gap = 4096, 48
    offs, end = [], 0
    for h, w in sizes:
        offs.append((end + gap + 15) // 16 * 16)
        end = offs[-1] + c * h * w
    buf = torch.full((guard + k + end + guard,), 255 if u8 else float("nan"), dtype=torch.uint8 if u8 else torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    pixels = buf[guard + k:guard + k + end]
    patches = []
    for (h, w), o in zip(sizes, offs):
        g = (1, c, h, w, patch, stride)
        im = guarded_images_u8(g, 0, device=DEV) if u8 else guarded_images(g, 0, device=DEV)
        pixels[o:o + c * h * w].copy_(im.reshape(-1))
        patches.append(unfold(im, patch, stride)[0])
    patches = torch.cat(patches)
    assert not (patches == 255).any() if u8 else bool(torch.isfinite(patches).all())
    return pixels, offs, patches


def slides_of(count):
    """Four slides on a view of fewer entries - idle, append, select, move - whose pieces are three ranges of the packed
    patches that end inside images -> ((B, 6) rows, the cap every table needs)."""
    n_a = n_s = count // 4
    n_m = count - n_a - n_s                                            # (the move slide has the most candidates)
    held = [2, 3, M + 2, 1]
    cand = [2, 3 + n_a, M + 2 + n_s, 1 + n_m]
    rows = [[held[0], cand[0], 0, 0, hip.COMMIT_IDLE, 0],
            [held[1], cand[1], 0, 0, hip.COMMIT_APPEND, 0],
            [held[2], cand[2], cand[2] - TAIL, n_a, hip.COMMIT_SELECT, 0],
            [held[3], cand[3], 0, n_a + n_s, hip.COMMIT_MOVE, 0]]
    return rows, max(cand) + 1


def selection(rows):
    """below 0 and beyond the candidates, the held segment, both sides of the seam, the last patch"""
    held, cand = rows[2][0], rows[2][1]
    sel = torch.zeros((4, M), dtype=torch.int64)
    sel[2] = torch.tensor([-3, 1 << 40, held - 1, held, cand - 1, 2])
    sel[0] = sel[1] = sel[3] = torch.tensor([5, 4, 3, 2, 1, 0])
    return sel.to(DEV)


def state(case, u8, k, seed):
    c, sizes, patch, stride = case
    pixels, offs, patches = packed_windows(case, u8, k)
    view = hip.RaggedView(c, sizes, offs, patch, stride)
    assert view.count == patches.shape[0]
    rows, cap = slides_of(view.count)
    gen = torch.Generator().manual_seed(seed)
    shape = tuple(patches.shape[1:])
    held = [(torch.randint(0, 251, (4, cap) + shape, generator=gen, dtype=torch.uint8) if u8 else torch.randn((4, cap) + shape, generator=gen)).to(DEV),
            torch.randn((4, cap, 128), generator=gen).to(DEV), torch.arange(4 * cap, dtype=torch.int64, device=DEV).view(4, cap),
            torch.randn((4, cap, 32), generator=gen).to(DEV)]
    pieces = [patches, torch.randn((view.count, 128), generator=gen).to(DEV), torch.arange(1000, 1000 + view.count, dtype=torch.int64, device=DEV),
              torch.randn((view.count, 32), generator=gen).to(DEV)]
    return pixels, view, rows, cap, held, pieces


def sentinels(held, rows):
    return [torch.full((4, rows) + tuple(h.shape[2:]), -5 if h.dtype == torch.int64 else (U8_SENTINEL if h.dtype == torch.uint8 else F32_SENTINEL),
                       dtype=h.dtype, device=DEV) for h in held]


def check_commit(name, u8, k):
    case = SETS[name]
    pixels, view, rows, cap, held, pieces = state(case, u8, k, 17 * k + len(name))
    elem = pixels.element_size()
    assert pixels.data_ptr() % 16 == (k * elem) % 16
    want_tier = tier(case, elem, k * elem)
    slides = torch.tensor(rows, dtype=torch.int64, device=DEV)
    sel = selection(rows)
    # in place: the append slide's piece goes behind its held rows; the slides that select or move there are not touched
    got, want = [h.clone() for h in held], [h.clone() for h in held]
    unit = hip.stream_commit_ragged([(got[0], None, got[0])] + [(got[t], pieces[t], got[t]) for t in (1, 2, 3)], sel, slides, M, cap,
                                    pixels=pixels, view=view)
    assert hip.stream_commit_ragged([(want[t], pieces[t], want[t]) for t in range(4)], sel, slides, M, cap) is None
    assert unit == want_tier, (name, u8, k, unit)
    n_a = rows[1][1] - rows[1][0]
    for t in range(4):
        assert torch.equal(got[t], want[t]), (name, u8, k, "in place", t)
        assert torch.equal(got[t][[0, 2, 3]], held[t][[0, 2, 3]]) and torch.equal(got[t][1, rows[1][1]:], held[t][1, rows[1][1]:])
    assert torch.equal(got[0][1, rows[1][0]:rows[1][1]], pieces[0][:n_a])
    # apart: append behind the rows in front, select (clamped), move; sentinels everywhere else, a guard row behind every slide
    got, want = sentinels(held, cap + 1), sentinels(held, cap + 1)
    unit = hip.stream_commit_ragged([(held[0], None, got[0]), (held[1], pieces[1], got[1]), (held[2], pieces[2], got[2]), (held[3], None, got[3])],
                                    sel, slides, M, cap, pixels=pixels, view=view)
    lg = held[3]                                                       # (the logits table holds every candidate itself)
    hip.stream_commit_ragged([(held[0], pieces[0], want[0]), (held[1], pieces[1], want[1]), (held[2], pieces[2], want[2]), (lg, None, want[3])],
                             sel, slides, M, cap)
    assert unit == want_tier
    for t in range(4):
        assert torch.equal(got[t], want[t]), (name, u8, k, "apart", t)
    fill = U8_SENTINEL if u8 else F32_SENTINEL
    written = [0, rows[1][1], M + TAIL, rows[3][1]]                    # rows [.., written) of each slide may have changed
    for b in range(4):
        assert bool((got[0][b, written[b]:] == fill).all()) and bool((got[2][b, written[b]:] == -5).all())
    assert bool((got[0][1, :rows[1][0]] == fill).all())                # append: the rows in front stay
    assert not (got[0][2, :M + TAIL] == 255).any() if u8 else bool(torch.isfinite(got[0]).all())
    cand2 = torch.cat((held[0][2, :rows[2][0]], pieces[0][rows[2][3]:rows[2][3] + rows[2][1] - rows[2][0]]))
    assert torch.equal(got[0][2, :M], cand2[sel[2].clamp(0, rows[2][1] - 1)]) and torch.equal(got[0][2, M:M + TAIL], cand2[-TAIL:])
    cand3 = torch.cat((held[0][3, :1], pieces[0][rows[3][3]:]))
    assert torch.equal(got[0][3, :rows[3][1]], cand3)
    torch.cuda.synchronize()


@pytest.mark.parametrize("k", [0, 1], ids=["base+0", "base+4"])
@pytest.mark.parametrize("name", list(SETS))
def test_the_view_commit_equals_the_commit_of_the_unfolded_patches_float32(name, k):
    check_commit(name, False, k)


@pytest.mark.parametrize("k", [0, 1, 2, 4])
@pytest.mark.parametrize("name", list(SETS))
def test_the_view_commit_equals_the_commit_of_the_unfolded_patches_uint8(name, k):
    check_commit(name, True, k)


@pytest.mark.parametrize("what", ["first_leaves_the_view", "cand_beyond_dst_rows", "select_without_sel"])
def test_a_slide_that_contradicts_a_table_is_left_untouched_in_all_of_them(what):
    pixels, view, rows, cap, held, pieces = state(SETS["p32_s16_w161"], False, 1, 3)
    sel, dst_rows, b = selection(rows), cap + 1, 2
    if what == "first_leaves_the_view":
        rows[2][3] = view.count - (rows[2][1] - rows[2][0]) + 1
    elif what == "cand_beyond_dst_rows":
        b, dst_rows = 3, rows[3][1] - 1                                # the move slide writes one row more than there is
        assert dst_rows >= max(M + TAIL, rows[1][1])
    else:
        sel = None
    slides = torch.tensor(rows, dtype=torch.int64, device=DEV)
    got, want = sentinels(held, dst_rows), sentinels(held, dst_rows)
    hip.stream_commit_ragged([(held[0], None, got[0]), (held[1], pieces[1], got[1]), (held[2], pieces[2], got[2]), (held[3], None, got[3])],
                             sel, slides, M, cap, pixels=pixels, view=view)
    hip.stream_commit_ragged([(held[0], pieces[0], want[0]), (held[1], pieces[1], want[1]), (held[2], pieces[2], want[2]), (held[3], None, want[3])],
                             sel, slides, M, cap)
    clean = sentinels(held, dst_rows)
    for t in range(4):
        assert torch.equal(got[t][b], clean[t][b]), (what, t)
        assert torch.equal(got[t], want[t]), (what, t)
    other = 3 if b == 2 else 2
    assert not torch.equal(got[0][other], clean[0][other])             # (the launch did run: the other slides moved)
    torch.cuda.synchronize()


def test_host_refusals_come_before_any_launch():
    case = SETS["p32_s16"]
    pixels, view, rows, cap, held, pieces = state(case, False, 0, 4)
    slides = torch.tensor(rows, dtype=torch.int64, device=DEV)
    sel = selection(rows)
    dst = sentinels(held, cap + 1)
    clean = [d.clone() for d in dst]
    lib = hip.lib()
    view.on(DEV)                                                       # (the view's table goes up once, here)
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_allocated(DEV)

    def tables(**change):
        arr = (hip.StreamTable * 2)()
        for t in (0, 1):
            arr[t].held, arr[t].held_rows, arr[t].held_bstride_rows = held[t].data_ptr(), cap, cap
            arr[t].dst, arr[t].dst_rows, arr[t].dst_bstride_rows = dst[t].data_ptr(), cap + 1, cap + 1
            arr[t].row_bytes = held[t][0, 0].numel() * held[t].element_size()
        arr[1].piece = pieces[1].data_ptr()
        for key, v in change.items():
            setattr(arr[0], key, v)
        return arr

    def raw(arr, elem=4, px=None, vw=None):
        unit = C.c_int(-1)
        px = pixels.data_ptr() if px is None else px
        rc = lib.ipsx_stream_commit_ragged_view(arr, 2, C.c_void_p(px), C.byref((vw or view).on(DEV).struct), elem, C.c_void_p(sel.data_ptr()),
                                                C.c_void_p(slides.data_ptr()), 4, M, cap, view.count, C.byref(unit), None)
        return rc, lib.ipsx_last_error().decode()

    # (the valid call first: it is what the refusals below differ from)
    assert raw(tables())[0] == 0
    torch.cuda.synchronize()
    for d, c in zip(dst[:2], clean[:2]):
        assert not torch.equal(d, c)
        d.copy_(c)
    torch.cuda.synchronize()
    for arr, kw, word in [(tables(piece=pieces[0].data_ptr()), {}, "no piece pointer"),
                          (tables(row_bytes=4 * 32 * 16), {}, "rows of"),
                          (tables(), dict(elem=2), "element of 2 bytes"),
                          (tables(dst=pixels.data_ptr() + 64), {}, "overlaps the pixels"),
                          (tables(dst=held[0].data_ptr() + 4096), {}, "overlaps the held rows"),      # what the sibling refuses
                          (tables(dst_rows=0), {}, "destination of 0 rows"),
                          (tables(), dict(px=0), "null pixels")]:
        rc, msg = raw(arr, **kw)
        assert rc != 0 and word in msg, (word, rc, msg)
    broken = hip.RaggedView(case[0], case[1], view.elem_offsets, case[2], case[3])
    broken.table[1].ny += 1                                            # a host table that is not the geometry's
    rc, msg = raw(tables(), vw=broken)
    assert rc != 0 and "grid" in msg
    torch.cuda.synchronize()
    # ... and through the wrapper
    for exc, tabs, kw in [(ValueError, [(held[0], pieces[0], dst[0])], dict(pixels=pixels, view=view)),
                          (ValueError, [(held[1], None, dst[1])], dict(pixels=pixels, view=view)),            # rows that are no patch
                          (TypeError, [(held[0], None, dst[0])], dict(pixels=pixels.double(), view=view)),
                          (ValueError, [(held[0], None, dst[0])], dict(pixels=pixels.view(1, -1), view=view)),
                          (ValueError, [(held[0], None, dst[0])], dict(pixels=pixels)),
                          (RuntimeError, [(held[0], None, dst[0]), (held[1], dst[1].view(-1, 128)[:view.count], dst[1])],
                           dict(pixels=pixels, view=view))]:                                                   # the destination overlaps the piece
        with pytest.raises(exc):
            hip.stream_commit_ragged(tabs, sel, slides, M, cap, **kw)
    del kw, tabs
    torch.cuda.synchronize()
    for d, c in zip(dst, clean):
        assert torch.equal(d, c)
    del broken
    gc.collect()                                                       # (the tracebacks of the refusals hold the test's own tensors)
    assert torch.cuda.memory_allocated(DEV) == allocated
