"""Exact blank-patch dedup inside the one counted launch on the three sources that went without it
(``ipsx_trunk_encode_parts_dedup_u8`` / ``_view`` / ``_view_u8``): uint8 patches with their table, a view of float32 images, a
view of uint8 images.  Kernel level, after ``tests/test_dedup_parts.py::check``: the embeddings are bit for bit those of the
counted launch WITHOUT dedup on the same source and lists (``encode_source(..., dedup=False)``, which the existing tests hold
to the oracle), they lie between untouched sentinel rows, every part's counter ends on the part's size and ``n_encoded`` is the
host's count of non-blank entries - blank worked out on the host from the unfolded input: all elements zero (floats, -0.0
among them), every byte 0 (bytes, whatever the table makes of byte 0)."""

import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from ips_amd import hip, quant, synth
from ips_amd.architecture import IPSNet

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

_SHARED = {}
POOL = 1200                    # uint8 patches of the pool
ZERO_BYTE = 7                  # a non-zero byte whose table entry is 0.0f in both tables
TABLES = ("zero", "norm")
# (H, W, stride, the load width the launcher must pick): float32 images 16-byte loads / dwords, uint8 images 16 / 4 / 1 bytes
F32_VIEWS = {"wide": (200, 232, (24, 8), 16), "dword": (200, 233, (24, 6), 0)}
U8_VIEWS = {"b16": (200, 240, (24, 16), 16), "b4": (200, 236, (24, 4), 4), "b1": (200, 235, (24, 5), 1)}
SOURCES = (["u8 " + t for t in TABLES] + ["view " + g for g in F32_VIEWS] +
           ["view_u8 %s %s" % (g, t) for g in U8_VIEWS for t in TABLES])


def plan():
    if "plan" not in _SHARED:
        net = synth.fill_weights(IPSNet(DEV, synth.mnist_conf(N=64, M=8, I=8)), 7).to(DEV).eval()
        p = hip.EncoderPlan(net.encoder, True)
        assert p.fused((1, 1, 32, 32))
        _SHARED["plan"] = (p, net)
    return _SHARED["plan"][0]


def table(name):
    """"zero": ToTensor's table, table[0][0] == 0.0f; "norm": a normalising table, table[0][0] != 0.0f.  In both the entry of
    byte ZERO_BYTE is 0.0f: a patch of that byte holds only zeros as floats and is still NOT blank by the rule for bytes."""
    if ("table", name) not in _SHARED:
        t = quant.patch_table(1) if name == "zero" else quant.patch_table(1, mean=[0.1307], std=[0.3081])
        t[0, ZERO_BYTE] = 0.0
        assert (float(t[0, 0]) == 0.0) == (name == "zero")
        _SHARED[("table", name)] = t.to(DEV)
    return _SHARED[("table", name)]


def unfolded(images, stride):
    """(B * ny * nx, 1024) on the host: the patch tensor a view stands for, in the grid's order."""
    u = images.cpu().unfold(2, 32, stride[0]).unfold(3, 32, stride[1])           # (B, 1, ny, nx, 32, 32)
    return u.reshape(-1, 1024)


def blobs(shape, rng, count):
    """(B, 1, H, W) float64 in [0.05, 1): zero but for `count` seeded rectangles per image."""
    B, _, H, W = shape
    x = np.zeros(shape)
    for b in range(B):
        for _ in range(count):
            y0, x0 = rng.integers(0, H - 8), rng.integers(0, W - 8)
            h, w = rng.integers(3, 40), rng.integers(3, 40)
            x[b, 0, y0:y0 + h, x0:x0 + w] = 0.05 + 0.95 * rng.random((min(h, H - y0), min(w, W - x0)))
    return x


def source(name):
    """-> (hip.PatchSource, blank (count,) bool on the host, special entries {"blank": [...], "full": [...]})."""
    if ("src", name) in _SHARED:
        return _SHARED[("src", name)]
    kind, *rest = name.split()
    rng = np.random.default_rng(len(name) * 131 + sum(map(ord, name)))
    if kind == "u8":
        q = rng.integers(0, 256, (POOL, 1, 32, 32), dtype=np.uint8)
        q[rng.random(POOL) < 0.5] = 0                                    # the seeded blank share
        q[3] = 0
        q[3, 0, 31, 31] = 1                                              # only the LAST byte is 1
        q[4] = ZERO_BYTE                                                 # every pixel 0.0f, no byte 0: not blank by the rule
        q[5] = 0
        q = torch.from_numpy(q)
        blank = (q.reshape(POOL, -1) == 0).all(1).numpy()
        assert blank[5] and not blank[3] and not blank[4]
        src = hip.PatchSource(q.to(DEV), table(rest[0]))
        special = {"blank": [5], "full": [3, 4]}
    else:
        H, W, stride, width = (F32_VIEWS if kind == "view" else U8_VIEWS)[rest[0]]
        shape = (3, 1, H, W)
        x = blobs(shape, rng, 12)
        x[1] = 0                      # image 1: nothing but the special windows below
        ny, nx = (H - 32) // stride[0] + 1, (W - 32) // stride[1] + 1
        corner, late = (ny + 2) * nx + 3, (ny + 5) * nx + nx - 2         # grid patches (1, 2, 3) and (1, 5, nx - 2)

        def at(p, y, xx):             # pixel (y, xx) of grid patch p of image 1
            py, px = divmod(p - ny * nx, nx)
            return (1, 0, py * stride[0] + y, px * stride[1] + xx)

        if kind == "view":
            f = x.astype(np.float32)
            f[2] = -0.0               # image 2: all -0.0, every patch blank
            f[at(corner, 31, 31)] = 0.5                                   # only the bottom-right pixel of its window
            f.view(np.uint32)[at(late, 11, 6)] = 1                        # one denormal, in patch rows 8 - 15
            images = torch.from_numpy(f)
            view = hip.PatchView(shape, (32, 32), stride)
            src = hip.PatchSource(images=images.to(DEV), view=view)
            assert view.load_bytes(src.images, (16,)) == width
        else:
            b = np.ceil(x * 255).astype(np.uint8)                         # (blobs: bytes 13 .. 255)
            b[2] = 0
            b[at(corner, 31, 31)] = 1
            b[at(late, 11, 6)] = ZERO_BYTE                                # a byte that stands for 0.0f: the window is not blank
            images = torch.from_numpy(b)
            view = hip.PatchView(shape, (32, 32), stride)
            src = hip.PatchSource(images=images.to(DEV), view=view, table=table(rest[1]))
            assert view.load_bytes(src.images, (16, 4, 1)) == width
        assert view.count == 3 * ny * nx
        u = unfolded(images, stride)
        blank = (u == 0).all(1).numpy()                                   # (-0.0 == 0)
        assert not blank[corner] and not blank[late] and blank[2 * ny * nx:].all()
        assert int((u[corner] != 0).sum()) == 1 and int((u[late] != 0).sum()) == 1
        assert bool(u[corner, 1023] != 0) and bool(u[late, 11 * 32 + 6] != 0)
        special = {"blank": [2 * ny * nx + 1, view.count - 1], "full": [corner, late]}
    assert blank.sum() >= 20 and (~blank).sum() >= 20
    _SHARED[("src", name)] = (src, blank, special)
    return _SHARED[("src", name)]


def draw(name, n, frac, seed=0):
    """A list of n entries of the source, round(n frac) of them blank, drawn with repeats and permuted; the source's special
    entries of either class lead the draws of that class."""
    _, blank, special = source(name)
    g = np.random.default_rng(1000 * n + int(frac * 100) + seed)
    k = int(round(n * frac))
    picks = []
    for cls, rows, m in (("blank", np.flatnonzero(blank), k), ("full", np.flatnonzero(~blank), n - k)):
        got = rows[g.integers(0, rows.size, m)]
        lead = special[cls][:m]
        got[:len(lead)] = lead
        picks.append(got)
    return np.concatenate(picks)[g.permutation(n)]


def check(name, numbers, sizes):
    """The list ``numbers`` cut into parts of ``sizes``: the counted launch with dedup against the one without."""
    p = plan()
    src, blank, _ = source(name)
    every = torch.as_tensor(np.asarray(numbers, dtype=np.int32)).to(DEV)
    n = every.numel()
    assert sum(sizes) == n
    ends = list(itertools.accumulate(sizes))
    done = torch.zeros((len(sizes),), dtype=torch.int32, device=DEV)
    want = p.encode_source(src, index=every, parts=(ends, done), dedup=False)
    torch.cuda.synchronize()
    assert done.tolist() == list(sizes) and bool(torch.isfinite(want).all())
    done.zero_()
    buf = torch.full((n + 2, 128), float("nan"), device=DEV)             # emb between two sentinel rows
    p.n_encoded = None
    got = p.encode_source(src, index=every, parts=(ends, done), dedup=True, out=buf[1:n + 1])
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[n + 1]).all())
    assert done.tolist() == list(sizes)
    assert int(p.n_encoded.item()) == int((~blank[np.asarray(numbers)]).sum())
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))    # bit for bit (-0.0 and +0.0 differ)


@pytest.mark.parametrize("frac", [0, 0.5, 0.93, 1])
@pytest.mark.parametrize("n,sizes", [(37, (37,)), (37, (20, 17)), (1100, (700, 300, 60, 40))], ids=["37", "37 in 2", "1100 in 4"])
@pytest.mark.parametrize("name", SOURCES)
def test_list_lengths_and_blank_fractions(name, n, sizes, frac):
    """37: one scan workgroup with a tail, a compacted count that is no multiple of 8; 1,100: 18 scan workgroups, 5 compaction
    workgroups, entries repeated and permuted.  frac 1: nothing to encode, the scan alone writes every row and fills every
    counter (``n_encoded`` 0); frac 0: no blank entry, the scan writes no row."""
    numbers = draw(name, n, frac)
    blank = source(name)[1][numbers]
    assert blank.sum() == int(round(n * frac))
    check(name, numbers, sizes)
    if frac == 1:
        assert int(plan().n_encoded.item()) == 0
    if frac == 0:
        assert int(plan().n_encoded.item()) == n


@pytest.mark.parametrize("name", SOURCES)
def test_sixteen_parts(name):
    sizes = (1, 2, 9, 3, 17, 1, 8, 5, 4, 30, 2, 7, 11, 6, 1, 13)
    check(name, draw(name, sum(sizes), 0.5, seed=16), sizes)


@pytest.mark.parametrize("order", ["blank dense sparse", "dense blank sparse"])
@pytest.mark.parametrize("few", [1, 2])
@pytest.mark.parametrize("name", SOURCES)
def test_workgroups_that_straddle_parts(name, few, order):
    """Three parts: one without a non-blank entry, one without a blank one (6 entries), one of 9 with ``few`` non-blank ones.
    The trunk's first workgroup then holds entries of two parts, or of the first and the third with the empty one between."""
    _, blank, _ = source(name)
    zero, full = np.flatnonzero(blank)[:40], np.flatnonzero(~blank)[:40]
    parts = {"blank": zero[:5], "dense": full[:6], "sparse": np.concatenate([zero[5:9], full[6:6 + few], zero[9:14 - few]])}
    lists = [parts[k] for k in order.split()]
    check(name, np.concatenate(lists), tuple(len(l) for l in lists))


# ---------------------------------------------------------------------------------------------------- the blank embeddings
@pytest.mark.parametrize("name", [s for s in SOURCES if s.startswith("view")])
def test_a_view_shares_its_tensor_kinds_blank_embedding(name):
    """``EncoderPlan.blank_embedding`` makes a view's row with the TENSOR kind's kernel (``ipsx_trunk_encode_parts`` /
    ``_parts_u8`` on one patch): the view kind's own kernel on one blank patch - a 32 x 32 image of zeros / of zero bytes,
    through the source's table - must give that row's bits."""
    p = plan()
    src = source(name)[0]
    shared = p.blank_embedding(src).clone()
    one = hip.PatchView((1, 1, 32, 32), (32, 32), (32, 32))
    image = torch.zeros((1, 1, 32, 32), dtype=src.dtype, device=DEV)
    words = torch.zeros((2,), dtype=torch.int32, device=DEV)
    own = p.encode_source(hip.PatchSource(images=image, view=one, table=src.table), index=words[:1], parts=([1], words[1:]))
    torch.cuda.synchronize()
    assert int(words[1]) == 1 and bool(torch.isfinite(own).all())
    assert torch.equal(own.view(torch.int32), shared.view(torch.int32))


def test_the_blank_embedding_follows_the_table():
    """Bytes: the blank row is the embedding of a patch of table[0][0] - one per table, renewed when the table is written in
    place, and apart from the float32 kinds' row unless table[0][0] is 0.0f."""
    p = plan()
    f32 = p.blank_embedding(source("view wide")[0]).clone()
    zero = p.blank_embedding(source("u8 zero")[0]).clone()
    norm = p.blank_embedding(source("u8 norm")[0]).clone()
    assert torch.equal(zero.view(torch.int32), f32.view(torch.int32)) and not torch.equal(norm, f32)
    mine = table("norm").clone()
    src = hip.PatchSource(source("u8 norm")[0].patches, mine)
    assert torch.equal(p.blank_embedding(src), norm)
    held = p.blank_emb
    assert p.blank_embedding(src) is held                                # kept while the table stands
    mine[0, 0] = 0.0                                                      # (in place: the version counter moves)
    assert torch.equal(p.blank_embedding(src), f32) and p.blank_emb is not held
    assert torch.equal(p.blank_embedding(source("view wide")[0]), f32)


# ---------------------------------------------------------------------------------------------------- refusals
def raw(p, src, every, ends, done, buf, blank, table_ptr="own", workspace=True):
    """The source's dedup export itself, on a caller's buffers -> its return code."""
    L, n = hip.lib(), every.numel()
    tab = (hip._p(src.table),) if src.table is not None else ()
    if table_ptr is None:
        tab = (C.c_void_p(0),)
    vs = (C.byref(src.view.struct),) if src.is_view else ()
    name = "ipsx_trunk_encode_parts_dedup" + ("_view" if src.is_view else "") + ("_u8" if src.table is not None else "")
    nb = L.ipsx_trunk_parts_dedup_workspace_bytes(C.byref(p.trunk), n)
    ws = torch.empty((nb,), dtype=torch.uint8, device=DEV)
    return getattr(L, name)(C.byref(p.trunk), hip._p(src.base), *tab, *vs, hip._p(every), n, hip._p(buf),
                            (C.c_int64 * len(ends))(*ends), len(ends), hip._p(done), hip._p(blank), hip._p(ws),
                            nb if workspace else nb - 8, None, hip._stream())


@pytest.mark.parametrize("name", ["u8 norm", "view wide", "view_u8 b4 norm"])
def test_refusals_launch_nothing(name):
    p = plan()
    src = source(name)[0]
    blank = p.blank_embedding(src)                                        # (made while the plan is whole)
    every = torch.as_tensor(draw(name, 24, 0.5).astype(np.int32)).to(DEV)
    done = torch.zeros((2,), dtype=torch.int32, device=DEV)
    buf = torch.full((24, 128), float("nan"), device=DEV)
    assert p.fused(src.shape)
    p.trunk.precision = 1
    try:
        with pytest.raises(Exception):
            p.encode_source(src, index=every, parts=([8, 24], done), dedup=True, out=buf)
        assert raw(p, src, every, [8, 24], done, buf, blank) != 0
    finally:
        p.trunk.precision = 0
    with pytest.raises(Exception):
        p.encode_source(src, index=every, parts=([8, 16], done), dedup=True, out=buf)       # ends short of the list
    # what only the trunk launch would refuse - its 128 -> 128 convolutions' tile16 packing missing - is refused before the scan
    conv = p.trunk.blocks[3].conv[1]
    kept = conv.w_packed_bf16
    conv.w_packed_bf16 = None
    try:
        with pytest.raises(Exception):
            p.encode_source(src, index=every, parts=([8, 24], done), dedup=True, out=buf)
    finally:
        conv.w_packed_bf16 = kept
    assert p.fused(src.shape)
    assert raw(p, src, every, [8, 24], done, buf, blank, workspace=False) != 0               # a workspace 8 bytes short
    if src.table is not None:                                             # a byte source without its table
        assert raw(p, src, every, [8, 24], done, buf, blank, table_ptr=None) != 0
        assert b"trunk_encode_parts_dedup" in hip.lib().ipsx_last_error()
        with pytest.raises(TypeError):
            hip.PatchSource(src.patches, None) if not src.is_view else hip.PatchSource(images=src.images, view=src.view)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all()) and not bool(done.any())
    assert raw(p, src, every, [8, 24], done, buf, blank) == 0, hip.lib().ipsx_last_error()   # (the same buffers are fine otherwise)
    torch.cuda.synchronize()
    assert done.tolist() == [8, 16] and not bool(torch.isnan(buf).any())
