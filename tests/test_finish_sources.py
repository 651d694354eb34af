"""The finish launch of the padded ragged calls on its three sources - packed rows (``ipsx_ragged_finish``), a
float32 ragged view and a uint8 one with its table (``ipsx_ragged_finish_view``, ``_u8``) - which share ONE slot rule: the
device-side guards that nothing else tests, and the three sources against each other on the same pixels.

The pixels: ``image_ragged_cases.FUSED_MIXED`` as bytes (four images of 12, 9, 1 and 10 patches; M = 10: a long image, two short
ones and one of exactly M), the float32 expansion ``table[c][byte]`` of the same buffer, and the patches of that expansion
materialised as packed rows.  table[c][0] is 0.5, so the padding (+0.0) and a blank byte differ."""

import pytest
import torch

import image_ragged_cases as ic
import ragged_u8_cases as uc
import view_u8_cases as vu
from ips_amd import hip
from ips_amd.quant import dequant
from view_cases import unfold

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CASE, M, D = ic.FUSED_MIXED, 10, 32
SOURCES = ("rows", "view", "view_u8")


class Data:
    def __init__(self):
        c, sizes, patch, stride = CASE
        table = vu.guard_table(c).to(DEV)
        imgs = uc.guarded_images_u8(CASE)
        self.bytes, _ = uc.pack_u8(CASE, imgs, device=DEV)
        self.floats = uc.expanded(self.bytes, table)
        self.rows = torch.cat([unfold(dequant(im.to(DEV), table)[None], patch, stride)[0] for im in imgs]).contiguous()
        self.table, self.rview_u8, self.rview = table, self.bytes.view(patch, stride), self.floats.view(patch, stride)
        self.B, self.total, self.lengths, self.firsts = len(sizes), self.rview.count, self.rview.lengths, self.rview.firsts
        assert list(self.lengths) == [12, 9, 1, 10] and self.rows.shape == (self.total, c) + tuple(patch)
        assert float(table[0, 0]) != 0.0
        g = torch.Generator().manual_seed(23)
        self.mem_idx = torch.stack([torch.randperm(max(n, M), generator=g)[:M] % n for n in self.lengths]).to(DEV)
        self.offsets = torch.tensor(tuple(self.firsts) + (self.total,), dtype=torch.int64, device=DEV)
        self.flat = torch.cat([f + torch.randperm(n, generator=g) for f, n in zip(self.firsts, self.lengths)]).to(torch.int32).to(DEV)
        self.pos = torch.randn((self.total, D), generator=g).to(DEV)
        self._plain = {}

    def run(self, source, offsets=None, mem_idx="own", flat=None, pos=None):
        """One finish launch into buffers of NaN (indices: -7) -> (mem_patch, mem_pos | None, mem_idx, rows)."""
        offsets = self.offsets if offsets is None else offsets
        mem_idx = self.mem_idx if isinstance(mem_idx, str) else mem_idx
        nan = float("nan")
        bufs = (torch.full((self.B, M) + tuple(self.rows.shape[1:]), nan, device=DEV),
                torch.full((self.B, M, D), nan, device=DEV) if pos is not None else None,
                torch.full((self.B, M), -7, dtype=torch.int64, device=DEV), torch.full((self.B, M), -7, dtype=torch.int64, device=DEV))
        if source == "rows":
            out = hip.ragged_finish(self.rows, offsets, mem_idx, M, flat, pos, out=bufs)
        elif source == "view":
            out = hip.ragged_finish_view(self.floats.pixels, self.rview, offsets, mem_idx, M, flat, pos, out=bufs)
        else:
            out = hip.ragged_finish_view(self.bytes.pixels, self.rview_u8, offsets, mem_idx, M, flat, pos, out=bufs, table=self.table)
        torch.cuda.synchronize()
        return out

    def plain(self, source):
        """The unperturbed call with ``flat`` and ``pos``, made once per source."""
        if source not in self._plain:
            self._plain[source] = self.run(source, flat=self.flat, pos=self.pos)
        return self._plain[source]


@pytest.fixture(scope="module")
def data():
    return Data()


def same(got, want, rows=slice(None)):
    return all(ic.same_bits(g[rows], w[rows]) for g, w in zip(got, want))


def untouched(got, b):
    """Image b's slots of all four outputs still hold what the buffers were filled with."""
    patch, pos, idx, grow = got
    return bool(torch.isnan(patch[b]).all()) and bool(torch.isnan(pos[b]).all()) and idx[b].tolist() == [-7] * M == grow[b].tolist()


# ---------------------------------------------------------------- 1. the device guards
# (entry of the offsets, its value as a function of (firsts, total), the sources it is wrong for, the image that is refused)
PERTURBED = [
    ("past_the_total", -1, lambda f, t: t + 1, SOURCES, 3),
    ("before_the_table", 0, lambda f, t: -1, SOURCES, 0),
    ("end_before_start", 0, lambda f, t: f[1] + 1, SOURCES, 0),
    ("not_the_entrys_first", 0, lambda f, t: 1, ("view", "view_u8"), 0),
    ("not_the_entrys_length", -1, lambda f, t: t - 1, ("view", "view_u8"), 3),
]


# (packed rows have no table entry to disagree with: there the last two are another slide's offsets, not wrong ones)
GUARDED = [(source,) + p for p in PERTURBED for source in p[3]]


@pytest.mark.parametrize("source,name,entry,value,wrong_for,refused", GUARDED, ids=["%s-%s" % (g[1], g[0]) for g in GUARDED])
def test_an_image_whose_offsets_are_wrong_is_left_untouched(data, source, name, entry, value, wrong_for, refused):
    offsets = data.offsets.clone()
    offsets[entry] = value(data.firsts, data.total)
    got, want = data.run(source, offsets, flat=data.flat, pos=data.pos), data.plain(source)
    assert untouched(got, refused)
    others = [b for b in range(data.B) if b != refused]
    assert same(got, want, others) and bool(torch.isfinite(got[0][others]).all())


@pytest.mark.parametrize("source", SOURCES)
def test_without_a_selection_only_the_long_images_are_left_untouched(data, source):
    got, want = data.run(source, mem_idx=None, flat=data.flat, pos=data.pos), data.plain(source)
    long = [b for b, n in enumerate(data.lengths) if n > M]
    short = [b for b, n in enumerate(data.lengths) if n <= M]
    assert long == [0] and all(untouched(got, b) for b in long)
    assert same(got, want, short)


@pytest.mark.parametrize("source", SOURCES)
def test_selection_and_flat_entries_are_clamped(data, source):
    """mem_idx entries -5 and n + 3 select rows 0 and n - 1 of their own image; flat entries -1 and total + 7 read packed
    rows 0 and total - 1: the call equals the one that names those rows itself, bit for bit."""
    n = data.lengths[0]
    wild, tame = data.mem_idx.clone(), data.mem_idx.clone()
    wild[0, 2], wild[0, 7] = -5, n + 3
    tame[0, 2], tame[0, 7] = 0, n - 1
    assert same(data.run(source, mem_idx=wild, pos=data.pos), data.run(source, mem_idx=tame, pos=data.pos))
    # the image of exactly M patches uses every packed row of its own, so both entries are read
    g = data.firsts[3]
    wild, tame = data.flat.clone(), data.flat.clone()
    wild[g], wild[g + 1] = -1, data.total + 7
    tame[g], tame[g + 1] = 0, data.total - 1
    got = data.run(source, flat=wild, pos=data.pos)
    assert same(got, data.run(source, flat=tame, pos=data.pos))
    assert ic.same_bits(got[0][3, 0], data.rows[0]) and ic.same_bits(got[0][3, 1], data.rows[data.total - 1])
    assert got[3][3, :2].tolist() == [g, g + 1]                              # the packed row stays the slot's own


# ---------------------------------------------------------------- 2. the three sources agree
@pytest.mark.parametrize("with_flat", [False, True])
@pytest.mark.parametrize("with_pos", [False, True])
def test_the_three_sources_agree(data, with_flat, with_pos):
    flat, pos = data.flat if with_flat else None, data.pos if with_pos else None
    rows, view, view_u8 = (data.run(source, flat=flat, pos=pos) for source in SOURCES)
    for other in (view, view_u8):
        assert ic.same_bits(other[0], rows[0])                               # mem_patch: the bits of table[c][byte]
        assert (other[1] is None and rows[1] is None) if pos is None else ic.same_bits(other[1], rows[1])
        assert torch.equal(other[2], rows[2]) and torch.equal(other[3], rows[3])
    # ... and what they agree on is the rule: every slot written, +0.0 behind a short image's rows, index and row -1 there
    patch, _, idx, grow = view_u8
    assert bool(torch.isfinite(patch).all())
    for b, (f, n) in enumerate(zip(data.firsts, data.lengths)):
        valid = min(n, M)
        local = data.mem_idx[b] if n > M else torch.arange(M, device=DEV)
        src = f + local[:valid] if flat is None else flat[f + local[:valid]].to(torch.int64)
        assert ic.same_bits(patch[b, :valid], data.rows[src])
        assert idx[b, :valid].tolist() == local[:valid].tolist() and grow[b, :valid].tolist() == (f + local[:valid]).tolist()
        assert ic.same_bits(patch[b, valid:], torch.zeros_like(patch[b, valid:]))
        assert idx[b, valid:].tolist() == [-1] * (M - valid) == grow[b, valid:].tolist()
