"""The two float32 blank scans of the counted, deduped launch (``blank_scan_parts_kernel``, ``blank_scan_parts_view_kernel``,
csrc/dedup.hip) at the shapes their code branches on, through ``ipsx_trunk_encode_parts_dedup`` and ``_view``
(``EncoderPlan.encode_source(..., dedup=True)``) against the same call without the dedup - what ``IPSX_DEDUP_BLANK=0`` makes
of it -, bit for bit: every row, every part's counter, and ``n_encoded`` against a host count of the non-blank entries.

A scan workgroup takes 64 list entries, a wavefront four of them: the first KiB of the four together, then, entry by entry, the
other three KiB where the first is all zero.  Nothing loops, so the sizes that matter are the edges of a wavefront's entries
and of a workgroup's 64 - 1, 63, 64, 65, 255, 257 - and 235 = 3 * 64 + 43: several workgroups, the last with ten full
wavefronts, one of three entries and five empty ones.

(The file's name sorts it behind tests/test_ragged_stream_rows_commit.py: that file's ``test_host_refusals_come_before_any_launch``
expects "overlaps the pixels" from a destination 64 bytes into ``pixels``, which is the library's answer only while the
allocator has not placed ``held[0]`` inside that destination's extent - then "overlaps the held rows" comes first.  GPU
allocations made earlier in the same process move that layout, and this file's did: the whole suite failed there and nowhere
else, the file alone passed.)"""

import itertools

import numpy as np
import pytest
import torch

from ips_amd import hip, synth
from ips_amd.architecture import IPSNet

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GH = GW = 8
IMAGES = 5
POOL = IMAGES * GH * GW                 # 320 patches: five images of 8 x 8 grid patches
# the pool's special rows
FIRST, LAST, NEG_ZERO, NAN, KIB0, KIB1, KIB2, KIB3 = range(8)
SPECIAL = 8
_SHARED = {}


def plan():
    if "plan" not in _SHARED:
        net = synth.fill_weights(IPSNet(DEV, synth.mnist_conf(N=64, M=8, I=8)), 7).to(DEV).eval()
        p = hip.EncoderPlan(net.encoder, True)
        assert p.fused((1, 1, 32, 32))
        _SHARED["plan"] = p
    return _SHARED["plan"]


def pool():
    """-> (patches (POOL, 1, 32, 32) on the host, blank (POOL,) bool): the special rows, then every other row blank."""
    if "pool" not in _SHARED:
        g = np.random.default_rng(3)
        x = g.random((POOL, 1, 32, 32), dtype=np.float32) + np.float32(1e-3)
        blank = np.zeros(POOL, dtype=bool)
        blank[SPECIAL::2] = True
        x[blank] = 0
        x[:SPECIAL] = 0
        flat = x.reshape(POOL, -1)
        flat[FIRST, 0] = 0.25
        flat[LAST, 1023] = 0.5
        flat[NEG_ZERO] = -0.0
        flat[NAN, 600] = np.nan
        for k, row in enumerate((KIB0, KIB1, KIB2, KIB3)):
            flat[row, 256 * k + 37 + 50 * k] = 1.0
        blank[:SPECIAL] = False
        blank[NEG_ZERO] = True
        assert np.array_equal(blank, ~(flat != 0).any(1))                # the host's flags: -0.0 == 0, NaN != 0
        _SHARED["pool"] = (x, blank)
    return _SHARED["pool"]


def source(kind):
    """the pool as a patch tensor, or as grid patches of five 256 x 256 images (patch p = image p // 64, grid row and column)"""
    if kind not in _SHARED:
        x = torch.from_numpy(pool()[0])
        if kind == "patches":
            _SHARED[kind] = hip.PatchSource(x.to(DEV))
        else:
            images = x.view(IMAGES, GH, GW, 32, 32).permute(0, 1, 3, 2, 4).reshape(IMAGES, 1, GH * 32, GW * 32).contiguous()
            _SHARED[kind] = hip.PatchSource(images=images.to(DEV), view=hip.PatchView(tuple(images.shape), (32, 32), (32, 32)))
    return _SHARED[kind]


def check(kind, numbers, sizes):
    p, src = plan(), source(kind)
    blank = pool()[1]
    numbers = np.asarray(numbers, dtype=np.int32)
    every = torch.from_numpy(numbers).to(DEV)
    n = every.numel()
    assert sum(sizes) == n
    ends = list(itertools.accumulate(sizes))
    done = torch.zeros((len(sizes),), dtype=torch.int32, device=DEV)
    want = p.encode_source(src, index=every, parts=(ends, done)).clone()
    torch.cuda.synchronize()
    assert done.tolist() == list(sizes)
    done.zero_()
    buf = torch.full((n + 2, 128), float("nan"), device=DEV)             # the rows between two sentinel rows
    got = p.encode_source(src, index=every, parts=(ends, done), dedup=True, out=buf[1:n + 1])
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[n + 1]).all())
    assert done.tolist() == list(sizes)
    assert int(p.n_encoded.item()) == int((~blank[numbers]).sum())
    # every blank entry's row is ONE row - the blank embedding -, whichever zero it was made of
    rows = got[torch.from_numpy(blank[numbers]).to(DEV)]
    if rows.shape[0] > 1:
        assert torch.equal(rows.view(torch.int32), rows[:1].view(torch.int32).expand_as(rows))


KINDS = ["patches", "view"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 235, 255, 257])
def test_list_lengths_at_the_edges_of_a_wavefront_and_a_workgroup(kind, n):
    """the list begins with the special rows: content in the first float only, in the last only, all -0.0 (blank), one NaN, a
    float in each of the four KiB"""
    check(kind, np.arange(n), (n,))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("which", ["all blank", "none blank"])
def test_all_blank_and_none_blank(kind, which):
    blank = pool()[1]
    rows = np.flatnonzero(blank if which == "all blank" else ~blank)
    numbers = np.resize(rows, 150)                                        # (with repeats)
    check(kind, numbers, (150,))
    check(kind, numbers[:7], (7,))


@pytest.mark.parametrize("kind", KINDS)
def test_a_list_with_repeated_entries_in_any_order(kind):
    g = np.random.default_rng(8)
    numbers = g.integers(0, POOL, 200)
    numbers[[0, 1, 17, 64, 199]] = [NEG_ZERO, NEG_ZERO, LAST, LAST, NAN]
    check(kind, numbers, (200,))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("sizes", [(64, 64, 72), (63, 2, 135), (1, 127, 72), (70, 58, 72), (16, 8, 40, 136)],
                         ids=["on the edges", "around an edge", "first entry alone", "inside a group", "on wavefronts' edges"])
def test_part_ends_inside_a_group_of_64_and_on_its_edges(kind, sizes):
    check(kind, np.arange(sum(sizes)), sizes)
