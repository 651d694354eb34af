"""Host side of the one-launch route of the fused fp32 trunk (no GPU): the joined index list and the parts' ends that the
selection code hands to ``ipsx_trunk_encode_parts`` are the per-part lists one after the other, also through a shuffle
map, and the header declares the new entries under the unchanged ABI version."""

import os
import re

import pytest
import torch

from ips_amd import hip
from ips_amd.selection import Selection

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ipsx.h")
CPU = torch.device("cpu")

CASES = [(1, 40, [0, 24, 32, 40]),
         (2, 200, [0, 112, 176, 192, 200]),
         (16, 2500, [0, 1344, 2048, 2432, 2500]),           # the headline's cut
         (3, 17, [0, 16, 17])]


@pytest.mark.parametrize("B,N,edges", CASES)
def test_joined_list_is_the_parts_lists_one_after_the_other(B, N, edges):
    lists = Selection.part_lists(B, N, edges, CPU)
    ends = Selection.part_ends(B, edges)
    assert len(lists) == len(ends) == len(edges) - 1
    every = torch.cat(lists)
    assert every.dtype == torch.int32 and every.numel() == B * N == ends[-1]
    start = 0
    for k, (part, end) in enumerate(zip(lists, ends)):
        # part k: rows edges[k] .. edges[k + 1] of every image, image-major - patches[:, lo:hi].reshape(-1, ...)
        want = (torch.arange(B * N).view(B, N)[:, edges[k]:edges[k + 1]]).reshape(-1)
        assert torch.equal(part.long(), want)
        assert end - start == part.numel() and torch.equal(every[start:end], part)
        start = end
    assert torch.equal(every.long().sort().values, torch.arange(B * N))      # every patch exactly once


@pytest.mark.parametrize("B,N,edges", CASES)
@pytest.mark.parametrize("shared", [False, True])
def test_a_shuffle_map_composes_into_the_joined_list(B, N, edges, shared):
    g = torch.Generator().manual_seed(B * N + shared)
    order = torch.stack([torch.randperm(N, generator=g) for _ in range(1 if shared else B)])
    flat = (order.expand(B, -1) + torch.arange(B).unsqueeze(1) * N).to(torch.int32)       # what Selection.flat_index builds
    every = torch.index_select(flat.reshape(-1), 0, Selection.part_map(B, N, edges, CPU))
    ends = Selection.part_ends(B, edges)
    parts = [flat[:, edges[k]:edges[k + 1]].reshape(-1) for k in range(len(edges) - 1)]   # the per-part lists of a shuffled call
    assert torch.equal(every, torch.cat(parts))
    assert [0] + ends == [sum(p.numel() for p in parts[:k]) for k in range(len(parts) + 1)]
    # through the unshuffled lists: entry j of the joined list is the patch the shuffled tensor holds at that place
    plain = torch.cat(Selection.part_lists(B, N, edges, CPU)).long()
    assert torch.equal(every, flat.reshape(-1)[plain])


def test_header_declares_the_new_entries_under_the_same_version():
    text = open(HEADER).read()
    assert re.search(r"^#define IPSX_VERSION 306$", text, re.M)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("ipsx_trunk_encode_parts", "ipsx_part_wait", "ipsx_logits_if"):
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in hip._EXPORTS
        assert name in text[text.index("3.06"):text.index("#define IPSX_VERSION")], name    # listed in the history comment
    assert hip.lib().ipsx_version() == 306
