"""``IPSNet.ips`` on the counted, deduped route with the trailing parts in ONE gated last launch (``Selection.parts_loop_logits``,
``IPSX_SCAN_TAIL``) against the chain it replaces (``IPSX_SCAN_TAIL=0``): everything the call returns and leaves behind,
bit for bit, on the first call and on the cached buffers.

2 images x (64 + 64 * 6 + 9) patches, content in a few of them.  The route's small-batch limit is lifted and - 457 patches are 7
iterations - its parts are set to 3, so that a batch of this size takes it, cut into parts of 192, 192 and 73 rows;
``IPSX_SCAN_TAIL=1`` asks for the tail at every size."""

import pytest
import torch

from ips_amd import hip, synth
from ips_amd.architecture import IPSNet
from ips_amd.selection import Selection

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M = I = 64
N = 64 + 64 * 6 + 9
_SHARED = {}


def setup():
    if not _SHARED:
        conf = synth.mnist_conf(N=N, M=M, I=I)
        net = synth.fill_weights(IPSNet(torch.device(DEV), conf), 3).to(DEV).eval()
        x = torch.zeros((2, N, conf.n_chan_in) + tuple(conf.patch_size))
        g = torch.Generator().manual_seed(9)
        for b, n in ((0, 3), (0, 70), (0, 200), (0, 456), (1, 0), (1, 64), (1, 300), (1, 448), (1, 455)):
            x[b, n] = torch.rand(tuple(x.shape[2:]), generator=g)
        _SHARED["net"], _SHARED["x"] = net, x.to(DEV)
    return _SHARED["net"], _SHARED["x"]


def ips(net, x, monkeypatch, tail, rows=None):
    """two calls under the given switches -> (what they returned and left, the gated launches as (part_begin, part_end))"""
    monkeypatch.setenv("IPSX_SCAN_TAIL", tail)
    if rows is None:
        monkeypatch.delenv("IPSX_SCAN_TAIL_ROWS", raising=False)
    else:
        monkeypatch.setenv("IPSX_SCAN_TAIL_ROWS", rows)
    gated, calls = [], [0]
    inner = hip.LogitsParts.scan_range

    def spy(*a, **kw):
        calls[0] += 1
        if kw.get("gate") is not None:
            gated.append((a[10], a[11]))
        return inner(*a, **kw)
    monkeypatch.setattr(hip.LogitsParts, "scan_range", spy)
    out = []
    for _ in range(2):
        mem_patch, mem_pos = net.ips(x)
        out.append((mem_patch.clone(), mem_pos.clone(), net.last_mem_idx.clone(), net.last_mem_emb.clone()))
    torch.cuda.synchronize()
    monkeypatch.setattr(hip.LogitsParts, "scan_range", inner)
    assert calls[0] > 0, "the counted route with the loop's own logits was meant to run"
    assert int(net.selection.scan_status_host.item()) == 0
    return out, gated


def lift(monkeypatch):
    monkeypatch.setattr(Selection, "small_batch_limit", lambda self, dev: 0)
    monkeypatch.setattr(Selection, "OVERLAP_PARTS", 3)
    assert hip.persistent_ok(DEV)


def chain(monkeypatch):
    if "chain" not in _SHARED:
        net, x = setup()
        _SHARED["chain"], gated = ips(net, x, monkeypatch, "0")
        assert gated == []
    return _SHARED["chain"]


def equal(got, want):
    for call, (g, w) in enumerate(zip(got, want)):
        for name, a, b in zip(("mem_patch", "mem_pos", "last_mem_idx", "last_mem_emb"), g, w):
            assert torch.equal(a, b), "%s, call %d" % (name, call)


def test_the_gated_tail_leaves_what_the_chain_leaves(monkeypatch):
    lift(monkeypatch)
    want = chain(monkeypatch)
    net, x = setup()
    got, gated = ips(net, x, monkeypatch, "1")
    # the last two parts, 192 + 73 rows, fit the default limit
    assert gated == [(1, 3), (1, 3)], gated
    equal(got, want)
    assert not torch.equal(want[0][2], torch.arange(M, device=DEV).expand(2, M)), "the loop was meant to select something"


def test_a_limit_no_part_fits_is_the_chain(monkeypatch):
    lift(monkeypatch)
    want = chain(monkeypatch)
    net, x = setup()
    got, gated = ips(net, x, monkeypatch, "1", rows="1")
    assert gated == []
    equal(got, want)
