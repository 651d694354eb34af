"""Where the patches of a launch lie - float32 patches, uint8 patches with their table, whole images through a patch-grid
view - times how they are addressed: from patch 0, from an offset (a slice of the tensor, ``first = 3`` of the view) and
through a permuted int32 index list.  The host code cuts a call into launches in three places, each by "the same source,
k patches further on": the fused trunk's whole rounds + pair-kernel remainder, the layered trunks' chunk loop, and the
two halves a layered call of 1,024 patches or more runs on two streams.  Every storage kind crosses every cut here, at the
smallest sizes where the rule can go wrong.

Yardstick: ``plan.encode`` on the expanded float32 patch tensor, ONE call per data set in one chunk, compared with
``torch.equal`` (same kernels behind the stem's load: no tolerance).  Written against ``plan.encode`` / ``encode_indexed`` /
``encode_view`` only.  Patch tensors go through an index list on the fused trunk alone (``ipsx_trunk_encode_indexed``), so
the layered trunks' indexed cases are those of the view."""

import ctypes as C

import pytest
import torch

from ips_amd import hip, quant, synth
from ips_amd.architecture import IPSNet
from view_cases import FUSED_ROUND, POOL50, POOL50_CUT, POOL100, guarded_images

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
_NETS, _DATA = {}, {}


def net_for(kind):
    if kind not in _NETS:
        conf = {"mnist": lambda: synth.mnist_conf(N=64, M=8, I=8), "mnist50": lambda: synth.mnist_conf(N=64, M=8, I=8, patch=50),
                "traffic": lambda: synth.traffic_conf(N=48, M=8, I=16)}[kind]()
        _NETS[kind] = synth.fill_weights(IPSNet(DEV, conf), 5).to(DEV).eval()
    return _NETS[kind]


def data(kind, geom=None, shape=None, count=None):
    """One data set per (net, geometry | patch shape), made and encoded ONCE: images + view + their float32 patches ``x``, or
    random float32 patches; uint8 patches ``q`` with a table; ``want_x`` / ``want_q``: the yardstick's rows."""
    key = (kind, geom, shape, count)
    if key not in _DATA:
        plan = net_for(kind).selection.plan()
        d = {"plan": plan}
        if geom is not None:
            b, c, h, w, patch, stride = geom
            d["images"] = guarded_images(geom, 0, device=DEV)
            d["view"] = hip.PatchView(d["images"].shape, patch, stride)
            x = hip.patchify(d["images"], patch, stride)
            d["x"] = x.reshape(-1, *x.shape[2:])
            count, shape = d["view"].count, d["view"].patch_shape
        else:
            d["x"] = torch.randn((count,) + shape, generator=torch.Generator().manual_seed(3)).to(DEV)
        g = torch.Generator().manual_seed(17)
        d["table"] = torch.randn((shape[0], 256), generator=g).to(DEV)
        q = torch.randint(0, 256, (count,) + shape, dtype=torch.uint8, generator=g)
        q[1::2] = 0                                                    # every second patch all-zero bytes: tied rows
        d["q"] = q.to(DEV)
        d["want_x"] = plan.encode(d["x"])
        d["want_q"] = plan.encode(quant.dequant(d["q"], d["table"]))
        d["perm"] = torch.randperm(count, generator=g).to(torch.int32).to(DEV)
        torch.cuda.synchronize()
        _DATA[key] = d
    return _DATA[key]


def check_tensor_kinds(d, n, off=3, indexed=False):
    """float32 and uint8 patches: n from patch 0, n from patch ``off`` (a slice), and - the fused trunk - n through the index."""
    plan, x, q, table = d["plan"], d["x"], d["q"], d["table"]
    for lo in (0, off):
        assert torch.equal(plan.encode(x[lo:lo + n]), d["want_x"][lo:lo + n]), ("float32", lo, n)
        assert torch.equal(plan.encode(q[lo:lo + n], table=table), d["want_q"][lo:lo + n]), ("uint8", lo, n)
    if indexed:
        ix = d["perm"][:n]
        assert torch.equal(plan.encode_indexed(x, ix), d["want_x"][ix.long()]), ("float32 index", n)
        assert torch.equal(plan.encode_indexed(q, ix, table=table), d["want_q"][ix.long()]), ("uint8 index", n)


def check_view(d, n, off=3):
    plan, images, view = d["plan"], d["images"], d["view"]
    for lo in (0, off):
        assert torch.equal(plan.encode_view(images, view, first=lo, n=n), d["want_x"][lo:lo + n]), ("view", lo, n)
    ix = d["perm"][:n]
    assert torch.equal(plan.encode_view(images, view, index=ix), d["want_x"][ix.long()]), ("view index", n)


# ---------------------------------------------------------------------------------------------- fused 1x32x32 trunk
@pytest.mark.parametrize("n", [13, "round+5"])
def test_fused_trunk_whole_rounds_and_pair_remainder(n):
    """13: everything goes to the pair kernel, with an odd tail.  8 * cus + 5: one whole round, then a remainder that starts
    at a non-zero patch and ends on an odd count."""
    n = 8 * hip.device_geometry(DEV).cus + 5 if n == "round+5" else n
    d = data("mnist", geom=FUSED_ROUND)
    assert n + 3 <= d["view"].count == 2116
    check_tensor_kinds(d, n, indexed=True)
    check_view(d, n)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- layered trunks: the chunk loop
def few_patch_budget(d, monkeypatch):
    """IPSX_TRUNK_WORKSPACE_MB (read per call) for a workspace of 2 .. 4 patches: 7 patches then take 2 .. 4 chunks."""
    per = hip.lib().ipsx_trunk_workspace_bytes(C.byref(d["plan"].trunk), 1)       # (the yardstick's call described the patches)
    assert per > 0
    mb = -(-3 * per // (1 << 20))
    assert 2 <= (mb << 20) // per <= 4, (per, mb)
    monkeypatch.setenv("IPSX_TRUNK_WORKSPACE_MB", str(mb))
    assert 2 * per <= hip.lib().ipsx_trunk_workspace_bytes(C.byref(d["plan"].trunk), 7) <= 4 * per


@pytest.mark.parametrize("kind,geom", [("mnist50", POOL50[0]), ("traffic", POOL100[0])], ids=["pool50", "pool100x3"])
def test_layered_trunk_in_several_chunks(kind, geom, monkeypatch):
    d = data(kind, geom=geom)                                          # (12 grid patches each)
    d["plan"].encode(d["x"][:1])
    few_patch_budget(d, monkeypatch)
    check_tensor_kinds(d, 7)
    check_view(d, 7)
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind,shape", [("traffic", (3, 37, 45)), ("mnist", (1, 41, 29))], ids=["3x37x45", "1x41x29"])
def test_generic_stem_in_several_chunks(kind, shape, monkeypatch):
    """Patch shapes no fused stem covers: conv_any_kernel reads floats or gathers bytes, rows at any address."""
    d = data(kind, shape=shape, count=10)
    d["plan"].encode(d["x"][:1])
    few_patch_budget(d, monkeypatch)
    check_tensor_kinds(d, 7)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- layered trunks: the two-stream cut
def test_two_stream_cut_of_bytes_and_of_an_indexed_view():
    """1,027 patches of 50 px: the call is cut at 513 and its halves run on two streams.  Bytes from patch 3 on; the view
    from grid patch 3 on and through an index list, whose second half is the list from entry 513 on."""
    d = data("mnist50", geom=POOL50_CUT)
    n = 1027
    assert d["view"].count == 1056
    assert torch.equal(d["plan"].encode(d["q"][3:3 + n], table=d["table"]), d["want_q"][3:3 + n])
    assert torch.equal(d["plan"].encode(d["x"][3:3 + n]), d["want_x"][3:3 + n])
    check_view(d, n)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- no call depends on an earlier one
def test_first_call_of_a_fresh_plan_and_first_call_after_a_rebuild():
    """``encode_indexed`` / ``encode_view`` as the FIRST call of a fresh EncoderPlan - no ``fused()``, ``view_supported()`` or
    ``encode()`` before it - and again right after ``hip.weights_changed()`` has made the plan rebuild its trunk description:
    every encode call describes its own patches.  (Before ``encode_source`` existed ``encode_indexed`` read the patch shape
    an earlier ``fused()`` / ``encode()`` had left in the shared trunk struct: as a first call it failed with "only the fused
    1x32x32 trunk is supported" - the struct still said 0 x 0.)"""
    d = data("mnist", geom=FUSED_ROUND)
    net, ix = net_for("mnist"), d["perm"][:13]
    want = d["want_x"][ix.long()]
    assert torch.equal(hip.EncoderPlan(net.encoder, True).encode_indexed(d["x"], ix), want)
    assert torch.equal(hip.EncoderPlan(net.encoder, True).encode_view(d["images"], d["view"], index=ix), want)
    plan = hip.EncoderPlan(net.encoder, True)
    assert torch.equal(plan.encode_view(d["images"], d["view"], first=3, n=13), d["want_x"][3:16])
    hip.weights_changed()
    assert torch.equal(plan.encode_indexed(d["x"], ix), want)
    hip.weights_changed()
    assert torch.equal(plan.encode_view(d["images"], d["view"], index=ix), want)
    torch.cuda.synchronize()
