"""Exact blank-patch dedup wherever ``Selection.parts_one_launch`` runs: float32 images through ``ips_image``,
uint8 images and uint8 patches under ``IPSX_ONE_LAUNCH_U8=1``.  With ``IPSX_DEDUP_BLANK`` unset every output of the call is
bit for bit that of the same call under ``IPSX_DEDUP_BLANK=0``, ``plan.n_encoded`` is the host's count of non-blank patches
(all elements zero for floats, every byte 0 for bytes), one counted launch is made, and the blank embedding follows the
weights and - for bytes - the patch table.  N = 200, M = I = 16 as in ``tests/test_trunk_parts_one_launch_u8.py``: far below
the small-batch limit, which is lifted here."""

import numpy as np
import pytest
import torch

from ips_amd import hip, quant, synth
from ips_amd.architecture import IPSNet
from ips_amd.selection import Selection

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

_SHARED = {}
NAMES = ("mem_patch", "mem_pos", "last_mem_idx", "last_mem_emb", "last_shuffle")
# kind -> (storage, image size and stride | None: patches); every one N = 200
KINDS = {"f32 images s32": ("f32", (320, 640), (32, 32)), "f32 images s16": ("f32", (176, 336), (16, 16)),
         "u8 images s32": ("u8", (320, 640), (32, 32)), "u8 images s16": ("u8", (176, 336), (16, 16)),
         "u8 patches": ("u8", None, None)}


def tables():
    """ToTensor's table (table[0][0] == 0.0f: the float32 expansion of a blank byte patch is blank too) and a normalising one."""
    if "tables" not in _SHARED:
        _SHARED["tables"] = (quant.patch_table(1), quant.patch_table(1, mean=[0.1307], std=[0.3081]))
        assert float(_SHARED["tables"][0][0, 0]) == 0.0 and float(_SHARED["tables"][1][0, 0]) != 0.0
    return _SHARED["tables"]


def ips_net(shuffle):
    if ("net", shuffle) not in _SHARED:
        conf = synth.mnist_conf(N=200, M=16, I=16, shuffle=shuffle, shuffle_style="instance")
        _SHARED[("net", shuffle)] = synth.fill_weights(IPSNet(DEV, conf), 7).to(DEV).eval()
    net = _SHARED[("net", shuffle)]
    net.set_patch_table(tables()[0])
    return net


def bytes_of(size, stride, content):
    """(16, 1, H, W) uint8 on the host and its (16, 200, 1, 32, 32) patches.  "blobs": zero but for seeded rectangles, few
    enough that at least half the patches are blank; "dense": no zero byte at all."""
    key = ("bytes", size, content)
    if key not in _SHARED:
        rng = np.random.default_rng(size[0] + (content == "dense"))
        if content == "dense":
            img = rng.integers(1, 256, (16, 1) + size, dtype=np.uint8)
        else:
            img = np.zeros((16, 1) + size, dtype=np.uint8)
            for b in range(16):
                for _ in range(5):
                    y0, x0 = rng.integers(0, size[0] - 30), rng.integers(0, size[1] - 30)
                    img[b, 0, y0:y0 + 30, x0:x0 + 30] = rng.integers(1, 256, (30, 30), dtype=np.uint8)
        img = torch.from_numpy(img)
        patches = img.unfold(2, 32, stride[0]).unfold(3, 32, stride[1]).permute(0, 2, 3, 1, 4, 5).reshape(16, 200, 1, 32, 32)
        _SHARED[key] = (img, patches.contiguous())
    return _SHARED[key]


def case(kind, B, content="blobs"):
    """-> (the call's input on the device, the host's count of non-blank patches among its B * 200)."""
    storage, size, stride = KINDS[kind]
    img, patches = bytes_of(size or (320, 640), stride or (32, 32), content)
    x = (patches if size is None else img)[:B].contiguous()
    blank = (patches[:B].reshape(B * 200, -1) == 0).all(1)                # (ToTensor's table: byte 0 <-> 0.0f, nothing else)
    if content == "blobs":
        assert int(blank.sum()) * 2 >= B * 200                            # at least half the patches are blank
    else:
        assert not bool(blank.any())
    x = x.to(DEV)
    if storage == "f32":
        x = quant.dequant(x, tables()[0].to(DEV))
        u = x.cpu().unfold(2, 32, stride[0]).unfold(3, 32, stride[1]).reshape(B * 200, -1)
        assert torch.equal((u == 0).all(1), blank)
    return x, B * 200 - int(blank.sum())


def run(net, kind, x):
    if KINDS[kind][1] is None:
        return net.ips(x)
    return net.ips_image(x, (32, 32), KINDS[kind][2])


def call(net, kind, x, monkeypatch, dedup, seed=3):
    monkeypatch.setenv("IPSX_ONE_LAUNCH", "1")
    monkeypatch.setenv("IPSX_ONE_LAUNCH_U8", "1")
    if dedup is None:
        monkeypatch.delenv("IPSX_DEDUP_BLANK", raising=False)
    else:
        monkeypatch.setenv("IPSX_DEDUP_BLANK", dedup)
    net.selection.plan().n_encoded = None
    torch.manual_seed(seed)
    out = run(net, kind, x)
    torch.cuda.synchronize()
    return [None if t is None else t.clone() for t in tuple(out) + (net.last_mem_idx, net.last_mem_emb, net.last_shuffle)]


def same(got, want, what):
    for name, a, b in zip(NAMES, got, want):
        assert (a is None) == (b is None), (what, name)
        if a is not None:
            assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), (what, name)


def counting(net, monkeypatch):
    """-> the ``parts`` of every ``encode_source`` call from here on."""
    launches = []
    plan = net.selection.plan()
    inner = plan.encode_source
    monkeypatch.setattr(plan, "encode_source", lambda *a, **kw: (launches.append(kw.get("parts")), inner(*a, **kw))[1], raising=False)
    return launches


def n_encoded(net):
    return int(net.selection.plan().n_encoded.item())


def compare(net, kind, x, nonblank, monkeypatch, f32=None):
    """The call under ``=0``, then twice with the switch unset; bytes also against the float32 call ``f32`` = (kind, input)."""
    want = call(net, kind, x, monkeypatch, "0")
    assert net.selection.plan().n_encoded is None                        # no dedup anywhere
    launches = counting(net, monkeypatch)
    got = call(net, kind, x, monkeypatch, None)
    assert n_encoded(net) == nonblank                                    # the scan ran, and the trunk encoded these only
    assert len(launches) == 1 and launches[0] is not None                # exactly one encode_source call, with parts
    again = call(net, kind, x, monkeypatch, None)                        # (cached buffers, counters zeroed again)
    assert n_encoded(net) == nonblank and len(launches) == 2
    same(got, want, "switch unset against =0")
    same(again, want, "second call on the cached buffers")
    if f32 is not None:
        same(got, call(net, f32[0], f32[1], monkeypatch, None), "bytes against the float32 call")
    return got


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("shuffle", [False, True], ids=["in order", "instance shuffle"])
@pytest.mark.parametrize("B", [2, 16])
def test_ips_leaves_the_same_bits_as_without_dedup(B, shuffle, kind, monkeypatch):
    monkeypatch.setattr(Selection, "small_batch_limit", lambda self, dev: 0)
    net = ips_net(shuffle)
    x, nonblank = case(kind, B)
    f32 = None
    if x.dtype == torch.uint8:                                           # the same bytes expanded, through the same entry point
        f32 = (kind, quant.dequant(x, net.patch_table))
    got = compare(net, kind, x, nonblank, monkeypatch, f32)
    assert got[0].dtype == torch.float32 and (got[4] is not None) == shuffle


@pytest.mark.parametrize("kind", list(KINDS))
def test_content_without_a_blank_patch(kind, monkeypatch):
    monkeypatch.setattr(Selection, "small_batch_limit", lambda self, dev: 0)
    net = ips_net(False)
    x, nonblank = case(kind, 16, "dense")
    assert nonblank == 16 * 200
    compare(net, kind, x, nonblank, monkeypatch)


@pytest.mark.parametrize("kind", ["f32 images s16", "u8 images s32", "u8 patches"])
def test_a_weight_change_renews_the_blank_embedding(kind, monkeypatch):
    monkeypatch.setattr(Selection, "small_batch_limit", lambda self, dev: 0)
    net = ips_net(False)
    x, nonblank = case(kind, 16)
    first = call(net, kind, x, monkeypatch, None)
    p = net.selection.plan()
    before = p.blank_emb.clone()
    bn = next(m for m in net.encoder.modules() if isinstance(m, torch.nn.BatchNorm2d))
    kept = bn.bias.detach().clone()
    try:
        with torch.no_grad():
            bn.bias.add_(0.25)                                           # (in place: the version counter moves)
        want = call(net, kind, x, monkeypatch, "0")
        got = call(net, kind, x, monkeypatch, None)
        same(got, want, "after the weight change")
        assert n_encoded(net) == nonblank
        assert not torch.equal(p.blank_emb, before)
        assert not torch.equal(got[3], first[3])                         # (the change is one the selection's output shows)
    finally:
        with torch.no_grad():
            bn.bias.copy_(kept)
    same(call(net, kind, x, monkeypatch, None), first, "the weights put back")


@pytest.mark.parametrize("kind", ["u8 images s16", "u8 patches"])
def test_another_patch_table_renews_the_blank_embedding(kind, monkeypatch):
    """A normalising table: byte 0 stands for a non-zero float, the blank patches stay blank (every byte 0) and their row is
    the embedding of a patch of table[0][0]."""
    monkeypatch.setattr(Selection, "small_batch_limit", lambda self, dev: 0)
    net = ips_net(False)
    x, nonblank = case(kind, 16)
    first = call(net, kind, x, monkeypatch, None)
    p = net.selection.plan()
    before = p.blank_emb.clone()
    try:
        net.set_patch_table(tables()[1])
        want = call(net, kind, x, monkeypatch, "0")
        got = call(net, kind, x, monkeypatch, None)
        same(got, want, "under the normalising table")
        assert n_encoded(net) == nonblank
        assert not torch.equal(p.blank_emb, before)
        assert not torch.equal(got[3], first[3])
        same(got, call(net, kind, quant.dequant(x, net.patch_table), monkeypatch, None), "bytes against the float32 call")
        assert n_encoded(net) == 16 * 200                                # (as floats, no patch of that call is blank)
    finally:
        net.set_patch_table(tables()[0])
    same(call(net, kind, x, monkeypatch, None), first, "the first table put back")
    assert torch.equal(p.blank_emb, before)


def test_the_explicit_switch_keeps_its_refusals(monkeypatch):
    """``IPSX_DEDUP_BLANK=1``: bytes are refused, and ``ips_image`` makes the patch tensor and hands it to ``ips()``."""
    monkeypatch.setattr(Selection, "small_batch_limit", lambda self, dev: 0)
    net = ips_net(False)
    for kind in ("u8 patches", "u8 images s32"):
        x, _ = case(kind, 2)
        monkeypatch.setenv("IPSX_DEDUP_BLANK", "1")
        with pytest.raises(TypeError):
            run(net, kind, x)
    x, _ = case("f32 images s16", 2)
    want = call(net, "f32 images s16", x, monkeypatch, "0")
    made = []
    inner = net._materialise
    monkeypatch.setattr(net, "_materialise", lambda *a, **kw: (made.append(1), inner(*a, **kw))[1], raising=False)
    same(call(net, "f32 images s16", x, monkeypatch, "1"), want, "the explicit route")
    assert made == [1]
    assert call(net, "f32 images s16", x, monkeypatch, None) and made == [1]       # (unset: the view, nothing materialised)
