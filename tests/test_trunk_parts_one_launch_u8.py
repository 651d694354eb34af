"""uint8 patches and whole uint8 images on the fused trunk's ONE counted launch (``ipsx_trunk_encode_parts_u8``,
``ipsx_trunk_encode_parts_view_u8``): the embeddings are bit for bit those of the per-part launches on the same
bytes and of the float32 counted launch on ``table[c][bytes]``, every part is counted, refused arguments launch nothing, and
``IPSNet.ips`` / ``ips_image`` leave the same bits behind on the one-launch route as on the per-part launches and as the
float32 call - also when every wait gave up and the call was redone inside itself.  The shapes and the part cuts are those of
``tests/test_trunk_parts_one_launch.py``: workgroups of eight patches against part edges."""

import ctypes as C
import itertools

import pytest
import torch

from ips_amd import hip, quant, synth
from ips_amd.architecture import IPSNet
from ips_amd.selection import Selection
from test_trunk_parts_one_launch import CASES, PERMUTED, lists_of
from view_cases import grid
from view_u8_cases import TIERS, expected_tier, guard_table, guarded_images_u8, plain_table

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

_SHARED = {}


def trunk():
    """(plan, q, table, x): the MNIST net's encoder with seeded weights, 64 seeded uint8 patches, a random table with
    table[0][0] != 0 and the float32 patches the bytes stand for - made once."""
    if "trunk" not in _SHARED:
        net = synth.fill_weights(IPSNet(DEV, synth.mnist_conf(N=64, M=8, I=8)), 7).to(DEV).eval()
        q = torch.randint(0, 256, (64, 1, 32, 32), dtype=torch.uint8, generator=torch.Generator().manual_seed(11)).to(DEV)
        table = plain_table(1).to(DEV)
        assert float(table[0, 0]) != 0.0 and q.data_ptr() % 16 == 0 and table.data_ptr() % 16 == 0
        plan = hip.EncoderPlan(net.encoder, True)
        assert plan.fused(q.shape)                                        # (also tells the trunk its patch size)
        _SHARED["trunk"] = (plan, q, table, quant.dequant(q, table), net)
    return _SHARED["trunk"][:4]


def ends_of(ends):
    return (C.c_int64 * len(ends))(*ends), len(ends)


def raw_u8(plan, q, table, every, ends, done, emb):
    """``ipsx_trunk_encode_parts_u8`` itself, on a caller's buffers -> its return code."""
    assert plan.fused(q.shape)
    return hip.lib().ipsx_trunk_encode_parts_u8(C.byref(plan.trunk), hip._p(q), hip._p(table), hip._p(every),
                                                0 if every is None else every.numel(), hip._p(emb), *ends_of(ends), hip._p(done),
                                                hip._stream())


def raw_f32(plan, x, every, ends, done, emb):
    assert plan.fused(x.shape)
    return hip.lib().ipsx_trunk_encode_parts(C.byref(plan.trunk), hip._p(x), hip._p(every), every.numel(), hip._p(emb),
                                             *ends_of(ends), hip._p(done), hip._stream())


def raw_view_u8(plan, images, table, view, every, ends, done, emb):
    assert plan.fused(view.patch_shape)                                   # (tells the trunk its patch size)
    return hip.lib().ipsx_trunk_encode_parts_view_u8(C.byref(plan.trunk), hip._p(images), hip._p(table), C.byref(view.struct),
                                                     hip._p(every), 0 if every is None else every.numel(), hip._p(emb),
                                                     *ends_of(ends), hip._p(done), hip._stream())


def raw_view_f32(plan, images, view, every, ends, done, emb):
    assert plan.view_supported(view)
    return hip.lib().ipsx_trunk_encode_parts_view(C.byref(plan.trunk), hip._p(images), C.byref(view.struct), hip._p(every),
                                                  every.numel(), hip._p(emb), *ends_of(ends), hip._p(done), hip._stream())


def between_sentinels(n):
    return torch.full((n + 2, 128), float("nan"), device=DEV)


def sentinels_intact(buf):
    return bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[-1]).all())


# ---------------------------------------------------------------------------------------------------- the kernel, patches
@pytest.mark.parametrize("sizes,numbers", CASES, ids=[str(c[0]) + ("" if c[1] is None else " permuted") for c in CASES])
def test_one_launch_on_bytes_equals_the_per_part_launches_and_the_float32_launch(sizes, numbers):
    plan, q, table, x = trunk()
    lists = lists_of(sizes, numbers)
    every = torch.cat(lists)
    n = every.numel()
    ends = list(itertools.accumulate(sizes))
    want = torch.cat([plan.encode_indexed(q, l, table=table) for l in lists])
    done = torch.zeros((len(sizes),), dtype=torch.int32, device=DEV)
    f32 = between_sentinels(n)
    assert raw_f32(plan, x, every, ends, done, f32[1:n + 1]) == 0, hip.lib().ipsx_last_error()
    torch.cuda.synchronize()
    assert done.tolist() == list(sizes)
    done.zero_()
    buf = between_sentinels(n)
    assert raw_u8(plan, q, table, every, ends, done, buf[1:n + 1]) == 0, hip.lib().ipsx_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(want).all())
    assert torch.equal(buf[1:n + 1], want)
    assert torch.equal(buf[1:n + 1], f32[1:n + 1])
    assert sentinels_intact(buf) and sentinels_intact(f32)
    assert done.tolist() == list(sizes)
    # and through the plan's method, the way the selection calls it
    done.zero_()
    assert torch.equal(plan.encode_indexed(q, every, table=table, parts=(ends, done)), want)
    assert done.tolist() == list(sizes)


# ---------------------------------------------------------------------------------------------------- the kernel, whole images
IMAGES = (2, 1, 96, 112, (32, 32), (16, 16))                  # 5 x 6 = 30 grid patches per image
VIEW_CASES = [((17, 9, 7, 4), None),                          # in grid order, P = 4, n not a multiple of 8
              ((7, 13), PERMUTED % 60)]                       # permuted with repeats (7 and 40 twice), inside the grid of 60
TIER_AT = {0: 16, 1: 1, 4: 4}                                 # w = 112 and sw = 16 are whole 16-byte units: the address decides


@pytest.mark.parametrize("k", sorted(TIER_AT))
@pytest.mark.parametrize("sizes,numbers", VIEW_CASES, ids=["grid order", "permuted"])
def test_one_launch_on_uint8_images_equals_the_per_part_launches_and_the_float32_launch(sizes, numbers, k):
    plan = trunk()[0]
    assert grid(IMAGES) == (5, 6)
    table = guard_table(1).to(DEV)
    images = guarded_images_u8(IMAGES, k, device=DEV)
    assert images.data_ptr() % 16 == k and images.dtype == torch.uint8
    view = hip.PatchView(images.shape, IMAGES[4], IMAGES[5])
    assert view.count == 60 and plan.view_kernel_name(view, u8=True) == "fused_trunk_view_u8_kernel"
    # the launcher's choice of load width, asserted the way tests/test_patch_view_u8.py asserts it
    got = view.load_bytes(images, TIERS["fused"])
    assert got == expected_tier("fused", IMAGES, k) == TIER_AT[k]
    lists = lists_of(sizes, numbers)
    every = torch.cat(lists)
    assert int(every.max()) < view.count
    n = every.numel()
    ends = list(itertools.accumulate(sizes))
    want = torch.cat([plan.encode_view(images, view, index=l, table=table) for l in lists])
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) < 1e20       # no guard byte was read
    floats = quant.dequant(images, table)
    done = torch.zeros((len(sizes),), dtype=torch.int32, device=DEV)
    f32 = between_sentinels(n)
    assert raw_view_f32(plan, floats, view, every, ends, done, f32[1:n + 1]) == 0, hip.lib().ipsx_last_error()
    torch.cuda.synchronize()
    assert done.tolist() == list(sizes)
    done.zero_()
    buf = between_sentinels(n)
    assert raw_view_u8(plan, images, table, view, every, ends, done, buf[1:n + 1]) == 0, hip.lib().ipsx_last_error()
    torch.cuda.synchronize()
    assert torch.equal(buf[1:n + 1], want)
    assert torch.equal(buf[1:n + 1], f32[1:n + 1])
    assert sentinels_intact(buf) and done.tolist() == list(sizes)
    done.zero_()
    assert torch.equal(plan.encode_view(images, view, index=every, table=table, parts=(ends, done)), want)
    assert done.tolist() == list(sizes)


# ---------------------------------------------------------------------------------------------------- refusals
def test_rejected_arguments_launch_nothing():
    plan, q, table, x = trunk()
    every = torch.arange(24, dtype=torch.int32, device=DEV)
    buf = torch.full((24, 128), float("nan"), device=DEV)
    done = torch.zeros((17,), dtype=torch.int32, device=DEV)
    images = guarded_images_u8(IMAGES, 0, device=DEV)
    view = hip.PatchView(images.shape, IMAGES[4], IMAGES[5])
    off = torch.zeros((260,), dtype=torch.float32, device=DEV)
    off[1:257] = table[0]
    off = off[1:257].view(1, 256)                                          # the same table, 4 bytes off a 16-byte boundary
    assert off.data_ptr() % 16 == 4

    def untouched():
        torch.cuda.synchronize()
        return bool(torch.isnan(buf).all()) and not bool(done.any())

    def refused(ends, tab=table, index=every):
        a = raw_u8(plan, q, tab, index, ends, done, buf)
        b = raw_view_u8(plan, images, tab, view, index, ends, done, buf)
        return a != 0 and b != 0 and untouched()

    assert plan.fused(q.shape)
    plan.trunk.precision = 1                                              # bf16
    try:
        assert refused([8, 24])
    finally:
        plan.trunk.precision = 0
    assert refused([8, 24], tab=None)                                     # no table
    assert refused([8, 24], tab=off)                                      # a table that is not 16-byte aligned
    assert refused([8, 24], index=None)                                   # no index list
    assert refused(list(range(1, 17)) + [24])                             # P = 17
    assert refused([8, 8, 24]) and refused([16, 8, 24])                   # part_end does not increase
    assert refused([8, 16])                                               # does not end on the list's length
    # the plan's method says the same before it reaches the library
    with pytest.raises(TypeError):
        plan.encode_indexed(q, every, parts=([8, 24], done))              # uint8 without a table
    with pytest.raises(TypeError):
        plan.encode_source(hip.PatchSource(q, table), parts=([8, 24], done))      # no index list
    with pytest.raises(TypeError):
        plan.encode_source(hip.PatchSource(images=images, view=view, table=table), parts=([8, 24], done))
    assert untouched()
    assert raw_u8(plan, q, table, every, [8, 24], done, buf) == 0         # (the same buffers are fine otherwise)
    torch.cuda.synchronize()
    assert done[:2].tolist() == [8, 16] and not bool(torch.isnan(buf).any())
    done.zero_()
    buf.fill_(float("nan"))
    assert raw_view_u8(plan, images, table, view, every, [8, 24], done, buf) == 0
    torch.cuda.synchronize()
    assert done[:2].tolist() == [8, 16] and not bool(torch.isnan(buf).any())


# ---------------------------------------------------------------------------------------------------- selection end to end
NAMES = ("mem_patch", "mem_pos", "last_mem_idx", "last_mem_emb", "last_shuffle")
KINDS = {"patches": None, "images_s32": ((320, 640), (32, 32)), "images_s16": ((176, 336), (16, 16))}     # every one N = 200


def ips_net(shuffle):
    key = ("net", shuffle)
    if key not in _SHARED:
        conf = synth.mnist_conf(N=200, M=16, I=16, shuffle=shuffle, shuffle_style="instance")
        net = synth.fill_weights(IPSNet(DEV, conf), 7).to(DEV).eval()
        net.set_patch_table(plain_table(1))
        _SHARED[key] = net
    return _SHARED[key]


def bytes_of(kind, B=16):
    """(uint8 input, the call on it and on its float32 expansion) - the inputs are made once per kind."""
    key = ("input", kind)
    if key not in _SHARED:
        g = torch.Generator().manual_seed(12)
        shape = (16, 200, 1, 32, 32) if KINDS[kind] is None else (16, 1) + KINDS[kind][0]
        _SHARED[key] = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g).to(DEV)
    return _SHARED[key][:B].contiguous()


def run(net, kind, x):
    if KINDS[kind] is None:
        return net.ips(x)
    return net.ips_image(x, (32, 32), KINDS[kind][1])


def route(monkeypatch, on):
    """Both routes by their switches, set explicitly."""
    monkeypatch.setenv("IPSX_ONE_LAUNCH", "1" if on else "0")
    monkeypatch.setenv("IPSX_ONE_LAUNCH_U8", "1")


def call(net, kind, x, monkeypatch, on, seed=3):
    route(monkeypatch, on)
    torch.manual_seed(seed)
    out = run(net, kind, x)
    torch.cuda.synchronize()
    _SHARED["parts"] = [tuple(e.shape[:2]) for e in net._emb_parts]       # (reading last_mem_emb joins and drops them)
    return [None if t is None else t.clone() for t in tuple(out) + (net.last_mem_idx, net.last_mem_emb, net.last_shuffle)]


def same(got, want, what):
    for name, a, b in zip(NAMES, got, want):
        assert (a is None) == (b is None), (what, name)
        if a is not None:
            assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), (what, name)


def counting(net, monkeypatch):
    """-> (launches: the ``parts`` of every ``encode_source`` call, waits: every ``part_wait``'s count)."""
    launches, waits = [], []
    plan = net.selection.plan()
    inner, inner_wait = plan.encode_source, hip.part_wait
    monkeypatch.setattr(plan, "encode_source", lambda *a, **kw: (launches.append(kw.get("parts")), inner(*a, **kw))[1], raising=False)
    monkeypatch.setattr(hip, "part_wait", lambda *a, **kw: (waits.append(a[1]), inner_wait(*a, **kw))[1])
    return launches, waits


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("shuffle", [False, True], ids=["in order", "instance shuffle"])
@pytest.mark.parametrize("B", [2, 16])
def test_ips_leaves_the_same_bits_on_both_routes(B, shuffle, kind, monkeypatch):
    """N = 200, M = I = 16: 12 iterations in 4 parts (rows 112 | 64 | 16 | 8 of every image).  These batches are far below
    the small-batch limit, which is lifted here so that they take the parts' route."""
    monkeypatch.setattr(Selection, "small_batch_limit", lambda self, dev: 0)
    net = ips_net(shuffle)
    x = bytes_of(kind, B)
    floats = quant.dequant(x, net.patch_table)
    want_f32 = call(net, kind, floats, monkeypatch, True)
    launches, waits = counting(net, monkeypatch)
    off = call(net, kind, x, monkeypatch, False)
    assert len(launches) == 4 and not any(launches) and waits == []
    del launches[:]
    on = call(net, kind, x, monkeypatch, True)
    assert len(launches) == 1 and launches[0] is not None and len(launches[0][0]) == 4
    assert waits == [B * 112, B * 64, B * 16]
    again = call(net, kind, x, monkeypatch, True)                         # (cached buffers, counters zeroed again)
    assert len(launches) == 2 and len(waits) == 6
    assert on[0].dtype == torch.float32 and (on[4] is not None) == shuffle
    same(on, off, "route on against route off")
    same(on, want_f32, "against the float32 call")
    same(again, on, "second call on the cached buffers")
    assert _SHARED["parts"] == [(B, 112), (B, 64), (B, 16), (B, 8)]


def test_default_route_for_bytes_is_one_trunk_launch_per_part(monkeypatch):
    """What ships (the measurement missed its rule on the patch shape): with no switch set, float32 takes the
    counted launch and bytes keep one launch per part; IPSX_ONE_LAUNCH_U8=1 puts bytes on the route, and IPSX_ONE_LAUNCH=0
    takes both off it."""
    monkeypatch.setattr(Selection, "small_batch_limit", lambda self, dev: 0)
    monkeypatch.delenv("IPSX_ONE_LAUNCH", raising=False)
    monkeypatch.delenv("IPSX_ONE_LAUNCH_U8", raising=False)
    net = ips_net(False)
    assert hip.persistent_ok(DEV)
    launches, waits = counting(net, monkeypatch)

    def counted(kind, x):
        del launches[:], waits[:]
        run(net, kind, x)
        return len(launches), sum(p is not None for p in launches), len(waits)

    for kind in KINDS:
        x = bytes_of(kind)
        assert counted(kind, quant.dequant(x, net.patch_table)) == (1, 1, 3), kind
        assert counted(kind, x) == (4, 0, 0), kind
        monkeypatch.setenv("IPSX_ONE_LAUNCH_U8", "1")
        assert counted(kind, x) == (1, 1, 3), kind
        monkeypatch.setenv("IPSX_ONE_LAUNCH", "0")
        assert counted(kind, x) == (4, 0, 0), kind
        monkeypatch.delenv("IPSX_ONE_LAUNCH")
        monkeypatch.delenv("IPSX_ONE_LAUNCH_U8")
    torch.cuda.synchronize()


def test_a_call_on_bytes_whose_waits_gave_up_is_redone_in_the_call(monkeypatch):
    """``Selection.parts_one_launch`` on uint8 patches with every wait giving up at once (``hip.part_wait`` replaced by a
    launch that only sets the status bit - nothing waits, nothing hangs): the conditional launches at the end of the call
    must leave the per-part route's bits.  The host sees the word one call later and counts the event once."""
    monkeypatch.setattr(Selection, "small_batch_limit", lambda self, dev: 0)
    net, x = ips_net(False), bytes_of("patches")
    want = call(net, "patches", x, monkeypatch, False)
    good = call(net, "patches", x, monkeypatch, True)                     # (buffers of the route exist; mirror clean)
    events, forced = [], []

    def gave_up(done, want_count, status, bit=1):
        forced.append(want_count)
        status.bitwise_or_(bit)                                           # (on the side stream, where the wait would run)

    monkeypatch.setattr(hip, "part_wait", gave_up)
    monkeypatch.setattr(hip, "persistent_timed_out", lambda dev: events.append(dev) or True)
    calls = hip._PERSIST_CALLS
    got = call(net, "patches", x, monkeypatch, True)
    assert forced == [16 * 112, 16 * 64, 16 * 16] and events == []
    same(got, want, "redone call against the per-part route")
    same(good, want, "undisturbed call against the per-part route")
    assert int(net.selection.scan_status_host.item()) & 1                 # mirrored behind the call
    monkeypatch.undo()                                                    # (the real wait kernel again)
    monkeypatch.setattr(Selection, "small_batch_limit", lambda self, dev: 0)
    monkeypatch.setattr(hip, "persistent_timed_out", lambda dev: events.append(dev) or True)
    again = call(net, "patches", x, monkeypatch, True)
    assert len(events) == 1 and hip._PERSIST_CALLS == calls + 2
    assert int(net.selection.scan_status_host.item()) == 0
    same(again, want, "the call after")


# ---------------------------------------------------------------------------------------------------- memory
def test_bytes_on_the_route_allocate_no_more_than_float32_images(monkeypatch):
    """16 images of 176x336 at stride 16 on a warmed net, the route on: the uint8 call's peak above its input does not
    exceed the float32 call's peak above ITS (four times larger) input - both take the same schedule, and the bytes' only
    extra is the table, which is resident before the call."""
    monkeypatch.setattr(Selection, "small_batch_limit", lambda self, dev: 0)
    route(monkeypatch, True)
    net = ips_net(False)
    bytes_ = bytes_of("images_s16")
    floats = quant.dequant(bytes_, net.patch_table)
    launches, _ = counting(net, monkeypatch)
    peaks = {}
    for name, images in (("uint8", bytes_), ("float32", floats)):
        net.ips_image(images, (32, 32), (16, 16))               # warmed: weights packed, the route's buffers exist
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(DEV)
        base = torch.cuda.max_memory_allocated(DEV)
        out = net.ips_image(images, (32, 32), (16, 16))
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated(DEV) - base
        assert out[0].shape == (16, 16, 1, 32, 32) and out[0].dtype == torch.float32
        del out
    assert len(launches) == 4 and all(p is not None for p in launches)   # the same schedule: one counted launch per call
    print("peak above the input: uint8 %d B, float32 %d B (input %d / %d B)" % (peaks["uint8"], peaks["float32"], bytes_.numel(),
                                                                               4 * floats.numel()))
    assert peaks["uint8"] <= peaks["float32"]
