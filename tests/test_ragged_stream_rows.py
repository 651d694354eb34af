"""The ragged ROW stream on the GPU (``IPSNet.ips_ragged_stream(patch_size=, patch_stride=)``): ``feed_rows`` over
bands that end anywhere, image by image, against ``ips_image_ragged`` on the joined bands with ``shuffle`` off - the stream's
state checked after every feed -, ``pad``, uint8 and host bands, overwritten buffers, the blank-patch dedup, the fallbacks,
memory, ``feed_rows_all`` and the refusals.

The fused images at stride (32, 32) give 55 / 18 / 15 patches and M = 16: ``ips_image_ragged`` refuses the third without
``pad``, so that case runs padded - the oracle must exist."""

import gc

import pytest
import torch

from ips_amd import hip, synth
from ips_amd.architecture import IPSNet
from ips_amd.ragged import Ragged
from ips_amd.ragged_image import RaggedImages
from tests import ragged_stream_rows_cases as rr
from view_cases import unfold
from view_u8_cases import plain_table

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
_NETS = {}


def net_for(kind, **over):
    key = (kind, tuple(sorted(over.items())))
    if key not in _NETS:
        conf = {"mnist": lambda: synth.mnist_conf(**over),
                "mnist50": lambda: synth.mnist_conf(patch=50, **over),
                "traffic": lambda: synth.traffic_conf(**over),
                "generic": lambda: synth.traffic_conf(patch=37, **over).clone(patch_size=[37, 45], patch_stride=[37, 45])}[kind]()
        net = synth.fill_weights(IPSNet(DEV, conf), 5).to(DEV).eval()
        net.shuffle = False
        _NETS[key] = net
    return _NETS[key]


FUSED = [(1, 352, 160), (1, 200, 96), (1, 120, 161)]                  # 189 / 55 / 54 patches at stride 16
ALL = ["ones", "stride", "straddle", "irregular", "whole"]
REST = ALL[1:]
# name: (net, image shapes, patch, stride, pad, patterns)
E2E = {
    "fused32_s16_pos": (lambda: net_for("mnist", N=300, M=16, I=16), FUSED, (32, 32), (16, 16), False, ALL),
    "fused32_s16": (lambda: net_for("mnist", N=300, M=16, I=16, use_pos=False), FUSED, (32, 32), (16, 16), False, ALL),
    "fused32_s32_pos": (lambda: net_for("mnist", N=300, M=16, I=16), FUSED, (32, 32), (32, 32), True, ALL),
    "fused32_s32": (lambda: net_for("mnist", N=300, M=16, I=16, use_pos=False), FUSED, (32, 32), (32, 32), True, ALL),
    "fused32_s16_pad": (lambda: net_for("mnist", N=300, M=16, I=16), FUSED + [(1, 40, 160)], (32, 32), (16, 16), True, REST),
    "pool50": (lambda: net_for("mnist50", N=64, M=8, I=8), [(1, 400, 200), (1, 250, 150)], (50, 50), (50, 50), False, REST),
    "pool100x3": (lambda: net_for("traffic", N=12, M=4, I=4), [(3, 400, 300), (3, 300, 200)], (100, 100), (100, 100), False, REST),
}
_E2E = {}


def image_logits(net, image, patch, stride):
    """(1, N, R) logits of every patch of one image (uint8: through the table), by the kernels ips() runs on the patch tensor"""
    x = unfold(image[None], patch, stride)[0]
    ca = net.transf.crs_attn
    emb = net._embed(x).unsqueeze(0)
    return hip.logits(emb, net.pos_enc[:, :x.shape[0]] if net.use_pos else None, ca.folded_query(), ca.H * ca.n_token)


def e2e_case(name, u8=False):
    """net, images, what ips_image_ragged returns and leaves behind, every image's full logits - computed once, shared,
    never changed"""
    if (name, u8) not in _E2E:
        make, shapes, patch, stride, pad, _ = E2E[name]
        net = make()
        gen = torch.Generator().manual_seed(sum(s[1] for s in shapes))
        if u8:
            net.set_patch_table(plain_table(shapes[0][0]))
            images = [torch.randint(0, 256, s, dtype=torch.uint8, generator=gen).to(DEV) for s in shapes]
        else:
            net.set_patch_table(None)
            images = [torch.randn(s, generator=gen).to(DEV) for s in shapes]
        want = rr.keep(rr.record(net, net.ips_image_ragged(images, patch, stride, pad=pad)))
        assert want[2] is not None and want[3] is not None
        lgs = [image_logits(net, im, patch, stride) for im in images]
        _E2E[(name, u8)] = (net, images, want, lgs)
    net, images, want, lgs = _E2E[(name, u8)]
    net.set_patch_table(plain_table(images[0].shape[0]) if u8 else None)
    return net, images, want, lgs


def check_rows(name, feeds, u8=False, view=True):
    """the stream over ``feeds``: rows, fed, iterations against the integers, mem_idx against the full loop resumed to the
    stream's iteration and view_feeds after every feed; the finished stream against the oracle"""
    net, images, want, lgs = e2e_case(name, u8)
    _, _, patch, stride, pad, _ = E2E[name]
    M, I, B = net.M, net.I, len(images)
    ca = net.transf.crs_attn
    widths = [im.shape[2] for im in images]
    rows, done, launched = [0] * B, [0] * B, [0]
    idx = [torch.empty((1, M), dtype=torch.int64, device=DEV) for _ in range(B)]
    tie = torch.zeros((1,), dtype=torch.int32, device=DEV)

    def after(s, bands):
        before = [rr.integers(rows[b], widths[b], patch, stride, M, I)[0] for b in range(B)]
        for b, band in enumerate(bands):
            rows[b] += 0 if band is None else band.shape[1]
        ints = [rr.integers(rows[b], widths[b], patch, stride, M, I) for b in range(B)]
        assert s.rows == tuple(rows) and s.fed == tuple(v[0] for v in ints) and s.iterations == tuple(v[1] for v in ints)
        launched[0] += any(ints[b][0] > before[b] for b in range(B))
        assert s.view_feeds == (launched[0] if view else 0)
        mem = s.mem_idx
        for b in range(B):
            fed, its = ints[b]
            if its > done[b]:                      # the full loop of this image resumed to the stream's iteration
                hip.scan_range(lgs[b], M, I, ca.H, ca.n_token, done[b], its, idx[b], tie)
                done[b] = its
            if fed < M:
                assert bool((mem[b] == -1).all())
            elif its == 0:
                assert torch.equal(mem[b], torch.arange(M, device=DEV))
            else:
                assert torch.equal(mem[b], idx[b][0]), "image %d after %d rows" % (b, rows[b])

    s, got = rr.run(net, feeds, patch, stride, pad, after)
    assert got[0].dtype == torch.float32 and got[0].is_cuda
    assert rr.same(got, want)
    assert torch.equal(s.mem_idx, want[2])
    return s, got


@pytest.mark.parametrize("name,pattern", [(n, p) for n in E2E for p in E2E[n][5]])
def test_feed_rows_equals_ips_image_ragged_on_the_joined_bands(name, pattern):
    _, images, _, _ = e2e_case(name)
    _, _, patch, stride, pad, _ = E2E[name]
    _, got = check_rows(name, rr.schedule(images, patch, stride, pattern))
    if name == "fused32_s16_pad":                  # 9 patches <= M: the count, the -1 indices and the +0.0 padding
        assert got[4] == (16, 16, 16, 9) and bool((got[2][3, 9:] == -1).all()) and bool((got[2][3, :9] == torch.arange(9, device=DEV)).all())
        assert bool((got[0][3, 9:].contiguous().view(torch.int32) == 0).all()) and bool((got[1][3, 9:].contiguous().view(torch.int32) == 0).all())
    if name.startswith("fused32_s32"):
        assert got[4] == (16, 16, 15)


def test_an_image_may_start_two_feeds_late():
    _, images, _, _ = e2e_case("fused32_s16_pos")
    feeds = rr.schedule(images, (32, 32), (16, 16), "straddle", late={1: 2})
    assert feeds[0][1] is None and feeds[1][1] is None and feeds[2][1] is not None
    feeds[1][1] = images[1][:, :0]                 # zero rows, as good as None
    check_rows("fused32_s16_pos", feeds)


def test_an_image_that_completes_no_patch_row_is_refused_at_finish():
    net, images, _, _ = e2e_case("fused32_s16_pos")
    s = net.ips_ragged_stream(pad=True, patch_size=(32, 32), patch_stride=(16, 16))
    s.feed_rows(images + [torch.zeros((1, 20, 160), device=DEV)])
    assert s.fed == (189, 55, 54, 0)
    with pytest.raises(ValueError, match="no patch row"):
        s.finish()


@pytest.mark.parametrize("name,pattern", [(n, p) for n in ("fused32_s16_pos", "fused32_s32", "fused32_s16_pad", "pool50") for p in REST])
def test_uint8_bands_equal_ips_image_ragged_on_the_uint8_images(name, pattern):
    _, images, _, _ = e2e_case(name, u8=True)
    _, _, patch, stride, _, _ = E2E[name]
    check_rows(name, rr.schedule(images, patch, stride, pattern), u8=True)


@pytest.mark.parametrize("u8", [False, True], ids=["float32", "uint8"])
def test_pageable_host_bands_give_the_device_result(u8):
    name = "fused32_s16_pos"
    _, images, _, _ = e2e_case(name, u8)
    host = [im.cpu() for im in images]
    for pattern in ("irregular", "straddle"):
        feeds = rr.schedule(host, (32, 32), (16, 16), pattern)
        feeds[1][2] = feeds[1][2].to(DEV)          # (each band may lie on either side)
        check_rows(name, feeds, u8)


def test_host_bands_of_three_channels_land_in_the_window():
    _, images, _, _ = e2e_case("pool100x3")
    check_rows("pool100x3", rr.schedule([im.cpu() for im in images], (100, 100), (100, 100), "irregular"))


def test_the_caller_may_overwrite_its_band_buffers_after_every_feed():
    name = "fused32_s16_pos"
    _, images, _, _ = e2e_case(name)
    bufs = [torch.empty((1, 45, im.shape[2]), device=DEV) for im in images]

    def feeds():
        for lo in range(0, 352, 45):
            bands = []
            for im, buf in zip(images, bufs):
                n = max(0, min(45, im.shape[1] - lo))
                buf.fill_(float("nan"))            # (stream-ordered behind the feed that read the buffer)
                buf[:, :n] = im[:, lo:lo + n]
                bands.append(buf[:, :n] if n else None)
            yield bands

    check_rows(name, feeds())


def test_blank_patches_are_encoded_once_with_the_same_bits(monkeypatch):
    """images that are zero except for a few 32-px blocks: IPSX_DEDUP_BLANK unset (the fused trunk dedups the feed's blank
    patches) and 0 (plain launches) give the same result, and both the oracle's"""
    net = net_for("mnist", N=300, M=16, I=16)
    net.set_patch_table(None)
    gen = torch.Generator().manual_seed(31)
    images = [torch.zeros(s, device=DEV) for s in FUSED]
    for im, spots in zip(images, ([(0, 0), (96, 64), (300, 100)], [(40, 10), (150, 60)], [(5, 120), (80, 0)])):
        for y, x in spots:
            im[:, y:y + 32, x:x + 32] = torch.randn((1, 32, 32), generator=gen).to(DEV)
    patch, stride = (32, 32), (16, 16)
    monkeypatch.delenv("IPSX_DEDUP_BLANK", raising=False)
    want = rr.keep(rr.record(net, net.ips_image_ragged(images, patch, stride)))
    got = {}
    for env in (None, "0"):
        if env is not None:
            monkeypatch.setenv("IPSX_DEDUP_BLANK", env)
        s, got[env] = rr.run(net, rr.schedule(images, patch, stride, "irregular"), patch, stride)
        got[env] = rr.keep(got[env])
        assert s.view_feeds > 0
    assert rr.same(got[None], got["0"]) and rr.same(got[None], want)


# ------------------------------------------------------------------ the fallbacks select the same
def feed_unfolded(net, images, patch, stride):
    s = net.ips_ragged_stream()
    s.feed([hip.patchify(im[None], patch, stride)[0] for im in images])
    return rr.keep(rr.record(net, s.finish()))


def test_a_generic_stem_takes_the_patch_tensors():
    net = net_for("generic", N=12, M=4, I=2)
    gen = torch.Generator().manual_seed(21)
    images = [torch.randn(s, generator=gen).to(DEV) for s in ((3, 125, 150), (3, 160, 100))]
    patch, stride = (37, 45), (37, 45)
    assert not net.plan.ragged_view_supported(hip.RaggedView(3, [(125, 150)], [0], patch, stride))
    want = feed_unfolded(net, images, patch, stride)
    for pattern in ("stride", "straddle", "irregular", "whole"):
        s, got = rr.run(net, rr.schedule(images, patch, stride, pattern), patch, stride)
        assert s.fed == (9, 8) and s.view_feeds == 0 and rr.same(got, want)


def test_bf16_precision_takes_the_patch_tensors(monkeypatch):
    monkeypatch.setenv("IPSX_PRECISION", "bf16")
    net = synth.fill_weights(IPSNet(DEV, synth.mnist_conf(N=300, M=16, I=16)), 5).to(DEV).eval()
    net.shuffle = False
    gen = torch.Generator().manual_seed(22)
    images = [torch.randn(s, generator=gen).to(DEV) for s in FUSED]
    patch, stride = (32, 32), (16, 16)
    want = feed_unfolded(net, images, patch, stride)
    for pattern in ("straddle", "irregular"):
        s, got = rr.run(net, rr.schedule(images, patch, stride, pattern), patch, stride)
        assert s.fed == (189, 55, 54) and s.view_feeds == 0 and rr.same(got, want)


# ------------------------------------------------------------------ memory
def test_the_state_does_not_grow_with_the_images():
    """Bands of 64 rows (slices of the resident images), 32 px at stride 16: every feed allocates the same - the peak above
    what is allocated before the stream is identical with the heights as given and with every height four times that."""
    net = net_for("mnist", N=1200, M=16, I=16, use_pos=False)
    net.set_patch_table(None)
    gen = torch.Generator().manual_seed(23)
    heights, widths = (512, 384, 256), (160, 96, 161)
    images = [torch.randn((1, 4 * h, w), generator=gen).to(DEV) for h, w in zip(heights, widths)]

    def run(scale):
        s = net.ips_ragged_stream(patch_size=(32, 32), patch_stride=(16, 16))
        s.feed_rows_all([im[:, :scale * h] for im, h in zip(images, heights)], 64)
        return s.finish()

    run(1)                                         # warm: weights packed, the folded query made
    peaks = {}
    for scale in (1, 4):
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(DEV)
        base = torch.cuda.memory_allocated(DEV)
        out = run(scale)
        torch.cuda.synchronize()
        peaks[scale] = torch.cuda.max_memory_allocated(DEV) - base
        del out
    print("peak above the resident images: heights x1: %d B, x4: %d B" % (peaks[1], peaks[4]))
    assert peaks[4] == peaks[1]


@pytest.mark.parametrize("dedup", ["0", None], ids=["plain", "dedup"])
def test_a_feed_does_not_allocate_its_patch_tensor(dedup, monkeypatch):
    """Widths 392 / 456 / 520, 32 px at stride 8, bands of 64 rows: a warmed feed's windows have 24 + 64 rows and complete 8
    patch rows of 46 / 54 / 62 patches.  Their patch tensor would be 1,296 x 4 KiB = 5.3 MB; what a feed of plain launches
    may allocate - windows 0.48 MB, piece embeddings 0.66 MB, piece logits 0.17 MB, ids - is under a quarter of that, so
    half the tensor's bytes is only reached by making it.  (The blank-patch dedup adds its workspace, the compacted
    embeddings: another 0.68 MB, still far below half.)"""
    widths, band, (ph, pw), (sh, sw) = (392, 456, 520), 64, (32, 32), (8, 8)
    if dedup is None:
        monkeypatch.delenv("IPSX_DEDUP_BLANK", raising=False)
    else:
        monkeypatch.setenv("IPSX_DEDUP_BLANK", dedup)
    net = net_for("mnist", N=2116, M=16, I=16, use_pos=False)
    net.set_patch_table(None)
    ca = net.transf.crs_attn
    rows = (ph - sh) + band
    n_k = sum(((rows - ph) // sh + 1) * ((w - pw) // sw + 1) for w in widths)
    tensor_bytes = n_k * ph * pw * 4
    legitimate = sum(rows * w * 4 + 64 for w in widths) + n_k * (net.D * 4 + ca.H * ca.n_token * 4 + 8)
    assert n_k == 8 * (46 + 54 + 62) and tensor_bytes >= 4 * legitimate
    gen = torch.Generator().manual_seed(24)
    images = [torch.randn((1, 5 * band, w), generator=gen).to(DEV) for w in widths]
    s = net.ips_ragged_stream(patch_size=(ph, pw), patch_stride=(sh, sw))
    for k in range(3):                             # warmed: the tables exist, the logits tables have their size
        s.feed_rows([im[:, k * band:(k + 1) * band] for im in images])
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.memory_allocated(DEV)
    fed = sum(s.fed)
    s.feed_rows([im[:, 3 * band:4 * band] for im in images])
    torch.cuda.synchronize()
    used = torch.cuda.max_memory_allocated(DEV) - base
    print("peak growth of a feed: %.2f MB (patch tensor %.2f MB, legitimate %.2f MB)" % (used / 1e6, tensor_bytes / 1e6, legitimate / 1e6))
    assert sum(s.fed) == fed + n_k and s.view_feeds == 4
    assert used < tensor_bytes // 2
    s.finish()


# ------------------------------------------------------------------ feed_rows_all
def test_feed_rows_all_on_a_device_list_and_on_a_host_batch():
    net, images, want, _ = e2e_case("fused32_s16_pos")
    patch, stride = (32, 32), (16, 16)
    s = net.ips_ragged_stream(patch_size=patch, patch_stride=stride)
    assert s.feed_rows_all(images, 100) is s
    assert s.rows == (352, 200, 120) and s.view_feeds == 4 and rr.same(rr.record(net, s.finish()), want)
    s = net.ips_ragged_stream(patch_size=patch, patch_stride=stride)
    s.feed_rows_all(RaggedImages.from_list([im.cpu() for im in images]), 77)
    assert rr.same(rr.record(net, s.finish()), want)


# ------------------------------------------------------------------ refusals
def test_refusals_come_before_any_launch_or_allocation_on_the_device(monkeypatch):
    net, images, want, _ = e2e_case("fused32_s16_pos")
    patch, stride = (32, 32), (16, 16)
    with pytest.raises(TypeError, match="patch stream"):
        net.ips_ragged_stream().feed_rows([im[:, :40] for im in images])
    net.ips_image_ragged(images, patch, stride)    # something to leave behind
    s = net.ips_ragged_stream(patch_size=patch, patch_stride=stride)
    s.feed_rows([im[:, :100] for im in images])
    nxt = [im[:, 100:120] for im in images]

    def swap(b, band):
        return [band if k == b else x for k, x in enumerate(nxt)]
    bad = [(ValueError, nxt[:2]),                                                      # another entry count than B
           (ValueError, swap(1, torch.zeros((2, 20, 96), device=DEV))),                # another C
           (ValueError, swap(1, torch.zeros((1, 20, 97), device=DEV))),                # another width
           (TypeError, swap(0, nxt[0].half())), (TypeError, swap(0, nxt[0].to(torch.uint8))),        # another dtype
           (ValueError, swap(0, nxt[0][0])), (ValueError, swap(0, nxt[0][None])),      # another dimensionality
           (ValueError, swap(0, torch.zeros((1, 16 * 40, 160), device=DEV))),          # 45 patch rows of 9 pass conf.N = 300
           (ValueError, [None, None, None]), (ValueError, [None, images[1][:, :0], None]),           # no pixel row at all
           (TypeError, Ragged(torch.zeros((4, 1, 32, 32), device=DEV), [2, 1, 1])),
           (TypeError, RaggedImages.from_list(nxt))]
    patches = Ragged(torch.zeros((4, 1, 32, 32), device=DEV), [2, 1, 1])
    torch.manual_seed(5)
    torch.cuda.manual_seed_all(5)
    torch.cuda.synchronize()

    def state():
        return ([None if t is None else t.clone() for st in s._sets for t in st], [None if c is None else c.clone() for c in s._carry],
                s._held, s._cur, s.fed, s.rows, s.iterations, s.view_feeds, [g.carry for g in s._geoms],
                rr.keep(rr.record(net, (None, None))), torch.get_rng_state(), torch.cuda.get_rng_state(DEV))

    def unchanged(a, b):
        return all((x is None and y is None) or torch.equal(x, y) for k in (0, 1) for x, y in zip(a[k], b[k])) and a[2:9] == b[2:9] and \
            rr.same(a[9], b[9]) and torch.equal(a[10], b[10]) and torch.equal(a[11], b[11])

    before = state()
    gc.collect()
    allocated = torch.cuda.memory_allocated(DEV)
    for exc, bands in bad:
        with pytest.raises(exc):
            s.feed_rows(bands)
        assert torch.cuda.memory_allocated(DEV) == allocated
    with pytest.raises(TypeError, match="row stream"):
        s.feed(patches)
    with monkeypatch.context() as m:
        m.setenv("IPSX_DEDUP_BLANK", "1")
        with pytest.raises(TypeError, match="dedup"):
            s.feed_rows(nxt)
    with monkeypatch.context() as m:
        m.setattr(hip, "_WEIGHTS_GENERATION", hip.weights_generation() + 1)            # a weight update between feeds
        with pytest.raises(RuntimeError, match="weights changed"):
            s.feed_rows(nxt)
    assert torch.cuda.memory_allocated(DEV) == allocated
    assert unchanged(before, state())
    del before
    # the first feed's own refusals: nothing has begun, nothing is allocated
    def fresh(size=patch):
        return net.ips_ragged_stream(patch_size=size, patch_stride=stride)
    u8 = torch.zeros((1, 40, 160), dtype=torch.uint8, device=DEV)
    c3 = torch.zeros((3, 40, 160), device=DEV)
    gc.collect()
    allocated = torch.cuda.memory_allocated(DEV)
    for exc, match, st, bands in [(ValueError, "do not fit", fresh((32, 100)), [im[:, :40] for im in images]),     # pw > W_1 = 96
                                  (ValueError, "channels", fresh(), [c3]),
                                  (TypeError, "dequantisation table", fresh(), [u8])]:
        with pytest.raises(exc, match=match):
            st.feed_rows(bands)
        assert st.rows is None and st.fed == () and st._sets is None
        assert torch.cuda.memory_allocated(DEV) == allocated
    net.patch_table = plain_table(2).to(DEV)       # a table of another row count (set_patch_table refuses it)
    try:
        with pytest.raises(ValueError, match="patch table"):
            fresh().feed_rows([u8])
    finally:
        net.set_patch_table(None)
    for mode in ("bf16", "fp32x3"):                # uint8 goes with the exact trunk
        with monkeypatch.context() as m:
            m.setenv("IPSX_PRECISION", mode)
            net.set_patch_table(plain_table(1))
            try:
                with pytest.raises(TypeError, match="exact trunk"):
                    fresh().feed_rows([u8])
            finally:
                net.set_patch_table(None)
    # the stream goes on as if nothing had been tried
    s.feed_rows([im[:, 100:] for im in images])
    assert rr.same(rr.record(net, s.finish()), want)
    with pytest.raises(RuntimeError, match="finished"):
        s.feed_rows(nxt)
