"""Row streams on the GPU (``IPSNet.ips_stream(patch_size, patch_stride)``, ips_amd/stream.py):
``hip.stream_commit_view`` against ``hip.stream_commit`` on the unfolded window - every load tier, odd image addresses,
guarded destinations and poisoned uncovered pixels -, ``feed_rows`` over bands that end anywhere against ``ips_image`` on
the concatenation with the stream's state checked after every feed, uint8 and host bands, the fallbacks, memory, and the
refusals."""

import pytest
import torch

from ips_amd import hip, synth
from ips_amd.architecture import IPSNet
from tests.stream_rows_cases import band_patterns, bands_of
from view_cases import guarded_images, unfold
from view_u8_cases import guarded_images_u8, plain_table

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


# ------------------------------------------------------------------ 1. the kernel against its sibling
# (B, C, H, W, patch, stride): what the window of a feed looks like
KERNEL_GEOMS = {
    "p32_w160_s16": (2, 1, 64, 160, (32, 32), (16, 16)),        # 16-byte tier
    "p32_w161_s16": (2, 1, 64, 161, (32, 32), (16, 16)),        # a row pitch that is no multiple of 4 pixels
    "p32_w128_s6": (2, 1, 64, 128, (32, 32), (16, 6)),          # a column stride that is no multiple of 4 pixels
    "p50_s25": (2, 1, 75, 125, (50, 50), (25, 25)),
    "p100x3_w212": (2, 3, 150, 212, (100, 100), (50, 100)),
}
F32_SENTINEL, U8_SENTINEL = 7e30, 254


def tier(g, elem, k_bytes):
    """The width the launch must take, from the numbers: the widest of 16 / 4 / 1 bytes that divides the images' address, and
    w, sw and pw in bytes (the tables come from the allocator: 256-byte aligned)."""
    w, pw, sw = g[3], g[4][1], g[5][1]
    for u in (16, 4, 1):
        if all(v % u == 0 for v in (k_bytes, w * elem, sw * elem, pw * elem)):
            return u


def test_the_tiers_of_the_lattice_written_out():
    got = {(n, e): tier(g, e, 0) for n, g in KERNEL_GEOMS.items() for e in (4, 1)}
    assert got == {("p32_w160_s16", 4): 16, ("p32_w160_s16", 1): 16, ("p32_w161_s16", 4): 4, ("p32_w161_s16", 1): 1,
                   ("p32_w128_s6", 4): 4, ("p32_w128_s6", 1): 1, ("p50_s25", 4): 4, ("p50_s25", 1): 1,
                   ("p100x3_w212", 4): 16, ("p100x3_w212", 1): 4}


def _tables(B, M, n_held, n_piece, patches, gen):
    """held rows and pieces of the four tables of a feed: patch rows, 128-float embeddings, ids (one piece shared by the
    images), 32-float logits (selection only: all rows held)"""
    u8 = patches.dtype == torch.uint8
    held_p = (torch.randint(0, 251, (B, n_held + 3) + tuple(patches.shape[2:]), generator=gen, dtype=torch.uint8) if u8 else
              torch.randn((B, n_held + 3) + tuple(patches.shape[2:]), generator=gen)).to(DEV)
    held_e = torch.randn((B, n_held + 3, 128), generator=gen).to(DEV)
    piece_e = torch.randn((B, n_piece, 128), generator=gen).to(DEV)
    held_i = torch.arange(B * (n_held + 3), dtype=torch.int64, device=DEV).view(B, -1)
    piece_i = torch.arange(1000, 1000 + n_piece, dtype=torch.int64, device=DEV).unsqueeze(0)
    lg = torch.randn((B, n_held + n_piece, 32), generator=gen).to(DEV)
    return held_p, held_e, piece_e, held_i, piece_i, lg


def check_commit_view(name, u8, k):
    g = KERNEL_GEOMS[name]
    B, M = g[0], 4
    patch, stride = g[4], g[5]
    # pixels no patch covers are NaN / 255, and so is everything around the images
    window = guarded_images_u8(g, k, device=DEV) if u8 else guarded_images(g, k, device=DEV)
    elem = window.element_size()
    assert window.data_ptr() % 16 == (k * elem) % 16
    view = hip.PatchView(window.shape, patch, stride)
    patches = unfold(window, patch, stride) if u8 else hip.patchify(window, patch, stride)
    assert not (patches == 255).any() if u8 else bool(torch.isfinite(patches).all())
    n_piece, n_held = view.per_image, M + 2
    n_cand = n_held + n_piece
    gen = torch.Generator().manual_seed(17 * k + len(name))
    held_p, held_e, piece_e, held_i, piece_i, lg = _tables(B, M, n_held, n_piece, patches, gen)
    want_tier = tier(g, elem, k * elem)

    def dsts(rows):
        fill = U8_SENTINEL if u8 else F32_SENTINEL
        return (torch.full((B, rows) + tuple(patches.shape[2:]), fill, dtype=patches.dtype, device=DEV),
                torch.full((B, rows, 128), F32_SENTINEL, device=DEV), torch.full((B, rows), -5, dtype=torch.int64, device=DEV),
                torch.full((B, rows, 32), F32_SENTINEL, device=DEV))

    for tail in (0, 1, 3):                         # selection: the m winners, then the last `tail` candidates
        sel = torch.stack([torch.randperm(n_cand, generator=gen)[:M] for _ in range(B)])
        sel[0, 0], sel[1, 1], sel[0, 2], sel[1, 3] = 0, n_held - 1, n_held, n_cand - 1       # both segments, the seam, the last patch
        sel = sel.to(DEV)
        got, want = dsts(M + tail + 1), dsts(M + tail + 1)                                   # (the last row is the guard)
        used = hip.stream_commit_view([(held_p, n_held, None, got[0]), (held_e, n_held, piece_e, got[1]),
                                       (held_i, n_held, piece_i, got[2]), (lg, n_cand, None, got[3])], window, view, sel, M, n_cand,
                                      n_cand - tail)
        hip.stream_commit([(held_p, n_held, patches, want[0]), (held_e, n_held, piece_e, want[1]),
                           (held_i, n_held, piece_i, want[2]), (lg, n_cand, None, want[3])], sel, M, n_cand, n_cand - tail)
        assert used == want_tier, (name, u8, k, used)
        for a, b in zip(got, want):
            assert torch.equal(a, b), (name, u8, k, tail)
        assert bool((got[0][:, M + tail] == (U8_SENTINEL if u8 else F32_SENTINEL)).all()) and bool((got[2][:, M + tail] == -5).all())
        assert not (got[0][:, :M + tail] == 255).any() if u8 else bool(torch.isfinite(got[0]).all())
    # append: the piece goes behind the held rows, in place; rows in front and the guard row behind stay
    got, want = dsts(n_cand + 1), dsts(n_cand + 1)
    for d in (got, want):
        d[0][:, :n_held], d[1][:, :n_held], d[2][:, :n_held] = held_p[:, :n_held], held_e[:, :n_held], held_i[:, :n_held]
    used = hip.stream_commit_view([(got[0], n_held, None, got[0]), (got[1], n_held, piece_e, got[1]), (got[2], n_held, piece_i, got[2])],
                                  window, view, None, M, n_cand)
    hip.stream_commit([(want[0], n_held, patches, want[0]), (want[1], n_held, piece_e, want[1]), (want[2], n_held, piece_i, want[2])],
                      None, M, n_cand)
    assert used == want_tier
    for a, b in zip(got[:3], want[:3]):
        assert torch.equal(a, b), (name, u8, k, "append")
    assert torch.equal(got[0][:, :n_held], held_p[:, :n_held]) and torch.equal(got[0][:, n_held:n_cand], patches)
    assert bool((got[0][:, n_cand] == (U8_SENTINEL if u8 else F32_SENTINEL)).all())
    torch.cuda.synchronize()


@pytest.mark.parametrize("k", [0, 1], ids=["base+0", "base+4"])
@pytest.mark.parametrize("name", list(KERNEL_GEOMS))
def test_commit_view_equals_commit_on_the_unfolded_window_float32(name, k):
    check_commit_view(name, False, k)


@pytest.mark.parametrize("k", [0, 1, 2, 4])
@pytest.mark.parametrize("name", list(KERNEL_GEOMS))
def test_commit_view_equals_commit_on_the_unfolded_window_uint8(name, k):
    check_commit_view(name, True, k)


# ------------------------------------------------------------------ 2. clamping
@pytest.mark.parametrize("n_held", [0, 3])
def test_commit_view_clamps_the_selection_into_the_candidates(n_held):
    g = KERNEL_GEOMS["p32_w161_s16"]
    B, M = 2, 4
    window = guarded_images(g, 1, device=DEV)      # NaN around the images and between the patches
    view = hip.PatchView(window.shape, g[4], g[5])
    patches = hip.patchify(window, g[4], g[5])
    n_cand = n_held + view.per_image
    held = torch.randn((B, 5, 1, 32, 32), generator=torch.Generator().manual_seed(2)).to(DEV)
    sel = torch.tensor([[-1, n_cand, 1, -(1 << 40)], [1 << 40, -1, n_cand - 1, n_cand]], device=DEV)
    dst = torch.full((B, M + 1, 1, 32, 32), F32_SENTINEL, device=DEV)
    hip.stream_commit_view([(held if n_held else None, n_held, None, dst)], window, view, sel, M, n_cand, n_cand)
    cand = torch.cat((held[:, :n_held], patches), 1)
    want = torch.gather(cand, 1, sel.clamp(0, n_cand - 1).view(B, M, 1, 1, 1).expand(-1, -1, 1, 32, 32))
    assert torch.equal(dst[:, :M], want) and bool((dst[:, M] == F32_SENTINEL).all())


# ------------------------------------------------------------------ 3. / 4. end to end
def results(net, out):
    return out[0], out[1], net.last_mem_idx, net.last_mem_emb


def same(a, b):
    return all((x is None and y is None) or (x is not None and y is not None and torch.equal(x, y)) for x, y in zip(a, b))


def full_logits(net, images, patch, stride):
    """(B, N, R) logits of every patch of the images, by the kernels ips() runs on the patch tensor"""
    x = unfold(images, patch, stride)
    B, N = x.shape[:2]
    ca = net.transf.crs_attn
    emb = net._embed(x.reshape(B * N, *x.shape[2:])).view(B, N, -1)
    return hip.logits(emb, net.pos_enc[:, :N] if net.use_pos else None, ca.folded_query(), ca.H * ca.n_token)


def check_rows(net, images, patch, stride, heights, want, lg, view=True, bands=None):
    M, I = net.M, net.I
    ca = net.transf.crs_attn
    B, W = images.shape[0], images.shape[3]
    nx = (W - patch[1]) // stride[1] + 1
    idx = torch.empty((B, M), dtype=torch.int64, device=DEV)
    tie = torch.zeros((B,), dtype=torch.int32, device=DEV)
    s = net.ips_stream(patch_size=patch, patch_stride=stride)
    rows = done = launched = 0
    for band in (bands if bands is not None else bands_of(images, heights)):
        before = s.fed
        s.feed_rows(band)
        rows += band.shape[2]
        fed = ((rows - patch[0]) // stride[0] + 1) * nx if rows >= patch[0] else 0
        assert s.rows == rows and s.fed == fed and s.iterations == max(0, fed - M) // I
        launched += fed > before
        if s.iterations > done:                    # the full loop resumed to this iteration
            hip.scan_range(lg, M, I, ca.H, ca.n_token, done, s.iterations, idx, tie)
            done = s.iterations
            assert torch.equal(s.mem_idx, idx), "after %d rows" % rows
        elif done == 0:
            assert s.mem_idx is None if fed < M else torch.equal(s.mem_idx, torch.arange(M, device=DEV).expand(B, M))
    assert s.view_feeds == (launched if view else 0)
    got = results(net, s.finish())
    assert got[0].dtype == torch.float32 and got[0].is_cuda and same(got, want)


E2E = {
    # name: (net, image shape, patch, stride, patterns)
    "fused32_s16_pos": (lambda: net_for("mnist", N=300, M=16, I=16), (2, 1, 352, 160), (32, 32), (16, 16),
                        ["ones", "stride", "straddle", "irregular", "whole"]),
    "fused32_s16": (lambda: net_for("mnist", N=300, M=16, I=16, use_pos=False), (2, 1, 352, 160), (32, 32), (16, 16),
                    ["stride", "straddle", "irregular", "whole"]),
    "fused32_s32": (lambda: net_for("mnist", N=300, M=16, I=16), (2, 1, 320, 160), (32, 32), (32, 32),
                    ["stride", "straddle", "irregular", "whole"]),
    "pool50": (lambda: net_for("mnist50", N=64, M=8, I=8), (2, 1, 400, 200), (50, 50), (50, 50),
               ["stride", "straddle", "irregular", "whole"]),
    "pool100x3": (lambda: net_for("traffic", N=12, M=4, I=4), (1, 3, 400, 300), (100, 100), (100, 100),
                  ["stride", "straddle", "irregular", "whole"]),
}
_E2E = {}


def e2e_case(name, u8=False):
    """net, images, what ips_image returns and leaves behind, the full logits - computed once, shared, never changed"""
    if (name, u8) not in _E2E:
        make, shape, patch, stride, _ = E2E[name]
        net = make()
        gen = torch.Generator().manual_seed(sum(shape))
        if u8:
            net.set_patch_table(plain_table(shape[1]))
            images = torch.randint(0, 256, shape, dtype=torch.uint8, generator=gen).to(DEV)
        else:
            net.set_patch_table(None)
            images = torch.randn(shape, generator=gen).to(DEV)
        want = tuple(None if t is None else t.clone() for t in results(net, net.ips_image(images, patch, stride)))
        assert want[2] is not None
        _E2E[(name, u8)] = (net, images, want, full_logits(net, images, patch, stride))
    return _E2E[(name, u8)]


@pytest.mark.parametrize("name,pattern", [(n, p) for n in E2E for p in E2E[n][4]])
def test_feed_rows_equals_ips_image_on_the_concatenation(name, pattern):
    net, images, want, lg = e2e_case(name)
    net.set_patch_table(None)
    _, shape, patch, stride, _ = E2E[name]
    check_rows(net, images, patch, stride, band_patterns(shape[2], patch[0], stride[0])[pattern], want, lg)


@pytest.mark.parametrize("name,pattern", [(n, p) for n in ("fused32_s16_pos", "fused32_s32", "pool50") for p in E2E[n][4]])
def test_uint8_bands_equal_ips_image_on_uint8_images(name, pattern):
    net, images, want, lg = e2e_case(name, u8=True)
    net.set_patch_table(plain_table(images.shape[1]))
    _, shape, patch, stride, _ = E2E[name]
    check_rows(net, images, patch, stride, band_patterns(shape[2], patch[0], stride[0])[pattern], want, lg)


@pytest.mark.parametrize("u8", [False, True], ids=["float32", "uint8"])
def test_host_bands_give_the_device_result(u8):
    name = "fused32_s16_pos"
    net, images, want, lg = e2e_case(name, u8=u8)
    net.set_patch_table(plain_table(1) if u8 else None)
    _, shape, patch, stride, _ = E2E[name]
    host = images.cpu()
    for pattern in ("irregular", "straddle"):
        heights = band_patterns(shape[2], 32, 16)[pattern]
        check_rows(net, images, patch, stride, heights, want, lg, bands=bands_of(host, heights))


def test_the_caller_may_overwrite_a_device_band_after_every_feed():
    name = "fused32_s16_pos"
    net, images, want, lg = e2e_case(name)
    net.set_patch_table(None)
    buf = torch.empty((2, 1, 45, 160), device=DEV)

    def bands():
        for lo in range(0, 352, 45):
            n = min(45, 352 - lo)
            buf.fill_(float("nan"))                # (stream-ordered behind the feed that read the buffer)
            buf[:, :, :n] = images[:, :, lo:lo + n]
            yield buf[:, :, :n]

    check_rows(net, images, (32, 32), (16, 16), None, want, lg, bands=bands())


# ------------------------------------------------------------------ 5. the fallbacks select the same
def feed_unfolded(net, images, patch, stride):
    s = net.ips_stream()
    s.feed(unfold(images, patch, stride) if images.dtype == torch.uint8 else hip.patchify(images, patch, stride))
    return results(net, s.finish())


def test_a_generic_stem_takes_the_patch_tensor():
    net = net_for("generic", N=9, M=4, I=2)
    images = torch.randn((2, 3, 125, 150), generator=torch.Generator().manual_seed(21)).to(DEV)
    patch, stride = (37, 45), (37, 45)
    assert not net.selection.plan().view_supported(hip.PatchView(images.shape, patch, stride))
    want = feed_unfolded(net, images, patch, stride)
    for pattern in ("stride", "straddle", "irregular", "whole"):
        s = net.ips_stream(patch, stride)
        for band in bands_of(images, band_patterns(125, 37, 37)[pattern]):
            s.feed_rows(band)
        assert s.fed == 9 and s.view_feeds == 0
        assert same(results(net, s.finish()), want)


def test_bf16_precision_takes_the_patch_tensor(monkeypatch):
    monkeypatch.setenv("IPSX_PRECISION", "bf16")
    net = synth.fill_weights(IPSNet(DEV, synth.mnist_conf(N=300, M=16, I=16)), 5).to(DEV).eval()
    net.shuffle = False
    images = torch.randn((2, 1, 352, 160), generator=torch.Generator().manual_seed(22)).to(DEV)
    patch, stride = (32, 32), (16, 16)
    want = feed_unfolded(net, images, patch, stride)
    for pattern in ("straddle", "irregular"):
        s = net.ips_stream(patch, stride)
        for band in bands_of(images, band_patterns(352, 32, 16)[pattern]):
            s.feed_rows(band)
        assert s.fed == 189 and s.view_feeds == 0
        assert same(results(net, s.finish()), want)


# ------------------------------------------------------------------ 6. memory
def test_the_state_does_not_grow_with_the_image():
    """Bands of 64 rows (slices of the resident images), 32 px at stride 16 on W = 160: every feed allocates the same - the
    peak above what is allocated before the stream is identical at H = 512 and H = 2,048."""
    net = net_for("mnist", N=1200, M=16, I=16, use_pos=False)
    images = torch.randn((2, 1, 2048, 160), generator=torch.Generator().manual_seed(23)).to(DEV)

    def run(H):
        s = net.ips_stream((32, 32), (16, 16))
        for lo in range(0, H, 64):
            s.feed_rows(images[:, :, lo:lo + 64])
        return s.finish()

    run(512)                                       # warm: weights packed, the folded query made
    peaks = {}
    for H in (512, 2048):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(DEV)
        base = torch.cuda.memory_allocated(DEV)
        out = run(H)
        torch.cuda.synchronize()
        peaks[H] = torch.cuda.max_memory_allocated(DEV) - base
        del out
    print("peak above the resident images: H = 512: %d B, H = 2,048: %d B" % (peaks[512], peaks[2048]))
    assert peaks[2048] == peaks[512]


def test_a_feed_does_not_allocate_its_patch_tensor():
    """B = 4, W = 392, 32 px at stride 8, bands of 64 rows: a warmed feed's window has 24 + 64 rows and completes 8 patch rows of
    46 patches.  Their patch tensor would be 4 x 368 x 4 KiB = 6.03 MB; what the feed may allocate - window 0.55 MB, piece
    embeddings 0.75 MB, piece logits 0.19 MB - is under a quarter of that, so half the tensor's bytes is only reached by
    making it."""
    B, W, band, (ph, pw), (sh, sw) = 4, 392, 64, (32, 32), (8, 8)
    net = net_for("mnist", N=2116, M=16, I=16, use_pos=False)
    ca = net.transf.crs_attn
    nx = (W - pw) // sw + 1
    rows = (ph - sh) + band
    n_k = ((rows - ph) // sh + 1) * nx
    tensor_bytes = B * n_k * ph * pw * 4
    legitimate = B * rows * W * 4 + B * n_k * net.D * 4 + B * n_k * ca.H * ca.n_token * 4
    assert (nx, n_k) == (46, 368) and tensor_bytes >= 4 * legitimate
    images = torch.randn((B, 1, 5 * band, W), generator=torch.Generator().manual_seed(24)).to(DEV)
    s = net.ips_stream((ph, pw), (sh, sw))
    for k in range(3):                             # warmed: the tables exist, the logits tables have their size
        s.feed_rows(images[:, :, k * band:(k + 1) * band])
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.memory_allocated(DEV)
    fed = s.fed
    s.feed_rows(images[:, :, 3 * band:4 * band])
    torch.cuda.synchronize()
    used = torch.cuda.max_memory_allocated(DEV) - base
    print("peak growth of a feed: %.2f MB (patch tensor %.2f MB, legitimate %.2f MB)" % (used / 1e6, tensor_bytes / 1e6, legitimate / 1e6))
    assert s.fed == fed + n_k and s.view_feeds == 4
    assert used < tensor_bytes // 2
    s.finish()


# ------------------------------------------------------------------ 7. refusals
def test_refusals_come_before_any_launch_on_the_device(monkeypatch):
    net, images, _, _ = e2e_case("fused32_s16_pos")
    net.set_patch_table(None)
    with pytest.raises(TypeError, match="patch stream"):
        net.ips_stream().feed_rows(images[:, :, :40])
    s = net.ips_stream((32, 32), (16, 16))
    s.feed_rows(images[:, :, :100])
    bad = [(TypeError, images[:, :, 100:140].half()), (TypeError, images[:, :, 100:140].to(torch.uint8)),
           (ValueError, images[:1, :, 100:140]), (ValueError, images[:, :, 100:140, :128]), (ValueError, images[0, :, 100:140]),
           (ValueError, torch.zeros((2, 1, 16 * 40, 160), device=DEV))]       # 40 more patch rows: past the 300 rows of the table
    patches = torch.zeros((2, 4, 1, 32, 32), device=DEV)
    torch.cuda.synchronize()

    def state():
        return ([None if t is None else t.clone() for st in s._sets for t in st], s._held, s._cur, s.fed, s.rows, s.iterations,
                s.view_feeds, net.selection.view_calls, s._carry.clone())

    def unchanged(a, b):
        return all(torch.equal(x, y) if torch.is_tensor(x) else x == y for x, y in zip(a[0], b[0])) and a[1:-1] == b[1:-1] and \
            torch.equal(a[-1], b[-1])

    before = state()
    allocated = torch.cuda.memory_allocated(DEV)
    for exc, band in bad:
        with pytest.raises(exc):
            s.feed_rows(band)
        assert torch.cuda.memory_allocated(DEV) == allocated
    with pytest.raises(TypeError, match="row stream"):
        s.feed(patches)
    monkeypatch.setenv("IPSX_DEDUP_BLANK", "1")
    with pytest.raises(TypeError, match="dedup"):
        s.feed_rows(images[:, :, 100:140])
    monkeypatch.delenv("IPSX_DEDUP_BLANK")
    assert torch.cuda.memory_allocated(DEV) == allocated
    assert unchanged(before, state())
    with pytest.raises(ValueError, match="do not fit"):
        net.ips_stream((32, 200), (16, 16)).feed_rows(images[:, :, :40])
    with pytest.raises(TypeError, match="dequantisation table"):
        net.ips_stream((32, 32), (16, 16)).feed_rows(torch.zeros((2, 1, 40, 160), dtype=torch.uint8, device=DEV))
    s.feed_rows(images[:, :, 100:])
    s.finish()
    with pytest.raises(RuntimeError, match="finished"):
        s.feed_rows(images[:, :, :40])
