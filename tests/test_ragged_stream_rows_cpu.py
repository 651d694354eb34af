"""The ragged ROW stream without a GPU (``IPSNet.ips_ragged_stream(patch_size=, patch_stride=)``): the ATen
route - B solo row streams - against ``ips_image_ragged`` on the joined bands of a CPU net, over every band pattern, with
``pad``, a late start and uint8 bands; the per-image geometry at ``sh > ph``; ``feed_rows_all``; every refusal with the
stream's state, ``last_*`` and the RNG untouched; the new export; and the extended wrapper's argument checks against a
stand-in library."""

import ctypes as C
import os
import re

import pytest
import torch

from ips_amd import hip, hip_encoder, hip_train, synth
from ips_amd.architecture import IPSNet
from ips_amd.ragged import Ragged
from ips_amd.ragged_image import RaggedImages
from tests import ragged_stream_rows_cases as rr
from view_u8_cases import plain_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ipsx.h")
CPU = torch.device("cpu")
_NETS = {}


def net_for(kind, **over):
    key = (kind, tuple(sorted(over.items())))
    if key not in _NETS:
        conf = synth.mnist_conf(patch=50, **over) if kind == "mnist50" else synth.mnist_conf(**over)
        net = synth.fill_weights(IPSNet(CPU, conf), 5).eval()
        net.shuffle = False
        _NETS[key] = net
    return _NETS[key]


# name: (net, image shapes, patch, stride, pad)
CASES = {
    "fused32_s16_pos": (lambda: net_for("mnist", N=300, M=8, I=8), [(1, 352, 160), (1, 200, 96), (1, 120, 161)], (32, 32), (16, 16), False),
    "fused32_s32": (lambda: net_for("mnist", N=300, M=8, I=8, use_pos=False), [(1, 352, 160), (1, 200, 96), (1, 120, 161)], (32, 32), (32, 32), False),
    "fused32_s16_pad": (lambda: net_for("mnist", N=300, M=16, I=16), [(1, 200, 96), (1, 40, 160), (1, 120, 161)], (32, 32), (16, 16), True),
    "pool50": (lambda: net_for("mnist50", N=64, M=8, I=8), [(1, 400, 200), (1, 250, 150)], (50, 50), (50, 50), False),
}
PATTERNS = ("ones", "stride", "straddle", "irregular", "whole")
_REF = {}


def case(name, u8=False):
    """net, images, what ips_image_ragged returns and leaves behind on them - computed once, shared, never changed"""
    if (name, u8) not in _REF:
        make, shapes, patch, stride, pad = CASES[name]
        net = make()
        gen = torch.Generator().manual_seed(sum(s[1] for s in shapes))
        if u8:
            net.set_patch_table(plain_table(shapes[0][0]))
            images = [torch.randint(0, 256, s, dtype=torch.uint8, generator=gen) for s in shapes]
        else:
            net.set_patch_table(None)
            images = [torch.randn(s, generator=gen) for s in shapes]
        want = rr.keep(rr.record(net, net.ips_image_ragged(images, patch, stride, pad=pad)))
        _REF[(name, u8)] = (net, images, want)
    net, images, want = _REF[(name, u8)]
    net.set_patch_table(plain_table(images[0].shape[0]) if u8 else None)
    return net, images, want


def check_integers(net, widths, patch, stride):
    """after every feed: rows, fed and iterations are the integers"""
    rows = [0] * len(widths)

    def after(s, bands):
        for b, band in enumerate(bands):
            rows[b] += 0 if band is None else band.shape[1]
        want = [rr.integers(rows[b], widths[b], patch, stride, net.M, net.I) for b in range(len(widths))]
        assert s.rows == tuple(rows) and s.fed == tuple(w[0] for w in want) and s.iterations == tuple(w[1] for w in want)
        assert s.view_feeds == 0
    return after


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("name", list(CASES))
def test_the_aten_route_equals_ips_image_ragged_on_the_joined_bands(name, pattern):
    net, images, want = case(name)
    _, _, patch, stride, pad = CASES[name]
    widths = [im.shape[2] for im in images]
    s, got = rr.run(net, rr.schedule(images, patch, stride, pattern), patch, stride, pad, check_integers(net, widths, patch, stride))
    assert rr.same(got, want)
    assert torch.equal(s.mem_idx, want[2])
    if pad:
        assert got[4] == (16, 9, 16) and bool((got[2][1, 9:] == -1).all())
        assert torch.equal(got[0][1, 9:].view(torch.int32), torch.zeros_like(got[0][1, 9:]).view(torch.int32))


def test_an_image_may_start_late_and_pass_zero_rows():
    net, images, want = case("fused32_s16_pos")
    feeds = rr.schedule(images, (32, 32), (16, 16), "straddle", late={1: 2})
    assert feeds[0][1] is None and feeds[1][1] is None and feeds[2][1] is not None
    feeds[1][1] = images[1][:, :0]                                    # zero rows, as good as None
    _, got = rr.run(net, feeds, (32, 32), (16, 16))
    assert rr.same(got, want)


@pytest.mark.parametrize("name", ["fused32_s16_pad", "pool50"])
def test_uint8_bands_with_a_table_equal_ips_image_ragged_on_the_bytes(name):
    net, images, want = case(name, u8=True)
    _, _, patch, stride, pad = CASES[name]
    assert want[0].dtype == torch.float32
    for pattern in ("irregular", "straddle"):
        _, got = rr.run(net, rr.schedule(images, patch, stride, pattern), patch, stride, pad)
        assert rr.same(got, want)


def test_the_geometry_of_every_image_at_a_stride_above_the_patch():
    """sh = 48 > ph = 32: the rows between two patch rows are skipped image by image, wherever the bands end."""
    net = net_for("mnist", N=300, M=8, I=8)
    net.set_patch_table(None)
    gen = torch.Generator().manual_seed(9)
    images = [torch.randn((1, 520, 96), generator=gen), torch.randn((1, 470, 128), generator=gen)]
    patch, stride = (32, 32), (48, 32)
    want = rr.keep(rr.record(net, net.ips_image_ragged(images, patch, stride)))
    widths = [96, 128]
    for pattern in ("irregular", "stride", "ones"):
        s, got = rr.run(net, rr.schedule(images, patch, stride, pattern), patch, stride, False,
                        check_integers(net, widths, patch, stride))
        assert s.fed == (11 * 3, 10 * 4) and rr.same(got, want)


def test_feed_rows_all_walks_bands_and_drops_the_images_that_ran_out():
    net, images, want = case("fused32_s16_pos")
    seen = []
    s = net.ips_ragged_stream(patch_size=(32, 32), patch_stride=(16, 16))
    feed = s.feed_rows
    s.feed_rows = lambda bands: (seen.append([None if b is None else tuple(b.shape) for b in bands]), feed(bands))[1]
    assert s.feed_rows_all(images, 100) is s
    assert seen == [[(1, 100, 160), (1, 100, 96), (1, 100, 161)], [(1, 100, 160), (1, 100, 96), (1, 20, 161)],
                    [(1, 100, 160), None, None], [(1, 52, 160), None, None]]
    assert rr.same(rr.record(net, s.finish()), want)
    s = net.ips_ragged_stream(patch_size=(32, 32), patch_stride=(16, 16))
    s.feed_rows_all(RaggedImages.from_list(images), 77)
    assert s.rows == (352, 200, 120) and rr.same(rr.record(net, s.finish()), want)
    with pytest.raises(ValueError):
        net.ips_ragged_stream(patch_size=(32, 32), patch_stride=(16, 16)).feed_rows_all(images, 0)


# ---------------------------------------------------------------- refusals
def test_the_constructor_mirrors_ips_stream():
    net = net_for("mnist", N=300, M=8, I=8)
    with pytest.raises(ValueError, match="both"):
        net.ips_ragged_stream(patch_size=(32, 32))
    with pytest.raises(ValueError, match="both"):
        net.ips_ragged_stream(patch_stride=(32, 32))
    feat = synth.fill_weights(IPSNet(CPU, synth.camelyon_conf(N=64, M=8, I=8, n_chan_in=16, D=32, D_k=8, D_v=8, D_inner=32)), 5).eval()
    with pytest.raises(TypeError, match="image encoder"):
        feat.ips_ragged_stream(patch_size=(32, 32), patch_stride=(16, 16))


def test_every_refusal_leaves_the_stream_and_the_net_as_they_were(monkeypatch):
    net, images, want = case("fused32_s16_pos")
    patch, stride = (32, 32), (16, 16)
    with pytest.raises(TypeError, match="patch stream"):
        net.ips_ragged_stream().feed_rows([im[:, :40] for im in images])
    net.ips_image_ragged(images, patch, stride)                       # something to leave behind
    s = net.ips_ragged_stream(patch_size=patch, patch_stride=stride)
    s.feed_rows([im[:, :50] for im in images])
    torch.manual_seed(5)

    def state():
        return (s.rows, s.fed, s.iterations, s.view_feeds, [g.carry for g in s._geoms], [x.fed for x in s._solo],
                [x.rows for x in s._solo], rr.keep(rr.record(net, (None, None))), torch.get_rng_state())

    def unchanged(a, b):
        return a[:7] == b[:7] and rr.same(a[7], b[7]) and torch.equal(a[8], b[8])

    before = state()
    nxt = [im[:, 50:90] for im in images]

    def swap(b, band):
        return [band if k == b else x for k, x in enumerate(nxt)]
    bad = [(ValueError, nxt[:2]),                                                      # another entry count than B
           (ValueError, swap(1, torch.zeros((2, 40, 96)))),                            # another C
           (ValueError, swap(1, torch.zeros((1, 40, 97)))),                            # another width
           (ValueError, swap(2, torch.zeros((1, 0, 160)))),                            # ... also of a band of no rows
           (TypeError, swap(0, nxt[0].double())), (TypeError, swap(0, nxt[0].to(torch.uint8))),     # another dtype
           (ValueError, swap(0, nxt[0][0])), (ValueError, swap(0, nxt[0][None])),      # another dimensionality
           (ValueError, swap(2, "band")),
           (ValueError, swap(0, torch.zeros((1, 16 * 40, 160)))),                      # 42 patch rows of 9 pass conf.N = 300 with positions
           (ValueError, [None, None, None]), (ValueError, [None, images[1][:, :0], None]),           # no pixel row at all
           (ValueError, []), (ValueError, torch.zeros((3, 1, 40, 160))),
           (TypeError, Ragged(torch.zeros((4, 1, 32, 32)), [2, 1, 1])), (TypeError, RaggedImages.from_list(nxt))]
    for exc, bands in bad:
        with pytest.raises(exc):
            s.feed_rows(bands)
        assert unchanged(before, state()), bands
    with pytest.raises(TypeError, match="row stream"):
        s.feed(Ragged(torch.zeros((4, 1, 32, 32)), [2, 1, 1]))
    with monkeypatch.context() as m:
        m.setenv("IPSX_DEDUP_BLANK", "1")
        with pytest.raises(TypeError, match="dedup"):
            s.feed_rows(nxt)
    with monkeypatch.context() as m:
        m.setattr(hip, "_WEIGHTS_GENERATION", hip.weights_generation() + 1)            # a weight update between feeds
        with pytest.raises(RuntimeError, match="weights changed"):
            s.feed_rows(nxt)
    assert unchanged(before, state())
    # the first feed's own refusals: nothing has begun
    fresh = lambda **kw: net.ips_ragged_stream(patch_size=kw.get("patch", patch), patch_stride=stride)     # noqa: E731
    for exc, match, st, bands in [
            (ValueError, "do not fit", fresh(patch=(32, 100)), [im[:, :40] for im in images]),         # pw > W_1 = 96
            (ValueError, "channels", fresh(), [torch.zeros((3, 40, 160))]),                           # not the encoder's channel count
            (TypeError, "dequantisation table", fresh(), [torch.zeros((1, 40, 160), dtype=torch.uint8)]),
            (TypeError, "float32", fresh(), [torch.zeros((1, 40, 160), dtype=torch.float16)])]:
        with pytest.raises(exc, match=match):
            st.feed_rows(bands)
        assert st.rows is None and st.fed == () and st.mem_idx is None
    net.patch_table = plain_table(2)                                   # a table of another row count (set_patch_table refuses it)
    try:
        with pytest.raises(ValueError, match="patch table"):
            fresh().feed_rows([torch.zeros((1, 40, 160), dtype=torch.uint8)])
    finally:
        net.set_patch_table(None)
    assert unchanged(before, state())
    # the stream goes on as if nothing had been tried
    for bands in rr.zipped([im[:, 50:] for im in images], [[im.shape[1] - 50] for im in images]):
        s.feed_rows(bands)
    assert rr.same(rr.record(net, s.finish()), want)
    with pytest.raises(RuntimeError, match="finished"):
        s.feed_rows(nxt)


def test_finish_refuses_what_ips_image_ragged_refuses():
    net, images, _ = case("fused32_s16_pos")
    patch, stride = (32, 32), (16, 16)
    for pad in (False, True):                                          # (1, 20, 160) completes no patch row
        s = net.ips_ragged_stream(pad=pad, patch_size=patch, patch_stride=stride)
        s.feed_rows([images[0], torch.zeros((1, 20, 160))])
        with pytest.raises(ValueError, match="no patch row"):
            s.finish()
        with pytest.raises(ValueError):
            net.ips_image_ragged([images[0], torch.zeros((1, 20, 160))], patch, stride, pad=pad)
    s = net.ips_ragged_stream(patch_size=patch, patch_stride=stride)   # 5 patches <= M without pad
    s.feed_rows([images[0], torch.zeros((1, 40, 96))])
    with pytest.raises(ValueError, match="memory M"):
        s.finish()
    with pytest.raises(RuntimeError, match="nothing was fed"):
        net.ips_ragged_stream(patch_size=patch, patch_stride=stride).finish()


def test_feed_still_refuses_uint8_patches():
    net = net_for("mnist", N=300, M=8, I=8)
    net.set_patch_table(plain_table(1))
    try:
        with pytest.raises(TypeError, match="uint8"):
            net.ips_ragged_stream().feed([torch.zeros((12, 1, 32, 32), dtype=torch.uint8)])
    finally:
        net.set_patch_table(None)


# ---------------------------------------------------------------- ABI
def test_the_new_export_is_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(ipsx_[a-z0-9_]+)\s*\(", text))
    lib = C.CDLL(hip.library_path())
    name = "ipsx_stream_commit_ragged_view"
    assert name in declared and hasattr(lib, name) and name in hip._EXPORTS
    assert len(hip._EXPORTS[name][1]) == 13
    assert hip.lib().ipsx_version() == 306


# ---------------------------------------------------------------- the wrapper's argument checks, nothing launched
class StandIn:
    """``hip.lib()`` that launches nothing: every export is recorded as (name, arguments) and returns 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def record(*args):
            self.calls.append((name, tuple(a.value if isinstance(a, C.c_void_p) else a for a in args)))
            return 0
        return record


def install(monkeypatch):
    stand, seen = StandIn(), {}

    def p(t):
        if t is None:
            return C.c_void_p(0)
        seen[t.data_ptr()] = t
        return C.c_void_p(t.data_ptr())
    for m in (hip, hip_train, hip_encoder):
        monkeypatch.setattr(m, "lib", lambda: stand)
        monkeypatch.setattr(m, "_stream", lambda: None)
        monkeypatch.setattr(m, "_p", p)
    monkeypatch.setattr(hip, "_gpu_device", lambda dev: True)
    return stand, seen


def wrapper_args():
    view = hip.RaggedView(1, [(64, 160), (48, 96)], [0, 64 * 160], (32, 32), (16, 16))      # (the real library fills the table)
    return dict(view=view, pixels=torch.arange(64 * 160 + 48 * 96, dtype=torch.float32), held=torch.zeros((3, 8, 1, 32, 32)),
                emb=torch.zeros((3, 8, 4)), piece=torch.ones((view.count, 4)), slides=torch.zeros((3, 6), dtype=torch.int64))


def commit(a, piece0=None):
    return hip.stream_commit_ragged([(a["held"], piece0, a["held"]), (a["emb"], a["piece"], a["emb"])], None, a["slides"], 4, 3,
                                    pixels=a["pixels"], view=a["view"])


def test_the_wrapper_hands_the_view_to_the_new_export(monkeypatch):
    a = wrapper_args()
    stand, seen = install(monkeypatch)
    assert commit(a) == 0                                              # (the stand-in leaves the unit as it was)
    assert [c[0] for c in stand.calls] == ["ipsx_stream_commit_ragged_view"]
    args = stand.calls[0][1]
    assert args[1] == 2 and args[2] == a["pixels"].data_ptr() and args[4] == 4 and args[7:11] == (3, 4, 3, a["view"].count)
    stand.calls.clear()
    hip.stream_commit_ragged([(a["emb"], a["piece"], a["emb"])], None, a["slides"], 4, 3)
    assert [c[0] for c in stand.calls] == ["ipsx_stream_commit_ragged"]            # without a view: the export it always ran


def test_strided_pixels_are_copied_and_bytes_stay_bytes(monkeypatch):
    a = wrapper_args()
    wide = torch.arange(2 * a["pixels"].numel(), dtype=torch.float32)
    a["pixels"] = wide[::2]
    before = a["pixels"].clone()
    stand, seen = install(monkeypatch)
    commit(a)
    handed = seen[stand.calls[0][1][2]]
    assert handed.is_contiguous() and handed.data_ptr() != a["pixels"].data_ptr() and torch.equal(handed, before)
    assert torch.equal(a["pixels"], before)
    stand.calls.clear()
    a["pixels"], a["held"] = before.to(torch.uint8), a["held"].to(torch.uint8)
    commit(a)
    assert stand.calls[0][1][4] == 1 and stand.calls[0][1][2] == a["pixels"].data_ptr()


@pytest.mark.parametrize("change", ["float64", "int32", "two_dims", "piece0", "pixels_alone", "view_alone", "row_shape", "row_dtype",
                                    "short_buffer"])
def test_the_wrapper_refuses_before_any_launch(change, monkeypatch):
    a = wrapper_args()
    kw = {}
    if change == "float64":
        a["pixels"] = a["pixels"].double()
    elif change == "int32":
        a["pixels"] = a["pixels"].to(torch.int32)
    elif change == "two_dims":
        a["pixels"] = a["pixels"].view(1, -1)
    elif change == "piece0":
        kw["piece0"] = torch.zeros((a["view"].count, 1, 32, 32))
    elif change == "row_shape":
        a["held"] = torch.zeros((3, 8, 1, 32, 16))
    elif change == "row_dtype":
        a["held"] = a["held"].to(torch.uint8)
    elif change == "short_buffer":
        a["pixels"] = a["pixels"][:-1]
    stand, _ = install(monkeypatch)
    with pytest.raises((TypeError, ValueError)) as err:
        if change == "pixels_alone":
            hip.stream_commit_ragged([(a["held"], None, a["held"])], None, a["slides"], 4, 3, pixels=a["pixels"])
        elif change == "view_alone":
            hip.stream_commit_ragged([(a["held"], None, a["held"])], None, a["slides"], 4, 3, view=a["view"])
        else:
            commit(a, **kw)
    assert stand.calls == [] and str(err.value)
    if change in ("float64", "int32"):
        assert err.type is TypeError
