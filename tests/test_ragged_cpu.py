"""``ips_amd.ragged`` without a GPU: the container and its collate function, everything ``ips_ragged`` refuses, and the
contract - a ragged call is, slide by slide and bit for bit, the loop of solo ``ips()`` calls it replaces - on the CPU
plumbing path, down to ``evaluate()`` of training/iterative.py driving ragged batches unchanged."""

import numpy as np
import pytest
import torch
from torch import nn
from torch.utils.data import DataLoader, Dataset

import ragged_cases as rc
from ips_amd import dist as ips_dist
from ips_amd.ragged import Ragged, collate_ragged
from ips_amd.training import iterative as loops

CPU = torch.device("cpu")
# 17: one candidate beyond the memory; 32: exactly one full chunk; 33 and 80: ragged ends; two slides of equal length
LENGTHS = (17, 32, 33, 80, 80)


# ------------------------------------------------------------------ container and collate
def test_container_offsets_views_and_moves():
    slides = [torch.arange(n * 3, dtype=torch.float32).view(n, 3) + 100 * k for k, n in enumerate((4, 1, 6))]
    r = Ragged.from_list(slides)
    assert len(r) == 3 and r.lengths == (4, 1, 6) and r.total == 11
    assert r.offsets.dtype == torch.int64 and r.offsets.tolist() == [0, 4, 5, 11]
    assert r.offsets is r.offsets                                  # made once, kept
    assert r.rows.is_contiguous() and tuple(r.rows.shape) == (11, 3)
    for k, s in enumerate(slides):
        assert torch.equal(r[k], s)
        assert r[k].data_ptr() == r.rows[r.starts[k]:].data_ptr()     # a view, not a copy
    assert torch.equal(r[-1], slides[-1])
    with pytest.raises(IndexError):
        r[3]
    assert r.device == CPU and r.dtype == torch.float32
    assert r.to(CPU) is r and r.to(CPU, non_blocking=True) is r
    h = r.to(torch.float16)
    assert h.dtype == torch.float16 and h.lengths == r.lengths and torch.equal(h[2], slides[2].half())
    assert torch.equal(h.offsets, r.offsets)
    assert r.row_base().tolist() == [0] * 4 + [4] + [5] * 6
    images = Ragged(torch.zeros(5, 1, 4, 4), (2, 3))
    assert tuple(images[1].shape) == (3, 1, 4, 4)
    with pytest.raises(ValueError):
        Ragged(torch.zeros(5, 3), (2, 2))
    with pytest.raises(TypeError):
        Ragged(torch.zeros(5), (5,))
    with pytest.raises(TypeError):
        Ragged.from_list([torch.zeros(2, 3), torch.zeros(2, 4)])


def test_collate_ragged_on_dict_samples_of_different_lengths():
    samples = [{'input': torch.full((n, 3), float(n)), 'label': torch.tensor(n), 'multi': torch.ones(4) * n} for n in (2, 5, 3)]
    out = collate_ragged(samples)
    assert isinstance(out['input'], Ragged) and out['input'].lengths == (2, 5, 3)
    assert torch.equal(out['input'][1], samples[1]['input'])
    assert out['label'].tolist() == [2, 5, 3] and tuple(out['multi'].shape) == (3, 4)
    loader = DataLoader(samples, batch_size=2, collate_fn=collate_ragged)
    got = [b['input'].lengths for b in loader]
    assert got == [(2, 5), (3,)]


# ------------------------------------------------------------------ the export
def test_the_export_is_declared_bound_and_checks_its_sizes_on_the_host():
    """``ipsx_scan_ragged`` in include/ipsx.h, in the binding with the header's 15 arguments, and refusing on the host -
    before any launch - what its kernels must not be handed (no GPU needed: every call below ends in the argument checks)."""
    import ctypes as C
    import os
    import re
    from ips_amd import hip
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ipsx.h")).read()
    assert "ipsx_scan_ragged" in text[text.index(" *   3.06 "):text.index("#define IPSX_VERSION")]       # listed in the history block
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"\bint\s+ipsx_scan_ragged\s*\(([^)]*)\)", plain)
    assert decl and len(decl.group(1).split(",")) == 15
    L = hip.lib()
    assert len(L.ipsx_scan_ragged.argtypes) == 15 and L.ipsx_scan_ragged.argtypes[1] is C.c_void_p
    lg, off, idx = (C.c_void_p(4096 * k) for k in (1, 2, 3))          # never dereferenced: the checks come first
    EINVAL = -1
    ok = dict(b=2, n_max=40, total=70, m=16, i=16, h=8, t=1)

    def call(lg=lg, off=off, idx=idx, **over):
        a = dict(ok, **over)
        return L.ipsx_scan_ragged(lg, off, a["b"], a["n_max"], a["total"], a["m"], a["i"], a["h"], a["t"], idx, None, None, None, 0, None)
    assert call(lg=None) == EINVAL and call(off=None) == EINVAL and call(idx=None) == EINVAL
    assert call(b=0) == EINVAL and call(m=0) == EINVAL and call(i=0) == EINVAL
    assert call(n_max=16) == EINVAL                                    # the longest slide has no more rows than the memory
    assert call(total=39) == EINVAL and call(total=81) == EINVAL      # fewer rows than the longest slide, more than b of them
    assert call(n_max=1 << 31, total=1 << 31) == EINVAL                # 2^31 rows


# ------------------------------------------------------------------ refusals
def test_refusals_before_anything_runs(monkeypatch):
    conf = rc.feature_conf(use_pos=True)
    net = rc.make_net(conf, CPU)
    ok = rc.make_slides(conf, (20, 30))
    state = torch.get_rng_state()
    with pytest.raises(ValueError, match="slide 1"):
        net.ips_ragged(rc.make_slides(conf, (20, 16)))             # N_b <= M
    with pytest.raises(ValueError, match="slide 0"):
        net.ips_ragged(rc.make_slides(conf, (conf.N + 1, 20)))      # use_pos with N_b > conf.N
    with pytest.raises(ValueError, match="empty"):
        net.ips_ragged([])
    with pytest.raises(ValueError, match="empty"):
        net.ips_ragged(Ragged(torch.zeros(0, conf.n_chan_in), ()))
    with pytest.raises(TypeError, match="uint8"):
        net.ips_ragged([s.to(torch.uint8) for s in ok])
    with pytest.raises(TypeError):
        net.ips_ragged(rc.make_slides(rc.image_conf(), (20, 30)))   # patches handed to a feature net
    assert torch.equal(torch.get_rng_state(), state)
    r = Ragged.from_list(ok)
    with pytest.raises(TypeError, match="Ragged"):
        net.ips_stream().feed(r)
    inet = rc.make_net(rc.image_conf(), CPU)
    with pytest.raises(TypeError, match="Ragged"):
        inet.ips_stream((32, 32), (32, 32)).feed_rows(r)
    with pytest.raises(TypeError, match="Ragged"):
        ips_dist.ips_sharded(net, r, 50)


def test_instance_shuffle_with_positions_is_refused_where_the_solo_call_fails():
    """``shuffle_instance`` permutes the WHOLE positional table with the slide's permutation: ``ips()`` on a slide shorter
    than conf.N raises there (as the reference does), so there is nothing for the ragged call to equal."""
    conf = rc.feature_conf(use_pos=True, shuffle=True, shuffle_style='instance')
    net = rc.make_net(conf, CPU)
    slides = rc.make_slides(conf, (20, conf.N))
    with pytest.raises(RuntimeError):
        net.ips(slides[0][None])
    state = torch.get_rng_state()
    with pytest.raises(ValueError, match="slide 0"):
        net.ips_ragged(slides)
    assert torch.equal(torch.get_rng_state(), state)
    net.ips_ragged([slides[1], slides[1]])           # N_b == conf.N: the solo calls run, and so does this


def test_blank_dedup_is_refused_as_streams_refuse_it(monkeypatch):
    conf = rc.feature_conf()
    net = rc.make_net(conf, CPU)
    slides = rc.make_slides(conf, (20, 30))
    monkeypatch.setenv("IPSX_DEDUP_BLANK", "1")
    with pytest.raises(TypeError, match="IPSX_DEDUP_BLANK"):
        net.ips_ragged(slides)
    with pytest.raises(TypeError, match="IPSX_DEDUP_BLANK"):
        net.ips_stream().feed(slides[0][None])
    monkeypatch.setenv("IPSX_DEDUP_BLANK", "0")
    net.ips_ragged(slides)


@pytest.mark.parametrize("pad, lengths", [(False, (4, 7)), (True, (0, 7))], ids=["short", "empty"])
def test_the_call_and_the_stream_refuse_short_and_empty_slides_in_the_same_words(pad, lengths):
    """M = 4: a slide of M rows without ``pad``, a slide of no rows with it - one ``ValueError`` text from ``ips_ragged`` and
    from ``RaggedIPSStream.finish()``."""
    conf = rc.feature_conf(M=4)
    net = rc.make_net(conf, CPU)
    slides = [torch.zeros(n, conf.n_chan_in) for n in lengths]
    with pytest.raises(ValueError) as call:
        net.ips_ragged(slides, pad=pad)
    with pytest.raises(ValueError) as stream:
        net.ips_ragged_stream(pad=pad).feed(slides).finish()
    assert str(call.value) == str(stream.value) and "slide 0" in str(call.value)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("style", ["batch", "instance"])
def test_the_draw_by_shape_consumes_the_rng_as_the_draw_on_a_tensor(style, B):
    from ips_amd.shuffle import draw_shuffle, draw_shuffle_for
    N = 7
    torch.manual_seed(23)
    want = draw_shuffle(torch.zeros(B, N, 5), style)
    want_next = torch.rand(1), torch.randperm(2)
    torch.manual_seed(23)
    got = draw_shuffle_for(B, N, CPU, style)
    assert got.dtype == want.dtype and torch.equal(got, want)
    assert torch.equal(torch.rand(1), want_next[0]) and torch.equal(torch.randperm(2), want_next[1])
    assert draw_shuffle_for(B, N, CPU, "none") is None and draw_shuffle(torch.zeros(B, N), "none") is None


# ------------------------------------------------------------------ the contract on CPU
@pytest.fixture(scope="module")
def nets():
    made = {}

    def get(kind, shuffle, style, use_pos):
        key = (kind, shuffle, style, use_pos)
        if key not in made:
            conf = (rc.feature_conf if kind == "feature" else rc.image_conf)(shuffle=shuffle, shuffle_style=style, use_pos=use_pos)
            made[key] = (conf, rc.make_net(conf, CPU))
        return made[key]
    return get


@pytest.mark.parametrize("kind", ["feature", "image"])
@pytest.mark.parametrize("shuffle,style,use_pos", [(False, "batch", False), (True, "batch", False), (True, "instance", False),
                                                   (False, "batch", True), (True, "batch", True)])
def test_ragged_equals_the_solo_loop_on_cpu(nets, kind, shuffle, style, use_pos):
    # ('instance' with use_pos has no solo call to equal unless N_b == conf.N: see the refusal below)
    conf, net = nets(kind, shuffle, style, use_pos)
    slides = rc.make_slides(conf, LENGTHS)
    want = rc.solo_loop(net, slides)
    assert tuple(want["mem_idx"].shape) == (len(LENGTHS), conf.M)
    assert (want["shuffle"] is not None) == shuffle
    rc.assert_same_record(rc.ragged_call(net, slides), want)
    rc.assert_same_record(rc.ragged_call(net, Ragged.from_list(slides), through_ips=True), want)
    for b, n in enumerate(LENGTHS):                                 # local indices, every slide's own range
        assert int(want["mem_idx"][b].max()) < n


def test_a_net_in_train_mode_is_scored_in_eval_mode_and_left_in_train_mode(nets):
    conf, net = nets("feature", False, "batch", False)
    slides = rc.make_slides(conf, LENGTHS)
    want = rc.solo_loop(net, slides)
    net.train()
    try:
        got = rc.ragged_call(net, slides)
        assert net.training and net.encoder.training and net.transf.training
    finally:
        net.eval()
    rc.assert_same_record(got, want)


# ------------------------------------------------------------------ evaluate() drives ragged batches unchanged
class _Slides(Dataset):
    def __init__(self, conf, lengths):
        self.x = rc.make_slides(conf, lengths, seed=23)
        self.y = [k % 2 for k in range(len(lengths))]

    def __len__(self):
        return len(self.x)

    def __getitem__(self, k):
        return {'input': self.x[k], 'metastases': torch.tensor(self.y[k])}


class _Recorder:
    def __init__(self):
        self.steps = []

    def update(self, losses, preds, labels):
        self.steps.append((losses, preds, labels))


def test_evaluate_over_ragged_batches_equals_batches_of_one():
    conf = rc.feature_conf(B=3, eps=1e-6)
    net = rc.make_net(conf, CPU)
    data = _Slides(conf, (17, 40, 33, 80, 21, 64, 50))
    crit = {'metastases': nn.BCELoss()}

    def one(x):           # a loader item of one slide: the (B_seq = 1, N, F) tensor the reference's loop sees
        out = collate_ragged(x)
        out['input'] = out['input'][0].unsqueeze(0)
        return out
    a, b = _Recorder(), _Recorder()
    loops.evaluate(net, crit, DataLoader(data, batch_size=1, collate_fn=one), CPU, a, conf)
    loops.evaluate(net, crit, DataLoader(data, batch_size=3, collate_fn=collate_ragged), CPU, b, conf)
    assert len(a.steps) == len(b.steps) == 3
    for (la, pa, ya), (lb, pb, yb) in zip(a.steps, b.steps):
        assert la == lb
        for t in pa:
            assert np.array_equal(pa[t], pb[t]) and np.array_equal(ya[t], yb[t])
