"""``ips_ragged(slides, pad=True)`` without a GPU: slides with no more rows than the memory come back
zero-padded to M rows, as ``fill_batch`` of training/iterative.py leaves them - the contract against the loop of solo
``ips()`` calls plus zero buffers on the CPU plumbing path, the refusals, the flag's way through the container, and
``evaluate()`` over padded batches against what the reference's own ``evaluate`` recorded (tests/golden/loop_ragged_pad.npz,
tools/gen_golden_ragged_pad.py)."""

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

import ragged_cases as rc
import ragged_pad_cases as pc
from ips_amd.ragged import Ragged, collate_ragged, collate_ragged_padded
from ips_amd.training import iterative as loops

CPU = torch.device("cpu")
M = 16


@pytest.fixture(scope="module")
def nets():
    made = {}

    def get(kind, shuffle, style, use_pos, N=None):
        key = (kind, shuffle, style, use_pos, N)
        if key not in made:
            conf = (rc.feature_conf if kind == "feature" else rc.image_conf)(M=M, shuffle=shuffle, shuffle_style=style, use_pos=use_pos)
            if N is not None:
                conf.N = N                          # (the positional table is made from it)
            made[key] = (conf, rc.make_net(conf, CPU))
        return made[key]
    return get


# ------------------------------------------------------------------ the contract
@pytest.mark.parametrize("kind", ["feature", "image"])
@pytest.mark.parametrize("shuffle,style", [(False, "batch"), (True, "batch"), (True, "instance")])
@pytest.mark.parametrize("use_pos", [False, True])
def test_padded_call_equals_the_solo_loop_plus_zero_buffers(nets, kind, shuffle, style, use_pos):
    lengths = pc.lengths(M)
    N = None
    if shuffle and style == "instance" and use_pos:
        # ips() itself raises on a LONG slide with N_b != conf.N here (tests/test_ragged_cpu.py): every long slide has conf.N rows
        N = 3 * M + 5
        lengths = tuple(n if n <= M else N for n in lengths)
    conf, net = nets(kind, shuffle, style, use_pos, N)
    slides = rc.make_slides(conf, lengths)
    want = pc.expected(net, slides)
    assert tuple(want["mem_patch"].shape[:2]) == (len(lengths), M) and want["count"] == tuple(min(n, M) for n in lengths)
    assert (want["shuffle"] is not None) == shuffle and (want["mem_pos"] is not None) == use_pos
    got = pc.padded_call(net, slides)
    pc.assert_same(got, want)
    pc.assert_same(pc.padded_call(net, Ragged.from_list(slides, pad=True), through_ips=True), want)
    for b, n in enumerate(lengths):
        if n <= M:                                  # stated once more, without the helper
            assert torch.equal(got["mem_patch"][b, :n], slides[b]) and got["mem_idx"][b].tolist() == list(range(n)) + [-1] * (M - n)
            pad = got["mem_patch"][b, n:]
            assert not pad.any() and not torch.signbit(pad).any()              # +0.0
            if use_pos:
                assert torch.equal(got["mem_pos"][b, :n], net.pos_enc[0, :n]) and not got["mem_pos"][b, n:].any()
            if n < M:                               # the padding's embedding: one all-zero row's
                assert all(torch.equal(got["mem_emb"][b, k], got["mem_emb"][b, n]) for k in range(n, M))


def test_a_batch_of_short_slides_only(nets):
    conf, net = nets("feature", True, "batch", True)
    slides = rc.make_slides(conf, (M, 1, M - 1))
    want = pc.expected(net, slides)
    assert want["shuffle"] is None
    calls = []
    real = net._embed
    net._embed = lambda x: (calls.append(x.shape[0]), real(x))[1]
    try:
        torch.manual_seed(11)
        net.ips_ragged(slides, pad=True)
        assert calls == [] and net.last_mem_count == (M, 1, M - 1)       # nothing is encoded until the embeddings are read
        assert net.last_mem_emb is not None and calls
    finally:
        del net._embed
    pc.assert_same(pc.padded_call(net, slides), want)


def test_a_batch_without_a_short_slide_equals_the_call_without_pad(nets):
    for shuffle in (False, True):
        conf, net = nets("feature", shuffle, "instance", False)
        slides = rc.make_slides(conf, (M + 1, 3 * M, 3 * M + 5))
        want = rc.ragged_call(net, slides)
        assert net.last_mem_count is None
        got = pc.padded_call(net, slides)
        rc.assert_same_record(got, want)
        assert got["count"] == (M, M, M)


def test_rng_shuffle_and_count_are_those_of_the_solo_loop(nets):
    conf, net = nets("feature", True, "instance", False)
    lengths = pc.lengths(M)
    slides = rc.make_slides(conf, lengths)
    torch.manual_seed(5)
    for s in slides:                                # short slides draw nothing: the generator ends where the long ones leave it
        if s.shape[0] > M:
            net.ips(s[None])
    after_long = torch.get_rng_state()
    torch.manual_seed(5)
    net.ips_ragged(slides, pad=True)
    assert torch.equal(torch.get_rng_state(), after_long)
    assert [s is None for s in net.last_shuffle] == [n <= M for n in lengths]
    assert net.last_mem_count == tuple(min(n, M) for n in lengths)
    net.last_mem_emb
    assert torch.equal(torch.get_rng_state(), after_long)
    # every other way into the selection leaves no count behind
    net.ips_ragged(rc.make_slides(conf, (M + 1, 2 * M)))
    assert net.last_mem_count is None
    net.ips_ragged(slides, pad=True)
    net.ips(slides[0][None])
    assert net.last_mem_count is None
    net.ips_ragged(slides, pad=True)
    net.ips(slides[1][None])                        # the M >= N shortcut
    assert net.last_mem_count is None and net.last_mem_emb is None
    net.ips_ragged(slides, pad=True)
    stream = net.ips_stream()
    stream.feed(slides[2][None])
    stream.finish()
    assert net.last_mem_count is None


# ------------------------------------------------------------------ refusals
def test_refusals_under_pad_before_anything_runs(monkeypatch):
    conf = rc.feature_conf(M=M, use_pos=True, shuffle=True, shuffle_style='instance')
    net = rc.make_net(conf, CPU)
    state = torch.get_rng_state()
    with pytest.raises(ValueError, match="slide 1"):
        net.ips_ragged([torch.zeros(5, conf.n_chan_in), torch.zeros(0, conf.n_chan_in)], pad=True)      # an empty slide
    with pytest.raises(ValueError, match="slide 0"):
        net.ips_ragged(rc.make_slides(conf, (conf.N + 1, 5)), pad=True)                                  # use_pos with N_b > conf.N
    with pytest.raises(ValueError, match="slide 1"):
        net.ips_ragged(rc.make_slides(conf, (5, 20, conf.N)), pad=True)       # 'instance' with positions on a LONG slide != conf.N
    with pytest.raises(TypeError, match="uint8"):
        net.ips_ragged([s.to(torch.uint8) for s in rc.make_slides(conf, (5, conf.N))], pad=True)
    with pytest.raises(ValueError, match="empty"):
        net.ips_ragged([], pad=True)
    with pytest.raises(ValueError, match="empty"):
        net.ips(Ragged(torch.zeros(0, conf.n_chan_in), (), pad=True))
    monkeypatch.setenv("IPSX_DEDUP_BLANK", "1")
    with pytest.raises(TypeError, match="IPSX_DEDUP_BLANK"):
        net.ips_ragged(rc.make_slides(conf, (5, conf.N)), pad=True)
    monkeypatch.delenv("IPSX_DEDUP_BLANK")
    assert torch.equal(torch.get_rng_state(), state)
    net.ips_ragged(rc.make_slides(conf, (5, conf.N, M)), pad=True)            # short slides are never shuffled: not refused
    assert [s is None for s in net.last_shuffle] == [True, False, True]


def test_without_pad_the_refusals_are_todays():
    conf = rc.feature_conf(M=M, use_pos=True)
    net = rc.make_net(conf, CPU)
    state = torch.get_rng_state()
    for arg in ({}, {"pad": False}):
        with pytest.raises(ValueError, match="slide 1 has 16 rows and the memory M = 16"):
            net.ips_ragged(rc.make_slides(conf, (20, 16)), **arg)
    with pytest.raises(ValueError, match="slide 1 has 16 rows"):
        net.ips(Ragged.from_list(rc.make_slides(conf, (20, 16))))
    with pytest.raises(ValueError, match="slide 0"):
        net.ips_ragged(rc.make_slides(conf, (conf.N + 1, 20)))
    assert torch.equal(torch.get_rng_state(), state)


# ------------------------------------------------------------------ the flag
def test_the_flag_travels_with_the_container(nets):
    conf, net = nets("feature", False, "batch", False)
    slides = rc.make_slides(conf, (20, 5))
    r = Ragged.from_list(slides, pad=True)
    assert r.pad and not Ragged.from_list(slides).pad and not Ragged(r.rows, r.lengths).pad and Ragged(r.rows, r.lengths, pad=True).pad
    assert r.to(torch.float64).pad and r.to(CPU).pad and "pad=True" in repr(r)
    if torch.cuda.is_available():
        assert r.pin_memory().pad
    else:
        moved = r._like(r.rows.clone())             # (what to() and pin_memory() build their result with)
        assert moved.pad and moved is not r
    p, _ = net.ips(r)
    assert tuple(p.shape) == (2, M, conf.n_chan_in) and net.last_mem_count == (M, 5)
    with pytest.raises(ValueError, match="slide 1"):
        net.ips(Ragged.from_list(slides))           # without the flag: refused as ever
    samples = [{'input': s, 'metastases': torch.tensor(k % 2)} for k, s in enumerate(slides)]
    out = collate_ragged_padded(samples)
    assert isinstance(out['input'], Ragged) and out['input'].pad and out['input'].lengths == (20, 5)
    assert out['metastases'].tolist() == [0, 1] and not collate_ragged(samples)['input'].pad
    net.ips(out['input'])
    assert net.last_mem_count == (M, 5)


# ------------------------------------------------------------------ evaluate() against the reference's record
@pytest.mark.parametrize("name", ["feature", "image"])
@pytest.mark.parametrize("reuse", [True, False])
def test_evaluate_over_padded_batches_reproduces_the_reference(name, reuse):
    """The reference's ``evaluate`` on a B = 4, B_seq = 1 loader of slides of 40, 16, 7, 33, 17 and 1 rows against ours on
    ``DataLoader(items, batch_size=4, collate_fn=collate_ragged_padded)``: 1e-6, the tolerance tests/test_loops_golden.py
    holds ``evaluate`` before any training step to on the CPU."""
    z = np.load(pc.GOLDEN, allow_pickle=False)
    conf, net, items, crit = pc.fixture_case(z, name, "cpu")
    if not reuse:
        class NoReuse(type(net)):
            last_mem_emb = property(lambda self: None)
        net.__class__ = NoReuse
    torch.manual_seed(int(z[name + "_torch_seed"]))
    rec = pc.Recorder()
    loops.evaluate(net, crit, DataLoader(items, batch_size=4, collate_fn=collate_ragged_padded), CPU, rec, conf)
    pc.check_fixture(z, name, rec, conf, 1e-6)
