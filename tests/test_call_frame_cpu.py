"""The call frame every way into the selection shares (``IPSNet._scoring``, ``IPSNet._iterate``, ``IPSNet.plan``), without a
GPU: the modes of the encoder and the transformer during and after a call of every entry point, one iteration of the ATen
loop through its three callers, and the encoder plan built once."""

import pytest
import torch
import torch.distributed as torch_dist

from ips_amd import dist, hip, synth
from ips_amd.architecture import IPSNet

PATCH, STRIDE = (32, 32), (16, 16)
B, M, I = 2, 4, 3


def image_net():
    """1 x 64 x 96 images in 32 x 32 patches every 16 pixels: N = 3 * 5 = 15 = M + 3 I + 2, a ragged last chunk."""
    conf = synth.mnist_conf(N=15, M=M, I=I)
    return synth.fill_weights(IPSNet(torch.device("cpu"), conf), 5)


def feature_net(use_pos):
    """N = M + 2 I + 1 feature rows: chunks [0, 4) [4, 7) [7, 10) [10, 11), a ragged last one -> (net, its configuration)."""
    conf = synth.camelyon_conf(N=M + 2 * I + 1, M=M, I=I, n_chan_in=16, D=32, H=4, D_k=8, D_v=8, D_inner=64, use_pos=use_pos)
    return synth.fill_weights(IPSNet(torch.device("cpu"), conf), 6).eval(), conf


@pytest.fixture(scope="module")
def images():
    return torch.randn((B, 1, 64, 96), generator=torch.Generator().manual_seed(3))


@pytest.fixture(scope="module")
def one_rank(tmp_path_factory):
    """A gloo group of one rank in this process (``ips_tournament``: the slab is the whole patch axis)."""
    store = tmp_path_factory.mktemp("gloo") / "store"
    torch_dist.init_process_group("gloo", init_method="file://{}".format(store), rank=0, world_size=1)
    yield
    torch_dist.destroy_process_group()


# ------------------------------------------------------------------ 1. the frame's rule
def run_ips(net, images):
    net.ips(IPSNet._unfold_images(images, PATCH, STRIDE).contiguous())


def run_ips_image(net, images):
    net.ips_image(images, PATCH, STRIDE)


def run_stream(net, images):
    """``feed`` and ``finish``: pieces of 7, 6 and 2 patches - iterations in both feeds that complete a chunk and, the
    ragged last one, in ``finish``; between the calls the net is as it was handed in."""
    modes = (net.encoder.training, net.transf.training)
    patches = IPSNet._unfold_images(images, PATCH, STRIDE)
    s = net.ips_stream()
    for lo, hi in ((0, 7), (7, 13), (13, 15)):
        s.feed(patches[:, lo:hi])
        assert (net.encoder.training, net.transf.training) == tuple(m or net.training for m in modes)
    s.finish()
    assert s.iterations == 4


def run_rows(net, images):
    """``feed_rows``: bands that complete no patch row (nothing runs), one and two of them; the last chunk in ``finish``."""
    s = net.ips_stream(PATCH, STRIDE)
    for lo, hi in ((0, 20), (20, 33), (33, 64)):
        s.feed_rows(images[:, :, lo:hi])
    s.finish()
    assert s.iterations == 4


def run_tournament(net, images):
    dist.ips_tournament(net, IPSNet._unfold_images(images, PATCH, STRIDE).contiguous(), 15)


ENTRIES = {"ips": run_ips, "ips_image": run_ips_image, "stream": run_stream, "feed_rows": run_rows, "tournament": run_tournament}


@pytest.fixture(params=list(ENTRIES))
def entry(request):
    if request.param == "tournament":
        request.getfixturevalue("one_rank")
    return ENTRIES[request.param]


def spy_on_scoring(net, monkeypatch):
    """Every ``score_and_select`` of a call notes the modes it runs in (every entry point scores through it on the CPU)."""
    seen, inner = [], net.score_and_select

    def spy(*args):
        seen.append((net.encoder.training, net.transf.training))
        return inner(*args)
    monkeypatch.setattr(net, "score_and_select", spy)
    return seen


def test_a_training_net_scores_in_eval_mode_and_comes_back_in_train_mode(entry, images, monkeypatch):
    net = image_net().train()
    seen = spy_on_scoring(net, monkeypatch)
    entry(net, images)
    assert len(seen) >= 4 and set(seen) == {(False, False)}
    assert net.training and net.encoder.training and net.transf.training
    assert all(m.training for m in net.modules())


def test_a_net_in_eval_mode_is_left_alone(entry, images, monkeypatch):
    net = image_net().eval()
    seen = spy_on_scoring(net, monkeypatch)
    entry(net, images)
    assert len(seen) >= 4 and set(seen) == {(False, False)}
    assert not any(m.training for m in net.modules())


def test_an_eval_net_with_a_training_encoder_keeps_both(entry, images, monkeypatch):
    """The frame is keyed on the NET's mode: a net in eval mode whose encoder was put back into train mode scores with that
    encoder as it is, and nothing is touched."""
    net = image_net().eval()
    net.encoder.train()
    seen = spy_on_scoring(net, monkeypatch)
    entry(net, images)
    assert set(seen) == {(True, False)}
    assert net.encoder.training and not net.transf.training and not net.training


def test_a_training_net_with_an_eval_encoder_comes_back_as_the_parent_leaves_it(entry, images, monkeypatch):
    """A net in train mode whose encoder alone was put into eval mode.  The parent's answer (every one of its seven
    frames: ``if was_training: encoder.train(); transf.train()``): the call scores in eval mode and BOTH modules come
    back in train mode - the encoder's own eval mode is not remembered."""
    net = image_net().train()
    net.encoder.eval()
    seen = spy_on_scoring(net, monkeypatch)
    entry(net, images)
    assert set(seen) == {(False, False)}
    assert net.training and net.encoder.training and net.transf.training


class Boom(Exception):
    pass


def test_the_modes_are_restored_after_an_exception(entry, images, monkeypatch):
    """``_select_aten`` raises inside ``ips`` / ``ips_image`` / ``ips_tournament``; the streams never call it: their
    iterations raise in ``score_and_select``."""
    def boom(*args, **kwargs):
        raise Boom()
    for mode in (True, False):
        net = image_net().train(mode)
        monkeypatch.setattr(net, "_select_aten", boom)
        if entry in (run_stream, run_rows):
            monkeypatch.setattr(net, "score_and_select", boom)
        with pytest.raises(Boom):
            entry(net, images)
        assert net.training == mode and net.encoder.training == mode and net.transf.training == mode


# ------------------------------------------------------------------ 2. one iteration, three callers
@pytest.mark.parametrize("use_pos", [False, True])
def test_the_three_aten_loops_select_the_same_patches(use_pos):
    net, conf = feature_net(use_pos)
    N = conf.N
    x = synth.make_patches(conf, B, seed=8)
    assert x.shape == (B, N, 16)
    with torch.no_grad():
        pos = net.pos_enc.expand(B, -1, -1) if use_pos else None
        want = net._select_aten(x, pos)
        emb = net._embed(x.reshape(B * N, -1)).view(B, N, -1)
        sharded = dist._scan_aten(net, emb)
    s = net.ips_stream()
    for j in range(N):                  # one row per feed
        s.feed(x[:, j:j + 1])
    s.finish()
    assert want.shape == (B, M) and want.dtype == torch.int64 and len({int(v) for v in want[0]}) == M
    assert torch.equal(sharded, want)
    assert torch.equal(net.last_mem_idx, want) and s.iterations == 3


# ------------------------------------------------------------------ 3. the plan
def test_the_plan_is_built_once_and_kept_in_its_attribute(monkeypatch):
    built = []

    class FakePlan:
        def __init__(self, encoder, is_image):
            built.append((encoder, is_image))
    monkeypatch.setattr(hip, "EncoderPlan", FakePlan)
    net = image_net()
    assert net._plan is None and not built
    plan = net.plan
    assert isinstance(plan, FakePlan) and plan is net._plan
    assert net.plan is plan and net.selection.plan() is plan and net.plan is net._plan
    assert built == [(net.encoder, True)]
    net._plan = other = FakePlan(net.encoder, True)         # (the attribute remains the one place the plan is kept)
    assert net.plan is other and net.selection.plan() is other
