"""``shuffle.draw_shuffle`` draws the permutation ``shuffle_batch`` / ``shuffle_instance`` would apply - the same calls on
the same generators - without applying it: indexing with it gives their result, and the RNG state afterwards is theirs."""

import pytest
import torch

from ips_amd.shuffle import draw_shuffle, shuffle_batch, shuffle_instance

SHAPES = [(3, 37, 16), (2, 23, 1, 4, 5)]


@pytest.mark.parametrize("shape", SHAPES)
def test_batch_draw_then_index_is_shuffle_batch(shape):
    x = torch.arange(float(torch.Size(shape).numel())).reshape(shape)
    torch.manual_seed(11)
    want, want_perm = shuffle_batch(x)
    want_state = torch.get_rng_state()
    torch.manual_seed(11)
    perm = draw_shuffle(x, 'batch')
    assert torch.equal(torch.get_rng_state(), want_state)
    assert perm.shape == (shape[1],) and perm.dtype == torch.int64 and torch.equal(perm, want_perm)
    assert torch.equal(x[:, perm], want)
    assert torch.equal(shuffle_batch(x, perm)[0], want)


@pytest.mark.parametrize("shape", SHAPES)
def test_instance_draw_then_index_is_shuffle_instance(shape):
    x = torch.arange(float(torch.Size(shape).numel())).reshape(shape)
    torch.manual_seed(12)
    want, want_perm = shuffle_instance(x, 1)
    want_state = torch.get_rng_state()
    torch.manual_seed(12)
    perm = draw_shuffle(x, 'instance')
    assert torch.equal(torch.get_rng_state(), want_state)
    assert perm.shape == shape[:2] and perm.dtype == torch.int64 and torch.equal(perm, want_perm)
    got = torch.stack([x[b, perm[b]] for b in range(shape[0])])
    assert torch.equal(got, want)
    assert torch.equal(shuffle_instance(x, 1, perm)[0], want)
    assert all(sorted(perm[b].tolist()) == list(range(shape[1])) for b in range(shape[0]))


def test_an_unknown_style_draws_nothing():
    x = torch.zeros((2, 5, 3))
    state = torch.get_rng_state()
    assert draw_shuffle(x, 'none') is None
    assert torch.equal(torch.get_rng_state(), state)


def test_cpu_net_keeps_the_permutation_of_a_shuffled_call():
    """``last_shuffle`` on the copy path (a CPU net): ``patches[b, last_shuffle[b, last_mem_idx[b]]] == mem_patch[b]``, and the
    call's results and RNG use are those of ``do_shuffle``."""
    from ips_amd import synth
    from ips_amd.architecture import IPSNet
    cpu = torch.device("cpu")
    for style in ('batch', 'instance'):
        conf = synth.camelyon_conf(N=40, M=8, I=8, n_chan_in=32, D=64, D_k=8, D_v=8, D_inner=64, shuffle=True, shuffle_style=style)
        net = synth.fill_weights(IPSNet(cpu, conf), 3).eval()
        x = synth.make_patches(conf, 2, seed=5)
        torch.manual_seed(3)
        mem_patch, _ = net.ips(x)
        state = torch.get_rng_state()
        order = net.last_shuffle
        assert order.shape == ((1, 40) if style == 'batch' else (2, 40)) and order.dtype == torch.int64
        src = torch.gather(order.expand(2, -1), 1, net.last_mem_idx)
        for b in range(2):
            assert torch.equal(x[b, src[b]], mem_patch[b])
        # the same call through do_shuffle itself (a subclass that merely forwards counts as an override)
        class Sub(IPSNet):
            def do_shuffle(self, patches, pos_enc):
                return super().do_shuffle(patches, pos_enc)
        ref = synth.fill_weights(Sub(cpu, conf), 3).eval()
        torch.manual_seed(3)
        want_patch, _ = ref.ips(x)
        assert ref.last_shuffle is None
        assert torch.equal(torch.get_rng_state(), state)
        assert torch.equal(want_patch, mem_patch) and torch.equal(ref.last_mem_idx, net.last_mem_idx)
