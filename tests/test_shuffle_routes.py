"""``shuffle: True`` without the copy on the one-call and one-image routes: ``ipsx_order_index`` and
``ipsx_trunk_stream_indexed`` on their own, then ``IPSNet.ips`` - feature slides through the ordered one call
(``ipsx_ips_call_run_ordered``), one image on the fused trunk stream, layer-by-layer trunks in one piece - under
``IPSX_SHUFFLE=index`` against ``copy``: the same bits in everything a call returns and leaves behind, the same RNG state,
on the route the same call takes at ``shuffle=False``, and no tensor of the input's size."""

import pytest
import torch

from ips_amd import hip, quant, synth
from ips_amd.architecture import IPSNet
from tests.util import Golden

from ips_amd import selection

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(autouse=True)
def ordered_native_route(monkeypatch):
    """The ordered one call is what these tests are about: where it ships behind ``IPSX_NATIVE_ORDER=1`` they set it."""
    if selection.NATIVE_ORDER_DEFAULT != "1":
        monkeypatch.setenv("IPSX_NATIVE_ORDER", "1")


# ---------------------------------------------------------------------------------------------- helpers
def shuffled_call(net, x, mode, seed, monkeypatch):
    """One seeded ips() call under IPSX_SHUFFLE=mode -> everything the two modes must agree on, and what the counters did."""
    monkeypatch.setenv("IPSX_SHUFFLE", mode)
    sel = net.selection
    before = (sel.index_calls, sel.native_calls, sel.native_ordered_calls, hip._PERSIST_CALLS)
    torch.manual_seed(seed)
    mem_patch, mem_pos = net.ips(x)
    emb = net.last_mem_emb
    torch.cuda.synchronize()
    out = dict(patch=mem_patch.clone(), pos=None if mem_pos is None else mem_pos.clone(), idx=net.last_mem_idx.clone(),
               emb=emb.clone(), order=net.last_shuffle.clone(), cpu_rng=torch.get_rng_state(), dev_rng=torch.cuda.get_rng_state(DEV),
               by_index=sel.index_calls - before[0], native=sel.native_calls - before[1],
               ordered=sel.native_ordered_calls - before[2], persist=hip._PERSIST_CALLS - before[3])
    monkeypatch.delenv("IPSX_SHUFFLE")
    return out


def assert_same(got, want, x, what):
    """``x``: the float32 patches the call selected from (uint8 input: its expansion)."""
    assert torch.equal(got["idx"], want["idx"]), what
    assert got["patch"].dtype == want["patch"].dtype and torch.equal(got["patch"], want["patch"]), what
    assert (got["pos"] is None) == (want["pos"] is None) and (got["pos"] is None or torch.equal(got["pos"], want["pos"])), what
    assert torch.equal(got["emb"], want["emb"]), what
    assert torch.equal(got["cpu_rng"], want["cpu_rng"]) and torch.equal(got["dev_rng"], want["dev_rng"]), what
    assert torch.equal(got["order"].cpu(), want["order"].cpu()), what
    for r in (got, want):                      # patches[b, last_shuffle[b, last_mem_idx[b]]] == mem_patch[b], on both paths
        B = x.shape[0]
        src = torch.gather(r["order"].to(DEV).expand(B, -1), 1, r["idx"])
        for b in range(B):
            assert torch.equal(x[b, src[b]], r["patch"][b]), what


class Env:
    """Environment switches for a block of calls."""

    def __init__(self, monkeypatch, env):
        self.mp, self.env = monkeypatch, env

    def __enter__(self):
        for k, v in self.env.items():
            self.mp.setenv(k, v)

    def __exit__(self, *exc):
        for k in self.env:
            self.mp.delenv(k)


def plain_native_calls(net, x):
    """How many library-enqueued calls the same ``ips(x)`` makes at ``shuffle=False`` (0 or 1): the route a shuffled call
    through the index must stay on."""
    net.shuffle = False
    before = net.selection.native_calls
    net.ips(x)
    torch.cuda.synchronize()
    net.shuffle = True
    return net.selection.native_calls - before


def feature_net(N, style, f=64, M=32, I=32):
    conf = synth.camelyon_conf(N=N, M=M, I=I, n_chan_in=f, use_pos=False, shuffle=True, shuffle_style=style)
    return conf, synth.fill_weights(IPSNet(DEV, conf), 7).to(DEV).eval()


# ---------------------------------------------------------------------------------------------- 1. ipsx_order_index
@pytest.mark.parametrize("B,N,shared", [(1, 1, True), (1, 37, True), (3, 321, False), (16, 2500, True)])
def test_order_index_is_the_flat_row_numbers_and_clamps(B, N, shared):
    g = torch.Generator().manual_seed(B * 1000 + N)
    order = torch.stack([torch.randperm(N, generator=g) for _ in range(1 if shared else B)]).to(DEV)
    want = (order.expand(B, -1) + torch.arange(B, device=DEV)[:, None] * N).int()
    sentinel = -0x5A5A5A5A
    guarded = torch.full((B * N + 16,), sentinel, dtype=torch.int32, device=DEV)
    out = hip.order_index(order, B, N, out=guarded[8:-8])
    torch.cuda.synchronize()
    assert out.shape == (B, N) and out.dtype == torch.int32 and torch.equal(out, want)
    assert bool((guarded[:8] == sentinel).all()) and bool((guarded[-8:] == sentinel).all())
    assert torch.equal(hip.order_index(order, B, N), want)                   # (an output of its own)
    # entries outside [0, N): each lands inside its own image's rows
    bad = order.clone()
    flat = bad.view(-1)
    for k, v in enumerate((-1, N, 2 ** 40)):
        flat[(k * 7) % flat.numel()] = v
        flat[flat.numel() - 1 - (k * 5) % flat.numel()] = v
    out = hip.order_index(bad, B, N, out=guarded[8:-8])
    torch.cuda.synchronize()
    rows = torch.arange(B, device=DEV)[:, None] * N
    assert bool((out >= rows).all()) and bool((out < rows + N).all())
    ok = ((bad >= 0) & (bad < N)).expand(B, -1)
    assert torch.equal(out[ok], want[ok])                                    # (the good entries are untouched)
    assert bool((guarded[:8] == sentinel).all()) and bool((guarded[-8:] == sentinel).all())


# ---------------------------------------------------------------------------------------------- 2. ipsx_trunk_stream_indexed
@pytest.fixture(scope="module")
def stream_plan():
    net = Golden("mnist_full").net(DEV)
    ca = net.transf.crs_attn
    return net, hip.EncoderPlan(net.encoder, True), ca.folded_query(), ca.H * ca.n_token


@pytest.mark.parametrize("n,wgs,use_pos,quads", [(1, 0, True, -1), (2, 3, False, 0), (77, 5, True, 2), (79, 5, True, 100),
                                                 (2501, 0, True, 1)])
def test_trunk_stream_indexed_equals_the_stream_on_the_gathered_patches(stream_plan, n, wgs, use_pos, quads):
    """The producer alone (no loop, nothing waits): patch j of the stream is patch index[j] of a source of n + 5 patches,
    five of which - 1e30 throughout, at both ends of the tensor - no index names."""
    net, plan, vq, R = stream_plan
    gen = torch.Generator().manual_seed(n)
    x = torch.randn((n + 5, 1, 32, 32), generator=gen)
    x[torch.rand(n + 5, generator=gen) < 0.5] = 0.0
    unnamed = torch.tensor([0, 1, 2, n + 3, n + 4])
    x[unnamed] = 1e30
    x = x.to(DEV)
    named = torch.arange(3, n + 3)
    pos = torch.randn((n, 128), generator=gen).to(DEV) if use_pos else None
    assert plan.image_stream_supported(x.shape, 128, R)
    for what, index in (("a permutation", named[torch.randperm(n, generator=gen)]),
                        ("an index with repeats", named[torch.randint(0, n, (n,), generator=gen)])):
        index = index.int().to(DEV)
        want_emb = plan.encode(x[index.long()])
        want_lg = hip.logits(want_emb.view(1, n, -1), pos.view(1, n, -1) if use_pos else None, vq, R)[0]
        assert bool(torch.isfinite(want_emb).all()) and float(want_emb.abs().max()) < 1e20
        emb = torch.full_like(want_emb, float("nan"))
        lg = torch.full_like(want_lg, float("nan"))
        for rep in range(2):
            ctl = torch.zeros((plan.image_stream_ctl_words(n),), dtype=torch.int32, device=DEV)
            ready = torch.zeros((1,), dtype=torch.int32, device=DEV)
            plan.image_stream(x, pos, vq, R, emb, lg, ctl, ready, workgroups=wgs, quad_pulls=quads, index=index)
            torch.cuda.synchronize()
            assert int(ready.item()) == n, what
            assert torch.equal(emb, want_emb), what
            assert torch.equal(lg, want_lg), what


# ---------------------------------------------------------------------------------------------- 3. + 8. feature slides
@pytest.mark.parametrize("style", ["batch", "instance"])
@pytest.mark.parametrize("B,N", [(1, 300), (3, 320)])
def test_feature_slides_go_through_the_ordered_one_call(B, N, style, monkeypatch):
    """... and the discipline of the persistent loop holds for it: every call is counted (``hip._PERSIST_CALLS``, the
    window of ``hip.persistent_timed_out``), ``check_strike`` reads the mirror the ordered call wrote - cleared by hand, it
    holds the loop's status word again after the next ordered call and a sync: bit 1 (the loop was resident) and not
    bit 0 (it gave up waiting), i.e. 2, of which ``check_strike`` reads bit 0.  No loop gave up, ``hip.persistent_timed_out``
    was not called, the persistent pipelines are on."""
    conf, net = feature_net(N, style)
    x = synth.make_patches(conf, B, seed=3).to(DEV)
    sel = net.selection
    assert sel.native_calls == 0 and sel.native_ordered_calls == 0
    strikes = hip._PERSIST_STRIKES
    want = shuffled_call(net, x, "copy", 5, monkeypatch)
    got = shuffled_call(net, x, "index", 5, monkeypatch)
    again = shuffled_call(net, x, "index", 6, monkeypatch)                   # (cached buffers; another permutation)
    assert (want["by_index"], want["native"], want["ordered"]) == (0, 1, 0)
    for r in (got, again):
        assert (r["by_index"], r["native"], r["ordered"], r["persist"]) == (1, 1, 1, 1)
    assert sel._flat_made is None                                            # (the library composed the index, not the host)
    assert_same(got, want, x, "index against copy")
    assert_same(again, shuffled_call(net, x, "copy", 6, monkeypatch), x, "another seed")
    assert not torch.equal(again["order"].cpu(), got["order"].cpu())
    assert got["order"].is_cuda                                              # last_shuffle: the device tensor through the index
    # the status mirror check_strike reads is the one the ordered call wrote
    assert sel.scan_status_host is sel.status_mirror() and sel.status_mirror().is_pinned()
    assert sel._calls["features"][1].status_host == sel.status_mirror().data_ptr()
    assert int(sel.status_mirror().item()) & 1 == 0
    sel.status_mirror().zero_()
    shuffled_call(net, x, "index", 7, monkeypatch)
    assert int(sel.status_mirror().item()) == 2
    assert hip._PERSIST_STRIKES == strikes and hip._PERSIST_OFF is None and hip.persistent_ok(DEV)
    with Env(monkeypatch, {"IPSX_NATIVE_CALL": "0"}):
        one_by_one = shuffled_call(net, x, "index", 5, monkeypatch)
    assert (one_by_one["by_index"], one_by_one["native"], one_by_one["ordered"]) == (1, 0, 0)
    assert_same(one_by_one, want, x, "IPSX_NATIVE_CALL=0")
    assert plain_native_calls(net, x) == 1


# ---------------------------------------------------------------------------------------------- 4. beyond the LDS
@pytest.mark.parametrize("B", [1, 2])
def test_feature_slides_beyond_the_lds_through_the_index(B, monkeypatch):
    N, M = 2000, 640
    conf, net = feature_net(N, "batch", M=M, I=M)
    ca = net.transf.crs_attn
    assert hip.scan_workspace(B, M, M, ca.H, ca.n_token, DEV) is not None    # the team loop and its workspace
    x = synth.make_patches(conf, B, seed=4).to(DEV)
    want = shuffled_call(net, x, "copy", 5, monkeypatch)
    got = shuffled_call(net, x, "index", 5, monkeypatch)
    again = shuffled_call(net, x, "index", 6, monkeypatch)
    assert want["by_index"] == 0 and got["by_index"] == 1 and again["by_index"] == 1
    assert_same(got, want, x, "index against copy")
    assert_same(again, shuffled_call(net, x, "copy", 6, monkeypatch), x, "another seed")
    # the route of the same call at shuffle=False
    plain = plain_native_calls(net, x)
    assert got["native"] == plain and got["ordered"] == plain and want["native"] == plain
    if B == 1:
        assert plain == 1


# ---------------------------------------------------------------------------------------------- 5. one image, fused trunk
@pytest.mark.parametrize("style", ["batch", "instance"])
@pytest.mark.parametrize("use_pos", [True, False])
@pytest.mark.parametrize("N", [24, 37, 2501])
def test_one_image_on_the_fused_trunk_streams_through_the_index(N, use_pos, style, monkeypatch):
    conf = synth.mnist_conf(N=N, M=8, I=8, shuffle=True, shuffle_style=style, use_pos=use_pos)
    net = synth.fill_weights(IPSNet(DEV, conf), 7).to(DEV).eval()
    x = torch.rand((1, N, 1, 32, 32), generator=torch.Generator().manual_seed(N)).to(DEV)
    for env, by_index, ordered in (({}, 1, 1), ({"IPSX_NATIVE_CALL": "0"}, 1, 0), ({"IPSX_IMAGE_STREAM": "0"}, None, 0),
                                   ({"IPSX_OVERLAP_SCAN": "0"}, None, 0)):
        with Env(monkeypatch, env):
            want = shuffled_call(net, x, "copy", 11, monkeypatch)
            got = shuffled_call(net, x, "index", 11, monkeypatch)
        assert_same(got, want, x, env)
        assert want["by_index"] == 0 and want["ordered"] == 0, env
        assert got["ordered"] == ordered, env
        if by_index is not None:
            assert got["by_index"] == by_index, env
            assert got["order"].is_cuda, env


# ---------------------------------------------------------------------------------------------- 6. layered trunks in one piece
def layered_net(name, style):
    conf = (synth.mnist_conf(N=36, M=4, I=8, patch=50) if name == "mnist50" else synth.traffic_conf(N=12, M=2, I=4))
    conf = conf.clone(shuffle=True, shuffle_style=style)
    return conf, synth.fill_weights(IPSNet(DEV, conf), 7).to(DEV).eval()


@pytest.mark.parametrize("style", ["batch", "instance"])
@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("name", ["mnist50", "traffic"])
def test_layered_trunks_in_one_piece_read_the_index_list(name, u8, style, monkeypatch):
    conf, net = layered_net(name, style)
    shape = (2, conf.N, conf.n_chan_in) + tuple(conf.patch_size)
    g = torch.Generator().manual_seed(17)
    if u8:
        table = torch.randn((conf.n_chan_in, 256), generator=g)
        assert bool((table[:, 0] != 0).all())
        net.set_patch_table(table.to(DEV))
        q = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)
        q.view(-1, *shape[2:])[1::2] = 0
        q = q.to(DEV)
        x = quant.dequant(q, net.patch_table)
    else:
        q = x = torch.rand(shape, generator=g).to(DEV)
    assert not net.selection.can_overlap(q) and net.selection.index_supported(q)      # one piece; its stem takes the list
    want = shuffled_call(net, q, "copy", 13, monkeypatch)
    got = shuffled_call(net, q, "index", 13, monkeypatch)
    assert want["by_index"] == 0 and got["by_index"] == 1
    assert got["patch"].dtype == torch.float32
    assert_same(got, want, x, (name, u8, style))


# ---------------------------------------------------------------------------------------------- 7. memory
def warm_peak(net, x, mode, seed, monkeypatch):
    """Peak of allocated memory of one WARM call above the state it starts from."""
    monkeypatch.setenv("IPSX_SHUFFLE", mode)
    torch.manual_seed(seed)
    net.ips(x)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.max_memory_allocated(DEV)
    torch.manual_seed(seed + 1)
    out = net.ips(x)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated(DEV) - base
    monkeypatch.delenv("IPSX_SHUFFLE")
    del out
    return rise


def test_a_layered_call_through_the_index_has_no_tensor_of_the_inputs_size(monkeypatch):
    conf = synth.mnist_conf(N=400, M=16, I=64, patch=50, shuffle=True, shuffle_style="batch")
    net = synth.fill_weights(IPSNet(DEV, conf), 7).to(DEV).eval()
    x = torch.rand((4, 400, 1, 50, 50), generator=torch.Generator().manual_seed(2)).to(DEV)
    nbytes = x.numel() * x.element_size()
    assert not net.selection.can_overlap(x)
    by_copy = warm_peak(net, x, "copy", 3, monkeypatch)
    by_index = warm_peak(net, x, "index", 3, monkeypatch)
    print("peak above the warm state: copy %d, index %d bytes; input %d" % (by_copy, by_index, nbytes))
    assert net.selection.index_calls == 2
    assert by_copy - by_index >= 0.9 * nbytes, (by_copy, by_index, nbytes)


def test_one_image_through_the_index_allocates_no_copy_of_the_input(monkeypatch):
    conf = synth.mnist_conf(N=2500, M=64, I=64, shuffle=True, shuffle_style="batch")
    net = synth.fill_weights(IPSNet(DEV, conf), 7).to(DEV).eval()
    x = torch.rand((1, 2500, 1, 32, 32), generator=torch.Generator().manual_seed(2)).to(DEV)
    nbytes = x.numel() * x.element_size()
    rise = warm_peak(net, x, "index", 3, monkeypatch)
    print("peak above the warm state: %d bytes of an input of %d" % (rise, nbytes))
    assert net.selection.index_calls == 2 and net.selection.native_ordered_calls == 2
    assert rise < nbytes // 2, (rise, nbytes)
