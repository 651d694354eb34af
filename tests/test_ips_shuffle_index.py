"""``IPSNet.ips`` with ``shuffle=True`` on device-resident patches selects through a permutation INDEX instead of a permuted
copy of the patch tensor (``IPSX_SHUFFLE=index``, the default; ``copy`` = the previous behaviour).  Under the same
``torch.manual_seed`` both leave the same bits - selected patches, positional rows, indices (in shuffled numbering),
embeddings - and the same RNG state, on every feature schedule and on the fused trunk; the index path allocates no
tensor the size of the input."""

import pytest
import torch

from ips_amd import synth
from ips_amd.architecture import IPSNet

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# the schedules of the feature pipeline (tests/test_hip_e2e.py::test_every_variant_of_the_feature_pipeline...), and the
# bf16 projector on float16 rows
VARIANTS = (("default", {}, False),
            ("the entry points one by one instead of ONE library call", {"IPSX_NATIVE_CALL": "0"}, False),
            ("per-part launches", {"IPSX_SCAN_PERSIST": "0"}, False),
            ("after", {"IPSX_OVERLAP_SCAN": "0"}, False),
            ("launch by launch beside the persistent loop", {"IPSX_CAM_STREAM": "0"}, False),
            ("latency-shaped parts", {"IPSX_CAM_PARTS": "latency", "IPSX_CAM_STREAM": "0"}, False),
            ("bf16 projector, float16 rows", {"IPSX_PRECISION": "bf16"}, True),
            ("bf16 projector, float16 rows, launch by launch", {"IPSX_PRECISION": "bf16", "IPSX_CAM_STREAM": "0"}, True),
            ("bf16 projector, float16 rows, per-part launches", {"IPSX_PRECISION": "bf16", "IPSX_SCAN_PERSIST": "0"}, True),
            ("bf16 projector, float16 rows, after", {"IPSX_PRECISION": "bf16", "IPSX_OVERLAP_SCAN": "0"}, True))


def feature_net(N, style, use_pos, f=64, M=32, I=32):
    conf = synth.camelyon_conf(N=N, M=M, I=I, n_chan_in=f, use_pos=use_pos, shuffle=True, shuffle_style=style)
    return conf, synth.fill_weights(IPSNet(DEV, conf), 7).to(DEV).eval()


def shuffled_call(net, x, mode, seed, monkeypatch):
    """One seeded ips() call under IPSX_SHUFFLE=mode -> everything the two modes must agree on."""
    monkeypatch.setenv("IPSX_SHUFFLE", mode)
    before = net.selection.index_calls
    torch.manual_seed(seed)
    mem_patch, mem_pos = net.ips(x)
    emb = net.last_mem_emb
    torch.cuda.synchronize()
    out = dict(patch=mem_patch.clone(), pos=None if mem_pos is None else mem_pos.clone(), idx=net.last_mem_idx.clone(),
               emb=emb.clone(), order=net.last_shuffle.clone(), cpu_rng=torch.get_rng_state(), dev_rng=torch.cuda.get_rng_state(DEV),
               by_index=net.selection.index_calls - before)
    monkeypatch.delenv("IPSX_SHUFFLE")
    return out


def assert_same(got, want, x, what):
    assert torch.equal(got["idx"], want["idx"]), what
    assert torch.equal(got["patch"], want["patch"]), what
    assert (got["pos"] is None) == (want["pos"] is None) and (got["pos"] is None or torch.equal(got["pos"], want["pos"])), what
    assert torch.equal(got["emb"], want["emb"]), what
    assert torch.equal(got["cpu_rng"], want["cpu_rng"]) and torch.equal(got["dev_rng"], want["dev_rng"]), what
    assert torch.equal(got["order"].cpu(), want["order"].cpu()), what
    for r in (got, want):                      # patches[b, last_shuffle[b, last_mem_idx[b]]] == mem_patch[b], on both paths
        B = x.shape[0]
        src = torch.gather(r["order"].to(DEV).expand(B, -1), 1, r["idx"])
        for b in range(B):
            assert torch.equal(x[b, src[b]], r["patch"][b]), what


@pytest.mark.parametrize("use_pos", [False, True])
@pytest.mark.parametrize("style", ["batch", "instance"])
@pytest.mark.parametrize("B,N", [(1, 300), (3, 320)])
def test_index_and_copy_leave_the_same_bits_on_every_feature_schedule(B, N, style, use_pos, monkeypatch):
    conf, net = feature_net(N, style, use_pos)
    x32 = synth.make_patches(conf, B, seed=3).to(DEV)
    for name, env, half in VARIANTS:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        x = x32.half() if half else x32
        want = shuffled_call(net, x, "copy", 5, monkeypatch)
        got = shuffled_call(net, x, "index", 5, monkeypatch)
        again = shuffled_call(net, x, "index", 6, monkeypatch)              # (cached buffers; another permutation)
        assert want["by_index"] == 0 and got["by_index"] == 1 and again["by_index"] == 1, name
        assert_same(got, want, x, name)
        assert_same(again, shuffled_call(net, x, "copy", 6, monkeypatch), x, name)
        assert not torch.equal(again["order"].cpu(), got["order"].cpu())
        for k in env:
            monkeypatch.delenv(k)


@pytest.mark.parametrize("style", ["batch", "instance"])
@pytest.mark.parametrize("B,takes_index", [(4, False), (16, True)])
def test_fused_trunk_selects_the_same_through_the_index(B, takes_index, style, monkeypatch):
    """The MNIST benchmark net on (B, 2500, 1, 32, 32) random patches.  16 images - the headline's shape - go through the
    fused trunk's index lists, into which the shuffle is composed; 4 images are a small batch, encoded in one piece,
    which keeps the copy: the same bits either way."""
    conf, _ = synth.bench_workload("mnist")
    conf = conf.clone(shuffle=True, shuffle_style=style)
    net = synth.fill_weights(IPSNet(DEV, conf), 7).to(DEV).eval()
    g = torch.Generator().manual_seed(8)
    x = torch.rand((B, 2500, 1, 32, 32), generator=g).to(DEV)
    want = shuffled_call(net, x, "copy", 9, monkeypatch)
    got = shuffled_call(net, x, "index", 9, monkeypatch)
    assert want["by_index"] == 0 and got["by_index"] == int(takes_index)
    assert_same(got, want, x, style)


def test_an_overridden_do_shuffle_is_still_called(monkeypatch):
    conf, net = feature_net(300, "instance", False)
    x = synth.make_patches(conf, 2, seed=4).to(DEV)
    calls = []
    inner = net.do_shuffle

    def spy(patches, pos_enc):
        calls.append(tuple(patches.shape))
        return inner(patches, pos_enc)

    net.do_shuffle = spy
    before = net.selection.index_calls
    torch.manual_seed(2)
    mem_patch, _ = net.ips(x)
    assert calls == [tuple(x.shape)] and net.selection.index_calls == before and net.last_shuffle is None
    del net.do_shuffle
    torch.manual_seed(2)
    again, _ = net.ips(x)
    assert net.selection.index_calls == before + 1 and torch.equal(again, mem_patch)


def test_host_patches_and_the_copy_switch_do_not_take_the_index(monkeypatch):
    conf, net = feature_net(300, "batch", False)
    x = synth.make_patches(conf, 2, seed=4)
    sel = net.selection
    torch.manual_seed(2)
    lazy, _ = net.ips(x)                                    # host-resident (lazy loading): shuffled by copy on the host
    assert sel.index_calls == 0 and net.last_shuffle is not None and not net.last_shuffle.is_cuda
    monkeypatch.setenv("IPSX_SHUFFLE", "copy")
    torch.manual_seed(2)
    copied, _ = net.ips(x.to(DEV))
    assert sel.index_calls == 0
    monkeypatch.delenv("IPSX_SHUFFLE")
    torch.manual_seed(2)
    indexed, _ = net.ips(x.to(DEV))
    assert sel.index_calls == 1
    assert torch.equal(indexed, copied) and torch.equal(indexed, lazy)
    assert not sel.index_supported(x) and sel.index_supported(x.to(DEV)) and not sel.index_supported(x.to(DEV)[:, ::2])


def test_a_shuffled_call_allocates_no_copy_of_the_input():
    """(1, 2048, 2048) fp32 = 16 MiB: one warm shuffled ips() raises the peak of allocated memory by less than half the
    input's bytes (the shuffled copy alone is 1.0 x; what a warm call does allocate - 32 gathered rows, the permutation,
    indices - is three orders of magnitude smaller)."""
    conf, net = feature_net(2048, "batch", False, f=2048)
    x = synth.make_patches(conf, 1, seed=6).to(DEV)
    nbytes = x.numel() * x.element_size()
    assert nbytes == 16 << 20
    torch.manual_seed(1)
    net.ips(x)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.max_memory_allocated(DEV)
    torch.manual_seed(2)
    mem_patch, _ = net.ips(x)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated(DEV) - base
    print("peak above the warm state: %d bytes of an input of %d" % (rise, nbytes))
    assert net.selection.index_calls == 2
    assert rise < nbytes // 2, (rise, nbytes)
    assert torch.equal(mem_patch[0], x[0, net.last_shuffle[0, net.last_mem_idx[0]]])
