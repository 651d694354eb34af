"""``IPSNet.ips_stream()`` on the CPU device: the state machine of ips_amd/stream.py on ATen ops - held to the
reference's recorded memory after EVERY iteration (``trace_idx`` of the fixtures under tests/golden/), to ``ips()`` on the
concatenation for piece sizes that never align with the chunks, and its refusals; the header / binding surface of the two
exports behind the device path, and the argument checks of ``ipsx_stream_commit`` that need no device."""

import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from ips_amd import hip, synth
from ips_amd.architecture import IPSNet
from ips_amd.stream import IPSStream
from tests.stream_cases import piece_patterns
from tests.util import Golden

CASES = ["mnist_mini", "mnist_ragged", "mnist_ties", "mnist_tok1", "cam_b2", "mnist_onechunk"]
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ipsx.h")


def feed_all(net, x, sizes):
    s = net.ips_stream()
    lo = 0
    for n in sizes:
        s.feed(x[:, lo:lo + n])
        lo += n
    assert lo == x.shape[1] and s.fed == lo
    return s


@pytest.fixture(scope="module")
def cases():
    """net (shuffle off), input in the order ips() saw it, and what ips() returns for it - computed once per fixture"""
    out = {}
    for name in CASES:
        g = Golden(name)
        net = g.net("cpu")
        net.shuffle = False
        x = g.shuffled(g.patches())
        mem_patch, mem_pos = net.ips(x)
        out[name] = (g, net, x, (mem_patch, mem_pos, net.last_mem_idx.clone(), net.last_mem_emb.clone()))
    return out


@pytest.mark.parametrize("case", CASES)
def test_memory_after_every_feed_is_the_references(case, cases):
    g, net, x, _ = cases[case]
    # (x is g.shuffled(patches); the reference permutes its positional table with the patches, a stream numbers patches as
    #  they arrive: a fixture with a permutation AND positions would need the table permuted here - none has both)
    assert g.perm is None or not g.conf.use_pos
    M, I, N = net.M, net.I, x.shape[1]
    s = net.ips_stream()
    assert isinstance(s, IPSStream) and s.mem_idx is None and s.fed == 0 and s.iterations == 0
    edges = [0, M] + list(range(M + I, N, I)) + [N]
    for k in range(len(edges) - 1):
        s.feed(x[:, edges[k]:edges[k + 1]])
        assert s.fed == edges[k + 1]
        # feed k completes iteration k unless it is the ragged last chunk, which finish() runs
        assert s.iterations == (edges[k + 1] - M) // I
        if k == 0:
            assert np.array_equal(s.mem_idx.numpy(), np.broadcast_to(np.arange(M), (g.B, M)))
        elif s.iterations == k:
            assert np.array_equal(s.mem_idx.numpy(), g.trace_idx[:, k - 1]), "iteration %d" % k
    mem_patch, mem_pos = s.finish()
    assert s.iterations == g.trace_idx.shape[1]
    assert np.array_equal(net.last_mem_idx.numpy(), g.mem_idx)
    assert np.array_equal(s.mem_idx.numpy(), g.mem_idx)
    got = mem_patch.double().sum(dim=tuple(range(2, mem_patch.dim()))).numpy()
    assert np.allclose(got, g.mem_patch_sum, rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize("pattern", ["ones", "short_first", "long_first", "chunks3p5", "whole"])
@pytest.mark.parametrize("case", CASES)
def test_piece_sizes_do_not_matter(case, pattern, cases):
    g, net, x, (want_patch, want_pos, want_idx, want_emb) = cases[case]
    sizes = piece_patterns(x.shape[1], net.M, net.I)[pattern]
    s = feed_all(net, x, sizes)
    mem_patch, mem_pos = s.finish()
    assert torch.equal(mem_patch, want_patch)
    assert (mem_pos is None and want_pos is None) or torch.equal(mem_pos, want_pos)
    assert torch.equal(net.last_mem_idx, want_idx) and torch.equal(net.last_mem_emb, want_emb)
    with torch.no_grad():        # forward(..., mem_emb=) keeps working after a stream
        a, b = net(mem_patch, mem_pos, mem_emb=net.last_mem_emb), net(mem_patch, mem_pos)
    for k in a:
        assert torch.allclose(a[k], b[k], atol=1e-6)


def small_net(**kw):
    conf = synth.mnist_conf(N=40, M=8, I=8, **kw)
    return synth.fill_weights(IPSNet(torch.device("cpu"), conf), 5).eval(), conf


def test_a_total_of_at_most_m_takes_the_shortcut():
    net, conf = small_net(use_pos=True)
    x = synth.make_patches(conf, 2, seed=3)
    for total, sizes in ((5, [2, 3]), (8, [8]), (8, [3, 5])):
        s = feed_all(net, x[:, :total], sizes)
        mem_patch, mem_pos = s.finish()
        assert torch.equal(mem_patch, x[:, :total]) and net.last_mem_idx is None and net.last_mem_emb is None
        assert tuple(mem_pos.shape) == (2, total, conf.D) and torch.equal(mem_pos[1], net.pos_enc[0, :total])


def test_refusals(monkeypatch):
    net, conf = small_net(use_pos=True)
    x = synth.make_patches(conf, 2, seed=3)
    s = net.ips_stream()
    s.feed(x[:, :10])
    with pytest.raises(ValueError):
        s.feed(x[:1, 10:12])                     # another B
    with pytest.raises(ValueError):
        s.feed(x[:, 10:12, :, :16])              # another patch shape
    with pytest.raises(TypeError):
        s.feed(x[:, 10:12].double())             # another dtype
    with pytest.raises(ValueError):
        s.feed(x[:, 10:10])                      # no rows
    with pytest.raises(ValueError, match="positional"):
        s.feed(torch.cat((x[:, 10:], x[:, :1]), 1))          # 41 patches, a table of 40 rows
    assert s.fed == 10                           # a refused piece leaves the stream as it was
    monkeypatch.setenv("IPSX_DEDUP_BLANK", "1")
    with pytest.raises(TypeError, match="dedup"):
        s.feed(x[:, 10:12])
    monkeypatch.delenv("IPSX_DEDUP_BLANK")
    s.feed(x[:, 10:])
    s.finish()
    with pytest.raises(RuntimeError, match="finished"):
        s.feed(x[:, :2])
    with pytest.raises(RuntimeError, match="finished"):
        s.finish()
    s = net.ips_stream()
    s.feed(x[:, :10])
    hip.weights_changed()                        # what an optimizer step does (hip.install_optimizer_hook)
    with pytest.raises(RuntimeError, match="weights changed"):
        s.feed(x[:, 10:12])
    with pytest.raises(RuntimeError, match="weights changed"):
        s.finish()
    with pytest.raises(TypeError):
        net.ips_stream().feed(torch.zeros((2, 4, 1, 32, 32), dtype=torch.uint8))        # uint8 without a table
    with pytest.raises(ValueError):
        net.ips_stream().feed(torch.zeros((2, 4, 64)))                                   # feature rows for an image net


def test_a_training_mode_net_is_restored_after_every_feed():
    net, conf = small_net()
    net.shuffle = False
    x = synth.make_patches(conf, 2, seed=4)
    want = net.ips(x)[0]
    want_idx = net.last_mem_idx
    net.train()
    stats = net.encoder[1].running_mean.clone()
    s = net.ips_stream()
    for lo in range(0, 40, 7):
        s.feed(x[:, lo:lo + 7])
        assert net.training and net.encoder.training and net.transf.training
    mem_patch, _ = s.finish()
    assert net.training and net.encoder.training and net.transf.training
    assert torch.equal(net.encoder[1].running_mean, stats)            # running statistics untouched
    assert torch.equal(mem_patch, want) and torch.equal(net.last_mem_idx, want_idx)


@pytest.mark.parametrize("rows", [10, 8, 3, 17])
def test_the_caller_may_overwrite_the_piece_after_every_feed(rows):
    """one buffer refilled for every feed (10 rows: feeds end with M <= held < M + I; 8 = M = I; 3; 17 > M + I): the stream
    keeps nothing of the caller's tensor"""
    net, conf = small_net(use_pos=True)
    net.shuffle = False
    x = synth.make_patches(conf, 2, seed=6)
    want_patch, want_pos = net.ips(x)
    want_idx, want_emb = net.last_mem_idx.clone(), net.last_mem_emb.clone()
    buf = torch.empty((2, rows) + tuple(x.shape[2:]))
    s = net.ips_stream()
    for lo in range(0, 40, rows):
        n = min(rows, 40 - lo)
        buf[:, :n] = x[:, lo:lo + n]
        s.feed(buf[:, :n])
        buf.fill_(float("nan"))
    mem_patch, mem_pos = s.finish()
    assert torch.equal(net.last_mem_idx, want_idx) and torch.equal(mem_patch, want_patch) and torch.equal(mem_pos, want_pos)
    assert torch.equal(net.last_mem_emb, want_emb)


def test_rows_strided_inside_an_image_are_taken_as_ips_takes_them():
    net, conf = small_net()
    net.shuffle = False
    wide = synth.make_patches(synth.mnist_conf(N=40, M=8, I=8, patch=48), 2, seed=8)
    x = wide[:, :, :, 5:37, 9:41]                # a spatial crop: (2, 40, 1, 32, 32), rows not contiguous
    assert not x[0].is_contiguous()
    want_patch, _ = net.ips(x)
    want_idx = net.last_mem_idx.clone()
    s = feed_all(net, x, [11, 11, 18])
    mem_patch, _ = s.finish()
    assert torch.equal(mem_patch, want_patch) and torch.equal(net.last_mem_idx, want_idx)


def test_uint8_pieces_on_the_cpu_device():
    net, conf = small_net()
    net.shuffle = False
    table = (torch.arange(256, dtype=torch.float32) / 255.0).view(1, 256)
    net.set_patch_table(table)
    q = torch.randint(0, 256, (2, 40, 1, 32, 32), dtype=torch.uint8, generator=torch.Generator().manual_seed(9))
    want_patch, _ = net.ips(q)
    want_idx = net.last_mem_idx
    s = feed_all(net, q, [5, 9, 26])
    mem_patch, _ = s.finish()
    assert mem_patch.dtype == torch.float32 and torch.equal(mem_patch, want_patch) and torch.equal(net.last_mem_idx, want_idx)


# ------------------------------------------------------------------ the two exports: header, binding, argument checks
def test_header_declares_both_exports_inside_the_306_block():
    text = open(HEADER).read()
    assert re.search(r"#define\s+IPSX_VERSION\s+306\b", text)
    block = text[text.index("3.06  (additions only)"):text.index("#define IPSX_VERSION")]
    assert "ipsx_scan_range_strided" in block and "ipsx_stream_commit" in block
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+ipsx_scan_range_strided\s*\(", plain) and re.search(r"\bint\s+ipsx_stream_commit\s*\(", plain)
    assert "ipsx_scan_range_strided" in hip._EXPORTS and "ipsx_stream_commit" in hip._EXPORTS
    lib = hip.lib()
    assert lib.ipsx_version() == 306
    assert lib.ipsx_scan_range_strided.argtypes[1] is C.c_int64 and len(lib.ipsx_scan_range_strided.argtypes) == 16


def test_stream_commit_refuses_bad_arguments_before_any_launch():
    lib = hip.lib()
    buf = (C.c_char * 256)()
    one = hip.StreamTable()
    one.held = one.piece = one.dst = C.addressof(buf)
    one.held_rows, one.held_bstride_rows, one.dst_rows, one.dst_bstride_rows, one.row_bytes = 2, 8, 8, 8, 16
    tabs = (hip.StreamTable * 5)(*([one] * 5))

    def refused(rc, what):
        assert rc != 0 and what in lib.ipsx_last_error().decode(), lib.ipsx_last_error()

    refused(lib.ipsx_stream_commit(None, 1, None, 1, 4, 4, 0, None), "null tables")
    refused(lib.ipsx_stream_commit(tabs, 1, None, 1, 0, 4, 0, None), "bad sizes")          # m <= 0
    refused(lib.ipsx_stream_commit(tabs, 1, None, 1, -3, 4, 0, None), "bad sizes")
    refused(lib.ipsx_stream_commit(tabs, 5, None, 1, 4, 4, 0, None), "5 tables")            # more than four
    refused(lib.ipsx_stream_commit(tabs, 0, None, 1, 4, 4, 0, None), "0 tables")
    refused(lib.ipsx_stream_commit(tabs, 1, None, 1, 4, 9, 0, None), "do not fit")          # 9 rows into room for 8
    sel = (C.c_int64 * 4)(0, 1, 2, 3)
    refused(lib.ipsx_stream_commit(tabs, 1, C.addressof(sel), 1, 4, 4, 5, None), "tail starts")
    refused(lib.ipsx_stream_commit(tabs, 1, C.addressof(sel), 1, 4, 4, 4, None), "in place")
    with pytest.raises(RuntimeError, match="null tables"):
        hip.stream_commit(None, None, 4, 4)
    t = torch.zeros((1, 8, 4))
    with pytest.raises(ValueError, match="5 tables"):         # (the wrapper's own count, in front of its device check)
        hip.stream_commit([(t, 2, t[:, :2], t)] * 5, None, 4, 4)
    with pytest.raises(ValueError, match="piece of 3 rows"):
        hip.stream_commit([(t, 2, t[:, :3], t)], None, 4, 4)
