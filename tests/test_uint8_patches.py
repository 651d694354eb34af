"""uint8 patch storage on the GPU: every stem that reads patches from memory looks bytes up in a per-channel table
(``ipsx_trunk_encode_u8`` / ``_indexed_u8``, ``ipsx_dequant_patches``), and ``IPSNet.ips`` selects on uint8 patches what it
selects on the expanded float32 tensor.

The yardstick everywhere is the float32 path on ``table[c][q]`` (held to the oracle and the reference by the rest of the
suite), compared with ``torch.equal``: a stem that stages ``table[c][byte]`` feeds its first fma the very bits the float32
stem reads, so there is no tolerance.  Tables are random normal floats with a different row per channel and
``table[c][0] != 0``: a dequantised pad, a wrong channel row or a signed byte read changes bits.  About half the patches are
all-zero bytes (Megapixel-MNIST's sparsity and its tied scores)."""

import pytest
import torch

from ips_amd import hip, quant, synth
from ips_amd.architecture import IPSNet

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def rand_table(n_chan, seed):
    t = torch.randn((n_chan, 256), generator=torch.Generator().manual_seed(seed))
    assert bool((t[:, 0] != 0).all()) and (n_chan == 1 or not torch.equal(t[0], t[1]))
    return t.to(DEV)


def rand_bytes(shape, seed):
    """uint8 patches (..., C, h, w): uniform over 0..255, 0 / 127 / 128 / 255 present, every second patch all zeros."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)
    flat = q.view(-1, *shape[-3:])
    flat[1::2] = 0
    flat[0].view(-1)[:4] = torch.tensor([0, 127, 128, 255], dtype=torch.uint8)
    return q


def expanded(q, table):
    """The float32 tensor the dataset would have delivered: table[c][q] by indexing."""
    return quant.dequant(q, table)


@pytest.fixture(scope="module")
def nets():
    made = {}

    def get(name):
        if name not in made:
            conf = {"mnist": lambda: synth.mnist_conf(N=2500, M=64, I=64),
                    "mnist50": lambda: synth.mnist_conf(N=196, M=32, I=48, patch=50),
                    "traffic": lambda: synth.traffic_conf(N=48, M=8, I=16, patch=100)}[name]()
            net = synth.fill_weights(IPSNet(DEV, conf), 7).to(DEV).eval()
            net.set_patch_table(rand_table(conf.n_chan_in, 11))
            made[name] = (conf, net)
        return made[name]
    return get


def round_plus_5():
    return 8 * hip.device_geometry(DEV).cus + 5          # one whole round of the eight-patch kernel and a remainder


# ---------------------------------------------------------------------------------------------- encode
def check_encode(net, shape, n, seed, kernel):
    plan = hip.EncoderPlan(net.encoder, True)
    table = rand_table(shape[0], seed)
    q = rand_bytes((n,) + shape, seed + 1).to(DEV)
    want = plan.encode(expanded(q, table))
    assert kernel in hip.encoder_kernel_name(plan), hip.encoder_kernel_name(plan)
    got = plan.encode(q, table=table)
    assert kernel in hip.encoder_kernel_name(plan)
    assert got.dtype == torch.float32 and torch.equal(got, want), (shape, n)
    return plan, table, q, want


@pytest.mark.parametrize("n", [1, 7, 8, 9, "round+5"])
def test_fused_trunk_on_bytes(nets, n):
    n = round_plus_5() if n == "round+5" else n
    check_encode(nets("mnist")[1], (1, 32, 32), n, 20, "fused_trunk_kernel")


def test_fused_trunk_through_an_index_list(nets):
    n = round_plus_5()
    plan, table, q, want = check_encode(nets("mnist")[1], (1, 32, 32), n, 22, "fused_trunk_kernel")
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3)).to(DEV)
    got = plan.encode_indexed(q, perm.to(torch.int32), table=table)
    assert torch.equal(got, want[perm])
    assert torch.equal(got, plan.encode_indexed(expanded(q, table), perm.to(torch.int32)))


@pytest.mark.parametrize("n", [1, 4, 5, 9, 1027])           # 1,027: across the two-stream split of encode_plain at 1,024
def test_stem_pool50_on_bytes(nets, n):
    check_encode(nets("mnist50")[1], (1, 50, 50), n, 30, "stem_pool50_kernel")


@pytest.mark.parametrize("n", [1, 3, 5])
def test_stem_pool100x3_on_bytes(nets, n):
    check_encode(nets("traffic")[1], (3, 100, 100), n, 40, "stem_pool100x3_kernel")


@pytest.mark.parametrize("n", [3, 5])
@pytest.mark.parametrize("name,shape", [("traffic", (3, 37, 45)), ("mnist", (1, 41, 29))])
def test_generic_stem_on_bytes(nets, name, shape, n):
    """Patch shapes no fused stem covers: conv_any_kernel gathers the bytes (odd, unequal sides: rows at any address)."""
    plan, _, _, _ = check_encode(nets(name)[1], shape, n, 50, "conv_nhwc_kernel (layer by layer)")
    assert hip.encoder_kernel_name(plan) == "conv_nhwc_kernel (layer by layer)"


# ---------------------------------------------------------------------------------------------- dequant_patches
@pytest.mark.parametrize("shape", [(9, 1, 32, 32), (5, 1, 50, 50), (3, 3, 100, 100), (3, 3, 37, 45), (5, 1, 41, 29), (2, 16, 1, 32, 32),
                                   (3, 1, 5, 7)])
def test_dequant_patches_is_the_table_by_indexing(shape):
    table = rand_table(shape[-3], 60)
    q = rand_bytes(shape, 61).to(DEV)
    got = hip.dequant_patches(q, table)
    assert got.dtype == torch.float32 and got.shape == q.shape and torch.equal(got, expanded(q, table))
    if q.numel() % 4 == 1:                               # a view that starts at an odd address: the byte-wise path
        tail = q.view(-1)[1:].view(1, 1, 1, -1)
        assert torch.equal(hip.dequant_patches(tail, table[:1]), expanded(tail, table[:1]))


# ---------------------------------------------------------------------------------------------- ips
def run_ips(net, x, seed=5):
    torch.manual_seed(seed)
    mem_patch, mem_pos = net.ips(x)
    emb = net.last_mem_emb
    torch.cuda.synchronize()
    return dict(patch=mem_patch.clone(), pos=None if mem_pos is None else mem_pos.clone(), idx=net.last_mem_idx.clone(),
                emb=emb.clone(), order=None if net.last_shuffle is None else net.last_shuffle.clone())


def assert_same_call(got, want, what):
    assert got["patch"].dtype == torch.float32, what
    assert torch.equal(got["idx"], want["idx"]), what
    assert torch.equal(got["patch"], want["patch"]), what
    assert (got["pos"] is None) == (want["pos"] is None) and (got["pos"] is None or torch.equal(got["pos"], want["pos"])), what
    assert torch.equal(got["emb"], want["emb"]), what
    assert (got["order"] is None) == (want["order"] is None), what
    assert got["order"] is None or torch.equal(got["order"].cpu(), want["order"].cpu()), what


@pytest.mark.parametrize("name,B,N", [("mnist", 16, 2500),      # parts with ranges, the fused trunk's index lists
                                      ("mnist", 2, 300),        # a small batch in one piece
                                      ("mnist", 1, 2500),       # float32: the one-image stream kernel; uint8: the parts
                                      ("mnist50", 2, 196),      # M = 32, I = 48: a ragged last chunk of 20
                                      ("traffic", 2, 48)])      # M = 8, I = 16: a ragged last chunk of 8
def test_ips_on_bytes_selects_what_it_selects_on_the_expanded_tensor(nets, name, B, N):
    conf, net = nets(name)
    if N != conf.N:
        net = synth.fill_weights(IPSNet(DEV, conf.clone(N=N)), 7).to(DEV).eval()
        net.set_patch_table(nets(name)[1].patch_table)
    q = rand_bytes((B, N, conf.n_chan_in) + tuple(conf.patch_size), 70).to(DEV)
    x = expanded(q, net.patch_table)
    want = run_ips(net, x)
    got = run_ips(net, q)
    assert_same_call(got, want, (name, B, N))
    for b in range(B):                                  # ... and they are the dequantised rows of the input
        assert torch.equal(got["patch"][b], x[b, got["idx"][b]])


@pytest.mark.parametrize("style", ["batch", "instance"])
def test_a_shuffled_call_on_bytes_goes_through_the_index(nets, style):
    conf, _ = nets("mnist")
    net = synth.fill_weights(IPSNet(DEV, conf.clone(shuffle=True, shuffle_style=style)), 7).to(DEV).eval()
    net.set_patch_table(rand_table(1, 11))
    q = rand_bytes((16, 2500, 1, 32, 32), 71).to(DEV)
    x = expanded(q, net.patch_table)
    want = run_ips(net, x, 9)
    before = net.selection.index_calls
    got = run_ips(net, q, 9)
    assert net.selection.index_calls == before + 1
    assert_same_call(got, want, style)
    # No uint8 tensor of the input's size is allocated.  What a warm ips() call does allocate: the embeddings (128 floats per
    # 1,024-byte patch: 0.5 x the input), the M gathered rows as bytes and as floats, indices - about 0.6 x in all; the
    # shuffled copy alone would add 1.0 x.  Taken on a net without positional encoding: the shuffled (B, N, D) positional
    # table - shuffled by copy on every storage type - is another 0.5 x of a uint8 input and not the subject here.  Only
    # the call itself is inside the window (last_mem_emb joins the parts' embeddings into a second 0.5 x, the caller's).
    del x, want, got
    net = synth.fill_weights(IPSNet(DEV, conf.clone(shuffle=True, shuffle_style=style, use_pos=False)), 7).to(DEV).eval()
    net.set_patch_table(rand_table(1, 11))
    torch.manual_seed(9)
    first, _ = net.ips(q)
    assert net.selection.index_calls == 1
    nbytes = q.numel()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.max_memory_allocated(DEV)
    torch.manual_seed(9)
    again, _ = net.ips(q)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated(DEV) - base
    print("peak above the warm state: %d bytes of an input of %d" % (rise, nbytes))
    assert net.selection.index_calls == 2
    assert rise < nbytes, (rise, nbytes)
    assert torch.equal(again, first)


@pytest.mark.parametrize("pinned", [True, False])
def test_host_bytes_give_the_device_resident_result(nets, pinned):
    conf, net = nets("mnist")
    q = rand_bytes((2, 2500, 1, 32, 32), 72)
    want = run_ips(net, q.to(DEV))
    host = q.pin_memory() if pinned else q
    assert host.is_pinned() == pinned and not host.is_cuda
    got = run_ips(net, host)
    assert got["patch"].is_cuda
    assert_same_call(got, want, pinned)


# ---------------------------------------------------------------------------------------------- refusals
def test_what_does_not_read_bytes_says_so(nets, monkeypatch):
    conf, net = nets("mnist")
    q = rand_bytes((2, 300, 1, 32, 32), 80).to(DEV)
    plan = hip.EncoderPlan(net.encoder, True)
    table = net.patch_table
    for prec in ("bf16", "fp32x3"):
        monkeypatch.setenv("IPSX_PRECISION", prec)
        with pytest.raises(TypeError, match="exact trunk"):
            net.ips(q)
        with pytest.raises(TypeError, match="exact trunk"):
            plan.encode(q[0], table=table)
        monkeypatch.delenv("IPSX_PRECISION")
    monkeypatch.setenv("IPSX_DEDUP_BLANK", "1")
    with pytest.raises(TypeError, match="dedup"):
        net.ips(q)
    with pytest.raises(TypeError, match="dedup"):
        plan.encode(q[0], table=table)
    monkeypatch.delenv("IPSX_DEDUP_BLANK")
    with pytest.raises(TypeError, match="dedup"):
        plan.encode(q[0], table=table, nonblank=torch.ones(300, dtype=torch.int32, device=DEV))
    from ips_amd import dist
    with pytest.raises(TypeError, match="float32"):
        dist.ips_sharded(net, q, 300)
    with pytest.raises(TypeError, match="set_patch_table"):
        plan.encode(q[0])
    with pytest.raises(TypeError, match="set_patch_table"):
        plan.image_stream(q[0], None, None, 8, None, None, None, None)
    with pytest.raises(ValueError):
        plan.encode(q[0], table=rand_table(3, 1))            # channel count
    with pytest.raises(ValueError):
        plan.encode(q[0], table=table[:, :128])              # shape
    with pytest.raises(TypeError):
        plan.encode(q[0], table=table.double())              # dtype
    with pytest.raises(ValueError):
        hip.dequant_patches(q, rand_table(3, 1))
    with pytest.raises(ValueError):
        net.set_patch_table(rand_table(3, 1))
    bad = table.clone()
    bad[0, 5] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        net.set_patch_table(bad)
    assert net.patch_table is table
    bare = synth.fill_weights(IPSNet(DEV, conf), 7).to(DEV).eval()
    with pytest.raises(TypeError, match="set_patch_table"):
        bare.ips(q)
    assert torch.equal(net.ips(q)[0], net.ips(expanded(q, table))[0])     # and the net is none the worse for it
