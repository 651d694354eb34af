"""``IPSNet.ips_stream()`` on the GPU (ips_amd/stream.py): the stream fed in pieces that never align with the
chunks against ``net.ips(torch.cat(pieces, 1))`` - ``torch.equal`` on everything the call returns and leaves behind, and
``s.mem_idx`` after every feed against ``hip.scan_range`` run to that iteration on the full logits -, the reference's
recorded memory per iteration, uint8 and half-stored pieces, and the two exports alone: ``hip.stream_commit`` against
``torch.cat`` + ``torch.gather`` on the host with guarded destinations and pieces that are slices at odd addresses,
``hip.scan_range_strided`` against ``hip.scan_range`` on the contiguous copy for every loop kernel the dispatcher picks."""

import numpy as np
import pytest
import torch

from ips_amd import hip, synth
from ips_amd.architecture import IPSNet
from tests.stream_cases import piece_patterns
from tests.util import Golden, head_shape_net, HEAD_SHAPES
from view_u8_cases import plain_table

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
PATTERNS = ["ones", "short_first", "long_first", "chunks3p5", "whole"]


def _mnist(**kw):
    return synth.fill_weights(IPSNet(DEV, synth.mnist_conf(**kw)), 5).to(DEV).eval()


NETS = {
    "fused32_pos": (lambda: _mnist(N=300, M=16, I=16), 2),
    "fused32": (lambda: _mnist(N=300, M=16, I=16, use_pos=False), 2),
    "layered50": (lambda: _mnist(N=64, M=8, I=8, patch=50), 2),
    "traffic": (lambda: synth.fill_weights(IPSNet(DEV, synth.traffic_conf(N=12, M=4, I=4)), 5).to(DEV).eval(), 1),
    "features": (lambda: synth.fill_weights(IPSNet(DEV, synth.camelyon_conf(N=180, M=16, I=48, n_chan_in=64)), 5).to(DEV).eval(), 3),
    "r40_d160": (lambda: head_shape_net("r40_d160", DEV), 2),
    # beyond the LDS: 4,200 candidates of 8 logits - the workgroup team by default, reached through the strided entry
    "team": (lambda: synth.fill_weights(IPSNet(DEV, synth.camelyon_conf(N=9000, M=2100, I=2100, n_chan_in=64)), 5).to(DEV).eval(), 2),
}
_CASES = {}


def full_logits(net, x):
    """(B, N, R) logits of the whole input, by the kernels ips() runs"""
    B, N = x.shape[:2]
    ca = net.transf.crs_attn
    emb = net._embed(x.reshape(B * N, *x.shape[2:])).view(B, N, -1)
    return hip.logits(emb, net.pos_enc[:, :N] if net.use_pos else None, ca.folded_query(), ca.H * ca.n_token)


def case(name):
    """net, input and what ips() returns and leaves behind - computed once, shared, never changed"""
    if name not in _CASES:
        make, B = NETS[name]
        net = make()
        assert not net.shuffle
        conf = HEAD_SHAPES[name][0] if name in HEAD_SHAPES else _CONFS[name]
        x = synth.make_patches(conf, B, seed=11).to(DEV)
        with torch.no_grad():
            mem_patch, mem_pos = net.ips(x)
            want = (mem_patch, mem_pos, net.last_mem_idx.clone(), net.last_mem_emb.clone())
            lg = full_logits(net, x)
        _CASES[name] = (net, x, want, lg)
    return _CASES[name]


_CONFS = {"fused32_pos": synth.mnist_conf(N=300, M=16, I=16), "fused32": synth.mnist_conf(N=300, M=16, I=16, use_pos=False),
          "layered50": synth.mnist_conf(N=64, M=8, I=8, patch=50), "traffic": synth.traffic_conf(N=12, M=4, I=4),
          "features": synth.camelyon_conf(N=180, M=16, I=48, n_chan_in=64),
          "team": synth.camelyon_conf(N=9000, M=2100, I=2100, n_chan_in=64)}


def check_stream(net, x, want, lg, sizes):
    M, I = net.M, net.I
    ca = net.transf.crs_attn
    B = x.shape[0]
    idx = torch.empty((B, M), dtype=torch.int64, device=DEV)
    tie = torch.zeros((B,), dtype=torch.int32, device=DEV)
    s = net.ips_stream()
    lo = done = 0
    for n in sizes:
        s.feed(x[:, lo:lo + n])                    # (a slice along the patch axis: read where it lies)
        lo += n
        assert s.fed == lo and s.iterations == max(0, lo - M) // I
        if s.iterations > done:                    # the full loop resumed to this iteration
            hip.scan_range(lg, M, I, ca.H, ca.n_token, done, s.iterations, idx, tie)
            done = s.iterations
            assert torch.equal(s.mem_idx, idx), "after %d patches" % lo
        elif done == 0:
            assert s.mem_idx is None if lo < M else torch.equal(s.mem_idx, torch.arange(M, device=DEV).expand(B, M))
    mem_patch, mem_pos = s.finish()
    want_patch, want_pos, want_idx, want_emb = want
    assert torch.equal(net.last_mem_idx, want_idx)
    assert torch.equal(mem_patch, want_patch)
    assert (mem_pos is None and want_pos is None) or torch.equal(mem_pos, want_pos)
    assert torch.equal(net.last_mem_emb, want_emb)
    return mem_patch, mem_pos


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("name", list(NETS))
def test_stream_equals_ips_on_the_concatenation(name, pattern):
    net, x, want, lg = case(name)
    sizes = piece_patterns(x.shape[1], net.M, net.I)[pattern]
    mem_patch, mem_pos = check_stream(net, x, want, lg, sizes)
    if pattern == "whole":                         # forward(..., mem_emb=) keeps working after a stream
        with torch.no_grad():
            a, b = net(mem_patch, mem_pos, mem_emb=net.last_mem_emb), net(mem_patch, mem_pos)
        for k in a:
            assert torch.equal(a[k], b[k])


def test_host_pieces_and_contiguous_pieces():
    """pieces on the host are copied to the device as they are; a contiguous device piece takes the one-launch encode"""
    net, x, want, lg = case("fused32_pos")
    xh = x.cpu()
    for src in (xh, x):
        s = net.ips_stream()
        for lo in range(0, 300, 70):
            s.feed(src[:, lo:lo + 70].contiguous() if src is x else src[:, lo:lo + 70])
        mem_patch, mem_pos = s.finish()
        assert mem_patch.is_cuda and torch.equal(mem_patch, want[0]) and torch.equal(mem_pos, want[1])
        assert torch.equal(net.last_mem_idx, want[2])


def test_rows_strided_inside_an_image_and_a_reused_buffer():
    """a spatial crop (rows not contiguous inside an image: one copy up front, as ips() makes), fed through ONE buffer that
    is overwritten after every feed on the same stream"""
    net, x, want, lg = case("fused32_pos")
    wide = torch.zeros((2, 300, 1, 40, 48), device=DEV)
    wide[:, :, :, 3:35, 7:39] = x
    crop = wide[:, :, :, 3:35, 7:39]
    assert not crop[0].is_contiguous()
    s = net.ips_stream()
    for lo in range(0, 300, 70):
        s.feed(crop[:, lo:lo + 70])
    mem_patch, mem_pos = s.finish()
    assert torch.equal(mem_patch, want[0]) and torch.equal(mem_pos, want[1]) and torch.equal(net.last_mem_idx, want[2])
    buf = torch.empty((2, 23, 1, 32, 32), device=DEV)
    s = net.ips_stream()
    for lo in range(0, 300, 23):
        n = min(23, 300 - lo)
        buf[:, :n] = x[:, lo:lo + n]
        s.feed(buf[:, :n])
        buf.fill_(float("nan"))
    mem_patch, mem_pos = s.finish()
    assert torch.equal(mem_patch, want[0]) and torch.equal(mem_pos, want[1]) and torch.equal(net.last_mem_idx, want[2])
    assert torch.equal(net.last_mem_emb, want[3])


@pytest.mark.parametrize("name", ["mnist_mini", "cam_b2"])
def test_memory_after_every_feed_is_the_references_on_the_device(name):
    g = Golden(name)
    assert g.perm is None
    net = g.net(DEV)
    x = g.patches().to(DEV)
    M, I, N = net.M, net.I, x.shape[1]
    s = net.ips_stream()
    edges = [0, M] + list(range(M + I, N, I)) + [N]
    for k in range(len(edges) - 1):
        s.feed(x[:, edges[k]:edges[k + 1]])
        assert s.iterations == (edges[k + 1] - M) // I
        if k and s.iterations == k:
            assert np.array_equal(s.mem_idx.cpu().numpy(), g.trace_idx[:, k - 1]), "iteration %d" % k
    mem_patch, _ = s.finish()
    assert np.array_equal(net.last_mem_idx.cpu().numpy(), g.mem_idx)
    got = mem_patch.double().sum(dim=tuple(range(2, mem_patch.dim()))).cpu().numpy()
    assert np.allclose(got, g.mem_patch_sum, rtol=1e-12, atol=1e-9)


def test_uint8_pieces():
    net = _mnist(N=300, M=16, I=16)
    net.set_patch_table(plain_table(1))
    q = torch.randint(0, 256, (2, 300, 1, 32, 32), dtype=torch.uint8, generator=torch.Generator().manual_seed(5)).to(DEV)
    want_patch, want_pos = net.ips(q)
    want_idx, want_emb = net.last_mem_idx.clone(), net.last_mem_emb.clone()
    for pattern in ("short_first", "chunks3p5"):
        s = net.ips_stream()
        lo = 0
        for n in piece_patterns(300, 16, 16)[pattern]:
            s.feed(q[:, lo:lo + n])
            lo += n
        mem_patch, mem_pos = s.finish()
        assert mem_patch.dtype == torch.float32 and torch.equal(mem_patch, want_patch) and torch.equal(mem_pos, want_pos)
        assert torch.equal(net.last_mem_idx, want_idx) and torch.equal(net.last_mem_emb, want_emb)


def test_half_stored_features_under_bf16(monkeypatch):
    """IPSX_PRECISION=bf16, float16 rows: the encoders stay per-row functions there, so the stream equals ips()"""
    monkeypatch.setenv("IPSX_PRECISION", "bf16")
    conf = synth.camelyon_conf(N=180, M=16, I=48, n_chan_in=64)
    net = synth.fill_weights(IPSNet(DEV, conf), 5).to(DEV).eval()
    x = synth.make_patches(conf, 3, seed=12).to(DEV).half()
    want_patch, _ = net.ips(x)
    want_idx, want_emb = net.last_mem_idx.clone(), net.last_mem_emb.clone()
    assert want_patch.dtype == torch.float16
    for pattern in ("short_first", "long_first", "ones"):
        s = net.ips_stream()
        lo = 0
        for n in piece_patterns(180, 16, 48)[pattern]:
            s.feed(x[:, lo:lo + n])
            lo += n
        mem_patch, mem_pos = s.finish()
        assert mem_pos is None and mem_patch.dtype == torch.float16 and torch.equal(mem_patch, want_patch)
        assert torch.equal(net.last_mem_idx, want_idx) and torch.equal(net.last_mem_emb, want_emb)


def test_refusals_come_before_any_launch_on_the_device(monkeypatch):
    net, x, _, _ = case("fused32_pos")
    s = net.ips_stream()
    s.feed(x[:, :20])
    with pytest.raises(TypeError):
        s.feed(x[:, 20:24].half())
    with pytest.raises(ValueError, match="positional"):
        s.feed(torch.cat((x[:, 20:], x[:, :1]), 1))
    with pytest.raises(TypeError):
        net.ips_stream().feed(x[:, :4].half())               # the exact trunk reads float32
    monkeypatch.setenv("IPSX_DEDUP_BLANK", "1")
    with pytest.raises(TypeError, match="dedup"):
        s.feed(x[:, 20:24])
    monkeypatch.delenv("IPSX_DEDUP_BLANK")
    assert s.fed == 20 and s.iterations == 0
    s.feed(x[:, 20:])
    s.finish()
    with pytest.raises(RuntimeError, match="finished"):
        s.feed(x[:, :4])


# ------------------------------------------------------------------ hip.stream_commit alone
ROW_BYTES = (4096, 2500, 4995, 8)          # the 16-byte tier, the 4-byte tier, the byte tier, the id table


def _bytes(shape, seed):
    return torch.randint(0, 251, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def _sliced_piece(B, n, rb, k, seed):
    """(B, n, rb) uint8 on the device as a slice of a larger tensor: its base ``k`` bytes past a 16-byte boundary, its batch
    stride two rows (rounded up to 16 bytes, so that every image starts k past a boundary) larger than its rows"""
    bs = -(-((n + 2) * rb) // 16) * 16
    big = torch.full((B * bs + 64,), 253, dtype=torch.uint8, device=DEV)
    assert big.data_ptr() % 16 == 0
    piece = big.as_strided((B, n, rb), (bs, rb, 1), storage_offset=16 + k)
    piece.copy_(_bytes((B, n, rb), seed).to(DEV))
    assert piece.data_ptr() % 16 == k and piece.stride(0) > n * rb
    return big, piece


@pytest.mark.parametrize("k", [0, 4, 1])
@pytest.mark.parametrize("tail", [0, 1, 3])
def test_stream_commit_against_cat_and_gather(tail, k):
    B, M, I = 3, 5, 4
    assert tail <= I - 1
    n_held, n_piece = M + 2, 7
    n_cand = n_held + n_piece
    g = torch.Generator().manual_seed(100 * tail + k)
    sel = torch.stack([torch.randperm(n_cand, generator=g)[:M] for _ in range(B)])
    sel[0, 0], sel[1, 2], sel[2, 4] = 0, n_held - 1, n_held          # both segments, and the seam between them
    sel[:, 1] = n_cand - 1                                             # the very last row of the piece
    sel[1, 3] = n_held + 1
    tables, keep, wants, guards = [], [], [], []
    for t, rb in enumerate(ROW_BYTES):
        held = torch.full((B, n_held + 3, rb), 252, dtype=torch.uint8, device=DEV)
        held[:, :n_held] = _bytes((B, n_held, rb), 7 * t + 1).to(DEV)
        big, piece = _sliced_piece(B, n_piece, rb, k if rb != 8 else 8 * (k != 0), 7 * t + 2)
        dst = torch.full((B, M + tail + 1, rb), 254, dtype=torch.uint8, device=DEV)        # (the last row is the guard)
        cand = torch.cat((held[:, :n_held].cpu(), piece.cpu()), dim=1)
        take = torch.cat((sel, torch.arange(n_cand - tail, n_cand).expand(B, tail)), dim=1)
        wants.append(torch.gather(cand, 1, take.unsqueeze(-1).expand(-1, -1, rb)))
        tables.append((held, n_held, piece, dst))
        keep.append(big)
    hip.stream_commit(tables, sel.to(DEV), M, n_cand, n_cand - tail)
    torch.cuda.synchronize()
    for (held, _, piece, dst), want, rb in zip(tables, wants, ROW_BYTES):
        got = dst.cpu()
        assert torch.equal(got[:, :M + tail], want), rb
        assert bool((got[:, M + tail] == 254).all()), "guard row of the %d-byte table" % rb
        assert bool((held[:, n_held:] == 252).all())


@pytest.mark.parametrize("k", [0, 4, 1])
def test_stream_commit_appends_when_there_is_no_selection(k):
    B, M = 3, 5
    n_held, n_piece = 3, 4                                             # the start-up phase: fewer than M rows so far
    tables, wants, keep = [], [], []
    for t, rb in enumerate(ROW_BYTES):
        buf = torch.full((B, n_held + n_piece + 1, rb), 254, dtype=torch.uint8, device=DEV)
        buf[:, :n_held] = _bytes((B, n_held, rb), 5 * t + 1).to(DEV)
        big, piece = _sliced_piece(B, n_piece, rb, k if rb != 8 else 8 * (k != 0), 5 * t + 2)
        want = buf.cpu().clone()
        want[:, n_held:n_held + n_piece] = piece.cpu()
        tables.append((buf, n_held, piece, buf))
        wants.append(want)
        keep.append(big)
    # (the logits table of a feed has no piece: its rows are in place already - such a table is skipped)
    lg = torch.full((B, 9, 8), 3.0, device=DEV)
    hip.stream_commit(tables[:3] + [(lg, n_held + n_piece, None, lg)], None, M, n_held + n_piece)
    hip.stream_commit(tables[3:], None, M, n_held + n_piece)
    torch.cuda.synchronize()
    for (buf, _, _, _), want, rb in zip(tables, wants, ROW_BYTES):
        assert torch.equal(buf.cpu(), want), rb                        # the piece behind the held rows, the guard row untouched
    assert bool((lg == 3.0).all())
    # one piece shared by every image (batch stride 0): the id table of a feed
    ids = torch.full((B, 8), -1, dtype=torch.int64, device=DEV)
    hip.stream_commit([(ids, 2, torch.arange(40, 45, device=DEV).unsqueeze(0), ids)], None, M, 7)
    assert torch.equal(ids.cpu(), torch.tensor([-1, -1, 40, 41, 42, 43, 44, -1]).expand(B, 8))


def test_stream_commit_clamps_and_refuses():
    B, M = 2, 3
    held = torch.arange(B * 6 * 4, dtype=torch.float32, device=DEV).view(B, 6, 4)
    piece = -torch.arange(B * 2 * 4, dtype=torch.float32, device=DEV).view(B, 2, 4) - 1
    dst = torch.zeros((B, 4, 4), device=DEV)
    sel = torch.tensor([[-7, 99, 2], [7, 0, 1 << 40]], device=DEV)              # clamped into the 8 candidates
    hip.stream_commit([(held, 6, piece, dst)], sel, M, 8, 8)
    cand = torch.cat((held, piece), 1)
    want = torch.gather(cand, 1, sel.clamp(0, 7).unsqueeze(-1).expand(-1, -1, 4))
    assert torch.equal(dst[:, :3], want) and bool((dst[:, 3] == 0).all())
    with pytest.raises(RuntimeError, match="do not fit"):
        hip.stream_commit([(held, 6, piece, dst)], sel, M, 8, 6)                # 3 + 2 rows into room for 4
    with pytest.raises(RuntimeError, match="in place"):
        hip.stream_commit([(held, 6, piece, held)], sel, M, 8, 8)
    # a destination at another base inside the held rows' allocation, or inside the piece's: refused by their byte ranges
    one = torch.arange(40, dtype=torch.float32, device=DEV).view(1, 10, 4)
    with pytest.raises(RuntimeError, match="in place"):
        hip.stream_commit([(one, 6, piece[:1], one[:, 4:8])], sel[:1], M, 8, 8)
    with pytest.raises(RuntimeError, match="overlaps the piece"):
        hip.stream_commit([(held[:1], 6, one[:, 2:4], one[:, 3:7])], sel[:1], M, 8, 8)


# ------------------------------------------------------------------ hip.scan_range_strided alone
@pytest.mark.parametrize("N,M,I,H,T", [
    (300, 16, 16, 8, 4),            # scan_fast_kernel, 32 logits per candidate
    (1000, 32, 48, 8, 1),           # scan_fast_kernel, 8 logits
    (3000, 256, 256, 8, 1),         # scan_cam_kernel
    (8950, 4200, 300, 3, 3),        # scan_large_kernel (one workgroup per image: other head / token counts)
    (9000, 2100, 2100, 8, 1),       # scan_large_team_kernel
])
def test_scan_range_strided_equals_scan_range_on_the_contiguous_copy(N, M, I, H, T):
    B, R = 2, H * T
    n_iter = -(-(N - M) // I)
    assert (N - M) % I, "a ragged last chunk"
    lg = (torch.randn((B, N, R), generator=torch.Generator().manual_seed(N + M)) * 3.0).to(DEV)
    cap = N + 37
    table = torch.full((B, cap, R), 1e30, device=DEV)
    table[:, :N] = lg
    want = torch.empty((B, M), dtype=torch.int64, device=DEV)
    want_tie = torch.zeros((B,), dtype=torch.int32, device=DEV)
    hip.scan_range(lg, M, I, H, T, 0, n_iter, want, want_tie)
    got = torch.full((B, M), -1, dtype=torch.int64, device=DEV)
    tie = torch.zeros((B,), dtype=torch.int32, device=DEV)
    hip.scan_range_strided(table, N, M, I, H, T, 0, n_iter, got, tie)
    assert torch.equal(got, want) and torch.equal(tie, want_tie)
    cut = max(1, n_iter // 2)                      # resumed, as every range entry is
    got.fill_(-1)
    tie.zero_()
    hip.scan_range_strided(table, N, M, I, H, T, 0, cut, got, tie)
    hip.scan_range_strided(table, N, M, I, H, T, cut, n_iter, got, tie)
    assert torch.equal(got, want) and torch.equal(tie, want_tie)
    with pytest.raises(ValueError):
        hip.scan_range_strided(table, cap + 1, M, I, H, T, 0, 1, got, tie)
    with pytest.raises(RuntimeError, match="rows between the images"):
        # (the library's own check, through the raw entry: fewer rows between the images than candidates)
        hip._ck(hip.lib().ipsx_scan_range_strided(table.data_ptr(), N - 1, B, N, M, I, H, T, 0, 1, got.data_ptr(), None,
                                                  tie.data_ptr(), None, 0, None), "ipsx_scan_range_strided")


def test_duplicated_rows_tie_the_same_way_through_the_strided_entry():
    """bit-equal candidates (torch.topk's order replayed): the tie flags and the order are those of the contiguous call"""
    B, N, M, I, H, T = 2, 301, 16, 24, 8, 4
    lg = (torch.randn((B, N, H * T), generator=torch.Generator().manual_seed(3)) * 3.0)
    lg[:, 40:60] = lg[:, 100:120]
    lg = lg.to(DEV)
    table = torch.full((B, N + 5, H * T), 1e30, device=DEV)
    table[:, :N] = lg
    n_iter = -(-(N - M) // I)
    out = []
    for f, a in ((hip.scan_range, (lg,)), (hip.scan_range_strided, (table, N))):
        idx = torch.empty((B, M), dtype=torch.int64, device=DEV)
        tie = torch.zeros((B,), dtype=torch.int32, device=DEV)
        f(*a, M, I, H, T, 0, n_iter, idx, tie)
        out.append((idx, tie))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


# ------------------------------------------------------------------ memory
def test_the_state_does_not_grow_with_the_input():
    """A warm 32-px net, B = 2, a stream of 16-row pieces (slices of a resident tensor): the peak above what was allocated
    before the stream is the same at N = 4,800 as at N = 1,200, up to 64 KiB of allocator rounding (the margin of
    test_neither_float_images_nor_patches_are_allocated).  The whole float32 input is 4.7 MB / 18.8 MB per image pair."""
    conf = synth.mnist_conf(N=4800, M=16, I=16)
    net = synth.fill_weights(IPSNet(DEV, conf), 5).to(DEV).eval()
    x = synth.make_patches(conf, 2, seed=13).to(DEV)

    def run(N):
        s = net.ips_stream()
        for lo in range(0, N, 16):
            s.feed(x[:, lo:lo + 16])
        return s.finish()

    run(1200)                                      # warm: weights packed, the folded query made
    peaks = {}
    for N in (1200, 4800):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(DEV)
        base = torch.cuda.max_memory_allocated(DEV)
        out = run(N)
        torch.cuda.synchronize()
        peaks[N] = torch.cuda.max_memory_allocated(DEV) - base
        del out
    print("peak above the resident input: N = 1,200: %d B, N = 4,800: %d B" % (peaks[1200], peaks[4800]))
    assert peaks[4800] <= peaks[1200] + 64 * 1024
