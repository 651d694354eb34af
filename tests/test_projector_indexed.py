"""The row-indexed feature producers (ABI 3.06): output row j is computed from source row ``index[j]`` of ``x``, and the
result is - bit for bit - that of the plain kernel run on the gathered tensor ``x[index]``.  An addressing change, not an
arithmetic one: everything is compared with ``torch.equal``.

Row counts around the 32-row unit, the 64-row tile and one row past a whole number of tiles; an index that is a random
permutation, and one with repeats over a strict subset of the source rows, whose other rows are NaN (a row read that
should not be read shows as NaN or as a difference); outputs sit between sentinel rows."""

import ctypes as C

import numpy as np
import pytest
import torch

from ips_amd import hip, synth
from ips_amd.architecture.ips_net import IPSNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = (1, 63, 64, 65, 130, 4097)
DTYPES = {"fp32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
SENTINEL = -777.25
_NETS = {}


def net_for(f, d):
    if (f, d) not in _NETS:
        conf = synth.camelyon_conf(N=256, M=32, I=32, n_chan_in=f, D=d, D_inner=2 * d)
        _NETS[f, d] = synth.fill_weights(IPSNet(torch.device(DEV), conf), 7).to(DEV).eval()
    return _NETS[f, d]


def cases(n, f, dtype, seed):
    """(name, x, index) - a permutation of n source rows; repeats over a strict subset of 2 n + 7 rows, the others NaN."""
    g = torch.Generator().manual_seed(1000 * seed + n)
    x = (torch.randn((n, f), generator=g) * 3.0 + 0.5).to(dtype).to(DEV)
    yield "permutation", x, torch.randperm(n, generator=g).to(torch.int32).to(DEV)
    rows = 2 * n + 7
    x = (torch.randn((rows, f), generator=g) * 3.0 + 0.5).to(dtype)
    named = torch.arange(0, rows, 2)[torch.randperm((rows + 1) // 2, generator=g)[:max(1, n // 2)]]
    index = named[torch.randint(0, named.numel(), (n,), generator=g)]
    keep = torch.zeros(rows, dtype=torch.bool)
    keep[index] = True
    x[~keep] = float("nan")
    yield "repeats over a subset", x.to(DEV), index.to(torch.int32).to(DEV)


def guarded(n, cols, dtype=torch.float32):
    """A (n, cols) output between four sentinel rows on either side -> (whole buffer, the output view)."""
    buf = torch.full((n + 8, cols), SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[4:4 + n]


def guards_intact(buf, n):
    return bool((buf[:4] == SENTINEL).all()) and bool((buf[4 + n:] == SENTINEL).all())


def stats_plain(x, eps=1e-5):
    out = torch.empty((x.shape[0], 2), dtype=torch.float32, device=DEV)
    hip._ck(hip.lib().ipsx_projector_stats_typed(hip._p(x), hip._PATCH_DTYPES[x.dtype], x.shape[0], x.shape[1], C.c_float(eps),
                                                 hip._p(out), hip._stream()), "ipsx_projector_stats_typed")
    return out


def stats_indexed(x, index, out, eps=1e-5):
    hip._ck(hip.lib().ipsx_projector_stats_indexed(hip._p(x), hip._PATCH_DTYPES[x.dtype], hip._p(index), x.shape[0], index.numel(),
                                                   x.shape[1], C.c_float(eps), hip._p(out), hip._stream()),
            "ipsx_projector_stats_indexed")
    return out


@pytest.mark.parametrize("f", [64, 2048])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_indexed_moments_are_the_moments_of_the_gathered_rows(f, dtype):
    for n in ROWS:
        for name, x, index in cases(n, f, DTYPES[dtype], 1):
            want = stats_plain(x[index.long()].contiguous())
            buf, out = guarded(n, 2)
            stats_indexed(x, index, out)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(out).all()), (n, name)
            assert torch.equal(out, want), (n, name)
            assert guards_intact(buf, n), (n, name)


@pytest.mark.parametrize("f,d", [(64, 512), (2048, 512), (64, 128)])
def test_indexed_fp32_apply_is_the_plain_gemm_on_the_gathered_rows(f, d, monkeypatch):
    """ipsx_projector_apply_indexed, without and with a publication word; 8,193 rows: the 64 x 512 workgroup shape that
    launches of more than 127 row tiles take at D = 512."""
    monkeypatch.delenv("IPSX_PRECISION", raising=False)
    plan = hip.EncoderPlan(net_for(f, d).encoder, False)
    for n in ROWS + ((8193,) if d == 512 else ()):
        for name, x, index in cases(n, f, torch.float32, 2):
            xg = x[index.long()].contiguous()
            stats = stats_plain(xg)
            want = plan.encode(xg, stats=stats)
            buf, out = guarded(n, d)
            got = plan.encode(x, stats=stats_indexed(x, index, torch.empty_like(stats)), out=out, index=index)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(got).all()), (n, name)
            assert torch.equal(got, want), (n, name, float((got - want).abs().max()))
            assert guards_intact(buf, n), (n, name)
            ready = torch.zeros((1,), dtype=torch.int32, device=DEV)
            buf, out = guarded(n, d)
            got = plan.encode(x, out=out, index=index, publish=(ready, 17))         # (moments in the plan's workspace)
            torch.cuda.synchronize()
            assert torch.equal(got, want) and int(ready.item()) == 17 and guards_intact(buf, n), (n, name)


@pytest.mark.parametrize("f,d", [(64, 512), (2048, 512), (64, 128)])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_indexed_bf16_apply_is_the_plain_bf16_projector_on_the_gathered_rows(f, d, dtype, monkeypatch):
    monkeypatch.setenv("IPSX_PRECISION", "bf16")
    plan = hip.EncoderPlan(net_for(f, d).encoder, False)
    for n in ROWS:
        for name, x, index in cases(n, f, DTYPES[dtype], 3):
            want = plan.encode(x[index.long()].contiguous())
            assert plan.bf16
            ready = torch.zeros((1,), dtype=torch.int32, device=DEV)
            buf, out = guarded(n, d)
            stats = stats_indexed(x, index, torch.empty((n, 2), dtype=torch.float32, device=DEV))
            got = plan.encode(x, stats=stats, out=out, index=index, publish=(ready, n))
            torch.cuda.synchronize()
            assert bool(torch.isfinite(got).all()), (n, name)
            assert torch.equal(got, want), (n, name, float((got - want).abs().max()))
            assert int(ready.item()) == n and guards_intact(buf, n), (n, name)


def run_stream(plan, net, x, index, n, wgs, short, slides):
    ca = net.transf.crs_attn
    vq, R = ca.folded_query(), ca.H * ca.n_token
    ebuf, emb = guarded(n, plan.d_out)
    lbuf, lg = guarded(n, R)
    ctl = torch.zeros((plan.stream_ctl_words(n),), dtype=torch.int32, device=DEV)
    ready = torch.zeros((slides,), dtype=torch.int32, device=DEV)
    plan.stream(x, vq, R, emb, lg, ctl, ready, workgroups=wgs, short_first=short, slide_rows=n // slides, index=index)
    torch.cuda.synchronize()
    return emb, lg, ready, guards_intact(ebuf, n) and guards_intact(lbuf, n)


@pytest.mark.parametrize("f", [64, 2048])
def test_indexed_stream_is_the_plain_stream_on_the_gathered_rows(f, monkeypatch):
    """ipsx_projector_stream_indexed: embeddings, logits and progress words.  The stream takes 64 rows or more and
    D = 512; the last three shapes: 32-row tiles only, several slides one after the other, and a guided launch whose
    leftover units go out as column quarters (the three tile shapes of the kernel)."""
    monkeypatch.delenv("IPSX_PRECISION", raising=False)
    net = net_for(f, 512)
    plan = hip.EncoderPlan(net.encoder, False)
    shapes = [(n, 0, -1, 1) for n in ROWS if n >= 64] + [(1000, 7, -2, 1), (3 * 352, 5, 2, 3), (203 * 32 - 7, 40, -12, 1)]
    for n, wgs, short, slides in shapes:
        assert plan.stream_supported(n, net.transf.crs_attn.H * net.transf.crs_attn.n_token)
        for name, x, index in cases(n, f, torch.float32, 4):
            want_emb, want_lg, want_ready, _ = run_stream(plan, net, x[index.long()].contiguous(), None, n, wgs, short, slides)
            emb, lg, ready, intact = run_stream(plan, net, x, index, n, wgs, short, slides)
            assert bool(torch.isfinite(emb).all()) and bool(torch.isfinite(lg).all()), (n, name)
            assert torch.equal(emb, want_emb), (n, name, float((emb - want_emb).abs().max()))
            assert torch.equal(lg, want_lg), (n, name, float((lg - want_lg).abs().max()))
            assert ready.tolist() == [n // slides] * slides == want_ready.tolist(), (n, name, ready.tolist())
            assert intact, (n, name)


def test_row_bases_beyond_4_gib(monkeypatch):
    """Source rows at both ends of a tensor of just over 4 GiB: a row base computed in 32 bits would read the wrong rows.
    Only the 128 named rows are written; every indexed producer against its plain form on those rows gathered."""
    free, _ = torch.cuda.mem_get_info()
    if free < 8 << 30:
        pytest.skip("needs 8 GiB of free device memory")
    f, d = 2048, 512
    rows = (4 << 30) // (f * 4) + 64
    x = torch.empty((rows, f), dtype=torch.float32, device=DEV)
    g = torch.Generator().manual_seed(99)
    ends = (torch.randn((128, f), generator=g) * 3.0 + 0.5).to(DEV)
    x[:64] = ends[:64]
    x[rows - 64:] = ends[64:]
    named = torch.cat((torch.arange(64), torch.arange(rows - 64, rows)))
    order = torch.randperm(128, generator=g)
    index = named[order].to(torch.int32).to(DEV)
    xg = ends[order.to(DEV)].contiguous()
    assert (int(index.max()) * f * 4) >> 32 >= 1
    net = net_for(f, d)
    monkeypatch.delenv("IPSX_PRECISION", raising=False)
    plan = hip.EncoderPlan(net.encoder, False)
    want_stats = stats_plain(xg)
    got_stats = stats_indexed(x, index, torch.empty_like(want_stats))
    assert torch.equal(got_stats, want_stats)
    assert torch.equal(plan.encode(x, stats=got_stats, index=index), plan.encode(xg, stats=want_stats))
    want_emb, want_lg, _, _ = run_stream(plan, net, xg, None, 128, 0, -1, 1)
    emb, lg, ready, intact = run_stream(plan, net, x, index, 128, 0, -1, 1)
    assert torch.equal(emb, want_emb) and torch.equal(lg, want_lg) and ready.tolist() == [128] and intact
    monkeypatch.setenv("IPSX_PRECISION", "bf16")
    plan16 = hip.EncoderPlan(net.encoder, False)
    assert torch.equal(plan16.encode(x, index=index), plan16.encode(xg))
    del x


def test_indexed_finish_gathers_from_the_unshuffled_tensor():
    """ipsx_ips_finish_indexed: patch rows through the permutation, positional rows and indices in the loop's numbering -
    one permutation per image, and one shared by all."""
    g = torch.Generator().manual_seed(5)
    B, N, M = 3, 50, 7
    src = torch.randn((B, N, 2, 4, 4), generator=g).to(DEV)
    pos = torch.randn((B, N, 8), generator=g).to(DEV)
    idx = torch.stack([torch.randperm(N, generator=g)[:M] for _ in range(B)]).to(DEV)
    status = torch.full((1,), 6, dtype=torch.int32, device=DEV)
    for shared in (False, True):
        order = torch.stack([torch.randperm(N, generator=g) for _ in range(1 if shared else B)]).to(DEV)
        mirror = torch.zeros((1,), dtype=torch.int32).pin_memory()
        got_idx, got_patch, got_pos = hip.ips_finish(src, pos, idx, status, mirror, order=order)
        torch.cuda.synchronize()
        through = torch.gather(order.expand(B, -1), 1, idx)
        assert torch.equal(got_idx, idx) and got_idx.data_ptr() != idx.data_ptr()
        assert torch.equal(got_patch, hip.gather_rows(src, through))
        assert torch.equal(got_pos, hip.gather_rows(pos, idx))
        assert int(mirror.item()) == 6
