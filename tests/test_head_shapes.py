"""The attention side's kernels at head shapes no shipped configuration uses (tests/util.py HEAD_SHAPES): R = H * n_token
from 32 to 256, D_k != D / H, D_v != D_k, D off the multiples of 128, n_class up to 130.

Each kernel is held bitwise against the oracle, and against the same IPSNet run in float64 through its plain torch
modules within HEAD_F64_BOUNDS - the bounds the oracle itself keeps at these shapes on the same inputs
(tests/test_oracle_props.py::test_oracle_tracks_float64_at_head_shapes_no_config_uses measures them; per element, the
worst case 2.3e-7 of the logits' scale, 7.3e-6 of a score, 1.8e-5 of an attention weight, 4.3e-6 of a prediction).
Shapes the kernels refuse must raise, naming the limit."""

import numpy as np
import pytest
import torch

from ips_amd import hip, synth
from ips_amd.architecture import IPSNet
from oracle import oracle as orc
from tests.util import (HEAD_F64_BOUNDS, HEAD_SHAPES, f64_logits, head_shape_inputs, head_shape_net, head_shape_net64,
                        head_shape_scores_lengths, rel_err, ulp_diff)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = sorted(HEAD_SHAPES)
AGGREGATING = [n for n in NAMES if HEAD_SHAPES[n][2]]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("name", NAMES)
def test_query_projection_and_logits(name):
    """query_proj, and the logits with a per-image positional table, a broadcast one (batch stride 0) and none: every
    column tile (partial last ones included), the 16-group trips, the 8-group tail, the scalar remainder and the masked
    path of D % 8 != 0."""
    net, o, net64 = head_shape_net(name, DEV), orc.Oracle(head_shape_net(name)), head_shape_net64(name)
    ca = net.transf.crs_attn
    R = ca.H * ca.n_token
    qs = hip.query_proj(ca.q[0], ca.q_w.weight, ca.attention.temperature)
    assert ulp_diff(qs.cpu().numpy(), o.qs) == 0
    inp = head_shape_inputs(name)
    x, pos = inp["x"], inp["pos"]
    vq = ca.folded_query()
    got = hip.logits(dev(x), dev(pos), vq, R).cpu().numpy()
    for b in range(2):
        assert ulp_diff(got[b], o.logits(x[b], pos[b])) == 0, b
        want, scale = f64_logits(net64, x[b], pos[b])
        assert (np.abs(got[b] - want) / scale).max() <= HEAD_F64_BOUNDS["logits"]
    got = hip.logits(dev(x), dev(pos[:1]), vq, R).cpu().numpy()
    for b in range(2):
        assert ulp_diff(got[b], o.logits(x[b], pos[0])) == 0, b
    got = hip.logits(dev(x), None, vq, R).cpu().numpy()
    for b in range(2):
        assert ulp_diff(got[b], o.logits(x[b])) == 0, b


@pytest.mark.parametrize("name", NAMES)
def test_scores_and_attention_maps(name):
    """Transformer.get_scores / get_attn at 53 candidates (logits staged in LDS) and at a candidate set past the 160 KiB
    staging limit of scores_kernel (read from global memory)."""
    net, o, net64 = head_shape_net(name, DEV), orc.Oracle(head_shape_net(name)), head_shape_net64(name)
    ca = net.transf.crs_attn
    R = ca.H * ca.n_token
    inp = head_shape_inputs(name)
    small, large = head_shape_scores_lengths(name)
    assert small * (R + 1) * 4 + 8 * R <= 160 * 1024 < large * (R + 1) * 4 + 8 * R
    for L in (small, large):
        rows = inp["rows%d" % L]
        with torch.no_grad():
            sc = net.transf.get_scores(dev(rows)).cpu().numpy()
            attn = ca.get_attn(dev(rows)).cpu().numpy()
            s64 = net64.transf.get_scores(torch.from_numpy(rows).double()).numpy()
            a64 = net64.transf.crs_attn.get_attn(torch.from_numpy(rows).double()).numpy()
        for b in range(2):
            ws, wa = o.scores(rows[b], want_attn=True)
            assert ulp_diff(sc[b], ws) == 0, (L, b)
            assert ulp_diff(attn[b], wa) == 0, (L, b)
            assert rel_err(sc[b], s64[b]) <= HEAD_F64_BOUNDS["scores"], (L, b)
            assert rel_err(attn[b], a64[b]) <= HEAD_F64_BOUNDS["attn"], (L, b)


def _f64_scores_from_logits(lg, H, T):
    """Transformer.get_scores on cached logits (L, H*T), float64: softmax over the candidates per (h, t), mean over heads,
    then over tokens"""
    lg = np.asarray(lg, dtype=np.float64).reshape(-1, H, T)
    e = np.exp(lg - lg.max(0))
    return (e / e.sum(0)).mean(1).mean(1)


def _f64_loop(score_fn, N, M, I):
    """The selection loop in float64; returns the final memory and the smallest relative gap between the M-th and the
    (M+1)-th score over all iterations (how far the selection is from a rounding-sensitive decision)"""
    cur, gap = np.arange(M, dtype=np.int64), np.inf
    for lo in range(M, N, I):
        cand = np.concatenate([cur, np.arange(lo, min(lo + I, N), dtype=np.int64)])
        s = score_fn(cand)
        order = np.argsort(-s, kind="stable")
        gap = min(gap, (s[order[M - 1]] - s[order[M]]) / s[order[M - 1]])
        cur = cand[order[:M]]
    return cur, gap


@pytest.mark.parametrize("name", NAMES)
def test_selection_loop_on_cached_logits(name):
    """hip.scan (every shape of the table takes scan_large_kernel: R = 32 at n_token 1 / 2 included) against the oracle's
    loop - memory and its scores - and a scan cut into two resumed scan_range calls; the memory against a float64
    restatement wherever every iteration's M-th / (M+1)-th score gap stays clear of the score bound."""
    conf = HEAD_SHAPES[name][0]
    H, T = conf.H, conf.n_token
    R, B, M, I = H * T, 2, 24, 56
    N = M + 5 * I + 17                                   # ragged last chunk
    assert hip.lib().ipsx_scan_workspace_bytes(B, M, I, H, T) > 0            # the generic loop, not the LDS-resident one
    lg = (np.random.default_rng(HEAD_SHAPES[name][1] + 7).standard_normal((B, N, R)) * 3.0).astype(np.float32)
    mem, sc = hip.scan(dev(lg), M, I, H, T, want_scores=True)
    mem, sc = mem.cpu().numpy(), sc.cpu().numpy()
    n_iter = -(-(N - M) // I)
    idx = torch.empty((B, M), dtype=torch.int64, device=DEV)
    tie = torch.zeros((B,), dtype=torch.int32, device=DEV)
    hip.scan_range(dev(lg), M, I, H, T, 0, 2, idx, tie)
    hip.scan_range(dev(lg), M, I, H, T, 2, n_iter, idx, tie)
    assert np.array_equal(idx.cpu().numpy(), mem)
    L = orc.lib()
    for b in range(B):
        cur = np.arange(M, dtype=np.int64)
        for lo in range(M, N, I):
            cand = np.concatenate([cur, np.arange(lo, min(lo + I, N), dtype=np.int64)])
            s = np.empty(len(cand), dtype=np.float32)
            L.orc_scores_from_logits(orc._f(lg[b][cand])[1], len(cand), H, T, s.ctypes.data_as(orc.f32p), None)
            top = orc.topm(s, M, aten_ties=True, rows=lg[b][cand])[0]
            cur, last = cand[top], s[top]
        assert np.array_equal(mem[b], cur), b
        assert ulp_diff(sc[b], last) == 0, b
        want, gap = _f64_loop(lambda cand: _f64_scores_from_logits(lg[b][cand], H, T), N, M, I)
        if gap > 2 * HEAD_F64_BOUNDS["scores"]:
            assert np.array_equal(np.sort(mem[b]), np.sort(want)), b


@pytest.mark.parametrize("name", AGGREGATING)
def test_selection_and_forward_end_to_end(name):
    """net.ips (B = 2, a ragged last chunk) and net(mem_patch, mem_pos) against the oracle: the memory's indices, patches
    and positional rows, every task's predictions (softmax and sigmoid heads, n_class from 1 to 130, the aggregation's
    tail above 64 KiB of LDS at r256_d512); the selection against the float64 loop where its gaps are clear; predictions
    of a fixed memory against the float64 net."""
    conf = HEAD_SHAPES[name][0]
    net, cpu, net64 = head_shape_net(name, DEV), head_shape_net(name), head_shape_net64(name)
    o = orc.Oracle(cpu)
    assert (conf.N - conf.M) % conf.I != 0
    x = synth.make_patches(conf, 2, seed=HEAD_SHAPES[name][1] + 11, blank_frac=0.3)
    pos_enc = cpu.pos_enc.numpy() if conf.use_pos else None
    mem_patch, mem_pos = net.ips(x.to(DEV))
    want = o.ips(x.numpy(), pos_enc, aten_ties=True)
    assert np.array_equal(net.last_mem_idx.cpu().numpy(), want["mem_idx"])
    assert np.array_equal(mem_patch.cpu().numpy(), want["mem_patch"])
    if conf.use_pos:
        assert np.array_equal(mem_pos.cpu().numpy(), want["mem_pos"])
    else:
        assert mem_pos is None
    for b in range(2):
        emb = torch.from_numpy(want["emb"][b]).double()
        if conf.use_pos:
            emb = emb + torch.from_numpy(pos_enc[0]).double()

        def score(cand):
            with torch.no_grad():
                return net64.transf.get_scores(emb[torch.from_numpy(cand)][None])[0].numpy()
        sel, gap = _f64_loop(score, conf.N, conf.M, conf.I)
        if gap > 2 * HEAD_F64_BOUNDS["scores"]:
            assert np.array_equal(np.sort(want["mem_idx"][b]), np.sort(sel)), b
    with torch.no_grad():
        preds = net(mem_patch, mem_pos)
    ref = o.forward(want["mem_patch"], want["mem_pos"])
    assert set(preds) == set(ref) == {"soft", "sig"}
    for k in ref:
        assert ulp_diff(preds[k].cpu().numpy(), ref[k]) == 0, k
    # a fixed memory, against the float64 net too
    inp = head_shape_inputs(name)
    mp, mpos = inp["mem_patch"], inp["mem_pos"]
    with torch.no_grad():
        preds = net(dev(mp), dev(mpos) if mpos is not None else None)
        p64 = net64(torch.from_numpy(mp).double(), torch.from_numpy(mpos).double() if mpos is not None else None)
    ref = o.forward(mp, mpos)
    for k in ref:
        got = preds[k].cpu().numpy()
        assert got.shape == (2, conf.n_class)
        assert ulp_diff(got, ref[k]) == 0, k
        assert rel_err(got, p64[k].numpy()) <= HEAD_F64_BOUNDS["preds"], k


@pytest.mark.parametrize("name", ["r64_d192", "r96_d36", "r128_d96"])
def test_bf16_logits_beyond_one_column_tile(name, monkeypatch):
    """ipsx_logits_bf16 with 2, 3 (the 4-tile kernel on a padded folded query) and 4 column tiles, against the fp32
    logits (2 % of their scale: operands of 8 significant bits) and, per element, against a float64 product of exactly the
    operands the kernel multiplies: x = emb + pos in fp32 and the fp32 folded query (bitwise the oracle's, see
    test_query_projection_and_logits), each rounded to bfloat16.  (Refolding V in float64 instead moves a bf16 operand
    by one ulp now and then.)"""
    net = head_shape_net(name, DEV)
    ca = net.transf.crs_attn
    R = ca.H * ca.n_token
    inp = head_shape_inputs(name)
    emb, pos = dev(inp["x"]), dev(inp["pos"])
    vq = ca.folded_query()
    want = hip.logits(emb, pos, vq, R)
    monkeypatch.setenv("IPSX_PRECISION", "bf16")
    vq16 = ca.folded_query()
    assert vq16.dtype == torch.uint8
    got = hip.logits(emb, pos, vq16, R)
    monkeypatch.delenv("IPSX_PRECISION")
    scale = float(want.abs().max())
    assert float((got - want).abs().max()) < 2e-2 * scale
    D = emb.shape[-1]
    r = torch.arange(R, device=DEV).view(R, 1)
    c = torch.arange(D, device=DEV).view(1, D)
    kgs = -(-D // 8)                                      # fold_query_kernel's packing of V (R, D)
    V = vq[(((r >> 5) * kgs + (c >> 3)) * 64 + (r & 31) + 32 * ((c & 7) >> 2)) * 4 + (c & 3)]
    V16 = V.to(torch.bfloat16).double()
    x16 = (emb + pos).to(torch.bfloat16).double()
    emu = torch.einsum("bnc,rc->bnr", x16, V16)
    mag = torch.einsum("bnc,rc->bnr", x16.abs(), V16.abs())
    assert float(((got.double() - emu).abs() / mag).max()) < 1e-5


# ---------------------------------------------------------------- shapes the kernels refuse
def _feature_net(**over):
    conf = synth.camelyon_conf(N=64, M=8, I=8, n_chan_in=64, **over)
    return synth.fill_weights(IPSNet(torch.device(DEV), conf), 5).to(DEV).eval()


def test_more_than_256_logits_per_patch_are_refused():
    net = _feature_net(D=64, H=33, n_token=8, D_k=4, D_v=4, D_inner=64)          # R = 264
    ca = net.transf.crs_attn
    x = torch.randn((2, 40, 64), device=DEV)
    with pytest.raises(RuntimeError, match="256"):
        hip.logits(x, None, ca.folded_query(), 264)
    with pytest.raises(RuntimeError, match="256"), torch.no_grad():
        net.transf.get_scores(x)
    with pytest.raises(RuntimeError, match="256"):
        hip.scan(torch.randn((2, 40, 264), device=DEV), 8, 8, 33, 8)
    torch.cuda.synchronize()


def test_more_than_128_bf16_logits_per_patch_are_refused(monkeypatch):
    net = _feature_net(D=64, H=20, n_token=8, D_k=4, D_v=4, D_inner=64)          # R = 160
    ca = net.transf.crs_attn
    x = torch.randn((2, 40, 64), device=DEV)
    hip.logits(x, None, ca.folded_query(), 160)                                   # fp32: up to 256
    monkeypatch.setenv("IPSX_PRECISION", "bf16")
    vq16 = ca.folded_query()
    assert vq16.dtype == torch.uint8
    with pytest.raises(RuntimeError, match="128"):
        hip.logits(x, None, vq16, 160)
    torch.cuda.synchronize()


def test_aggregation_refuses_token_state_beyond_the_lds():
    net = _feature_net(D=512, H=8, n_token=16, D_k=64, D_v=64, D_inner=2048)     # 16 * (512 + 1024 + 2048) * 4 = 224 KiB
    with pytest.raises(RuntimeError, match="160 KiB"), torch.no_grad():
        net.transf(torch.randn((2, 8, 512), device=DEV))
    torch.cuda.synchronize()


def test_aggregation_refuses_d_not_a_multiple_of_32():
    net = _feature_net(D=48, H=4, n_token=1, D_k=12, D_v=12, D_inner=64)
    with pytest.raises(RuntimeError, match="multiple of 32"), torch.no_grad():
        net(torch.rand((2, 8, 64), device=DEV))
    torch.cuda.synchronize()
