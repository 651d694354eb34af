"""Tensor VIEWS through the kernel wrappers on the GPU: every view the argument contract accepts - transposed,
row-strided, column-sliced, expanded, channels-first, off a 16-byte address where the kernel has a scalar route or the wrapper
copies (tests/test_wrapper_contract_cpu.py proves which) - must give (a) the bits of the same call on the compact tensor
and (b) the operation's plain reference, within the bound the suite already holds that kernel to.  Only accepted arguments
are passed: no refused call is made here and no misaligned pointer reaches a vector path.  Shapes are the smallest at which
a layout mistake shows: one full 32-row wavefront plus a row, D on the logits' vector / trip / masked paths, two images."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wrapper_cases as wc
from ips_amd import hip, synth
from ips_amd.architecture import IPSNet
from ips_amd.data.megapixel_mnist import _unfold
from oracle import oracle as orc
from tests.util import HEAD_F64_BOUNDS, Golden, _feat, f64_logits, head_shape_net, ulp_diff

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CL = torch.channels_last
B, H, T, DK, R = 2, 2, 4, 3, 8


def rnd(shape, seed):
    return wc.rnd(shape, seed, DEV)


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


# ---------------------------------------------------------------- logits / logits_stats
@pytest.mark.parametrize("D", [24, 136, 20])
def test_logits_views(D):
    """D = 24: the float4 path with fewer than 8 k-groups; 136: one 16-group trip plus a single group; 20: the masked path."""
    net = synth.fill_weights(IPSNet(torch.device(DEV), _feat(D, H, T, DK, DK, 32, 1)), 400 + D).to(DEV).eval()
    net64 = synth.fill_weights(IPSNet(torch.device("cpu"), _feat(D, H, T, DK, DK, 32, 1)), 400 + D).double()
    vq = net.transf.crs_attn.folded_query()
    n = 33
    x, pos = rnd((B, n, D), 1), rnd((B, n, D), 2)
    want = hip.logits(x, pos, vq, R)
    for b in range(B):
        ref, scale = f64_logits(net64, x[b].cpu().numpy(), pos[b].cpu().numpy())
        assert (np.abs(want[b].cpu().numpy() - ref) / scale).max() <= HEAD_F64_BOUNDS["logits"]
    for view in (wc.transposed, wc.row_strided, wc.col_sliced, wc.off4):
        v = view(x)
        assert torch.equal(v, x) and (view is wc.off4 or not v.is_contiguous())
        assert torch.equal(hip.logits(v, pos, vq, R), want), view.__name__
    assert torch.equal(hip.logits(x, wc.col_sliced(pos), vq, R), want)
    assert torch.equal(hip.logits(x, wc.off4(pos), vq, R), want)
    # one positional table for every image: expanded over the batch (stride 0), and as pos[:1]
    shared = hip.logits(x, pos[:1].contiguous(), vq, R)
    ref1, scale1 = f64_logits(net64, x[1].cpu().numpy(), pos[0].cpu().numpy())
    assert (np.abs(shared[1].cpu().numpy() - ref1) / scale1).max() <= HEAD_F64_BOUNDS["logits"]
    assert torch.equal(hip.logits(x, pos[:1].expand(B, -1, -1), vq, R), shared)
    assert torch.equal(hip.logits(x, pos[:1], vq, R), shared)
    # out: a row range of a longer table - written in place, nothing around it touched
    table = torch.full((B, n + 7, R), -7.0, device=DEV)
    got = hip.logits(x, pos, vq, R, out=table[:, 3:3 + n])
    assert got.data_ptr() == table[:, 3:3 + n].data_ptr() and torch.equal(table[:, 3:3 + n], want)
    assert bool((table[:, :3] == -7.0).all()) and bool((table[:, 3 + n:] == -7.0).all())
    # logits_stats: the same logits, and the row moments of a row range of a longer feature table
    plan = hip.EncoderPlan(head_shape_net("r33_d64", DEV).encoder, False)          # (64 features per row)
    feats = rnd((12, 64), 3)
    moments = plan.row_stats(feats[3:8].contiguous())
    for emb_view, pos_view in ((wc.transposed, wc.col_sliced), (wc.off4, lambda t: t)):
        table.fill_(-7.0)
        stats = torch.zeros((5, 2), device=DEV)
        hip.logits_stats(emb_view(x), pos_view(pos), vq, R, table[:, 3:3 + n], feats[3:8], stats, plan.ln_eps)
        assert torch.equal(table[:, 3:3 + n], want) and torch.equal(stats, moments)


# ---------------------------------------------------------------- scan / scan_range / topm
def test_scan_and_topm_views():
    N, M, I = 41, 4, 8
    lg = (rnd((B, N, R), 4) * 3.0)
    view = wc.permuted(lg)                           # (B, R, N).permute(0, 2, 1)
    assert torch.equal(view, lg) and not view.is_contiguous()
    mem, sc = hip.scan(lg, M, I, H, T, want_scores=True)
    mem_v, sc_v = hip.scan(view, M, I, H, T, want_scores=True)
    assert torch.equal(mem, mem_v) and torch.equal(sc, sc_v)
    idx = torch.empty((B, M), dtype=torch.int64, device=DEV)
    tie = torch.zeros((B,), dtype=torch.int32, device=DEV)
    n_iter = -(-(N - M) // I)
    hip.scan_range(view, M, I, H, T, 0, 2, idx, tie)
    hip.scan_range(view, M, I, H, T, 2, n_iter, idx, tie)
    assert torch.equal(idx, mem)
    L, lgn = orc.lib(), lg.cpu().numpy()
    for b in range(B):                               # the oracle's loop, as test_scan_matches_oracle runs it
        cur = np.arange(M, dtype=np.int64)
        for lo in range(M, N, I):
            cand = np.concatenate([cur, np.arange(lo, min(lo + I, N), dtype=np.int64)])
            s = np.empty(len(cand), dtype=np.float32)
            L.orc_scores_from_logits(orc._f(lgn[b][cand])[1], len(cand), H, T, s.ctypes.data_as(orc.f32p), None)
            top, _ = orc.topm(s, M)
            cur, last = cand[top], s[top]
        assert np.array_equal(mem[b].cpu().numpy(), cur)
        assert ulp_diff(sc[b].cpu().numpy(), last) == 0
    g = np.random.default_rng(37)
    s = np.stack([g.permutation(37), g.permutation(37)]).astype(np.float32) / 37
    sc_t = torch.from_numpy(np.ascontiguousarray(s.T)).to(DEV).t()          # (37, 2).t()
    assert not sc_t.is_contiguous()
    top = hip.topm(sc_t, M)
    assert torch.equal(top, hip.topm(sc_t.contiguous(), M))
    for b in range(B):
        assert np.array_equal(top[b].cpu().numpy(), orc.topm(s[b], M)[0])
        assert np.array_equal(top[b].cpu().numpy(), torch.topk(torch.from_numpy(s[b]), M)[1].numpy())


# ---------------------------------------------------------------- scores / attn_map / aggregate / head
def test_head_views_at_mnist_minis_shape():
    g = Golden("mnist_mini")
    net, o = g.net(DEV), orc.Oracle(g.net("cpu"))
    ca, conf = net.transf.crs_attn, g.conf
    D, Tn = conf.D, conf.n_token
    rows = rnd((B, 53, D), 5)
    qs = ca.scaled_query()
    for view in (wc.transposed, wc.row_strided):
        v = view(rows)
        assert torch.equal(v, rows) and not v.is_contiguous()
        sc = hip.scores(v, qs, ca.k_w.weight, ca.H, ca.D_k, Tn)
        attn = hip.attn_map(v, qs, ca.k_w.weight, ca.H, ca.D_k, Tn)
        assert torch.equal(sc, hip.scores(rows, qs, ca.k_w.weight, ca.H, ca.D_k, Tn))
        assert torch.equal(attn, hip.attn_map(rows, qs, ca.k_w.weight, ca.H, ca.D_k, Tn))
        for b in range(B):
            ws, wa = o.scores(rows[b].cpu().numpy(), want_attn=True)
            assert ulp_diff(sc[b].cpu().numpy(), ws) == 0 and ulp_diff(attn[b].cpu().numpy(), wa) == 0
    mem = rnd((B, conf.M, D), 6)
    want = o.aggregate(mem.cpu().numpy())
    for view in (wc.transposed, wc.row_strided):
        with torch.no_grad():
            got = hip.aggregate(net.transf, view(mem))
        assert ulp_diff(got.cpu().numpy(), want) == 0, view.__name__
    emb = torch.from_numpy(want).to(DEV)
    for task in net.tasks.values():
        lin = net.output_layers[task["name"]][0]
        w, bias = orc._np(lin.weight), orc._np(lin.bias)
        ref = np.empty((B, w.shape[0]), dtype=np.float32)
        for b in range(B):
            orc.lib().orc_head(orc._f(want[b, task["id"]])[1], D, orc._f(w)[1], orc._f(bias)[1], w.shape[0],
                               0 if task["act_fn"] == "softmax" else 1, ref[b].ctypes.data_as(orc.f32p))
        for view in (wc.transposed, wc.row_strided):
            got = hip.head(view(emb), task["id"], lin, task["act_fn"])
            assert ulp_diff(got.cpu().numpy(), ref) == 0, (task["name"], view.__name__)


# ---------------------------------------------------------------- gather_rows
@pytest.mark.parametrize("dtype,width", [(torch.float32, 5), (torch.uint8, 3)])
def test_gather_rows_views(dtype, width):
    M = 4
    src = wc.ints((B, 9, width), 200, 2, DEV, dtype)
    idx = wc.ints((M, B), 9, 0, DEV).t()                        # (M, B).t()
    assert not idx.is_contiguous()
    want = torch.gather(src, 1, idx.unsqueeze(-1).expand(-1, -1, width))
    assert torch.equal(hip.gather_rows(src, idx), want)
    assert torch.equal(hip.gather_rows(wc.permuted(src), idx), want)
    one = src[:1].expand(B, -1, -1)                              # one image's table for the whole batch
    assert torch.equal(hip.gather_rows(one, idx), torch.gather(one, 1, idx.unsqueeze(-1).expand(-1, -1, width)))


# ---------------------------------------------------------------- patchify / patchify_sparse / dequant_patches
@pytest.mark.parametrize("patch,stride", [((32, 32), (32, 32)), ((10, 7), (3, 5))])
def test_patchify_views(patch, stride):
    big = rnd((B, 1, 70, 75), 8)
    crop = big[:, :, 3:67, 5:69]                                 # a crop: not contiguous
    rgb = rnd((B, 3, 64, 64), 9).contiguous(memory_format=CL)     # a channels-last image
    shifted = wc.off4(crop.contiguous())                         # 4 mod 16: the scalar route ipsx_patchify selects itself
    for img in (crop, rgb, shifted):
        got = hip.patchify(img, patch, stride)
        for b in range(B):
            assert torch.equal(got[b], _unfold(img[b], patch, stride))


def test_patchify_sparse_views():
    Hc, Wc, Cc, patch, stride = 40, 48, 1, (32, 32), (8, 16)
    g = np.random.default_rng(11)
    per = [7, 5]
    flat = np.concatenate([g.choice(Hc * Wc * Cc, n, replace=False) for n in per]).astype(np.int64)
    val = g.standard_normal(sum(per)).astype(np.float32)
    val[2] = 0.0                                                 # a stored zero: lands in the patches, sets no flag
    dense = np.zeros((B, Hc * Wc * Cc), dtype=np.float32)
    offs = np.concatenate([[0], np.cumsum(per)])
    for b in range(B):
        dense[b, flat[offs[b]:offs[b + 1]]] = val[offs[b]:offs[b + 1]]
    images = torch.from_numpy(dense.reshape(B, Hc, Wc, Cc)).permute(0, 3, 1, 2)
    want = torch.stack([_unfold(images[b], patch, stride) for b in range(B)])
    flags = (want != 0).flatten(2).any(2).flatten().to(torch.int32)
    index, value = torch.from_numpy(flat).to(DEV), torch.from_numpy(val).to(DEV)
    offsets = torch.from_numpy(offs.astype(np.int64)).to(DEV)
    got, nb = hip.patchify_sparse(wc.row_strided(index), wc.row_strided(value), offsets, (Hc, Wc, Cc), patch, stride, flags=True)
    assert torch.equal(got.cpu(), want) and torch.equal(nb.cpu(), flags)


def test_dequant_patches_views():
    table = rnd((3, 256), 12)
    q = wc.ints((B, 5, 3, 4, 6), 256, 1, DEV, torch.uint8)
    view = q.permute(1, 0, 2, 3, 4).contiguous().permute(1, 0, 2, 3, 4)
    assert torch.equal(view, q) and not view.is_contiguous()
    want = table[torch.arange(3, device=DEV).view(1, 1, 3, 1, 1), q.long()]
    assert torch.equal(hip.dequant_patches(view, table), want)


# ---------------------------------------------------------------- the training step's kernels
@pytest.mark.parametrize("P,ci,co,k,s,Hm", [(5, 64, 128, 3, 2, 8), (3, 64, 64, 3, 1, 8)])
def test_conv_gradient_views(P, ci, co, k, s, Hm):
    pad, Ho = 1, (Hm + 2 - k) // s + 1
    w = (rnd((co, ci, k, k), 13) * 0.05)
    x = rnd((P, ci, Hm, Hm), 14).contiguous(memory_format=CL)
    dy = rnd((P, co, Ho, Ho), 15).contiguous(memory_format=CL)
    one = dy[:1].expand(P, -1, -1, -1)                           # one map's gradient for every image
    for grad, compact in ((dy.contiguous(), dy), (one, one.contiguous(memory_format=CL))):      # NCHW-contiguous; expanded
        assert not grad.is_contiguous(memory_format=CL)
        xs = x.double().requires_grad_()
        ws = w.double().requires_grad_()
        F.conv2d(xs, ws, None, s, pad).backward(grad.double())
        dx = hip.conv2d_nhwc_dgrad(grad, w, s, pad, (Hm, Hm))
        dw = hip.conv2d_nhwc_wgrad(x, grad, (co, ci, k, k), s, pad)
        assert torch.equal(dx, hip.conv2d_nhwc_dgrad(compact, w, s, pad, (Hm, Hm)))
        assert torch.equal(dw, hip.conv2d_nhwc_wgrad(x, compact, (co, ci, k, k), s, pad))
        assert _rel(dx.double(), xs.grad) < 2e-6 and _rel(dw.double(), ws.grad) < 1e-5


def test_maxpool_views():
    x = torch.relu(rnd((3, 32, 16, 16), 16) - 0.4)                # NCHW-contiguous, post-ReLU-like: windows of equal zeros
    dy = rnd((3, 32, 8, 8), 17)
    xs = x.clone().requires_grad_()
    want = F.max_pool2d(xs, 3, 2, 1)
    want.backward(dy)
    got = hip.maxpool_3x3s2_nhwc(x)
    assert got.is_contiguous(memory_format=CL) and torch.equal(got, want.detach())
    assert torch.equal(hip.maxpool_3x3s2_bwd_nhwc(x, dy), xs.grad)


def test_bn_train_views():
    P, Cn, Hm = 5, 64, 8
    x = (rnd((P, Cn, Hm, Hm), 18) * 2 + 3).contiguous(memory_format=CL)
    dy = rnd((P, Cn, Hm, Hm), 19).contiguous(memory_format=CL)
    gamma, beta = rnd((Cn,), 20).abs() + 0.5, rnd((Cn,), 21)
    rm0, rv0 = rnd((3 * Cn,), 22), rnd((3 * Cn,), 23).abs() + 0.5
    base_rm, base_rv = rm0[Cn:2 * Cn].clone(), rv0[Cn:2 * Cn].clone()
    y0, mean0, invstd0 = hip.bn_train_forward(x, None, gamma, beta, 1e-5, 0.1, base_rm, base_rv, True)
    buf_m, buf_v = rm0.clone(), rv0.clone()
    y, mean, invstd = hip.bn_train_forward(x, None, wc.row_strided(gamma), wc.row_strided(beta), 1e-5, 0.1,
                                           buf_m[Cn:2 * Cn], buf_v[Cn:2 * Cn], True)
    assert torch.equal(y, y0) and torch.equal(mean, mean0) and torch.equal(invstd, invstd0)
    # the running statistics: updated where they lie, nothing around them touched
    assert torch.equal(buf_m[Cn:2 * Cn], base_rm) and torch.equal(buf_v[Cn:2 * Cn], base_rv)
    for buf, orig in ((buf_m, rm0), (buf_v, rv0)):
        assert torch.equal(buf[:Cn], orig[:Cn]) and torch.equal(buf[2 * Cn:], orig[2 * Cn:])
    xs, gs, bs = x.clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    want = torch.relu(F.batch_norm(xs.double(), rm0[Cn:2 * Cn].double(), rv0[Cn:2 * Cn].double(), gs.double(), bs.double(), True, 0.1, 1e-5))
    want.backward(dy.double())
    ref_mean, ref_var = x.double().mean((0, 2, 3)), x.double().var((0, 2, 3), unbiased=False)
    n = P * Hm * Hm
    assert _rel(y.double(), want.detach()) < 2e-6
    assert _rel(mean.double(), ref_mean) < 1e-6 and _rel(invstd.double(), 1 / torch.sqrt(ref_var + 1e-5)) < 1e-6
    assert _rel(buf_m[Cn:2 * Cn].double(), 0.9 * rm0[Cn:2 * Cn].double() + 0.1 * ref_mean) < 1e-6
    assert _rel(buf_v[Cn:2 * Cn].double(), 0.9 * rv0[Cn:2 * Cn].double() + 0.1 * ref_var * n / (n - 1)) < 1e-6
    dx0 = hip.bn_train_backward(dy, y, x, gamma, mean, invstd, True, False)
    dx, _, dgamma, dbeta = hip.bn_train_backward(dy, y, x, wc.row_strided(gamma), mean, invstd, True, False)
    assert torch.equal(dx, dx0[0]) and torch.equal(dgamma, dx0[2]) and torch.equal(dbeta, dx0[3])
    assert _rel(dx.double(), xs.grad.double()) < 2e-5 and _rel(dgamma.double(), gs.grad.double()) < 2e-5
    assert _rel(dbeta.double(), bs.grad.double()) < 2e-5
