"""Shared helpers of the test-suite: golden fixtures, deterministic nets and inputs."""

import collections
import hashlib
import json
import os

import numpy as np
import torch

from ips_amd import synth
from ips_amd.architecture import IPSNet

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

GOLDEN_CASES = sorted(f[:-4] for f in os.listdir(GOLDEN_DIR)
                      if f.endswith(".npz") and not f.startswith(("loop_", "bench_", "seeds_", "margin", "bf16_trunk")))
# what the CPU oracle replays in seconds (the rest is checked on the GPU only)
ORACLE_FAST_CASES = [c for c in GOLDEN_CASES if c not in ("traffic_full", "mnist_native50")]


class Golden:
    def __init__(self, name):
        z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
        self.name = name
        self.conf = synth.Conf(**json.loads(str(z["conf"])))
        self.B = int(z["B"])
        self.weight_seed, self.patch_seed, self.torch_seed = (int(z[k]) for k in
                                                              ("weight_seed", "patch_seed", "torch_seed"))
        self.trace_idx = z["trace_idx"]          # (B, n_iter, M)
        self.trace_score = z["trace_score"]
        self.mem_idx = self.trace_idx[:, -1]
        self.min_rel_gap = float(z["min_rel_gap"])
        self.emb_head = z["emb_head"]
        self.state_checksum = float(z["state_checksum"])
        self.perm = z["perm"] if "perm" in z.files else None
        self.preds = {k[5:]: z[k] for k in z.files if k.startswith("pred_")}
        self.mem_patch_sum = z["mem_patch_sum"]
        self.mem_pos_sum = z["mem_pos_sum"] if "mem_pos_sum" in z.files else None

    def net(self, device="cpu"):
        net = IPSNet(torch.device(device), self.conf)
        synth.fill_weights(net, self.weight_seed)
        chk = float(sum(v.double().abs().sum().item() for k, v in net.state_dict().items()
                        if not k.endswith("num_batches_tracked")))
        assert abs(chk - self.state_checksum) <= 1e-9 * abs(self.state_checksum), "weights differ from fixture"
        return net.to(device).eval()

    def patches(self):
        return synth.make_patches(self.conf, self.B, seed=self.patch_seed)

    def shuffled(self, x):
        """patches in the order ips() sees them (applies the fixture's permutation)."""
        if self.perm is None:
            return x
        take = torch.from_numpy(self.perm).view(x.shape[0], -1, *(1,) * (x.dim() - 2)).expand_as(x)
        return torch.gather(x, 1, take)


def row_digests(rows):
    """(n, 16) uint8: blake2b-16 of every row's bytes (C order, little-endian float32) - bytewise identity of a row, so
    -0.0 and +0.0 differ (tests/golden/bf16_trunk.npz, tools/gen_golden_bf16_trunk.py)"""
    rows = np.ascontiguousarray(rows, dtype="<f4")
    out = np.empty((rows.shape[0], 16), dtype=np.uint8)
    for k, r in enumerate(rows):
        out[k] = np.frombuffer(hashlib.blake2b(r.tobytes(), digest_size=16).digest(), dtype=np.uint8)
    return out


def max_rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def ulp_diff(a, b):
    """max distance in units in the last place between two float32 arrays"""
    a = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7FFFFFFF), a)
    b = np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return int(np.abs(a - b).max()) if a.size else 0


# ---------------------------------------------------------------- head shapes no shipped configuration uses
# Every fixture runs H = 8 (4), n_token <= 4, D in {32, 128, 512} and D_k = D / H, so R = H * n_token <= 32.  This table
# reaches the kernels' other shape-picked paths (tests/test_head_shapes.py on the GPU; the oracle's float64 anchor at the
# same shapes in tests/test_oracle_props.py):
#   R = 33, 40, 64, 96, 128, 256: 2, 3, 4 and 8 column tiles of the logits, partial last tiles;
#   R = 32 with n_token = 1 and 2: the generic selection loop instead of the LDS-resident one;
#   D = 64 (8 k-groups: the logits' 8-group tail only), 96 (tail + scalar remainder), 160 (a 16-group trip + remainder),
#   192 (trip + tail), 512 (trips only), 36 (D % 8 != 0: the masked scalar logits path - no aggregation, which needs
#   D % 32 == 0);  D_k above and below D / H, D_v != D_k;  n_token = 8 at D = 512, D_inner = 2048 (112 KiB of token
#   state: the aggregation's tail above 64 KiB of LDS);  n_class = 1, 10, 65 and 130 under softmax and sigmoid heads.
def _heads(n_token):
    """a softmax and a sigmoid task, on the first and the last token"""
    return {'task0': {'id': 0, 'name': 'soft', 'act_fn': 'softmax', 'metric': 'accuracy'},
            'task1': {'id': n_token - 1, 'name': 'sig', 'act_fn': 'sigmoid', 'metric': 'auc'}}


def _feat(D, H, T, Dk, Dv, Di, n_class, use_pos=False, N=180, M=16, I=48):
    return synth.camelyon_conf(N=N, M=M, I=I, n_chan_in=64, D=D, H=H, n_token=T, D_k=Dk, D_v=Dv, D_inner=Di,
                               n_class=n_class, use_pos=use_pos, tasks=_heads(T))


HEAD_SHAPES = {
    # name: (configuration, weight seed, runs the aggregation)
    "r33_d64": (_feat(64, 11, 3, 8, 12, 96, 65), 301, True),
    "r40_d160": (_feat(160, 8, 5, 24, 16, 256, 130, use_pos=True), 302, True),
    "r64_d192": (_feat(192, 16, 4, 8, 20, 128, 1), 303, True),
    "r96_d36": (_feat(36, 12, 8, 5, 4, 64, 65), 304, False),
    "r128_d96": (_feat(96, 32, 4, 4, 3, 64, 65, use_pos=True), 305, True),
    "r256_d512": (_feat(512, 32, 8, 16, 16, 2048, 130), 306, True),
    "r32t1_d128": (_feat(128, 32, 1, 6, 5, 160, 1), 307, True),
    "r32t2_mnist": (synth.mnist_conf(N=100, M=8, I=40, H=16, n_token=2, D_k=12, D_v=10, D_inner=256, n_class=65,
                                     tasks=_heads(2)), 308, True),
}


def head_shape_net(name, device="cpu"):
    conf, seed, _ = HEAD_SHAPES[name]
    net = IPSNet(torch.device(device), conf)
    synth.fill_weights(net, seed)
    return net.to(device).eval()


def head_shape_net64(name):
    """the same net in float64 on the CPU: its plain torch modules are the yardstick"""
    return head_shape_net(name).double()


def f64_logits(net64, x, pos=None):
    """Attention logits (L, H*n_token) of rows x (+ pos) through the float64 net's q_w / k_w, and per element the scale
    sum_c |x_c| sum_j |qs_j| |k_w[j, c]| that bounds the rounding of any fp32 order of the contraction."""
    ca = net64.transf.crs_attn
    H, T, Dk = ca.H, ca.n_token, ca.D_k
    x = torch.as_tensor(np.asarray(x)).double()
    if pos is not None:
        x = x + torch.as_tensor(np.asarray(pos)).double()
    with torch.no_grad():
        qs = (ca.q_w(ca.q[0]) / ca.attention.temperature).view(T, H, Dk)
        k = ca.k_w(x).view(-1, H, Dk)
        lg = torch.einsum("thj,lhj->lht", qs, k).reshape(-1, H * T)
        wk = ca.k_w.weight.view(H, Dk, -1)
        absv = torch.einsum("thj,hjc->htc", qs.abs(), wk.abs()).reshape(H * T, -1)
        scale = x.abs() @ absv.T
    return lg.numpy(), scale.numpy()


def rel_err(got, want, floor=0.0):
    """largest per-element |got - want| / max(|want|, floor)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float((np.abs(got - want) / np.maximum(np.abs(want), floor)).max()) if want.size else 0.0


# Bounds of the oracle (so of any kernel bitwise equal to it) against the float64 nets on head_shape_inputs, per element:
# logits |err| / f64_logits' scale, scores / attention maps / predictions relative to the float64 value.  Measured worst
# case over HEAD_SHAPES: 2.3e-7, 7.3e-6, 1.8e-5, 4.3e-6 (tests/test_oracle_props.py lists them per configuration).
HEAD_F64_BOUNDS = {"logits": 1e-6, "scores": 3e-5, "attn": 1e-4, "preds": 2e-5}


def head_shape_scores_lengths(name):
    """53 candidates, and a candidate set past the 160 KiB LDS staging of the scores kernel (L (R + 1) 4 + 8 R bytes)"""
    ca = HEAD_SHAPES[name][0]
    R = ca.H * ca.n_token
    return 53, (160 * 1024 - 8 * R) // ((R + 1) * 4) + 40


def head_shape_inputs(name):
    """Deterministic inputs of one configuration: logits rows x / pos (2, 333, D), scores rows per length, and a memory
    (2, M, ...) with positional rows for forward()."""
    conf, seed, _ = HEAD_SHAPES[name]
    g = np.random.default_rng(seed)
    D = conf.D
    out = {"x": g.standard_normal((2, 333, D)).astype(np.float32), "pos": g.standard_normal((2, 333, D)).astype(np.float32)}
    for L in head_shape_scores_lengths(name):
        out["rows%d" % L] = g.standard_normal((2, L, D)).astype(np.float32)
    out["mem_patch"] = synth.make_patches(conf, 2, seed=seed, N=conf.M, blank_frac=0.3).numpy()
    out["mem_pos"] = (0.5 * g.standard_normal((2, conf.M, D))).astype(np.float32) if conf.use_pos else None
    return out


# ---------------------------------------------------------------- layer-by-layer convolutions over a geometry lattice
# conv_any_kernel (NCHW, any C_in; csrc/conv.hip) and conv_nhwc_kernel (csrc/conv_nhwc.hip) on the GPU in
# tests/test_conv_lattice.py, the oracle alone in tests/test_oracle_props.py; conv_nhwc_bf16_kernel in
# tests/test_conv_bf16_lattice.py.  One pad for both axes, as the ABI has it.
ConvCase = collections.namedtuple("ConvCase", "c_in c_out kh kw stride pad h w n res relu affine")
# affine: "as" alpha and shift, "a" alpha alone, "s" shift alone, "-" neither - the epilogues read
# `alpha ? fma(v, alpha, shift ? shift : 0) : shift ? v + shift : v`
_T, _F = True, False

CONV_LATTICE_NCHW = [ConvCase(*c) for c in [
    # c_in, c_out, kh, kw, stride, pad, h, w, n, residual, relu, affine
    # -- output-pixel totals at the half (32), wave (64) and workgroup (256) edges, from 1x1 and 2x2 output maps: an even
    #    total once with howo % 4 == 0 (float4 stores) and once with howo = 1 (scalar stores; img = m / howo is the identity)
    (1, 1, 1, 1, 1, 0, 1, 1, 1, _F, _F, "as"),       # 1 pixel, 1 channel, K = 1: one lane of one tile does all the work
    (3, 31, 3, 3, 1, 0, 3, 3, 31, _T, _T, "as"),     # 31 pixels: 1x1 outputs of pad = 0 under k = 3; K = 27, C_out = 31
    (5, 33, 1, 1, 1, 0, 1, 1, 32, _T, _F, "a"),      # 32, scalar; K = 5 with C_out = 33: K % 8 != 0 and C_out % 32 != 0 in the packing
    (2, 32, 2, 2, 1, 0, 3, 3, 8, _F, _T, "s"),       # 32, float4 (2x2 outputs); even kernel, K = 8: one whole k-group
    (8, 64, 3, 3, 1, 1, 1, 1, 33, _F, _T, "as"),     # 33; a 1x1 map under 3x3 / pad 1: narrower than the kernel, only the centre tap is real
    (12, 65, 1, 1, 2, 0, 2, 2, 63, _T, _T, "as"),    # 63; stride 2 picks one pixel of a 2x2 map; C_out = 65: one channel in the 2nd workgroup column
    (3, 100, 1, 1, 1, 0, 1, 1, 64, _F, _F, "-"),     # 64, scalar; no affine, no residual, no ReLU: the bare chain
    (1, 64, 3, 3, 2, 1, 3, 3, 16, _T, _T, "as"),     # 64, float4: 3x3 / stride 2 / pad 1 on 3x3 -> 2x2
    (33, 32, 1, 1, 1, 0, 1, 1, 65, _F, _T, "s"),     # 65: the second wave holds one pixel; C_in = 33
    (2, 33, 1, 1, 3, 0, 3, 3, 255, _F, _F, "as"),    # 255; stride 3
    (5, 31, 2, 2, 1, 0, 2, 2, 256, _T, _T, "as"),    # 256, scalar: 2x2 kernel on 2x2 maps -> 1x1
    (8, 65, 2, 2, 2, 1, 2, 2, 64, _F, _T, "a"),      # 256, float4: 2x2 / stride 2 / pad 1 = k - 1 on 2x2 -> 2x2, every window one real tap
    (3, 1, 1, 1, 1, 0, 1, 1, 257, _T, _F, "s"),      # 257: the second workgroup holds one pixel
    (12, 100, 3, 1, 1, 1, 2, 2, 33, _T, _T, "as"),   # 264 = 256 + 8 with howo = 8: float4 stores in a ragged last workgroup; 3x1 kernel
    (1, 33, 1, 1, 1, 0, 2, 2, 9, _F, _T, "as"),      # 36 = 32 + 4 with howo = 4: float4 stores, the second half of a wave holds one quad
    # -- kernels that are not square, even kernels, stride 3, pad in {0, (k-1)/2, k-1, k+1}
    (3, 33, 1, 3, 1, 0, 5, 7, 2, _F, _T, "as"),      # 1x3, no pad: 5x5 outputs
    (5, 64, 5, 3, 1, 2, 7, 6, 2, _T, _F, "s"),       # 5x3, pad (kh-1)/2 = kw-1: 7x8 outputs (float4), residual without ReLU
    (2, 31, 5, 3, 2, 4, 6, 5, 3, _F, _T, "as"),      # 5x3 / stride 2, pad kh-1 = kw+1: corner windows lie wholly in padding
    (8, 100, 1, 3, 2, 1, 6, 9, 5, _T, _T, "a"),      # 1x3 / stride 2 / pad 1 (= kh: whole rows of padding): 4x5 outputs, 100 pixels
    (12, 64, 3, 1, 3, 1, 10, 4, 4, _F, _T, "as"),    # 3x1 / stride 3 / pad 1: 4x2 outputs
    (1, 32, 7, 7, 1, 3, 13, 13, 1, _F, _T, "as"),    # 7x7 same-size on 13x13 (169 pixels, not a multiple of 4)
    (3, 65, 7, 7, 2, 3, 13, 11, 2, _T, _T, "as"),    # the 3-channel stem's shape on an odd map, C_out = 65
    (3, 64, 7, 7, 3, 6, 9, 9, 1, _F, _F, "a"),       # 7x7 / stride 3 / pad k-1: 5x5 outputs
    (8, 33, 3, 3, 1, 4, 4, 4, 2, _T, _T, "as"),      # pad k+1: 10x10 outputs, the outer two rings are exactly shift + res
    (1, 100, 3, 3, 1, 2, 5, 5, 1, _F, _F, "-"),      # pad k-1: a corner output sees one pixel; no epilogue at all
    (2, 1, 2, 2, 1, 3, 3, 3, 2, _F, _T, "s"),        # 2x2, pad k+1: 8x8 outputs, C_out = 1
    (12, 31, 2, 2, 2, 1, 7, 7, 3, _T, _F, "as"),     # 2x2 / stride 2 / pad k-1 on an odd map: 4x4 outputs
    (5, 32, 3, 3, 3, 1, 11, 13, 2, _F, _T, "as"),    # 3x3 / stride 3: 4x5 outputs, the windows skip columns
    (33, 100, 3, 3, 2, 0, 9, 9, 3, _T, _T, "as"),    # C_in = 33 (K = 297 = 37 k-groups + 1), pad 0 under stride 2: 4x4 outputs
    (33, 65, 1, 1, 1, 0, 13, 13, 2, _F, _F, "s"),    # 1x1 on 13x13: 338 pixels, two workgroups, K = 33
    (2, 65, 1, 1, 1, 2, 3, 3, 4, _F, _F, "as"),      # 1x1 kernel with pad k+1 = 2: 7x7 outputs of which 9 see data
    (12, 1, 7, 7, 1, 8, 2, 2, 1, _F, _F, "as"),      # pad k+1 = 8 round a 2x2 map: 12x12 outputs (float4), C_out = 1
    (5, 100, 3, 3, 1, 0, 6, 4, 3, _T, _T, "s"),      # pad 0 under k = 3, stride 1: 4x2 outputs
    (8, 31, 3, 3, 2, 2, 5, 5, 2, _F, _T, "a"),       # pad k-1 under stride 2: 4x4 outputs
    # -- maps narrower than the kernel, the widest kernel, the largest k table
    (3, 32, 3, 3, 1, 1, 2, 9, 3, _F, _T, "as"),      # 2 rows under a 3x3 kernel
    (5, 100, 5, 3, 1, 1, 3, 13, 2, _T, _T, "as"),    # 3 rows under a 5-row kernel, pad 1: ONE output row of 13
    (1, 33, 31, 31, 1, 15, 4, 4, 2, _T, _T, "as"),   # 31x31 taps (every bit of the row / column masks), K = 961, on 4x4 maps
    (8, 31, 31, 31, 1, 15, 3, 2, 1, _F, _T, "s"),    # K = 7688: a k table of 61.5 KiB, just under its 64 KiB gate
    (2, 64, 31, 1, 2, 15, 5, 3, 2, _F, _F, "as"),    # 31x1 / stride 2: 3x17 outputs, most of them padding columns
    (12, 33, 1, 1, 1, 0, 1, 1, 1, _T, _T, "as"),     # 1 pixel again, with every epilogue step, C_out one over a tile
]]

CONV_LATTICE_NHWC = [ConvCase(*c) for c in [
    # Dispatches by C_out: <= 64 (workgroup 256 pixels x 64 channels), 65 .. 255 (128 x 128), >= 256 (64 x 256).
    # A stage is 8 of K = kh kw C_in; three stages are primed ahead of a loop of four.
    # -- stage counts against the ring: 4 (= one trip, every primed load past the end re-reads the last stage), 8, 12
    (32, 32, 1, 1, 1, 0, 1, 1, 1, _F, _F, "as"),     # 4 stages, 1 pixel, 1x1 map
    (32, 8, 1, 1, 1, 0, 5, 5, 3, _T, _T, "as"),      # 4 stages, C_out = 8: a quarter of an n-tile
    (32, 96, 1, 1, 1, 0, 3, 3, 5, _F, _T, "s"),      # 4 stages in the middle dispatch: n-tile 3 is a clamped re-read of tile 2
    (32, 264, 1, 1, 1, 0, 2, 2, 3, _T, _F, "a"),     # 4 stages in the wide dispatch, C_out = 256 + 8
    (64, 33, 1, 1, 1, 0, 3, 3, 3, _F, _T, "as"),     # 8 stages, C_out = 33: one channel in the second n-tile
    (64, 65, 1, 1, 2, 0, 5, 5, 2, _T, _T, "as"),     # 8 stages, C_out = 65: one channel for the wave along N, strided 1x1
    (96, 256, 1, 1, 1, 0, 2, 2, 4, _T, _T, "as"),    # 12 stages (C_in = 96), whole tiles of the wide dispatch
    (32, 64, 1, 3, 1, 0, 1, 3, 2, _F, _F, "-"),      # 12 stages from 3 taps; 1x3 kernel on a 1x3 map -> 1x1, the bare chain
    # -- workgroup edges in M: 255 / 256 / 257 (C_out <= 64), 127 / 128 / 129 (middle), 63 / 64 / 65 (wide)
    (32, 33, 1, 1, 1, 0, 1, 1, 255, _F, _T, "as"),
    (32, 64, 2, 2, 1, 0, 2, 2, 256, _T, _F, "a"),    # 2x2 kernel on 2x2 maps -> 1x1; even kernel, 16 stages
    (64, 32, 1, 1, 1, 0, 1, 1, 257, _F, _F, "s"),
    (32, 160, 1, 1, 1, 0, 1, 1, 127, _T, _T, "as"),
    (64, 160, 3, 3, 2, 1, 3, 3, 32, _F, _T, "as"),   # 128 = 32 x (2x2 outputs)
    (32, 255, 1, 1, 1, 0, 1, 1, 129, _F, _F, "s"),   # C_out = 255: the last channel of the last tile is missing
    (32, 288, 1, 1, 1, 0, 1, 1, 63, _F, _T, "as"),   # C_out = 288 = 256 + 32: the second workgroup column has one live wave
    (32, 544, 3, 3, 1, 0, 3, 3, 64, _T, _T, "as"),   # pad 0 under k = 3: 1x1 outputs; C_out = 544 = 2 x 256 + 32: three columns
    (64, 264, 1, 1, 1, 0, 1, 1, 65, _T, _F, "a"),
    # -- kernels that are not square, even kernels, stride 3, pad in {0, (k-1)/2, k-1, k+1}, narrow maps
    (32, 65, 1, 3, 1, 1, 4, 5, 2, _F, _T, "as"),     # 1x3 / pad 1 (= kh): 6x5 outputs, the first and last rows are padding
    (32, 32, 3, 1, 2, 1, 7, 4, 3, _T, _T, "as"),     # 3x1 / stride 2 / pad 1: 4x3 outputs
    (32, 96, 5, 3, 1, 2, 6, 5, 2, _T, _F, "s"),      # 5x3, pad (kh-1)/2 = kw-1: 6x7 outputs, residual without ReLU
    (64, 64, 5, 3, 2, 4, 6, 5, 2, _F, _T, "as"),     # 5x3 / stride 2, pad kh-1 = kw+1: corner windows wholly in padding
    (32, 256, 7, 7, 2, 3, 13, 11, 1, _F, _T, "as"),  # 7x7 / stride 2 on an odd map: 196 stages, 7x6 outputs
    (32, 33, 7, 7, 3, 6, 9, 9, 2, _T, _T, "a"),      # 7x7 / stride 3 / pad k-1: 5x5 outputs
    (32, 160, 2, 2, 2, 1, 7, 7, 3, _F, _F, "as"),    # 2x2 / stride 2 / pad k-1: 4x4 outputs
    (64, 8, 2, 2, 1, 3, 3, 3, 2, _T, _T, "as"),      # 2x2, pad k+1: 8x8 outputs, the outer rings exactly shift + res
    (96, 288, 3, 3, 1, 4, 2, 2, 1, _T, _T, "as"),    # 3x3, pad k+1 round a 2x2 map: 8x8 outputs, 4 of 64 windows see data
    (32, 255, 3, 3, 1, 2, 5, 5, 1, _F, _F, "-"),     # pad k-1: a corner output sees one pixel; no epilogue at all
    (96, 64, 3, 3, 3, 1, 11, 13, 2, _F, _T, "s"),    # 3x3 / stride 3: 4x5 outputs
    (64, 96, 3, 3, 2, 0, 9, 9, 3, _T, _T, "as"),     # pad 0 under stride 2: 4x4 outputs
    (32, 264, 1, 1, 3, 0, 7, 7, 2, _F, _T, "as"),    # 1x1 / stride 3: 3x3 outputs
    (32, 33, 1, 1, 1, 2, 3, 3, 4, _F, _F, "as"),     # 1x1 kernel with pad k+1 = 2: 7x7 outputs of which 9 see data
    (64, 65, 3, 3, 1, 1, 1, 1, 33, _T, _T, "as"),    # 1x1 maps under 3x3 / pad 1: only the centre tap is real
    (32, 544, 3, 3, 1, 1, 2, 9, 2, _F, _T, "s"),     # 2 rows under a 3x3 kernel
    (96, 32, 5, 3, 1, 1, 3, 13, 2, _T, _F, "as"),    # 3 rows under a 5-row kernel, pad 1: ONE output row of 13
    (32, 8, 31, 1, 2, 15, 5, 3, 2, _F, _T, "as"),    # 31x1 / stride 2: 3x17 outputs, most of them padding columns
    # -- C_out one under / over the tiles that are left, the other C_in, long chains
    (160, 64, 3, 3, 1, 1, 5, 7, 2, _T, _T, "as"),    # C_in = 160: 20 stages per tap, 180 in all
    (160, 544, 3, 3, 1, 1, 4, 4, 5, _T, _T, "as"),   # the long case in the wide dispatch: 80 pixels, a ragged second row tile
    (160, 160, 1, 1, 1, 0, 13, 13, 1, _F, _T, "a"),  # 20 stages, 169 pixels: two workgroups of the middle dispatch
    (96, 255, 3, 3, 2, 1, 13, 13, 2, _T, _F, "as"),  # 7x7 outputs x 2 = 98 pixels
    (64, 256, 3, 3, 1, 1, 13, 13, 1, _F, _T, "s"),   # 169 pixels: three row tiles of the wide dispatch, the last of 41
]]


def conv_case_id(c):
    return "%dto%d_k%dx%d_s%d_p%d_%dx%d_n%d_%s%s%s" % (c.c_in, c.c_out, c.kh, c.kw, c.stride, c.pad, c.h, c.w, c.n,
                                                       c.affine.replace("-", "none"), "_res" if c.res else "", "_relu" if c.relu else "")


def conv_case_out(c):
    """(ho, wo) of a case"""
    return (c.h + 2 * c.pad - c.kh) // c.stride + 1, (c.w + 2 * c.pad - c.kw) // c.stride + 1


def conv_case_inputs(c, seed):
    """x (n, C_in, h, w), OIHW weights, alpha / shift (C_out,) or None, residual (n, C_out, ho, wo) or None: float32"""
    g = np.random.default_rng(seed)
    ho, wo = conv_case_out(c)
    K = c.kh * c.kw * c.c_in

    def rnd(shape, scale=1.0):
        return (g.standard_normal(shape) * scale).astype(np.float32)

    x, wt = rnd((c.n, c.c_in, c.h, c.w)), rnd((c.c_out, c.c_in, c.kh, c.kw), (2.0 / K) ** 0.5)
    alpha, shift, r = (1 + 0.2 * rnd((c.c_out,))).astype(np.float32), rnd((c.c_out,), 0.1), rnd((c.n, c.c_out, ho, wo))
    return x, wt, (alpha if "a" in c.affine else None), (shift if "s" in c.affine else None), (r if c.res else None)


def conv_case_f64(c, x, wt, alpha, shift, r):
    """The float64 result e of a case (after the ReLU where there is one), per element the bound
    1.01 (K + 3) 2^-24 (|alpha| A + |shift| + |res|) with A = conv(|x|, |w|) - first order of a K-term fp32 fma chain in
    any order plus the two roundings of the epilogue; the ReLU does not widen it - and A itself (A == 0: a window wholly
    in padding)."""
    import torch.nn.functional as F
    xd, wd = torch.from_numpy(x).double(), torch.from_numpy(wt).double()
    co = (1, c.c_out, 1, 1)
    al = torch.from_numpy(alpha).double().view(co) if alpha is not None else torch.ones(co, dtype=torch.float64)
    sh = torch.from_numpy(shift).double().view(co) if shift is not None else torch.zeros(co, dtype=torch.float64)
    e = F.conv2d(xd, wd, None, c.stride, c.pad) * al + sh
    A = F.conv2d(xd.abs(), wd.abs(), None, c.stride, c.pad)
    scale = al.abs() * A + sh.abs()
    if r is not None:
        e = e + torch.from_numpy(r).double()
        scale = scale + torch.from_numpy(r).double().abs()
    if c.relu:
        e = torch.relu(e)
    K = c.kh * c.kw * c.c_in
    return e.numpy(), (1.01 * (K + 3) * 2.0 ** -24 * scale).numpy(), A.numpy()


def conv_bound_ratio(got, e, bound):
    """worst |got - e| / bound over the elements (an element with bound 0 must be exact: inf otherwise)"""
    err = np.abs(np.asarray(got, dtype=np.float64) - e)
    ratio = np.where(err == 0.0, 0.0, err / np.where(bound > 0.0, bound, 1.0))
    ratio = np.where((bound <= 0.0) & (err > 0.0), np.inf, ratio)
    return float(ratio.max())


def conv_case_oracle(c, x, wt, alpha, shift, r):
    """orc_conv2d_affine on a case: (n, C_out, ho, wo) float32"""
    import ctypes as C

    from oracle import oracle as orc
    ho, wo = conv_case_out(c)
    hold = [orc._f(a) if a is not None else (None, None) for a in (wt, alpha, shift, x, r)]
    cv = orc._Conv(c.c_in, c.c_out, c.kh, c.kw, c.stride, c.pad, hold[0][1], hold[1][1], hold[2][1])
    want = np.full((c.n, c.c_out, ho, wo), np.nan, dtype=np.float32)
    orc.lib().orc_conv2d_affine(C.byref(cv), hold[3][1], hold[4][1], want.ctypes.data_as(orc.f32p), C.c_int64(c.n),
                                c.h, c.w, int(c.relu))
    return want


def conv_padding_only_value(c, shift, r, A):
    """what an output whose window lies wholly in padding must be, exactly: relu(shift + res) in float32 (fma(0, alpha,
    shift) is shift); returns (mask of such outputs, their values)"""
    v = np.zeros(A.shape, dtype=np.float32)
    if shift is not None:
        v = v + shift.reshape(1, -1, 1, 1)
    if r is not None:
        v = (v + r).astype(np.float32)
    if c.relu:
        v = np.maximum(v, np.float32(0))
    return A == 0.0, v


# ---------------------------------------------------------------- the float64 emulation of one bf16 convolution
def r16(t):
    """rounded to bfloat16 (nearest even), as float64"""
    return t.float().to(torch.bfloat16).double()


def bf16_conv_emulation(x, wt, alpha, shift, stride, pad, r, relu, acc=torch.float64):
    """conv_nhwc_bf16_kernel's contract (csrc/conv_nhwc_bf16.hip) BEFORE its last rounding: x (n, h, w, C_in) and r
    (n, ho, wo, C_out) or None are the stored bfloat16 tensors, the float32 OIHW weights are rounded to bf16, the
    convolution is summed in float64, then affine (alpha / shift float32 or None), + r, ReLU.  (n, ho, wo, C_out) float64.
    acc = float32: ATen's fp32 convolution and a float32 epilogue in the kernel's place (fma-free: a reference-only
    figure for how far two correct fp32 evaluations lie from the float64 one)."""
    import torch.nn.functional as F
    e = F.conv2d(x.to(acc).permute(0, 3, 1, 2), r16(wt).to(acc), None, stride, pad).permute(0, 2, 3, 1)
    if alpha is not None:
        e = e * alpha.to(acc)
    if shift is not None:
        e = e + shift.to(acc)
    if r is not None:
        e = e + r.to(acc)
    if relu:
        e = torch.relu(e)
    return e.double()
