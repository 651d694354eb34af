"""The argument contract of every launching wrapper of ``ips_amd/hip.py`` and ``ips_amd/hip_train.py``, written
once: per wrapper a builder of valid arguments at the smallest useful shape, the launching exports a valid call reaches (in
order: recorded at the commit before the guards went in - a guard must not change what a correct call launches), the
buffers the kernel writes (handed over by their own address), the argument changes the wrapper ACCEPTS by normalising, the
changes it REFUSES, and the address alignment the kernel's widest access assumes, as read in csrc/.

No fixtures, no GPU: tests/test_wrapper_contract_cpu.py runs the table against a stand-in library that launches nothing;
tests/test_wrapper_views.py runs the accepted views on the GPU.

Alignment notes (``align``): ``16`` - the kernel reads or writes 16-byte units and its entry point has no scalar route, so a
read-only input at another address is copied and a written buffer refused; ``fallback`` - the C entry point tests the
addresses itself and takes a narrower route; ``4`` / ``8`` - the element's own size is all the kernel assumes; ``C`` - the C
entry point refuses a misaligned address before its launch; ``?`` - not settled by reading the code: held to 16 bytes."""

import collections

import torch
import torch.nn as nn

from ips_amd import hip, hip_train
from ips_amd.architecture.transformer import Transformer

Entry = collections.namedtuple("Entry", "name fn build launches written accept refuse align covers")
Accept = collections.namedtuple("Accept", "label arg view at layout copied align")      # at: (export, index of the pointer)

H, T, DK, D, R = 2, 4, 3, 24, 8          # the head of the small cases: R = H * T folded query rows of D
B, N, M, I = 2, 41, 4, 8                 # two images of 41 candidates, memory 4, chunk 8
CL = torch.channels_last


def rnd(shape, seed=0, dev="cpu"):
    g = torch.Generator().manual_seed(1234 + seed)
    return torch.randn(shape, generator=g).to(dev)


def ints(shape, hi, seed=0, dev="cpu", dtype=torch.int64):
    g = torch.Generator().manual_seed(99 + seed)
    return torch.randint(0, hi, shape, generator=g).to(dtype).to(dev)


# ---------------------------------------------------------------- views of a tensor that hold the same values
def transposed(t):
    """the last two axes swapped in memory"""
    return t.transpose(-1, -2).contiguous().transpose(-1, -2)


def permuted(t):
    """axes 1 and 2 of a 3-d tensor swapped in memory: ``(B, R, N).permute(0, 2, 1)``"""
    return t.permute(0, 2, 1).contiguous().permute(0, 2, 1)


def row_strided(t):
    """every second row (axis 1, or axis 0 of a 1-d / 2-d tensor) of a tensor twice as long"""
    ax = 1 if t.dim() >= 3 else 0
    shape = list(t.shape)
    shape[ax] *= 2
    big = torch.zeros(shape, dtype=t.dtype, device=t.device)
    view = big[:, ::2] if ax == 1 else big[::2]
    view.copy_(t)
    return view


def col_sliced(t):
    """columns 4 .. 4 + D of wider rows"""
    big = torch.zeros(t.shape[:-1] + (t.shape[-1] + 8,), dtype=t.dtype, device=t.device)
    view = big[..., 4:4 + t.shape[-1]]
    view.copy_(t)
    return view


def off4(t):
    """the same compact tensor one element further: for float32 an address that is 4 mod 16"""
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == t.element_size() and view.is_contiguous()
    return view


def expanded(t):
    """image 0 expanded over the batch (the tensor's images must be equal: builders use it on broadcast tables)"""
    return t[:1].expand(t.shape[0] if t.shape[0] > 1 else B, *t.shape[1:])


def nchw(t):
    """a channels-last tensor in NCHW memory"""
    return t.contiguous()


def row_range(t):
    """rows 3 .. 3 + n (axis 1) of a longer table: the ``out`` of a logits part"""
    big = torch.zeros((t.shape[0], t.shape[1] + 7) + tuple(t.shape[2:]), dtype=t.dtype, device=t.device)
    return big[:, 3:3 + t.shape[1]]


# ---------------------------------------------------------------- refusals
def to(dtype):
    def change(name):
        def apply(a):
            a[name] = a[name].to(dtype)
        return ("%s as %s" % (name, str(dtype).replace("torch.", "")), apply)
    return change


def put(name, make, label):
    def apply(a):
        a[name] = make(a)
    return ("%s: %s" % (name, label), apply)


f64, i32, i64, f16 = to(torch.float64), to(torch.int32), to(torch.int64), to(torch.float16)


def strided1(name):
    return put(name, lambda a: row_strided(a[name]), "every second element of a longer buffer")


def misaligned(name):
    return put(name, lambda a: off4(a[name]), "at an address 4 mod 16")


# ---------------------------------------------------------------- builders
def folded(dev, r=R, d=D, bf16=False):
    n = hip.lib().ipsx_folded_query_bf16_bytes(r, 1, d) if bf16 else hip.lib().ipsx_folded_query_elems(r, 1, d)
    return (torch.zeros(n, dtype=torch.uint8) if bf16 else rnd((n,), 7)).to(dev)


def b_logits(dev):
    return dict(emb=rnd((B, 33, D), 1, dev), pos=rnd((1, 33, D), 2, dev), vq=folded(dev), R=R, out=None, cond=None)


def b_logits_stats(dev):
    a = b_logits(dev)
    del a["cond"]
    a.update(out=torch.zeros((B, 33, R), device=dev), stats_x=rnd((5, 16), 3, dev), stats_out=torch.zeros((5, 2), device=dev), ln_eps=1e-5)
    return a


def b_scan(dev):
    return dict(lg=rnd((B, N, R), 4, dev), M=M, I=I, H=H, T=T)


def b_scan_state(dev, **more):
    a = b_scan(dev)
    a.update(it_begin=0, it_end=2, mem_idx=torch.zeros((B, M), dtype=torch.int64, device=dev),
             tie=torch.zeros((B,), dtype=torch.int32, device=dev))
    a.update(more)
    return a


def word(dev):
    return torch.zeros((1,), dtype=torch.int32, device=dev)


def b_scores(dev):
    return dict(x=rnd((B, 9, D), 5, dev), qs=rnd((T, H * DK), 6, dev), wk=rnd((H * DK, D), 7, dev), H=H, Dk=DK, T=T)


def b_finish(dev):
    return dict(src=rnd((B, 9, 4), 8, dev), pos=rnd((1, 9, 4), 9, dev), idx_buf=ints((B, M), 9, 1, dev), status=word(dev),
                status_host=torch.zeros((1,), dtype=torch.int32))


def b_ragged_rows(dev):
    return dict(rows=rnd((71, 4), 10, dev), offsets=torch.tensor([0, 41, 71], dtype=torch.int64, device=dev),
                mem_idx=ints((B, M), 30, 2, dev), M=M, flat=None, pos=rnd((71, 4), 11, dev))


def ragged_view():
    return hip.RaggedView(1, [(40, 48), (32, 64)], [0, 40 * 48], (32, 32), (8, 16))


def b_ragged_view(dev):
    rv = ragged_view()
    return dict(pixels=rnd((40 * 48 + 32 * 64,), 12, dev), rview=rv, offsets=torch.tensor([0, rv.lengths[0], rv.count], dtype=torch.int64, device=dev),
                mem_idx=ints((B, M), 3, 3, dev), M=M, flat=None, pos=None)


IMG = (2, 1, 40, 48)


def b_images(dev):
    return dict(img=rnd(IMG, 13, dev), patch_size=(32, 32), patch_stride=(8, 16))


def b_commit(dev):
    held = rnd((B, 8, 4), 14, dev)
    return dict(held=held, piece=rnd((B, 3, 4), 15, dev), sel=None)


def b_conv(dev, ci=64, co=64, n=3, hw=8):
    return dict(x=rnd((n, ci, hw, hw), 16, dev).contiguous(memory_format=CL), weight=rnd((co, ci, 3, 3), 17, dev), stride=1, pad=1)


def b_bn(dev):
    c = 64
    return dict(x=rnd((5, c, 8, 8), 18, dev).contiguous(memory_format=CL), residual=None, gamma=rnd((c,), 19, dev), beta=rnd((c,), 20, dev),
                eps=1e-5, momentum=0.1, running_mean=torch.zeros(c, device=dev), running_var=torch.ones(c, device=dev), relu=True)


def b_bn_bwd(dev):
    c = 64
    x = rnd((5, c, 8, 8), 18, dev).contiguous(memory_format=CL)
    return dict(dy=torch.ones_like(x), y=torch.relu(x), x=x, gamma=rnd((c,), 19, dev), mean=rnd((c,), 21, dev), invstd=rnd((c,), 22, dev).abs(),
                relu=True, want_residual=False)


def b_attn_pool(dev):
    return dict(x=rnd((2, 5, 32), 23, dev), A=rnd((8, 32), 24, dev), keep=None)


def b_attn_pool_bwd(dev):
    a = b_attn_pool(dev)
    a.update(P=rnd((2, 8, 5), 25, dev), Z=rnd((2, 8, 32), 26, dev), dZ=rnd((2, 8, 32), 27, dev))
    return a


def transformer(dev):
    with torch.random.fork_rng(devices=[]):          # (the global generator stays as the caller left it)
        torch.manual_seed(5)
        return Transformer(T, H, 32, DK, DK, 16).to(dev).eval()


def linear(dev, d=D, n_class=5):
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(6)
        return nn.Linear(d, n_class).to(dev)


def kw(fn, *names):
    """call ``fn`` with the named entries of the argument dict, in that order"""
    return lambda a: fn(*[a[n] for n in names])


def commit_tables(a):
    return [(a["held"], 2, a["piece"], a["held"])]


LOGITS_VIEWS = [
    Accept("emb transposed", "emb", transposed, ("ipsx_logits", 0), "contiguous", True, 16),
    Accept("emb every second row", "emb", row_strided, ("ipsx_logits", 0), "contiguous", True, 16),
    Accept("emb a column slice", "emb", col_sliced, ("ipsx_logits", 0), "contiguous", True, 16),
    Accept("emb at 4 mod 16", "emb", off4, ("ipsx_logits", 0), "contiguous", True, 16),
    Accept("pos a column slice", "pos", col_sliced, ("ipsx_logits", 2), "contiguous", True, 16),
    Accept("pos at 4 mod 16", "pos", off4, ("ipsx_logits", 2), "contiguous", True, 16),
    Accept("pos expanded over the batch", "pos", expanded, ("ipsx_logits", 2), "rows", False, 16),
]


def retarget(views, export):
    return [v._replace(at=(export, v.at[1])) for v in views]


SCAN_STATE_REFUSALS = [f64("lg"), i32("mem_idx"), i64("tie"), put("mem_idx", lambda a: a["mem_idx"][:, :3], "another M"),
                       strided1("tie"), put("H", lambda a: 3, "lg.shape[2] != H * T"), put("M", lambda a: N, "N <= M")]

ENTRIES = [
    # ------------------------------------------------------------ ips_amd/hip.py
    Entry("query_proj", kw(hip.query_proj, "q", "wq", "temperature"),
          lambda dev: dict(q=rnd((T, D), 1, dev), wq=rnd((H * DK, D), 2, dev), temperature=2.0),
          ["ipsx_query_proj"], {},
          [Accept("q transposed", "q", transposed, ("ipsx_query_proj", 0), "contiguous", True, 4),
           Accept("wq every second row", "wq", row_strided, ("ipsx_query_proj", 1), "contiguous", True, 4),
           Accept("q at 4 mod 16", "q", off4, ("ipsx_query_proj", 0), "contiguous", False, 4)],
          [f64("q"), f64("wq"), put("wq", lambda a: a["wq"][:, :D - 1], "another D")],
          "4: query_proj_kernel reads q and wq element by element", None),
    Entry("fold_query", kw(hip.fold_query, "qs", "wk_weight", "H", "Dk", "T"),
          lambda dev: dict(qs=rnd((T, H * DK), 1, dev), wk_weight=rnd((H * DK, D), 2, dev), H=H, Dk=DK, T=T),
          ["ipsx_pack_conv_weight", "ipsx_fold_query"], {},
          [Accept("qs transposed", "qs", transposed, ("ipsx_fold_query", 0), "contiguous", True, 4)],
          [f64("qs"), f64("wk_weight"), put("qs", lambda a: a["qs"][:, :5], "not (T, H * Dk)"), put("H", lambda a: 3, "wk_weight rows != H * Dk")],
          "4: fold_query_kernel reads qs element by element; the packed key weight and the output are fresh allocations", None),
    Entry("fold_query_bf16", kw(hip.fold_query_bf16, "qs", "wk_weight", "H", "Dk", "T"),
          lambda dev: dict(qs=rnd((T, H * DK), 1, dev), wk_weight=rnd((H * DK, D), 2, dev), H=H, Dk=DK, T=T),
          ["ipsx_pack_conv_weight", "ipsx_fold_query_bf16"], {},
          [Accept("qs transposed", "qs", transposed, ("ipsx_fold_query_bf16", 0), "contiguous", True, 4)],
          [f64("qs"), f64("wk_weight"), put("qs", lambda a: a["qs"][:3], "not (T, H * Dk)")],
          "4: fold_query_bf16_kernel reads qs element by element", None),
    Entry("logits", kw(hip.logits, "emb", "pos", "vq", "R", "out", "cond"), b_logits,
          ["ipsx_logits"], {},
          LOGITS_VIEWS + [Accept("pos[:1]", "pos", lambda t: t.expand(B, -1, -1).contiguous()[:1], ("ipsx_logits", 2), "contiguous", False, 16)],
          [f64("emb"), f64("pos"), f64("vq"), put("vq", lambda a: a["vq"][:-8], "shorter than ipsx_folded_query_elems"),
           put("out", lambda a: torch.zeros((B, 33, R), dtype=torch.float64), "float64"),
           put("out", lambda a: torch.zeros((B, 32, R)), "another n"),
           put("out", lambda a: torch.zeros((B, 33, R + 1))[..., :R], "rows not R apart"),
           put("pos", lambda a: a["pos"][:, :32], "another n"), put("pos", lambda a: rnd((3, 33, D)), "a batch of 3 beside B = 2"),
           put("cond", lambda a: torch.zeros(1), "float32"), put("R", lambda a: 40, "vq folded for another R")],
          "emb, pos 16 when D % 8 == 0 (logits_wave's float4 operand loads, no scalar route at that D; 4 otherwise); vq 16 (float4, "
          "always); out 4 (scalar stores)", None),
    Entry("logits (out given)", kw(hip.logits, "emb", "pos", "vq", "R", "out", "cond"),
          lambda dev: dict(b_logits(dev), out=torch.zeros((B, 33, R), device=dev)),
          ["ipsx_logits"], {"out": ("ipsx_logits", 9)},
          [Accept("out a row range of a longer table", "out", row_range, ("ipsx_logits", 9), "rows", False, 4)], [],
          "see logits", "logits"),
    Entry("logits (bf16 query)", kw(hip.logits, "emb", "pos", "vq", "R", "out", "cond"),
          lambda dev: dict(b_logits(dev), vq=folded(dev, bf16=True)),
          ["ipsx_logits_bf16"], {}, retarget(LOGITS_VIEWS[:4], "ipsx_logits_bf16"),
          [put("vq", lambda a: a["vq"][:-16], "shorter than ipsx_folded_query_bf16_bytes"), put("cond", lambda a: word("cpu"), "with a bf16 query")],
          "emb, pos 16 (logits_bf16_kernel: uint4 / float4 loads); vq 16", "logits"),
    Entry("logits (conditional)", kw(hip.logits, "emb", "pos", "vq", "R", "out", "cond"),
          lambda dev: dict(b_logits(dev), cond=word(dev)),
          ["ipsx_logits_if"], {}, [], [i64("cond"), put("cond", lambda a: torch.zeros(2, dtype=torch.int32), "two words")],
          "see logits; cond 4", "logits"),
    Entry("part_wait", kw(hip.part_wait, "done", "want", "status"),
          lambda dev: dict(done=word(dev), want=3, status=word(dev)),
          ["ipsx_part_wait"], {"done": ("ipsx_part_wait", 0), "status": ("ipsx_part_wait", 2)}, [],
          [i64("done"), put("status", lambda a: torch.zeros(2, dtype=torch.int32), "two words"), to(torch.float32)("status")],
          "4: one int32 word each", None),
    Entry("logits_stats", kw(hip.logits_stats, "emb", "pos", "vq", "R", "out", "stats_x", "stats_out", "ln_eps"), b_logits_stats,
          ["ipsx_logits_stats"], {"out": ("ipsx_logits_stats", 9), "stats_out": ("ipsx_logits_stats", 15)},
          retarget(LOGITS_VIEWS, "ipsx_logits_stats") +
          [Accept("stats_x every second row", "stats_x", row_strided, ("ipsx_logits_stats", 11), "contiguous", True, 16),
           Accept("out a row range of a longer table", "out", row_range, ("ipsx_logits_stats", 9), "rows", False, 4)],
          [f64("emb"), f64("stats_x"), f64("stats_out"), put("stats_out", lambda a: torch.zeros((4, 2)), "rows of another P"),
           put("stats_out", lambda a: torch.zeros((5, 4))[:, :2], "strided"), misaligned("stats_out"),
           put("vq", lambda a: folded("cpu", bf16=True), "a bf16 query"), put("out", lambda a: None, "missing")],
          "as logits; stats_x ? (row_moments_wave32 not read to the end: held to 16, copied); stats_out 8 (float2 stores)", None),
    Entry("scan", kw(hip.scan, "lg", "M", "I", "H", "T"), b_scan,
          ["ipsx_scan"], {},
          [Accept("lg from (B, R, N).permute(0, 2, 1)", "lg", permuted, ("ipsx_scan", 0), "contiguous", True, 16),
           Accept("lg at 4 mod 16", "lg", off4, ("ipsx_scan", 0), "contiguous", True, 16)],
          [f64("lg"), put("H", lambda a: 3, "lg.shape[2] != H * T"), put("M", lambda a: N, "N <= M"), put("lg", lambda a: a["lg"][0], "2-d")],
          "lg 16: scan_large.hip and scan_cam.hip load logits rows as float4, no scalar route; mem_idx / tie are the wrapper's own", None),
    Entry("scan_range", kw(hip.scan_range, "lg", "M", "I", "H", "T", "it_begin", "it_end", "mem_idx", "tie"), b_scan_state,
          ["ipsx_scan_range"], {"mem_idx": ("ipsx_scan_range", 9), "tie": ("ipsx_scan_range", 11)},
          [Accept("lg from (B, R, N).permute(0, 2, 1)", "lg", permuted, ("ipsx_scan_range", 0), "contiguous", True, 16)],
          SCAN_STATE_REFUSALS,
          "lg 16 (see scan): a finished table, so a view is copied; mem_idx 8, tie 4: loop state, element-sized accesses", None),
    Entry("scan_range_strided", lambda a: hip.scan_range_strided(a["lg"], 41, M, I, H, T, 0, 2, a["mem_idx"], a["tie"]),
          lambda dev: dict(b_scan_state(dev), lg=rnd((B, 48, R), 4, dev)),
          ["ipsx_scan_range_strided"], {"mem_idx": ("ipsx_scan_range_strided", 10), "tie": ("ipsx_scan_range_strided", 12), "lg": ("ipsx_scan_range_strided", 0)},
          [], [f64("lg"), i32("mem_idx"), i64("tie"), put("lg", lambda a: permuted(a["lg"]), "not row-contiguous"), misaligned("lg"),
               put("lg", lambda a: rnd((B, 48, R + 1)), "lg.shape[2] != H * T")],
          "lg 16, refused otherwise: the stream's candidate table is written between the calls and read where it lies", None),
    Entry("scan_ragged", lambda a: hip.scan_ragged(a["lg"], a["offsets"], a["lengths"], M, I, H, T),
          lambda dev: dict(lg=rnd((71, R), 4, dev), offsets=torch.tensor([0, 41, 71], dtype=torch.int64, device=dev), lengths=[41, 30]),
          ["ipsx_scan_ragged"], {},
          [], [f64("lg"), i32("offsets"), put("lg", lambda a: a["lg"][:70], "rows != sum of the lengths"), misaligned("lg"),
               put("lengths", lambda a: [67, 4], "a slide of M rows")],
          "lg 16, refused otherwise (the packed table is never copied); offsets 8", None),
    Entry("scan_ragged_spans", lambda a: hip.scan_ragged_spans(a["lg"], a["spans"], 41, M, I, H, T, a["mem_idx"], a["tie"]),
          lambda dev: dict(lg=rnd((80, R), 4, dev), spans=torch.tensor([[0, 41], [41, 30]], dtype=torch.int64, device=dev),
                           mem_idx=torch.zeros((B, M), dtype=torch.int64, device=dev), tie=torch.zeros((B,), dtype=torch.int32, device=dev)),
          ["ipsx_scan_ragged_spans"], {"mem_idx": ("ipsx_scan_ragged_spans", 9), "tie": ("ipsx_scan_ragged_spans", 11)},
          [], [f64("lg"), i32("spans"), i32("mem_idx"), i64("tie"), misaligned("lg"), put("spans", lambda a: a["spans"].t(), "(2, B)")],
          "lg 16, refused otherwise; spans, mem_idx 8; tie 4", None),
    Entry("stream_commit_ragged", lambda a: hip.stream_commit_ragged([(a["held"], a["piece"], a["held"])], None, a["slides"], M, 3),
          lambda dev: dict(held=rnd((B, 8, 4), 14, dev), piece=rnd((6, 4), 15, dev), slides=torch.zeros((B, 6), dtype=torch.int64, device=dev)),
          ["ipsx_stream_commit_ragged"], {},
          [], [f64("piece"), i32("slides"), put("held", lambda a: a["held"][:, ::2], "strided")],
          "fallback: the commit kernels pick 16, 4 or 1 bytes per lane from the addresses and row sizes", None),
    Entry("stream_commit", lambda a: hip.stream_commit(commit_tables(a), a["sel"], M, 5),
          b_commit, ["ipsx_stream_commit"], {}, [],
          [f64("piece"), put("sel", lambda a: torch.zeros((B, M), dtype=torch.int32), "int32"),
           put("piece", lambda a: a["piece"][:, :2], "rows != n_cand - held_rows"), put("held", lambda a: a["held"][:, ::2], "strided")],
          "fallback (see stream_commit_ragged)", None),
    Entry("stream_commit_view", lambda a: hip.stream_commit_view([(None, 0, None, a["dst"])], a["images"], hip.PatchView(IMG, (32, 32), (8, 16)), None, M, 4),
          lambda dev: dict(images=rnd(IMG, 13, dev), dst=torch.zeros((2, 8, 1, 32, 32), device=dev)),
          ["ipsx_stream_commit_view"], {}, [],
          [f64("images"), put("images", lambda a: a["images"][..., :40], "another shape than the view's"), f64("dst")],
          "fallback (the call returns the bytes per lane it copied with)", None),
    Entry("scan_range_if", lambda a: hip.scan_range_if(a["lg"], a["M"], a["I"], a["H"], a["T"], 0, 2, a["mem_idx"], a["tie"], a["cond"]),
          lambda dev: b_scan_state(dev, cond=word(dev)),
          ["ipsx_scan_range_if"], {"mem_idx": ("ipsx_scan_range_if", 9), "tie": ("ipsx_scan_range_if", 11), "cond": ("ipsx_scan_range_if", 12),
                                   "lg": ("ipsx_scan_range_if", 0)},
          [], SCAN_STATE_REFUSALS + [i64("cond"), put("lg", lambda a: permuted(a["lg"]), "a view"), misaligned("lg")],
          "lg 16, refused otherwise (the redo of a loop reads the table its producers wrote, where it lies); cond 4", None),
    Entry("scan_persistent", lambda a: hip.scan_persistent(a["lg"], a["M"], a["I"], a["H"], a["T"], a["mem_idx"], a["tie"], a["ready"], a["status"]),
          lambda dev: b_scan_state(dev, ready=torch.zeros((B,), dtype=torch.int32, device=dev), status=word(dev)),
          ["ipsx_scan_persistent_on"], {"mem_idx": ("ipsx_scan_persistent_on", 7), "tie": ("ipsx_scan_persistent_on", 9), "ready": ("ipsx_scan_persistent_on", 10),
                                        "status": ("ipsx_scan_persistent_on", 12), "lg": ("ipsx_scan_persistent_on", 0)},
          [], SCAN_STATE_REFUSALS + [i64("ready"), i64("status"), put("ready", lambda a: torch.zeros(3, dtype=torch.int32), "three words for B = 2"),
                                     put("lg", lambda a: permuted(a["lg"]), "a view"), misaligned("lg")],
          "lg 16, refused otherwise: producers write the table while the loop runs - a copy would never fill; ready / status 4", None),
    Entry("scan_gate", kw(hip.scan_gate, "status"), lambda dev: dict(status=word(dev)),
          ["ipsx_scan_gate"], {"status": ("ipsx_scan_gate", 0)}, [], [i64("status"), put("status", lambda a: torch.zeros(2, dtype=torch.int32), "two words")],
          "4: one int32 word", None),
    Entry("publish_rows", kw(hip.publish_rows, "ready", "n_rows"), lambda dev: dict(ready=word(dev), n_rows=7),
          ["ipsx_publish_rows"], {"ready": ("ipsx_publish_rows", 0)}, [], [i64("ready"), put("ready", lambda a: torch.zeros(2, dtype=torch.int32), "two words")],
          "4: one int32 word", None),
    Entry("scores", kw(hip.scores, "x", "qs", "wk", "H", "Dk", "T"), b_scores,
          ["ipsx_pack_conv_weight", "ipsx_scores"], {},
          [Accept("x transposed", "x", transposed, ("ipsx_scores", 0), "contiguous", True, 16),
           Accept("x every second row", "x", row_strided, ("ipsx_scores", 0), "contiguous", True, 16),
           Accept("x at 4 mod 16", "x", off4, ("ipsx_scores", 0), "contiguous", True, 16)],
          [f64("x"), f64("qs"), f64("wk"), put("wk", lambda a: rnd((H * DK, D + 8)), "another D than x"), put("qs", lambda a: a["qs"][:3], "not (T, H * Dk)")],
          "x 16: ipsx_scores runs the logits kernel on it (float4 loads when D % 8 == 0); qs 4", "_scores_impl"),
    Entry("attn_map", kw(hip.attn_map, "x", "qs", "wk", "H", "Dk", "T"), b_scores,
          ["ipsx_pack_conv_weight", "ipsx_scores"], {},
          [Accept("x transposed", "x", transposed, ("ipsx_scores", 0), "contiguous", True, 16)],
          [f64("x"), put("wk", lambda a: rnd((H * DK, D + 8)), "another D than x")],
          "see scores", "_scores_impl"),
    Entry("topm", kw(hip.topm, "sc", "M"), lambda dev: dict(sc=rnd((B, 37), 1, dev), M=M),
          ["ipsx_topm"], {},
          [Accept("sc from .t()", "sc", transposed, ("ipsx_topm", 0), "contiguous", True, 4)],
          [f64("sc"), put("M", lambda a: 38, "M > L"), put("sc", lambda a: a["sc"][0], "1-d")],
          "4: topm_kernel reads scores element by element", None),
    Entry("gather_rows", kw(hip.gather_rows, "src", "idx"), lambda dev: dict(src=rnd((B, 9, 5), 1, dev), idx=ints((B, M), 9, 0, dev)),
          ["ipsx_gather_rows"], {},
          [Accept("src permuted", "src", permuted, ("ipsx_gather_rows", 0), "contiguous", True, 4),
           Accept("idx from (M, B).t()", "idx", transposed, ("ipsx_gather_rows", 1), "contiguous", True, 8),
           Accept("src at 4 mod 16", "src", off4, ("ipsx_gather_rows", 0), "contiguous", False, 4)],
          [i32("idx"), put("idx", lambda a: ints((3, M), 9), "3 rows of indices beside a batch of 2"), put("idx", lambda a: a["idx"][0], "1-d")],
          "fallback: ipsx_gather_rows copies rows in 16-, 4- or 1-byte units, picked from the addresses and the row size", None),
    Entry("dequant_patches", kw(hip.dequant_patches, "q", "table"),
          lambda dev: dict(q=ints((2, 3, 1, 4, 4), 256, 0, dev, torch.uint8), table=rnd((1, 256), 1, dev)),
          ["ipsx_dequant_patches"], {},
          [Accept("q permuted", "q", lambda t: t.permute(1, 0, 2, 3, 4).contiguous().permute(1, 0, 2, 3, 4), ("ipsx_dequant_patches", 0), "contiguous", True, 1),
           Accept("q at an odd address", "q", off4, ("ipsx_dequant_patches", 0), "contiguous", False, 1)],
          [to(torch.float32)("q"), f64("table"), put("table", lambda a: rnd((2, 256)), "rows != channels")],
          "fallback: ipsx_dequant_patches takes its 4-byte-load / 16-byte-store route only where q and out allow it", None),
    Entry("ips_finish", kw(hip.ips_finish, "src", "pos", "idx_buf", "status", "status_host"), b_finish,
          ["ipsx_ips_finish"], {"idx_buf": ("ipsx_ips_finish", 7), "status": ("ipsx_ips_finish", 13), "status_host": ("ipsx_ips_finish", 14)},
          [], [i32("idx_buf"), i64("status"), i64("status_host"), misaligned("src"), put("src", lambda a: rnd((B, 9, 5)), "rows of 20 bytes"),
               put("pos", lambda a: rnd((1, 8, 4)), "another N than src"), put("src", lambda a: rnd((3, 9, 4)), "a batch of 3 beside B = 2")],
          "C: src, pos rows are whole 16-byte units at 16-byte addresses (ips_finish_supported says so beforehand); status_host is "
          "the one pinned-host argument", None),
    Entry("ips_finish (ordered)", lambda a: hip.ips_finish(a["src"], a["pos"], a["idx_buf"], a["status"], a["status_host"], order=a["order"]),
          lambda dev: dict(b_finish(dev), order=ints((1, 9), 9, 4, dev)),
          ["ipsx_ips_finish_indexed"], {}, [], [i32("order"), put("order", lambda a: ints((1, 8), 8), "another N")],
          "see ips_finish", "ips_finish"),
    Entry("ragged_finish", lambda a: hip.ragged_finish(a["rows"], a["offsets"], a["mem_idx"], M, a["flat"], a["pos"]), b_ragged_rows,
          ["ipsx_ragged_finish"], {}, [],
          [i32("offsets"), i32("mem_idx"), misaligned("rows"), put("pos", lambda a: a["pos"][:70], "rows != total"),
           put("flat", lambda a: torch.zeros(71, dtype=torch.int64), "int64")],
          "C: rows, pos of whole 16-byte units at 16-byte addresses (ragged_finish_supported)", None),
    Entry("ragged_finish_view", lambda a: hip.ragged_finish_view(a["pixels"], a["rview"], a["offsets"], a["mem_idx"], M, a["flat"], a["pos"]), b_ragged_view,
          ["ipsx_ragged_finish_view"], {}, [],
          [f64("pixels"), i32("offsets"), i32("mem_idx"), put("pixels", lambda a: a["pixels"].view(2, -1), "2-d")],
          "fallback for pixels (float4 only where the view allows it); pos C: 16", None),
    Entry("ragged_blank_flags", lambda a: hip.ragged_blank_flags(a["pixels"], a["rview"], a["index"]),
          lambda dev: dict(pixels=rnd((40 * 48 + 32 * 64,), 12, dev), rview=ragged_view(), index=ints((5,), 4, 0, dev, torch.int32)),
          ["ipsx_ragged_view_blank_flags"], {}, [],
          [f64("pixels"), i64("index"), put("index", lambda a: a["index"].view(1, 5), "2-d")],
          "fallback (the view's load width is picked from the addresses, csrc/ipsx_internal.h)", None),
    Entry("order_index", lambda a: hip.order_index(a["order"], B, 9), lambda dev: dict(order=ints((1, 9), 9, 4, dev)),
          ["ipsx_order_index"], {}, [], [i32("order"), put("order", lambda a: ints((1, 8), 8), "another N"), put("order", lambda a: ints((2, 18), 9)[:, ::2], "strided")],
          "8: int64 elements", None),
    Entry("patchify", kw(hip.patchify, "img", "patch_size", "patch_stride"), b_images,
          ["ipsx_patchify"], {},
          [Accept("a crop of a larger image", "img", lambda t: torch.nn.functional.pad(t, (5, 3, 3, 2))[:, :, 3:43, 5:53], ("ipsx_patchify", 0), "contiguous", True, 4),
           Accept("img at 4 mod 16", "img", off4, ("ipsx_patchify", 0), "contiguous", False, 4)],
          [f64("img"), put("patch_size", lambda a: (64, 32), "taller than the image"), put("img", lambda a: a["img"][0], "3-d")],
          "fallback: ipsx_patchify takes float4 only where img, out, the widths and the stride allow it (its v4 test is the kernel's "
          "only vector access)", None),
    Entry("gather_patches_view", lambda a: hip.gather_patches_view(a["img"], hip.PatchView(IMG, (32, 32), (8, 16)), a["idx"]),
          lambda dev: dict(b_images(dev), idx=ints((2, 3), 4, 0, dev)),
          ["ipsx_gather_patches_view"], {}, [],
          [f64("img"), i32("idx"), put("idx", lambda a: ints((3, 3), 4), "3 rows of indices beside 2 images")],
          "fallback (as ipsx_patchify)", None),
    Entry("patchify_sparse", lambda a: hip.patchify_sparse(a["index"], a["value"], a["offsets"], (40, 48, 1), (32, 32), (8, 16)),
          lambda dev: dict(index=ints((6,), 40 * 48, 0, dev), value=rnd((6,), 1, dev), offsets=torch.tensor([0, 3, 6], dtype=torch.int64, device=dev)),
          ["ipsx_patchify_sparse"], {},
          [Accept("index every second element", "index", row_strided, ("ipsx_patchify_sparse", 0), "contiguous", True, 8),
           Accept("value every second element", "value", row_strided, ("ipsx_patchify_sparse", 1), "contiguous", True, 4)],
          [i32("index"), f64("value"), i32("offsets"), put("value", lambda a: a["value"][:5], "shorter than index")],
          "4 / 8: patchify_sparse_kernel reads one element per thread (and no entry past index.numel(), whatever offsets[-1] says)", None),
    Entry("conv2d_nhwc_bf16", kw(hip.conv2d_nhwc_bf16, "x", "weight", "alpha", "shift", "stride", "pad"),
          lambda dev: dict(x=rnd((1, 4, 4, 16), 1, dev).bfloat16(), weight=rnd((8, 16, 3, 3), 2, dev), alpha=rnd((8,), 3, dev), shift=rnd((8,), 4, dev), stride=1, pad=1),
          ["ipsx_pack_conv_weight_bf16", "ipsx_conv2d_affine_nhwc_bf16"], {}, [],
          [to(torch.float32)("x"), f64("weight"), put("x", lambda a: a["x"][..., :8], "another C_in"), put("alpha", lambda a: a["alpha"][:4], "not (C_out,)")],
          "C: x, y, residual at 16-byte addresses (ipsx_conv2d_affine_nhwc_bf16 refuses otherwise)", None),
    Entry("avgpool_nhwc_bf16", kw(hip.avgpool_nhwc_bf16, "x"), lambda dev: dict(x=rnd((2, 2, 2, 8), 1, dev).bfloat16()),
          ["ipsx_avgpool_nhwc_bf16"], {}, [], [to(torch.float32)("x"), put("x", lambda a: a["x"][:, ::2], "strided")],
          "2: avgpool_nhwc_bf16_kernel reads one bfloat16 per thread and pixel", None),
    Entry("aggregate", lambda a: hip.aggregate(a["transf"], a["x"]), lambda dev: dict(transf=transformer(dev), x=rnd((B, 8, 32), 1, dev)),
          ["ipsx_query_proj", "ipsx_pack_conv_weight", "ipsx_fold_query", "ipsx_pack_conv_weight", "ipsx_aggregate_packed"], {},
          [Accept("x transposed", "x", transposed, ("ipsx_aggregate_packed", 3), "contiguous", True, 16),
           Accept("x every second row", "x", row_strided, ("ipsx_aggregate_packed", 3), "contiguous", True, 16)],
          [f64("x"), put("x", lambda a: rnd((B, 8, 64)), "another D than the weights")],
          "x 16: the aggregation's logits pass is the logits kernel (float4 loads at D % 32 == 0)", None),
    Entry("head", kw(hip.head, "emb", "token", "linear", "act"), lambda dev: dict(emb=rnd((B, T, D), 1, dev), token=1, linear=linear(dev), act="softmax"),
          ["ipsx_head"], {},
          [Accept("emb transposed", "emb", transposed, ("ipsx_head", 0), "contiguous", True, 4),
           Accept("emb every second row", "emb", row_strided, ("ipsx_head", 0), "contiguous", True, 4)],
          [f64("emb"), put("linear", lambda a: linear("cpu", D + 8), "a Linear of another D"), put("token", lambda a: T, "past the last token"),
           put("act", lambda a: "tanh", "unknown")],
          "4: head_kernel reads emb, weight and bias element by element", None),
    # ------------------------------------------------------------ ips_amd/hip_train.py
    Entry("pack_conv_views", lambda a: hip_train.pack_conv_views([(a["weight"], False), (a["weight"], True)]),
          lambda dev: dict(weight=rnd((64, 64, 3, 3), 17, dev)),
          ["ipsx_pack_conv_weights_batch"], {}, [], [f64("weight"), put("weight", lambda a: a["weight"][0], "3-d")],
          "4: the packing kernels read the weight through its strides, element by element - any view is read where it lies", "_pack_conv_view"),
    Entry("conv2d_nhwc", kw(hip_train.conv2d_nhwc, "x", "weight", "stride", "pad"), b_conv,
          ["ipsx_pack_conv_weight_strided", "ipsx_conv2d_lds_nhwc"], {"x": (-1, 1)}, [],
          [f64("x"), put("x", lambda a: nchw(a["x"]), "NCHW-contiguous"), put("weight", lambda a: rnd((64, 32, 3, 3)), "another C_in than x"),
           f64("weight"), misaligned("x")],
          "x 16: conv_nhwc_kernel / the LDS stage kernels read 16-byte buffer loads along the channels; x is a saved activation: refused, "
          "never copied", "_pack_conv_view"),
    Entry("conv2d_nhwc (packed, stats)", lambda a: hip_train.conv2d_nhwc(a["x"], a["weight"], 1, 1, packed=a["packed"], stats_shift=a["stats_shift"]),
          lambda dev: dict(b_conv(dev), packed=torch.zeros(hip.lib().ipsx_packed_conv_weight_elems(64, 64, 3, 3), device=dev), stats_shift=torch.zeros(64, device=dev)),
          ["ipsx_conv2d_lds_nhwc_stats"], {}, [],
          [f64("packed"), f64("stats_shift"), put("stats_shift", lambda a: torch.zeros(32), "not (C_out,)"), strided1("stats_shift")],
          "packed 16 (float4 operand loads); stats_shift 4", "conv2d_nhwc"),
    Entry("conv2d_nhwc_dgrad", lambda a: hip_train.conv2d_nhwc_dgrad(a["dy"], a["weight"], 1, 1, (8, 8)),
          lambda dev: dict(dy=b_conv(dev)["x"], weight=rnd((64, 64, 3, 3), 17, dev)),
          ["ipsx_pack_conv_weight_strided", "ipsx_conv2d_lds_nhwc"], {},
          [Accept("dy NCHW-contiguous", "dy", nchw, (-1, 1), "channels_last", True, 16),
           Accept("dy at 4 mod 16", "dy", lambda t: off4(t.permute(0, 2, 3, 1)).permute(0, 3, 1, 2), (-1, 1), "channels_last", True, 16)],
          [f64("dy"), put("dy", lambda a: a["dy"][:, :, :7], "another map size"), f64("weight")],
          "dy 16 (the forward kernel's operand loads; dgrad_s2_lds_kernel reads float4): a gradient is read only - copied to channels-last", None),
    Entry("conv2d_nhwc_wgrad", lambda a: hip_train.conv2d_nhwc_wgrad(a["x"], a["dy"], (64, 64, 3, 3), 1, 1),
          lambda dev: dict(x=b_conv(dev)["x"], dy=rnd((3, 64, 8, 8), 30, dev).contiguous(memory_format=CL)),
          ["ipsx_conv2d_wgrad_nhwc"], {"x": ("ipsx_conv2d_wgrad_nhwc", 0)},
          [Accept("dy NCHW-contiguous", "dy", nchw, ("ipsx_conv2d_wgrad_nhwc", 1), "channels_last", True, 16),
           Accept("dy expanded from one map", "dy", lambda t: t[:1].contiguous(memory_format=CL).expand(3, -1, -1, -1), ("ipsx_conv2d_wgrad_nhwc", 1), "channels_last", True, 16)],
          [f64("x"), put("x", lambda a: nchw(a["x"]), "NCHW-contiguous"), f64("dy"), put("dy", lambda a: a["dy"][:, :32], "another C_out"),
           put("dy", lambda a: a["dy"][:2], "another batch"), misaligned("x")],
          "4: conv_wgrad_kernel reads x and dy with 4-byte buffer loads; the wrapper still holds both to 16 (one rule for activations); "
          "x is the saved activation: refused as conv2d_nhwc refuses it", None),
    Entry("bn_train_forward", kw(hip_train.bn_train_forward, "x", "residual", "gamma", "beta", "eps", "momentum", "running_mean", "running_var", "relu"), b_bn,
          ["ipsx_bn_train_forward"], {"running_mean": ("ipsx_bn_train_forward", 8), "running_var": ("ipsx_bn_train_forward", 9), "x": ("ipsx_bn_train_forward", 0)},
          [Accept("gamma as buf[::2]", "gamma", row_strided, ("ipsx_bn_train_forward", 4), "contiguous", True, 16),
           Accept("beta as buf[::2]", "beta", row_strided, ("ipsx_bn_train_forward", 5), "contiguous", True, 16),
           Accept("gamma at 4 mod 16", "gamma", off4, ("ipsx_bn_train_forward", 4), "contiguous", True, 16),
           Accept("running_mean a slice buf[64:128]", "running_mean", lambda t: torch.cat([t, t, t])[64:128], ("ipsx_bn_train_forward", 8), "contiguous", False, 4)],
          [f64("x"), put("x", lambda a: nchw(a["x"]), "NCHW-contiguous"), strided1("running_mean"), f64("running_var"), f64("gamma"),
           put("running_mean", lambda a: torch.zeros(32), "not (C,)"), put("beta", lambda a: a["beta"][:32], "not (C,)"),
           put("residual", lambda a: a["x"][:4], "another batch than x")],
          "x, residual, y, gamma, beta, mean, invstd 16: bn_train.hip reads and writes whole float4, no scalar route; running_mean / "
          "running_var 4 (bn_write_stats: one float per channel)", None),
    Entry("maxpool_3x3s2_nhwc", kw(hip_train.maxpool_3x3s2_nhwc, "x"), lambda dev: dict(x=rnd((3, 32, 16, 16), 1, dev).contiguous(memory_format=CL)),
          ["ipsx_maxpool_3x3s2_nhwc"], {},
          [Accept("x NCHW-contiguous", "x", nchw, ("ipsx_maxpool_3x3s2_nhwc", 0), "channels_last", True, 16)],
          [f64("x"), put("x", lambda a: a["x"][0], "3-d")],
          "16: maxpool_3x3s2_nhwc_kernel reads and writes float4 along the channels", None),
    Entry("maxpool_3x3s2_bwd_nhwc", kw(hip_train.maxpool_3x3s2_bwd_nhwc, "x", "dy"),
          lambda dev: dict(x=rnd((3, 32, 16, 16), 1, dev).contiguous(memory_format=CL), dy=rnd((3, 32, 8, 8), 2, dev).contiguous(memory_format=CL)),
          ["ipsx_maxpool_3x3s2_bwd_nhwc"], {},
          [Accept("x NCHW-contiguous", "x", nchw, ("ipsx_maxpool_3x3s2_bwd_nhwc", 0), "channels_last", True, 16),
           Accept("dy NCHW-contiguous", "dy", nchw, ("ipsx_maxpool_3x3s2_bwd_nhwc", 1), "channels_last", True, 16)],
          [f64("x"), f64("dy"), put("dy", lambda a: rnd((3, 32, 7, 7)), "of another map size"), put("dy", lambda a: a["dy"][:2], "another batch")],
          "16: maxpool_3x3s2_bwd_nhwc_kernel stages x, dy and writes dx as float4", None),
    Entry("bn_train_forward_partials", lambda a: hip_train.bn_train_forward_partials(a["x"], None, a["gamma"], a["beta"], 1e-5, 0.1, a["running_mean"], a["running_var"],
                                                                                   True, a["partial"], 2, a["shift"]),
          lambda dev: dict(b_bn(dev), partial=torch.zeros((2, 2, 64), device=dev), shift=torch.zeros(64, device=dev)),
          ["ipsx_bn_train_forward_partials"], {"running_mean": ("ipsx_bn_train_forward_partials", 8), "partial": ("ipsx_bn_train_forward_partials", 14),
                                               "shift": ("ipsx_bn_train_forward_partials", 16)},
          [Accept("gamma as buf[::2]", "gamma", row_strided, ("ipsx_bn_train_forward_partials", 4), "contiguous", True, 16)],
          [f64("partial"), put("partial", lambda a: torch.zeros((1, 2, 64)), "fewer slabs than the count"), put("partial", lambda a: torch.zeros((2, 2, 32)), "another C"),
           strided1("shift"), f64("running_mean")],
          "as bn_train_forward; partial 16 (float4); shift 4 - it may BE running_mean, so it is taken where it lies", None),
    Entry("bn_train_backward", kw(hip_train.bn_train_backward, "dy", "y", "x", "gamma", "mean", "invstd", "relu", "want_residual"), b_bn_bwd,
          ["ipsx_bn_train_backward"], {},
          [Accept("gamma as buf[::2]", "gamma", row_strided, ("ipsx_bn_train_backward", 5), "contiguous", True, 16),
           Accept("mean at 4 mod 16", "mean", off4, ("ipsx_bn_train_backward", 6), "contiguous", True, 16)],
          [f64("dy"), put("dy", lambda a: nchw(a["dy"]), "NCHW-contiguous"), put("y", lambda a: a["y"][:4], "another batch than x"), f64("gamma"),
           put("invstd", lambda a: a["invstd"][:32], "not (C,)")],
          "16 throughout (float4, see bn_train_forward)", None),
    Entry("projector_train_forward", kw(hip_train.projector_train_forward, "x", "weight", "bias", "ln_eps"),
          lambda dev: dict(x=rnd((6, 32), 1, dev), weight=rnd((32, 32), 2, dev), bias=rnd((32,), 3, dev), ln_eps=1e-5),
          ["ipsx_pack_conv_weight", "ipsx_projector_stats_typed", "ipsx_projector_train_forward"], {},
          [Accept("x every second row", "x", row_strided, ("ipsx_projector_train_forward", 2), "contiguous", True, 16)],
          [f64("x"), put("x", lambda a: a["x"][:, :16], "another F than the weight"), put("bias", lambda a: a["bias"][:16], "not (D,)"),
           put("weight", lambda a: rnd((48, 32)), "D no power of two")],
          "? x is read with 16- and 8-byte buffer loads; rows of F % 32 == 0 floats keep every load aligned when the base is: not "
          "checked by the wrapper beyond contiguity (allocations are aligned)", None),
    Entry("projector_wgrad", kw(hip_train.projector_wgrad, "x", "dz", "stats"),
          lambda dev: dict(x=rnd((6, 32), 1, dev), dz=rnd((6, 32), 2, dev), stats=rnd((6, 2), 3, dev)),
          ["ipsx_projector_wgrad"], {},
          [Accept("dz transposed", "dz", transposed, ("ipsx_projector_wgrad", 2), "contiguous", True, 4),
           Accept("stats a column pair of wider rows", "stats", lambda t: torch.cat([t, t], 1)[:, :2], ("ipsx_projector_wgrad", 3), "contiguous", True, 8)],
          [f64("dz"), f64("stats"), put("stats", lambda a: a["stats"][:5], "other rows than x"), put("dz", lambda a: a["dz"][:5], "other rows than x")],
          "x 16 / 8 (buffer loads, see projector_train_forward); dz 4; stats 8 ((mean, rstd) pairs)", None),
    Entry("attn_pool_forward", kw(hip_train.attn_pool_forward, "x", "A", "keep"), b_attn_pool,
          ["ipsx_attn_pool_forward"], {}, [],
          [f64("x"), put("x", lambda a: transposed(a["x"]), "transposed"), misaligned("A"), put("A", lambda a: rnd((8, 64)), "another D than x"),
           put("keep", lambda a: rnd((2, 8, 4)), "not (B, R, M)")],
          "16: attn_pool_train.hip loads x, A, dZ rows as float4; keep and P (rows of M) are read float by float: 4; the wrapper refuses "
          "views (a training step's tensors are its own)", None),
    Entry("attn_pool_backward", kw(hip_train.attn_pool_backward, "x", "A", "keep", "P", "Z", "dZ"), b_attn_pool_bwd,
          ["ipsx_attn_pool_backward"], {}, [],
          [f64("dZ"), put("P", lambda a: a["P"][:, :, :4], "not (B, R, M)"), misaligned("dZ"), put("Z", lambda a: transposed(a["Z"]), "transposed")],
          "16 (see attn_pool_forward)", None),
]

BY_NAME = {e.name: e for e in ENTRIES}


def covered():
    """wrapper function name -> the entries that hold it to the contract (``covers``: the private helper or the wrapper an
    entry with another name runs)"""
    out = collections.defaultdict(list)
    for e in ENTRIES:
        out[e.covers or e.name].append(e.name)
        if e.covers is not None and "(" not in e.name:
            out[e.name].append(e.name)
    return out
