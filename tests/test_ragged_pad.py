"""``ips_ragged(slides, pad=True)`` on the device: ``ipsx_ragged_finish`` - the end of a padded call in ONE
launch - against a host restatement, the call end to end against the loop of solo ``ips()`` calls plus zero buffers, bit
for bit, its launch counts, and ``evaluate()`` over padded batches against the reference's record."""

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

import ragged_cases as rc
import ragged_pad_cases as pc
from ips_amd import hip
from ips_amd.ragged import Ragged, collate_ragged_padded
from ips_amd.training import iterative as loops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M = 16


# ------------------------------------------------------------------ the finish launch
def _restate(rows, lengths, mem_idx, m, flat, pos):
    """``ipsx_ragged_finish`` slot by slot, on host tensors."""
    B, total = len(lengths), rows.shape[0]
    patch = torch.zeros((B, m) + tuple(rows.shape[1:]), dtype=rows.dtype)
    out_pos = torch.zeros((B, m, pos.shape[1]), dtype=pos.dtype) if pos is not None else None
    idx = torch.full((B, m), -1, dtype=torch.int64)
    grow = torch.full((B, m), -1, dtype=torch.int64)
    off = 0
    for b, n in enumerate(lengths):
        for j in range(m):
            if n > m:
                r = min(max(int(mem_idx[b, j]), 0), n - 1)
            elif j < n:
                r = j
            else:
                continue
            g = off + r
            src = min(max(int(flat[g]), 0), total - 1) if flat is not None else g
            patch[b, j] = rows[src]
            if pos is not None:
                out_pos[b, j] = pos[g]
            idx[b, j], grow[b, j] = r, g
        off += n
    return patch, out_pos, idx, grow


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


# 16 B: one unit; 272 B: 17 units, fewer than the lanes; 4,112 B: 257 units, a second trip of the copy loop; float16 rows
@pytest.mark.parametrize("width,dtype", [(4, torch.float32), (68, torch.float32), (1028, torch.float32), (24, torch.float16)])
@pytest.mark.parametrize("with_flat", [False, True])
@pytest.mark.parametrize("with_pos", [False, True])
def test_ragged_finish_equals_its_restatement(width, dtype, with_flat, with_pos):
    lengths = (M - 1, M + 1, M, 1, 3 * M + 5, M - 1)          # short slides first and last
    B, total = len(lengths), sum(lengths)
    g = torch.Generator().manual_seed(width + 2 * with_flat + with_pos)
    rows = torch.randn((total, width), generator=g).to(dtype)
    pos = torch.randn((total, 8), generator=g) if with_pos else None
    flat = None
    if with_flat:
        flat = torch.randperm(total, generator=g).to(torch.int32)
        flat[5], flat[M + 3] = -1, total + 3                  # clamped into the table
    mem_idx = torch.stack([torch.randperm(max(n, M), generator=g)[:M] for n in lengths])
    mem_idx[1, 0], mem_idx[1, 1], mem_idx[4, 2], mem_idx[4, 3] = -3, M + 1, 1 << 62, 3 * M + 5     # leave their own slide
    want = _restate(rows, lengths, mem_idx, M, flat, pos)
    for b, n in enumerate(lengths):                            # out-of-range entries of a long slide stay inside that slide
        if n > M:
            start = sum(lengths[:b])
            assert int(want[3][b].min()) >= start and int(want[3][b].max()) < start + n
    offsets = torch.tensor([sum(lengths[:k]) for k in range(B + 1)], dtype=torch.int64, device=DEV)
    dev = lambda t: t.to(DEV) if t is not None else None
    assert hip.ragged_finish_supported(dev(rows), dev(pos))
    results = []
    for poison in (float("nan"), None, (1 << 62, -7)):
        idx_in = mem_idx.clone()
        if isinstance(poison, tuple):                          # the loop leaves the rows of short slides unwritten: never read
            for b, n in enumerate(lengths):
                if n <= M:
                    idx_in[b, 0::2], idx_in[b, 1::2] = poison
        out = (torch.empty((B, M, width), dtype=dtype, device=DEV), torch.empty((B, M, 8), device=DEV) if with_pos else None,
               torch.empty((B, M), dtype=torch.int64, device=DEV), torch.empty((B, M), dtype=torch.int64, device=DEV))
        for t in out:                                          # the padding is WRITTEN: nothing depends on what the buffers held
            if t is not None and poison is None:
                t.view(torch.uint8).fill_(0x7f)
            elif t is not None:
                t.fill_(float("nan")) if t.dtype.is_floating_point else t.fill_(-99)
        got = hip.ragged_finish(dev(rows), offsets, dev(idx_in), M, dev(flat), dev(pos), out=out)
        torch.cuda.synchronize()
        assert all(a is b for a, b in zip(got, out))
        results.append(got)
    for got in results:
        for a, w, name in zip(got, want, ("mem_patch", "mem_pos", "mem_idx", "rows")):
            if w is None:
                assert a is None
            else:
                assert a.dtype == w.dtype and torch.equal(_bits(a.cpu()), _bits(w)), name


def test_ragged_finish_without_a_selection_and_what_it_refuses():
    lengths = (M, 1, M - 1)
    rows = torch.randn(sum(lengths), 68, device=DEV)
    offsets = torch.tensor([0, M, M + 1, 2 * M], dtype=torch.int64, device=DEV)
    got = hip.ragged_finish(rows, offsets, None, M)
    want = _restate(rows.cpu(), lengths, None, M, None, None)
    assert got[1] is None and all(torch.equal(a.cpu(), w) for a, w in zip(got, want) if w is not None)
    assert not hip.ragged_finish_supported(torch.zeros(8, 37 * 45 * 3, device=DEV), None)       # 19,980 B: no 16-byte units
    assert not hip.ragged_finish_supported(torch.zeros(8, 5, device=DEV)[:, :4], None)
    assert not hip.ragged_finish_supported(rows.cpu(), None)
    with pytest.raises(ValueError):
        hip.ragged_finish(torch.zeros(8, 5, device=DEV), offsets, None, M)
    with pytest.raises(ValueError):
        hip.ragged_finish(rows, offsets.cpu(), None, M)
    with pytest.raises(ValueError):
        hip.ragged_finish(rows, offsets, torch.zeros(3, M, dtype=torch.int32, device=DEV), M)
    with pytest.raises(ValueError):
        hip.ragged_finish(rows, offsets, None, M, flat=torch.zeros(5, dtype=torch.int32, device=DEV))


def test_scan_ragged_short_ok_leaves_short_slides_alone():
    lengths = (M - 1, 3 * M + 5, M, M + 1)
    H, T = 8, 1
    lg = torch.randn(sum(lengths), H * T, device=DEV)
    offsets = torch.tensor([sum(lengths[:k]) for k in range(len(lengths) + 1)], dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="slide 0"):
        hip.scan_ragged(lg, offsets, lengths, M, M, H, T)
    with pytest.raises(ValueError, match="no slide"):
        hip.scan_ragged(lg[:2 * M - 1].contiguous(), torch.tensor([0, M - 1, 2 * M - 1], dtype=torch.int64, device=DEV), (M - 1, M),
                        M, M, H, T, short_ok=True)
    got = hip.scan_ragged(lg, offsets, lengths, M, M, H, T, short_ok=True)
    for b in (1, 3):                                           # the long slides: what the loop selects in them alone
        lo = sum(lengths[:b])
        alone = hip.scan_ragged(lg[lo:lo + lengths[b]].contiguous(), torch.tensor([0, lengths[b]], dtype=torch.int64, device=DEV),
                                lengths[b:b + 1], M, M, H, T)
        assert torch.equal(got[b], alone[0])


# ------------------------------------------------------------------ end to end
def _on_device(slides):
    return [s.to(DEV) for s in slides]


@pytest.fixture(scope="module")
def feature_nets():
    made = {}

    def get(shuffle, use_pos):
        if (shuffle, use_pos) not in made:
            conf = rc.feature_conf(M=M, shuffle=shuffle is not None, shuffle_style=shuffle or 'batch', use_pos=use_pos)
            made[(shuffle, use_pos)] = (conf, rc.make_net(conf, DEV))
        return made[(shuffle, use_pos)]
    return get


@pytest.mark.parametrize("shuffle,use_pos", [(None, False), ("instance", False), (None, True), ("batch", True)])
def test_feature_slides_equal_the_solo_loop_plus_zero_buffers(feature_nets, shuffle, use_pos):
    conf, net = feature_nets(shuffle, use_pos)
    lengths = pc.lengths(M)
    slides = _on_device(rc.make_slides(conf, lengths))
    want = pc.expected(net, slides)
    assert (want["shuffle"] is not None) == (shuffle is not None)
    got = pc.padded_call(net, slides)
    pc.assert_same(got, want)
    assert tuple(got["mem_idx"].shape) == (len(lengths), M) and tuple(got["mem_emb"].shape) == (len(lengths), M, conf.D)
    pad = got["mem_patch"][3, 1:]
    assert not pad.any() and not torch.signbit(pad).any()


def test_the_gather_route_for_unaligned_rows_gives_the_same(feature_nets, monkeypatch):
    """Rows that are no whole 16-byte units end in the ``gather_rows`` launches plus the padding on ATen ops."""
    conf, net = feature_nets("batch", True)
    slides = _on_device(rc.make_slides(conf, pc.lengths(M)))
    want = pc.expected(net, slides)
    monkeypatch.setattr(hip, "ragged_finish_supported", lambda rows, pos: False)
    monkeypatch.setattr(hip, "ragged_finish", None)
    pc.assert_same(pc.padded_call(net, slides), want)
    pc.assert_same(pc.padded_call(net, _on_device(rc.make_slides(conf, (M, 1, M - 1)))),
                   pc.expected(net, _on_device(rc.make_slides(conf, (M, 1, M - 1)))))


def test_half_rows_under_the_bf16_projector(monkeypatch):
    monkeypatch.setenv("IPSX_PRECISION", "bf16")
    for shuffle in (False, True):
        conf = rc.feature_conf(M=M, shuffle=shuffle, shuffle_style='instance')
        net = rc.make_net(conf, DEV)
        slides = _on_device(rc.make_slides(conf, pc.lengths(M), dtype=torch.float16))
        want = pc.expected(net, slides)
        got = pc.padded_call(net, slides)
        pc.assert_same(got, want)
        assert got["mem_patch"].dtype == torch.float16


@pytest.mark.parametrize("shuffle", [False, True])
def test_image_slides_equal_the_solo_loop_plus_zero_buffers(shuffle):
    conf = rc.image_conf(M=M, shuffle=shuffle, shuffle_style='batch')
    net = rc.make_net(conf, DEV)
    slides = _on_device(rc.make_slides(conf, (17, 16, 40, 3)))
    want = pc.expected(net, slides)
    pc.assert_same(pc.padded_call(net, slides), want)
    assert want["mem_pos"] is not None and tuple(want["mem_patch"].shape) == (4, M, 1, 32, 32)


def test_host_pinned_and_device_ragged_agree(feature_nets):
    conf, net = feature_nets(None, True)
    host = rc.make_slides(conf, pc.lengths(M))
    on_dev = pc.padded_call(net, Ragged.from_list(_on_device(host)))
    pc.assert_same(on_dev, pc.expected(net, _on_device(host)))
    pc.assert_same(pc.padded_call(net, Ragged.from_list(host)), on_dev)
    pc.assert_same(pc.padded_call(net, Ragged.from_list(host, pad=True).pin_memory(), through_ips=True), on_dev)
    pc.assert_same(pc.padded_call(net, Ragged.from_list(_on_device(host), pad=True), through_ips=True), on_dev)
    assert Ragged.from_list(host, pad=True).pin_memory().pad and Ragged.from_list(host, pad=True).to(DEV).pad


def test_a_batch_of_short_slides_only(feature_nets):
    for key in ((None, True), ("batch", False)):
        conf, net = feature_nets(*key)
        slides = _on_device(rc.make_slides(conf, (M, 1, M - 1)))
        want = pc.expected(net, slides)
        assert want["shuffle"] is None
        pc.assert_same(pc.padded_call(net, slides), want)


def test_a_batch_without_a_short_slide_equals_the_call_without_pad(feature_nets):
    conf, net = feature_nets("batch", True)
    slides = _on_device(rc.make_slides(conf, (M + 1, 3 * M, 3 * M + 5, 7 * M)))
    want = rc.ragged_call(net, slides)
    got = pc.padded_call(net, slides)
    rc.assert_same_record(got, want)
    assert got["count"] == (M,) * 4


# ------------------------------------------------------------------ launch counts
def _count(monkeypatch, net):
    seen = []

    def counted(name, real):
        def call(*a, **k):
            seen.append(name)
            return real(*a, **k)
        return call
    for name in ("scan_ragged", "ragged_finish", "gather_rows", "logits", "scan", "scan_range"):
        monkeypatch.setattr(hip, name, counted(name, getattr(hip, name)))
    plan = type(net.plan)                                      # (every eval-mode encoder pass on the device goes through the plan)
    for name in ("encode", "encode_source"):
        monkeypatch.setattr(plan, name, counted("encode", getattr(plan, name)))
    return seen


@pytest.mark.parametrize("shuffle", [None, "batch"])
def test_one_scan_and_one_finish_launch_per_call(feature_nets, monkeypatch, shuffle):
    """ONE ``ipsx_scan_ragged`` and ONE ``ipsx_ragged_finish`` per call, one encoder pass, one logits table, and on aligned
    rows no ``gather_rows`` launch (``last_mem_emb``, made on first use, gathers its rows as it always did)."""
    conf, net = feature_nets(shuffle, True)
    slides = _on_device(rc.make_slides(conf, pc.lengths(M)))
    seen = _count(monkeypatch, net)
    net.ips_ragged(slides, pad=True)
    assert sorted(seen) == ["encode", "logits", "ragged_finish", "scan_ragged"]
    del seen[:]
    assert net.last_mem_emb is not None
    assert sorted(seen) == ["encode", "gather_rows"]           # the one all-zero row, and the rows of the slots


def test_a_batch_of_short_slides_launches_no_loop_and_no_encoder(feature_nets, monkeypatch):
    conf, net = feature_nets(None, True)
    slides = _on_device(rc.make_slides(conf, (M, 1, M - 1)))
    seen = _count(monkeypatch, net)
    net.ips_ragged(slides, pad=True)
    assert seen == ["ragged_finish"]
    del seen[:]
    assert tuple(net.last_mem_emb.shape) == (3, M, conf.D)
    assert "scan_ragged" not in seen and "logits" not in seen and seen.count("encode") == 2      # the rows, the all-zero row


# ------------------------------------------------------------------ evaluate() against the reference's record
@pytest.mark.parametrize("name", ["feature", "image"])
def test_evaluate_over_padded_batches_on_the_device(name):
    """1e-4: what tests/test_loops_golden.py holds ``evaluate`` on the HIP path to."""
    z = np.load(pc.GOLDEN, allow_pickle=False)
    conf, net, items, crit = pc.fixture_case(z, name, DEV)
    torch.manual_seed(int(z[name + "_torch_seed"]))
    rec = pc.Recorder()
    loops.evaluate(net, crit, DataLoader(items, batch_size=4, collate_fn=collate_ragged_padded), torch.device(DEV), rec, conf)
    pc.check_fixture(z, name, rec, conf, 1e-4)
