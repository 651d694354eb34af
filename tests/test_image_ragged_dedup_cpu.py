"""Exact blank-patch dedup on the ragged view without a GPU ("Dedup"): the new exports, the workspace size, the
one function that decides the route, and ips_image_ragged() on a CPU device - unchanged, record for record."""

import ctypes as C
import os
import re

import pytest
import torch

import image_ragged_cases as ic
import image_ragged_dedup_cases as dc
import ragged_cases as rc
from ips_amd import hip, ragged_image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ipsx.h")
NEW = ("ipsx_trunk_ragged_view_dedup_workspace_bytes", "ipsx_ragged_view_blank_flags", "ipsx_trunk_encode_ragged_view_dedup")


def test_new_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(ipsx_[a-z0-9_]+)\s*\(", text))
    lib = C.CDLL(hip.library_path())
    for s in NEW:
        assert s in declared and hasattr(lib, s) and s in hip._EXPORTS, s
    assert callable(hip.ragged_blank_flags)


def test_workspace_is_nothing_for_no_entries_and_grows_with_them():
    L, t = hip.lib(), C.byref(hip.Trunk())
    size = L.ipsx_trunk_ragged_view_dedup_workspace_bytes
    assert size(t, 0) == 0 and size(t, -5) == 0 and size(None, 100) == 0
    sizes = [size(t, n) for n in (1, 2, 8, 9, 1000, 118257)]
    assert all(a < b for a, b in zip(sizes, sizes[1:]))
    # the flags, the list and the slots (int32 each) and up to n + 1 compacted rows of 128 floats
    for n, s in zip((1, 2, 8, 9, 1000, 118257), sizes):
        assert s >= 12 * n + 4 + 512 * (n + 1)


def test_host_refusals_need_no_gpu():
    """Null pointers, too many entries and a view without a table are refused before anything is launched."""
    L = hip.lib()
    assert L.ipsx_ragged_view_blank_flags(None, None, None, 0, 4, None, None) == -1
    assert L.ipsx_trunk_encode_ragged_view_dedup(None, None, None, None, 0, 4, None, None, 0, None, None) == -1
    rv = hip.RaggedView(1, [(64, 64), (32, 96)], [0, 4096], (32, 32), (32, 32))      # no device table
    buf = (C.c_float * 16)()
    t = hip.Trunk()
    assert L.ipsx_ragged_view_blank_flags(buf, C.byref(rv.struct), None, 0, 4, buf, None) == -1
    assert L.ipsx_ragged_view_blank_flags(buf, C.byref(rv.struct), None, 0, 1 << 31, buf, None) == -1
    assert L.ipsx_trunk_encode_ragged_view_dedup(C.byref(t), buf, C.byref(rv.struct), None, 0, 4, buf, buf, 1 << 20, None, None) == -1


class _Plan:
    def __init__(self, fused):
        self.is_fused, self.asked = fused, []

    def fused(self, shape):
        self.asked.append(tuple(shape))
        return self.is_fused


class _View:
    patch_shape = (1, 32, 32)


def test_the_route_decision():
    decide = ragged_image.ragged_dedup
    plan = _Plan(True)
    assert decide({}, plan, _View) is True and plan.asked == [(1, 32, 32)]
    assert decide({"IPSX_DEDUP_BLANK": "auto"}, _Plan(True), _View) is True
    assert decide({"IPSX_DEDUP_BLANK": "0"}, _Plan(True), _View) is False            # today's plain launches
    assert decide({"IPSX_DEDUP_BLANK": "1"}, _Plan(True), _View) is False            # (refused earlier, by ragged._check)
    assert decide({}, _Plan(False), _View) is False                                  # a trunk that is not the fused one
    assert decide({"IPSX_DEDUP_BLANK": "auto"}, _Plan(False), _View) is False


SIZES = [(160, 192), (192, 224), (128, 416)]                   # 30, 42, 52 patches at stride 32: all longer than M = 16
PATCH, STRIDE = (32, 32), (32, 32)


@pytest.mark.parametrize("shuffle", [False, True])
def test_cpu_call_is_unchanged_record_for_record(shuffle, monkeypatch):
    net = rc.make_net(rc.image_conf(M=16, shuffle=shuffle, shuffle_style="batch"), "cpu")
    imgs = dc.planted_images(SIZES)
    flags = dc.host_flags(dc.flat_patches(imgs, PATCH, STRIDE))
    assert 0 < int(flags.sum()) < flags.numel() // 2
    want = ic.solo_loop(net, imgs, PATCH, STRIDE)
    for value in (None, "auto", "0"):
        monkeypatch.delenv("IPSX_DEDUP_BLANK", raising=False)
        if value is not None:
            monkeypatch.setenv("IPSX_DEDUP_BLANK", value)
        rc.assert_same_record(ic.image_call(net, imgs, PATCH, STRIDE), want)
    sizes = SIZES + [(128, 128), (64, 96)]
    imgs = dc.planted_images(sizes)
    slides = [dc.flat_patches([im], PATCH, STRIDE) for im in imgs]
    ic.assert_same_padded(ic.image_call(net, imgs, PATCH, STRIDE, pad=True), ic.patch_call(net, slides, pad=True))


def test_the_explicit_switch_is_still_refused_before_the_rng_moves(monkeypatch):
    net = rc.make_net(rc.image_conf(M=16, shuffle=True, shuffle_style="batch"), "cpu")
    imgs = dc.planted_images(SIZES)
    monkeypatch.setenv("IPSX_DEDUP_BLANK", "1")
    for pad in (False, True):
        torch.manual_seed(5)
        before = torch.get_rng_state()
        net.last_mem_idx = "untouched"
        with pytest.raises(TypeError):
            net.ips_image_ragged(imgs, PATCH, STRIDE, pad=pad)
        assert torch.equal(torch.get_rng_state(), before) and net.last_mem_idx == "untouched"
