"""The rule that picks the trailing parts of a counted call for its one gated last launch (``Selection.tail_parts``,
``Selection.parts_loop_logits``) and the host checks of ``ipsx_scan_range_logits_gate`` - no GPU."""

import ctypes as C

import pytest
import torch

from ips_amd import hip
from ips_amd.dist import part_iterations
from ips_amd.selection import SCAN_TAIL_ROWS_DEFAULT, Selection

M = I = 64


def rows_of(N, parts=Selection.OVERLAP_PARTS):
    """rows per image of the parts ``Selection.parts_with_ranges`` cuts N patches into"""
    its = part_iterations(-(-(N - M) // I), parts)
    edges = [0] + [min(N, M + it * I) for it in its[1:]]
    edges[-1] = N
    return [edges[k + 1] - edges[k] for k in range(len(edges) - 1)]


def test_the_default_limit():
    assert int(SCAN_TAIL_ROWS_DEFAULT) == 512


def test_the_headline_cut_hands_its_last_two_parts_over():
    rows = rows_of(2500)
    assert rows == [1344, 704, 384, 68]
    assert Selection.tail_parts(rows, 512) == 2


def test_mnist3000_hands_its_last_part_over():
    rows = rows_of(10000)
    assert rows == [5056, 3008, 1472, 464]
    assert Selection.tail_parts(rows, 512) == 3


def test_a_two_part_cut_keeps_one_part_on_the_side_stream():
    assert Selection.tail_parts([192, 128], 512) == 1
    assert Selection.tail_parts([192, 128], 1 << 30) == 1          # never the whole call: there would be nothing to wait for


def test_a_last_part_above_the_limit_leaves_the_chain_as_it_was():
    assert Selection.tail_parts([1344, 704, 384, 600], 512) == 4
    assert Selection.tail_parts([1344, 704, 384, 68], 1) == 4
    assert Selection.tail_parts([1344, 704, 384, 68], 68) == 3
    assert Selection.tail_parts([1344, 704, 384, 68], 451) == 3
    assert Selection.tail_parts([1344, 704, 384, 68], 452) == 2


# ---------------------------------------------------------------------------------------------------- the export's host checks
def call_gate(gate, target, status, bit, it_begin=1, it_end=3):
    """``ipsx_scan_range_logits_gate`` on made-up (aligned, never read) addresses: every check is made before anything is launched"""
    parts = hip.LogitsParts(rows=[192, 128])
    for k in range(2):
        parts.array[k].emb = 4096 * (k + 1)
    p = C.c_void_p
    return hip.lib().ipsx_scan_range_logits_gate(p(1 << 20), 1, 320, M, I, 8, 4, it_begin, it_end, p(1 << 21), None, None, parts.array, 2, 1, 2,
                                                 16, None, 0, p(1 << 22), None, 0, p(gate), target, None, p(status), bit, None, None)


@pytest.mark.parametrize("gate, target, status, bit, text", [
    (1 << 23, 0, 1 << 24, 1, "goes with its target"),
    (0, 1, 0, 0, "goes with its target"),
    (1 << 23, 1, 0, 0, "needs the status word"),
    (1 << 23, 1, 1 << 24, 0, "needs the status word"),
])
def test_a_gate_without_its_target_or_its_status_word_is_refused(gate, target, status, bit, text):
    assert call_gate(gate, target, status, bit) == -1
    assert text in hip.lib().ipsx_last_error().decode()


def test_a_target_in_front_of_the_range_is_refused():
    assert call_gate(1 << 23, 1, 1 << 24, 1, it_begin=2, it_end=4) == -1
    assert "goes with its target" in hip.lib().ipsx_last_error().decode()


def wrapper_call(monkeypatch, **kw):
    """``LogitsParts.scan_range`` on CPU tensors with the device test lifted; the library would be reached only by a valid call"""
    monkeypatch.setattr(hip, "_gpu_device", lambda dev: True)
    reached = []
    real = hip.lib()

    class Lib:
        def __getattr__(self, name):
            if name == "ipsx_folded_query_elems":
                return getattr(real, name)
            return lambda *a: (reached.append(name), 0)[1]
    monkeypatch.setattr(hip, "lib", lambda: Lib())
    monkeypatch.setattr(hip, "_stream", lambda: None)
    B, D = 2, 16
    embs = [torch.zeros((B, 192, D)), torch.zeros((B, 128, D))]
    vq = torch.zeros((real.ipsx_folded_query_elems(32, 1, D),))
    a = dict(gate=torch.zeros((B,), dtype=torch.int32), status=torch.zeros((1,), dtype=torch.int32), out=torch.zeros((B, M), dtype=torch.int64))
    a.update(kw)
    mem = torch.zeros((B, M), dtype=torch.int64)
    if isinstance(a.get("out"), str):
        a["out"] = mem
    hip.LogitsParts(embs).scan_range(torch.zeros((B, 320, 32)), M, I, 8, 4, 1, 4, mem, torch.zeros((B,), dtype=torch.int32), 1, 2, None, vq, **a)
    return reached


def test_the_wrapper_hands_a_valid_gated_call_to_the_new_export(monkeypatch):
    assert wrapper_call(monkeypatch) == ["ipsx_scan_range_logits_gate"]


@pytest.mark.parametrize("change", [
    dict(out=torch.zeros((2, M + 1), dtype=torch.int64)), dict(out=torch.zeros((3, M), dtype=torch.int64)),
    dict(out=torch.zeros((2, M), dtype=torch.int32)), dict(out=torch.zeros((M, 2), dtype=torch.int64).t()), dict(out="mem_idx"),
    dict(gate=torch.zeros((3,), dtype=torch.int32)), dict(gate_publish=torch.zeros((2,), dtype=torch.int64)),
    dict(status=torch.zeros((2,), dtype=torch.int32)),
], ids=["out-columns", "out-rows", "out-dtype", "out-strides", "out-is-mem_idx", "gate-words", "publish-dtype", "status-words"])
def test_an_output_buffer_or_a_word_of_the_wrong_shape_is_refused_before_the_library(monkeypatch, change):
    with pytest.raises(ValueError):
        wrapper_call(monkeypatch, **change)
