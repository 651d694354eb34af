"""A shuffle index on the one-call and one-image routes, the part that needs no device: the three 3.06 additions are
declared, listed, exported and bound; ``ipsx_ips_call`` kept its layout; everything ``ipsx_order_index`` and
``ipsx_ips_call_run_ordered`` refuse about the order is refused before the first runtime call; on a CPU net nothing
selects through an index and ``ips()`` is what it was."""

import ctypes
import os
import re

import torch

from ips_amd import hip, synth
from ips_amd.architecture import IPSNet

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ipsx.h")
NEW = ("ipsx_order_index", "ipsx_trunk_stream_indexed", "ipsx_ips_call_run_ordered")
EINVAL = -1


def header_text():
    return open(HEADER).read()


def without_comments(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


# ---------------------------------------------------------------- header and bindings
def test_the_header_declares_and_lists_the_additions_at_3_06():
    text = header_text()
    assert re.search(r"^#define IPSX_VERSION 306$", text, re.M)
    code = without_comments(text)
    block = text[text.index("3.06  (additions only)"):text.index("#define IPSX_VERSION")]
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name            # declared outside comments
        assert name in block, name                                          # listed in the 3.06 history block
    assert re.search(r"typedef\s+struct\s+ipsx_call_order\s*\{", code) and "ipsx_call_order" in block


def test_the_additions_are_exported_and_bound():
    raw = ctypes.CDLL(hip.library_path())
    for name in NEW:
        assert hasattr(raw, name), name
        assert name in hip._EXPORTS, name
    lib = hip.lib()
    assert lib.ipsx_version() == 306
    # argument counts of the declarations and of the ctypes table
    code = without_comments(header_text())
    for name in NEW:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m and len(m.group(1).split(",")) == len(hip._EXPORTS[name][1]), name


def test_ipsx_ips_call_keeps_its_layout():
    # ipsx_ips_call on LP64, every member at its natural alignment (field list of include/ipsx.h, in order):
    #   b 4 (+4 pad) | n 8 | m, i, h, n_token 16                                     ->  32
    #   logits, mem_idx, words 24 | words_total 8                                    ->  64
    #   loops 4 (+4) | scan_workspace 8 | scan_workspace_bytes 8                     ->  88
    #   trunk 8 | pos 8 | quad_pulls 4 (+4)                                          -> 112
    #   lin 8 | ln_eps 4 | short_first 4                                             -> 128
    #   x, emb, v_packed 24 | r, workgroups 8                                        -> 160
    #   src 8 | src_row_bytes, src_bstride_rows 16                                   -> 184
    #   pos_table 8 | pos_row_bytes, pos_bstride_rows 16                             -> 208
    #   mem_patch, mem_pos, mem_idx_out, status_host 32                              -> 240
    #   timing_slot 4 (+4) | stream, side_stream 16                                  -> 264
    assert ctypes.sizeof(hip.IpsCall) == 264
    assert hip.IpsCall.side_stream.offset == 256 and hip.IpsCall.x.offset == 128
    assert ctypes.sizeof(hip.IpsCallOrder) == 24
    code = without_comments(header_text())
    body = re.search(r"typedef\s+struct\s+ipsx_ips_call\s*\{(.*?)\}\s*ipsx_ips_call\s*;", code, re.S).group(1)
    names = [re.sub(r"[\s\*]", "", n) for decl in body.split(";") if decl.strip()
             for n in re.sub(r"^\s*(const\s+)?\w+\s*\**", "", decl.strip(), count=1).split(",")]
    assert names == [f[0] for f in hip.IpsCall._fields_]


# ---------------------------------------------------------------- refusals before any launch
def test_order_index_refuses_bad_arguments_before_any_launch():
    lib = hip.lib()
    order = (ctypes.c_int64 * 8)()
    index = (ctypes.c_int32 * 8)()
    o, ix = ctypes.addressof(order), ctypes.addressof(index)
    for what, args in (("a null order", (None, 0, 1, 8, ix)), ("a null index", (o, 0, 1, 8, None)),
                       ("b < 1", (o, 0, 0, 8, ix)), ("n < 1", (o, 0, 1, 0, ix)),
                       ("order_bstride neither 0 nor n", (o, 4, 2, 8, ix)), ("order_bstride neither 0 nor n", (o, -8, 1, 8, ix))):
        assert lib.ipsx_order_index(*args, None) == EINVAL, what
        assert b"order_index" in lib.ipsx_last_error(), what


def test_the_ordered_call_refuses_a_bad_order_before_any_launch():
    lib = hip.lib()
    call = hip.IpsCall()
    call.b, call.n, call.m, call.i, call.h, call.n_token = 1, 300, 32, 32, 8, 1
    words = (ctypes.c_int64 * 8)()
    p = ctypes.addressof(words)
    for what, (order, stride, index) in (("a null o->order", (None, 0, p)), ("a null o->index", (p, 0, None)),
                                         ("a bad order_bstride", (p, 7, p)), ("a bad order_bstride", (p, 299, p))):
        o = hip.IpsCallOrder(order, stride, index)
        assert lib.ipsx_ips_call_run_ordered(ctypes.byref(call), ctypes.byref(o)) == EINVAL, what
        assert b"order" in lib.ipsx_last_error(), what
    assert lib.ipsx_ips_call_run_ordered(ctypes.byref(call), None) == EINVAL


# ---------------------------------------------------------------- host logic, no launch
def test_a_cpu_net_selects_through_no_index_and_ips_is_what_it_was():
    cpu = torch.device("cpu")
    for style in ("batch", "instance"):
        conf = synth.camelyon_conf(N=60, M=8, I=8, n_chan_in=32, shuffle=True, shuffle_style=style)
        net = synth.fill_weights(IPSNet(cpu, conf), 3).eval()
        x = synth.make_patches(conf, 2, seed=1)
        sel = net.selection
        assert sel.native_calls == 0 and sel.native_ordered_calls == 0
        assert not sel.index_supported(x)
        torch.manual_seed(4)
        mem_patch, mem_pos = net.ips(x)
        idx, order = net.last_mem_idx, net.last_shuffle
        assert sel.index_calls == 0 and sel.native_calls == 0 and sel.native_ordered_calls == 0
        assert order is not None and not order.is_cuda
        # the selection of the shuffled copy: a net that does not shuffle, on the tensor permuted by the order that was drawn
        plain = synth.fill_weights(IPSNet(cpu, conf.clone(shuffle=False)), 3).eval()
        rows = order.expand(2, -1)
        shuffled = torch.gather(x, 1, rows.unsqueeze(-1).expand(-1, -1, x.shape[2]))
        want_patch, _ = plain.ips(shuffled)
        assert torch.equal(mem_patch, want_patch) and torch.equal(idx, plain.last_mem_idx)
        for b in range(2):
            assert torch.equal(x[b, rows[b, idx[b]]], mem_patch[b])
        torch.manual_seed(4)
        again, _ = net.ips(x)
        assert torch.equal(again, mem_patch)


def test_the_flat_index_is_composed_on_first_use():
    """``select`` keeps the order and composes ``_flat`` only when a route asks for it (no device: the fields alone)."""
    from ips_amd.selection import Selection
    conf = synth.camelyon_conf(N=60, M=8, I=8, n_chan_in=32)
    sel = Selection(synth.fill_weights(IPSNet(torch.device("cpu"), conf), 3).eval())
    assert sel._flat is None
    order = torch.randperm(7).unsqueeze(0)
    sel._order, sel._order_bn = order, (3, 7)
    assert sel._flat_made is None
    flat = sel._flat
    assert sel._flat_made is flat and flat.dtype == torch.int32
    assert torch.equal(flat, (order.expand(3, -1) + torch.arange(3)[:, None] * 7).int())
