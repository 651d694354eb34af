"""Every launching wrapper of ``ips_amd/hip.py`` and ``ips_amd/hip_train.py`` held to its argument contract (DESIGN 2.9,
tests/wrapper_cases.py) WITHOUT a GPU: the library is replaced by a stand-in that forwards pure host queries and records
every other export as (name, arguments), returning 0 - nothing is launched, so nothing malformed can reach a device (the
file is safe on a GPU machine too).  Checked per entry of the table: a valid call reaches exactly the launching exports the
entry lists (recorded at the commit before the guards: a guard changes nothing a correct call launches); every refused
change raises ValueError / TypeError before the first recorded export; every accepted change arrives as a compact tensor
of the kernel's layout, dtype and alignment, the caller's tensor unchanged; written buffers arrive by their own address;
with the device test unpatched every wrapper refuses CPU tensors; and the table is complete."""

import ctypes as C
import inspect

import pytest
import torch

import wrapper_cases as wc
from ips_amd import hip, hip_encoder, hip_train

HOST_SUFFIXES = ("_bytes", "_elems", "_words", "_floats", "_count", "_slabs", "_rows", "_supported", "_groupable")
HOST_NAMES = ("ipsx_version", "ipsx_last_error", "ipsx_scan_workgroups_per_image")
LAUNCHERS = ("ipsx_publish_rows", "ipsx_gather_rows")          # end in ``_rows`` like a host query, yet take pointers and a stream
MODULES = (hip, hip_train, hip_encoder)


class StandIn:
    """``hip.lib()`` that launches nothing: host queries go to the real library, everything else is recorded."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        if name in HOST_NAMES or (name.endswith(HOST_SUFFIXES) and name not in LAUNCHERS):
            return getattr(self._real, name)

        def record(*args):
            self.calls.append((name, tuple(a.value if isinstance(a, C.c_void_p) else a for a in args)))
            return 0
        return record

    @property
    def names(self):
        return [c[0] for c in self.calls]


def install(monkeypatch, gpu=True):
    """The stand-in as ``lib`` of the three binding modules, ``_stream`` -> None, ``_p`` remembering the tensor behind every
    pointer it hands over, and (``gpu``) the device test accepting CPU tensors -> (stand-in, {pointer: tensor})."""
    stand, seen = StandIn(hip.lib()), {}

    def p(t):
        if t is None:
            return C.c_void_p(0)
        seen[t.data_ptr()] = t
        return C.c_void_p(t.data_ptr())
    for m in MODULES:
        monkeypatch.setattr(m, "lib", lambda: stand)
        monkeypatch.setattr(m, "_stream", lambda: None)
        monkeypatch.setattr(m, "_p", p)
    if gpu:
        monkeypatch.setattr(hip, "_gpu_device", lambda dev: True)
        monkeypatch.setattr(hip_train, "_gpu_device", lambda dev: True)
    return stand, seen


def tensors_of(a):
    return [k for k, v in a.items() if torch.is_tensor(v) and k != "status_host"]


def refusals(e):
    """the entry's refusals and, where a call has two tensors or more, each of them on another device"""
    out = list(e.refuse)
    names = tensors_of(e.build("cpu"))
    if len(names) >= 2:
        out += [wc.put(n, lambda a, n=n: a[n].to("meta"), "on another device than the rest") for n in names]
    return out


ENTRY_IDS = [e.name for e in wc.ENTRIES]
REFUSALS = [(e.name, k) for e in wc.ENTRIES for k in range(len(refusals(e)))]
ACCEPTS = [(e.name, k) for e in wc.ENTRIES for k in range(len(e.accept))]


def pointer(stand, at):
    name, index = at
    call = stand.calls[-1] if name == -1 else next(c for c in stand.calls if c[0] == name)
    return call[1][index]


@pytest.mark.parametrize("name", ENTRY_IDS)
def test_valid_call_reaches_the_recorded_exports(name, monkeypatch):
    e = wc.BY_NAME[name]
    a = e.build("cpu")
    stand, _ = install(monkeypatch)
    e.fn(a)
    assert stand.names == e.launches


@pytest.mark.parametrize("name,k", REFUSALS, ids=["%s-%d" % r for r in REFUSALS])
def test_refused_before_any_launch(name, k, monkeypatch):
    e = wc.BY_NAME[name]
    label, change = refusals(e)[k]
    a = e.build("cpu")
    change(a)
    stand, _ = install(monkeypatch)
    with pytest.raises((ValueError, TypeError)) as err:
        e.fn(a)
    assert stand.calls == [], "%s - %s: reached %s before %r" % (name, label, stand.names, err.value)
    assert str(err.value), label


@pytest.mark.parametrize("name,k", ACCEPTS, ids=["%s-%d" % r for r in ACCEPTS])
def test_accepted_view_arrives_normalised(name, k, monkeypatch):
    e = wc.BY_NAME[name]
    acc = e.accept[k]
    a = e.build("cpu")
    view = acc.view(a[acc.arg])
    before = view.clone()
    a[acc.arg] = view
    stand, seen = install(monkeypatch)
    e.fn(a)
    assert stand.names == e.launches, acc.label
    ptr = pointer(stand, acc.at)
    handed = seen[ptr]
    assert handed.dtype == view.dtype and handed.shape == view.shape and torch.equal(handed, view), acc.label
    if acc.layout == "contiguous":
        assert handed.is_contiguous()
    elif acc.layout == "channels_last":
        assert handed.is_contiguous(memory_format=torch.channels_last)
    else:                                   # "rows": contiguous rows, any batch stride
        assert handed.stride(-1) == 1 and handed.stride(-2) == handed.shape[-1]
    assert ptr % acc.align == 0, "%s: handed over at %d mod %d" % (acc.label, ptr % acc.align, acc.align)
    assert (ptr != view.data_ptr()) == acc.copied, acc.label
    assert torch.equal(view, before), "the caller's tensor changed"


WRITTEN = [(e.name, arg) for e in wc.ENTRIES for arg in e.written]


@pytest.mark.parametrize("name,arg", WRITTEN, ids=["%s-%s" % w for w in WRITTEN])
def test_written_buffers_go_by_their_own_address(name, arg, monkeypatch):
    e = wc.BY_NAME[name]
    a = e.build("cpu")
    stand, _ = install(monkeypatch)
    e.fn(a)
    assert pointer(stand, e.written[arg]) == a[arg].data_ptr()


@pytest.mark.parametrize("name", ENTRY_IDS)
def test_cpu_tensors_are_refused(name, monkeypatch):
    """the device test unpatched: ``status_host`` of ``ips_finish`` is the one host argument, and it does not save the call"""
    e = wc.BY_NAME[name]
    a = e.build("cpu")
    stand, _ = install(monkeypatch, gpu=False)
    with pytest.raises((ValueError, TypeError)):
        e.fn(a)
    assert stand.calls == []


def launching(module):
    """the functions that call an export themselves: by name, or - the float32 / uint8 twins - through ``hip._call_twin``"""
    return sorted(n for n, f in vars(module).items()
                  if inspect.isfunction(f) and f.__module__ == module.__name__ and n != "_call_twin"
                  and ("_ck(lib()." in inspect.getsource(f) or "_call_twin(" in inspect.getsource(f)))


def test_every_launching_wrapper_has_an_entry():
    covered = wc.covered()
    names = {m: launching(m) for m in (hip, hip_train)}
    assert len(names[hip]) == 34 and len(names[hip_train]) == 14, "a wrapper came or went: give it an entry (tests/wrapper_cases.py)"
    missing = [n for m in names for n in names[m] if not covered.get(n)]
    assert missing == []
    # the two private helpers are covered THROUGH their public callers, nothing else is exempt
    assert sorted(covered["_scores_impl"]) == ["attn_map", "scores"] and sorted(covered["_pack_conv_view"]) == ["conv2d_nhwc", "pack_conv_views"]
    for e in wc.ENTRIES:
        assert e.launches and e.align and (e.refuse or e.covers), e.name
