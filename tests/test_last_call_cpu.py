"""What a selection leaves on the net - ``last_mem_idx``, ``last_mem_emb``, ``last_shuffle``, ``last_mem_count`` - belongs to
that selection alone: after any entry point, whatever ran on the net before and whether or not its embeddings were read,
the four hold bit for bit what a fresh net with the same weights holds after that call from the same seed.  Every ordered
pair of the six ways into a selection, on the CPU plumbing path; the first call of a pair runs on inputs of another
length than the second."""

import itertools

import pytest
import torch
import torch.distributed as torch_dist

import ragged_cases as rc
from ips_amd import dist

M, I, B = 8, 4, 2
SEED = 11
CONF = rc.feature_conf(M=M, shuffle=True, shuffle_style='batch', use_pos=False).clone(I=I)


def _batch(n, seed):
    return torch.stack(rc.make_slides(CONF, (n,) * B, seed=seed))


def _ips_long(net, first):
    net.ips(_batch(23 if first else 30, 5))


def _ips_short(net, first):                        # the M >= N shortcut
    net.ips(_batch(5 if first else M, 6))


def _ragged(net, first):
    net.ips_ragged(rc.make_slides(CONF, (9, 21) if first else (30, 13), seed=7))


def _ragged_pad(net, first):                       # one short slide
    net.ips_ragged(rc.make_slides(CONF, (3, 17) if first else (26, M - 1), seed=8), pad=True)


def _stream(net, first):
    x = _batch(19 if first else 27, 9)
    s = net.ips_stream()
    s.feed(x[:, :10])
    s.feed(x[:, 10:])
    s.finish()


def _sharded(net, first):
    x = _batch(22 if first else 29, 10)
    dist.ips_sharded(net, x.contiguous(), x.shape[1])


CALLS = {"ips": _ips_long, "ips_all": _ips_short, "ragged": _ragged, "ragged_pad": _ragged_pad, "stream": _stream,
         "sharded": _sharded}


PAIRS = list(itertools.product(CALLS, CALLS))


@pytest.fixture(scope="module")
def one_rank(tmp_path_factory):
    """A single-process group, as tests/test_dedup_switch_cpu.py sets one up."""
    store = tmp_path_factory.mktemp("last_call") / "store"
    torch_dist.init_process_group("gloo", init_method="file://{}".format(store), rank=0, world_size=1)
    yield
    torch_dist.destroy_process_group()


def _left(net):
    return {"last_mem_idx": net.last_mem_idx, "last_mem_emb": net.last_mem_emb, "last_shuffle": net.last_shuffle,
            "last_mem_count": net.last_mem_count}


def _second(net, name):
    torch.manual_seed(SEED)
    CALLS[name](net, False)
    return _left(net)


@pytest.fixture(scope="module")
def alone(one_rank):
    """What a fresh net holds after each call alone: made once, never changed."""
    return {name: _second(rc.make_net(CONF, "cpu"), name) for name in CALLS}


def _equal(got, want):
    if want is None or got is None:
        return got is None and want is None
    if isinstance(want, (list, tuple)):
        return type(got) is type(want) and len(got) == len(want) and all(_equal(g, w) for g, w in zip(got, want))
    if torch.is_tensor(want):
        return torch.is_tensor(got) and rc._same(got, want)
    return type(got) is type(want) and got == want


def test_the_calls_leave_what_they_should(alone):
    """The references themselves: every kind of leftover occurs, so that the pairs below compare more than Nones."""
    for name in ("ips", "ragged", "ragged_pad", "stream"):
        assert tuple(alone[name]["last_mem_idx"].shape) == (B, M) and tuple(alone[name]["last_mem_emb"].shape) == (B, M, CONF.D)
    assert all(v is None for v in alone["ips_all"].values())
    assert torch.is_tensor(alone["ips"]["last_shuffle"]) and isinstance(alone["ragged"]["last_shuffle"], list)
    assert alone["ragged_pad"]["last_shuffle"][1] is None and alone["ragged_pad"]["last_mem_count"] == (M, M - 1)
    assert alone["stream"]["last_shuffle"] is None
    assert [k for k, v in alone["sharded"].items() if v is not None] == ["last_mem_idx"]
    assert all(alone[name]["last_mem_count"] is None for name in CALLS if name != "ragged_pad")


@pytest.mark.parametrize("read_between", [False, True], ids=["unread", "read"])
@pytest.mark.parametrize("first,second", PAIRS, ids=["-".join(p) for p in PAIRS])
def test_nothing_outlives_its_call(alone, first, second, read_between):
    net = rc.make_net(CONF, "cpu")
    torch.manual_seed(SEED + 1)
    CALLS[first](net, True)
    if read_between:
        net.last_mem_emb
    got = _second(net, second)
    for key, want in alone[second].items():
        assert _equal(got[key], want), "{} after {} then {}".format(key, first, second)
