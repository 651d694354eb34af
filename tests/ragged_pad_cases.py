"""What the tests of ``IPSNet.ips_ragged(slides, pad=True)`` share: the expected record - the loop of solo ``net.ips()`` calls
plus zero buffers filled as ``fill_batch`` of training/iterative.py fills them, as DESIGN 2.6 states the contract - and its
comparison, bit for bit.  Nets and slides come from ``ragged_cases``."""

import json
import os

import numpy as np
import torch
from torch import nn

import ragged_cases as rc
from ips_amd import synth
from ips_amd.architecture import IPSNet

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loop_ragged_pad.npz")


def _seed(seed):
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


def _rng():
    return torch.get_rng_state(), (torch.cuda.get_rng_state() if torch.cuda.is_available() else None)


def lengths(M):
    """Long and short slides mixed: one row beyond the memory, exactly the memory, whole chunks, one row, a ragged end,
    one row short of the memory - a short slide last."""
    return (M + 1, M, 3 * M, 1, 3 * M + 5, M - 1)


@torch.no_grad()
def expected(net, slides, seed=11):
    """The record a padded call must equal, on the host.  A long slide: what ``net.ips(slide[None])`` returns and leaves
    behind.  A short one (N_b <= M): the solo call's result - all N_b rows, nothing drawn - written into zero buffers of M
    slots as ``init_batch`` / ``fill_batch`` do; indices 0 .. N_b-1 then -1; the eval-mode embeddings of its rows and, in
    the padding, the embedding of one all-zero row; no permutation."""
    M, D, dev = net.M, net.D, net.device
    _seed(seed)
    patch, pos, idx, emb, shuf, count = [], [], [], [], [], []
    for s in slides:
        n = s.shape[0]
        p, q = net.ips(s[None])
        assert net.last_mem_count is None
        if n > M:
            e, i, sh = net.last_mem_emb, net.last_mem_idx, net.last_shuffle
        else:
            assert tuple(p.shape[:2]) == (1, n) and net.last_mem_idx is None
            buf = torch.zeros((1, M) + tuple(p.shape[2:]), dtype=p.dtype, device=dev)
            buf[:, :n] = p
            p = buf
            if q is not None:
                buf = torch.zeros((1, M, D), dtype=q.dtype, device=dev)
                buf[:, :n] = q[:, :n]
                q = buf
            i = torch.cat((torch.arange(n), torch.full((M - n,), -1, dtype=torch.int64)))[None]
            x = s.to(dev)
            e = net._embed(x)
            if n < M:
                e = torch.cat((e, net._embed(torch.zeros_like(x[:1])).expand(M - n, -1)))
            e, sh = e[None], None
        patch.append(rc._host(p))
        pos.append(rc._host(q))
        idx.append(rc._host(i))
        emb.append(rc._host(e))
        shuf.append(rc._host(sh))
        count.append(min(n, M))
    rng, rng_cuda = _rng()
    return {"mem_patch": torch.cat(patch), "mem_pos": torch.cat(pos) if pos[0] is not None else None, "mem_idx": torch.cat(idx),
            "mem_emb": torch.cat(emb), "shuffle": shuf if any(s is not None for s in shuf) else None, "count": tuple(count),
            "rng": rng, "rng_cuda": rng_cuda}


@torch.no_grad()
def padded_call(net, slides, seed=11, through_ips=False):
    """``net.ips_ragged(slides, pad=True)`` (``through_ips``: ``net.ips`` on a ``Ragged`` that carries the flag) from the same
    seed -> the same record."""
    _seed(seed)
    p, q = net.ips(slides) if through_ips else net.ips_ragged(slides, pad=True)
    rng, rng_cuda = _rng()
    return {"mem_patch": rc._host(p), "mem_pos": rc._host(q), "mem_idx": rc._host(net.last_mem_idx),
            "mem_emb": rc._host(net.last_mem_emb), "shuffle": rc._host(net.last_shuffle),
            "count": net.last_mem_count, "rng": rng, "rng_cuda": rng_cuda}


def assert_same(got, want):
    for key in ("mem_patch", "mem_pos", "mem_idx", "mem_emb"):
        if want[key] is None:
            assert got[key] is None, key
        else:
            assert got[key] is not None and rc._same(got[key], want[key]), key
    if want["shuffle"] is None:
        assert got["shuffle"] is None
    else:
        assert isinstance(got["shuffle"], list) and len(got["shuffle"]) == len(want["shuffle"])
        for b, (g, w) in enumerate(zip(got["shuffle"], want["shuffle"])):
            if w is None:
                assert g is None, "slide {} is short: no permutation".format(b)
            else:
                assert g is not None and g.shape == w.shape and torch.equal(g, w), "permutation of slide {}".format(b)
    assert got["count"] == want["count"] and all(type(c) is int for c in got["count"])
    assert torch.equal(got["rng"], want["rng"]), "the CPU generator's state"
    if want["rng_cuda"] is not None:
        assert torch.equal(got["rng_cuda"], want["rng_cuda"]), "the device generator's state"


# ------------------------------------------------------------------ tests/golden/loop_ragged_pad.npz
class Recorder:
    def __init__(self):
        self.steps = []

    def update(self, losses, preds, labels):
        self.steps.append((losses, preds, labels))


def fixture_case(z, name, device):
    """-> (conf, net, loader items, criterions) of a case of tests/golden/loop_ragged_pad.npz on ``device``."""
    conf = synth.Conf(**json.loads(str(z[name + "_conf"])))
    net = IPSNet(torch.device(device), conf).to(device)
    synth.fill_weights(net, int(z[name + "_weight_seed"]))
    if conf.use_pos:                # the table of the machine that recorded the fixture (synth.pos_table_record)
        net.pos_enc = synth.pos_table_from(z[name + "_pos_freq"], conf.N).unsqueeze(0).to(device)
    items = synth.make_slide_items(conf, [int(n) for n in z["lengths"]], seed=int(z[name + "_data_seed"]))
    crit = {t['name']: (nn.NLLLoss() if t['act_fn'] == 'softmax' else nn.BCELoss()) for t in conf.tasks.values()}
    return conf, net, items, crit


def check_fixture(z, name, rec, conf, tol):
    """The comparison tests/test_loops_golden.py makes for ``evaluate``."""
    assert len(rec.steps) == int(z[name + "_n_step"])
    for s, (losses, preds, labels) in enumerate(rec.steps):
        for task in conf.tasks.values():
            t = task['name']
            want_pred = z["%s_%d_pred_%s" % (name, s, t)]
            assert preds[t].shape == want_pred.shape and preds[t].dtype == want_pred.dtype
            np.testing.assert_allclose(preds[t], want_pred, rtol=0, atol=tol)
            np.testing.assert_allclose(losses[t], float(z["%s_%d_loss_%s" % (name, s, t)]), rtol=tol * 10, atol=tol * 10)
            want_label = z["%s_%d_label_%s" % (name, s, t)]
            assert labels[t].dtype == want_label.dtype and np.array_equal(labels[t], want_label)
