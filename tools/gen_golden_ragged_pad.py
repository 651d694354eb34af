#!/usr/bin/env python
"""Generate tests/golden/loop_ragged_pad.npz by RUNNING THE REFERENCE's own ``evaluate`` (training/iterative.py, imported through
tools/refimport) on a B = 4, B_seq = 1 loader of slides of DIFFERENT lengths, some of them no longer than the memory:
40, 16, 7, 33, 17 and 1 rows at M = I = 16.  Such a slide takes the M >= N shortcut of ``ips()`` and ``fill_batch`` writes
its rows into the zero-initialised (B, M, ...) buffers; the padded rows go through the encoder and the aggregator like any
others.  ``IPSNet.ips_ragged(slides, pad=True)`` builds that batch directly (tests/test_ragged_pad_cpu.py and
tests/test_ragged_pad.py run ``evaluate`` over ``collate_ragged_padded`` batches against this record).

(The file carries the ``loop_`` prefix of the other loop fixtures: tests/util.py takes every other .npz for a selection case.)
The fixture holds what the loop hands its log writer per step (task losses, predictions, labels), the configurations and the
seeds the inputs are regenerated from (``synth.make_slide_items``) - data only.

Two cases: ``feature`` - a feature net, 'batch' shuffling on (short slides draw nothing) - and ``image`` - the 32-px image
net with positions on.  With positions the reference's ``fill_batch`` takes the table a short slide's ``ips()`` returns only
when the net was built for exactly that many patches (``mem_pos_enc[:, :len_seq] = pos_enc`` needs conf.N == N_b), so the
loader below hands the net, before such an item, the table ``pos_enc_1d(D, N_b)`` a net built for N_b patches owns - bit for
bit the first N_b rows of the table for conf.N, which is what the padded call writes - and the table for conf.N before a
long one.  Nothing of the reference's code is changed or copied.

    python tools/gen_golden_ragged_pad.py
"""

import json
import os
import sys

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np
import torch
from torch import nn
from torch.utils.data import DataLoader, Dataset

from ips_amd import synth
from tools.refimport import import_reference, import_reference_training

GOLDEN = os.path.join(REPO, "tests", "golden")
LENGTHS = (40, 16, 7, 33, 17, 1)

# name -> (conf, weight seed, data seed, torch seed)
CASES = {
    "feature": (synth.camelyon_conf(N=96, M=16, I=16, n_chan_in=64, D=64, D_k=8, D_v=8, D_inner=128, B=4, B_seq=1,
                                    shuffle=True, shuffle_style='batch'), 41, 51, 9),
    "image": (synth.mnist_conf(N=40, M=16, I=16, B=4, B_seq=1), 42, 52, 10),
}


class Recorder:
    def __init__(self):
        self.steps = []

    def update(self, losses, preds, labels):
        self.steps.append((dict(losses), {k: np.array(v) for k, v in preds.items()},
                           {k: np.array(v) for k, v in labels.items()}))


class SoloSlides(Dataset):
    """The B_seq = 1 dataset: one slide per item, (1, N_k, ...) with (1,) labels, read in order by a ``DataLoader`` without
    workers (like any ``DataLoader`` it draws its base seed from torch's generator when the loop starts iterating - as the
    one the tests build does).  With positions on, the net owns the table of the slide's own length before a short item
    (see the module docstring)."""

    def __init__(self, items, net, conf, pos_enc_1d):
        self.items, self.net, self.conf, self.pos_enc_1d = items, net, conf, pos_enc_1d

    def __len__(self):
        return len(self.items)

    def __getitem__(self, k):
        item = self.items[k]
        n = item['input'].shape[0]
        if self.conf.use_pos:
            self.net.pos_enc = self.pos_enc_1d(self.conf.D, n if n <= self.conf.M else self.conf.N).unsqueeze(0)
        return {k: v.unsqueeze(0) for k, v in item.items()}


def run_case(name, ref_ips, ref_transf, ref_loop, out):
    conf, wseed, dseed, tseed = CASES[name]
    items = synth.make_slide_items(conf, LENGTHS, seed=dseed)
    net = ref_ips.IPSNet(torch.device("cpu"), conf)
    synth.fill_weights(net, wseed)
    if conf.use_pos:
        full = ref_transf.pos_enc_1d(conf.D, conf.N)
        for n in LENGTHS:
            if n <= conf.M:
                assert torch.equal(ref_transf.pos_enc_1d(conf.D, n), full[:n]), n       # the prefix IS the shorter net's table
        out[name + "_pos_freq"] = synth.pos_table_record(conf)["pos_freq"]
    crit = {t['name']: (nn.NLLLoss() if t['act_fn'] == 'softmax' else nn.BCELoss()) for t in conf.tasks.values()}
    rec = Recorder()
    torch.manual_seed(tseed)
    loader = DataLoader(SoloSlides(items, net, conf, ref_transf.pos_enc_1d), batch_size=None, shuffle=False)
    ref_loop.evaluate(net, crit, loader, torch.device("cpu"), rec, conf)
    out[name + "_conf"] = json.dumps(conf.__dict__)
    out[name + "_weight_seed"], out[name + "_data_seed"], out[name + "_torch_seed"] = wseed, dseed, tseed
    out[name + "_n_step"] = len(rec.steps)
    for s, (losses, preds, labels) in enumerate(rec.steps):
        for task in conf.tasks.values():
            t = task['name']
            out["%s_%d_loss_%s" % (name, s, t)] = np.float64(losses[t])
            out["%s_%d_pred_%s" % (name, s, t)] = preds[t]
            out["%s_%d_label_%s" % (name, s, t)] = labels[t]
    print("{:8s} eval steps {}  losses {}".format(name, len(rec.steps), [sorted(l.items()) for l, _, _ in rec.steps]))


def main():
    ref_ips, ref_transf, _ = import_reference()
    ref_loop = import_reference_training()
    out = {"lengths": np.array(LENGTHS, dtype=np.int64)}
    for name in CASES:
        run_case(name, ref_ips, ref_transf, ref_loop, out)
    np.savez_compressed(os.path.join(GOLDEN, "loop_ragged_pad.npz"), **out)


if __name__ == "__main__":
    main()
