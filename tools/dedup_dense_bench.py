#!/usr/bin/env python
"""What exact blank-patch dedup inside the counted launch (IPSX_DEDUP_BLANK unset = auto) costs where it gains nothing, and
what its blank embedding costs after a weight update.  The headline shape (16 x 2,500 patches of 1x32x32, M = I = 64), whole
synced ips() calls, in ONE process with the legs alternated call by call (the switch is read per call):

  dense     make_patches(..., blank_frac=0): `auto` against IPSX_DEDUP_BLANK=0.  The scan reads a KiB of every patch and finds
            nothing; the criterion is that the `auto` median exceeds the other's by no more than that leg's own max - min.
  update    the headline's data (93 % blank), every call behind hip.weights_changed(): the plan packs its weights again in
            both legs, `auto` also encodes its one zero patch again - the difference of the medians is that launch.

    python tools/dedup_dense_bench.py [--repeats 20] [--warmup 3]        -> one JSON line"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ips_amd import hip, synth                                    # noqa: E402
from ips_amd.architecture import IPSNet                           # noqa: E402

LEGS = (("auto", None), ("off", "0"))


def set_leg(value):
    if value is None:
        os.environ.pop("IPSX_DEDUP_BLANK", None)
    else:
        os.environ["IPSX_DEDUP_BLANK"] = value


def timed(net, x, bump):
    if bump:
        hip.weights_changed()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    net.ips(x)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def measure(net, x, repeats, warmup, bump):
    ms = {name: [] for name, _ in LEGS}
    for k in range(warmup + repeats):
        for name, value in (LEGS if k % 2 == 0 else LEGS[::-1]):   # alternated, and neither leg always first
            set_leg(value)
            t = timed(net, x, bump)
            if k >= warmup:
                ms[name].append(t)
    return {name: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "spread_ms": max(v) - min(v)}
            for name, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    conf = synth.mnist_conf()
    net = synth.fill_weights(IPSNet(dev, conf), 7).to(dev).eval()
    dense = synth.make_patches(conf, 16, seed=21, blank_frac=0).to(dev)
    sparse = synth.make_patches(conf, 16, seed=21).to(dev)
    out = {"shape": list(dense.shape), "repeats": args.repeats, "warmup": args.warmup}
    out["dense"] = d = measure(net, dense, args.repeats, args.warmup, False)
    excess = d["auto"]["median_ms"] - d["off"]["median_ms"]
    out["dense"]["auto_minus_off_ms"] = excess
    out["dense"]["within_spread"] = bool(excess <= d["off"]["spread_ms"])
    out["headline"] = measure(net, sparse, args.repeats, args.warmup, False)
    out["update"] = u = measure(net, sparse, args.repeats, args.warmup, True)
    # the blank embedding's share: what a weight update adds under `auto` beyond what it adds without dedup
    out["update"]["blank_embedding_ms"] = ((u["auto"]["median_ms"] - out["headline"]["auto"]["median_ms"]) -
                                           (u["off"]["median_ms"] - out["headline"]["off"]["median_ms"]))
    set_leg(None)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
