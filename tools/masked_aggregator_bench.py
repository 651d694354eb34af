#!/usr/bin/env python
"""The masked aggregator against the parent commit's unmasked kernels, at the shipped CAMELYON size:
B = 16, M = 5000, D = 512, H = 8, T = 1.  Two groups - the training step's attention pool (``hip.attn_pool_forward`` +
``hip.attn_pool_backward``) and the eval aggregation (``hip.aggregate``) - and per group four legs:

    parent         the unmasked call on the PARENT commit's library (``--parent-lib``: its libipsx.so, built beforehand)
    unmasked       the unmasked call on this checkout's library (the same export; its kernels are template instantiations now)
    counted_full   (a) count = M for every slide: the counted export over the same rows
    counted_short  (b) the counts of tools/ragged_pad_bench.py's M = 5000 batch (five short slides of sixteen)

The protocol is this repository's: whole synced calls through the Python wrappers (every leg runs the SAME wrapper code, the
library behind ``hip.lib()`` switched), 20 repeats after 3 warm-up calls, the legs alternated in one process, median and
max - min.  ``level`` says whether a leg's median lies within the parent's own max - min of the parent's median.  Nothing is
accepted or refused here.

    python tools/masked_aggregator_bench.py --parent-lib <parent checkout>/ips_amd/lib/libipsx.so --out profiles/masked_aggregator.json"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", required=True, help="libipsx.so built from the parent commit: the baseline")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    from ips_amd import hip, hip_train, synth
    from ips_amd.architecture import IPSNet
    from ragged_pad_bench import WORKLOADS

    head = hip.lib()
    parent = C.CDLL(os.path.abspath(args.parent_lib))
    for name, (res, argtypes) in hip._EXPORTS.items():          # (the parent lacks the counted exports: never called on it)
        if hasattr(parent, name):
            fn = getattr(parent, name)
            fn.restype, fn.argtypes = res, argtypes
    assert not hasattr(parent, "ipsx_aggregate_counted"), "--parent-lib has the counted exports: not the parent commit's library"

    def use(library):
        hip.lib = hip_train.lib = lambda: library

    dev = torch.device("cuda:0")
    B, M = 16, 5000
    conf = synth.camelyon_conf(N=65536, M=M, I=M)
    assert (conf.D, conf.H, conf.n_token) == (512, 8, 1)
    transf = synth.fill_weights(IPSNet(dev, conf), 7).to(dev).transf.eval()
    lengths = WORKLOADS["features_m5000_short"][1]
    short = tuple(min(n, M) for n in lengths)
    assert len(short) == B and sum(c < M for c in short) == 4 and sum(n <= M for n in lengths) == 5
    full = (M,) * B
    g = torch.Generator(device=dev).manual_seed(21)
    x = torch.randn((B, M, conf.D), device=dev, generator=g)
    for b, c in enumerate(short):          # what pad=True leaves: zero rows behind a short slide
        x[b, c:] = 0.0
    R = conf.H * conf.n_token
    A = torch.randn((R, conf.D), device=dev, generator=g) * (2.0 / conf.D ** 0.5)
    dZ = torch.randn((B, R, conf.D), device=dev, generator=g)
    counts = {"full": torch.tensor(full, dtype=torch.int32, device=dev), "short": torch.tensor(short, dtype=torch.int32, device=dev)}

    def node(count):
        Z, P = hip.attn_pool_forward(x, A, None, count) if count is not None else hip.attn_pool_forward(x, A, None)
        if count is not None:
            return hip.attn_pool_backward(x, A, None, P, Z, dZ, count=count)
        return hip.attn_pool_backward(x, A, None, P, Z, dZ)

    def aggregate(count):
        with torch.no_grad():
            return hip.aggregate(transf, x, count) if count is not None else hip.aggregate(transf, x)

    groups = {"train_node_forward_backward": node, "eval_aggregate": aggregate}
    legs = [("parent", parent, None), ("unmasked", head, None), ("counted_full", head, counts["full"]), ("counted_short", head, counts["short"])]
    result = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "warmup": args.warmup,
              "size": {"B": B, "M": M, "D": conf.D, "H": conf.H, "T": conf.n_token}, "short_counts": list(short), "groups": {}}
    for gname, fn in groups.items():
        times = {k: [] for k, _, _ in legs}
        for rep in range(args.warmup + args.repeats):
            for k, library, count in legs:
                use(library)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn(count)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                del out
                if rep >= args.warmup:
                    times[k].append(dt)
        use(head)
        rec = {k: {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "spread_ms": max(ts) - min(ts)}
               for k, ts in times.items()}
        p = rec["parent"]
        for k in rec:
            if k != "parent":
                rec[k]["minus_parent_ms"] = rec[k]["median_ms"] - p["median_ms"]
                rec[k]["level"] = abs(rec[k]["minus_parent_ms"]) <= p["spread_ms"]
        rec["counted_short"]["minus_counted_full_ms"] = rec["counted_short"]["median_ms"] - rec["counted_full"]["median_ms"]
        result["groups"][gname] = rec
        print(gname, json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
