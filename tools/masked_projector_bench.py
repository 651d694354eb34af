#!/usr/bin/env python
"""The masked encoder pass of the feature projector at the shipped CAMELYON size: B = 16, M = 5000, F = 2048,
D = 512 - the training step's projector node, forward + backward (``fused_projector.encode`` and the backward of its
result), on 80,000 padded rows.  Five legs:

    parent          the uncounted node on all 80,000 rows, on the PARENT commit's library (``--parent-lib``, built beforehand)
    uncounted       the same on this checkout's library (the plain exports: the `false` instantiations)
    indexed_full    ``encode(rows=)`` with every count = M: the index's own cost
    indexed_short   ``encode(rows=)`` with the counts of tools/ragged_pad_bench.py's M = 5000 batch (n_fill = 71,400)
    generic_short   the generic route on those counts: ``x.index_select(0, rows)``, then the uncounted node on the copy

The protocol is this repository's: whole synced calls through the Python wrappers (every leg runs the SAME wrapper code, the
library behind ``hip.lib()`` switched), 20 repeats after 3 warm-up calls, the legs alternated in one process, median and
max - min.  Peak memory above what is allocated before the call (input, weights, the caller's gradient) is taken once per leg
behind the timed repeats.  Nothing is accepted or refused here.

    python tools/masked_projector_bench.py --parent-lib <parent checkout>/ips_amd/lib/libipsx.so --out profiles/masked_projector.json"""
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
    from ips_amd import hip, hip_encoder, hip_train, synth
    from ips_amd.architecture import IPSNet
    from ips_amd.training import fused_projector
    from ragged_pad_bench import WORKLOADS

    head = hip.lib()
    parent = C.CDLL(os.path.abspath(args.parent_lib))
    for name, (res, argtypes) in hip._EXPORTS.items():          # (the parent lacks the indexed exports: never called on it)
        if hasattr(parent, name):
            fn = getattr(parent, name)
            fn.restype, fn.argtypes = res, argtypes
    assert not hasattr(parent, "ipsx_projector_wgrad_indexed"), "--parent-lib has the indexed exports: not the parent commit's library"

    def use(library):
        hip.lib = hip_train.lib = hip_encoder.lib = lambda: library

    dev = torch.device("cuda:0")
    B, M = 16, 5000
    conf = synth.camelyon_conf(N=65536, M=M, I=M)
    F, D = conf.n_chan_in, conf.D
    assert (F, D) == (2048, 512)
    enc = synth.fill_weights(IPSNet(dev, conf), 7).to(dev).encoder.train()
    assert fused_projector.supported(enc)
    lengths = WORKLOADS["features_m5000_short"][1]
    short = tuple(min(n, M) for n in lengths)
    assert len(short) == B and sum(short) == 71400

    def index(counts):
        return torch.cat([torch.arange(b * M, b * M + c, dtype=torch.int32) for b, c in enumerate(counts)]).to(dev)

    rows = {"full": index((M,) * B), "short": index(short)}
    rows64 = rows["short"].long()
    g = torch.Generator(device=dev).manual_seed(21)
    x = torch.randn((B * M, F), device=dev, generator=g)
    xv = x.view(B, M, F)
    for b, c in enumerate(short):          # what pad=True leaves: zero rows behind a short slide
        xv[b, c:] = 0.0
    dy = {n: torch.randn((n, D), device=dev, generator=g) for n in (B * M, sum(short))}

    def node(leg):
        if leg == "indexed_full":
            y = fused_projector.encode(enc, x, rows=rows["full"])
        elif leg == "indexed_short":
            y = fused_projector.encode(enc, x, rows=rows["short"])
        elif leg == "generic_short":
            y = fused_projector.encode(enc, x.index_select(0, rows64))
        else:
            y = fused_projector.encode(enc, x)
        y.backward(dy[y.shape[0]])
        return y

    legs = [("parent", parent), ("uncounted", head), ("indexed_full", head), ("indexed_short", head), ("generic_short", head)]
    result = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "warmup": args.warmup,
              "size": {"B": B, "M": M, "F": F, "D": D}, "short_counts": list(short), "n_fill": sum(short)}
    times = {k: [] for k, _ in legs}
    for rep in range(args.warmup + args.repeats):
        for k, library in legs:
            use(library)
            enc.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = node(k)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            del out
            if rep >= args.warmup:
                times[k].append(dt)
    rec = {k: {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "spread_ms": max(ts) - min(ts)}
           for k, ts in times.items()}
    for k, library in legs:                 # peak memory above what lies there before the call
        use(library)
        enc.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = node(k)
        torch.cuda.synchronize()
        rec[k]["peak_above_input_mb"] = (torch.cuda.max_memory_allocated() - base) / 1e6
        del out
    use(head)
    p = rec["parent"]
    for k in rec:
        if k != "parent":
            rec[k]["minus_parent_ms"] = rec[k]["median_ms"] - p["median_ms"]
            rec[k]["level"] = abs(rec[k]["minus_parent_ms"]) <= p["spread_ms"]
    gen = rec["generic_short"]
    rec["indexed_short"]["minus_generic_short_ms"] = rec["indexed_short"]["median_ms"] - gen["median_ms"]
    rec["indexed_short"]["no_slower_than_generic"] = rec["indexed_short"]["minus_generic_short_ms"] <= gen["spread_ms"]
    result["legs"] = rec
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
