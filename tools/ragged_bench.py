#!/usr/bin/env python
"""ips_ragged() on slides of different lengths against the loop of solo ips() calls it replaces: whole synced
calls, warmed, the legs alternated in one process (the protocol of tools/stream_bench.py).  The slides are device-resident
and drawn on the device from a fixed seed, their lengths from a fixed seed on the host.

The ``solo`` leg uses only what exists without ``ips_ragged``, so the same file run on the parent commit gives the baseline -
the baseline is never the code under test:

    python tools/ragged_bench.py --repo <parent checkout> --label parent --out parent.json
    python tools/ragged_bench.py --parent parent.json --out profiles/ips_ragged.json

Nothing is accepted or refused here.  The ragged call saves the per-call host work and launches of B - 1 calls; it loses the
loop running beside the encoder and, beyond the LDS (M = I = 5000), the team of workgroups per slide - the figures say which
weighs more for a shape.  Peak memory is the allocator's peak above what is allocated when the leg starts (the resident input)."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import torch

WORKLOADS = {
    # name: (configuration, overrides, slides per call, (shortest, longest) slide)
    "features_m256": ("camelyon", {"M": 256, "I": 256, "shuffle": False}, 16, (8192, 65536)),
    "features_m256_shuffle": ("camelyon", {"M": 256, "I": 256, "shuffle": True}, 16, (8192, 65536)),
    "features_m5000": ("camelyon", {"M": 5000, "I": 5000, "shuffle": False}, 16, (12000, 38000)),      # the shipped CAMELYON sizes
    "images_32px": ("mnist", {"M": 64, "I": 64, "shuffle": False}, 16, (1500, 2500)),
}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout to import ips_amd from")
    ap.add_argument("--label", default="head", help="what the figures belong to, e.g. the commit (stored in the JSON)")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--parent", help="JSON this tool wrote on the parent commit: the baseline")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.repo))
    from ips_amd import synth
    from ips_amd.architecture import IPSNet

    dev = torch.device("cuda:0")
    parent = json.load(open(args.parent))["workloads"] if args.parent else {}
    result = {"label": args.label, "repeats": args.repeats, "device": torch.cuda.get_device_name(0), "workloads": {}}
    for name in args.workloads.split(","):
        kind, over, B, (lo, hi) = WORKLOADS[name]
        lengths = [random.Random(1000 + k).randint(lo, hi) for k in range(B)]
        conf = (synth.mnist_conf if kind == "mnist" else synth.camelyon_conf)(N=max(lengths), **over)
        net = synth.fill_weights(IPSNet(dev, conf), 7).to(dev).eval()
        g = torch.Generator(device=dev).manual_seed(21)
        row = (1, 32, 32) if conf.is_image else (conf.n_chan_in,)
        if conf.is_image:      # Megapixel-MNIST's sparsity: most patches blank, the others U[0, 1) (synth.make_patches)
            rows = torch.rand((sum(lengths),) + row, device=dev, generator=g)
            rows = rows * (torch.rand((sum(lengths), 1, 1, 1), device=dev, generator=g) >= 0.93)
        else:                  # post-ReLU features
            rows = torch.randn((sum(lengths),) + row, device=dev, generator=g).relu_()
        slides = list(rows.split(lengths))

        def solo():
            return [net.ips(s[None]) for s in slides]

        legs = {"solo": solo}
        if hasattr(net, "ips_ragged"):
            from ips_amd.ragged import Ragged
            packed = Ragged(rows, lengths)
            legs["ragged"] = lambda: net.ips_ragged(packed)
        times = {k: [] for k in legs}
        peaks = {}
        for rep in range(args.warmup + args.repeats):
            for k, fn in legs.items():
                torch.manual_seed(rep)
                # (a net keeps the embeddings of its last call for last_mem_emb: dropped, so that a leg's peak is its own)
                if hasattr(net, "_reset_last"):
                    net._reset_last()
                else:             # (the parent commit: the baseline)
                    net._emb_parts = net._mem_emb = None
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats(dev)
                base = torch.cuda.memory_allocated(dev)
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                peaks[k] = torch.cuda.max_memory_allocated(dev) - base
                del out
                if rep >= args.warmup:
                    times[k].append(dt)
        rec = {"slides": B, "lengths": lengths, "rows": sum(lengths), "M": conf.M, "I": conf.I, "shuffle": bool(conf.shuffle),
               "input_bytes": rows.numel() * rows.element_size(), "legs": {}}
        for k, ts in times.items():
            rec["legs"][k] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "spread_ms": max(ts) - min(ts),
                              "rows_per_s": sum(lengths) / (statistics.median(ts) * 1e-3), "peak_bytes_above_input": int(peaks[k])}
        if name in parent:
            p = parent[name]["legs"]["solo"]
            rec["parent_solo"] = p
            for k in rec["legs"]:
                rec["legs"][k]["over_parent_solo"] = rec["legs"][k]["median_ms"] / p["median_ms"]
        result["workloads"][name] = rec
        print(name, json.dumps(rec["legs"]), flush=True)
        del net, rows, slides, legs
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
