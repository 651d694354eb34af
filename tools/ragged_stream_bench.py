#!/usr/bin/env python
"""ips_ragged_stream() against the ips_ragged() call it bounds the memory of: whole synced calls, warmed, the
legs alternated in one process (the protocol of tools/ragged_bench.py), on a device-resident and on a host-resident (pinned)
batch.  Legs: ``ips_ragged`` on each batch - the reference -, and the ragged stream fed whole and in slabs of 65,536 and
8,192 packed rows (``feed_all``) on each batch.

The ``ragged_*`` legs use only what exists without ``ips_ragged_stream``, so the same file run on the parent commit gives the
baseline - the baseline is never the code under test:

    python tools/ragged_stream_bench.py --repo <parent checkout> --label parent --out parent.json
    python tools/ragged_stream_bench.py --parent parent.json --out profiles/ips_ragged_stream.json

Nothing is accepted or refused here.  Peak memory is the allocator's peak above what is allocated when the leg starts: the
input for the device-resident legs, nothing for the host-resident ones (the device copy of the input is then part of the
peak - the whole batch for ``ips_ragged``, one slab for the stream)."""
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
    "features_m5000": ("camelyon", {"M": 5000, "I": 5000, "shuffle": False}, 16, (12000, 38000)),      # the shipped CAMELYON sizes
    "images_32px": ("mnist", {"M": 64, "I": 64, "shuffle": False}, 16, (1500, 2500)),
}
SLABS = (65536, 8192)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout to import ips_amd from")
    ap.add_argument("--label", default="head", help="what the figures belong to, e.g. the commit (stored in the JSON)")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--legs", default="", help="only the legs whose names start with one of these (comma-separated); default: all")
    ap.add_argument("--parent", help="JSON this tool wrote on the parent commit: the baseline")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.repo))
    from ips_amd import synth
    from ips_amd.architecture import IPSNet
    from ips_amd.ragged import Ragged

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
        host = Ragged(rows.cpu().pin_memory(), lengths)
        del rows
        torch.cuda.empty_cache()

        legs = {"ragged_host": lambda: net.ips_ragged(host)}
        if hasattr(net, "ips_ragged_stream"):
            legs["stream_whole_host"] = lambda: net.ips_ragged_stream().feed(host).finish()
            for slab in SLABS:
                legs["stream_%d_host" % slab] = lambda slab=slab: net.ips_ragged_stream().feed_all(host, slab).finish()
        on_dev = {"ragged_device": lambda d: net.ips_ragged(d)}
        if hasattr(net, "ips_ragged_stream"):
            on_dev["stream_whole_device"] = lambda d: net.ips_ragged_stream().feed(d).finish()
            for slab in SLABS:
                on_dev["stream_%d_device" % slab] = lambda d, slab=slab: net.ips_ragged_stream().feed_all(d, slab).finish()
        if args.legs:
            keep = tuple(args.legs.split(","))
            legs = {k: v for k, v in legs.items() if k.startswith(keep)}
            on_dev = {k: v for k, v in on_dev.items() if k.startswith(keep)}
        times = {k: [] for k in list(legs) + list(on_dev)}
        peaks = {}

        def run(k, fn):
            torch.manual_seed(rep)
            net._reset_last()          # (a net keeps the embeddings of its last call: dropped, so that a leg's peak is its own)
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

        # (the host-resident legs first, with nothing resident; then the batch is put on the device once for the others)
        for rep in range(args.warmup + args.repeats):
            for k, fn in legs.items():
                run(k, fn)
        resident = host.to(dev)
        for rep in range(args.warmup + args.repeats):
            for k, fn in on_dev.items():
                run(k, lambda: fn(resident))
        rec = {"slides": B, "lengths": lengths, "rows": sum(lengths), "M": conf.M, "I": conf.I,
               "input_bytes": host.rows.numel() * host.rows.element_size(), "legs": {}}
        for k, ts in times.items():
            rec["legs"][k] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "spread_ms": max(ts) - min(ts),
                              "rows_per_s": sum(lengths) / (statistics.median(ts) * 1e-3), "peak_bytes_above_resident": int(peaks[k])}
        if name in parent:
            rec["parent"] = {k: parent[name]["legs"][k] for k in ("ragged_host", "ragged_device")}
            for k in rec["legs"]:
                p = rec["parent"]["ragged_host" if k.endswith("_host") else "ragged_device"]
                rec["legs"][k]["over_parent_ragged"] = rec["legs"][k]["median_ms"] / p["median_ms"]
        result["workloads"][name] = rec
        print(name, json.dumps(rec["legs"]), flush=True)
        del net, host, resident, legs, on_dev
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
