#!/usr/bin/env python
"""ips_ragged(pad=True) on batches that hold slides no longer than the memory against what the parent commit can
do with such a batch - the loop of solo ips() calls plus zero buffers filled as ``fill_batch`` of training/iterative.py fills
them.  The protocol is tools/ragged_bench.py's: whole synced calls, warmed, the legs alternated in one process, median and
max - min, peak memory above the resident input.  The slides are device-resident and drawn on the device from a fixed seed.

The ``solo_fill`` and ``ragged`` legs use only what exists without the ``pad`` argument, so the same file run on the parent
commit gives the baseline - the baseline is never the code under test:

    python tools/ragged_pad_bench.py --repo <parent checkout> --label parent --out parent.json
    python tools/ragged_pad_bench.py --parent parent.json --out profiles/ips_ragged_pad.json

The ``*_long`` workloads hold no short slide: there ``pad=True`` against the parent's ``ips_ragged`` sets the one finish launch
(``ipsx_ragged_finish``) against the offset add, the index conversions and the two ``ipsx_gather_rows`` launches it replaces.
Nothing is accepted or refused here."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import torch


def _lengths(short, lo, hi, n_long):
    """The short slides as given, one slide of ``hi`` rows, the others drawn in (lo, hi) from fixed seeds - interleaved."""
    longs = [hi] + [random.Random(2000 + k).randint(lo + 1, hi) for k in range(n_long - 1)]
    out, short = [], list(short)
    while longs or short:
        if longs:
            out.append(longs.pop(0))
        if short and (len(out) % 3 == 2 or not longs):
            out.append(short.pop(0))
    return out


WORKLOADS = {
    # name: (overrides, lengths): 16 slides of 2,048 floats a row
    # the shipped CAMELYON sizes, lengths in [1,200, 38,000], five of them at or below M
    "features_m5000_short": ({"M": 5000, "I": 5000}, _lengths((1200, 2300, 3400, 4500, 5000), 5000, 38000, 11)),
    # M = I = 256, lengths in [100, 65,536], three short
    "features_m256_short": ({"M": 256, "I": 256}, _lengths((100, 180, 256), 256, 65536, 13)),
    # no short slide: pad=True against ips_ragged as the parent has it
    "features_m5000_long": ({"M": 5000, "I": 5000}, [random.Random(1000 + k).randint(12000, 38000) for k in range(16)]),
    "features_m256_long": ({"M": 256, "I": 256}, [random.Random(1000 + k).randint(8192, 65536) for k in range(16)]),
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
    import inspect
    from ips_amd import synth
    from ips_amd.architecture import IPSNet
    from ips_amd.ragged import Ragged

    dev = torch.device("cuda:0")
    parent = json.load(open(args.parent))["workloads"] if args.parent else {}
    has_pad = "pad" in inspect.signature(IPSNet.ips_ragged).parameters
    result = {"label": args.label, "repeats": args.repeats, "device": torch.cuda.get_device_name(0), "workloads": {}}
    for name in args.workloads.split(","):
        over, lengths = WORKLOADS[name]
        conf = synth.camelyon_conf(N=max(lengths), shuffle=False, **over)
        net = synth.fill_weights(IPSNet(dev, conf), 7).to(dev).eval()
        M, B = conf.M, len(lengths)
        g = torch.Generator(device=dev).manual_seed(21)
        rows = torch.randn((sum(lengths), conf.n_chan_in), device=dev, generator=g).relu_()       # post-ReLU features
        slides = list(rows.split(lengths))
        packed = Ragged(rows, lengths)
        n_short = sum(n <= M for n in lengths)

        def solo_fill():          # what the parent can do: init_batch + fill_batch around the solo calls
            buf = torch.zeros((B, M, conf.n_chan_in), device=dev)
            for b, s in enumerate(slides):
                p, _ = net.ips(s[None])
                buf[b:b + 1, :p.shape[1]] = p
            return buf

        legs = {}
        if n_short:
            legs["solo_fill"] = solo_fill
        else:
            legs["ragged"] = lambda: net.ips_ragged(packed)
        if has_pad:
            legs["padded"] = lambda: net.ips_ragged(packed, pad=True)
        times = {k: [] for k in legs}
        peaks = {}
        for rep in range(args.warmup + args.repeats):
            for k, fn in legs.items():
                torch.manual_seed(rep)
                # (a net keeps the embeddings of its last call for last_mem_emb: dropped, so that a leg's peak is its own)
                if hasattr(net, "_reset_last"):
                    net._reset_last()
                else:             # (the parent commit: the baseline)
                    net._emb_parts = net._mem_emb = net._pad_state = None
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
        rec = {"slides": B, "lengths": lengths, "short_slides": n_short, "rows": sum(lengths), "M": M, "I": conf.I,
               "input_bytes": rows.numel() * rows.element_size(), "legs": {}}
        for k, ts in times.items():
            rec["legs"][k] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "spread_ms": max(ts) - min(ts),
                              "rows_per_s": sum(lengths) / (statistics.median(ts) * 1e-3), "peak_bytes_above_input": int(peaks[k])}
        if name in parent:
            base_leg = "solo_fill" if n_short else "ragged"
            p = parent[name]["legs"][base_leg]
            rec["parent_" + base_leg] = p
            for k in rec["legs"]:
                rec["legs"][k]["over_parent"] = rec["legs"][k]["median_ms"] / p["median_ms"]
            if "padded" in rec["legs"]:
                # the condition of DESIGN 2.6: the head's median no more than the parent's own max - min above the parent's
                rec["padded_minus_parent_ms"] = rec["legs"]["padded"]["median_ms"] - p["median_ms"]
                rec["within_parent_spread"] = rec["padded_minus_parent_ms"] <= p["spread_ms"]
        result["workloads"][name] = rec
        print(name, json.dumps(rec["legs"]), flush=True)
        del net, rows, slides, packed, legs
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
