#!/usr/bin/env python
"""ips() on a patch tensor against ips_image() on the images themselves: whole synced calls, warmed, the legs
alternated in one process.

    (a) hip.patchify(images) + net.ips(patches)      (b) net.ips(patches) alone      (c) net.ips_image(images)

Legs (a) and (b) use only what exists without the patch view, so the same file run on the parent commit gives the baseline:

    python tools/patch_view_bench.py --repo <parent checkout> --label parent --out parent.json
    python tools/patch_view_bench.py --parent parent.json --out profiles/patch_view.json

Acceptance (printed and stored per shape): median(c) - median(parent b) <= the parent's own run-to-run spread of (b)
(max - min of its repeats).  Peak memory is the allocator's peak above what is allocated when the leg starts (the images,
and for (b) the patch tensor too)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

SHAPES = {
    # name: (configuration, its overrides, image batch, patch, stride)
    "mnist_16x1600_s32": ("mnist", dict(N=2500), (16, 1, 1600, 1600), (32, 32), (32, 32)),
    "mnist_16x1600_s16": ("mnist", dict(N=9801), (16, 1, 1600, 1600), (32, 32), (16, 16)),
    "mnist50_16x1500_s25": ("mnist", dict(N=3481, patch=50), (16, 1, 1500, 1500), (50, 50), (25, 25)),
    "traffic_16x1200x1600": ("traffic", dict(N=192), (16, 3, 1200, 1600), (100, 100), (100, 100)),
}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout to import ips_amd from")
    ap.add_argument("--label", default="head", help="what the figures belong to, e.g. the commit (stored in the JSON)")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--parent", help="JSON this tool wrote on the parent commit: the baseline of the acceptance")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.repo))
    from ips_amd import hip, synth
    from ips_amd.architecture import IPSNet

    dev = torch.device("cuda:0")
    parent = json.load(open(args.parent))["shapes"] if args.parent else {}
    result = {"label": args.label, "repeats": args.repeats, "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name in args.shapes.split(","):
        kind, over, ishape, patch, stride = SHAPES[name]
        conf = (synth.mnist_conf if kind == "mnist" else synth.traffic_conf)(**over)
        net = synth.fill_weights(IPSNet(dev, conf), 7).to(dev).eval()
        images = torch.randn(ishape, generator=torch.Generator().manual_seed(1)).to(dev)
        patches = hip.patchify(images, patch, stride)
        legs = {"a_patchify_ips": lambda: net.ips(hip.patchify(images, patch, stride)),
                "b_ips": lambda: net.ips(patches)}
        if hasattr(net, "ips_image"):
            legs["c_ips_image"] = lambda: net.ips_image(images, patch, stride)
        times = {k: [] for k in legs}
        peaks = {}
        for rep in range(args.warmup + args.repeats):
            for k, fn in legs.items():
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
        rec = {"patches": int(patches.shape[0] * patches.shape[1]), "image_bytes": images.numel() * 4,
               "patch_tensor_bytes": patches.numel() * 4, "view_calls": getattr(net.selection, "view_calls", None), "legs": {}}
        for k, ts in times.items():
            rec["legs"][k] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "spread_ms": max(ts) - min(ts),
                              "peak_bytes_above_input": int(peaks[k])}
        if name in parent and "c_ips_image" in rec["legs"]:
            pb = parent[name]["legs"]["b_ips"]
            pa = parent[name]["legs"]["a_patchify_ips"]
            c = rec["legs"]["c_ips_image"]["median_ms"]
            rec["parent"] = {"a_patchify_ips": pa, "b_ips": pb}
            rec["c_minus_parent_b_ms"] = c - pb["median_ms"]
            rec["c_no_slower_than_parent_b"] = bool(c - pb["median_ms"] <= pb["spread_ms"])
            rec["c_over_parent_a"] = c / pa["median_ms"]
        result["shapes"][name] = rec
        print(name, json.dumps(rec["legs"]), {k: rec[k] for k in rec if k.startswith("c_")}, flush=True)
        del net, images, patches, legs
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
