#!/usr/bin/env python
"""ips_image() on uint8 images against ips_image() on the float32 images they stand for ("uint8 images"): whole
synced calls, warmed, the legs alternated in one process - the scheme of tools/patch_view_bench.py, on its four shapes.

    (f) net.ips_image(float32 images)           (u) net.ips_image(uint8 images)
    (f_host) / (u_host): the same with the images on the host, the whole call including their copy to the device

Leg (f) uses only what exists without the view over bytes, so the same file run on the parent commit gives the baseline:

    python tools/view_u8_bench.py --repo <parent checkout> --label parent --out profiles/view_u8_parent.json
    python tools/view_u8_bench.py --parent profiles/view_u8_parent.json --out profiles/view_u8.json

Acceptance (printed and stored per shape): median(u) - median(parent f) <= the parent's own run-to-run spread of (f) (max - min
of its repeats).  Peak memory is the allocator's peak above what is allocated when the leg starts (the images)."""
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
    from ips_amd import quant, synth
    from ips_amd.architecture import IPSNet

    dev = torch.device("cuda:0")
    parent = json.load(open(args.parent))["shapes"] if args.parent else {}
    result = {"label": args.label, "repeats": args.repeats, "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name in args.shapes.split(","):
        kind, over, ishape, patch, stride = SHAPES[name]
        conf = (synth.mnist_conf if kind == "mnist" else synth.traffic_conf)(**over)
        net = synth.fill_weights(IPSNet(dev, conf), 7).to(dev).eval()
        table = (quant.patch_table(3, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)) if ishape[1] == 3 else quant.patch_table(1))
        net.set_patch_table(table)
        host_u8 = torch.randint(0, 256, ishape, dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
        host_f32 = quant.dequant(host_u8, table)
        dev_u8, dev_f32 = host_u8.to(dev), host_f32.to(dev)
        legs = {"f_ips_image_f32": lambda: net.ips_image(dev_f32, patch, stride),
                "f_host_ips_image_f32": lambda: net.ips_image(host_f32, patch, stride)}
        try:                                   # (a commit without the view over bytes refuses them)
            same = torch.equal(net.ips_image(dev_u8, patch, stride)[0], net.ips_image(dev_f32, patch, stride)[0])
            legs["u_ips_image_u8"] = lambda: net.ips_image(dev_u8, patch, stride)
            legs["u_host_ips_image_u8"] = lambda: net.ips_image(host_u8, patch, stride)
        except TypeError:
            same = None
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
        rec = {"patches": ishape[0] * ((ishape[2] - patch[0]) // stride[0] + 1) * ((ishape[3] - patch[1]) // stride[1] + 1),
               "image_bytes_f32": dev_f32.numel() * 4, "image_bytes_u8": dev_u8.numel(),
               "view_calls": getattr(net.selection, "view_calls", None), "mem_patch_equal": same, "legs": {}}
        for k, ts in times.items():
            rec["legs"][k] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "spread_ms": max(ts) - min(ts),
                              "peak_bytes_above_input": int(peaks[k])}
        if name in parent and "u_ips_image_u8" in rec["legs"]:
            pf = parent[name]["legs"]["f_ips_image_f32"]
            u = rec["legs"]["u_ips_image_u8"]["median_ms"]
            rec["parent"] = {k: parent[name]["legs"][k] for k in ("f_ips_image_f32", "f_host_ips_image_f32")}
            rec["u_minus_parent_f_ms"] = u - pf["median_ms"]
            rec["u_no_slower_than_parent_f"] = bool(u - pf["median_ms"] <= pf["spread_ms"])
            rec["u_host_over_parent_f_host"] = (rec["legs"]["u_host_ips_image_u8"]["median_ms"] /
                                                parent[name]["legs"]["f_host_ips_image_f32"]["median_ms"])
        result["shapes"][name] = rec
        print(name, json.dumps(rec["legs"]), {k: rec[k] for k in rec if k.startswith("u_")}, flush=True)
        del net, legs, dev_u8, dev_f32, host_u8, host_f32
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
