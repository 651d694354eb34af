#!/usr/bin/env python
"""Blank-patch dedup on the sources of the counted launch that went without it: whole synced calls of
``ips_image()`` / ``ips()``, warmed, the legs of a shape alternated in one process.

    shapes    16 x 1x1600x1600 at stride 32 (2,500 patches per image), at stride 16 (9,801), 16 x 2,500 patches
    storage   float32 images, uint8 images, uint8 patches - the byte legs under IPSX_ONE_LAUNCH_U8=1
    content   "mnist": the bench workload's patches (synth.make_patches, 93 % blank) folded onto a dense canvas, stored as
              bytes (ceil(255 x): what is non-zero stays non-zero), the float32 images their expansion through ToTensor's
              table - one content for every storage kind;  "dense": no zero byte anywhere

The legs use nothing but ``set_patch_table``, ``ips`` and ``ips_image``, so the same file run on the parent commit gives the
baseline - never the head with the switch off:

    python tools/dedup_sources_bench.py --repo <parent checkout> --label parent --out parent.json
    python tools/dedup_sources_bench.py --parent parent.json --out profiles/dedup_sources.json

Two conditions per leg, stored and printed: (1) "mnist": the head's median is below the parent's by more than the parent's own
max - min;  (2) "dense": the head's median exceeds the parent's by no more than the parent's max - min.
``--legs`` narrows the run to legs whose name contains one of the given strings (a kernel trace of one kind)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

SHAPES = {
    # name: (N of the configuration, stride | None: the patch tensor itself, storage kinds)
    "images_s32": (2500, (32, 32), ("f32", "u8")),
    "images_s16": (9801, (16, 16), ("f32", "u8")),
    "patches": (2500, None, ("u8",)),
}
CONTENTS = ("mnist", "dense")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout to import ips_amd from")
    ap.add_argument("--label", default="head", help="what the figures belong to, e.g. the commit (stored in the JSON)")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--legs", default="", help="comma-separated substrings: only the legs whose name holds one of them")
    ap.add_argument("--parent", help="JSON this tool wrote on the parent commit: the baseline of the two conditions")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    os.environ["IPSX_ONE_LAUNCH_U8"] = "1"
    os.environ.pop("IPSX_DEDUP_BLANK", None)
    sys.path.insert(0, os.path.abspath(args.repo))
    from ips_amd import quant, synth
    from ips_amd.architecture import IPSNet

    dev = torch.device("cuda:0")
    B = 16
    table = quant.patch_table(1)
    # the two contents as (B, 2500, 1, 32, 32) bytes and as the (B, 1, 1600, 1600) canvas they tile
    floats = synth.make_patches(synth.mnist_conf(N=2500), B, seed=21)
    stored = {"mnist": torch.ceil(floats * 255).to(torch.uint8),
              "dense": torch.from_numpy(np.random.default_rng(5).integers(1, 256, (B, 2500, 1, 32, 32), dtype=np.uint8))}
    assert bool(((stored["mnist"] == 0) == (floats == 0)).all())
    canvas = {k: q.reshape(B, 50, 50, 32, 32).permute(0, 1, 3, 2, 4).reshape(B, 1, 1600, 1600).contiguous() for k, q in stored.items()}
    parent = json.load(open(args.parent))["legs"] if args.parent else {}
    wanted = [w for w in args.legs.split(",") if w]
    result = {"label": args.label, "repeats": args.repeats, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "legs": {}}
    for shape in args.shapes.split(","):
        N, stride, kinds = SHAPES[shape]
        net = synth.fill_weights(IPSNet(dev, synth.mnist_conf(N=N)), 7).to(dev).eval()
        net.set_patch_table(table)
        legs, blank = {}, {}
        for content in CONTENTS:
            q = (stored[content] if stride is None else canvas[content]).to(dev)
            if stride is None:
                share = float((stored[content].reshape(B * 2500, -1) == 0).all(1).float().mean())
            else:
                u = canvas[content].unfold(2, 32, stride[0]).unfold(3, 32, stride[1])
                share = float((u == 0).all(-1).all(-1).float().mean())
            for kind in kinds:
                x = q if kind == "u8" else quant.dequant(q, table.to(dev))
                name = "%s %s %s" % (shape, kind, content)
                if wanted and not any(w in name for w in wanted):
                    continue
                legs[name] = (lambda x=x: net.ips(x)) if stride is None else (lambda x=x: net.ips_image(x, (32, 32), stride))
                blank[name] = share
        times = {k: [] for k in legs}
        encoded = {}
        for rep in range(args.warmup + args.repeats):
            for k, fn in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                del out
                held = getattr(net.selection.plan(), "n_encoded", None)
                encoded[k] = None if held is None else int(held.item())
                if rep >= args.warmup:
                    times[k].append(dt)
        for k, ts in times.items():
            rec = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "spread_ms": max(ts) - min(ts),
                   "patches": B * N, "blank_share": blank[k], "n_encoded": encoded[k]}
            if k in parent:
                p = parent[k]
                rec["parent"] = {f: p[f] for f in ("median_ms", "min_ms", "max_ms", "spread_ms")}
                rec["head_minus_parent_ms"] = rec["median_ms"] - p["median_ms"]
                if k.endswith("mnist"):
                    rec["faster_by_more_than_parent_spread"] = bool(p["median_ms"] - rec["median_ms"] > p["spread_ms"])
                else:
                    rec["no_slower_than_parent_spread"] = bool(rec["median_ms"] - p["median_ms"] <= p["spread_ms"])
            result["legs"][k] = rec
            print(k, json.dumps(rec), flush=True)
        del net, legs
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
