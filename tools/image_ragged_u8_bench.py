#!/usr/bin/env python
"""ips_image_ragged() on uint8 images of different sizes against what a caller had before the ragged routes took bytes (DESIGN
2.8): the loop of solo ips_image(uint8[None]) calls, and ips_image_ragged() on the float32 expansion.  The protocol of
tools/image_ragged_bench.py and its shapes: whole synced calls, 20 repeats after 3, the legs alternated in one process, median
with max - min; 16 images 1,100 - 1,700 px a side, drawn from fixed seeds as bytes, the float32 images their expansion through
``quant.patch_table``.

The baselines use only what exists without this feature, so the same file run on the parent commit gives them - the baseline
is never the code under test:

    python tools/image_ragged_u8_bench.py --repo <parent checkout> --label parent --out parent.json
    python tools/image_ragged_u8_bench.py --parent parent.json --out profiles/ips_image_ragged_u8.json

Legs, device-resident input: ``solo_u8`` (the loop of ips_image(uint8[None])), ``ragged_f32`` (ips_image_ragged on the packed
float32 expansion) and - where the tree takes them - ``ragged_u8`` (ips_image_ragged on the packed bytes).  Host-resident
input in pinned memory, the copy inside the timed call: ``host_ragged_f32`` and ``host_ragged_u8`` - a quarter of the bytes
across the bus.  Peak memory is the allocator's peak above what is allocated when the leg starts (the resident input).  Nothing is
accepted or refused here; ``u8_slower_than_f32_beyond_spread`` says where the byte call's median lies above the float32 ragged
call's by more than that leg's own max - min."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import torch

WORKLOADS = {
    # name: (configuration, overrides, images per call, (shortest, longest) side, patch, stride)
    "fused32_stride32": ("mnist", {}, 16, (1100, 1700), 32, 32),
    "fused32_stride16": ("mnist", {}, 16, (1100, 1700), 32, 16),
    "pool50_stride25": ("mnist", {"patch": 50}, 16, (1100, 1700), 50, 25),
    "pool100x3_stride100": ("traffic", {}, 16, (1100, 1700), 100, 100),
}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout to import ips_amd from")
    ap.add_argument("--label", default="head", help="what the figures belong to, e.g. the commit (stored in the JSON)")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--blank", type=float, default=0.93, help="share of blank 32-px tiles (Megapixel-MNIST: 0.93; 0: dense images)")
    ap.add_argument("--parent", help="JSON this tool wrote on the parent commit: the baselines")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.repo))
    from ips_amd import quant, synth
    from ips_amd.architecture import IPSNet
    from ips_amd.ragged_image import RaggedImages

    dev = torch.device("cuda:0")
    parent = json.load(open(args.parent))["workloads"] if args.parent else {}
    result = {"label": args.label, "repeats": args.repeats, "blank": args.blank, "device": torch.cuda.get_device_name(0), "workloads": {}}
    for name in args.workloads.split(","):
        kind, over, B, (lo, hi), p, s = WORKLOADS[name]
        rnd = random.Random(2000)
        sizes = [(rnd.randint(lo, hi) // 4 * 4, rnd.randint(lo, hi) // 4 * 4) for _ in range(B)]
        grids = [((h - p) // s + 1) * ((w - p) // s + 1) for h, w in sizes]
        conf = (synth.mnist_conf if kind == "mnist" else synth.traffic_conf)(N=max(grids), **over)
        net = synth.fill_weights(IPSNet(dev, conf), 7).to(dev).eval()
        c = conf.n_chan_in
        table = quant.patch_table(c)
        net.set_patch_table(table)
        g = torch.Generator(device=dev).manual_seed(21)
        bytes_ = []
        for h, w in sizes:      # Megapixel-MNIST's sparsity on the 32-px grid: most tiles all-zero bytes, the others any byte
            keep = (torch.rand((1, h // 32 + 1, w // 32 + 1), device=dev, generator=g) >= args.blank)
            keep = keep.repeat_interleave(32, 1).repeat_interleave(32, 2)[:, :h, :w]
            bytes_.append((torch.randint(0, 256, (c, h, w), device=dev, generator=g, dtype=torch.uint8) * keep).contiguous())
        floats = [quant.dequant(im, table.to(dev)).contiguous() for im in bytes_]
        patch, stride = (p, p), (s, s)
        packed_f32 = RaggedImages.from_list(floats)
        host_f32 = packed_f32.to("cpu").pin_memory()
        packed_u8 = RaggedImages.from_list(bytes_)
        host_u8 = packed_u8.to("cpu").pin_memory()
        legs = {"solo_u8": lambda: [net.ips_image(im[None], patch, stride) for im in bytes_],
                "ragged_f32": lambda: net.ips_image_ragged(packed_f32, patch, stride),
                "host_ragged_f32": lambda: net.ips_image_ragged(host_f32, patch, stride)}
        try:
            net.ips_image_ragged(packed_u8, patch, stride)
            legs["ragged_u8"] = lambda: net.ips_image_ragged(packed_u8, patch, stride)
            legs["host_ragged_u8"] = lambda: net.ips_image_ragged(host_u8, patch, stride)
        except TypeError:           # a tree whose ragged call refuses bytes: the baselines only
            pass
        times = {k: [] for k in legs}
        peaks = {}
        for rep in range(args.warmup + args.repeats):
            for k, fn in legs.items():
                torch.manual_seed(rep)
                net._reset_last()          # (a net keeps the embeddings of its last call for last_mem_emb: a leg's peak is its own)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats(dev)
                base = torch.cuda.memory_allocated(dev)
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                peaks[k] = max(peaks.get(k, 0), torch.cuda.max_memory_allocated(dev) - base)
                del out
                if rep >= args.warmup:
                    times[k].append(dt)
        rec = {"images": B, "sizes": sizes, "patches": grids, "total_patches": sum(grids), "patch": p, "stride": s, "M": conf.M, "I": conf.I,
               "input_bytes_u8": sum(im.numel() for im in bytes_), "input_bytes_f32": sum(im.numel() * 4 for im in bytes_),
               "patch_tensor_bytes_u8": sum(grids) * c * p * p, "legs": {}}
        for k, ts in times.items():
            rec["legs"][k] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "spread_ms": max(ts) - min(ts),
                              "patches_per_s": sum(grids) / (statistics.median(ts) * 1e-3), "peak_bytes_above_input": int(peaks[k])}
        if name in parent:
            rec["parent"] = parent[name]["legs"]
            for head, base_leg in (("ragged_u8", "solo_u8"), ("ragged_u8", "ragged_f32"), ("host_ragged_u8", "host_ragged_f32")):
                if head in rec["legs"] and base_leg in rec["parent"]:
                    b = rec["parent"][base_leg]
                    rec["legs"][head]["over_parent_" + base_leg] = rec["legs"][head]["median_ms"] / b["median_ms"]
        for head, twin in (("ragged_u8", "ragged_f32"), ("host_ragged_u8", "host_ragged_f32")):
            if head in rec["legs"]:
                t = (rec.get("parent") or rec["legs"]).get(twin, rec["legs"][twin])
                rec["legs"][head]["u8_slower_than_f32_beyond_spread"] = bool(
                    rec["legs"][head]["median_ms"] > t["median_ms"] + rec["legs"][head]["spread_ms"])
        result["workloads"][name] = rec
        print(name, json.dumps(rec["legs"]), flush=True)
        del net, bytes_, floats, legs, packed_f32, packed_u8, host_f32, host_u8
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
