#!/usr/bin/env python
"""ips_image_ragged() on whole images of different sizes against what a caller has without it: the loop of solo
ips_image() calls, and ips_ragged() on materialised patch tensors.  The protocol of tools/ragged_bench.py: whole synced calls,
20 repeats after 3, the legs alternated in one process, median with max - min.  The images are device-resident, drawn on the
device from a fixed seed, their sides from a fixed seed on the host (rounded to multiples of 4 pixels).

The ``solo`` leg uses only what exists without ``ips_image_ragged``, so the same file run on the parent commit gives the
baseline - the baseline is never the code under test:

    python tools/image_ragged_bench.py --repo <parent checkout> --label parent --out parent.json
    python tools/image_ragged_bench.py --parent parent.json --out profiles/ips_image_ragged.json

Legs on the head: ``solo`` (the loop of ips_image(image[None]) calls), ``patches`` (hip.patchify per image, then
ips_ragged(list): the materialised route, its patch tensors made inside the timed call) and ``image_ragged``
(ips_image_ragged on the packed RaggedImages, the environment as it is: the default), and, where the tree has the exact
blank-patch dedup on the ragged view, ``image_ragged_plain`` (the same call under IPSX_DEDUP_BLANK=0: plain launches).  With
``--parent`` the parent's ``solo`` and ``image_ragged`` legs are the baselines (profiles/ips_image_ragged_dedup.json).  Nothing
is accepted or refused here.  Peak memory is the allocator's peak above what is allocated when the leg starts (the resident input: the images as a list and as one packed buffer)."""
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
    ap.add_argument("--blank", type=float, default=0.93, help="share of blank 32-px tiles (Megapixel-MNIST: 0.93; 0: dense images - the solo "
                    "loop's counted launch skips blank patches on the fused trunk, the packed pass encodes every patch)")
    ap.add_argument("--parent", help="JSON this tool wrote on the parent commit: the baseline")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.repo))
    from ips_amd import hip, synth
    from ips_amd.architecture import IPSNet

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
        g = torch.Generator(device=dev).manual_seed(21)
        c = conf.n_chan_in
        images = []
        for h, w in sizes:      # Megapixel-MNIST's sparsity on the 32-px grid: most tiles blank, the others U[0, 1)
            keep = (torch.rand((1, h // 32 + 1, w // 32 + 1), device=dev, generator=g) >= args.blank).float()
            keep = keep.repeat_interleave(32, 1).repeat_interleave(32, 2)[:, :h, :w]
            images.append((torch.rand((c, h, w), device=dev, generator=g) * keep).contiguous())
        patch, stride = (p, p), (s, s)

        def solo():
            return [net.ips_image(im[None], patch, stride) for im in images]

        legs = {"solo": solo}
        if hasattr(net, "ips_image_ragged"):
            from ips_amd.ragged_image import RaggedImages
            packed = RaggedImages.from_list(images)
            legs["patches"] = lambda: net.ips_ragged([hip.patchify(im[None], patch, stride)[0] for im in images])
            legs["image_ragged"] = lambda: net.ips_image_ragged(packed, patch, stride)
            from ips_amd import ragged_image
            if hasattr(ragged_image, "ragged_dedup"):
                def under(key, value):
                    def leg():
                        os.environ[key] = value
                        try:
                            return net.ips_image_ragged(packed, patch, stride)
                        finally:
                            del os.environ[key]
                    return leg
                legs["image_ragged_plain"] = under("IPSX_DEDUP_BLANK", "0")
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
               "input_bytes": sum(im.numel() * 4 for im in images), "patch_tensor_bytes": sum(grids) * c * p * p * 4, "legs": {}}
        for k, ts in times.items():
            rec["legs"][k] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "spread_ms": max(ts) - min(ts),
                              "patches_per_s": sum(grids) / (statistics.median(ts) * 1e-3), "peak_bytes_above_input": int(peaks[k])}
        if name in parent:
            ps = parent[name]["legs"]["solo"]
            rec["parent_solo"] = ps
            for k in rec["legs"]:
                rec["legs"][k]["over_parent_solo"] = rec["legs"][k]["median_ms"] / ps["median_ms"]
            pr = parent[name]["legs"].get("image_ragged")
            if pr is not None and "image_ragged" in rec["legs"]:
                rec["parent_image_ragged"] = pr
                for k in rec["legs"]:
                    if k.startswith("image_ragged"):
                        rec["legs"][k]["within_parent_image_ragged_spread"] = bool(rec["legs"][k]["median_ms"] <= pr["median_ms"] + pr["spread_ms"])
                        rec["legs"][k]["within_parent_solo_spread"] = bool(rec["legs"][k]["median_ms"] <= ps["median_ms"] + ps["spread_ms"])
            if "image_ragged" in rec["legs"]:
                rec["image_ragged_within_parent_spread"] = bool(rec["legs"]["image_ragged"]["median_ms"] <= ps["median_ms"] + ps["spread_ms"])
                rec["image_ragged_peak_below_patches"] = bool(rec["legs"]["image_ragged"]["peak_bytes_above_input"] <
                                                              rec["legs"]["patches"]["peak_bytes_above_input"])
        result["workloads"][name] = rec
        print(name, json.dumps(rec["legs"]), flush=True)
        del net, images, legs
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
