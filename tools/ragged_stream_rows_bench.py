#!/usr/bin/env python
"""Row bands of whole images of different sizes (IPSNet.ips_ragged_stream(patch_size=, patch_stride=)) against
what a caller has without it.  The protocol of tools/image_ragged_bench.py: whole synced calls, 20 repeats after 3, the legs
alternated in one process, median with max - min.  16 images of 1,100 - 1,700 pixels a side (sides from a fixed seed, rounded
to multiples of 4), at Megapixel-MNIST's sparsity (--blank 0.93) or dense (--blank 0); device-resident, or host-resident in
pinned memory (--host).

The parent's legs use only what exists without the ragged row stream, so the same file run on a build of the parent commit
gives the baseline - the baseline is never the code under test:

    python tools/ragged_stream_rows_bench.py --repo <parent checkout> --label parent --out parent.json
    python tools/ragged_stream_rows_bench.py --parent parent.json --out profiles/ips_ragged_stream_rows.json

Legs: ``solo_rows_8sh`` / ``solo_rows_sh`` (B solo ``ips_stream(patch_size, patch_stride)`` row streams, image after image, fed
``band[None]`` in bands of 8 * sh / sh rows), ``image_ragged`` (``ips_image_ragged`` on the resident images: every pixel on
the device) and, where the tree has it, ``stream_whole`` / ``stream_8sh`` / ``stream_sh`` (the ragged row stream fed whole images,
bands of 8 * sh rows, bands of sh rows).  Per leg: time, feeds, time per feed, and the allocator's peak above what is
allocated when the leg starts (device-resident: the images; host-resident: nothing of the input).  Nothing is accepted or
refused here."""
import argparse
import inspect
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
    ap.add_argument("--host", action="store_true", help="the images lie in pinned host memory")
    ap.add_argument("--legs", default="", help="only these legs (comma separated)")
    ap.add_argument("--parent", help="JSON this tool wrote on a build of the parent commit: the baseline")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.repo))
    from ips_amd import synth
    from ips_amd.architecture import IPSNet

    dev = torch.device("cuda:0")
    parent = json.load(open(args.parent))["workloads"] if args.parent else {}
    result = {"label": args.label, "repeats": args.repeats, "blank": args.blank, "resident": "host (pinned)" if args.host else "device",
              "device": torch.cuda.get_device_name(0), "workloads": {}}
    has_rows = "patch_size" in inspect.signature(IPSNet.ips_ragged_stream).parameters
    for name in args.workloads.split(","):
        kind, over, B, (lo, hi), p, s = WORKLOADS[name]
        rnd = random.Random(2000)
        sizes = [(rnd.randint(lo, hi) // 4 * 4, rnd.randint(lo, hi) // 4 * 4) for _ in range(B)]
        grids = [((h - p) // s + 1) * ((w - p) // s + 1) for h, w in sizes]
        conf = (synth.mnist_conf if kind == "mnist" else synth.traffic_conf)(N=max(grids), **over)
        net = synth.fill_weights(IPSNet(dev, conf), 7).to(dev).eval()
        net.shuffle = False
        g = torch.Generator(device=dev).manual_seed(21)
        c = conf.n_chan_in
        images = []
        for h, w in sizes:      # Megapixel-MNIST's sparsity on the 32-px grid: most tiles blank, the others U[0, 1)
            keep = (torch.rand((1, h // 32 + 1, w // 32 + 1), device=dev, generator=g) >= args.blank).float()
            keep = keep.repeat_interleave(32, 1).repeat_interleave(32, 2)[:, :h, :w]
            im = (torch.rand((c, h, w), device=dev, generator=g) * keep).contiguous()
            images.append(im.cpu().pin_memory() if args.host else im)
        patch, stride = (p, p), (s, s)
        feeds = {}

        def solo_rows(rows):
            def leg():
                out, n = [], 0
                for im in images:
                    st = net.ips_stream(patch_size=patch, patch_stride=stride)
                    for y in range(0, im.shape[1], rows):
                        st.feed_rows(im[None, :, y:y + rows])
                        n += 1
                    out.append(st.finish())
                feeds["solo_rows_" + ("8sh" if rows == 8 * s else "sh")] = n
                return out
            return leg

        def stream(rows, key):
            def leg():
                st = net.ips_ragged_stream(patch_size=patch, patch_stride=stride)
                if rows is None:
                    st.feed_rows(images)
                    feeds[key] = 1
                else:
                    st.feed_rows_all(images, rows)
                    feeds[key] = -(-max(h for h, _ in sizes) // rows)
                return st.finish()
            return leg

        legs = {"solo_rows_8sh": solo_rows(8 * s), "solo_rows_sh": solo_rows(s)}
        if hasattr(net, "ips_image_ragged"):
            legs["image_ragged"] = lambda: net.ips_image_ragged(images, patch, stride)
            feeds["image_ragged"] = 1
        if has_rows:
            legs.update(stream_whole=stream(None, "stream_whole"), stream_8sh=stream(8 * s, "stream_8sh"), stream_sh=stream(s, "stream_sh"))
        if args.legs:
            legs = {k: v for k, v in legs.items() if k in args.legs.split(",")}
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
            med = statistics.median(ts)
            rec["legs"][k] = {"median_ms": med, "min_ms": min(ts), "max_ms": max(ts), "spread_ms": max(ts) - min(ts), "feeds": feeds[k],
                              "ms_per_feed": med / feeds[k], "patches_per_s": sum(grids) / (med * 1e-3),
                              "peak_bytes_above_resident": int(peaks[k])}
        if name in parent:
            rec["parent"] = parent[name]["legs"]
            for k, base_leg in (("stream_8sh", "solo_rows_8sh"), ("stream_sh", "solo_rows_sh"), ("stream_whole", "image_ragged")):
                if k in rec["legs"] and base_leg in rec["parent"]:
                    rec["legs"][k]["over_parent_" + base_leg] = rec["legs"][k]["median_ms"] / rec["parent"][base_leg]["median_ms"]
                    if k != "stream_whole":    # one feed of the stream against ONE solo row-stream feed of the parent
                        rec["legs"][k]["ms_per_feed_over_parent_solo_feed"] = rec["legs"][k]["ms_per_feed"] / rec["parent"][base_leg]["ms_per_feed"]
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
