#!/usr/bin/env python
"""ips_image() on resident whole images against a row stream fed the same images in bands of pixel rows:
whole synced calls, warmed, the legs alternated in one process.  The bands are slices of the device-resident images, so the
timing is that of the stream itself, not of a reader.

    ips_image                 net.ips_image(images)                                  - the baseline
    rows_whole / _8sh / _sh   ips_stream(patch, stride).feed_rows(band), bands of H / 8 sh / sh pixel rows
    patches_8sh / _sh         ips_stream().feed(hip.patchify(window)) at the same band heights: what a caller had to do
                              before - unfold every band and carry the rows a straddling patch row needs by hand

The ``ips_image`` leg uses only what exists without row streams, so the same file run on the parent commit gives the baseline:

    python tools/stream_rows_bench.py --repo <parent checkout> --label parent --baseline-only --out parent.json
    python tools/stream_rows_bench.py --parent parent.json --out profiles/ips_stream_rows.json

Nothing is accepted or refused here: small bands are launch-bound, and the figures say what that costs.  Peak
memory is the allocator's peak above what is allocated when the leg starts (the resident images)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

SHAPES = {
    # name: (overrides of the mnist configuration, image batch, patch, stride) - the ips_image shapes of profiles/patch_view.json
    "mnist_16x1600_s32": (dict(N=2500), (16, 1, 1600, 1600), (32, 32), (32, 32)),
    "mnist_16x1600_s16": (dict(N=9801), (16, 1, 1600, 1600), (32, 32), (16, 16)),
    "mnist50_16x1500_s25": (dict(N=3481, patch=50), (16, 1, 1500, 1500), (50, 50), (25, 25)),
}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout to import ips_amd from")
    ap.add_argument("--label", default="head", help="what the figures belong to, e.g. the commit (stored in the JSON)")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--baseline-only", action="store_true", help="time the ips_image() leg alone (what a checkout without row streams runs)")
    ap.add_argument("--parent", help="JSON this tool wrote on the parent commit: the ips_image() baseline")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.repo))
    from ips_amd import hip, synth
    from ips_amd.architecture import IPSNet

    dev = torch.device("cuda:0")
    parent = json.load(open(args.parent))["shapes"] if args.parent else {}
    result = {"label": args.label, "repeats": args.repeats, "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name in args.shapes.split(","):
        over, ishape, patch, stride = SHAPES[name]
        conf = synth.mnist_conf(shuffle=False, **over)
        # one net per leg (the same weights): a layer-by-layer trunk keeps its workspace with the net and gives it back after
        # several small requests in a row - alternated on ONE net, a leg of small bands would make the next whole-image leg
        # allocate gigabytes again and report them as its own peak
        nets = {}

        def net_of(leg):
            if leg not in nets:
                nets[leg] = synth.fill_weights(IPSNet(dev, conf), 7).to(dev).eval()
            return nets[leg]

        images = torch.randn(ishape, generator=torch.Generator().manual_seed(1)).to(dev)
        H, (ph, sh) = ishape[2], (patch[0], stride[0])

        def rows(leg, step):
            s = net_of(leg).ips_stream(patch_size=patch, patch_stride=stride)
            for lo in range(0, H, step):
                s.feed_rows(images[:, :, lo:lo + step])
            return s.finish()

        def patches(leg, step):
            """the caller's side of the same bands before row streams: keep the rows from the next patch row on, unfold the
            complete patch rows of every band, feed the patch tensor"""
            s = net_of(leg).ips_stream()
            carry = None
            for lo in range(0, H, step):
                band = images[:, :, lo:lo + step]
                window = band if carry is None else torch.cat((carry, band), 2)
                n = window.shape[2]
                ny = (n - ph) // sh + 1 if n >= ph else 0
                if ny:
                    s.feed(hip.patchify(window[:, :, :(ny - 1) * sh + ph], patch, stride))
                carry = window[:, :, ny * sh:]         # (sh <= ph in every shape here: never beyond the window)
            return s.finish()

        legs = {"ips_image": lambda: net_of("ips_image").ips_image(images, patch, stride)}
        if not args.baseline_only:
            legs.update({"rows_whole": lambda: rows("rows_whole", H), "rows_8sh": lambda: rows("rows_8sh", 8 * sh),
                         "rows_sh": lambda: rows("rows_sh", sh), "patches_8sh": lambda: patches("patches_8sh", 8 * sh),
                         "patches_sh": lambda: patches("patches_sh", sh)})
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
        ny, nx = (H - ph) // sh + 1, (ishape[3] - patch[1]) // stride[1] + 1
        rec = {"images": ishape[0], "patches_per_image": ny * nx, "M": conf.M, "I": conf.I, "image_bytes": images.numel() * 4,
               "patch_tensor_bytes": ishape[0] * ny * nx * ishape[1] * patch[0] * patch[1] * 4,
               "band_rows": {"rows_whole": H, "rows_8sh": 8 * sh, "rows_sh": sh, "patches_8sh": 8 * sh, "patches_sh": sh}, "legs": {}}
        for k, ts in times.items():
            rec["legs"][k] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "spread_ms": max(ts) - min(ts),
                              "peak_bytes_above_input": int(peaks[k])}
        if name in parent:
            p = parent[name]["legs"]["ips_image"]
            rec["parent_ips_image"] = p
            for k in rec["legs"]:
                rec["legs"][k]["over_parent_ips_image"] = rec["legs"][k]["median_ms"] / p["median_ms"]
        result["shapes"][name] = rec
        print(name, json.dumps(rec["legs"]), flush=True)
        nets.clear()
        del images, legs
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
