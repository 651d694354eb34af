#!/usr/bin/env python
"""ips() on the whole input against ips_stream() fed in pieces: whole synced calls, warmed, the legs alternated
in one process.  The pieces are slices of a device-resident tensor - one chunk, eight chunks, N / 4, N -, so the timing is
that of the stream itself, not of a source.

The ``ips`` leg uses only what exists without the stream, so the same file run on the parent commit gives the baseline:

    python tools/stream_bench.py --repo <parent checkout> --label parent --out parent.json
    python tools/stream_bench.py --parent parent.json --out profiles/ips_stream.json

Nothing is accepted or refused here: the loop of a stream is fully exposed (no encoder runs beside it), and the figures say
what that costs.  Peak memory is the allocator's peak above what is allocated when the leg starts (the resident input)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

WORKLOADS = {
    # name: (configuration, images / slides per call)
    "mnist_16x2500": ("mnist", 16),                  # the headline: 16 images of 2,500 32-px patches, M = I = 64
    "camelyon_1x65536": ("camelyon", 1),             # one slide of 65,536 x 2,048 features, M = I = 256
}


def launches_per_feed(net, x, contiguous):
    """Counted from ips_amd/stream.py: the encoder (the fused trunk: 1, a layer-by-layer trunk: its layers, the projector:
    moments + GEMM = 2; once per image when the piece is a slice along the patch axis of several images), the logits, the
    piece's global ids, the loop when a chunk is complete, the commit - and a copy of the held logits whenever a piece is
    larger than any before it (the logits tables grow)."""
    B = x.shape[0]
    per = 1 if contiguous or B == 1 else B
    if not net.is_image:
        enc = 2 * per
    elif net.selection.plan().fused(tuple(x.shape[2:])):
        enc = per
    else:
        enc = "%d x the launches of the layer-by-layer trunk" % per
    return {"encoder": enc, "logits": 1, "ids": 1, "loop_if_a_chunk_completes": 1, "commit": 1,
            "copy_of_the_held_logits_when_a_larger_piece_than_any_before_arrives": 1}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout to import ips_amd from")
    ap.add_argument("--label", default="head", help="what the figures belong to, e.g. the commit (stored in the JSON)")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--ips-only", action="store_true", help="time the ips() leg alone (what a checkout without the stream runs)")
    ap.add_argument("--parent", help="JSON this tool wrote on the parent commit: the ips() baseline")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.repo))
    from ips_amd import synth
    from ips_amd.architecture import IPSNet

    dev = torch.device("cuda:0")
    parent = json.load(open(args.parent))["workloads"] if args.parent else {}
    result = {"label": args.label, "repeats": args.repeats, "device": torch.cuda.get_device_name(0), "workloads": {}}
    for name in args.workloads.split(","):
        kind, B = WORKLOADS[name]
        conf = (synth.mnist_conf if kind == "mnist" else synth.camelyon_conf)(shuffle=False)
        net = synth.fill_weights(IPSNet(dev, conf), 7).to(dev).eval()
        x = synth.make_patches(conf, B, seed=1).to(dev)
        N, I = x.shape[1], conf.I

        def stream(step):
            s = net.ips_stream()
            for lo in range(0, N, step):
                s.feed(x[:, lo:lo + step])
            return s.finish()

        legs = {"ips": lambda: net.ips(x)}
        streams = hasattr(net, "ips_stream") and not args.ips_only
        if streams:
            for label, step in (("stream_1_chunk", I), ("stream_8_chunks", 8 * I), ("stream_quarter", -(-N // 4)), ("stream_whole", N)):
                legs[label] = (lambda step=step: stream(step))
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
        rec = {"images": B, "patches_per_image": N, "M": conf.M, "I": I, "input_bytes": x.numel() * x.element_size(), "legs": {}}
        for k, ts in times.items():
            rec["legs"][k] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "spread_ms": max(ts) - min(ts),
                              "peak_bytes_above_input": int(peaks[k])}
        if streams:
            rec["piece_rows"] = {"stream_1_chunk": I, "stream_8_chunks": 8 * I, "stream_quarter": -(-N // 4), "stream_whole": N}
            rec["launches_per_feed"] = {"slice": launches_per_feed(net, x, False), "contiguous_piece": launches_per_feed(net, x, True)}
        if name in parent:
            p = parent[name]["legs"]["ips"]
            rec["parent_ips"] = p
            for k in rec["legs"]:
                rec["legs"][k]["over_parent_ips"] = rec["legs"][k]["median_ms"] / p["median_ms"]
        result["workloads"][name] = rec
        print(name, json.dumps(rec["legs"]), flush=True)
        del net, x, legs
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
