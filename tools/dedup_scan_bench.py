#!/usr/bin/env python
"""The float32 blank scan of the counted, deduped launch (blank_scan_parts_kernel, csrc/dedup.hip) against a plain read of the
same bytes: the headline's patch tensor (16 x 2,500 patches of 1x32x32 float32, 164 MB, 93 % of the patches blank) and the
same tensor without a blank patch, where the scan reads one KiB per patch.

The two kinds of kernel are timed by the profiler, not by the host: run the launches under a kernel trace (no counters),

    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python tools/dedup_scan_bench.py run [--repeats 10]

and read the kernels' durations back:

    python tools/dedup_scan_bench.py summary DIR        -> one JSON line (medians in us, bytes / time, the ratio)

``run`` launches, `repeats` times each, alternating: the counted deduped encode of every patch in list order (scan, compaction,
the trunk's launches) on the headline's data and on the dense data, and two plain reads of the tensor - an int32 maximum and a
float32 sum, whichever torch reduction is faster counts.  The first KiB of every patch being a quarter of the bytes, the
dense scan's time is set against a quarter of the plain read's."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ips_amd import hip, synth                                    # noqa: E402
from ips_amd.architecture import IPSNet                           # noqa: E402

B, N = 16, 2500
MARK = 12345                                                      # elements of the marker fill between the legs of `run`


def run(repeats):
    dev = torch.device("cuda:0")
    conf = synth.mnist_conf(N=N, M=64, I=64)
    net = synth.fill_weights(IPSNet(dev, conf), 7).to(dev).eval()
    plan = hip.EncoderPlan(net.encoder, True)
    sparse = synth.make_patches(conf, B, seed=21).reshape(B * N, 1, 32, 32).to(dev)
    dense = synth.make_patches(conf, B, seed=21, blank_frac=0).reshape(B * N, 1, 32, 32).to(dev)
    every = torch.arange(B * N, dtype=torch.int32, device=dev)
    ends = [B * N]
    done = torch.zeros((1,), dtype=torch.int32, device=dev)
    marker = torch.empty((MARK,), device=dev)
    for k in range(repeats + 2):
        for x in (sparse, dense):                                 # (the trace keeps the order: sparse, dense, sparse, ...)
            done.zero_()
            plan.encode_source(hip.PatchSource(x), index=every, parts=(ends, done), dedup=True)
            marker.zero_()
            x.view(torch.int32).amax()
            x.sum()
            torch.cuda.synchronize()


def summary(path):
    f = glob.glob(path + "/**/*kernel_trace.csv", recursive=True)[0]
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    scans = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if "blank_scan_parts_kernel" in r["Kernel_Name"]]
    reads = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if "reduce_kernel" in r["Kernel_Name"]]
    scans = scans[4:]                                             # two warm-up rounds
    sparse, dense = scans[0::2], scans[1::2]
    # a reduction of 41 M elements is two launches: the long one reads the tensor
    reads = sorted(t for t in reads if t > 10.0)
    nbytes = B * N * 4096
    out = {"bytes": nbytes, "scan_sparse_us": statistics.median(sparse), "scan_dense_us": statistics.median(dense),
           "plain_read_us": reads[0] if reads else None, "plain_read_median_us": statistics.median(reads) if reads else None,
           "launches": {"sparse": len(sparse), "dense": len(dense), "plain reads": len(reads)}}
    out["scan_sparse_TBps"] = nbytes / out["scan_sparse_us"] / 1e6
    if reads:
        best = statistics.median(sorted(reads)[:max(1, len(reads) // 2)])       # the faster of the two reductions
        out["plain_read_us"] = best
        out["plain_read_TBps"] = nbytes / best / 1e6
        out["sparse_over_plain"] = out["scan_sparse_us"] / best
        out["dense_over_quarter_plain"] = out["scan_dense_us"] / (best / 4)
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["run", "summary"])
    ap.add_argument("dir", nargs="?")
    ap.add_argument("--repeats", type=int, default=10)
    a = ap.parse_args()
    if a.mode == "run":
        run(a.repeats)
    else:
        summary(a.dir)
