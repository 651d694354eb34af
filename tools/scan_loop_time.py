#!/usr/bin/env python
"""Microseconds per iteration of scan_mnist_kernel's loop ALONE (8 heads x 4 tokens, M = I = 64, 16 images; HIP events around
20 launches after warm-up, the variants alternating three times), as profiles/scan_mnist_loop.json records it:
    plain       the instantiation without the logits prologue (hip.scan_range over the whole loop)
    prologue    the instantiation WITH it, launched with no part of its own (part_begin == part_end): the same iterations
                through the other instantiation's code - the prologue is outside the iterations, so the two must agree
    publish     the instantiation with the prologue AND the gate's parameter, publishing the iteration it reached per image at
                its end (gate_publish=): what the side stream's last loop launch of a gated call runs
    *_slope     (time of all iterations - time of the first half) / the other half: microseconds per iteration without what a
                launch costs once (kernel arguments, the empty prologue, the loop's own set-up); *_per_launch: that remainder
    python tools/scan_loop_time.py [out.json]"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ips_amd import hip  # noqa: E402

DEV = "cuda:0"
M = I = 64
H, T, D, B = 8, 4, 128, 16


def timed(fn, reps=20, warm=5):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


out = {}
g = torch.Generator().manual_seed(1)
vq = hip.fold_query((torch.randn((T, H * 16), generator=g) * 0.5).to(DEV), (torch.randn((H * 16, D), generator=g) * 0.3).to(DEV), H, 16, T)
for N in (2500, 10000):
    n_iter = -(-(N - M) // I)
    lg = (torch.randn((B, N, H * T), generator=g) * 3.0).to(DEV)
    mem = torch.empty((B, M), dtype=torch.int64, device=DEV)
    tie = torch.zeros((B,), dtype=torch.int32, device=DEV)
    parts = hip.LogitsParts([torch.zeros((B, N, D), device=DEV)])
    def plain(n):
        return lambda: hip.scan_range(lg, M, I, H, T, 0, n, mem, tie)

    def prologue(n):
        return lambda: parts.scan_range(lg, M, I, H, T, 0, n, mem, tie, 1, 1, None, vq)

    words = torch.zeros((B,), dtype=torch.int32, device=DEV)

    def publish(n):
        return lambda: parts.scan_range(lg, M, I, H, T, 0, n, mem, tie, 1, 1, None, vq, gate_publish=words)

    half = n_iter // 2
    variants = (("plain", plain), ("prologue", prologue), ("publish", publish))
    res = {k + suffix: [] for k, _ in variants for suffix in ("", "_slope", "_per_launch")}
    for _ in range(3):
        for k, fn in variants:
            whole, part = timed(fn(n_iter)), timed(fn(half))
            slope = (whole - part) / (n_iter - half)                 # us per iteration WITHOUT what a launch costs once
            res[k].append(round(whole / n_iter, 3))
            res[k + "_slope"].append(round(slope, 3))
            res[k + "_per_launch"].append(round(whole - slope * n_iter, 2))
    out["B%d_N%d_iters%d_us_per_iteration" % (B, N, n_iter)] = res
text = json.dumps(out, indent=1)
print(text)
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write(text + "\n")
