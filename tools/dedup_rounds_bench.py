#!/usr/bin/env python
"""Time the counted launch behind the blank scan (ipsx_trunk_encode_parts_dedup: scan, compaction, eight-patch launch, pair
launch) on lists with a given number of surviving entries, under the switch's three modes: 0 the rule (trunk_split_n8), 1
eight-patch workgroups only, 2 pair workgroups only.  A count is `q:r` = q whole rounds (8 patches per compute unit) + r, or a
plain number; a fifth of each list besides are blank entries.

    python tools/dedup_rounds_bench.py [q:r ...]
"""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ips_amd import hip, synth   # noqa: E402


def main():
    dev = torch.device("cuda:0")
    R = 8 * hip.device_geometry(dev).cus
    args = sys.argv[1:] or ["%d:%d" % (q, r) for q in (0, 1, 2, 3, 5, 8) for r in (R // 4, R // 2, 3 * R // 4)]
    counts = [int(a.split(":")[0]) * R + int(a.split(":")[1]) if ":" in a else int(a) for a in args]
    conf, _ = synth.bench_workload("mnist")
    from ips_amd.architecture.ips_net import IPSNet
    net = synth.fill_weights(IPSNet(dev, conf), 7).to(dev).eval()
    plan = hip.EncoderPlan(net.encoder, True)
    mode = hip.lib().ipsx_dbg_fused_trunk_pair
    mode.restype, mode.argtypes = None, [C.c_int]
    full, blank = 4096, 64
    x = torch.rand((full + blank, 1, 32, 32), device=dev) + 1e-3
    x[full:] = 0
    g = np.random.default_rng(1)
    for arg, s in zip(args, counts):
        numbers = np.concatenate([g.integers(0, full, s), full + g.integers(0, blank, s // 5 + 8)])
        g.shuffle(numbers)
        every = torch.as_tensor(numbers.astype(np.int32)).to(dev)
        n = every.numel()
        done = torch.zeros((1,), dtype=torch.int32, device=dev)
        out = torch.empty((n, 128), device=dev)
        line = "%-8s %6d survivors of %6d" % (arg, s, n)
        try:
            for m, name in ((1, "eight only"), (0, "rule"), (2, "pairs only")):
                mode(m)
                for _ in range(3):
                    plan.encode_source(hip.PatchSource(x), index=every, parts=([n], done), dedup=True, out=out)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(20):
                    plan.encode_source(hip.PatchSource(x), index=every, parts=([n], done), dedup=True, out=out)
                e1.record()
                torch.cuda.synchronize()
                line += "   %s %.3f ms" % (name, e0.elapsed_time(e1) / 20)
        finally:
            mode(0)
        assert int(plan.n_encoded.item()) == s
        print(line, flush=True)


if __name__ == "__main__":
    main()
