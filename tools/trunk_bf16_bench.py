#!/usr/bin/env python
"""The bf16 trunk ALONE (no selection loop beside it): patches/s of plan.encode at whole rounds of the chip (a round = 16
patches per unit: two workgroups of eight) and at the headline's part sizes.  Per size: 3 warm-up calls, then five
batches of 10 calls between two syncs; the median batch with the fastest and the slowest beside it.
    python tools/trunk_bf16_bench.py"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["IPSX_PRECISION"] = "bf16"
from ips_amd import hip, synth
from ips_amd.architecture import IPSNet

dev = torch.device("cuda:0")
conf = synth.mnist_conf(N=2500)
net = synth.fill_weights(IPSNet(dev, conf), 7).to(dev).eval()
x = synth.make_patches(conf, 20, seed=21).reshape(-1, 1, 32, 32).contiguous().to(dev)
plan = hip.EncoderPlan(net.encoder, True)
units = hip.device_geometry(dev).cus
for _ in range(60):                     # clocks up before the first size
    plan.encode(x[:8 * units * 10])
for n in (8 * units * 10, 16 * units * 5, 21504, 11264, 6144, 40000):
    xs = x[:n]
    for _ in range(3):
        plan.encode(xs)
    torch.cuda.synchronize()
    dts = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(10):
            plan.encode(xs)
        torch.cuda.synchronize()
        dts.append((time.perf_counter() - t0) / 10)
    dts.sort()
    print("%6d patches   %6.1f us  %5.2f M patches/s   (fastest %6.1f us, slowest %6.1f us)"
          % (n, dts[2] * 1e6, n / dts[2] / 1e6, dts[0] * 1e6, dts[-1] * 1e6))
