"""Shuffled ``ips()`` through a permutation index against the shuffled copy (``IPSX_SHUFFLE=index`` / ``copy``), in ONE
process, the modes alternating call by call: device-synchronised wall time of the whole call (median, quartiles) and the
peak of allocated device memory above the resident input, plus a ``shuffle=False`` control row per size (the plain path).

    python tools/shuffle_bench.py [--reps 30] [--out profiles/shuffle_bench.json] [--only NAME]
"""

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ips_amd import synth                     # noqa: E402
from ips_amd.architecture import IPSNet       # noqa: E402

SIZES = (
    # name, configuration, slides / images, input dtype, IPSX_PRECISION
    ("cam 1x65536x2048 fp32", lambda: synth.camelyon_conf(N=65536, M=256, I=256), 1, torch.float32, "fp32"),
    ("cam 1x65536x2048 f16 under bf16", lambda: synth.camelyon_conf(N=65536, M=256, I=256), 1, torch.float16, "bf16"),
    ("cam 16x65536x2048 fp32", lambda: synth.camelyon_conf(N=65536, M=256, I=256), 16, torch.float32, "fp32"),
    ("cam 1x38000x2048 fp32 M=I=5000", lambda: synth.camelyon_conf(N=38000, M=5000, I=5000), 1, torch.float32, "fp32"),
    ("mnist 16x2500x1x32x32 fp32", lambda: synth.mnist_conf(N=2500, M=64, I=64), 16, torch.float32, "fp32"),
)


def patches(conf, B, dtype, dev):
    g = torch.Generator(device=dev).manual_seed(21)
    if conf.is_image:
        p = conf.patch_size
        return torch.rand((B, conf.N, conf.n_chan_in, p[0], p[1]), generator=g, device=dev)
    x = torch.empty((B, conf.N, conf.n_chan_in), dtype=dtype, device=dev)
    for b in range(B):                                         # slide by slide: no second tensor of the input's size
        x[b] = torch.randn((conf.N, conf.n_chan_in), generator=g, device=dev).relu_().to(dtype)
    return x


def one_call(net, x, mode, dev):
    net.shuffle = mode != "plain"
    os.environ["IPSX_SHUFFLE"] = "copy" if mode == "copy" else "index"
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    t0 = time.perf_counter()
    net.ips(x)
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    return dt * 1e3, torch.cuda.max_memory_allocated(dev) - base


def quartiles(v):
    q = statistics.quantiles(v, n=4)
    return {"median_ms": round(statistics.median(v), 4), "q1_ms": round(q[0], 4), "q3_ms": round(q[2], 4), "min_ms": round(min(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "shuffle_bench.json"))
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for name, conf_fn, B, dtype, prec in SIZES:
        if args.only and args.only not in name:
            continue
        os.environ["IPSX_PRECISION"] = prec
        conf = conf_fn().clone(shuffle=True, shuffle_style="batch")
        net = synth.fill_weights(IPSNet(dev, conf), 7).to(dev).eval()
        x = patches(conf, B, dtype, dev)
        modes = ("copy", "index", "plain")
        for _ in range(args.warmup):
            for m in modes:
                one_call(net, x, m, dev)
        times, peaks, taken = {m: [] for m in modes}, {m: 0 for m in modes}, {}
        for _ in range(args.reps):
            for m in modes:                                    # alternating: drift of the device hits every mode alike
                before = net.selection.index_calls
                dt, peak = one_call(net, x, m, dev)
                times[m].append(dt)
                peaks[m] = max(peaks[m], peak)
                taken[m] = net.selection.index_calls > before
        nbytes = x.numel() * x.element_size()
        for m in modes:
            row = {"size": name, "mode": {"copy": "shuffle=True, IPSX_SHUFFLE=copy", "index": "shuffle=True, IPSX_SHUFFLE=index",
                                          "plain": "shuffle=False"}[m],
                   "reads_through_index": taken[m], "input_bytes": nbytes, "peak_bytes_above_input": peaks[m],
                   "patches_per_call": B * conf.N, "reps": args.reps}
            row.update(quartiles(times[m]))
            rows.append(row)
            print(json.dumps(row), flush=True)
        del x, net
        torch.cuda.empty_cache()
    os.environ.pop("IPSX_SHUFFLE", None)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"tool": "tools/shuffle_bench.py", "device": torch.cuda.get_device_name(dev), "rows": rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
