"""``shuffle: True`` on the routes that make a call fast: the lone slide through the library's one call, one
image on the fused trunk stream, layer-by-layer trunks in one piece.  The scheme of tools/shuffle_bench.py - ONE process,
``IPSX_SHUFFLE=copy``, ``index`` and ``shuffle=False`` alternating call by call, whole device-synchronised calls, median,
quartiles and minimum, the peak of allocated device memory above the resident input - on the shapes of those routes.
Only ``net.ips`` and the environment are used, so the same file runs unchanged on a checkout of an earlier commit: that
is how profiles/shuffle_routes_parent*.json were taken.

    python tools/shuffle_routes_bench.py [--reps 30] [--out profiles/shuffle_routes.json] [--only NAME] [--native-order-ab]

``--native-order-ab`` adds a fourth mode to the alternation: ``index`` with ``IPSX_NATIVE_ORDER=0`` (a feature call through
the index enqueues its launches one by one) beside ``index`` with ``IPSX_NATIVE_ORDER=1`` (the library's ordered one call).
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
    # name, configuration, slides / images
    ("cam 1x65536x2048", lambda: synth.camelyon_conf(N=65536, M=256, I=256), 1),
    ("cam 1x38000x2048 M=I=5000", lambda: synth.camelyon_conf(N=38000, M=5000, I=5000), 1),
    ("cam 16x65536x2048", lambda: synth.camelyon_conf(N=65536, M=256, I=256), 16),
    ("mnist 1x2500x1x32x32 M=I=64", lambda: synth.mnist_conf(N=2500, M=64, I=64), 1),
    ("mnist50 16x900x1x50x50 M=I=100", lambda: synth.mnist_conf(N=900, M=100, I=100, patch=50), 16),
    ("traffic 16x192x3x100x100", lambda: synth.traffic_conf(N=192), 16),
)


AB_MODES = {}       # --native-order-ab: IPSX_NATIVE_ORDER per mode (without the flag the environment is left as it is)


def patches(conf, B, dev):
    g = torch.Generator(device=dev).manual_seed(21)
    if conf.is_image:
        p = conf.patch_size
        return torch.rand((B, conf.N, conf.n_chan_in, p[0], p[1]), generator=g, device=dev)
    x = torch.empty((B, conf.N, conf.n_chan_in), dtype=torch.float32, device=dev)
    for b in range(B):                                         # slide by slide: no second tensor of the input's size
        x[b] = torch.randn((conf.N, conf.n_chan_in), generator=g, device=dev).relu_()
    return x


def one_call(net, x, mode, dev):
    net.shuffle = mode != "plain"
    os.environ["IPSX_SHUFFLE"] = "copy" if mode == "copy" else "index"
    if mode in AB_MODES:
        os.environ["IPSX_NATIVE_ORDER"] = AB_MODES[mode]
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    t0 = time.perf_counter()
    net.ips(x)
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    if mode in AB_MODES:
        os.environ.pop("IPSX_NATIVE_ORDER", None)
    return dt * 1e3, torch.cuda.max_memory_allocated(dev) - base


def quartiles(v):
    q = statistics.quantiles(v, n=4)
    return {"median_ms": round(statistics.median(v), 4), "q1_ms": round(q[0], 4), "q3_ms": round(q[2], 4), "min_ms": round(min(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "shuffle_routes.json"))
    ap.add_argument("--only", default=None)
    ap.add_argument("--native-order-ab", action="store_true")
    args = ap.parse_args()
    if args.native_order_ab:
        AB_MODES.update({"index": "1", "index one by one": "0"})
    dev = torch.device("cuda:0")
    rows = []
    for name, conf_fn, B in SIZES:
        if args.only and args.only not in name:
            continue
        conf = conf_fn().clone(shuffle=True, shuffle_style="batch")
        net = synth.fill_weights(IPSNet(dev, conf), 7).to(dev).eval()
        x = patches(conf, B, dev)
        modes = ("copy", "index", "index one by one", "plain") if args.native_order_ab else ("copy", "index", "plain")
        for _ in range(args.warmup):
            for m in modes:
                one_call(net, x, m, dev)
        times, peaks, taken, native = {m: [] for m in modes}, {m: 0 for m in modes}, {}, {}
        for _ in range(args.reps):
            for m in modes:                                    # alternating: drift of the device hits every mode alike
                sel = net.selection
                before = (sel.index_calls, getattr(sel, "native_calls", None))      # (an earlier commit does not count them)
                dt, peak = one_call(net, x, m, dev)
                times[m].append(dt)
                peaks[m] = max(peaks[m], peak)
                taken[m] = sel.index_calls > before[0]
                native[m] = None if before[1] is None else sel.native_calls > before[1]
        nbytes = x.numel() * x.element_size()
        for m in modes:
            row = {"size": name, "mode": {"copy": "shuffle=True, IPSX_SHUFFLE=copy", "index": "shuffle=True, IPSX_SHUFFLE=index",
                                          "index one by one": "shuffle=True, IPSX_SHUFFLE=index, IPSX_NATIVE_ORDER=0",
                                          "plain": "shuffle=False"}[m] + (", IPSX_NATIVE_ORDER=1" if args.native_order_ab and m == "index" else ""),
                   "reads_through_index": taken[m], "one_library_call": native[m], "input_bytes": nbytes, "peak_bytes_above_input": peaks[m],
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
            json.dump({"tool": "tools/shuffle_routes_bench.py", "device": torch.cuda.get_device_name(dev), "rows": rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
