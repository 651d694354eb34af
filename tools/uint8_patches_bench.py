"""uint8 patch storage against float32, in ONE process, the two alternating call by call (the timing scheme of
tools/shuffle_bench.py): device-synchronised wall time of the whole call (median, quartiles, minimum), patches per second
and the peak of allocated device memory above what was resident before the call.

  ips      ``IPSNet.ips`` on device-resident patches: 16 x 2,500 x 1x32x32, 16 x 900 x 1x50x50, 16 x 192 x 3x100x100, and
           one 2,500-patch image alone (float32: the one-image stream kernel; uint8: the parts)
  stem     the layer-by-layer trunks' stem + max-pool kernels alone (through the C ABI on a trunk description without
           residual blocks, ``stem_alone``), and the whole trunk on the same patches for scale
  lazy     ``ips`` on a HOST tensor of the 16 x 2,500 shape, pinned and pageable

    python tools/uint8_patches_bench.py [--reps 30] [--out profiles/uint8_patches.json] [--only NAME] [--repo CHECKOUT]

``--repo``: the checkout to import ``ips_amd`` from (default: this file's) - the same tool on a parent commit's build gives the
baseline of a comparison; ``max_ms`` - ``min_ms`` of a row is that commit's own run-to-run spread.
"""

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--repo" in sys.argv[1:-1]:                 # (read here: the imports below are the checkout's)
    REPO = os.path.abspath(sys.argv[sys.argv.index("--repo") + 1])
sys.path.insert(0, REPO)

from ips_amd import hip, quant, synth         # noqa: E402
from ips_amd.architecture import IPSNet       # noqa: E402

IPS_SIZES = (
    ("mnist 16x2500x1x32x32", lambda: synth.mnist_conf(N=2500, M=64, I=64), 16),
    ("native50 16x900x1x50x50", lambda: synth.mnist_conf(N=900, M=100, I=100, patch=50), 16),
    ("traffic 16x192x3x100x100", lambda: synth.traffic_conf(N=192, M=16, I=32, patch=100), 16),
    ("mnist 1x2500x1x32x32 (one image)", lambda: synth.mnist_conf(N=2500, M=64, I=64), 1),
)
STEMS = (("stem_pool50 4096x1x50x50", lambda: synth.mnist_conf(N=900, M=100, I=100, patch=50), 4096),
         ("stem_pool100x3 1024x3x100x100", lambda: synth.traffic_conf(N=192, M=16, I=32, patch=100), 1024))


def table_for(conf):
    if conf.n_chan_in == 3:
        return quant.patch_table(3, [0.485, 0.456, 0.406], [0.229, 0.224, 0.225])
    return quant.patch_table(1)


def byte_patches(conf, B, N=None):
    """Megapixel-MNIST-like bytes: most patches blank (1-channel nets), uniform bytes elsewhere."""
    g = torch.Generator().manual_seed(21)
    p = conf.patch_size
    q = torch.randint(0, 256, (B, N or conf.N, conf.n_chan_in, p[0], p[1]), dtype=torch.uint8, generator=g)
    if conf.n_chan_in == 1:
        q *= (torch.rand((B, N or conf.N, 1, 1, 1), generator=g) >= 0.5).to(torch.uint8)
    return q


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    return dt * 1e3, torch.cuda.max_memory_allocated(dev) - base


def quartiles(v):
    q = statistics.quantiles(v, n=4)
    return {"median_ms": round(statistics.median(v), 4), "q1_ms": round(q[0], 4), "q3_ms": round(q[2], 4), "min_ms": round(min(v), 4),
            "max_ms": round(max(v), 4), "spread_ms": round(max(v) - min(v), 4)}


def alternate(calls, reps, warmup, dev):
    """calls: {mode: fn} -> {mode: (times, peak)} with the modes alternating call by call."""
    for _ in range(warmup):
        for fn in calls.values():
            timed(fn, dev)
    times, peaks = {m: [] for m in calls}, {m: 0 for m in calls}
    for _ in range(reps):
        for m, fn in calls.items():
            dt, peak = timed(fn, dev)
            times[m].append(dt)
            peaks[m] = max(peaks[m], peak)
    return times, peaks


def rows_of(kind, name, times, peaks, inputs, n_patches, reps, extra=None):
    out = []
    for m in times:
        row = {"kind": kind, "size": name, "storage": m, "input_bytes": inputs[m], "peak_bytes_above_input": peaks[m],
               "patches_per_call": n_patches, "reps": reps}
        row.update(quartiles(times[m]))
        row["patches_per_s"] = round(n_patches / (row["median_ms"] * 1e-3))
        row.update(extra or {})
        out.append(row)
        print(json.dumps(row), flush=True)
    return out


def stem_alone(plan, dev):
    """A trunk description with the plan's stem and NO residual blocks: ``ipsx_trunk_encode`` then launches the stem + pool
    kernel and the average pool of its output, nothing else.  -> (trunk, run(patches, table or None, out, workspace))"""
    t = hip.Trunk()
    t.c_in, t.h, t.w, t.stem = plan.trunk.c_in, plan.trunk.h, plan.trunk.w, plan.trunk.stem
    t.n_block, t.blocks, t.precision, t.patch_dtype = 0, None, 0, 0
    lib = hip.lib()

    def run(x, table, out, ws):
        n = x.shape[0]
        if table is None:
            hip._ck(lib.ipsx_trunk_encode(C.byref(t), hip._p(x), n, hip._p(out), hip._p(ws), ws.numel(), hip._stream()), "ipsx_trunk_encode")
        else:
            hip._ck(lib.ipsx_trunk_encode_u8(C.byref(t), hip._p(x), hip._p(table), n, hip._p(out), hip._p(ws), ws.numel(), hip._stream()),
                    "ipsx_trunk_encode_u8")
    return t, run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "uint8_patches.json"))
    ap.add_argument("--only", default=None)
    ap.add_argument("--repo", default=REPO, help="checkout to import ips_amd from")
    ap.add_argument("--label", default="head", help="what the figures belong to, e.g. the commit (stored in the JSON)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []

    def wanted(name):
        return not args.only or args.only in name

    # ---- ips() on device-resident patches
    for name, conf_fn, B in IPS_SIZES:
        if not wanted(name):
            continue
        conf = conf_fn()
        net = synth.fill_weights(IPSNet(dev, conf), 7).to(dev).eval()
        net.set_patch_table(table_for(conf))
        q = byte_patches(conf, B).to(dev)
        x = quant.dequant(q, net.patch_table)
        same = torch.equal(net.ips(q)[0], net.ips(x)[0])
        times, peaks = alternate({"float32": lambda: net.ips(x), "uint8": lambda: net.ips(q)}, args.reps, args.warmup, dev)
        rows += rows_of("ips, device-resident", name, times, peaks, {"float32": x.numel() * 4, "uint8": q.numel()}, B * conf.N,
                        args.reps, {"same_selection": same})
        del x, q, net
        torch.cuda.empty_cache()

    # ---- the stem + pool kernels alone (and, for scale, the whole layer-by-layer trunk on the same patches)
    for name, conf_fn, n in STEMS:
        if not wanted(name):
            continue
        conf = conf_fn()
        net = synth.fill_weights(IPSNet(dev, conf), 7).to(dev).eval()
        plan = hip.EncoderPlan(net.encoder, True)
        table = table_for(conf).to(dev)
        q = byte_patches(conf, 1, n)[0].to(dev)
        x = quant.dequant(q, table)
        whole = plan.encode(x)
        same = torch.equal(plan.encode(q, table=table), whole)
        kernel = hip.encoder_kernel_name(plan)
        inputs = {"float32": x.numel() * 4, "uint8": q.numel()}
        t0, run = stem_alone(plan, dev)
        ws = torch.empty(hip.lib().ipsx_trunk_workspace_bytes(C.byref(t0), n), dtype=torch.uint8, device=dev)
        o32, o8 = (torch.empty((n, 64), dtype=torch.float32, device=dev) for _ in range(2))
        run(x, None, o32, ws)
        run(q, table, o8, ws)
        same_stem = torch.equal(o32, o8)
        times, peaks = alternate({"float32": lambda: run(x, None, o32, ws), "uint8": lambda: run(q, table, o8, ws)},
                                 args.reps, args.warmup, dev)
        rows += rows_of("stem + pool kernel alone (+ the average pool of its output: a trunk without blocks)", name, times, peaks,
                        inputs, n, args.reps, {"same_output": same_stem})
        out = torch.empty_like(whole)
        times, peaks = alternate({"float32": lambda: plan.encode(x, out=out), "uint8": lambda: plan.encode(q, out=out, table=table)},
                                 args.reps, args.warmup, dev)
        rows += rows_of("encode, whole trunk (%s)" % kernel, name, times, peaks, inputs, n, args.reps, {"same_embeddings": same})
        del x, q, net, plan, ws
        torch.cuda.empty_cache()

    # ---- lazy loading: the patches on the host
    name = "lazy mnist 16x2500x1x32x32"
    if wanted(name):
        conf = synth.mnist_conf(N=2500, M=64, I=64)
        net = synth.fill_weights(IPSNet(dev, conf), 7).to(dev).eval()
        net.set_patch_table(table_for(conf))
        q = byte_patches(conf, 16)
        x = quant.dequant(q, net.patch_table.cpu())
        for kind, pin in (("pinned", True), ("pageable", False)):
            qh, xh = (q.pin_memory(), x.pin_memory()) if pin else (q, x)
            same = torch.equal(net.ips(qh)[0], net.ips(xh)[0])
            times, peaks = alternate({"float32": lambda: net.ips(xh), "uint8": lambda: net.ips(qh)}, args.reps, args.warmup, dev)
            rows += rows_of("ips, lazy (%s host tensor)" % kind, name, times, peaks, {"float32": x.numel() * 4, "uint8": q.numel()},
                            16 * conf.N, args.reps, {"same_selection": same})
        del net
        torch.cuda.empty_cache()

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"tool": "tools/uint8_patches_bench.py", "label": args.label, "device": torch.cuda.get_device_name(dev), "rows": rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
