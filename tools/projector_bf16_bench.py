"""The bf16 feature projector (IPSX_PRECISION=bf16, csrc/projector_bf16.hip) on CAMELYON-sized slides (65,536 x 2048,
M = I = 256), one JSON object on stdout:

  kernels  - one slide: the typed row moments and the bf16 GEMM timed with HIP events (median of 20), per storage type,
             against the fp32 projector's two launches (ipsx_projector_stats + ipsx_projector_apply)
  ips      - ips() at B = 1 and 16 slides, float32 / float16 / bfloat16 storage under bf16, float32 under fp32: synced
             median rows/s, and the time of the projector's launches inside a call (HIP events around each
             EncoderPlan.encode / row_stats of the call, summed; null for the fp32 rows, whose projector is one
             persistent launch together with the logits - not measured here)
  loops    - B = 16, float16 storage: the loop-count sweep (IPSX_CAM_LOOPS = 2 / 4 / 8 / 16)

bench.py pads --batch 16 with float32 slides, so it cannot time half storage at B = 16; this script can.
    python tools/projector_bf16_bench.py --steps 8 > profiles/r09_projector_bf16_bench.json"""

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ips_amd import synth  # noqa: E402
from ips_amd.architecture import IPSNet  # noqa: E402
from ips_amd.hip_encoder import EncoderPlan  # noqa: E402

DEV = torch.device("cuda:0")
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def events_ms(fn, reps=20):
    ts = []
    for _ in range(reps + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts[3:])


def kernels(net, x32):
    out = {}
    for prec, storages in (("fp32", ("f32",)), ("bf16", ("f32", "f16", "bf16"))):
        os.environ["IPSX_PRECISION"] = prec
        plan = EncoderPlan(net.encoder, False)
        for st in storages:
            x = x32.to(DTYPES[st])
            stats = plan.row_stats(x)
            emb = plan.encode(x, stats=stats)
            t_stats = events_ms(lambda: plan.row_stats(x, out=stats))
            t_gemm = events_ms(lambda: plan.encode(x, stats=stats, out=emb))
            n = x.shape[0]
            out["%s_%s" % (prec, st)] = {"rows": n, "moments_us": 1e3 * t_stats, "gemm_us": 1e3 * t_gemm,
                                         "gemm_tflops": 2.0 * n * x.shape[1] * emb.shape[1] / (t_gemm * 1e-3) / 1e12,
                                         "moments_GBps": n * x.shape[1] * x.element_size() / (t_stats * 1e-3) / 1e9}
    os.environ["IPSX_PRECISION"] = "bf16"
    return out


class ProjectorTimer:
    """HIP events around every EncoderPlan.encode / row_stats launch of a call (the projector's share of its stream)."""

    def __init__(self):
        self.pairs = []
        self.orig = (EncoderPlan.encode, EncoderPlan.row_stats)
        timer = self

        def wrap(f):
            def g(*a, **k):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                r = f(*a, **k)
                e.record()
                timer.pairs.append((s, e))
                return r
            return g
        EncoderPlan.encode, EncoderPlan.row_stats = wrap(self.orig[0]), wrap(self.orig[1])

    def take_ms(self):
        torch.cuda.synchronize()
        ms = sum(s.elapsed_time(e) for s, e in self.pairs)
        self.pairs = []
        return ms

    def close(self):
        EncoderPlan.encode, EncoderPlan.row_stats = self.orig


def ips_rate(net, x, steps):
    net.ips(x)
    net.ips(x)
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        net.ips(x)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    t = statistics.median(ts)
    return {"ms": 1e3 * t, "rows_per_s": x.shape[0] * x.shape[1] / t}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--kernels-only", action="store_true", help="the one-slide kernel timings only (e.g. under rocprofv3)")
    args = ap.parse_args()
    conf = synth.camelyon_conf(N=args.rows, M=256, I=256)
    net = synth.fill_weights(IPSNet(DEV, conf), 7).to(DEV).eval()
    x16 = synth.make_patches(conf, 1 if args.kernels_only else 16, seed=21).to(DEV)
    res = {"kernels": kernels(net, x16[0])}
    if args.kernels_only:
        print(json.dumps(res))
        return
    ips = {}
    timer = ProjectorTimer()
    try:
        for prec, st in (("fp32", "f32"), ("bf16", "f32"), ("bf16", "f16"), ("bf16", "bf16")):
            os.environ["IPSX_PRECISION"] = prec
            for B in (1, 16):
                x = x16[:B].to(DTYPES[st])
                r = ips_rate(net, x, args.steps)
                timer.take_ms()
                net.ips(x)
                ms = timer.take_ms()
                r["projector_launches_ms"] = ms if prec == "bf16" else None
                ips["%s_%s_B%d" % (prec, st, B)] = r
                print(json.dumps({"ips": "%s_%s_B%d" % (prec, st, B), **r}), file=sys.stderr)
        res["ips"] = ips
        os.environ["IPSX_PRECISION"] = "bf16"
        xh = x16.half()
        loops = {}
        for L in (2, 4, 8, 16):
            os.environ["IPSX_CAM_LOOPS"] = str(L)
            loops[str(L)] = ips_rate(net, xh, args.steps)
            print(json.dumps({"loops": L, **loops[str(L)]}), file=sys.stderr)
        os.environ.pop("IPSX_CAM_LOOPS")
        res["loops_B16_f16"] = loops
    finally:
        timer.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
