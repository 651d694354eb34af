#!/usr/bin/env python
"""Device time and peak memory of the feature projector's training step - LayerNorm + Linear + BatchNorm1d + ReLU, forward
and backward - on stock ATen ops and on libipsx's kernels (training/fused_projector.py), at the reference's shipped
CAMELYON size (B * M, F, D) = (80,000, 2048, 512) and at a smaller one.

Stock and fused ALTERNATE inside one process (the clocks and the neighbours are the same for both); every sample is a HIP
event pair around one forward or one backward, the figure the median of ``--reps`` samples after ``--warmup`` rounds.
Prints one JSON line per (shape, dtype); ``--out`` also writes them to a file.

    python tools/train_projector_bench.py --out profiles/train_projector_bench.json
"""
import argparse
import json
import os
import statistics
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ips_amd.training import fused_projector          # noqa: E402

FP32_MFMA_PEAK = 157.3e12          # MI355X: 256 CUs x 256 flop / cycle (v_mfma_f32_32x32x2_f32) x 2.4 GHz


def _sample(enc, x, fused):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    enc.zero_grad(set_to_none=True)
    ev[0].record()
    emb = fused_projector.encode(enc, x) if fused else enc(x.float())
    ev[1].record()
    g = torch.ones_like(emb)
    ev[2].record()
    emb.backward(g)
    ev[3].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]), ev[2].elapsed_time(ev[3])


def _peak(enc, x, fused):
    enc.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    emb = fused_projector.encode(enc, x) if fused else enc(x.float())
    emb.backward(torch.ones_like(emb))
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del emb
    enc.zero_grad(set_to_none=True)
    return peak


def run(rows, f, d, dtype, reps, warmup):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    enc = nn.Sequential(nn.LayerNorm(f, eps=1e-5, elementwise_affine=False), nn.Linear(f, d), nn.BatchNorm1d(d), nn.ReLU()).to(dev).train()
    assert fused_projector.supported(enc)
    x = (torch.randn((rows, f), device=dev) * 0.7 + 0.3).to(dtype)
    t = {"stock": ([], []), "fused": ([], [])}
    for it in range(warmup + reps):
        for name in ("stock", "fused"):
            fwd, bwd = _sample(enc, x, name == "fused")
            if it >= warmup:
                t[name][0].append(fwd)
                t[name][1].append(bwd)
    flop = 2.0 * rows * f * d
    out = {"rows": rows, "F": f, "D": d, "dtype": str(dtype).replace("torch.", ""), "reps": reps, "gemm_gflop": flop / 1e9}
    for name in ("stock", "fused"):
        fwd, bwd = statistics.median(t[name][0]), statistics.median(t[name][1])
        out[name] = {"forward_ms": round(fwd, 4), "backward_ms": round(bwd, 4), "step_ms": round(fwd + bwd, 4),
                     "forward_min_ms": round(min(t[name][0]), 4), "backward_min_ms": round(min(t[name][1]), 4),
                     "peak_mb": round(_peak(enc, x, name == "fused") / 1e6, 1)}
    # the whole forward / backward holds one GEMM each (plus the memory passes): a LOWER bound of what the GEMM reaches
    out["fused"]["forward_frac_of_fp32_mfma_peak"] = round(flop / (out["fused"]["forward_ms"] * 1e-3) / FP32_MFMA_PEAK, 3)
    out["fused"]["backward_frac_of_fp32_mfma_peak"] = round(flop / (out["fused"]["backward_ms"] * 1e-3) / FP32_MFMA_PEAK, 3)
    out["speedup_step"] = round(out["stock"]["step_ms"] / out["fused"]["step_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="80000x2048x512,16384x2048x512")
    ap.add_argument("--dtypes", default="float32,float16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 20, "medians of at least 20 samples"
    lines = []
    for shape in a.shapes.split(","):
        rows, f, d = (int(v) for v in shape.split("x"))
        for dt in a.dtypes.split(","):
            line = json.dumps(run(rows, f, d, getattr(torch, dt), a.reps, a.warmup))
            print(line, flush=True)
            lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
