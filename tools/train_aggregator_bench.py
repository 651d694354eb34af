#!/usr/bin/env python
"""Device time and peak memory of the cross-attention aggregator's training step - ``Transformer.forward`` and its backward -
on stock ATen ops (``IPSX_TRAIN_AGGREGATOR=0``: K and V of all B x M embeddings) and on libipsx's attention pool on folded
queries (training/fused_aggregator.py), at the three shipped shapes, attention dropout off and on.

Stock and fused ALTERNATE inside one process (the clocks and the neighbours are the same for both); every sample is a HIP
event pair around one forward or one backward, the figure the median of ``--reps`` samples after ``--warmup`` rounds.
Prints one JSON line per (shape, dropout); ``--out`` also writes them to a file.

    python tools/train_aggregator_bench.py --out profiles/train_aggregator_bench.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ips_amd.architecture.transformer import Transformer          # noqa: E402
from ips_amd.training import fused_aggregator                     # noqa: E402

# name: (B, M, n_token, H, D, D_k, D_v, D_inner) - config/camelyon_config.yml, traffic_config.yml, mnist_config.yml
SHAPES = {"camelyon": (16, 5000, 1, 8, 512, 64, 64, 2048), "traffic": (16, 10, 1, 8, 512, 64, 64, 2048),
          "mnist": (16, 100, 4, 8, 128, 16, 16, 512)}


def _route(fused):
    os.environ["IPSX_TRAIN_AGGREGATOR"] = "1" if fused else "0"


def _sample(transf, x, fused):
    _route(fused)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    transf.zero_grad(set_to_none=True)
    x.grad = None
    ev[0].record()
    out = transf(x)
    ev[1].record()
    g = torch.ones_like(out)
    ev[2].record()
    out.backward(g)
    ev[3].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]), ev[2].elapsed_time(ev[3])


def _peak(transf, x, fused):
    _route(fused)
    transf.zero_grad(set_to_none=True)
    x.grad = None
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = transf(x)
    out.backward(torch.ones_like(out))
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    transf.zero_grad(set_to_none=True)
    x.grad = None
    return peak


def run(name, dropout, reps, warmup):
    B, M, T, H, D, Dk, Dv, Di = SHAPES[name]
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    transf = Transformer(T, H, D, Dk, Dv, Di, attn_dropout=0.1, dropout=0.1).to(dev)
    transf.train(dropout)
    assert fused_aggregator.supported(transf)
    x = torch.randn((B, M, D), device=dev).requires_grad_()          # (the encoder's output: it takes a gradient)
    t = {"stock": ([], []), "fused": ([], [])}
    for it in range(warmup + reps):
        for route in ("stock", "fused"):
            fwd, bwd = _sample(transf, x, route == "fused")
            if it >= warmup:
                t[route][0].append(fwd)
                t[route][1].append(bwd)
    out = {"shape": name, "B": B, "M": M, "D": D, "R": H * T, "dropout": dropout, "reps": reps}
    for route in ("stock", "fused"):
        fwd, bwd = statistics.median(t[route][0]), statistics.median(t[route][1])
        step = sorted(f + b for f, b in zip(*t[route]))
        out[route] = {"forward_ms": round(fwd, 4), "backward_ms": round(bwd, 4), "step_ms": round(fwd + bwd, 4),
                      "step_min_ms": round(step[0], 4), "step_max_ms": round(step[-1], 4),
                      "peak_mb": round(_peak(transf, x, route == "fused") / 1e6, 1)}
    out["speedup_step"] = round(out["stock"]["step_ms"] / out["fused"]["step_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="camelyon,traffic,mnist")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 20, "medians of at least 20 samples"
    before = os.environ.get("IPSX_TRAIN_AGGREGATOR")
    lines = []
    for name in a.shapes.split(","):
        for dropout in (False, True):
            line = json.dumps(run(name, dropout, a.reps, a.warmup))
            print(line, flush=True)
            lines.append(line)
    if before is None:
        os.environ.pop("IPSX_TRAIN_AGGREGATOR", None)
    else:
        os.environ["IPSX_TRAIN_AGGREGATOR"] = before
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
