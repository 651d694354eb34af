#!/usr/bin/env python
"""tests/golden/bf16_trunk.npz: what the bf16 fused trunk (IPSX_PRECISION=bf16, csrc/fused_trunk_bf16.h) computes on
the first 1203 patches of the mnist_full fixture, stored as float32 and as float16
(tests/test_hip_kernels.py::test_bf16_trunk_matches_recorded_first_build holds the library to it bit for bit):

    rows_f32, rows_f16      (24, 128) float32     the embeddings of patches 0 .. 23 from one plan.encode of all 1203
    digest_f32, digest_f16  (1203, 16) uint8      blake2b-16 of every row's 512 bytes (C order, little-endian float32)
    recorded_at             str                   where the record was taken

The COMMITTED file was recorded at commit e723970 from the trunk's first build (wave = patch, fused_trunk_split.h's
PL = 1 instantiation), which that commit could still force and which its test showed bit-identical to the two later
builds; the first and second builds were deleted in the commit after it.  The file is therefore the arithmetic contract
of the kernel that is left: if the library and the file disagree, the kernel changed arithmetic.  Rewriting the file
is only right when the arithmetic is changed ON PURPOSE.

    python tools/gen_golden_bf16_trunk.py                               compare the library with the committed file
    python tools/gen_golden_bf16_trunk.py --write --recorded-at TEXT    overwrite the file (needs a GPU either way)
"""

import argparse
import os
import sys

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
os.environ["IPSX_PRECISION"] = "bf16"

import numpy as np
import torch

from ips_amd import hip
from tests.util import Golden, row_digests

PATH = os.path.join(REPO, "tests", "golden", "bf16_trunk.npz")
N, HEAD = 1203, 24
STORAGES = (("f32", torch.float32), ("f16", torch.float16))


def compute():
    g = Golden("mnist_full")
    net = g.net("cuda:0")
    plan = hip.EncoderPlan(net.encoder, True)
    x_all = g.patches()[0, :N].to("cuda:0")
    pack = {}
    for tag, storage in STORAGES:
        emb = plan.encode(x_all.to(storage)).cpu().numpy()
        assert emb.shape == (N, 128) and emb.dtype == np.float32 and np.isfinite(emb).all()
        pack["rows_" + tag] = emb[:HEAD].copy()
        pack["digest_" + tag] = row_digests(emb)
    return pack


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--write", action="store_true", help="overwrite the committed file with this library's output")
    ap.add_argument("--recorded-at", default=None, help="with --write: the commit and kernel the record is taken from")
    args = ap.parse_args(argv)
    pack = compute()
    if args.write:
        if not args.recorded_at:
            ap.error("--write needs --recorded-at")
        np.savez_compressed(PATH, recorded_at=np.array(args.recorded_at), **pack)
        print("%s: %d KB, recorded at %s" % (os.path.relpath(PATH, REPO), os.path.getsize(PATH) // 1024, args.recorded_at))
        return 0
    z = np.load(PATH)
    print("committed file recorded at: %s" % str(z["recorded_at"]))
    bad = 0
    for tag, _ in STORAGES:
        rows = np.flatnonzero((pack["rows_" + tag].view(np.uint32) != z["rows_" + tag].view(np.uint32)).any(1))
        dig = np.flatnonzero((pack["digest_" + tag] != z["digest_" + tag]).any(1))
        print("%s: %d of %d rows differ in rows_%s %s, %d of %d in digest_%s %s" % (
            tag, rows.size, HEAD, tag, rows[:16].tolist(), dig.size, N, tag, dig[:16].tolist()))
        bad += rows.size + dig.size
    print("the library matches the committed file" if not bad else "MISMATCH: the library's arithmetic is not the file's")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
