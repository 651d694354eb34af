"""bench.py's plain line and ``--dump-outputs``: what a plain run prints, what it writes, and that the written arrays are
what the timed ``ips()`` call returns on the bench's inputs."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from ips_amd import synth
from ips_amd.architecture.transformer import pos_enc_1d
from tests.util import GOLDEN_DIR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_keeps_small_arrays_whole_and_samples_large_ones_the_same_way(tmp_path, monkeypatch):
    import bench
    small = {"a": np.arange(12, dtype=np.float32).reshape(3, 4), "b": np.linspace(0, 1, 5)}
    bench.dump_outputs(small, str(tmp_path / "small"))
    for k, v in small.items():
        got = np.load(str(tmp_path / "small" / (k + ".npy")))
        assert got.dtype == v.dtype and np.array_equal(got, v)

    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096)
    big = {"p": np.random.default_rng(1).random((64, 64), dtype=np.float32), "i": np.arange(1000, dtype=np.float64)}
    for run in ("one", "two"):
        bench.dump_outputs(big, str(tmp_path / run))
    sizes = 0
    for k, v in big.items():
        one, two = (np.load(str(tmp_path / r / (k + ".npy"))) for r in ("one", "two"))
        assert np.array_equal(one, two), "the sample must not change from run to run"
        assert one.ndim == 1 and 0 < one.size < v.size and np.isin(one, v).all()
        sizes += one.nbytes
    assert sizes <= 4096
    idx = np.load(str(tmp_path / "one" / "i.npy"))
    assert (np.diff(idx) > 0).all(), "sampled elements keep their order"


def test_steps_must_be_positive(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "7", "--warmup", "2"])
    args = bench.parse()
    assert args.steps == 7 and not args.full and args.dump_outputs is None


def test_options_of_the_full_run_are_not_ignored_silently(monkeypatch, capsys):
    import bench
    for argv, warned in ((["--steps", "3"], None), (["--full", "--cpu-seconds", "8", "--also", "none"], None),
                         (["--cpu-seconds", "8", "--no-kernel-events"], ("--cpu-seconds", "--no-kernel-events")),
                         (["--also", "cam", "--leg-timeout", "30", "--also-steps", "5"], ("--also", "--leg-timeout", "--also-steps"))):
        monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
        bench.parse()
        err = capsys.readouterr().err
        if warned is None:
            assert err == "", argv
        else:
            assert "ignored without --full" in err and all(o in err for o in warned), (argv, err)


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_call(tmp_path):
    out_dir = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--dump-outputs", str(out_dir)]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["metric"] == "patches scored/sec (no-grad IPS loop)" and line["unit"] == "patches/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    conf, B = synth.bench_workload("mnist")
    assert line["ms_per_step"] > 0 and abs(line["value"] - B * conf.N / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
    for extra in ("also_measured", "cpu_baseline", "rank_shard_model", "parity", "roofline", "value_pipelined"):
        assert extra not in line, extra

    got = {k: np.load(str(out_dir / (k + ".npy"))) for k in ("mem_patch", "mem_pos", "mem_idx")}
    assert got["mem_patch"].dtype == np.float32 and got["mem_idx"].dtype == np.float64
    assert got["mem_patch"].shape == (B, conf.M, 1, 32, 32) and got["mem_idx"].shape == (B, conf.M)
    idx = got["mem_idx"].astype(np.int64)
    want = np.load(os.path.join(GOLDEN_DIR, "bench_mnist.npz"))["trace_idx"][:, -1].astype(np.int64)
    assert np.array_equal(idx, want), "the timed call's selection differs from the reference's"
    x = synth.make_patches(conf, B, seed=21).numpy()
    assert np.array_equal(got["mem_patch"], x[np.arange(B)[:, None], idx]), "mem_patch is not the selected patches"
    pos = pos_enc_1d(conf.D, conf.N).numpy()                       # the host-made table IPSNet carries
    assert np.array_equal(got["mem_pos"], pos[idx]), "mem_pos is not the selected patches' positional rows"
