"""tests/golden/bf16_trunk.npz is what tests/test_hip_kernels.py::test_bf16_trunk_matches_recorded_first_build takes it
for (tools/gen_golden_bf16_trunk.py wrote it): checked without a GPU."""

import os

import numpy as np
import pytest

from tests.util import GOLDEN_DIR, row_digests

N, HEAD, D = 1203, 24, 128


@pytest.fixture(scope="module")
def record():
    return np.load(os.path.join(GOLDEN_DIR, "bf16_trunk.npz"))


def test_shapes_and_dtypes(record):
    assert sorted(record.files) == ["digest_f16", "digest_f32", "recorded_at", "rows_f16", "rows_f32"]
    for tag in ("f32", "f16"):
        rows, dig = record["rows_" + tag], record["digest_" + tag]
        assert rows.shape == (HEAD, D) and rows.dtype == np.float32
        assert dig.shape == (N, 16) and dig.dtype == np.uint8
    at = str(record["recorded_at"])
    assert record["recorded_at"].shape == () and "build 1" in at and len(at) < 64


@pytest.mark.parametrize("tag", ["f32", "f16"])
def test_rows_are_finite_and_carry_their_digests(record, tag):
    rows = record["rows_" + tag]
    assert np.isfinite(rows).all()
    assert np.array_equal(row_digests(rows), record["digest_" + tag][:HEAD])


def test_the_two_storages_were_recorded_from_different_inputs(record):
    assert (record["rows_f32"].view(np.uint32) != record["rows_f16"].view(np.uint32)).any()
    assert (record["digest_f32"] != record["digest_f16"]).any()


def test_row_digests_tell_the_sign_of_zero_apart():
    a = np.zeros((2, D), dtype=np.float32)
    a[1, 5] = -0.0
    d = row_digests(a)
    assert d.shape == (2, 16) and (d[0] != d[1]).any() and np.array_equal(a[0], a[1])
