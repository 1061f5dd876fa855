"""`bench.py --dump-outputs DIR`: what the timed path returned in its last step, as .npy files (bench.dump_outputs).
The writer is testable here on host tensors; the GPU test runs the benchmark itself twice and compares."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_BYTES = 64 << 20


def _frame(total, seed=3):
    gen = torch.Generator().manual_seed(seed)
    rows = torch.rand((15, total), generator=gen, dtype=torch.float64)
    rows[7, ::97] = float("nan")  # rays that leave the scene leave NaN in some columns
    return rows


def _written(directory):
    return {name[:-4]: np.load(os.path.join(directory, name)) for name in sorted(os.listdir(directory))}


def test_a_large_frame_is_written_as_a_seeded_sample(tmp_path):
    rows, counts = _frame(bench.DUMP_ROWS_MAX + 12345), [200000, 62345, 50000]
    names = bench.dump_outputs(str(tmp_path / "a"), rows, counts)
    bench.dump_outputs(str(tmp_path / "b"), rows, counts)
    a, b = _written(tmp_path / "a"), _written(tmp_path / "b")
    assert sorted(a) == names == ["column_sums", "counts", "row_index", "rows"]
    for name in names:
        assert a[name].dtype in (np.float32, np.float64), name
        assert np.array_equal(a[name], b[name], equal_nan=True), name  # same frame, same files
    index = a["row_index"].astype(np.int64)
    assert a["rows"].shape == (15, bench.DUMP_ROWS_MAX) and index.shape == (bench.DUMP_ROWS_MAX,)
    assert np.all(np.diff(index) > 0) and index[-1] < rows.shape[1]
    assert np.array_equal(a["rows"], rows.numpy()[:, index], equal_nan=True)
    assert np.array_equal(a["counts"], counts)
    assert np.allclose(a["column_sums"], np.nansum(rows.numpy(), axis=1), rtol=1e-12, atol=0)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= LIMIT_BYTES


def test_a_small_frame_is_written_whole_and_ranks_keep_apart(tmp_path):
    rows = _frame(5000)
    for rank in range(2):
        assert bench.dump_outputs(str(tmp_path), rows, [4000, 1000], rank=rank, world=2) == \
            [f"{name}_rank{rank}" for name in ("column_sums", "counts", "row_index", "rows")]
    got = _written(tmp_path)
    assert len(got) == 8
    assert np.array_equal(got["rows_rank1"], rows.numpy(), equal_nan=True)
    assert np.array_equal(got["row_index_rank0"], np.arange(5000))


@pytest.mark.gpu
def test_bench_dumps_the_same_outputs_from_run_to_run(tmp_path):
    """Two short runs with the same arguments: the JSON line holds ms_per_step and the steps asked for, and the
    arrays of the last timed step are identical."""
    lines = []
    for run in ("a", "b"):
        done = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                               "--reps", "1", "--rays", "100000", "--side-steps", "0", "--no-cpu-baseline",
                               "--dump-outputs", str(tmp_path / run)], capture_output=True, text=True, timeout=600)
        assert done.returncode == 0, done.stderr[-2000:]
        lines.append(json.loads(done.stdout.strip().splitlines()[-1]))
    for line in lines:
        assert line["steps"] == 3 and line["ms_per_step"] > 0
        assert line["dumped_outputs"]["arrays"] == ["column_sums", "counts", "row_index", "rows"]
    a, b = _written(tmp_path / "a"), _written(tmp_path / "b")
    assert sorted(a) == ["column_sums", "counts", "row_index", "rows"]
    for name in a:
        assert np.array_equal(a[name], b[name], equal_nan=True), name
    assert a["rows"].shape == (15, a["row_index"].shape[0]) and a["row_index"][-1] < a["counts"].sum()
