"""`bench.py` without --full times the steps and prints the line; --full adds the checks and side figures around the
same timed steps.  The option is testable here; the GPU test runs the benchmark both ways."""
import json
import os
import subprocess
import sys

import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
SIDE_FIGURES = ("value_replay", "value_one_stream", "value_synchronous", "value_cold", "value_no_hints",
                "value_first_trace", "result_sink", "record_plans")


def test_full_is_off_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert bench.parse_args().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--full"])
    assert bench.parse_args().full is True


def _line(extra):
    done = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                           "--reps", "1", "--rays", "100000", "--side-steps", "2", "--no-cpu-baseline"] + extra,
                          capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stderr[-2000:]
    return json.loads(done.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_a_plain_run_prints_the_headline_and_full_adds_the_rest():
    plain, full = _line([]), _line(["--full"])
    for line in (plain, full):
        assert all(key in line for key in HEADLINE), sorted(line)
        assert line["value"] > 0 and line["ms_per_step"] > 0 and line["steps"] == 3
        assert line["roofline"]["kernel_ms_per_step"] > 0  # priced on the timed region itself
    assert plain["config"]["full"] is False and full["config"]["full"] is True
    assert not any(key in plain for key in SIDE_FIGURES), sorted(plain)
    assert plain["roofline"]["one_stream"] is None and plain["end_to_end_trace"] is None and plain["verified"] is None
    assert all(key in full for key in SIDE_FIGURES), sorted(full)
    assert full["roofline"]["one_stream"]["avg_launch_ms"] > 0 and full["end_to_end_trace"]["ms"] > 0
    # the same timed steps: the same rows
    assert plain["config"]["rows_per_generation"] == full["config"]["rows_per_generation"]
