"""bench.py --full: a plain run does what its headline figure needs (set-up, warm-up, the timed steps, --dump-outputs, the
line); the CPU baseline with its comparison against the device, the repeat of a launch-bound solve without per-launch events
and the recorded PMC traffic wait behind --full.  CPU: the option.  GPU: a small Laplacian both ways, same outputs."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
spec = importlib.util.spec_from_file_location("bench_under_test_full", BENCH)
bench = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bench)

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("cpu_baseline", "without_per_launch_events")


def test_full_is_an_option_and_off_by_default():
    assert bench.parse_args(["--gpus", "1", "--steps", "2", "--warmup", "1"]).full is False
    assert bench.parse_args(["--gpus", "1", "--steps", "2", "--warmup", "1", "--full"]).full is True
    a = bench.parse_args(["--full", "--no-cpu-baseline"])
    assert a.full and a.no_cpu_baseline


def _run(tmp_path, name, *flags):
    d = tmp_path / name
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--grid-edge", "24", "--krylov-steps", "20", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(d), *flags], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0]), {f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))}


@pytest.mark.gpu
def test_plain_line_is_lean_and_full_line_carries_the_rest(tmp_path):
    plain, plain_out = _run(tmp_path, "plain")
    full, full_out = _run(tmp_path, "full", "--full")
    for line in (plain, full):
        for k in HEADLINE:
            assert k in line, k
        assert line["metric"] == "lanczos_krylov_iterations_per_second" and line["unit"] == "iterations/s"
        assert line["higher_is_better"] is True and line["dtype"] == "f64"
        assert line["value"] > 0 and abs(line["value"] - 20 / (line["ms_per_step"] * 1e-3)) <= 1e-9 * line["value"]
        assert line["roofline"]["launches"] > 0  # booked by the timed steps themselves
    assert plain["full"] is False and full["full"] is True
    for k in FULL_ONLY:
        assert k not in plain, k
        assert k in full, k
    assert plain["roofline"]["traffic_is_current"] is None
    # 24^3 fits any host: the oracle ran on the same input, its coefficients are the device's to round-off
    assert full["cpu_baseline"]["value"] > 0
    assert full["cpu_baseline"]["max_abs_alpha_beta_difference_vs_device"] < 1e-12
    assert full["without_per_launch_events"]["value"] > 0
    assert "cpu_baseline" not in _run(tmp_path, "full_nocpu", "--full", "--no-cpu-baseline")[0]
    # the timed steps are the same steps: what they returned does not depend on --full
    assert sorted(plain_out) == sorted(full_out) == ["alpha", "beta", "eigenvalues"]
    for k in plain_out:
        np.testing.assert_array_equal(plain_out[k], full_out[k])
