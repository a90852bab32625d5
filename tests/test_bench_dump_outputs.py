"""bench.py --dump-outputs DIR: the arrays the last timed step returned, as DIR/<name>.npy in float64, the same for the same
arguments from run to run.  CPU: the writer and the argument checks.  GPU: a small Laplacian end to end against the oracle."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
spec = importlib.util.spec_from_file_location("bench_under_test", BENCH)
bench = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bench)


def test_dump_writes_float64_arrays_and_splits_complex(tmp_path):
    r = {"iterations": 5, "info_name": "Success", "alpha": np.arange(5.0), "beta": np.arange(4, dtype=np.float32),
         "eigenvalues": np.array([1 + 2j, 3 - 4j]), "eigenvectors": np.zeros((0, 0)), "nvec": np.int64(6)}
    bench.dump_outputs(str(tmp_path), r)
    assert sorted(os.listdir(tmp_path)) == ["alpha.npy", "beta.npy", "eigenvalues_imag.npy", "eigenvalues_real.npy"]
    for f in os.listdir(tmp_path):
        assert np.load(tmp_path / f).dtype == np.float64
    np.testing.assert_array_equal(np.load(tmp_path / "alpha.npy"), r["alpha"])
    np.testing.assert_array_equal(np.load(tmp_path / "beta.npy"), r["beta"])
    np.testing.assert_array_equal(np.load(tmp_path / "eigenvalues_real.npy"), [1.0, 3.0])
    np.testing.assert_array_equal(np.load(tmp_path / "eigenvalues_imag.npy"), [2.0, -4.0])


def test_dump_samples_large_arrays_by_fixed_rows(tmp_path):
    rows, cols = 3 * bench.DUMP_MAX_ENTRIES // 4 + 7, 4
    X = np.arange(rows * cols, dtype=np.float64).reshape(rows, cols, order="F")
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"eigenvectors": X, "eigenvalues": np.ones(cols)})
    got = np.load(tmp_path / "a" / "eigenvectors.npy")
    np.testing.assert_array_equal(got, np.load(tmp_path / "b" / "eigenvectors.npy"))  # the same sample every run
    assert got.shape == (bench.DUMP_MAX_ENTRIES // cols, cols) and got.nbytes <= bench.DUMP_MAX_BYTES
    picked = got[:, 0].astype(np.int64)  # column 0 of X holds the row index
    assert np.all(np.diff(picked) > 0)
    np.testing.assert_array_equal(got, X[picked])


@pytest.mark.parametrize("flags", [["--steps", "0"], ["--warmup", "-1"]])
def test_steps_and_warmup_are_checked(flags):
    with pytest.raises(SystemExit):
        bench.parse_args(flags)
    assert bench.parse_args(["--steps", "7", "--warmup", "0"]).steps == 7


@pytest.mark.gpu
def test_dump_of_the_timed_path_matches_the_oracle_and_repeats(tmp_path):
    from oracle import cref
    from cmpt_eigenex_amd import solver

    n, m = 24, 20
    out = {}
    for steps, warmup in ((1, 0), (3, 1)):
        d = tmp_path / f"s{steps}"
        p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--grid-edge", str(n), "--krylov-steps", str(m), "--steps", str(steps),
                            "--warmup", str(warmup), "--no-cpu-baseline", "--dump-outputs", str(d)],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        line = json.loads(p.stdout.decode().strip().splitlines()[-1])
        assert line["steps"] == steps and line["warmup"] == warmup
        out[steps] = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
    assert sorted(out[1]) == ["alpha", "beta", "eigenvalues"]
    for k in out[1]:
        assert out[1][k].dtype == np.float64
        np.testing.assert_array_equal(out[1][k], out[3][k])  # same arguments but the step count: the same numbers
    rowptr, col, val = cref.laplacian3d(n)
    ref = cref.CLanczos(rowptr, col, val, solver.default_start_vector(n ** 3), cap=m + 2)
    assert ref.run(m + 1) == m + 1
    np.testing.assert_allclose(out[1]["alpha"], ref.alpha, rtol=0, atol=1e-12)
    np.testing.assert_allclose(out[1]["beta"], ref.beta, rtol=0, atol=1e-12)
