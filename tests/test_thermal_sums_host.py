"""The host arithmetic of the finite-temperature Lanczos method (include/cmpt/eigen_ex/thermal_sums.hpp) in a stand-alone
program under AddressSanitizer + UBSan: tests/cpp/thermal_sums_test.cpp holds Z, E, C, S, F and an observable of a two-level
system and of a truncated harmonic ladder against their closed forms within 50 eps relative, keeps every sum finite at
beta (theta_max - theta_min) = 1e4, and checks the delete-one jackknife (zero for identical samples).  No GPU, no library."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_thermal_sums_against_closed_forms(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "thermal_sums_test")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-I", os.path.join(ROOT, "cmpt-eigenex_amd", "include"), os.path.join(ROOT, "tests", "cpp", "thermal_sums_test.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    print(out.stdout.decode())
    assert out.returncode == 0, (out.stdout.decode()[-1500:], out.stderr.decode()[-3000:])
    assert b"THERMAL SUMS OK" in out.stdout
