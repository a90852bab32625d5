"""Builds and runs tests/cpp/spin_frontend_logs_amd.cpp (the log and info() of every spin front-end class over the outcomes that
pass through spin_frontend.hpp) and returns its cases.  Shared by tests/test_gpu_spin_frontend_logs.py and
scripts/record_spin_frontend_logs.py, which wrote tests/golden/spin_frontend_logs.json."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "spin_frontend_logs.json")


def run(workdir):
    """[{"case": name, "info": ComputationInfo as int, "log": [line, ...]}, ...] of this tree's headers, on the GPU"""
    exe = os.path.join(str(workdir), "spin_frontend_logs_amd")
    lib = os.path.join(ROOT, "cmpt-eigenex_amd", "lib")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "cmpt-eigenex_amd", "include"), os.path.join(ROOT, "tests", "cpp", "spin_frontend_logs_amd.cpp"),
                           "-o", exe, "-L", lib, "-leigenex_hip", "-Wl,-rpath," + lib])
    return json.loads(subprocess.check_output([exe], timeout=300).decode())
