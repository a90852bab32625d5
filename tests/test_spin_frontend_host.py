"""What the spin front-end classes share (cmpt/eigen_ex/spin_frontend.hpp), as far as it needs no device, in a stand-alone
program under AddressSanitizer + UBSan (tests/cpp/spin_frontend_sanitize.cpp): the row of every product state of the sectors
(6,3), (5,0), (5,5) and (32,1) against the library's own listing and the two refusals, site masks with a repeated, a negative
and a 33rd site, the destination sector of the three kinds at the ends of the range, the normalisation of a zero, a NaN and a
non-unit state, the coefficient checks in each class's wording, and the pair masks with their unpacking at 2 and 5 sites."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_spin_frontend_helpers_under_sanitizers(tmp_path):
    import __graft_entry__ as g

    g.build()
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "spin_frontend_sanitize")
    lib = os.path.join(ROOT, "cmpt-eigenex_amd", "lib")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cmpt-eigenex_amd", "include"),
                           os.path.join(ROOT, "tests", "cpp", "spin_frontend_sanitize.cpp"), "-o", exe, "-L", lib, "-leigenex_hip", "-Wl,-rpath," + lib])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")  # the HIP runtime's own start-up allocations are not ours to judge
    out = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0, (out.stdout.decode()[-1500:], out.stderr.decode()[-2000:])
    assert b"SPIN FRONTEND OK" in out.stdout
