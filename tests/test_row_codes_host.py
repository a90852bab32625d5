"""CPU tests of the row-code encoding (cmpt-eigenex_amd/csrc/row_codes.hpp): the host replay tests/cpp/row_codes_replay_host.cpp
under AddressSanitizer + UBSan and -ffp-contract=off -- detection, encoding, decoding back to every row's (column, value)
sequence, and the kernel's row loop against the stored-order row loop bit for bit -- on the seeded structures of
tests/structures.py and on corner cases built inside the program (empty rows, explicit and signed zeros, NaN payloads,
255 / 256 values, 8 / 9 / 16 / 17 offsets, conflicting stored orders, a column twice in a row, Laplacian shards of 1, 2, 3
and 8 loopback shards with their halo offsets)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_row_codes_host_replay(tmp_path):
    from structures import random_structure

    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "row_codes_replay_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                           "-pthread", "-I", os.path.join(ROOT, "cmpt-eigenex_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "row_codes_replay_host.cpp"), "-o", exe])
    files = []
    for seed in (1, 0, 2, 4, 7):
        n, rowptr, col, val, x, counts, shards, K = random_structure(seed)
        path = str(tmp_path / f"structure{seed}.bin")
        with open(path, "wb") as f:
            np.array([n, col.size, 0, 0, 0, 0, 0], np.int64).tofile(f)
            rowptr.tofile(f), col.tofile(f), val.tofile(f)
        files.append(path)
    out = subprocess.run([exe] + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, (out.stdout.decode()[-3000:], out.stderr.decode()[-1500:])
    assert b"ROW CODES REPLAY OK" in out.stdout
    text = out.stdout.decode()
    assert "255 values: 1 slots, 255 values" in text and "256 values: plain" in text
    assert "16 offsets: 16 slots" in text and "17 offsets: plain" in text and "8 offsets: 8 slots" in text
    assert "conflicting stored orders: plain" in text and "column twice in a row: plain" in text
