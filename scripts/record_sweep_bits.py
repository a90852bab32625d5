#!/usr/bin/env python3
"""Record tests/golden/sweep_bits_parent.npz: the bits of the Lanczos step kernels before a change that must keep them.

    python scripts/record_sweep_bits.py [OUT.npz]

Run it ONCE, on an MI355X, with the build whose numbers are to be kept (the parent of a change to k_sweep, k_dots,
k_update or to what the operator of a step stores), and commit the file; tests/test_gpu_sweep_bits.py then holds
every later build against it, bit for bit.  The cases are those of tests/sweep_bits_cases.py, one child process per
configuration (default, EIGENEX_TWO_SWEEPS=1); the keys are "<configuration>/<case>/<schedule>/<key>" and "cus", the
CU count of the recording device.
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import sweep_bits_cases as cases  # noqa: E402


def main(argv):
    dst = argv[0] if argv else os.path.join(ROOT, "tests", "golden", "sweep_bits_parent.npz")
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for name, _ in cases.CONFIGS:
            res = cases.run_config(name, os.path.join(d, name + ".npz"))
            cus = res.pop("cus")
            assert "cus" not in out or out["cus"] == cus
            out["cus"] = cus
            out.update({name + "/" + k: v for k, v in res.items()})
    tmp = dst + ".part.npz"
    np.savez_compressed(tmp, **out)
    os.replace(tmp, dst)
    print("%d arrays, %d CUs -> %s (%d bytes)" % (len(out), int(out["cus"]), dst, os.path.getsize(dst)))


if __name__ == "__main__":
    main(sys.argv[1:])
