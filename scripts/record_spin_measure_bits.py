#!/usr/bin/env python3
"""Record tests/golden/spin_measure_bits_parent.npz: the bits of k_spin_measure before a change that must keep them.

    python scripts/record_spin_measure_bits.py [OUT.npz]

Run it ONCE, on an MI355X, with the build whose numbers are to be kept (the parent of a change to k_spin_measure,
k_spin_measure_reduce or the row walk they share with the spin operator kernels), and commit the file;
tests/test_gpu_spin_measure.py::test_measurement_bits_equal_the_parent_build then holds every later build against it, bit for
bit.  The shapes, term lists and the vector are those of tests/spin_measure_cases.py; the keys are "<sites>_<n_up or full>/norm2",
".../diag" and ".../flip" (raw bytes) and "cus", the CU count of the recording device, which the last shape's grid depends on.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import spin_measure_cases as cases  # noqa: E402


def main(argv):
    import torch

    from cmpt_eigenex_amd import capi

    dst = argv[0] if argv else os.path.join(ROOT, "tests", "golden", "spin_measure_bits_parent.npz")
    out = {"cus": np.array(int(torch.cuda.get_device_properties(0).multi_processor_count), np.int64)}
    for (L, n_up, per_cu) in cases.BITS_SHAPES:
        for k, v in cases.measure_bits(capi, L, n_up, per_cu).items():
            out[cases.bits_key(L, n_up) + "/" + k] = v
    tmp = dst + ".part.npz"
    np.savez_compressed(tmp, **out)
    os.replace(tmp, dst)
    print("%d arrays, %d CUs -> %s (%d bytes)" % (len(out), int(out["cus"]), dst, os.path.getsize(dst)))


if __name__ == "__main__":
    main(sys.argv[1:])
