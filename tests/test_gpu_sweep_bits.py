"""The Lanczos step kernels (k_sweep; k_dots and k_update under EIGENEX_TWO_SWEEPS=1) keep their bits.

tests/golden/sweep_bits_parent.npz was recorded (scripts/record_sweep_bits.py) with the build in which the operator of a one-sweep
step still stored the raw column k+1.  The sweep is now that column's only writer, and any change to how the step kernels schedule
their loads has to leave the arithmetic alone: same operations on the same operands in the same order, so alpha, beta, the state
fields, the repair counter, every basis column and W are the same bytes.  The cases are in tests/sweep_bits_cases.py: every count
of streamed columns 0..11 (remainders 0..3 behind none, one, two full groups), k = 0 and k = 1, partial, exact and one-row tiles,
several tiles per workgroup, row codes with inline finalisers, and batch edges, where the closing pass meets the column the
operator no longer stores.  One child process per configuration."""
import os

import numpy as np
import pytest

from tests import sweep_bits_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sweep_bits_parent.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """configuration -> {key: array}; after a child that did not exit normally no further child is started"""
    d = tmp_path_factory.mktemp("sweep_bits")
    res = {"_failure": None}
    for name, _ in cases.CONFIGS:
        try:
            res[name] = cases.run_config(name, str(d / (name + ".npz")))
        except RuntimeError as e:
            res["_failure"] = str(e)
            break
    return res


@pytest.mark.parametrize("case", list(cases.CASES))
@pytest.mark.parametrize("config", [c[0] for c in cases.CONFIGS])
def test_bits_of_the_parent_build(runs, golden, config, case):
    if config not in runs:
        pytest.fail("no results for %s: %s" % (config, runs["_failure"]))
    got = runs[config]
    cus, cus_rec = int(got["cus"]), int(golden["cus"])
    assert cus == cus_rec, ("this device has %d CUs, the fixture was recorded on %d: the grid fixes the partial sums, so the "
                            "recorded bits do not apply here" % (cus, cus_rec))
    for sched in cases.SCHEDULES:
        for k in cases.KEYS:
            key = "%s/%s/%s" % (case, sched, k)
            want, have = golden[config + "/" + key], got[key]
            assert have.dtype == want.dtype and have.shape == want.shape and have.tobytes() == want.tobytes(), \
                "%s %s differs from the recorded bits" % (config, key)
