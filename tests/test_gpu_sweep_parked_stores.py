"""The full sweep's parked stores (kernels.hip: SweepPark) against its direct stores (EIGENEX_SWEEP_DIRECT_STORES=1), byte for byte.

k_sweep<false, true> keeps a tile's two results (column k and w) in LDS and stores them from the next tile, at a boundary of the
chip-wide clock, or at that tile's end when none has passed, or behind the tile loop.  The same values must reach the same
addresses as when every tile stores at its end: alpha, beta, every column, W, the state and the repair counter of
tests/sweep_parked_cases.py are compared between child processes (the switches are read once per process):

    direct           EIGENEX_SWEEP_DIRECT_STORES=1, the reference
    parked           the default: the slot follows the expected duration of a tile
    parked_no_graphs the same launches outside recorded graphs
    parked_late      EIGENEX_SWEEP_SLOT_SHIFT=50: no boundary ever passes, every tile leaves at its successor's end or at the flush
    parked_early     EIGENEX_SWEEP_SLOT_SHIFT=0: a boundary has passed at the first column group, where there is one

The longest basis a one-sweep state takes (capacity 1023, k up to 1022) needs 81,904 bytes of LDS with the parking, 16 below
the 80 KB per workgroup beside which launch_sweep stores directly: no solve crosses that point, so the case runs up to it."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import sweep_parked_cases as cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = (
    ("direct", {"EIGENEX_SWEEP_DIRECT_STORES": "1"}),
    ("parked", {}),
    ("parked_no_graphs", {"EIGENEX_NO_GRAPHS": "1"}),
    ("parked_late", {"EIGENEX_SWEEP_SLOT_SHIFT": "50"}),
    ("parked_early", {"EIGENEX_SWEEP_SLOT_SHIFT": "0"}),
)
PARKED = [c[0] for c in CONFIGS[1:]]
KEYS = ("alpha", "beta", "state", "V", "W")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """configuration -> {key: array}; after a child that did not exit normally no further child is started"""
    d = tmp_path_factory.mktemp("sweep_parked")
    res, failure = {}, None
    for name, extra in CONFIGS:
        env = {k: v for k, v in os.environ.items() if not k.startswith("EIGENEX_")}
        env.update(extra)
        out = str(d / (name + ".npz"))
        try:
            r = subprocess.run([sys.executable, "-m", "tests.sweep_parked_cases", out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
        except subprocess.TimeoutExpired as e:
            failure = "%s: timed out\n%s" % (name, (e.stderr or b"")[-4000:])
            break
        if r.returncode != 0:
            failure = "%s: exit status %d\n%s" % (name, r.returncode, r.stderr[-4000:])
            break
        with np.load(out) as z:
            res[name] = {k: z[k] for k in z.files}
    res["_failure"] = failure
    return res


def _need(runs, name):
    if name not in runs:
        pytest.fail("no results for %s: %s" % (name, runs["_failure"]))
    return runs[name]


def _same(runs, config, case, keys=KEYS):
    ref, got = _need(runs, "direct"), _need(runs, config)
    for k in keys:
        a, b = ref["%s/%s" % (case, k)], got["%s/%s" % (case, k)]
        assert a.shape == b.shape and np.array_equal(a, b), "%s %s %s differs from the direct stores" % (config, case, k)


@pytest.mark.parametrize("config", PARKED)
@pytest.mark.parametrize("case", ["n1", "n2047", "n2048", "n2049", "second_partial_tile", "three_tiles"])
def test_tile_shapes_and_column_counts(runs, config, case):
    """one workgroup per CU; k = 0..11 in every shape"""
    ref = _need(runs, "direct")
    G = int(ref["G"][0])
    st = ref[case + "/state"]
    if cases.shape_rows(G)[case] > cases.CALLS:
        assert st[0] == cases.CALLS and st[4] == 0  # all twelve steps ran
    _same(runs, config, case)


@pytest.mark.parametrize("config", ["direct"] + PARKED)
@pytest.mark.parametrize("sched", list(cases.BATCHES))
def test_batch_cuts_leave_nothing_parked(runs, config, sched):
    """the newest column read between batches, and everything at the end, as in one batch of the direct path"""
    ref, got = _need(runs, "direct"), _need(runs, config)
    case = "second_partial_tile"
    for k in KEYS:
        a, b = ref["%s/%s" % (case, k)], got["%s/%s/%s" % (case, sched, k)]
        assert a.shape == b.shape and np.array_equal(a, b), "%s %s %s differs from one batch with direct stores" % (config, sched, k)
    a, b = ref["%s/%s/newest" % (case, sched)], got["%s/%s/newest" % (case, sched)]
    assert a.shape == b.shape and a.shape[0] == len(cases.BATCHES[sched]) - 1 and np.array_equal(a, b)


@pytest.mark.parametrize("config", PARKED)
def test_up_to_the_lds_budget(runs, config):
    ref = _need(runs, "direct")
    st = ref["long/state"]
    assert st[0] == cases.LONG_CAP and st[4] == 0, st  # every step up to k = 1022 ran
    _same(runs, config, "long")
