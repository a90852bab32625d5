"""The full sweep's queue of parked tiles (kernels.hip: SweepPark<DEPTH>) against its direct stores, byte for byte.

k_sweep<false, DEPTH> keeps the two results (column k and w) of up to DEPTH tiles in LDS.  A boundary of the chip-wide clock
releases all of them, oldest first; a tile that finds the queue full at its end releases the oldest; the flush behind the tile
loop releases the rest in order.  The same values must reach the same addresses as when every tile stores at its end
(EIGENEX_SWEEP_DIRECT_STORES=1): alpha, beta, the state with the repair counter, every column and W of
tests/sweep_park_depth_cases.py are compared between child processes (the switches are read once per process).

    direct                   the reference
    d1 / d2                  EIGENEX_SWEEP_PARK_TILES=1 / the default (two tiles where they fit), the depth's default slot
    d1_early / d2_early      EIGENEX_SWEEP_SLOT_SHIFT=0: a boundary has passed at the first column group, where there is one
    d1_mid / d2_mid          EIGENEX_SWEEP_SLOT_SHIFT=9 (5 us): releases fall inside tiles, with one or both places occupied
    d1_late / d2_late        EIGENEX_SWEEP_SLOT_SHIFT=50: no boundary ever passes, tiles leave at a full queue or at the flush
    d2_no_graphs             the default launches outside recorded graphs

All cases run one workgroup per CU (tune(1, 4, 0), G workgroups) on one_sweep_reference's tridiagonal operator; the shapes give a
workgroup one, two (queue never full), three (first release at a tile end with the queue full) and five tiles (the queue wraps
twice).  The long case crosses the step at which launch_sweep falls from two parked tiles to one: beside 6 (k + 1) doubles of sums
and 32 bytes of static LDS, 2 * 32768 bytes of parking fit into the 81920-byte budget while 48 (k + 1) <= 16352, that is up to
k = 339; a basis of 345 columns takes k = 0..344."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import sweep_park_depth_cases as cases
from tests import sweep_parked_cases as parked_cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = (
    ("direct", {"EIGENEX_SWEEP_DIRECT_STORES": "1"}),
    ("d1", {"EIGENEX_SWEEP_PARK_TILES": "1"}),
    ("d1_early", {"EIGENEX_SWEEP_PARK_TILES": "1", "EIGENEX_SWEEP_SLOT_SHIFT": "0"}),
    ("d1_mid", {"EIGENEX_SWEEP_PARK_TILES": "1", "EIGENEX_SWEEP_SLOT_SHIFT": "9"}),
    ("d1_late", {"EIGENEX_SWEEP_PARK_TILES": "1", "EIGENEX_SWEEP_SLOT_SHIFT": "50"}),
    ("d2", {}),
    ("d2_early", {"EIGENEX_SWEEP_PARK_TILES": "2", "EIGENEX_SWEEP_SLOT_SHIFT": "0"}),
    ("d2_mid", {"EIGENEX_SWEEP_PARK_TILES": "2", "EIGENEX_SWEEP_SLOT_SHIFT": "9"}),
    ("d2_late", {"EIGENEX_SWEEP_PARK_TILES": "2", "EIGENEX_SWEEP_SLOT_SHIFT": "50"}),
    ("d2_no_graphs", {"EIGENEX_NO_GRAPHS": "1"}),
)
PARKED = [c[0] for c in CONFIGS[1:]]
KEYS = ("alpha", "beta", "state", "V", "W")


def test_depth_change_lies_inside_the_long_case():
    """the constants of the docstring: two tiles fit up to k = 339, and the long case runs past that"""
    budget, park, static = 80 * 1024, 2 * cases.TILE * 8, 4 * 8

    def fits(depth, k):
        return depth * park + 6 * 8 * (k + 1) + static <= budget

    k2 = max(k for k in range(1024) if fits(2, k))
    assert k2 == cases.LAST_K_AT_DEPTH_2 == 339
    assert k2 + 1 < cases.LONG_CAP - 1 and fits(1, cases.LONG_CAP - 1)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """configuration -> {key: array}; after a child that did not exit normally no further child is started"""
    d = tmp_path_factory.mktemp("sweep_park_depth")
    res, failure = {}, None
    for name, extra in CONFIGS:
        env = {k: v for k, v in os.environ.items() if not k.startswith("EIGENEX_")}
        env.update(extra)
        out = str(d / (name + ".npz"))
        try:
            r = subprocess.run([sys.executable, "-m", "tests.sweep_park_depth_cases", out], cwd=ROOT, env=env, capture_output=True, text=True,
                               timeout=120)
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
@pytest.mark.parametrize("case", ["n1", "n2047", "n2048", "n2049", "two_tiles", "three_tiles", "five_tiles"])
def test_queue_states_and_tile_shapes(runs, config, case):
    """one workgroup per CU; k = 0..11 in every shape"""
    ref = _need(runs, "direct")
    G = int(ref["G"][0])
    st = ref[case + "/state"]
    if cases.shape_rows(G)[case] > cases.CALLS:
        assert st[0] == cases.CALLS and st[4] == 0  # all twelve steps ran
    _same(runs, config, case)


@pytest.mark.parametrize("config", ["direct"] + PARKED)
@pytest.mark.parametrize("sched", list(parked_cases.BATCHES))
@pytest.mark.parametrize("case", cases.CUT_CASES)
def test_batch_cuts_leave_nothing_parked(runs, config, sched, case):
    """the newest column read between batches, and everything at the end, as in one batch of the direct path"""
    ref, got = _need(runs, "direct"), _need(runs, config)
    for k in KEYS:
        a, b = ref["%s/%s" % (case, k)], got["%s/%s/%s" % (case, sched, k)]
        assert a.shape == b.shape and np.array_equal(a, b), "%s %s %s differs from one batch with direct stores" % (config, sched, k)
    a, b = ref["%s/%s/newest" % (case, sched)], got["%s/%s/newest" % (case, sched)]
    assert a.shape == b.shape and a.shape[0] == len(parked_cases.BATCHES[sched]) - 1 and np.array_equal(a, b)


@pytest.mark.parametrize("config", PARKED)
def test_across_the_depth_change(runs, config):
    ref = _need(runs, "direct")
    st = ref["long/state"]
    assert st[0] == cases.LONG_CAP and st[4] == 0, st  # every step up to k = 344 ran
    _same(runs, config, "long")
