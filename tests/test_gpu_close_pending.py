"""A batch of one-sweep Lanczos steps writes its newest column only when something reads it -- and nothing can tell.

The closing pass of a batch is split: alpha and the kept a' at the batch end, the column when a call that is not the next
one-sweep step touches the state (library.hip: settle_columns; EIGENEX_EAGER_CLOSE=1 writes it at every batch end, as before).
Everything here is bitwise: alpha, beta, the state fields, the repair counter, every column and W are the same bytes wherever the
batches are cut, whatever is called between them, with and without recorded graphs, and equal to the eager run.  The cases are in
tests/close_pending_cases.py (laplacian3d(17): two full tiles + 817 rows, also on one workgroup per CU; the tridiagonal
operators tri2049 / tri4097 of sweep_bits_cases; 16 calls).  One child process per configuration."""
import numpy as np
import pytest

from tests import close_pending_cases as cases

pytestmark = pytest.mark.gpu

STATE_KEYS = ("alpha", "beta", "state", "V", "W")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """configuration -> {key: array}; after a child that did not exit normally no further child is started"""
    d = tmp_path_factory.mktemp("close_pending")
    res = {"_failure": None}
    for name, _ in cases.CONFIGS:
        try:
            res[name] = cases.run_config(name, str(d / (name + ".npz")))
        except RuntimeError as e:
            res["_failure"] = str(e)
            break
    return res


def _need(runs, *names):
    missing = [n for n in names if n not in runs]
    if missing:
        pytest.fail("no results for %s: %s" % (", ".join(missing), runs["_failure"]))
    return [runs[n] for n in names]


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), "%s differs" % what


def _same_state(d1, p1, d2, p2, what):
    for k in STATE_KEYS:
        _same(d1[p1 + k], d2[p2 + k], "%s: %s" % (what, k))


def _same_prefix(d1, d2, prefix):
    k1, k2 = sorted(k for k in d1 if k.startswith(prefix)), sorted(k for k in d2 if k.startswith(prefix))
    assert k1 == k2 and k1
    for k in k1:
        if not k.endswith(("pending_before", "pending_after", "pending")):
            _same(d1[k], d2[k], k)


@pytest.mark.parametrize("case", list(cases.CASES))
def test_schedules_read_nothing_in_between(runs, case):
    """[all], [1, 1, 1, ...] and a mixed schedule, nothing read between the batches: the same bits, and those of the eager run"""
    lazy, eager = _need(runs, "default", "eager")
    ref = "%s/sched_whole/" % case
    assert lazy[ref + "state"][0] == cases.NCALLS and lazy[ref + "state"][4] == 0
    for sched in cases.SCHEDULES:
        _same_state(lazy, "%s/sched_%s/" % (case, sched), lazy, ref, "default " + sched)
        _same_state(eager, "%s/sched_%s/" % (case, sched), lazy, ref, "eager " + sched)


# what the flag reads behind each reader: configure leaves it to the next enqueue, clear is followed by the same batches again
PENDING_AFTER = {"configure": True, "clear": True}
UNCHANGED_BY = ("download", "dots", "ritz", "clone", "reserve", "clear")  # the run ends in the state of an undisturbed one


@pytest.mark.parametrize("reader", cases.READERS)
@pytest.mark.parametrize("case", list(cases.CASES))
def test_a_reader_between_two_batches(runs, case, reader):
    """each kind of call on a pending state, stepping on behind it: its result and the final state are those of the eager run"""
    lazy, eager = _need(runs, "default", "eager")
    key = "%s/read_%s/" % (case, reader)
    assert bool(lazy[key + "pending_before"]) and not bool(eager[key + "pending_before"])
    assert not eager[key + "pending_after"].any()
    assert (lazy[key + "pending_after"] == PENDING_AFTER.get(reader, False)).all()
    _same_prefix(lazy, eager, key)
    if reader in UNCHANGED_BY:
        _same_state(lazy, key, lazy, "%s/sched_whole/" % case, reader)
    if reader == "clone":
        _same_state(lazy, key + "copy_", lazy, key, "the copy")
    if reader in ("restart", "configure", "update"):  # the reader did change the course of the run
        assert not np.array_equal(lazy[key + "W"], lazy["%s/sched_whole/W" % case])


def test_the_closing_bytes_are_saved(runs):
    """one-call batches with the profile on: the run books the full sweeps under K_UPDATE, sum 8 N (k + 4), and no more; the flag
    reads 1 behind each batch and 0 behind a download, which books the one closing pass, 8 N (k + 3); the eager run books all"""
    lazy, eager = _need(runs, "default", "eager")
    key = "lap17/bytes/"
    n, s = (int(v) for v in lazy[key + "n_steps"])
    sweeps = sum(8.0 * n * (k + 4) for k in range(s))
    closes = [8.0 * n * (k + 3) for k in range(s)]
    print("K_UPDATE bytes: default %.0f (+ %.0f behind the download), eager %.0f; sweeps %.0f, closing passes %.0f"
          % (lazy[key + "update_bytes"], lazy[key + "update_bytes_after_download"] - lazy[key + "update_bytes"], eager[key + "update_bytes"],
             sweeps, sum(closes)))
    assert float(lazy[key + "update_bytes"]) == sweeps
    assert lazy[key + "pending_after_batch"].all() and not bool(lazy[key + "pending_after_download"])
    assert float(lazy[key + "update_bytes_after_download"]) == sweeps + closes[-1]
    assert float(eager[key + "update_bytes"]) == sweeps + sum(closes)
    assert not eager[key + "pending_after_batch"].any()
    assert float(eager[key + "update_bytes_after_download"]) == sweeps + sum(closes)


@pytest.mark.parametrize("case", list(cases.CASES))
def test_recorded_batches(runs, case):
    """batches of >= 4 calls repeated from the same state with a clear in between (recorded, then replayed): the bits of plain launches"""
    lazy, eager, plain = _need(runs, "default", "eager", "no_graphs")
    assert int(lazy[case + "/graphs/count"]) >= 1 and int(plain[case + "/graphs/count"]) == 0
    for rep in range(3):
        for name, d in (("default", lazy), ("eager", eager), ("no_graphs", plain)):
            _same_state(d, "%s/graphs_%d/" % (case, rep), plain, case + "/graphs_0/", "%s, run %d" % (name, rep))
    _same_state(lazy, case + "/graphs_0/", lazy, case + "/sched_whole/", "three batches and one")


def test_a_batch_cut_behind_an_armed_repair(runs):
    """diag(1..60), five entries 1 and the rest 1e-11: the guard arms a repair; a batch that ends with that very call"""
    lazy, eager = _need(runs, "default", "eager")
    armed = int(lazy["guard/armed_after_calls"])
    print("the repair counter first moved behind call", armed)
    assert 0 < armed < cases.GUARD_CALLS and armed == int(eager["guard/armed_after_calls"])
    assert bool(lazy["guard/cut/pending"]) and not bool(eager["guard/cut/pending"])
    assert int(lazy["guard/cut/repairs_at_cut"]) >= 1
    _same_prefix(lazy, eager, "guard/")
    for sched in ("ones", "cut"):
        _same_state(lazy, "guard/%s/" % sched, lazy, "guard/whole/", sched)
    assert lazy["guard/whole/state"][6] >= 1 and lazy["guard/whole/state"][0] == cases.GUARD_CALLS
