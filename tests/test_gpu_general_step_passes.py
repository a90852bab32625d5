"""Krylov steps whose Gram-Schmidt passes run over a general column set, step by step: every Lanczos or Arnoldi step that is not the
one-sweep step goes through enq_orthogonalize (library.hip), and with orthogonalizing vectors, a re-orthogonalisation interval
other than 1, complex data, several shards or a scheme other than the batched one k_dots and k_update (kernels.hip) sweep
first / stride / count basis columns followed by nq orthogonalizing vectors.  The pass-mode suites (tests/test_gpu_spin_krylov_passes.py,
tests/test_gpu_layout_krylov_passes.py) hold the steps with "every column, stride 1, nq = 0"; the general sets had trajectory tests
against a real-valued oracle only.

Every case of tests/general_step_cases.py makes its calls with the runners of tests/krylov_pass_runs.py (the orthogonalizing
vectors go up as VEC_ORTHO(q) before the start vector), downloads the state and gives it to the general local check of
tests/krylov_local_reference.py: every step from the stored columns in extended precision, with the column set restated
(lanczos_columns), the scheme's form (one classical pass, two, one vector after another, the second pass exactly when
|r_1|^2 < 0.5 |hu|^2), column 0 against the deflated start vector, within

    (n + k + nq) eps (|H|_1 + |shift|) max(1, sum_i |c_i| / |w0|_2)      per step
    (n + nq) eps |x0|_2                                                    for column 0

and max |U^H U - I|, max |Q^H U| <= (n + k) eps where the scheme promises orthogonality.  tests/test_general_step_reference_host.py
holds the fp64 recurrence of every case to a tenth of that and shows that every number-only fault that applies to a case (a column
set moved by one, the orthogonalizing vectors on the wrong steps or in the wrong order, a dropped conjugate, a second pass left out
or a decision taken with 0.25, two coefficients exchanged across the boundary of a chunk, a start vector not deflated) is a hundred
times outside it.

Also: the counters and series lengths; no repair and no pending close on a real one-shard Lanczos case (the one-sweep step was not
taken); a second schedule of batches, (1, 3, 4) instead of one captured batch of 8 (1, 3 and the rest of 10 or 24), gives the same
bytes in every series and every column wherever the library promises it (not across the ends of batches with a fused alpha
between shards); the adaptive Arnoldi cases took and skipped their second pass at least twice each, by the device's own columns.

Measured ratios per case family, the seeded device faults and the time beside tests/test_gpu_layout_krylov_passes.py:
profiles/general_step_passes.md."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import general_step_cases as gc  # noqa: E402
import krylov_local_reference as kl  # noqa: E402
from krylov_pass_runs import arnoldi, lanczos  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    from cmpt_eigenex_amd import capi

    assert capi.device_count() >= 1
    return capi


class _Handles:
    """contexts by shards and operators by (shards, op, n, layout), built once for the module; every state a case creates is
    registered here and closed before its operator and its context"""

    def __init__(self, capi):
        self.capi, self.ctxs, self.ops, self.bases = capi, {}, {}, []

    def ctx(self, shards):
        if shards not in self.ctxs:
            self.ctxs[shards] = self.capi.Context(loopback_shards=shards) if shards > 1 else self.capi.Context()
        return self.ctxs[shards]

    def op(self, c):
        key = (c["shards"], c["op"], c["n"], c["layout"])
        if key not in self.ops:
            A = gc.upload(self.capi, self.ctx(c["shards"]), c)
            assert bool(getattr(A, "is_complex", False)) == gc.is_complex(c["op"])
            if c["layout"] == "plain":
                assert (A.layout(), A.encoding(), A.column_blocks()) == ("csr", "plain", 1), (key, A.layout(), A.encoding(), A.column_blocks())
            print(f"operator {key}: layout {A.layout()}, encoding {A.encoding()}, column blocks {A.column_blocks()}")
            self.ops[key] = A
        return self.ops[key]

    def register(self, b):
        self.bases.append(b)

    def close_bases(self):
        for b in self.bases:
            b.close()
        self.bases.clear()

    def close(self):
        self.close_bases()
        for A in self.ops.values():
            A.close()
        for c in self.ctxs.values():
            c.close()


@pytest.fixture(scope="module")
def handles(mods):
    h = _Handles(mods)
    yield h
    h.close()


@pytest.fixture(autouse=True)
def _states_closed(handles):
    yield
    handles.close_bases()  # also when the test failed: basis, then (at the end of the module) operator, then context


def _run(handles, c, batches):
    capi = handles.capi
    _, x0, Q = gc.inputs(c)

    def prepare(b):
        handles.register(b)
        for q in range(c["nq"]):
            b.upload(capi.VEC_ORTHO(q), Q[q])

    run = lanczos if c["kind"] == "lanczos" else arnoldi
    got, b = run(capi, handles.ctx(c["shards"]), handles.op(c), c["n"], x0, batches, c["shift"], getattr(capi, c["mode"]), c["calls"] + 1,
                 prepare=prepare, interval=c["interval"], n_ortho=c["nq"], fusion=c["fusion"])
    if c["kind"] == "lanczos":
        got["w"], got["v"] = b.download(capi.VEC_W), b.download(capi.VEC_V)
    return got


def _counters(c, got):
    calls = c["calls"]
    if c["kind"] == "lanczos":
        assert got["state"] == (calls, calls - 1, 0) and got["lengths"] == (calls, calls - 1), (c["name"], got["state"], got["lengths"])
        if c["shards"] == 1 and not gc.is_complex(c["op"]):
            assert got["repairs"] == 0 and not got["pending"], c["name"]  # the one-sweep step was not taken
    else:
        assert got["state"][0] == calls and got["state"][2] == 0 and got["lengths"][0] == calls, (c["name"], got["state"], got["lengths"])


def _case(handles, c):
    t0 = time.perf_counter()
    got = _run(handles, c, (c["calls"],))
    t1 = time.perf_counter()
    _counters(c, got)
    rep = gc.check(c, got)
    print(rep.line(c["name"]))
    print(f"RATIO {c['name']} {rep.ratio():.3e} steps {rep['step_ratio']:.3e} start {rep['start_ratio']:.3e} "
          f"ortho {rep['ortho'] / rep['ortho_bound']:.3e} device {t1 - t0:.2f} s check {time.perf_counter() - t1:.2f} s")
    assert rep.ok(), rep.line(c["name"])
    if c["kind"] == "arnoldi" and c["mode"] == "ORTHO_BATCHED_ADAPTIVE" and not c["budget"]:
        d = np.array(rep["decisions"], np.float64)
        print(f"{c['name']}: |r_1|^2 / |hu|^2 per step {np.array2string(d, precision=4)}")
        assert np.count_nonzero(d < kl.ETA2) >= 2 and np.count_nonzero(d > kl.ETA2) >= 2 and np.abs(d - kl.ETA2).min() > 1e-3
    if c["split"]:
        handles.close_bases()
        again = _run(handles, c, c["split"])
        _counters(c, again)
        for key in ("U", "alpha", "beta", "w", "v") if c["kind"] == "lanczos" else ("U", "H", "residue", "w"):
            assert np.asarray(got[key]).tobytes() == np.asarray(again[key]).tobytes(), f"{c['name']}: {key} differs between the batches {(c['calls'],)} and {c['split']}"


STEP_CASES = [c["name"] for c in gc.CASES if not c["budget"]]
CHUNK_CASES = [c["name"] for c in gc.CASES if c["budget"]]


@pytest.mark.parametrize("name", STEP_CASES)
def test_general_steps_pass_the_local_check(handles, name):
    _case(handles, gc.BY_NAME[name])


@pytest.mark.parametrize("name", CHUNK_CASES)
def test_sets_beyond_one_dots_launch_pass_the_local_check(handles, name):
    """a set of more accumulators than one k_dots launch keeps in LDS is swept in chunks (library.hip: for_each_chunk): the set
    crosses the budget during the run, the head chunk carries the inline alpha (real, one shard) or the decision of the adaptive
    second pass, the two-source k_dots of the fused alpha has half the budget, and the chunk at the boundary holds basis columns
    (strided with interval 3) and orthogonalizing vectors"""
    _case(handles, gc.BY_NAME[name])
