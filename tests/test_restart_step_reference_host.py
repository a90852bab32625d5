"""The cases of tests/restart_step_cases.py on the host: what makes the assertions of tests/test_gpu_restart_steps.py fair, and what
shows that they can fail.  No GPU.

For every case the fp64 recurrence of tests/krylov_local_reference.py (thick_restart_fp64, krylov_schur_fp64) passes, in every
cycle, the three checks of a restarted state at a ratio of at most 0.1: the local step check from first = nkeep with its unchanged
bound (orthogonality of all columns included), the kept relation, and the combination check of tests/ritz_reference.py with its own
bound.  An input on which it comes nearer would be replaced, not tolerated.

For every fault that applies to a case (restart_step_cases.applicable_faults) the faulty fp64 state fails at a ratio of at least
100; every fault of kl.RESTART_FAULTS has a case and no case is without a fault.  The recurrence does not depend on the shards or
the fused alpha, so the cases that differ only in those share one run (restart_step_cases.REFERENCES).

first = 0 reproduces check_lanczos and check_arnoldi exactly on an unrestarted state.  Measured ratios: profiles/restart_steps.md."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import krylov_local_reference as kl  # noqa: E402
import restart_step_cases as rc  # noqa: E402

ROOM = 0.1    # a reference recurrence that uses more than a tenth of a bound means another input
CAUGHT = 100  # a fault must be this far outside a bound
REFS = [c["name"] for c in rc.REFERENCES.values()]


@pytest.mark.parametrize("name", REFS)
def test_fp64_recurrence_passes_with_room(name):
    c = rc.BY_NAME[name]
    cycles = rc.reference(c)
    assert len(cycles) == 1 + c["cycles"]
    for i, cy in enumerate(cycles[1:], 1):
        r = rc.check_cycle(c, cy)
        print("HOST RATIO " + rc.line(name, i, r))
        assert cy["U"].shape[0] == rc.M + (c["kind"] == "lanczos"), (name, i, cy["U"].shape)  # no breakdown: every call made a column
        assert r["step"].ok() and r["kept"].ok() and r["worst"] <= ROOM, rc.line(name, i, r)


PAIRS = [(c["name"], f) for c in rc.REFERENCES.values() for f in c["faults"]]


@pytest.mark.parametrize("name,fault", PAIRS, ids=[f"{n}-{f}" for n, f in PAIRS])
def test_fault_is_caught(name, fault):
    c = rc.BY_NAME[name]
    cy = rc.reference(c, fault)[1]  # the first restart shows it
    r = rc.check_cycle(c, cy)
    print(f"FAULT RATIO {fault} " + rc.line(name, 1, r))
    assert r["worst"] >= CAUGHT, rc.line(f"{name} with {fault}", 1, r)


def test_every_fault_has_a_case_and_every_case_a_fault():
    assert {f for c in rc.CASES for f in c["faults"]} == set(kl.RESTART_FAULTS)
    assert all(c["faults"] for c in rc.CASES)
    assert all(rc.reference_key(c) in rc.REFERENCES and rc.REFERENCES[rc.reference_key(c)]["faults"] == c["faults"] for c in rc.CASES)


def test_the_dropped_column_carries_weight():
    """last_basis_column_dropped shows only where |C[m - 1, e]| is not negligible for a kept e: the dropped term is that times an
    entry of a unit vector, against a bound of about 32 u times such an entry, so that 0.01 is thirteen orders of magnitude clear.
    Held here for every reference (the lowest Ritz vector alone, nkeep = 1, has 0.036; seven or more have above 0.2)."""
    for c in rc.REFERENCES.values():
        cy = rc.reference(c)[1]
        last = np.abs((cy["S"] if c["kind"] == "lanczos" else cy["Q"])[rc.M - 1])
        print(f"{c['name']}: max |C[m-1, e]| = {last.max():.3e}")
        assert last.max() >= 0.01, c["name"]


def test_the_table_holds_the_required_axes():
    have = lambda cs, **kw: any(all(c[k] == v for k, v in kw.items()) for c in cs)  # noqa: E731
    for scheme in ("front", "batched", "seq", "adaptive"):
        for cplx in (False, True):
            for nkeep in (7, 17):
                for shards, fusion in rc.SHARDINGS:
                    assert have(rc.LANCZOS_GRID, scheme=scheme, cplx=cplx, nkeep=nkeep, shards=shards, fusion=fusion)
    for nkeep in (1, rc.M):
        assert have(rc.LANCZOS_EDGES, nkeep=nkeep, cplx=False, shards=1) and have(rc.LANCZOS_EDGES, nkeep=nkeep, cplx=True, shards=3)
    for cplx in (False, True):
        assert have(rc.LANCZOS_SHIFT, cplx=cplx, shift=rc.SHIFT)
        for shards in (1, 3):
            assert have(rc.LANCZOS_CYCLES, cplx=cplx, shards=shards, cycles=3, nkeep=7) and have(rc.ARNOLDI_CYCLES, cplx=cplx, shards=shards, cycles=3)
    for cplx, keeps, shifts in ((False, (7, 17), (0.0,)), (True, (3, 9), (0.0, rc.SHIFT_Z))):
        for nkeep in keeps:
            for scheme in ("default", "adaptive"):
                for shards in (1, 3):
                    for shift in shifts:
                        assert have(rc.ARNOLDI_GRID, cplx=cplx, nkeep=nkeep, scheme=scheme, shards=shards, shift=shift)


def test_first_zero_reproduces_the_existing_checks():
    for cplx in (False, True):
        rows, x = rc.inputs("lanczos", cplx)
        a, b, V = kl.lanczos_fp64(kl.csr_matmul(rows), x, 7, -0.3)
        assert dict(kl.check_lanczos(rows, -0.3, V, a, b, first=0)) == dict(kl.check_lanczos(rows, -0.3, V, a, b))
        skipped = kl.check_lanczos(rows, -0.3, V, a, b, first=8)  # no step left: orthogonality and the bound stay
        assert skipped.worst() == 0.0 and skipped["ortho"] == kl.check_lanczos(rows, -0.3, V, a, b)["ortho"] > 0.0
        rows, x = rc.inputs("arnoldi", cplx)
        V, H, residue, w = kl.arnoldi_fp64(kl.csr_matmul(rows), x, 8, rc.SHIFT_Z if cplx else rc.SHIFT, 2)
        old = kl.check_arnoldi(rows, rc.SHIFT_Z if cplx else rc.SHIFT, V, H, residue, w)
        assert dict(kl.check_arnoldi(rows, rc.SHIFT_Z if cplx else rc.SHIFT, V, H, residue, w, first=0)) == dict(old) and old.ok()


def test_breakdown_inputs_span_twelve_dimensions():
    rows, x = rc.breakdown_inputs()
    assert np.count_nonzero(x) == np.count_nonzero(rows[2]) == rc.BREAK_D == np.unique(rc.BREAK_VALUES).size
    assert set(rc.BREAK_ROWS // 2048) == {0, 1, 2} and np.array_equal(np.flatnonzero(x), rc.BREAK_ROWS)
