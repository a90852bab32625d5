"""The numpy restatement of SpinTimeCorrelationSolver (tests/spin_time_correlation_reference.py) against dense exponentials, on
the CPU: at the tolerance and Krylov dimension of tests/test_gpu_spin_time_correlation.py every value stays within the
restatement's own bound plus its excess at tol = 1e-13, so the bound's formula and the quadrature behind it are right before the
device is held to them.  Also the operators of the cases against the longdouble restatement of spin_site_z_reference.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spin_dynamics_reference as dr  # noqa: E402
import spin_site_z_reference as zr  # noqa: E402
import spin_time_correlation_reference as tr  # noqa: E402


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g

    g.build()
    from cmpt_eigenex_amd import capi as c

    return c


@pytest.mark.parametrize("name", ["neel", "ring", "ring eigen"])
def test_restatement_stays_within_its_bound(capi, name):
    case = tr.case(capi, name)
    excess = tr.excess(case)
    r = case.restatement(tr.M, tr.TOL)
    assert np.all(np.abs(r.values() - case.dense_values(0.0)) <= 1e-15)
    worst = worst_bound = 0.0
    for k in range(tr.CALLS):
        r.evolve(tr.DT)
        err, bound = np.abs(r.values() - case.dense_values(tr.DT * (k + 1))), r.bounds()
        worst, worst_bound = max(worst, float(err.max())), max(worst_bound, float(bound.max()))
        assert r.eps_psi <= (k + 1) * tr.TOL and r.eps_phi <= (k + 1) * tr.TOL
        assert np.all(err <= bound + excess + r.applications * tr.EPS * case.norms * case.source_norm)
    print(f"{name}: worst error {worst:.2e}, largest bound {worst_bound:.2e}, excess at tol = 1e-13 {excess:.2e}, applications {r.applications}")
    if name != "neel":  # the eigenstate breaks down at once: psi takes one operator application per call and no error
        assert r.eps_psi == 0.0


def test_operators_of_the_cases_are_the_state_list_restatement(capi):
    L, n_up = 10, 5
    c = tr.momentum_z(L, 2 * np.pi * 3 / 10)
    for kind in (dr.Z, dr.MINUS, dr.PLUS):
        want = zr.site_matrix(capi, L, n_up, kind, c.real).astype(np.float64) + 1j * zr.site_matrix(capi, L, n_up, kind, c.imag).astype(np.float64)
        assert np.allclose(tr.operator(capi, L, n_up, kind, c), want, rtol=0, atol=1e-15)
    assert abs(np.sum(np.abs(c) ** 2) - 1.0) < 1e-15 and tr.norm_bound(dr.Z, c) == 0.5 * tr.norm_bound(dr.MINUS, c)
