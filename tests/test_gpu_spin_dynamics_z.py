"""SpinDynamicsSolver's complex run (spin_dynamics.hpp: computeStructureFactorZSingleRun, setSiteOperator with complex
coefficients, setState with a complex vector) against dense diagonalisation: the 12-site Heisenberg ring in (12,6), Sz_q =
L^{-1/2} sum_r e^{iqr} Sz_r at q = 2 pi k / 12, k = 1, 5, 6, weights |<n| Sz_q |psi>|^2 from numpy.  Moments 0..3 to
dr.MOMENT_TOL of sum w |p|^k, the spectrum at dr.ETA on dr.OMEGA to dr.SPECTRUM_TOL of its maximum, and totalWeight() to
MOMENT_TOL of the two-run computeStructureFactorZ(q).  A numpy complex Lanczos fraction of 60 steps meets these on the same
cases with 1e-14 (spectra) and 1e-14 (moments), so a failure here is the device's.  NOT part of the reference project."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spin_dynamics_reference as dr  # noqa: E402

pytestmark = pytest.mark.gpu
L, N_UP, STEPS = 12, 6, 60


@pytest.fixture(scope="module")
def mods():
    from cmpt_eigenex_amd import capi, solver

    assert capi.device_count() >= 1
    return capi, solver


@pytest.fixture(scope="module")
def ring12(mods):
    """levels and vectors of the ring's (12,6) matrix, computed once; Sz_q keeps the sector"""
    capi, _ = mods
    E, V = np.linalg.eigh(dr.hamiltonian(capi, dr.ring(L), N_UP))
    return E, V


def _dense(mods, ring12, q):
    """(poles, weights) of Szz(q, w) of the ground state"""
    capi, _ = mods
    E, V = ring12
    c, s = dr.sz_q(L, q)
    phi = (dr.site_operator(capi, L, N_UP, dr.Z, c) + 1j * dr.site_operator(capi, L, N_UP, dr.Z, s)) @ V[:, 0]
    return E - E[0], np.abs(V.T @ phi) ** 2


def _solver(mods, ctx, psi):
    _, solver = mods
    n, bonds, hz, hx = dr.ring(L)
    return solver.SpinDynamicsSolver().setModel(ctx, n, bonds, hz, hx, N_UP).setState(psi).setLanczosSteps(STEPS)


@pytest.mark.parametrize("k", [1, 5, 6])
def test_single_run_structure_factor_against_dense_diagonalisation(mods, ring12, k):
    capi, _ = mods
    q = 2 * np.pi * k / L
    poles, weights = _dense(mods, ring12, q)
    ctx = capi.Context()
    sd = _solver(mods, ctx, 1.5 * ring12[1][:, 0]).computeStructureFactorZSingleRun(q)  # not normalised: the solver divides by <v|v>
    r = sd.results()
    assert r["info_name"] == "Success", sd.log()
    assert 1 <= r["npoles"] <= STEPS and r["nalpha"] == r["npoles"]  # ONE fraction
    assert abs(r["stateEnergy"] - ring12[0][0]) <= 1e-12 * abs(ring12[0][0]) and abs(r["stateNormSquared"] - 2.25) < 1e-12
    assert np.all(np.diff(r["poles"]) >= 0) and np.all(r["weights"] >= 0)
    for j in range(4):
        dense, scale = float(np.sum(weights * poles ** j)), float(np.sum(weights * np.abs(poles) ** j))
        err = abs(sd.moment(j) - dense) / scale
        print(f"k = {k}: moment {j} = {sd.moment(j)!r}, dense {dense!r}, relative error {err:.2e}")
        assert err <= dr.MOMENT_TOL
    ref = dr.lorentzians(poles, weights, dr.OMEGA, dr.ETA)
    err = float(np.max(np.abs(sd.spectrum(dr.OMEGA, dr.ETA) - ref)) / ref.max())
    print(f"k = {k}: spectrum error / maximum {err:.2e}, poles {r['npoles']}")
    assert err <= dr.SPECTRUM_TOL
    single = r["totalWeight"]
    two = sd.computeStructureFactorZ(q).results()  # the same solver goes back to the real run
    assert two["info_name"] == "Success", sd.log()
    print(f"k = {k}: total weight {single!r}, of the two real runs {two['totalWeight']!r}")
    assert abs(single - two["totalWeight"]) <= dr.MOMENT_TOL * two["totalWeight"] and single > 1e-3
    again = sd.computeStructureFactorZSingleRun(q).results()  # and forth: the same bits
    assert again["totalWeight"] == single and np.array_equal(again["poles"], r["poles"]) and np.array_equal(again["weights"], r["weights"])
    sd.close()
    ctx.close()


def test_complex_coefficients_and_complex_states_through_compute(mods, ring12):
    """setSiteOperator with the complex coefficients of Sz_q gives the moments of computeStructureFactorZSingleRun(q); a complex state
    e^{i a} psi gives the same response within MOMENT_TOL (a phase of the state leaves |<n|O|psi>|^2 alone); real coefficients
    handed over as complex ones give the real run's moments."""
    capi, _ = mods
    q = 2 * np.pi * 5 / L
    c, s = dr.sz_q(L, q)
    psi = ring12[1][:, 0]
    ctx = capi.Context()
    sd = _solver(mods, ctx, psi)
    want = sd.computeStructureFactorZSingleRun(q).results()
    want_moments = [sd.moment(j) for j in range(4)]
    got = sd.setSiteOperator(dr.Z, c + 1j * s).compute().results()  # numpy's coefficients: the last bit of some differs from the solver's
    assert got["info_name"] == "Success" and got["npoles"] == want["npoles"]
    for j in range(4):
        assert abs(want_moments[j] - sd.moment(j)) <= dr.MOMENT_TOL * abs(want_moments[j])
    turned = sd.setState(np.exp(0.7j) * psi).compute().results()
    assert turned["info_name"] == "Success", sd.log()
    moments = [sd.moment(j) for j in range(4)]
    sd.setState(psi).setSiteOperator(dr.Z, c + 1j * s).compute()
    for j in range(4):
        assert abs(moments[j] - sd.moment(j)) <= dr.MOMENT_TOL * abs(sd.moment(j))
    real = sd.setSiteOperator(dr.Z, c).compute().results()
    real_moments = [sd.moment(j) for j in range(4)]
    as_complex = sd.setSiteOperator(dr.Z, c + 0j).compute().results()
    assert as_complex["info_name"] == "Success" and abs(as_complex["totalWeight"] - real["totalWeight"]) <= dr.MOMENT_TOL * real["totalWeight"]
    for j in range(4):
        assert abs(real_moments[j] - sd.moment(j)) <= dr.MOMENT_TOL * abs(real_moments[j])
    # q = 0: the total Sz annihilates the sector's states: no weight, no poles, Success
    zero = sd.computeStructureFactorZSingleRun(0.0).results()
    assert zero["info_name"] == "Success" and zero["totalWeight"] == 0.0 and zero["npoles"] == 0, sd.log()
    bad = sd.setSiteOperator(dr.Z, np.array([complex(0.0, np.inf)] + [0j] * (L - 1))).compute().results()
    assert bad["info_name"] == "InvalidInput" and any("not finite" in l for l in sd.log())
    sd.close()
    ctx.close()


def test_the_two_run_structure_factor_refuses_a_complex_state(mods, ring12):
    """computeStructureFactorZ(q) is the sum of a cos and a sin run, which holds for real states only: after setState(real) and
    then setState(complex) it must not answer for the earlier real state; it is refused and logged, with or without a real state
    set before, and answers again once a real state is set."""
    capi, solver = mods
    q = 2 * np.pi * 5 / L
    psi, other = ring12[1][:, 0], ring12[1][:, 3]
    ctx = capi.Context()
    sd = _solver(mods, ctx, psi)
    want = sd.computeStructureFactorZ(q).results()
    assert want["info_name"] == "Success"
    r = sd.setState(np.exp(0.3j) * other).computeStructureFactorZ(q).results()
    assert r["info_name"] == "InvalidInput" and r["npoles"] == 0 and r["totalWeight"] == 0.0
    assert any(l.startswith("ERROR") and "needs a real state" in l and "computeStructureFactorZSingleRun" in l for l in sd.log())
    assert sd.computeStructureFactorZSingleRun(q).results()["info_name"] == "Success"  # the complex state's own call
    fresh = solver.SpinDynamicsSolver().setModel(ctx, *dr.ring(L), n_up=N_UP).setLanczosSteps(STEPS).setState(psi + 0j)
    assert fresh.computeStructureFactorZ(q).results()["info_name"] == "InvalidInput" and any("needs a real state" in l for l in fresh.log())
    again = sd.setState(psi).computeStructureFactorZ(q).results()
    assert again["info_name"] == "Success" and again["totalWeight"] == want["totalWeight"] and np.array_equal(again["poles"], want["poles"])
    for h in (sd, fresh, ctx):
        h.close()
