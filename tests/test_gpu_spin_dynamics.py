"""SpinDynamicsSolver (spin_dynamics.hpp) on the device against dense diagonalisation (tests/spin_dynamics_reference.py: numpy
eigh of the sector matrices from eigenex_spin_sector_csr, w_n = |<n|O|psi>|^2).  The first 2m moments of an m-step continued
fraction are exact in exact arithmetic (Gauss quadrature), so moment(k), k = 0..3, agrees to 1e-10 of sum w_n |p_n|^k, the
project's asserted tolerance for Ritz values; spectrum(w, eta = 0.1) on 141 points of [-1, 6] agrees to 1e-9 of the dense
spectrum's maximum (a pole error of 1e-10 divided by eta) where the fraction is converged or complete.  The numpy continued
fraction of the reference module meets the same tolerances on the same cases in tests/test_spin_site_host.py (2e-15 .. 6e-15 on
the moments, 2e-15 .. 2e-14 on the spectra), so a failure here is the device's.  Then the sum rules and the C++ program.
NOT part of the reference project."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spin_dynamics_reference as dr  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mods():
    from cmpt_eigenex_amd import capi, solver

    assert capi.device_count() >= 1
    return capi, solver


@pytest.fixture(scope="module")
def ring12(mods):
    """the ground state of the 12-site Heisenberg ring in (12,6) and its exact Szz(pi, w), computed once"""
    capi, _ = mods
    return dr.Dense(capi, dr.ring(12), 6, [(dr.Z, dr.sz_q(12, np.pi)[0])])


def _solver(mods, ctx, model, n_up, psi, m):
    _, solver = mods
    L, bonds, hz, hx = model
    return solver.SpinDynamicsSolver().setModel(ctx, L, bonds, hz, hx, n_up).setState(psi).setLanczosSteps(m)


@pytest.mark.parametrize("name", sorted(dr.moment_cases()))
def test_moments_against_dense_diagonalisation(mods, name):
    capi, _ = mods
    model, n_up, parts, m = dr.moment_cases()[name]
    dense = dr.Dense(capi, model, n_up, parts)
    (kind, coef), = parts
    ctx = capi.Context()
    sd = _solver(mods, ctx, model, n_up, 1.5 * dense.psi, m).setSiteOperator(kind, coef).compute()  # not normalised: the solver divides by <v|v>
    r = sd.results()
    assert r["info_name"] == "Success", sd.log()
    assert r["npoles"] == m == r["nalpha"] and r["nbeta"] == m - 1
    assert abs(r["stateEnergy"] - dense.E0) <= 1e-12 * max(1.0, abs(dense.E0)) and abs(r["stateNormSquared"] - 2.25) < 1e-12
    assert np.all(np.diff(r["poles"]) >= 0) and np.all(r["weights"] >= 0)
    for k in range(4):
        err = abs(sd.moment(k) - dense.moment(k)) / dense.moment_scale(k)
        print(f"{name}: moment {k} = {sd.moment(k)!r}, dense {dense.moment(k)!r}, relative error {err:.2e}")
        assert err <= dr.MOMENT_TOL
    assert abs(r["totalWeight"] - dense.moment(0)) <= dr.MOMENT_TOL * dense.moment(0)
    sd.close()
    ctx.close()


@pytest.mark.parametrize("name", sorted(dr.spectrum_cases()))
def test_spectrum_against_dense_diagonalisation(mods, ring12, name):
    capi, _ = mods
    model, n_up, parts, m = dr.spectrum_cases()[name]
    dense = ring12 if name.startswith("ring (12,6)") else dr.Dense(capi, model, n_up, parts)
    (kind, coef), = parts
    ctx = capi.Context()
    sd = _solver(mods, ctx, model, n_up, dense.psi, m)
    if name.startswith("ring"):
        sd.setStateEnergy(dense.E0).computeStructureFactorZ(np.pi)  # the sin part, sin(pi i) ~ 1e-16, carries nothing
    else:
        sd.setSiteOperator(kind, coef).compute()
    r = sd.results()
    assert r["info_name"] == "Success", sd.log()
    ref = dense.spectrum(dr.OMEGA, dr.ETA)
    got = sd.spectrum(dr.OMEGA, dr.ETA)
    err = float(np.max(np.abs(got - ref)) / ref.max())
    heavy = r["poles"][r["weights"] > 1e-12 * r["weights"].sum()]
    print(f"{name}: spectrum error / maximum {err:.2e}; lowest pole {heavy.min():.6f}, dense {dense.lowest_pole():.6f}; poles {r['npoles']}")
    assert err <= dr.SPECTRUM_TOL
    assert abs(heavy.min() - dense.lowest_pole()) <= dr.MOMENT_TOL * max(1.0, abs(dense.lowest_pole()))
    if name.startswith("ring"):  # the lowest pole at q = pi is the triplet gap: the lowest level of (L, L/2 + 1), a triplet's Sz = 1
        up = np.linalg.eigvalsh(dr.hamiltonian(capi, model, n_up + 1))[0]
        assert abs(heavy.min() - (up - dense.E0)) <= 1e-9
    if "complete" in name:  # m = the destination's dimension: every pole of the dense response, one by one
        assert r["npoles"] <= m
        big = dense.weights > 1e-9 * dense.weights.sum()
        for p in dense.poles[big]:
            assert np.min(np.abs(r["poles"] - p)) <= 1e-9
    sd.close()
    ctx.close()


def test_sum_rules_of_the_structure_factor(mods, ring12):
    """totalWeight() of computeStructureFactorZ(q) is the static structureFactorZ(q) of SpinCorrelationSolver: both are sums of at
    most L^2 = 144 products of O(1), 144 * 2^-52 with a factor of 30 for the two summation orders stays below 1e-12.  At q = 0
    the operator is the total Sz / sqrt(L), which annihilates a state of the sector Sz = 0: no weight, no poles."""
    capi, _ = mods
    ctx = capi.Context()
    sd = _solver(mods, ctx, dr.ring(12), 6, ring12.psi, 40)
    for q in (np.pi, np.pi / 2, 2 * np.pi / 12):
        sd.computeStructureFactorZ(q)
        r = sd.results()
        static = sd.staticStructureFactorZ(q)
        print(f"q = {q:.6f}: total weight {r['totalWeight']!r}, static {static!r}, difference {abs(r['totalWeight'] - static):.2e}, poles {r['npoles']}")
        assert r["info_name"] == "Success" and abs(r["totalWeight"] - static) <= 1e-12 and static > 1e-3
        assert abs(r["weights"].sum() - r["totalWeight"]) <= 1e-12
    sd.computeStructureFactorZ(0.0)
    r = sd.results()
    assert r["info_name"] == "Success" and r["totalWeight"] == 0.0 and r["npoles"] == 0, sd.log()
    assert abs(sd.staticStructureFactorZ(0.0)) <= 1e-12
    sd.close()
    ctx.close()


def test_su2_on_the_singlet(mods, ring12):
    """<S+ S-> = 2 <Sz Sz> on a singlet: the MINUS response with c = L^{-1/2} cos(pi i) has twice the Z response's total weight,
    and their lowest poles agree (the Sz = -1 and Sz = 0 members of the same triplet)"""
    capi, _ = mods
    ctx = capi.Context()
    c = dr.sz_q(12, np.pi)[0]
    sd = _solver(mods, ctx, dr.ring(12), 6, ring12.psi, 60).setStateEnergy(ring12.E0)
    rz = sd.setSiteOperator(dr.Z, c).compute().results()
    rm = sd.setSiteOperator(dr.MINUS, c).compute().results()
    rp = sd.setSiteOperator(dr.PLUS, c).compute().results()
    lowest = [r["poles"][r["weights"] > 1e-12 * r["weights"].sum()].min() for r in (rz, rm, rp)]
    print(f"total weights {rz['totalWeight']!r}, {rm['totalWeight']!r}, {rp['totalWeight']!r}; lowest poles {lowest}")
    for r in (rm, rp):
        assert r["info_name"] == "Success" and abs(r["totalWeight"] - 2 * rz["totalWeight"]) <= 1e-10
    assert abs(lowest[1] - lowest[0]) <= 1e-10 and abs(lowest[2] - lowest[0]) <= 1e-10
    sd.close()
    ctx.close()


def test_invalid_input_is_logged_not_thrown(mods, ring12):
    capi, solver = mods
    ctx = capi.Context()
    sd = solver.SpinDynamicsSolver()
    assert sd.compute().results()["info_name"] == "InvalidInput" and any(l.startswith("ERROR") and "no model" in l for l in sd.log())
    sd.setModel(ctx, *dr.ring(12), n_up=6).setSiteOperator(dr.Z, np.ones(12))
    assert sd.setState(np.ones(5)).compute().results()["info_name"] == "InvalidInput" and any("one entry per row" in l for l in sd.log())
    assert sd.setState(np.zeros(924)).compute().results()["info_name"] == "InvalidInput" and any("state is zero" in l for l in sd.log())
    assert sd.setState(ring12.psi).setSiteOperator(dr.Z, np.ones(11)).compute().results()["info_name"] == "InvalidInput"
    assert sd.setSiteOperator(7, np.ones(12)).compute().results()["info_name"] == "InvalidInput"
    top = solver.SpinDynamicsSolver().setModel(ctx, *dr.ring(6), n_up=6).setState(np.ones(1)).setSiteOperator(dr.PLUS, np.ones(6))
    assert top.compute().results()["info_name"] == "InvalidInput" and any("leaves the sectors" in l for l in top.log())
    r = top.setSiteOperator(dr.MINUS, np.ones(6)).compute().results()  # and S- of it is a state of (6,5)
    assert r["info_name"] == "Success" and abs(r["totalWeight"] - 6.0) < 1e-12
    for h in (sd, top, ctx):
        h.close()


def test_cpp_program_spin_dynamics(tmp_path, ring12):
    """tests/cpp/spin_dynamics_amd.cpp: LanczosEigenSolver for the ground state of the ring (12,6), then SpinDynamicsSolver, in a
    C++11 user program built with -Wall -Wextra.  The lowest pole at q = pi is the triplet gap; the ground vector comes from a
    Lanczos run converged to 1e-13 in the eigenvalue, so the pole (first order in the vector's error) holds to 1e-6."""
    exe = str(tmp_path / "spin_dynamics_amd")
    lib = os.path.join(ROOT, "cmpt-eigenex_amd", "lib")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cmpt-eigenex_amd", "include"),
                           os.path.join(ROOT, "tests", "cpp", "spin_dynamics_amd.cpp"), "-o", exe, "-L", lib, "-leigenex_hip", "-Wl,-rpath," + lib])
    o = json.loads(subprocess.check_output([exe]).decode())
    print(o)
    assert o["info"] == 1 and o["sites"] == 12 and o["rows"] == 924
    assert abs(o["energy"] - ring12.E0) < 1e-9
    assert abs(o["lowest_pole"] - ring12.lowest_pole()) < 1e-6 and abs(o["total_weight"] - ring12.moment(0)) < 1e-6
    assert abs(o["total_weight"] - o["static_structure_factor"]) < 1e-12
    assert (o["refused_no_model"], o["refused_length"], o["refused_plus_from_full"], o["refused_zero"]) == (1, 1, 1, 1)
