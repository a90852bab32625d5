"""SpinTimeEvolutionSolver (spin_evolution.hpp) on the device, through solver.SpinTimeEvolutionSolver and through a C++11 user
program.

Closed form: two sites, Heisenberg J, |up down> in the sector (2,1): <Sz_0(t)> = cos(J t) / 2 to 1e-13; the Krylov space is the
whole sector, so errorBound() == 0.

Quenches against numpy.linalg.eigh of the dense matrix: the Neel state in the open XXZ chain (10,5), and every site up in the
full-space Ising chain of 8 sites with a transverse field; eight calls of evolve(0.25), m = 12, tol = 1e-9.  After each call
|psi_dev - psi_dense| <= sum of errorBound() + 10 floor and errorBound() <= tol, where floor is the rounding error of the numpy
restatement of the same algorithm (tests/spin_evolution_reference.py) run at tol = 1e-13 against the dense exponential, and the
factor 10 covers the device's different summation order.  Measured on the CPU: floor = 1.23e-13 for (10,5) and 6.24e-13 for the
Ising chain (at m = 12 a call is one sub-step whose bound of 1.5e-14 resp. 7.8e-14 the error saturates: the floor is mostly
truncation, eight calls of it); the restatement at tol = 1e-9 is within its own bound after every call.

Invariants at (20,10), m = 20, evolve(0.5).  Norm and energy are conserved by a Krylov step in exact arithmetic whatever its
truncation (|c| = 1 and c^H T c = e_1^T T e_1), so their drift is rounding alone, and the bound is the restatement's own drift on
(12,6), scaled by the operator-application counts A and by the factor 10 for the device's other summation order:
    |<psi|psi> - 1| <= 10 (A_dev / A_small) max(drift_small, eps)
    energy drift    <= 10 (A_dev / A_small) max(drift_small, eps |E_0|)
The restatement's drift is one sample of rounding noise and depends on the BLAS underneath numpy: measured on the CPU it was
1.3e-15 (norm) and 1.3e-15 (energy) after 20 applications on one machine, exactly 0 and 4.4e-16 on another.  Its smallest non-zero
value is one unit in the last place of the quantity measured, so that is its floor: eps for the norm of a unit vector, eps |E_0|
for the energy.  With A_dev = 22 the bounds are 1.5e-14 and 1.5e-14 with the first drifts, 2.4e-15 and 8.2e-15 with the second
(|E_0| = 3.34).  evolve(dt) followed by evolve(-dt) returns psi_0 within the two calls' errorBound() + 10 floor, floor = 3.1e-15 /
2.6e-15 being the restatement's distance from the dense exponential on (12,6) beyond its own bound."""
import json
import os
import subprocess
import sys
from math import comb

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spin_evolution_reference as er  # noqa: E402
import spin_measure_reference as mr  # noqa: E402
import spin_reference as sr  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def mods():
    from cmpt_eigenex_amd import capi, solver

    assert capi.device_count() >= 1
    return capi, solver


def test_two_sites_closed_form_is_exact(mods):
    capi, solver = mods
    ctx = capi.Context()
    J = 1.3
    te = solver.SpinTimeEvolutionSolver().setModel(ctx, 2, [(0, 1, J, J)], n_up=1).setProductState(0b01)
    assert te.info() == "Success" and te.overlapWithInitial() == 1.0 and te.time() == 0.0
    for k in range(1, 9):
        dt = -0.4 if k % 3 == 0 else 0.7
        assert te.evolve(dt) == 1 and te.info() == "Success"
        t = te.time()
        sz = te.magnetisation()
        print(f"t = {t:.2f}: <Sz_0> error {abs(sz[0] - 0.5 * np.cos(J * t)):.3e}, bound {te.errorBound()}")
        assert abs(sz[0] - 0.5 * np.cos(J * t)) <= 1e-13 and abs(sz[1] + 0.5 * np.cos(J * t)) <= 1e-13
        assert te.errorBound() == 0.0 and te.totalErrorBound() == 0.0
        assert abs(te.overlapWithInitial() - np.exp(0.25j * J * t) * np.cos(J * t / 2)) <= 1e-13
        assert abs(te.normSquared() - 1.0) <= 1e-14
    te.close()
    ctx.close()


def _solver(solver, ctx, name, m, tol):
    L, n_up, bonds, hz, hx, bits = er.QUENCHES[name]
    te = solver.SpinTimeEvolutionSolver().setModel(ctx, L, bonds, hz, hx, n_up=n_up)
    te.setKrylovDimension(m).setTolerance(tol).setProductState(bits)
    assert te.info() == "Success", te.log()
    return te


@pytest.mark.parametrize("name", list(er.QUENCHES))
def test_quench_against_the_dense_exponential(mods, name):
    capi, solver = mods
    H, psi0, dense = er.quench_reference(name)
    floor = er.quench_floor(name)
    # the restatement at the test's tolerance is within its own bound: the quadrature is right
    p = er.KrylovPropagator(H, psi0, er.QUENCH_M, er.QUENCH_TOL)
    total = 0.0
    for k in range(er.QUENCH_CALLS):
        p.evolve(er.QUENCH_DT)
        total += p.bound
        assert np.linalg.norm(p.psi - dense[k]) <= total + floor and p.bound <= er.QUENCH_TOL
    ctx = capi.Context()
    te = _solver(solver, ctx, name, er.QUENCH_M, er.QUENCH_TOL)
    assert np.array_equal(te.state(), psi0)
    total = 0.0
    for k in range(er.QUENCH_CALLS):
        steps = te.evolve(er.QUENCH_DT)
        assert steps >= 1 and te.info() == "Success", te.log()
        total += te.errorBound()
        err = float(np.linalg.norm(te.state() - dense[k]))
        print(f"{name} call {k}: {steps} sub-steps, error {err:.3e}, sum of bounds {total:.3e}, floor {floor:.3e}, bound of the call {te.errorBound():.3e}")
        assert te.errorBound() <= er.QUENCH_TOL
        assert err <= total + 10 * floor
    assert abs(te.time() - er.QUENCH_CALLS * er.QUENCH_DT) < 1e-15 and abs(te.totalErrorBound() - total) <= 1e-12 * total
    assert abs(te.overlapWithInitial() - np.vdot(psi0, dense[-1])) <= total + 10 * floor
    te.close()
    ctx.close()


@pytest.mark.parametrize("name", list(er.QUENCHES))
def test_long_call_takes_several_sub_steps_within_its_bound(mods, name):
    """one evolve(3.0) at m = 8: the whole remainder does not pass the tolerance, the bisection picks the sub-steps; held to the same
    bound, with the floor of the restatement run the same way at tol = 1e-13"""
    capi, solver = mods
    H, psi0, _ = er.quench_reference(name)
    want = er.Dense(H).propagate(psi0, 3.0)
    q = er.KrylovPropagator(H, psi0, 8, 1e-13)
    q.evolve(3.0)
    floor = float(np.linalg.norm(q.psi - want))
    p = er.KrylovPropagator(H, psi0, 8, 1e-9)
    ref_steps = p.evolve(3.0)
    assert np.linalg.norm(p.psi - want) <= p.bound + floor
    ctx = capi.Context()
    te = _solver(solver, ctx, name, 8, 1e-9)
    steps = te.evolve(3.0)
    err = float(np.linalg.norm(te.state() - want))
    print(f"{name}: {steps} sub-steps (restatement {ref_steps}), error {err:.3e}, bound {te.errorBound():.3e}, floor {floor:.3e}, applications {te.operatorApplications()}")
    assert steps > 1 and abs(steps - ref_steps) <= 1 and te.info() == "Success"
    assert te.errorBound() <= 1e-9 and err <= te.errorBound() + 10 * floor
    assert te.operatorApplications() == 9 * steps and abs(te.time() - 3.0) < 1e-15
    te.close()
    ctx.close()


def test_measurements_equal_numpy_on_the_downloaded_state(mods):
    capi, solver = mods
    ctx = capi.Context()
    for name in er.QUENCHES:
        L, n_up, bonds, hz, hx, bits = er.QUENCHES[name]
        te = _solver(solver, ctx, name, 12, 1e-9)
        te.evolve(0.8)
        x = te.state()
        st = mr.states(L, n_up)
        p = (np.abs(x) ** 2) / np.sum(np.abs(x) ** 2)
        sigma = np.array([2.0 * ((st >> np.uint64(i)) & np.uint64(1)).astype(np.float64) - 1.0 for i in range(L)])
        sz, zz = te.magnetisation(), te.correlationsZZ()
        assert np.abs(sz - 0.5 * sigma @ p).max() <= 1e-14
        assert np.abs(zz - 0.25 * (sigma * p) @ sigma.T).max() <= 1e-14
        H = er.quench_reference(name)[0]
        assert abs(te.energy() - np.vdot(x, H @ x).real / np.vdot(x, x).real) <= 1e-13
        # <Sx Sx + Sy Sy> of a pair through the restated Hermitian measurement
        xy = te.correlationsXY()
        _, flip, n2, *_ = er.measure_z(L, n_up, x, [], mr.pair_masks(L))
        for k, (i, j) in enumerate(mr.pairs(L)):
            assert abs(xy[i, j] - float(flip[k] / (2 * n2))) <= 1e-14 and xy[i, j] == xy[j, i]
        assert np.all(np.diag(zz) == 0.25) and np.all(np.diag(xy) == 0.5)
        te.close()
    ctx.close()


def test_invariants_at_20_10(mods):
    capi, solver = mods
    L, n_up, n = 20, 10, comb(20, 10)
    bonds, hz = sr.chain(L, 0.6, 1.0, periodic=True) + [(2, 9, 0.3, 0.4)], np.linspace(-0.5, 0.5, L)
    d_norm, d_energy, floor, a_small = er.invariant_drift()
    print(f"restatement on (12,6): norm drift {d_norm:.3e}, energy drift {d_energy:.3e}, floor {floor:.3e}, {a_small} applications")
    ctx = capi.Context()
    states = []
    for run in range(2):
        te = solver.SpinTimeEvolutionSolver().setModel(ctx, L, bonds, hz, n_up=n_up)
        te.setKrylovDimension(er.INVARIANT_M).setTolerance(er.INVARIANT_TOL).setProductState(er.neel(L))
        assert te.info() == "Success", te.log()
        assert te.overlapWithInitial() == 1.0 and te.normSquared() == 1.0
        e0 = te.energy()
        psi0 = te.state()
        steps = te.evolve(er.INVARIANT_DT)
        eb1, a_dev = te.errorBound(), te.operatorApplications()
        assert steps >= 1 and te.info() == "Success" and eb1 <= er.INVARIANT_TOL
        x = te.state()
        n2, e1 = te.normSquared(), te.energy()
        scale = a_dev / a_small
        b_norm = 10 * scale * max(d_norm, EPS)
        b_energy = 10 * scale * max(d_energy, EPS * abs(e0))
        print(f"run {run}: {steps} sub-steps, {a_dev} applications, |norm2 - 1| = {abs(n2 - 1):.3e} (bound {b_norm:.3e}), energy drift {abs(e1 - e0):.3e} (bound {b_energy:.3e}), "
              f"error bound {eb1:.3e}")
        assert abs(n2 - 1.0) <= b_norm and abs(e1 - e0) <= b_energy
        assert abs(te.overlapWithInitial() - np.vdot(psi0, x)) <= n * EPS
        te.evolve(-er.INVARIANT_DT)
        eb2 = te.errorBound()
        back = float(np.linalg.norm(te.state() - psi0))
        print(f"run {run}: return distance {back:.3e}, bounds {eb1:.3e} + {eb2:.3e}, floor {floor:.3e}")
        assert back <= eb1 + eb2 + 10 * floor and abs(te.time()) < 1e-15
        states.append((x, te.state(), n2, e1))
        te.close()
    assert states[0][0].tobytes() == states[1][0].tobytes() and states[0][1].tobytes() == states[1][1].tobytes()
    assert states[0][2:] == states[1][2:]
    ctx.close()


def test_invalid_input_is_reported(mods):
    capi, solver = mods
    ctx = capi.Context()
    te = solver.SpinTimeEvolutionSolver()
    assert te.evolve(0.1) == 0 and te.info() == "InvalidInput" and any("ERROR" in l for l in te.log())
    te.setModel(ctx, 6, sr.chain(6), n_up=3)
    assert te.evolve(0.1) == 0 and te.info() == "InvalidInput"  # no state
    te.setProductState(0b000011)
    assert te.info() == "InvalidInput"  # two sites up: outside the sector
    te.setProductState(0b1000111)
    assert te.info() == "InvalidInput"  # a site that does not exist
    te.setState(np.ones(7))
    assert te.info() == "InvalidInput"
    te.setState(np.zeros(20))
    assert te.info() == "InvalidInput"
    te.setState(np.arange(20.0) + 1j)  # not normalised: the norm is kept
    nrm = np.linalg.norm(np.arange(20.0) + 1j)
    assert te.info() == "Success" and abs(te.initialNorm() - nrm) < 1e-12 and abs(te.normSquared() - 1) < 1e-14
    assert np.abs(te.state() - (np.arange(20.0) + 1j)).max() < 1e-13
    te.setTolerance(0.0)
    assert te.evolve(0.1) == 0 and te.info() == "InvalidInput"
    te.setTolerance(1e-10)
    assert te.evolve(float("nan")) == 0 and te.info() == "InvalidInput"
    assert te.evolve(0.0) == 0 and te.info() == "Success"
    assert te.evolve(0.2) >= 1 and te.info() == "Success" and abs(np.linalg.norm(te.state()) - nrm) < 1e-11
    # a transverse field has no sector
    bad = solver.SpinTimeEvolutionSolver().setModel(ctx, 6, sr.chain(6), hx=np.full(6, 0.1), n_up=3).setProductState(0b000111)
    assert bad.info() == "InvalidInput" and any("transverse" in l for l in bad.log())
    for h in (te, bad, ctx):
        h.close()


def test_cpp_program_spin_evolution(tmp_path):
    """tests/cpp/spin_evolution_amd.cpp: the closed form and a Neel quench with its return in a C++11 user program built with -Wall
    -Wextra -Werror"""
    exe = str(tmp_path / "spin_evolution_amd")
    lib = os.path.join(ROOT, "cmpt-eigenex_amd", "lib")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cmpt-eigenex_amd", "include"),
                           os.path.join(ROOT, "tests", "cpp", "spin_evolution_amd.cpp"), "-o", exe, "-L", lib, "-leigenex_hip", "-Wl,-rpath," + lib])
    o = json.loads(subprocess.check_output([exe], timeout=300).decode())
    print(o)
    assert o["worst_sz"] <= 1e-13 and o["worst_overlap"] <= 1e-13 and o["worst_bound"] == 0.0
    assert o["rows"] == 252 and abs(o["t_forward"] - 1.0) < 1e-15 and abs(o["t_back"]) < 1e-15
    assert (o["overlap0_re"], o["overlap0_im"]) == (1.0, 0.0) and o["overlap1"] < 1.0
    floor = er.quench_floor("neel_xxz_10_5")
    assert abs(o["norm2"] - 1.0) <= 1e-13 and abs(o["e1"] - o["e0"]) <= 1e-12 and abs(o["sum_sz"]) <= 1e-13
    assert o["bounds"] <= 5e-9 and abs(o["bounds"] - o["total_bound"]) <= 1e-3 * o["bounds"]
    assert o["return_distance"] <= o["bounds"] + 10 * floor
    assert o["substeps"] >= 5 and o["applications"] >= 13 * o["substeps"]
    assert (o["refused_no_model"], o["refused_outside"], o["refused_length"], o["refused_tiny"]) == (1, 1, 1, 1)
