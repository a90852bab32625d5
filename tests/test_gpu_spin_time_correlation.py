"""SpinTimeCorrelationSolver (spin_time_correlation.hpp) on the device against dense exponentials of both vectors
(tests/spin_time_correlation_reference.py: spin_evolution_reference.Dense and KrylovPropagator).  Cases, each with eight calls of
evolve(0.25) at m = 12 and tol = 1e-9: (a) the Neel state of the open XXZ chain (10,5), B = S-_4, A_j = S-_j for every site,
(10,5) -> (10,4); (b) the ground state of the Heisenberg ring (10,5), A = B = Sz_q at q = 2 pi 3 / 10, with psi evolved and with
setEigenstate(E0).  After each call, for every measured operator,
    |C_dev - C_dense| <= errorBound(n) + 10 floor,    floor = max(excess, applications * eps * ||A_n|| |B psi_0|),
where excess is the restatement's excess over its own bound at tol = 1e-13 and the second term is one rounding per operator
application on numbers of the correlation's size, and errorBound(n) equals its formula ||A_n|| |B psi_0| (eps_psi + eps_phi) with
each eps at most calls * tol.  The restatement alone, on the CPU (tests/test_spin_time_correlation_host.py): (a) worst error
1.9e-14 under a bound of 2.1e-13; (b) error 1.1e-15 with a bound of 5.5e-22, an eigenstate breaking down exactly.  Then (b) against
the poles and weights of SpinDynamicsSolver, t = 0 against numpy, two sites in closed form, the invalid inputs and the C++
program.  NOT part of the reference project."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spin_dynamics_reference as dr  # noqa: E402
import spin_evolution_reference as er  # noqa: E402
import spin_time_correlation_reference as tr  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = tr.EPS


@pytest.fixture(scope="module")
def mods():
    from cmpt_eigenex_amd import capi, solver

    assert capi.device_count() >= 1
    return capi, solver


@pytest.fixture(scope="module")
def cases(mods):
    """the three cases and the excess of each restatement, computed once"""
    capi, _ = mods
    out = {}
    for name in ("neel", "ring", "ring eigen"):
        c = tr.case(capi, name)
        out[name] = (c, tr.excess(c))
    return out


def _solver(mods, ctx, name, case):
    _, solver = mods
    L, bonds, hz, hx = case.model
    tc = solver.SpinTimeCorrelationSolver().setModel(ctx, L, bonds, hz, hx, n_up=case.n_up).setKrylovDimension(tr.M).setTolerance(tr.TOL)
    if name == "neel":
        tc.setProductState(er.QUENCHES["neel_xxz_10_5"][5]).setSourceOperator(dr.MINUS, np.eye(L)[4]).setMeasuredSites()
    else:
        tc.setState(1.7 * case.psi0).setMomentumZ(2 * np.pi * 3 / 10)  # not normalised: the solver divides by <psi|psi>
        if name == "ring eigen":
            tc.setEigenstate(case.eigen_energy)
    return tc


@pytest.mark.parametrize("name", ["neel", "ring", "ring eigen"])
def test_correlations_against_the_dense_exponentials(mods, cases, name):
    capi, _ = mods
    case, excess = cases[name]
    ctx = capi.Context()
    tc = _solver(mods, ctx, name, case)
    K = len(case.measured)
    # t = 0: <A psi_0 | B psi_0> from numpy; each is a sum of at most rows products below ||A|| |B psi_0|, formed with L roundings each
    c0 = tc.values()
    assert tc.info() == "Success", tc.log()
    want0 = case.dense_values(0.0)
    assert c0.shape == (K,) and np.all(np.abs(c0 - want0) <= (case.H_dst.shape[0] + 4 * case.model[0]) * EPS * case.norms * case.source_norm)
    assert abs(tc.sourceNormSquared() - case.source_norm ** 2) <= (case.H_dst.shape[0] + 4 * case.model[0]) * EPS * case.source_norm ** 2
    assert tc.time() == 0.0 and tc.errorBound() == 0.0 and tc.operatorApplications() == 0
    for k in range(tr.CALLS):
        steps = tc.evolve(tr.DT)
        assert steps >= 1 and tc.info() == "Success", tc.log()
        got = tc.values()
        assert tc.info() == "Success", tc.log()
        want = case.dense_values(tr.DT * (k + 1))
        eps_psi, eps_phi, apps = tc.stateErrorBound(), tc.sourceErrorBound(), tc.operatorApplications()
        assert 0.0 <= eps_psi <= (k + 1) * tr.TOL and 0.0 <= eps_phi <= (k + 1) * tr.TOL
        if name == "ring eigen":
            assert eps_psi == 0.0
        scale = case.norms * np.sqrt(tc.sourceNormSquared())
        formula = scale * (eps_psi + eps_phi)
        bounds = np.array([tc.errorBound(n) for n in range(K)])
        slack = (case.model[0] + 4) * EPS  # the two sums of |a_i| are taken in different orders
        assert np.all(np.abs(bounds - formula) <= slack * formula) and abs(tc.errorBound() - formula.max()) <= slack * formula.max()
        floor = np.maximum(excess, apps * EPS * scale)
        err = np.abs(got - want)
        worst = int(np.argmax(err - bounds))
        print(f"{name} call {k}: {steps} sub-steps, {apps} applications, operator {worst}: error {err[worst]:.3e}, bound {bounds[worst]:.3e}, "
              f"floor {floor[worst]:.3e} (excess {excess:.3e}), eps {eps_psi:.3e} + {eps_phi:.3e}")
        assert np.all(err <= bounds + 10 * floor)
    assert abs(tc.time() - tr.CALLS * tr.DT) < 1e-15
    tc.close()
    ctx.close()


def test_ground_state_response_is_the_sum_over_the_poles_of_the_dynamics_solver(mods, cases):
    """C(t) = sum_n w_n exp(-i p_n t) with the poles and weights of SpinDynamicsSolver's single complex run at the same q: both
    are |<n| Sz_q |psi_0>|^2 resolved by energy.  A pole within MOMENT_TOL (relative to the spectrum's scale, which 1 + t covers at
    these energies of order one) moves its phase by MOMENT_TOL t; the weights agree to MOMENT_TOL of their sum."""
    capi, solver = mods
    case, _ = cases["ring eigen"]
    q = 2 * np.pi * 3 / 10
    ctx = capi.Context()
    L, bonds, hz, hx = case.model
    sd = solver.SpinDynamicsSolver().setModel(ctx, L, bonds, hz, hx, case.n_up).setState(case.psi0.real).setStateEnergy(case.eigen_energy)
    r = sd.setLanczosSteps(120).computeStructureFactorZSingleRun(q).results()
    assert r["info_name"] == "Success", sd.log()
    tc = _solver(mods, ctx, "ring eigen", case)
    for k in range(tr.CALLS + 1):
        if k:
            tc.evolve(tr.DT)
        t = tc.time()
        got = tc.values()[0]
        want = np.sum(r["weights"] * np.exp(-1j * r["poles"] * t))
        print(f"t = {t:.2f}: C = {got!r}, from the poles {want!r}, difference {abs(got - want):.2e}, bound {tc.errorBound():.2e}")
        assert abs(got - want) <= dr.MOMENT_TOL * r["weights"].sum() * (1 + t)
    for h in (tc, sd, ctx):
        h.close()


def test_two_sites_closed_form(mods):
    """J Heisenberg on two sites from |up down>: <Sz_0(t) Sz_0(0)> = cos(J t) / 4, and <Sz_1(t) Sz_0(0)> = -cos(J t) / 4; the Krylov
    space is the whole sector, so the bound is 0"""
    capi, solver = mods
    ctx = capi.Context()
    J = 1.3
    tc = solver.SpinTimeCorrelationSolver().setModel(ctx, 2, [(0, 1, J, J)], n_up=1).setProductState(0b01)
    tc.setSourceOperator(dr.Z, [1.0, 0.0]).setMeasuredSites()
    for k in range(9):
        if k:
            assert tc.evolve(-0.4 if k % 3 == 0 else 0.7) == 2 and tc.info() == "Success", tc.log()
        t = tc.time()
        c = tc.values()
        print(f"t = {t:.2f}: errors {abs(c[0] - np.cos(J * t) / 4):.3e}, {abs(c[1] + np.cos(J * t) / 4):.3e}")
        assert abs(c[0] - np.cos(J * t) / 4) <= 1e-13 and abs(c[1] + np.cos(J * t) / 4) <= 1e-13
        assert tc.errorBound() == 0.0 and tc.sourceNormSquared() == 0.25
    tc.close()
    ctx.close()


def test_a_vanishing_source_gives_a_zero_response(mods, cases):
    """the total Sz annihilates a state of the sector Sz = 0 (up to the rounding of the application): Success, zeros, logged"""
    capi, _ = mods
    case, _ = cases["ring"]
    ctx = capi.Context()
    _, solver = mods
    L, bonds, hz, hx = case.model
    tc = solver.SpinTimeCorrelationSolver().setModel(ctx, L, bonds, hz, hx, n_up=case.n_up).setState(case.psi0).setMomentumZ(0.0)
    assert tc.evolve(0.5) == 0 and tc.info() == "Success" and any("identically zero" in l for l in tc.log())
    assert np.array_equal(tc.values(), np.zeros(1)) and tc.info() == "Success" and any("identically zero" in l for l in tc.log())
    assert tc.time() == 0.5 and tc.sourceNormSquared() == 0.0 and tc.errorBound() == 0.0 and tc.operatorApplications() == 0
    tc.close()
    ctx.close()


def test_invalid_input_is_logged_not_thrown(mods, cases):
    capi, solver = mods
    case, _ = cases["ring"]
    L, bonds, hz, hx = case.model
    ctx = capi.Context()

    def refused(tc, word, call="evolve"):
        out = tc.evolve(0.1) if call == "evolve" else tc.values()
        ok = tc.info() == "InvalidInput" and any(l.startswith("ERROR") and word in l for l in tc.log())
        return ok and (out == 0 if call == "evolve" else out.size == 0)

    new = lambda n_up=5: solver.SpinTimeCorrelationSolver().setModel(ctx, L, bonds, hz, hx, n_up=n_up)  # noqa: E731
    assert refused(solver.SpinTimeCorrelationSolver(), "no model")
    assert refused(new(), "no state") and refused(new(), "no state", "values")
    assert refused(new().setState(case.psi0), "no source operator")
    ok = np.ones(L)
    assert refused(new().setState(case.psi0[:-1]).setSourceOperator(dr.Z, ok), "one entry per row")
    assert refused(new().setState(np.zeros(case.psi0.size)).setSourceOperator(dr.Z, ok), "state is zero")
    assert refused(new().setState(case.psi0).setSourceOperator(dr.Z, ok[:-1]), "one coefficient per site")
    assert refused(new().setState(case.psi0).setSourceOperator(dr.Z, ok).addMeasuredOperator(np.ones(L + 1)), "one coefficient per site")
    bad = ok.astype(np.complex128)
    bad[3] = complex(1.0, np.nan)
    assert refused(new().setState(case.psi0).setSourceOperator(dr.Z, bad), "not finite")
    assert refused(new().setState(case.psi0).setSourceOperator(dr.Z, ok).addMeasuredOperator(bad), "not finite")
    assert refused(new().setState(case.psi0).setSourceOperator(7, ok), "kind")
    assert refused(new(n_up=L).setState(np.ones(1)).setSourceOperator(dr.PLUS, ok), "leave the sectors")
    assert refused(new(n_up=0).setState(np.ones(1)).setSourceOperator(dr.MINUS, ok), "leave the sectors")
    assert refused(new().setProductState(0b11).setSourceOperator(dr.Z, ok), "does not lie in the sector")
    assert refused(new().setState(case.psi0).setSourceOperator(dr.Z, ok).setKrylovDimension(1), "at least 2")
    assert refused(new().setState(case.psi0).setSourceOperator(dr.Z, ok).setTolerance(0.0), "positive tolerance")
    # a measured operator added after the start is checked where it is used, and the solver goes on once it is right
    tc = new().setState(case.psi0).setSourceOperator(dr.Z, np.eye(L)[0]).addMeasuredOperator(np.eye(L)[0])
    assert tc.evolve(0.1) >= 1 and tc.info() == "Success"
    assert refused(tc.addMeasuredOperator(np.ones(L - 1)), "one coefficient per site", "values")
    tc.clearMeasuredOperators().addMeasuredOperator(np.eye(L)[1])
    assert tc.values().size == 1 and tc.info() == "Success" and tc.time() == 0.1
    tc.close()
    ctx.close()


def test_cpp_program_spin_time_correlation(tmp_path, mods, cases):
    """tests/cpp/spin_time_correlation_amd.cpp: the closed form and the Neel case in a C++11 user program built with -Wall -Wextra
    -Werror"""
    exe = str(tmp_path / "spin_time_correlation_amd")
    lib = os.path.join(ROOT, "cmpt-eigenex_amd", "lib")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cmpt-eigenex_amd", "include"),
                           os.path.join(ROOT, "tests", "cpp", "spin_time_correlation_amd.cpp"), "-o", exe, "-L", lib, "-leigenex_hip", "-Wl,-rpath," + lib])
    o = json.loads(subprocess.check_output([exe], timeout=300).decode())
    print(o)
    case, excess = cases["neel"]
    assert o["worst"] <= 1e-13 and o["worst_bound"] == 0.0
    assert (o["c0_re"], o["c0_im"], o["others0"], o["source_norm2"]) == (1.0, 0.0, 0.0, 1.0)
    want = case.dense_values(1.0)
    floor = max(excess, o["applications"] * EPS)
    assert abs(complex(o["c1_re"], o["c1_im"]) - want[4]) <= o["bound"] + 10 * floor
    assert abs(o["sum1"] - float(np.sum(np.abs(want) ** 2))) <= 2 * len(want) * (o["bound"] + 10 * floor)
    assert abs(o["time"] - 1.0) < 1e-15 and 0.0 < o["bound"] <= 8e-9 and abs(o["bound"] - (o["eps_state"] + o["eps_source"])) <= 1e-3 * o["bound"]
    assert o["substeps"] >= 8 and o["applications"] >= 13 * o["substeps"]
    assert (o["refused_no_model"], o["refused_no_source"], o["refused_length"], o["refused_count"], o["refused_leaves"]) == (1, 1, 1, 1, 1)


def test_a_change_in_the_middle_of_a_run_restarts_and_says_so_and_a_failed_call_is_not_read_from(mods, cases):
    """setKrylovDimension after some evolution starts again at t = 0 with a log line.  A tolerance no inexact step can pass
    (1e-300) ends evolve() in NumericalIssue; the two vectors may then stand at different times, so evolve() and values() are
    refused until the run is set up again."""
    capi, _ = mods
    case, excess = cases["neel"]
    ctx = capi.Context()
    tc = _solver(mods, ctx, "neel", case)
    assert tc.evolve(tr.DT) >= 2 and tc.info() == "Success" and tc.time() == tr.DT and tc.errorBound() > 0.0
    assert not any("starts again" in l for l in tc.log())
    tc.setKrylovDimension(tr.M + 2)
    c0 = tc.values()
    assert tc.info() == "Success" and any(l.startswith("INFO") and "starts again at t = 0" in l for l in tc.log())
    assert tc.time() == 0.0 and tc.errorBound() == 0.0 and tc.operatorApplications() == 0 and c0[4] == 1.0
    tc.values()
    assert not any("starts again" in l for l in tc.log())  # said once, by the call that did it
    assert tc.evolve(tr.DT) >= 2 and tc.info() == "Success"
    tc.setTolerance(1e-300)
    assert tc.evolve(tr.DT) == 0 and tc.info() == "NumericalIssue" and any("no step passes" in l for l in tc.log())
    assert tc.time() == tr.DT  # the failed call did not count
    for call in (tc.values, lambda: tc.evolve(tr.DT)):
        out = call()
        assert tc.info() == "InvalidInput" and any(l.startswith("ERROR") and "last evolve() failed" in l for l in tc.log())
        assert np.size(out) == 0 or out == 0
    tc.setTolerance(tr.TOL).setKrylovDimension(tr.M)
    assert tc.evolve(tr.DT) >= 2 and tc.info() == "Success" and tc.time() == tr.DT
    got, want = tc.values(), case.dense_values(tr.DT)
    floor = max(excess, tc.operatorApplications() * EPS)  # as in the first test; ||A_n|| |B psi_0| = 1 here
    assert tc.info() == "Success" and np.all(np.abs(got - want) <= np.array([tc.errorBound(n) for n in range(len(want))]) + 10 * floor)
    tc.close()
    ctx.close()
