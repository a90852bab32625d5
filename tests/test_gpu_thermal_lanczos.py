"""The finite-temperature Lanczos solver on the device (thermal_lanczos.hpp: ThermalLanczosSolver, ThermalEnsemble, through their
Python wrappers) against dense diagonalisation (tests/thermal_reference.py).

Exact cases: with an orthonormal basis of the space as the start vectors and as many steps as rows every run ends in a breakdown
and the trace is complete, so log Z, E, C, S and every correlation must equal the dense answers: asserted to 1e-10, the project's
margin for Lanczos-derived moments against dense results.  Statistical case: R = 40 sign vectors, M = 50, every quantity within 5
reported standard errors.  Thermodynamics alone on momentum handles, real and complex."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spin_reference as sr  # noqa: E402
import thermal_reference as tr  # noqa: E402

pytestmark = pytest.mark.gpu
BETAS = (0.0, 0.5, 2.0, 10.0)
L8 = 8
BONDS8 = sr.chain(L8, 1.0, 0.7, periodic=True)


@pytest.fixture(scope="module")
def mods():
    from cmpt_eigenex_amd import capi, solver

    assert capi.device_count() >= 1
    return capi, solver


@pytest.fixture(scope="module")
def ring8():
    """dense answers of the sector (8,4): H, the pair operators and their diagonals in the eigenbasis"""
    H, zz, xy = tr.sector_matrices(L8, 4, BONDS8)
    E, U = np.linalg.eigh(H)
    pairs = sorted(zz)
    diag_of = [(U * (zz[p][:, None] * U)).sum(axis=0) for p in pairs] + [(U * (xy[p] @ U)).sum(axis=0) for p in pairs]
    return H, pairs, tr.exact(E, BETAS, diag_of)


def _exact_solver(capi, solver, S, vectors, dtype=np.float64):
    n = vectors.shape[1]
    th = solver.ThermalLanczosSolver(dtype)
    th.setDeviceOperator(S).set(lanczosSteps=n).setSampleVectors(vectors)
    return th


@pytest.mark.parametrize("basis", ["orthogonal", "unit"])
def test_exact_trace_of_the_sector_of_the_ring(mods, ring8, basis):
    """Ring of 8 sites, Jz = 1, Jxy = 0.7, sector (8,4), 70 rows; the 70 columns of a random orthogonal matrix, then the 70 unit
    vectors, M = 70.  Samples break down early (the k, -k degeneracies): wanted.  Largest deviation from dense diagonalisation on
    an MI355X, over beta = 0, 0.5, 2, 10: orthogonal basis 1.1e-14 on log Z, E, S, 2.2e-15 on C, 3.7e-15 on the correlations; unit
    vectors 1.8e-14, 4.9e-15 and 3.5e-15."""
    capi, solver = mods
    H, pairs, ex = ring8
    n = H.shape[0]
    assert n == 70
    vectors = np.linalg.qr(np.random.RandomState(8).standard_normal((n, n)))[0].T.copy() if basis == "orthogonal" else np.eye(n)
    ctx = capi.Context()
    S = capi.Csr.spin_half_sector(ctx, L8, 4, BONDS8)
    th = _exact_solver(capi, solver, S, vectors)
    assert th.setAllSitesAndPairs() == "Success"
    th.compute()
    r = th.results()
    assert r["info_name"] == "Success" and r["dimension"] == 70 and r["samples"] == 70 and r["sites"] == 8
    assert r["ndiag"] == 8 + 28 and r["nflip"] == 28 and any("breakdown" in line for line in th.log())
    assert r["operatorApplications"] < 70 * 70  # breakdowns ended samples early
    worst = dict(thermo=0.0, C=0.0, corr=0.0)
    for b in BETAS:
        logz, e, c, s, obs = ex[b]
        got = (th.logPartitionFunction(b), th.energy(b), th.specificHeat(b), th.entropy(b))
        worst["thermo"] = max(worst["thermo"], abs(got[0] - logz), abs(got[1] - e), abs(got[3] - s))
        worst["C"] = max(worst["C"], abs(got[2] - c))
        for k, (i, j) in enumerate(pairs):
            worst["corr"] = max(worst["corr"], abs(th.correlationZZ(i, j, b) - obs[k]), abs(th.correlationXY(j, i, b) - obs[len(pairs) + k]))
            assert abs(th.correlationSS(i, j, b) - obs[k] - obs[len(pairs) + k]) < 1e-10
        if b > 0:
            assert abs(th.freeEnergy(b) + logz / b) < 1e-10
    print(f"exact trace ({basis}): largest deviation from dense: log Z, E, S {worst['thermo']:.3e}, C {worst['C']:.3e}, correlations {worst['corr']:.3e}")
    assert max(worst.values()) < 1e-10
    # beta = 0: Z = 70, <sigma_i sigma_j> = ((2 n_up - L)^2 - L) / (L (L - 1)) = -1/7 for every pair, <sigma_i> = 0
    assert abs(np.exp(th.logPartitionFunction(0.0)) - 70.0) < 1e-10 * 70
    for t in range(8):
        assert abs(th.diagonal(t, 0.0)) < 1e-10
    for t in range(28):
        assert abs(th.diagonal(8 + t, 0.0) + 1.0 / 7.0) < 1e-10
    assert th.correlationZZ(3, 3, 1.0) == 0.25 and th.correlationXY(3, 3, 1.0) == 0.5 and th.correlationSS(3, 3, 1.0) == 0.75
    # identical physics from every sample's complete trace: the scatter between samples is not zero, the error is finite
    assert np.isfinite(th.standardError("energy", 0.5)) and np.isfinite(th.standardError("observable", 0.5, th.observableIndex("ZZ", 0, 1)))
    theta, w = th.sample(0)
    assert abs(w.sum() - 1.0) < 1e-12 and theta.size <= 70 and np.all(np.diff(theta) >= 0)
    with pytest.raises(capi.EigenexError, match="outside the model"):
        th.correlationZZ(0, 8, 1.0)
    for h in (th, S, ctx):
        h.close()


def test_ensemble_of_all_sectors_against_the_dense_hamiltonian(mods):
    """All nine Sz sectors of the ring of 8 exactly (unit vectors, M = rows); n_up < 4 enters with multiplicity 2, n_up = 4 once.
    Z, E, C, S and the susceptibility against the dense 256-row Hamiltonian to 1e-10."""
    capi, solver = mods
    Hd = sr.dense_kron(L8, BONDS8)
    E, U = np.linalg.eigh(Hd)
    mag = np.array([bin(s).count("1") - L8 / 2 for s in range(1 << L8)])
    m2 = (U * (mag[:, None] ** 2 * U)).sum(axis=0)
    ex = tr.exact(E, BETAS, [m2])
    ctx = capi.Context()
    en = solver.ThermalEnsemble(L8)
    logz, keep = {}, []
    for n_up in range(L8 + 1):
        S = capi.Csr.spin_half_sector(ctx, L8, n_up, BONDS8)
        n = S.info()["n_global"]
        th = _exact_solver(capi, solver, S, np.eye(n)).compute()
        assert th.results()["info_name"] == "Success" and th.results()["samples"] == n
        logz[n_up] = [th.logPartitionFunction(b) for b in BETAS]
        if n_up <= 4:
            en.add(th, 1.0 if n_up == 4 else 2.0, n_up - L8 / 2)
        keep += [th, S]
    for n_up in range(4):  # spin inversion: what the multiplicity stands for
        assert np.abs(np.array(logz[n_up]) - np.array(logz[L8 - n_up])).max() < 1e-10
    worst = 0.0
    for b in BETAS:
        lz, e, c, s, (mm,) = ex[b]
        got = (en.logPartitionFunction(b), en.energy(b), en.specificHeat(b), en.entropy(b), en.susceptibility(b))
        want = (lz, e, c, s, b * mm / L8)  # <M> = 0 without a field
        worst = max(worst, max(abs(g - w) for g, w in zip(got, want)))
    print(f"ensemble of 9 sectors: largest deviation from the dense 256-row Hamiltonian {worst:.3e}")
    assert worst < 1e-10
    assert abs(np.exp(en.logPartitionFunction(0.0)) - 256.0) < 1e-10 * 256
    en.close()
    for h in keep + [ctx]:
        h.close()


def test_ensemble_observable_weights_the_sectors(mods):
    """<Sz_0 Sz_1> of the whole ring from the sectors n_up <= 4 (an even mask: invariant under spin inversion) against the dense
    256-row Hamiltonian, 1e-10"""
    capi, solver = mods
    E, U = np.linalg.eigh(sr.dense_kron(L8, BONDS8))
    zz01 = np.array([(1 if s & 1 else -1) * (1 if s & 2 else -1) for s in range(1 << L8)], float)
    ex = tr.exact(E, BETAS, [(U * (zz01[:, None] * U)).sum(axis=0)])
    ctx = capi.Context()
    en, keep = solver.ThermalEnsemble(L8), []
    for n_up in range(5):
        S = capi.Csr.spin_half_sector(ctx, L8, n_up, BONDS8)
        th = _exact_solver(capi, solver, S, np.eye(S.info()["n_global"]))
        assert th.setSpinObservables([0b11], []) == "Success"
        en.add(th.compute(), 1.0 if n_up == 4 else 2.0, n_up - L8 / 2)
        keep += [th, S]
    for b in BETAS:
        assert abs(en.observable(0, b) - ex[b][4][0]) < 1e-10
    en.close()
    for h in keep + [ctx]:
        h.close()


def test_random_vectors_within_five_standard_errors(mods):
    """Sector (12,6), Jz = 1, Jxy = 0.7, R = 40 sign vectors of seed 20260 (thermal_reference.STAT; its numpy restatement with the
    same vectors deviates by at most 3.43 reported standard errors), M = 50, beta = 0.1, 0.5, 1, 2: log Z, E, C, S and all 12
    nearest-neighbour ZZ and XY correlations within 5 reported standard errors of dense diagonalisation, none left out."""
    capi, solver = mods
    c = tr.STAT
    L = c["L"]
    bonds = [(i, (i + 1) % L, c["jz"], c["jxy"]) for i in range(L)]
    H, zz, xy = tr.sector_matrices(L, c["n_up"], bonds)
    nn = [(min(i, (i + 1) % L), max(i, (i + 1) % L)) for i in range(L)]
    E, U = np.linalg.eigh(H)
    diag_of = [(U * (zz[p][:, None] * U)).sum(axis=0) for p in nn] + [(U * (xy[p] @ U)).sum(axis=0) for p in nn]
    ex = tr.exact(E, c["betas"], diag_of)
    ctx = capi.Context()
    S = capi.Csr.spin_half_sector(ctx, L, c["n_up"], bonds)
    th = solver.ThermalLanczosSolver().setDeviceOperator(S).set(lanczosSteps=c["M"], randomVectors=c["R"], seed=c["seed"], firstStream=c["first_stream"])
    assert th.setAllSitesAndPairs() == "Success"
    th.compute()
    r = th.results()
    assert r["info_name"] == "Success" and r["samples"] == c["R"] and r["operatorApplications"] == c["R"] * c["M"]
    worst = 0.0
    for b in c["betas"]:
        lz, e, cv, s, obs = ex[b]
        rows = [("logPartitionFunction", th.logPartitionFunction(b), lz, 0), ("energy", th.energy(b), e, 0), ("specificHeat", th.specificHeat(b), cv, 0),
                ("entropy", th.entropy(b), s, 0)]
        for k, (i, j) in enumerate(nn):
            rows.append(("observable", th.correlationZZ(i, j, b), obs[k], th.observableIndex("ZZ", i, j)))
            rows.append(("observable", th.correlationXY(i, j, b), obs[len(nn) + k], th.observableIndex("XY", i, j)))
        for k, (name, got, want, t) in enumerate(rows):
            scale = 1.0 if name != "observable" else (0.25 if k % 2 == 0 else 0.5)  # the error is that of the raw average
            err = th.standardError(name, b, t) * scale
            assert err > 0 and np.isfinite(err)
            worst = max(worst, abs(got - want) / err)
            assert abs(got - want) <= 5 * err, (b, name, t, got, want, err)
    print(f"R = {c['R']}, M = {c['M']}, seed {c['seed']}: worst deviation {worst:.2f} reported standard errors")
    for h in (th, S, ctx):
        h.close()


def test_thermodynamics_on_momentum_handles(mods):
    """(12,6) of the Heisenberg ring: the 12 momentum sectors, complex states where the momentum is not 0 or pi, each with its unit
    vectors as samples; the summed Z(beta) is the Sz sector's (dense) to 1e-10 relative."""
    capi, solver = mods
    L, n_up = 12, 6
    bonds = sr.chain(L, 1.0, 0.7, periodic=True)
    E = np.linalg.eigvalsh(tr.sector_matrices(L, n_up, bonds)[0])
    ctx = capi.Context()
    en, keep, total = solver.ThermalEnsemble(L), [], 0
    for k in range(L):
        is_complex = k not in (0, L // 2)
        n = capi.spin_momentum_dim(L, n_up, k)
        total += n
        M = capi.Csr.spin_half_momentum(ctx, L, n_up, k, bonds, complex_states=is_complex)
        th = _exact_solver(capi, solver, M, np.eye(n), np.complex128 if is_complex else np.float64)
        assert th.setAllSitesAndPairs() == "InvalidInput" and th.setSpinObservables([1], []) == "InvalidInput"
        en.add(th.compute(), 1.0, 0.0)
        assert th.results()["info_name"] == "Success" and th.results()["ndiag"] == 0
        keep += [th, M]
    assert total == E.size
    worst = 0.0
    for b in (0.0, 0.5, 2.0):
        want = tr.exact(E, [b])[b]
        worst = max(worst, abs(en.logPartitionFunction(b) - want[0]), abs(en.energy(b) - want[1]), abs(en.specificHeat(b) - want[2]))
    print(f"12 momentum sectors of (12,6): largest deviation of log Z, E, C from the Sz sector {worst:.3e}")
    assert worst < 1e-10
    en.close()
    for h in keep + [ctx]:
        h.close()


def test_cpp_program_thermal_lanczos(ring8, tmp_path):
    """tests/cpp/thermal_lanczos_amd.cpp: the classes in a C++11 user program, built with -Wall -Wextra -Werror: the exact-trace
    case with unit vectors and the ensemble of the sectors n_up <= 4, against the same dense answers, 1e-10."""
    import json
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, lib = str(tmp_path / "thermal_lanczos_amd"), os.path.join(root, "cmpt-eigenex_amd", "lib")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(root, "include"), "-I", os.path.join(root, "cmpt-eigenex_amd", "include"),
                           os.path.join(root, "tests", "cpp", "thermal_lanczos_amd.cpp"), "-o", exe, "-L", lib, "-leigenex_hip", "-Wl,-rpath," + lib])
    o = json.loads(subprocess.check_output([exe], timeout=120).decode())
    _, pairs, ex = ring8
    assert (o["rows"], o["samples"], o["info"], o["masks"], o["complex_masks"], o["no_operator"]) == (70, 70, 0, 0, 3, 3) and o["applications"] < 4900
    worst = 0.0
    for row in o["sector"]:
        logz, e, c, s, obs = ex[row["beta"]]
        worst = max(worst, abs(row["logZ"] - logz), abs(row["E"] - e), abs(row["C"] - c), abs(row["S"] - s),
                    np.abs(np.array(row["zz"]) - obs[: len(pairs)]).max(), np.abs(np.array(row["xy"]) - obs[len(pairs) :]).max())
        assert np.isfinite(row["energy_error"])
    E, U = np.linalg.eigh(sr.dense_kron(L8, BONDS8))
    mag = np.array([bin(s).count("1") - L8 / 2 for s in range(1 << L8)])
    zz01 = np.array([(1 if s & 1 else -1) * (1 if s & 2 else -1) for s in range(1 << L8)], float) / 4
    exd = tr.exact(E, BETAS, [(U * (mag[:, None] ** 2 * U)).sum(axis=0), (U * (zz01[:, None] * U)).sum(axis=0)])
    for row in o["ensemble"]:
        b = row["beta"]
        logz, e, c, s, (m2, zz) = exd[b]
        worst = max(worst, abs(row["logZ"] - logz), abs(row["E"] - e), abs(row["C"] - c), abs(row["S"] - s), abs(row["chi"] - b * m2 / L8), abs(row["zz01"] - zz))
    print(f"C++ program: largest deviation from dense {worst:.3e}")
    assert worst < 1e-10


def test_invalid_input(mods):
    capi, solver = mods
    ctx = capi.Context()
    th = solver.ThermalLanczosSolver()
    th.compute()
    assert th.results()["info_name"] == "InvalidInput" and th.setAllSitesAndPairs() == "InvalidInput"
    S = capi.Csr.spin_half_sector(ctx, 6, 3, sr.chain(6))
    th.setDeviceOperator(S).setSampleVectors(np.ones((2, 19)))  # 20 rows
    assert th.compute().results()["info_name"] == "InvalidInput"
    th.setSampleVectors(None).set(lanczosSteps=0)
    assert th.compute().results()["info_name"] == "InvalidInput"
    assert th.set(lanczosSteps=5, randomVectors=3).compute().results()["info_name"] == "Success" and th.results()["samples"] == 3
    with pytest.raises(capi.EigenexError, match="setAllSitesAndPairs"):
        th.correlationZZ(0, 1, 1.0)
    rowptr, col, val = capi.spin_sector_csr(6, 3, sr.chain(6))
    A = capi.Csr.upload(ctx, 20, rowptr, col, val, column_blocks=0)
    ta = solver.ThermalLanczosSolver().setDeviceOperator(A)
    assert ta.setSpinObservables([1], []) == "InvalidInput" and ta.setSpinObservables([], []) == "Success"
    assert ta.set(lanczosSteps=20).setSampleVectors(np.eye(20)).compute().results()["info_name"] == "Success"  # thermodynamics of any operator
    assert abs(ta.logPartitionFunction(0.0) - np.log(20.0)) < 1e-12
    for h in (ta, th, A, S, ctx):
        h.close()
