"""The reduced density matrix of a complex state on the device (eigenex_spin_rdm_z, kernels.hip: k_spin_rdm<SECTOR, TILE, SpinZ> and
k_spin_rdm_reduce<SpinZ>) against the long double restatement of tests/spin_rdm_z_reference.py, within 2 n_b eps times the sums of
magnitudes -- the rounding of a 2 n_b-term sum in any grouping, so it holds for every launch grid, slice count and tile size.  The
shapes are those of tests/test_gpu_spin_rdm.py, for its reasons: the complex kernel takes the same plan.  On every shape: the
bound, the diagonal's imaginary part +0.0, (j, i) the conjugate of (i, j) bit for bit, two calls bitwise equal, the vector
unchanged, the trace.  Then: a state a + 0i against the real kernel; a complex Lanczos run that does not notice a call between its
batches; the refusals; the two-site closed form; the quench of tests/test_gpu_spin_evolution.py against dense diagonalisation
through SpinTimeEvolutionSolver; SpinEntanglementSolver with a complex state; and both C++ classes in a user program.

Tolerances of the entropy tests.
  rounding term  rz.entropy_tolerance_z(d, n_b): rr.entropy_tolerance re-derived for sums of 2 n_b products and for
                 small_eigen::hermitian (the real symmetric embedding of order 2d): delta = (3 n_b + 2 d) eps per eigenvalue.
  closed form    two sites: the step is exact (breakdown, m >= dimension), so the error is the rounding of a 2 x 2 problem.  Per
                 evolve call an amplitude is off by at most 16 eps: 2 eps from the normalisation of W, 4 eps each from alpha, beta
                 and from the 2 x 2 eigen-decomposition (the gap is Jxy, the vectors are (1, +-1) / sqrt 2), |tau theta| + 1 <= 3 eps
                 from the phase and its cosine and sine, 3 eps from the combination of two columns.  A probability |psi_s|^2 is
                 then off by 32 eps per call, and divided by the trace (off by twice that) an eigenvalue of rho_A by delta =
                 100 k eps after k calls.  Two eigenvalues: |S - S_exact| <= 2 (-delta ln delta).
  quench         Fannes-Audenaert: |S(rho) - S(sigma)| <= T ln(d - 1) + h2(T) for trace distance T; the trace distance of two
                 reduced density matrices is at most that of the pure states, which is at most |psi - phi| = totalErrorBound() +
                 quench_floor.  d = 32.  Plus the rounding term for each of the two computed entropies.
  Renyi-2        -ln ||rho||_F^2 against -ln sum lambda^2: sum lambda^2 >= 1/d moves by at most 2 sum lambda (2d eps) = 4d eps from
                 the eigenvalues; the sum of 2 d^2 squares has a relative error of at most 2 d^2 eps: the logarithms differ by at
                 most (4 d^2 + 2 d^2) eps, held to 8 d^2 eps."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
from math import log, pi

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spin_evolution_reference as er  # noqa: E402
import spin_rdm_reference as rr  # noqa: E402
import spin_rdm_z_reference as rz  # noqa: E402
import spin_reference as sr  # noqa: E402
from test_gpu_spin_rdm import SHAPES  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(rr.EPS)
QUENCH = "neel_xxz_10_5"
A10, B10 = 0b0000011111, 0b1111100000  # sites 0..4 of the 10-site chain and the others
ROUND_10_5 = rz.entropy_tolerance_z(32, 10)  # 32 eigenvalues in blocks of at most C(5,2) = 10 rows, sums of at most 10 b's


@pytest.fixture(scope="module")
def mods():
    from cmpt_eigenex_amd import capi, solver

    assert capi.device_count() >= 1
    return capi, solver


def _operator(capi, ctx, L, n_up, bonds=None, complex_states=True):
    bonds = sr.chain(L, 1.0, 0.7, periodic=True) if bonds is None else bonds
    if n_up is None:
        return capi.Csr.spin_half(ctx, L, bonds, complex_states=complex_states)
    return capi.Csr.spin_half_sector(ctx, L, n_up, bonds, complex_states=complex_states)


@pytest.mark.parametrize("L,n_up,mask,tuned", SHAPES)
def test_device_blocks_equal_the_restatement_within_the_bound(mods, L, n_up, mask, tuned):
    capi, _ = mods
    ctx = capi.Context()
    S = _operator(capi, ctx, L, n_up)
    n = rr.rows(L, n_up)
    b = capi.Basis(ctx, S, n, 2)
    assert b.is_complex
    if tuned:
        b.tune(2, 16, 0)  # as many workgroups as the operator has tiles: the b range of the small blocks is cut into slices
    x = er.vector_z(L, n_up)
    b.upload(capi.VEC_COL(1), x)
    got = b.spin_rdm_z(capi.VEC_COL(1), mask)
    rz.check_z(f"device_z ({L},{n_up},{mask:#x})", got, rz.rdm_z(L, n_up, x, mask))  # the bound, Im diag = +0.0, Hermitian bits
    again = b.spin_rdm_z(capi.VEC_COL(1), mask)
    assert [k for k, _ in again] == [k for k, _ in got] and all(p.tobytes() == q.tobytes() for (_, p), (_, q) in zip(got, again))
    assert b.download(capi.VEC_COL(1)).tobytes() == x.tobytes()
    rz.trace_check(got, x, n)
    kf, dims, _ = capi.spin_rdm_layout(L, n_up, mask)
    assert [k for k, _ in got] == [kf + i for i in range(len(dims))] and [m.shape[0] for _, m in got] == dims
    for h in (b, S, ctx):
        h.close()


@pytest.mark.parametrize("L,n_up,mask", [(10, None, 0b1011011101), (12, 6, 0b111111100000), (17, None, (1 << 16) | 1)])
def test_a_real_state_gives_the_real_kernels_blocks(mods, L, n_up, mask):
    """x = a + 0i: the real part is the real kernel's rho of a within the bound (each is within n_b eps |M||M|^T of the true sum; the
    chunk differs, so the bits need not be equal) and the imaginary part is zero exactly: every product has a zero factor"""
    capi, _ = mods
    ctx = capi.Context()
    a = rr.vector(L, n_up)
    R, Z = _operator(capi, ctx, L, n_up, complex_states=False), _operator(capi, ctx, L, n_up)
    br, bz = capi.Basis(ctx, R, a.size, 1), capi.Basis(ctx, Z, a.size, 1)
    br.upload(capi.VEC_COL(0), a)
    bz.upload(capi.VEC_COL(0), a.astype(np.complex128))
    real, cplx = br.spin_rdm(capi.VEC_COL(0), mask), bz.spin_rdm_z(capi.VEC_COL(0), mask)
    for (k, r), (kz, z), (_, _, bound) in zip(real, cplx, rr.rdm(L, n_up, a, mask)):
        assert k == kz and not z.imag.any()
        assert np.all(np.abs(z.real.astype(rr.LD) - r.astype(rr.LD)) <= 2 * bound)
    for h in (br, bz, R, Z, ctx):
        h.close()


STEPS = 20


def _live(capi):
    """(live device allocations, their bytes) of the library"""
    v = [C.c_int64() for _ in range(3)]
    assert capi.lib().eigenex_debug_allocations(*[C.byref(x) for x in v]) == 0
    return v[0].value, v[1].value


def _run(capi, interrupt):
    """alpha, beta, the counters, the basis columns and both work vectors after STEPS step calls of a complex state at (12,6) from
    a fixed start vector; interrupt: two batches with the reduced density matrix of column 3 taken in between, else one batch"""
    L, n_up, n = 12, 6, 924
    ctx = capi.Context()
    S = capi.Csr.spin_half_sector(ctx, L, n_up, sr.chain(L, periodic=True), complex_states=True)
    b = capi.Basis(ctx, S, n, STEPS + 2)
    b.upload(capi.VEC_W, er.vector_z(L, n_up, seed=5))
    blocks = None
    if interrupt:
        b.lanczos_enqueue(STEPS // 2)
        blocks = b.spin_rdm_z(capi.VEC_COL(3), 0b000000111111)
        b.lanczos_enqueue(STEPS - STEPS // 2)
    else:
        b.lanczos_enqueue(STEPS)
    st, alpha, beta = b.lanczos_state()
    out = dict(alpha=alpha, beta=beta, state=np.array([st.nvec, st.iterations, st.nalpha, st.nbeta, st.stopped, st.calls_true]),
               V=np.stack([b.download(capi.VEC_COL(c)) for c in range(st.nvec)]), W=b.download(capi.VEC_W), v=b.download(capi.VEC_V))
    for h in (b, S, ctx):
        h.close()
    return out, blocks


def test_a_complex_lanczos_run_does_not_notice_a_call(mods):
    capi, _ = mods
    whole, _ = _run(capi, False)
    cut, blocks = _run(capi, True)
    assert whole["state"].tolist()[0] == STEPS and whole["V"].shape == (STEPS, 924) and whole["V"].dtype == np.complex128
    for key in ("alpha", "beta", "state", "V", "W", "v"):
        assert whole[key].tobytes() == cut[key].tobytes(), key
    # column 3 is a unit vector
    assert [k for k, _ in blocks] == list(range(7)) and abs(sum(float(np.trace(m).real) for _, m in blocks) - 1.0) < 1e-12


def test_refusals(mods):
    capi, _ = mods
    ctx = capi.Context()
    L, n_up, n = 6, 3, 20
    lib = capi.lib()
    rowptr, col, val = capi.spin_sector_csr(L, n_up, sr.chain(L))
    A = capi.Csr.upload(ctx, n, rowptr, col, val.astype(np.complex128), column_blocks=0)
    ba = capi.Basis(ctx, A, n, 1)
    assert ba.is_complex
    bh = capi.Basis(ctx, None, n, 1, dtype=np.complex128)
    bh.set_host_operator(lambda v: v)
    R = _operator(capi, ctx, L, n_up, complex_states=False)
    brl = capi.Basis(ctx, R, n, 1)
    brl.upload(capi.VEC_COL(0), np.ones(n))
    S = _operator(capi, ctx, L, n_up)
    bs = capi.Basis(ctx, S, n, 2)
    x = np.arange(1.0, n + 1) * (1 - 0.5j)
    bs.upload(capi.VEC_COL(0), x)
    big = [(_operator(capi, ctx, LL, nu), LL, nu, mask) for LL, nu, mask in ((14, None, 0x1FFF), (16, 8, 0x7FFF))]
    bigb = [capi.Basis(ctx, T, rr.rows(LL, nu), 1) for T, LL, nu, _ in big]
    out = np.full(80, -7.0)
    dp = out.ctypes.data_as(capi._dp)
    live = _live(capi)

    # the state: CSR-backed, behind a host callback, real (the message names the real entry point)
    with pytest.raises(capi.EigenexError, match="eigenex_spin_rdm_z: the operator of this state is not a matrix-free spin operator"):
        ba.spin_rdm_z(capi.VEC_COL(0), 3)
    assert lib.eigenex_spin_rdm_z(ba.h, 0, 3, dp, 40) == -4  # EIGENEX_ERR_STATE
    with pytest.raises(capi.EigenexError, match="host callback") as e:
        bh.spin_rdm_z(capi.VEC_COL(0), 3)
    assert str(e.value).count("eigenex_spin_rdm_z: ") == 1 and lib.eigenex_spin_rdm_z(bh.h, 0, 3, dp, 40) == -4
    with pytest.raises(capi.EigenexError, match="eigenex_spin_rdm_z: complex states only") as e:
        brl.spin_rdm_z(capi.VEC_COL(0), 0b000111)
    assert re.search(r"eigenex_spin_rdm(?!_)", str(e.value))  # it names the real entry point
    assert lib.eigenex_spin_rdm_z(brl.h, 0, 0b000111, dp, 40) == -4
    # the subsystem
    for word, mask in (("zero", 0), ("outside", 1 << 6), ("leaves no site out", 63)):
        with pytest.raises(capi.EigenexError, match=word) as e:
            bs.spin_rdm_z(capi.VEC_COL(0), mask)
        assert str(e.value).count("eigenex_spin_rdm_z: ") == 1
        assert lib.eigenex_spin_rdm_z(bs.h, 0, mask, dp, 40) == -1  # EIGENEX_ERR_ARG
    # a block above 4096 rows: nA = 13 in the full space at L = 14, nA = 15 at (16, 8)
    for bt, (_, _, _, mask) in zip(bigb, big):
        with pytest.raises(capi.EigenexError, match="eigenex_spin_rdm_z: a block of the reduced density matrix has more than 4096 rows"):
            bt.spin_rdm_z(capi.VEC_COL(0), mask)
        assert lib.eigenex_spin_rdm_z(bt.h, 0, mask, dp, 40) == -1
    # a wrong out_len, either way (20 is the real call's length); NULL out; a bad vector reference
    _, dims, offs = capi.spin_rdm_layout(L, n_up, 0b000111)
    assert dims == [1, 3, 3, 1] and offs[-1] == 20
    for wrong in (20, 39, 41, 0):
        assert lib.eigenex_spin_rdm_z(bs.h, 0, 0b000111, dp, wrong) == -1 and "out_len" in lib.eigenex_last_error().decode()
    assert lib.eigenex_spin_rdm_z(bs.h, 0, 0b000111, None, 40) == -1 and "out is NULL" in lib.eigenex_last_error().decode()
    with pytest.raises(capi.EigenexError, match="bad vector reference"):
        bs.spin_rdm_z(capi.VEC_COL(2), 0b000111)
    # no refused call touched out or left an allocation behind
    assert np.all(out == -7.0) and _live(capi) == live
    assert lib.eigenex_spin_rdm_z(bs.h, 0, 0b000111, dp, 40) == 0 and np.all(out[40:] == -7.0) and not np.any(out[:40:2] == -7.0)
    assert _live(capi) == live  # nor did the call that ran
    # any vector reference will do; nothing above changed the vector
    bs.upload(capi.VEC_W, x)
    one, two = bs.spin_rdm_z(capi.VEC_W, 0b000111), bs.spin_rdm_z(capi.VEC_COL(0), 0b000111)
    assert all(p.tobytes() == q.tobytes() for (_, p), (_, q) in zip(one, two))
    assert bs.download(capi.VEC_COL(0)).tobytes() == x.tobytes()
    for h in bigb + [T for T, _, _, _ in big] + [bs, ba, bh, brl, S, R, A, ctx]:
        h.close()


def _entropy_two_sites(Jxy, t):
    c2, s2 = np.cos(Jxy * t / 2) ** 2, np.sin(Jxy * t / 2) ** 2
    return float(-c2 * np.log(c2) - s2 * np.log(s2))


def test_two_sites_closed_form(mods):
    """S_A(t) = -c^2 ln c^2 - s^2 ln s^2 at three times, the last t = pi / (2 Jxy) where S = ln 2; the tolerance 2 (-delta ln delta),
    delta = 100 k eps after k calls, is derived in the module's docstring"""
    capi, solver = mods
    ctx = capi.Context()
    Jz, Jxy = 0.6, 1.3
    te = solver.SpinTimeEvolutionSolver().setModel(ctx, 2, [(0, 1, Jz, Jxy)], n_up=1).setProductState(0b01)
    assert te.info() == "Success" and te.entanglementEntropy(1) == 0.0 and te.entanglementEntropy([1]) == 0.0
    for k, t_want in enumerate((0.4, 1.1, pi / (2 * Jxy)), start=1):
        assert te.evolve(t_want - te.time()) == 1 and te.info() == "Success" and te.errorBound() == 0.0
        t = te.time()
        delta = 100 * k * EPS
        tol = 2 * (-delta * log(delta))
        got, want = te.entanglementEntropy(1), _entropy_two_sites(Jxy, t)
        print(f"t = {t:.6f}: S = {got:.16f}, closed form {want:.16f}, difference {abs(got - want):.3e}, tolerance {tol:.3e}")
        assert abs(got - want) <= tol and abs(te.entanglementEntropy([1]) - want) <= tol  # the other site: the same entropy
        lam = te.entanglementSpectrum([0])
        assert lam.shape == (2,) and abs(lam.sum() - 1.0) <= 4 * EPS and abs(lam[0] - max(np.cos(Jxy * t / 2) ** 2, np.sin(Jxy * t / 2) ** 2)) <= delta
    assert abs(te.time() - pi / (2 * Jxy)) <= 2 * EPS and abs(te.entanglementEntropy(1) - log(2)) <= tol
    te.close()
    ctx.close()


def _quench_solver(solver, ctx):
    L, n_up, bonds, hz, hx, bits = er.QUENCHES[QUENCH]
    te = solver.SpinTimeEvolutionSolver().setModel(ctx, L, bonds, hz, hx, n_up=n_up)
    te.setKrylovDimension(er.QUENCH_M).setTolerance(er.QUENCH_TOL).setProductState(bits)
    assert te.info() == "Success", te.log()
    return te


def _h2(T):
    return 0.0 if T <= 0.0 else float(-T * np.log(T) - (1 - T) * np.log(1 - T))


def test_quench_entropy_against_dense_diagonalisation(mods):
    capi, solver = mods
    L, n_up = er.QUENCHES[QUENCH][:2]
    _, _, dense = er.quench_reference(QUENCH)
    floor = er.quench_floor(QUENCH)
    d = 32
    ctx = capi.Context()
    te, plain = _quench_solver(solver, ctx), _quench_solver(solver, ctx)
    assert te.entanglementEntropy(A10) == 0.0 and te.entanglementEntropy(B10) == 0.0 and te.entanglementRenyi2(A10) == 0.0  # a product state: exactly
    for k in range(er.QUENCH_CALLS):
        assert te.evolve(er.QUENCH_DT) == plain.evolve(er.QUENCH_DT) and te.info() == "Success"
        s_a, s_b, r2, lam = te.entanglementEntropy(A10), te.entanglementEntropy(list(range(5, 10))), te.entanglementRenyi2(A10), te.entanglementSpectrum(A10)
        assert te.info() == "Success", te.log()
        s_ref = rr.entropy(rz.spectrum_z(rz.rho_of_state(L, n_up, dense[k], A10)))
        T = te.totalErrorBound() + floor
        fannes = T * log(d - 1) + _h2(T)
        print(f"call {k}: S(A) = {s_a:.15f}, dense {s_ref:.15f}, difference {abs(s_a - s_ref):.3e}, Fannes-Audenaert {fannes:.3e} + rounding {2 * ROUND_10_5:.3e}; "
              f"S(A) - S(B) = {abs(s_a - s_b):.3e}; renyi2 - (-ln sum lambda^2) = {abs(r2 + log(float((lam ** 2).sum()))):.3e}, bound {8 * d * d * EPS:.3e}")
        assert abs(s_a - s_ref) <= fannes + 2 * ROUND_10_5
        assert abs(s_a - s_b) <= 2 * ROUND_10_5
        assert lam.size == d and np.all(np.diff(lam) <= 0) and lam[-1] >= 0 and abs(lam.sum() - 1.0) <= 2 * d * EPS
        assert abs(r2 + log(float((lam ** 2).sum()))) <= 8 * d * d * EPS
        assert abs(rr.entropy(lam) - s_a) <= d * EPS * max(1.0, s_a)  # the same spectrum
        # the trajectory is the one without the entanglement calls, bit for bit
        assert te.state().tobytes() == plain.state().tobytes()
        assert (te.time(), te.totalErrorBound(), te.operatorApplications()) == (plain.time(), plain.totalErrorBound(), plain.operatorApplications())
    assert s_a > 0.1  # the quench entangles the halves
    # an invalid subsystem is logged, not thrown, and changes nothing
    for bad in (0, (1 << 10) - 1, 1 << 10, [0, 0], [3, 40]):
        assert te.entanglementEntropy(bad) == 0.0 and te.info() == "InvalidInput" and any(l.startswith("ERROR") for l in te.log()), bad
        assert te.entanglementSpectrum(bad).size == 0
    assert te.entanglementEntropy(A10) == s_a and te.info() == "Success" and te.state().tobytes() == plain.state().tobytes()
    for h in (te, plain, ctx):
        h.close()


def test_python_spin_entanglement_solver_with_a_complex_state(mods):
    capi, solver = mods
    L, n_up, bonds = er.QUENCHES[QUENCH][:3]
    x = er.vector_z(L, n_up, seed=17) * 1.5
    ctx = capi.Context()
    Z, R = capi.Csr.spin_half_sector(ctx, L, n_up, bonds, complex_states=True), capi.Csr.spin_half_sector(ctx, L, n_up, bonds)
    se = solver.SpinEntanglementSolver()
    se.setDeviceOperator(Z).setState(x).setSubsystemMask(A10).compute()
    ra = se.results()
    assert ra["info_name"] == "Success", se.log()
    ref = rz.rho_of_state(L, n_up, x, A10)
    lam = rz.spectrum_z(ref)
    s_ref = rr.entropy(lam)
    d = 32
    print(f"S(A) = {ra['entropy']:.15f}, numpy {s_ref:.15f}, difference {abs(ra['entropy'] - s_ref):.3e}, tolerance {2 * ROUND_10_5:.3e}")
    assert [k for k, _ in ra["blocks"]] == list(range(6)) and all(m.dtype == np.complex128 for _, m in ra["blocks"])
    n2 = float(np.vdot(x, x).real)
    assert abs(ra["normSquared"] - n2) <= 2 * x.size * EPS * n2 and abs(sum(float(np.trace(m).real) for _, m in ra["blocks"]) - 1.0) <= 2 * d * EPS
    for (_, m), (_, want) in zip(ra["blocks"], ref):
        assert np.array_equal(m, m.conj().T) and not m.imag.diagonal().any()
        # an entry of the unit-trace block: each part is a sum of 2 n_b products on either side, 2 n_b eps (|M||M|^H) / n2 <= 2 n_b eps
        # each, sqrt 2 for the modulus of the two parts, n_b = 10: 57 eps, and the division
        assert np.abs(m - want / n2).max() <= 60 * EPS
    assert ra["spectrum"].size == d and np.all(np.diff(ra["spectrum"]) <= 0) and ra["spectrum"][-1] >= 0
    assert abs(ra["entropy"] - s_ref) <= 2 * ROUND_10_5
    assert abs(ra["renyi2"] + log(float((ra["spectrum"] ** 2).sum()))) <= 8 * d * d * EPS and abs(se.renyi(2.0) - ra["renyi2"]) <= 8 * d * d * EPS
    sb = solver.SpinEntanglementSolver()
    sb.setDeviceOperator(Z).setState(x).setSubsystem(list(range(5, 10))).compute()
    assert abs(sb.results()["entropy"] - ra["entropy"]) <= 2 * ROUND_10_5
    # a complex state on the operator for real states: InvalidInput, and the log says which operator to build
    bad = solver.SpinEntanglementSolver()
    bad.setDeviceOperator(R).setState(x).setSubsystemMask(A10).compute()
    rb = bad.results()
    assert rb["info_name"] == "InvalidInput" and rb["nblocks"] == 0 and any(l.startswith("ERROR") and "eigenex_spin_sector_upload_z" in l for l in bad.log())
    bad.setState(x.real.copy()).compute()  # and a real state on it works as before
    assert bad.results()["info_name"] == "Success" and all(m.dtype == np.float64 for _, m in bad.results()["blocks"])
    for h in (se, sb, bad, Z, R, ctx):
        h.close()


def test_cpp_program_spin_entanglement_z(tmp_path):
    """tests/cpp/spin_entanglement_z_amd.cpp: both classes in a C++11 user program, built with -Wall -Wextra -Werror: the two-site closed
    form (three calls: delta = 300 eps) and the 10-site quench at t = 1, with the tolerances of the module's docstring"""
    exe = str(tmp_path / "spin_entanglement_z_amd")
    lib = os.path.join(ROOT, "cmpt-eigenex_amd", "lib")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cmpt-eigenex_amd", "include"),
                           os.path.join(ROOT, "tests", "cpp", "spin_entanglement_z_amd.cpp"), "-o", exe, "-L", lib, "-leigenex_hip", "-Wl,-rpath," + lib])
    o = json.loads(subprocess.check_output([exe], timeout=300).decode())
    print(o)
    delta = 300 * EPS
    closed = 2 * (-delta * log(delta))
    assert o["closed_evolution"] <= closed and o["closed_class"] <= closed
    assert abs(o["t_last"] - pi / 2.6) <= 2 * EPS and abs(o["s_last"] - log(2)) <= closed
    _, _, dense = er.quench_reference(QUENCH)
    s_ref = rr.entropy(rz.spectrum_z(rz.rho_of_state(10, 5, dense[3], A10)))
    T = o["total_bound"] + er.quench_floor(QUENCH)
    d = 32
    assert o["s0"] == 0.0 and o["s_mask"] == o["s_list"] and abs(o["s_mask"] - s_ref) <= T * log(d - 1) + _h2(T) + 2 * ROUND_10_5
    assert abs(o["s_mask"] - o["s_complement"]) <= 2 * ROUND_10_5 and abs(o["renyi2"] - o["renyi2_spectrum"]) <= 8 * d * d * EPS
    assert o["eigenvalues"] == d and abs(o["sum"] - 1.0) <= 2 * d * EPS and o["descending"] == 1 and o["untouched"] == 1
    # the class on the downloaded state: the same vector up to the kept norm (1 here), the same kernel
    assert abs(o["class_entropy"] - o["s_mask"]) <= 2 * ROUND_10_5 and abs(o["class_renyi2"] - o["renyi2"]) <= 8 * d * d * EPS
    assert o["class_blocks"] == 6 and abs(o["class_norm2"] - 1.0) <= 1e-12 and abs(o["trace"] - 1.0) <= 2 * d * EPS
    assert o["asymmetry"] == 0.0 and o["diagonal_imag"] == 0.0
    assert (o["real_block_throws"], o["refused_zero"], o["refused_twice"], o["refused_all"], o["refused_no_state"], o["refused_real_operator"], o["still_works"]) == (1,) * 7


@pytest.mark.parametrize("L,mask", [(6, 0b000111), (12, 0b000000111111)])
def test_spectrum_of_a_rho_that_is_tridiagonal_up_to_1e_9_i(mods, L, mask):
    """test_spectrum_of_a_rho_that_is_tridiagonal_up_to_1e_9 of tests/test_gpu_spin_rdm.py with the Hermitian T + E (rr.t_plus_e(d, True): +-1e-9 i beyond the
    sub-diagonal) and its complex Cholesky factor, rho_A = M M^H: d = 8 with an environment of 8 rows, d = 64 with tiles of 64 rows.
    The raw blocks against the long double restatement within the bound of this file; the spectrum of SpinEntanglementSolver against
    numpy.linalg.eigvalsh of the solver's own unit-trace block within delta = (3 n_b + 2 d) eps, the eigenvalue bound of
    rz.entropy_tolerance_z.  small_eigen::hermitian goes through symmetric() on the embedding of order 2d and inherited its skipped
    columns: before the fix the spectrum on the MI355X was off by 3.2e-11 at d = 8 and 9.9e-13 at d = 64, 3600 and 14 times delta;
    it is now off by 5.6e-17 and 4.2e-17."""
    capi, solver = mods
    d = 1 << bin(mask).count("1")
    n_b = (1 << L) // d
    psi = rr.t_plus_e_state(d, True)
    ctx = capi.Context()
    S = _operator(capi, ctx, L, None)
    b = capi.Basis(ctx, S, 1 << L, 1)
    b.upload(capi.VEC_COL(0), psi)
    rz.check_z(f"device_z T + E ({L},{mask:#x})", b.spin_rdm_z(capi.VEC_COL(0), mask), rz.rdm_z(L, None, psi, mask))
    se = solver.SpinEntanglementSolver()
    se.setDeviceOperator(S).setState(psi).setSubsystemMask(mask).compute()
    r = se.results()
    assert r["info_name"] == "Success", se.log()
    (k, block), = r["blocks"]
    assert k == 0 and block.shape == (d, d) and block.dtype == np.complex128 and r["spectrum"].shape == (d,)
    own = np.sort(np.linalg.eigvalsh(block))[::-1]
    delta = (3 * n_b + 2 * d) * EPS
    off = float(np.abs(r["spectrum"] - own).max())
    print(f"d = {d}: spectrum off LAPACK's of the same block by {off:.3e}, delta {delta:.3e}; block off T + E by {np.abs(block - rr.t_plus_e(d, True)).max():.3e}")
    assert own[-1] > 0 and off <= delta
    for h in (se, b, S, ctx):
        h.close()
