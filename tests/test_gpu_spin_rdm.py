"""The reduced density matrix on the device (eigenex_spin_rdm, kernels.hip: k_spin_rdm<SECTOR, TILE> and k_spin_rdm_reduce)
against the long double restatement of tests/spin_rdm_reference.py, within |out - ref| <= n_b eps (|M_k| |M_k|^T) elementwise
-- the rounding of an n_b-term sum in any grouping, so it holds for every launch grid, slice count and tile size.  The shapes
are the smallest at which the kernels can still go wrong.  Full space: L = 3 (everything ragged), 6 (contiguous and interleaved
deposit), 10 with nA = 6 (exactly one 64-tile) and nA = 7 (three tile pairs: the off-diagonal tile and the mirror), 17 with
A = {0, 16} (the 16-tile, 2^15 b's, the state tuned to many workgroups so that the b range is sliced) and with nA = 7 including
site 16.  Sectors: (4,2) (blocks of 1, 2, 1), (6,0) and (6,6) (one row), (10,5) across the split of the rank tables, (11,5),
(12,6) with nA = 7 (kmin = 1), (32,2) with nA = 14 including sites 30 and 31 (d = 91: a ragged second tile), (32,31), (20,10)
with nA = 9 (d = 126, 462 b's) and with nA = 2 sliced, (14,7) with nA = 12 (d = 924: 120 tile pairs of at most 2 b's).  On every
shape: the bound, (i, j) and (j, i) bitwise equal, two calls bitwise equal, the vector unchanged.  Then a Lanczos run that does not
notice a call between its batches, the refusals, the ground state of the 12-ring end to end through SpinEntanglementSolver,
and the C++ class in a user program."""
import json
import os
import subprocess
import sys
from math import comb, log

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spin_rdm_reference as rr  # noqa: E402
import spin_reference as sr  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E0_HEIS12 = -5.387390917445  # the periodic 12-site Heisenberg ring

# (n_sites, n_up or None, mask_a, tuned to 16 workgroups per CU)
SHAPES = [
    (3, None, 0b010, False),
    (6, None, 0b000111, False),
    (6, None, 0b101010, False),
    (10, None, 0b0000111111, False),
    (10, None, 0b1011011101, False),
    (17, None, (1 << 16) | 1, True),
    (17, None, (1 << 16) | 0b10011000110010, False),
    (4, 2, 0b0011, False),
    (6, 0, 0b000101, False),
    (6, 6, 0b000101, False),
    (10, 5, 0b0001111000, False),
    (11, 5, 0b10100100011, False),
    (12, 6, 0b111111100000, False),
    (32, 2, 0xC0000FFF, False),
    (32, 31, 0x80000005, False),
    (20, 10, 0b10000000111100110101, False),
    (20, 10, (1 << 19) | (1 << 3), True),
    (14, 7, 0x0FFF, False),
]


@pytest.fixture(scope="module")
def mods():
    from cmpt_eigenex_amd import capi, solver

    assert capi.device_count() >= 1
    return capi, solver


def _operator(capi, ctx, L, n_up, bonds=None):
    bonds = sr.chain(L, 1.0, 0.7, periodic=True) if bonds is None else bonds
    return capi.Csr.spin_half(ctx, L, bonds) if n_up is None else capi.Csr.spin_half_sector(ctx, L, n_up, bonds)


def test_the_shapes_are_what_they_claim():
    """the block dimensions the docstring names, from math.comb alone (no GPU work): a typing error in a mask would test less"""
    dims = {}
    for L, n_up, mask, _ in SHAPES:
        nA, nB, _, ks = rr.geometry(L, n_up, mask)
        dims[(L, n_up, mask)] = [1 << nA] if n_up is None else [comb(nA, k) for k in ks]
    assert dims[(10, None, 0b0000111111)] == [64] and dims[(10, None, 0b1011011101)] == [128]
    assert dims[(17, None, (1 << 16) | 1)] == [4] and dims[(17, None, (1 << 16) | 0b10011000110010)] == [128]
    assert dims[(4, 2, 0b0011)] == [1, 2, 1] and dims[(6, 0, 0b000101)] == [1] and dims[(6, 6, 0b000101)] == [1]
    assert dims[(12, 6, 0b111111100000)] == [7, 21, 35, 35, 21, 7]
    assert dims[(32, 2, 0xC0000FFF)] == [1, 14, 91] and dims[(32, 31, 0x80000005)] == [3, 1]
    assert max(dims[(20, 10, 0b10000000111100110101)]) == 126 and comb(11, 6) == 462
    assert dims[(20, 10, (1 << 19) | (1 << 3))] == [1, 2, 1] and dims[(14, 7, 0x0FFF)] == [792, 924, 792]


@pytest.mark.parametrize("L,n_up,mask,tuned", SHAPES)
def test_device_blocks_equal_the_restatement_within_the_bound(mods, L, n_up, mask, tuned):
    capi, _ = mods
    ctx = capi.Context()
    S = _operator(capi, ctx, L, n_up)
    n = rr.rows(L, n_up)
    b = capi.Basis(ctx, S, n, 2)
    if tuned:
        b.tune(2, 16, 0)  # as many workgroups as the operator has tiles: the b range of the small blocks is cut into slices
    x = rr.vector(L, n_up)
    b.upload(capi.VEC_COL(1), x)
    got = b.spin_rdm(capi.VEC_COL(1), mask)
    rr.check(f"device ({L},{n_up},{mask:#x})", got, rr.rdm(L, n_up, x, mask))  # the bound, and (i, j) = (j, i) bit for bit
    again = b.spin_rdm(capi.VEC_COL(1), mask)
    assert [k for k, _ in again] == [k for k, _ in got] and all(p.tobytes() == q.tobytes() for (_, p), (_, q) in zip(got, again))
    assert b.download(capi.VEC_COL(1)).tobytes() == x.tobytes()
    # the trace is sum x^2: n terms in some grouping on either side
    trace = sum(float(np.trace(m)) for _, m in got)
    assert abs(trace - float(x @ x)) <= 2 * n * rr.EPS * float(x @ x)
    kf, dims, offs = capi.spin_rdm_layout(L, n_up, mask)
    assert [k for k, _ in got] == [kf + i for i in range(len(dims))] and [m.shape[0] for _, m in got] == dims
    for h in (b, S, ctx):
        h.close()


STEPS = 20


def _run(capi, interrupt):
    """alpha, beta, the counters, the basis columns and both work vectors after STEPS step calls at (12,6) from a fixed start
    vector; interrupt: two batches with the reduced density matrix of column 3 taken in between, else one batch"""
    L, n_up, n = 12, 6, 924
    ctx = capi.Context()
    S = capi.Csr.spin_half_sector(ctx, L, n_up, sr.chain(L, periodic=True))
    b = capi.Basis(ctx, S, n, STEPS + 2)
    b.upload(capi.VEC_W, np.random.RandomState(5).standard_normal(n))
    blocks = None
    if interrupt:
        b.lanczos_enqueue(STEPS // 2)
        blocks = b.spin_rdm(capi.VEC_COL(3), 0b000000111111)
        b.lanczos_enqueue(STEPS - STEPS // 2)
    else:
        b.lanczos_enqueue(STEPS)
    st, alpha, beta = b.lanczos_state()
    out = dict(alpha=alpha, beta=beta, state=np.array([st.nvec, st.iterations, st.nalpha, st.nbeta, st.stopped, st.calls_true]),
               V=np.stack([b.download(capi.VEC_COL(c)) for c in range(st.nvec)]), W=b.download(capi.VEC_W), v=b.download(capi.VEC_V))
    for h in (b, S, ctx):
        h.close()
    return out, blocks


def test_a_lanczos_run_does_not_notice_a_call(mods):
    capi, _ = mods
    whole, _ = _run(capi, False)
    cut, blocks = _run(capi, True)
    assert whole["state"].tolist()[0] == STEPS and whole["V"].shape == (STEPS, 924)
    for key in ("alpha", "beta", "state", "V", "W", "v"):
        assert whole[key].tobytes() == cut[key].tobytes(), key
    # column 3 is a unit vector
    assert [k for k, _ in blocks] == list(range(7)) and abs(sum(float(np.trace(m)) for _, m in blocks) - 1.0) < 1e-12


def test_refusals(mods):
    capi, _ = mods
    ctx = capi.Context()
    L, n_up, n = 6, 3, 20
    rowptr, col, val = capi.spin_sector_csr(L, n_up, sr.chain(L))
    A = capi.Csr.upload(ctx, n, rowptr, col, val, column_blocks=0)
    ba = capi.Basis(ctx, A, n, 1)
    ba.upload(capi.VEC_COL(0), np.ones(n))
    with pytest.raises(capi.EigenexError, match="eigenex_spin_rdm: the operator of this state is not a matrix-free spin operator"):
        ba.spin_rdm(capi.VEC_COL(0), 3)
    assert capi.lib().eigenex_spin_rdm(ba.h, 0, 3, None, 0) == -4  # EIGENEX_ERR_STATE
    bh = capi.Basis(ctx, None, n, 1)
    bh.set_host_operator(lambda v: v)
    with pytest.raises(capi.EigenexError, match="host callback"):
        bh.spin_rdm(capi.VEC_COL(0), 3)
    S = _operator(capi, ctx, L, n_up)
    bs = capi.Basis(ctx, S, n, 2)
    x = np.arange(1.0, n + 1)
    bs.upload(capi.VEC_COL(0), x)
    for word, mask in (("zero", 0), ("outside", 1 << 6), ("leaves no site out", 63)):
        with pytest.raises(capi.EigenexError, match=word) as e:
            bs.spin_rdm(capi.VEC_COL(0), mask)
        assert str(e.value).count("eigenex_spin_rdm: ") == 1
    # a block above 4096 rows: nA = 13 in the full space at L = 14, nA = 15 at (16, 8)
    for LL, nu, mask in ((14, None, 0x1FFF), (16, 8, 0x7FFF)):
        T = _operator(capi, ctx, LL, nu)
        bt = capi.Basis(ctx, T, rr.rows(LL, nu), 1)
        with pytest.raises(capi.EigenexError, match="eigenex_spin_rdm: a block of the reduced density matrix has more than 4096 rows"):
            bt.spin_rdm(capi.VEC_COL(0), mask)
        assert capi.lib().eigenex_spin_rdm(bt.h, 0, mask, None, 0) == -1  # EIGENEX_ERR_ARG
        bt.close()
        T.close()
    # a wrong out_len, either way; NULL out; a bad vector reference
    out = np.full(40, -7.0)
    dp = out.ctypes.data_as(capi._dp)
    _, dims, offs = capi.spin_rdm_layout(L, n_up, 0b000111)
    assert dims == [1, 3, 3, 1] and offs[-1] == 20
    for wrong in (19, 21, 0):
        assert capi.lib().eigenex_spin_rdm(bs.h, 0, 0b000111, dp, wrong) == -1 and "out_len" in capi.lib().eigenex_last_error().decode()
    assert capi.lib().eigenex_spin_rdm(bs.h, 0, 0b000111, None, 20) == -1 and "out is NULL" in capi.lib().eigenex_last_error().decode()
    assert np.all(out == -7.0)
    with pytest.raises(capi.EigenexError, match="bad vector reference"):
        bs.spin_rdm(capi.VEC_COL(2), 0b000111)
    assert capi.lib().eigenex_spin_rdm(bs.h, 0, 0b000111, dp, 20) == 0 and np.all(out[20:] == -7.0) and not np.any(out[:20] == -7.0)
    # any vector reference will do; nothing above changed the vector
    bs.upload(capi.VEC_W, x)
    one, two = bs.spin_rdm(capi.VEC_W, 0b000111), bs.spin_rdm(capi.VEC_COL(0), 0b000111)
    assert all(p.tobytes() == q.tobytes() for (_, p), (_, q) in zip(one, two))
    assert bs.download(capi.VEC_COL(0)).tobytes() == x.tobytes()
    for h in (bs, ba, bh, S, A, ctx):
        h.close()


def test_ground_state_of_the_ring_end_to_end(mods):
    """LanczosEigenSolver on the sector (12,6) of the Heisenberg ring (120 steps: the ground vector is converged far below the
    margins), S of A = sites 0..5 through SpinEntanglementSolver against numpy.linalg.eigvalsh of the restatement's rho.  The
    tolerance is derived: by Weyl an eigenvalue of the unit-trace rho moves by at most ||Delta||_F <= n_b eps (Cauchy-Schwarz on
    the elementwise bound), the eigen-solver adds d eps, and |x ln x - y ln y| <= -delta ln delta, so |Delta S| <= d (-delta ln
    delta) with delta = (n_b + d) eps, d = 64 eigenvalues and n_b = 20 b's at most.  S(A) = S(complement) twice that (two
    computed entropies).  renyi2() = -ln sum lambda^2: sum lambda^2 >= 1/d moves by at most 2 sum lambda (d eps) = 2 d eps from the
    eigenvalues and by d^2 eps relative from the d^2-term sum of squares, so the logarithms differ by at most 4 d^2 eps."""
    capi, solver = mods
    L, n_up, n = 12, 6, 924
    A, B = 0b000000111111, 0b111111000000
    ctx = capi.Context()
    S = _operator(capi, ctx, L, n_up, sr.chain(L, periodic=True))
    es = solver.LanczosEigenSolver()
    es.setDeviceOperator(S).set(minIterations=120, maxIterations=120, maxEigenvalues=1, initialVector=solver.random_vector(1, n))
    es.compute()
    r = es.results()
    E0, x = r["eigenvalues"][0], np.ascontiguousarray(r["eigenvectors"][:, 0])
    assert abs(E0 - E0_HEIS12) < 1e-9
    se = solver.SpinEntanglementSolver()
    se.setDeviceOperator(S).setState(x).setSubsystem([0, 1, 2, 3, 4, 5]).compute()
    ra = se.results()
    assert ra["info_name"] == "Success", se.log()
    assert [k for k, _ in ra["blocks"]] == list(range(7)) and [m.shape[0] for _, m in ra["blocks"]] == [comb(6, k) for k in range(7)]
    ref = rr.rdm(L, n_up, x, A)
    lam = rr.spectrum([(k, m.astype(np.float64)) for k, m, _ in ref])
    d, n_b = 64, 20
    tol = rr.entropy_tolerance(d, n_b)
    s_ref = rr.entropy(lam)
    sc = solver.SpinEntanglementSolver()
    sc.setDeviceOperator(S).setState(x).setSubsystemMask(B).compute()
    rb = sc.results()
    r2 = -log(float((ra["spectrum"] ** 2).sum()))
    print(f"E0 = {E0:.13f}, S(A) = {ra['entropy']:.15f}, reference {s_ref:.15f}, difference {abs(ra['entropy'] - s_ref):.3e}, bound {tol:.3e}; "
          f"S(A) - S(B) = {abs(ra['entropy'] - rb['entropy']):.3e}; renyi2 = {ra['renyi2']:.15f}, -ln sum lambda^2 = {r2:.15f}, "
          f"difference {abs(ra['renyi2'] - r2):.3e}, bound {4 * d * d * rr.EPS:.3e}")
    assert ra["spectrum"].size == 64 and np.all(np.diff(ra["spectrum"]) <= 0) and ra["spectrum"][-1] >= 0
    assert abs(ra["normSquared"] - 1.0) < 1e-12 and abs(sum(float(np.trace(m)) for _, m in ra["blocks"]) - 1.0) < 1e-13
    assert abs(ra["entropy"] - s_ref) <= tol
    assert abs(ra["entropy"] - rb["entropy"]) <= 2 * tol
    assert abs(ra["renyi2"] - r2) <= 4 * d * d * rr.EPS
    assert 0.5 < ra["entropy"] < 6 * log(2)  # the singlet ground state is entangled across the cut
    assert abs(se.renyi(2.0) - ra["renyi2"]) <= 4 * d * d * rr.EPS and se.schmidtRank(1e-14) <= 64
    # invalid input is logged, not thrown
    bad = solver.SpinEntanglementSolver()
    bad.setDeviceOperator(S).setState(x).setSubsystem([0, 0]).compute()
    assert bad.results()["info_name"] == "InvalidInput" and any(l.startswith("ERROR") for l in bad.log())
    for h in (se, sc, bad, es, S, ctx):
        h.close()


def test_cpp_program_spin_entanglement(tmp_path):
    """tests/cpp/spin_entanglement_amd.cpp: SpinEntanglementSolver in a C++11 user program, built with -Wall -Wextra -Werror: the
    same ring.  The margins: the entropy tolerance derived above for S(A) = S(complement); the state went in scaled by 3."""
    exe = str(tmp_path / "spin_entanglement_amd")
    lib = os.path.join(ROOT, "cmpt-eigenex_amd", "lib")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cmpt-eigenex_amd", "include"),
                           os.path.join(ROOT, "tests", "cpp", "spin_entanglement_amd.cpp"), "-o", exe, "-L", lib, "-leigenex_hip", "-Wl,-rpath," + lib])
    o = json.loads(subprocess.check_output([exe, "12"]).decode())
    print(o)
    tol = rr.entropy_tolerance(64, 20)
    assert o["sites"] == 12 and o["n_up"] == 6 and o["rows"] == 924 and o["info"] == 1 and abs(o["energy"] - E0_HEIS12) < 1e-9
    assert o["blocks"] == [[k, comb(6, k)] for k in range(7)] and o["eigenvalues"] == 64
    assert (o["sites_seen"], o["n_up_seen"], o["mask"]) == (12, 6, 63)
    assert abs(o["trace"] - 1.0) < 1e-13 and o["asymmetry"] == 0.0 and abs(o["norm2"] - 9.0) < 1e-9
    assert abs(o["entropy"] - o["entropy_complement"]) <= 2 * tol and 0.5 < o["entropy"] < 6 * log(2)
    assert abs(o["renyi2"] - o["renyi2_spectrum"]) <= 4 * 64 * 64 * rr.EPS
    assert o["renyi_half"] >= o["entropy"] - 1e-12 >= o["renyi2"] - 2e-12  # the Renyi entropies decrease with alpha
    assert abs(o["renyi_near_one"] - o["entropy"]) < 1e-4 and 1 <= o["schmidt_rank"] <= 64 and 0 < o["largest"] < 1
    assert (o["refused_csr"], o["refused_empty"], o["refused_twice"], o["refused_length"], o["refused_no_operator"], o["refused_all"], o["no_result_throws"]) == (1,) * 7
    assert o["uniform_info"] == 1 and o["uniform_blocks"] == 2 and abs(o["uniform_entropy"] - log(2)) < 1e-12


@pytest.mark.parametrize("L,mask", [(6, 0b000111), (12, 0b000000111111)])
def test_spectrum_of_a_rho_that_is_tridiagonal_up_to_1e_9(mods, L, mask):
    """Full space, A = the low half of the sites: d = 8 with an environment of 8 rows, d = 64 with tiles of 64 rows.  The state is
    psi[a + d e] = M[a, e] with M the Cholesky factor of rr.t_plus_e(d), so rho_A = M M^T is tridiagonal plus entries of 1e-9 of the
    sub-diagonal: the columns on which small_eigen::symmetric decides whether a Householder step is needed.  The raw blocks
    against M M^T in long double within the bound of this file; the spectrum of SpinEntanglementSolver against
    numpy.linalg.eigvalsh of the solver's own unit-trace block within delta = (n_b + d) eps, the eigenvalue bound of
    rr.entropy_tolerance (the n_b part is not even needed: both sides start from the same block).  Before symmetric() summed the
    column tail directly it skipped every one of these columns without zeroing it, and on the MI355X the spectrum was off by
    7.3e-11 at d = 8 and 9.0e-12 at d = 64 -- 20000 and 315 times delta; it is now off by 2.8e-17 and 4.5e-17."""
    capi, solver = mods
    d = 1 << bin(mask).count("1")
    n_b = (1 << L) // d
    psi = rr.t_plus_e_state(d)
    ctx = capi.Context()
    S = _operator(capi, ctx, L, None)
    b = capi.Basis(ctx, S, 1 << L, 1)
    b.upload(capi.VEC_COL(0), psi)
    rr.check(f"device T + E ({L},{mask:#x})", b.spin_rdm(capi.VEC_COL(0), mask), rr.rdm(L, None, psi, mask))
    se = solver.SpinEntanglementSolver()
    se.setDeviceOperator(S).setState(psi).setSubsystemMask(mask).compute()
    r = se.results()
    assert r["info_name"] == "Success", se.log()
    (k, block), = r["blocks"]
    assert k == 0 and block.shape == (d, d) and r["spectrum"].shape == (d,)
    own = np.sort(np.linalg.eigvalsh(block))[::-1]
    delta = (n_b + d) * float(rr.EPS)
    off = float(np.abs(r["spectrum"] - own).max())
    print(f"d = {d}: spectrum off LAPACK's of the same block by {off:.3e}, delta {delta:.3e}; block off T + E by {np.abs(block - rr.t_plus_e(d)).max():.3e}")
    assert own[-1] > 0 and off <= delta
    for h in (se, b, S, ctx):
        h.close()
