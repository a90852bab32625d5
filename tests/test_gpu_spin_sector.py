"""The matrix-free spin-1/2 operator in one sector of fixed magnetisation (eigenex_spin_sector_upload, kernels.hip:
k_spin_sector_spmv) on the device.  The reference for operator outputs is the plain-CSR upload (eigenex_csr_upload_ex,
column_blocks = 0) of eigenex_spin_sector_csr's rows of the same sector: the kernel adds a row's products in that stored
order, so y is compared bit for bit.  Shapes (L, n_up): (4,2); (6,0) and (6,6), the diagonal alone; (13,1); (9,4); (10,5), one
ragged tile; (11,5), two tiles and bonds across the split of the rank tables; (12,6); (31,2), odd L and bit 30; (32,1),
(32,31), (32,2), bit 31; (20,10) with one operator workgroup per CU (722 tiles: the tile loop goes round more than once)."""
import ctypes as C
import json
import os
import subprocess
import sys
from math import comb

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spin_reference as sr  # noqa: E402
import spin_sector_reference as ss  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
SHAPES = [(4, 2), (6, 0), (6, 6), (13, 1), (9, 4), (10, 5), (11, 5), (12, 6), (31, 2), (32, 1), (32, 31), (32, 2), (20, 10)]


@pytest.fixture(scope="module")
def mods():
    from cmpt_eigenex_amd import capi, solver

    assert capi.device_count() >= 1
    return capi, solver


def _models(L, n_up):
    """name -> (n_sites, n_up, bonds, hz)"""
    if L == 20:  # the large shape: one model with every kind of term (bonds on low, middle and top bits, across the split, hz)
        rng = np.random.RandomState(20)
        return {"periodic_fields": (L, n_up, sr.chain(L, 1.0, 0.7, periodic=True) + [(3, 12, 0.4, 0.0), (5, 19, 0.0, 0.6), (9, 10, 0.3, -0.8)], rng.standard_normal(L))}
    full = sr.models(L)
    m = {name: (L, n_up, full[name][1], full[name][2]) for name in ("open", "periodic", "random40", "fields")}
    m["top_bond"] = (L, n_up, [(0, L - 1, 0.9, -1.3)] + sr.chain(L, 0.5, 1.0)[: max(L - 2, 0)], None)
    if (L, n_up) == (11, 5):
        m["b64"] = (L, n_up, sr.random_bonds(L, 64, 64), np.linspace(-1.0, 1.0, L))
    return m


CASES = [(L, n_up, name) for (L, n_up) in SHAPES for name in _models(L, n_up)]


def _pair(capi, ctx, model):
    """the matrix-free handle and the plain-CSR handle of one sector"""
    n_sites, n_up, bonds, hz = model
    n = comb(n_sites, n_up)
    rowptr, col, val = capi.spin_sector_csr(n_sites, n_up, bonds, hz)
    assert rowptr.size == n + 1 and (col.size == 0 or (col.min() >= 0 and col.max() < n))
    S = capi.Csr.spin_half_sector(ctx, n_sites, n_up, bonds, hz)
    A = capi.Csr.upload(ctx, n, rowptr, col, val, column_blocks=0)
    assert S.layout() == "matrix_free_spin_sector" and S.encoding() == "plain"
    assert A.layout() == "csr" and A.encoding() == "plain"
    assert S.info() == dict(n_global=n, n_local=n, nnz_local=0, n_halo_local=0)
    return S, A, n


@pytest.mark.parametrize("L,n_up,name", CASES)
def test_apply_is_bit_identical_to_the_csr_upload(mods, L, n_up, name):
    capi, _ = mods
    ctx = capi.Context()
    S, A, n = _pair(capi, ctx, _models(L, n_up)[name])
    bs, ba = capi.Basis(ctx, S, n, 2), capi.Basis(ctx, A, n, 2)
    if L == 20:
        bs.tune(2, 1, 0)  # 256 workgroups for 722 tiles
    x = np.random.RandomState(L + n_up).standard_normal(n)
    for b in (bs, ba):
        b.upload(capi.VEC_COL(0), x)
    for shift in (0.0, -0.37):
        dots = []
        for b in (bs, ba):
            dots.append(b.apply(capi.VEC_COL(0), capi.VEC_V, shift, want_dot=True))
        ys, ya = bs.download(capi.VEC_V), ba.download(capi.VEC_V)
        assert ys.tobytes() == ya.tobytes(), f"{name} ({L},{n_up}) shift={shift}: {np.count_nonzero(ys != ya)} rows differ, max {np.abs(ys - ya).max():.3e}"
        xl, yl = x.astype(np.longdouble), ys.astype(np.longdouble)
        ref, bound = (xl * yl).sum(), n * EPS * float((np.abs(xl) * np.abs(yl)).sum())
        print(f"{name} ({L},{n_up}) shift={shift}: dot error {abs(float(dots[0] - ref)):.3e}, bound {bound:.3e}")
        assert abs(dots[0] - ref) <= bound
        bs.apply(capi.VEC_COL(0), capi.VEC_COL(1), shift)  # without the dot: the same y
        assert bs.download(capi.VEC_COL(1)).tobytes() == ya.tobytes()
    np.testing.assert_array_equal(bs.download(capi.VEC_COL(0)), x)
    for h in (bs, ba, S, A, ctx):
        h.close()


HEIS12 = (12, sr.chain(12, periodic=True))
E0_HEIS12 = -5.387390917445  # the periodic 12-site Heisenberg ring
# an open XXZ chain in a random longitudinal field: no symmetry but Sz is left, so every level of a sector is simple
XXZ10_HZ = (10, sr.chain(10, 0.8, 1.1), np.random.RandomState(3).standard_normal(10))


def test_lanczos_steps_match_the_csr_backed_state(mods):
    capi, _ = mods
    ctx = capi.Context()
    S, A, n = _pair(capi, ctx, (12, 6, HEIS12[1], None))
    m = 20
    init = np.random.RandomState(5).standard_normal(n)
    out = []
    for op in (S, A):
        b = capi.Basis(ctx, op, n, m + 2)
        b.upload(capi.VEC_W, init)
        b.lanczos_enqueue(m + 1)
        st, alpha, beta = b.lanczos_state()
        assert (st.nvec, st.iterations, st.stopped) == (m + 1, m, 0)
        V = np.stack([b.download(capi.VEC_COL(c)) for c in range(m + 1)])
        out.append((alpha, beta, V))
        b.close()
    print(f"alpha differs by {np.abs(out[0][0] - out[1][0]).max():.3e}, beta by {np.abs(out[0][1] - out[1][1]).max():.3e}")
    np.testing.assert_allclose(out[0][0], out[1][0], rtol=0, atol=5e-11)
    np.testing.assert_allclose(out[0][1], out[1][1], rtol=0, atol=5e-11)
    for _, _, V in out:
        assert np.abs(V @ V.T - np.eye(m + 1)).max() < 1e-12
    for h in (S, A, ctx):
        h.close()


def test_lanczos_solver_lowest_levels_residuals_and_the_full_space_vector(mods):
    """Fixed work (m = 120 steps, full reorthogonalisation) in the sector (10,5) of a chain whose sector levels are simple.  The
    residual bound is that of tests/test_gpu_spin_operator.py: the estimate |beta_{m-1} s_{m-1,e}| of T_m plus the rounding of
    one operator application and one combination of m vectors, (n + m) eps |H|_1.  The ground vector, scattered into the full
    space through eigenex_spin_sector_states, is an eigenvector of the Kronecker Hamiltonian to the same bound."""
    capi, solver = mods
    n_sites, bonds, hz = XXZ10_HZ
    H = ss.dense(n_sites, 5, bonds, hz)
    lam = np.linalg.eigvalsh(H)
    ctx = capi.Context()
    S = capi.Csr.spin_half_sector(ctx, n_sites, 5, bonds, hz)
    n, m = 252, 120
    es = solver.LanczosEigenSolver()
    es.setDeviceOperator(S).set(minIterations=m, maxIterations=m, maxEigenvalues=4, initialVector=solver.default_start_vector(n))
    es.compute()
    r = es.results()
    assert r["iterations"] == m
    np.testing.assert_allclose(r["eigenvalues"], lam[:4], rtol=1e-10, atol=0)
    alpha, beta = r["alpha"], r["beta"]
    T = np.diag(alpha[:m]) + np.diag(beta[: m - 1], 1) + np.diag(beta[: m - 1], -1)
    _, Sm = np.linalg.eigh(T)
    rounding = (n + m) * EPS * np.abs(H).sum(0).max()
    X = r["eigenvectors"]
    for e in range(4):
        true = np.linalg.norm(H @ X[:, e] - r["eigenvalues"][e] * X[:, e])
        est = abs(beta[m - 1] * Sm[m - 1, e])
        print(f"pair {e}: true residual {true:.3e}, estimate {est:.3e}, rounding {rounding:.3e}")
        assert true <= est + rounding
    K = sr.dense_kron(n_sites, bonds, hz, None)
    states = capi.spin_sector_states(n_sites, 5)
    full = np.zeros(1 << n_sites)
    full[states] = X[:, 0]
    true = np.linalg.norm(K @ full - r["eigenvalues"][0] * full)
    bound = abs(beta[m - 1] * Sm[m - 1, 0]) + (n + m) * EPS * np.abs(K).sum(0).max()
    print(f"ground vector in the full space: residual {true:.3e}, bound {bound:.3e}")
    assert true <= bound
    es.close()
    S.close()
    ctx.close()


def test_thick_restart_ground_state_with_a_basis_of_24(mods):
    capi, solver = mods
    n_sites, bonds, hz = XXZ10_HZ
    H = ss.dense(n_sites, 5, bonds, hz)
    lam = np.linalg.eigvalsh(H)
    ctx = capi.Context()
    S = capi.Csr.spin_half_sector(ctx, n_sites, 5, bonds, hz)
    n = 252
    es = solver.ThickRestartLanczosEigenSolver()
    es.setDeviceOperator(S).set(numberOfEigenvalues=1, maxBasisSize=24, tolerance=1e-11, initialVector=solver.default_start_vector(n))
    es.compute()
    r = es.results()
    assert r["info_name"] == "Success" and r["restarts"] >= 1
    assert abs(r["eigenvalues"][0] - lam[0]) <= 1e-10 * abs(lam[0])
    x = r["eigenvectors"][:, 0]
    true = np.linalg.norm(H @ x - r["eigenvalues"][0] * x)
    rounding = (n + 24) * EPS * np.abs(H).sum(0).max()
    print(f"ground state {r['eigenvalues'][0]:.15g} after {r['restarts']} restarts: true residual {true:.3e}, estimate {r['residuals'][0]:.3e}")
    assert true <= r["residuals"][0] + rounding
    es.close()
    S.close()
    ctx.close()


def test_degenerate_levels_are_resolved_sector_by_sector(mods):
    """The point of the sectors.  In the full space the triplet above the singlet ground state of the Heisenberg ring appears
    three times (Sz = -1, 0, 1) and a Krylov space of one start vector sees it once; sector by sector every level asked for
    is simple.  n_up = 6 (Sz = 0) holds the ground state, E_0 = -5.387390917445; the lowest level of n_up = 5 (Sz = -1: the
    triplet) lies strictly above it.  Both against dense eigvalsh of the two sector matrices."""
    capi, solver = mods
    L, bonds = HEIS12
    ctx = capi.Context()
    got, want = {}, {}
    for n_up in (6, 5):
        n = comb(L, n_up)
        want[n_up] = np.linalg.eigvalsh(ss.dense(L, n_up, bonds))[0]
        S = capi.Csr.spin_half_sector(ctx, L, n_up, bonds)
        es = solver.LanczosEigenSolver()
        # a random start vector: the ring is symmetric, and a symmetric start would span one symmetry class only
        es.setDeviceOperator(S).set(minIterations=100, maxIterations=100, maxEigenvalues=1, initialVector=solver.random_vector(1, n))
        es.compute()
        got[n_up] = es.results()["eigenvalues"][0]
        es.close()
        S.close()
    ctx.close()
    print(f"E_0(n_up=6) = {got[6]:.13f}, E_0(n_up=5) = {got[5]:.13f}; dense {want[6]:.13f}, {want[5]:.13f}")
    assert abs(got[6] - E0_HEIS12) < 1e-9 and abs(want[6] - E0_HEIS12) < 1e-9
    assert abs(got[5] - want[5]) <= 1e-10 * abs(want[5]) and abs(got[6] - want[6]) <= 1e-10 * abs(want[6])
    assert got[5] > got[6] + 1e-3 and want[5] > want[6] + 1e-3  # the gap of the 12-site ring is about 0.36


FM_MODEL = (11, 5, sr.random_bonds(11, 40, 77), np.random.RandomState(111).standard_normal(11))


def _range(capi, model):
    rowptr, col, val = capi.spin_sector_csr(*model)
    radius = float(np.add.reduceat(np.abs(val), rowptr[:-1]).max())
    return 0.0, 1.01 * radius


def test_filter_apply_is_bit_identical_to_the_csr_backed_state(mods):
    """the CSR kernel takes the Chebyshev step in its epilogue, the sector kernel stores y and k_cheb_combine follows: t_k is the
    same bits in both forms"""
    capi, _ = mods
    import filter_reference as fr

    ctx = capi.Context()
    S, A, n = _pair(capi, ctx, FM_MODEL)
    c, h = _range(capi, FM_MODEL)
    x = np.random.RandomState(9).standard_normal(n)
    for degree in (1, 2, 7, 24):
        mu = fr.delta_coefficients(-0.3 * h, c, h, degree)
        ys = []
        for op in (S, A):
            b = capi.Basis(ctx, op, n, 2)
            b.upload(capi.VEC_COL(0), x)
            b.set_filter(mu, c, h)
            b.filter_apply(capi.VEC_COL(0), capi.VEC_COL(1))
            ys.append(b.download(capi.VEC_COL(1)))
            b.close()
        assert np.abs(ys[1]).max() > 0 and ys[0].tobytes() == ys[1].tobytes(), degree
    for hd in (S, A, ctx):
        hd.close()


def test_moments_within_the_dot_product_bound(mods):
    """eigenex_kpm_moments on the sector-backed state: the last Chebyshev vector equals the float64 restatement over the CSR rows
    bit for bit, every moment is within the bound of tests/test_gpu_density.py of the long double dots of the restatement's vectors"""
    capi, _ = mods
    import density_reference as dr
    import scipy.sparse as sp
    import test_gpu_density as td

    n = comb(11, 5)
    rowptr, col, val = capi.spin_sector_csr(*FM_MODEL)
    A = sp.csr_matrix((val, col, rowptr), shape=(n, n))
    c, h = _range(capi, FM_MODEL)
    x = np.random.RandomState(19).standard_normal(n)
    ctx = capi.Context()
    S = capi.Csr.spin_half_sector(ctx, *FM_MODEL)
    b = capi.Basis(ctx, S, n, 2)
    b.upload(capi.VEC_COL(0), x)
    ts = dr.chebyshev_vectors(dr.device_matmul(A), x, c, h, dr.applications(65))
    for nm in (1, 2, 3, 4, 5, 64, 65):
        mu = b.kpm_moments(capi.VEC_COL(0), nm, c, h)
        np.testing.assert_array_equal(b.download(capi.VEC_V), ts[dr.applications(nm)])
        td._check_moments("spin sector (11,5)", mu, "spin", ts, nm)
    for hd in (b, S, ctx):
        hd.close()


def _live(capi):
    v = [C.c_int64() for _ in range(3)]
    assert capi.lib().eigenex_debug_allocations(*[C.byref(x) for x in v]) == 0
    return v[0].value, v[1].value


def test_refusals_and_no_allocation_left_behind(mods):
    capi, _ = mods
    n_sites, n_up, bonds, hz = 6, 3, sr.chain(6, 0.8, 1.1), np.random.RandomState(106).standard_normal(6)
    lb = capi.Context(loopback_shards=2)
    before = _live(capi)
    with pytest.raises(capi.EigenexError, match="one shard"):
        capi.Csr.spin_half_sector(lb, n_sites, n_up, bonds, hz)
    assert _live(capi) == before
    lb.close()
    ctx = capi.Context()
    before = _live(capi)
    with pytest.raises(capi.EigenexError, match="transverse"):
        capi.Csr.spin_half_sector(ctx, n_sites, n_up, bonds, hz, hx=[0.0, 0.0, 0.0, 0.3, 0.0, 0.0])
    assert _live(capi) == before
    S = capi.Csr.spin_half_sector(ctx, n_sites, n_up, bonds, hz, hx=np.zeros(6))  # an all-zero transverse field is none
    assert _live(capi)[0] == before[0] + 3  # the model table and the two rank tables are all an operator holds
    assert S.layout() == "matrix_free_spin_sector" and S.info() == dict(n_global=20, n_local=20, nnz_local=0, n_halo_local=0)
    with pytest.raises(capi.EigenexError, match="complex"):
        capi.Basis(ctx, S, 20, 4, dtype=np.complex128)
    assert _live(capi)[0] == before[0] + 3
    b1, b2 = capi.Basis(ctx, S, 20, 4), capi.Basis(ctx, S, 20, 3)
    b1.upload(capi.VEC_W, np.ones(20))
    b1.lanczos_enqueue(3)
    b2.upload(capi.VEC_COL(0), np.ones(20))
    b2.kpm_moments(capi.VEC_COL(0), 8, 0.0, 50.0)  # the streaming path's extra vectors
    for h in (b1, b2, S):
        h.close()
    assert _live(capi) == before
    ctx.close()


def test_cpp_program_spin_sector(tmp_path):
    """tests/cpp/spin_sector_amd.cpp: SpinHalfModel's sector calls and device::spinHalfSectorOperator in a C++11 user program,
    built with -Wall -Wextra"""
    exe = str(tmp_path / "spin_sector_amd")
    lib = os.path.join(ROOT, "cmpt-eigenex_amd", "lib")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cmpt-eigenex_amd", "include"),
                           os.path.join(ROOT, "tests", "cpp", "spin_sector_amd.cpp"), "-o", exe, "-L", lib, "-leigenex_hip", "-Wl,-rpath," + lib])
    o = json.loads(subprocess.check_output([exe, "12", "6"]).decode())
    print(o)
    assert o["sites"] == 12 and o["n_up"] == 6 and o["rows"] == 924 and abs(o["norm"] - 1.0) < 1e-12
    assert abs(o["energy_matrix_free"] - o["energy_csr"]) <= 1e-10 * abs(o["energy_csr"])
    assert abs(o["energy_matrix_free"] - E0_HEIS12) < 1e-9
    # converged to 1e-13 in the eigenvalue: the residual is about its square root times the spectral width, far below 1e-5
    assert o["residual"] < 1e-5 and o["first_state"] == 63 and o["last_state"] == 4032
