"""The matrix-free spin-1/2 operator (eigenex_spin_upload, kernels.hip: k_spin_spmv) on the device.  The reference for
operator outputs is the plain-CSR upload (eigenex_csr_upload_ex, column_blocks = 0) of eigenex_spin_csr's rows of the same
model: the kernel adds a row's products in that stored order, so y is compared bit for bit.  Shapes: L = 3 and 6 (one ragged
tile), 8 (exactly one tile, every flip inside it), 9 (the top bit crosses tiles), 11, and 17 with one operator workgroup
per CU (512 tiles: the tile loop goes round more than once)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spin_reference as sr  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def mods():
    from cmpt_eigenex_amd import capi, solver

    assert capi.device_count() >= 1
    return capi, solver


def _models(L):
    m = dict(sr.models(L))
    m["top_bond"] = (L, [(0, L - 1, 0.9, -1.3)] + sr.chain(L, 0.5, 1.0)[: max(L - 2, 0)], None, None)
    if L == 11:
        m["b64"] = (L, sr.random_bonds(L, 64, 64), None, np.linspace(-1.0, 1.0, L))
    if L == 17:  # the large shape: one model with every kind of term (bonds on low, middle and top bits, both fields)
        rng = np.random.RandomState(17)
        m = {"periodic_fields": (L, sr.chain(L, 1.0, 0.7, periodic=True) + [(3, 12, 0.4, 0.0), (5, 16, 0.0, 0.6)], rng.standard_normal(L),
                                 np.where(np.arange(L) % 3 == 0, rng.standard_normal(L), 0.0))}
    return m


CASES = [(L, name) for L in (3, 6, 8, 9, 11, 17) for name in _models(L)]


def _pair(capi, ctx, model):
    """the matrix-free handle and the plain-CSR handle of one model"""
    n_sites, bonds, hz, hx = model
    rowptr, col, val = capi.spin_csr(n_sites, bonds, hz, hx)
    S = capi.Csr.spin_half(ctx, n_sites, bonds, hz, hx)
    A = capi.Csr.upload(ctx, 1 << n_sites, rowptr, col, val, column_blocks=0)
    assert S.layout() == "matrix_free_spin" and S.encoding() == "plain"
    assert A.layout() == "csr" and A.encoding() == "plain"
    assert S.info() == dict(n_global=1 << n_sites, n_local=1 << n_sites, nnz_local=0, n_halo_local=0)
    return S, A


@pytest.mark.parametrize("L,name", CASES)
def test_apply_is_bit_identical_to_the_csr_upload(mods, L, name):
    capi, _ = mods
    ctx = capi.Context()
    S, A = _pair(capi, ctx, _models(L)[name])
    n = 1 << L
    bs, ba = capi.Basis(ctx, S, n, 2), capi.Basis(ctx, A, n, 2)
    if L == 17:
        bs.tune(2, 1, 0)  # 256 workgroups for 512 tiles
    x = np.random.RandomState(L).standard_normal(n)
    for b in (bs, ba):
        b.upload(capi.VEC_COL(0), x)
    for shift in (0.0, -0.37):
        dots = []
        for b in (bs, ba):
            dots.append(b.apply(capi.VEC_COL(0), capi.VEC_V, shift, want_dot=True))
        ys, ya = bs.download(capi.VEC_V), ba.download(capi.VEC_V)
        assert ys.tobytes() == ya.tobytes(), f"{name} L={L} shift={shift}: {np.count_nonzero(ys != ya)} rows differ, max {np.abs(ys - ya).max():.3e}"
        xl, yl = x.astype(np.longdouble), ys.astype(np.longdouble)
        ref, bound = (xl * yl).sum(), n * EPS * float((np.abs(xl) * np.abs(yl)).sum())
        print(f"{name} L={L} shift={shift}: dot error {abs(float(dots[0] - ref)):.3e}, bound {bound:.3e}")
        assert abs(dots[0] - ref) <= bound
        bs.apply(capi.VEC_COL(0), capi.VEC_COL(1), shift)  # without the dot: the same y
        assert bs.download(capi.VEC_COL(1)).tobytes() == ya.tobytes()
    np.testing.assert_array_equal(bs.download(capi.VEC_COL(0)), x)
    for h in (bs, ba, S, A, ctx):
        h.close()


HEIS10 = (10, sr.chain(10, periodic=True), None, None)
# no symmetry left, so no degenerate level: a Krylov space of one start vector holds one vector per eigenspace, and "the four
# lowest eigenvalues" of the full spectrum can only be asked of a solver where every level is simple
XXZ10_FIELDS = (10, sr.chain(10, 0.8, 1.1), np.random.RandomState(3).standard_normal(10), np.random.RandomState(4).standard_normal(10))


def test_lanczos_steps_match_the_csr_backed_state(mods):
    capi, _ = mods
    ctx = capi.Context()
    S, A = _pair(capi, ctx, HEIS10)
    n, m = 1024, 20
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


def _dense(model):
    n_sites, bonds, hz, hx = model
    return sr.dense_kron(n_sites, bonds, hz, hx)


def test_lanczos_solver_lowest_levels_and_residuals(mods):
    """Fixed work (m = 120 steps, full reorthogonalisation) on a chain without degenerate levels.  The solver's estimate of a
    Ritz pair's residual is |beta_j s_je| (last component of the tridiagonal eigenvector times the coupling to the next vector);
    the series it returns end with beta_{m-1}, so the estimate is formed for T_m and the true residual of the returned vectors
    (Ritz vectors of T_{m+1}, whose pairs are no worse once converged) is held to it plus the rounding of one operator
    application and one combination of m vectors, (n + m) eps |H|_1."""
    capi, solver = mods
    H = _dense(XXZ10_FIELDS)
    lam = np.linalg.eigvalsh(H)
    ctx = capi.Context()
    S = capi.Csr.spin_half(ctx, *XXZ10_FIELDS)
    n, m = 1024, 120
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
    es.close()
    S.close()
    ctx.close()


def test_thick_restart_ground_state_with_a_basis_of_24(mods):
    capi, solver = mods
    H = _dense(XXZ10_FIELDS)
    lam = np.linalg.eigvalsh(H)
    ctx = capi.Context()
    S = capi.Csr.spin_half(ctx, *XXZ10_FIELDS)
    n = 1024
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


def _range(model):
    rowptr, col, val = sr.rows_csr(*model)
    radius = float(np.add.reduceat(np.abs(val), rowptr[:-1]).max())
    return 0.0, 1.01 * radius


def test_filter_apply_is_bit_identical_to_the_csr_backed_state(mods):
    """the CSR kernel takes the Chebyshev step in its epilogue, the spin kernel stores y and k_cheb_combine follows: t_k is the
    same bits in both forms"""
    capi, _ = mods
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import filter_reference as fr

    model = sr.models(9)["random40_fields"]
    ctx = capi.Context()
    S, A = _pair(capi, ctx, model)
    n = 512
    c, h = _range(model)
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
    """eigenex_kpm_moments on the spin-backed state: the last Chebyshev vector equals the float64 restatement over the CSR rows bit
    for bit, every moment is within the bound of tests/test_gpu_density.py of the long double dots of the restatement's vectors"""
    capi, _ = mods
    import density_reference as dr
    import scipy.sparse as sp
    import test_gpu_density as td

    model = sr.models(9)["random40_fields"]
    n = 512
    rowptr, col, val = capi.spin_csr(*model)
    A = sp.csr_matrix((val, col, rowptr), shape=(n, n))
    c, h = _range(model)
    x = np.random.RandomState(19).standard_normal(n)
    ctx = capi.Context()
    S = capi.Csr.spin_half(ctx, *model)
    b = capi.Basis(ctx, S, n, 2)
    b.upload(capi.VEC_COL(0), x)
    ts = dr.chebyshev_vectors(dr.device_matmul(A), x, c, h, dr.applications(65))
    for nm in (1, 2, 3, 4, 5, 64, 65):
        mu = b.kpm_moments(capi.VEC_COL(0), nm, c, h)
        np.testing.assert_array_equal(b.download(capi.VEC_V), ts[dr.applications(nm)])
        td._check_moments("spin L=9", mu, "spin", ts, nm)
    for hd in (b, S, ctx):
        hd.close()


def _live(capi):
    v = [C.c_int64() for _ in range(3)]
    assert capi.lib().eigenex_debug_allocations(*[C.byref(x) for x in v]) == 0
    return v[0].value, v[1].value


def test_refusals_and_no_allocation_left_behind(mods):
    capi, _ = mods
    model = sr.models(6)["fields"]
    lb = capi.Context(loopback_shards=2)
    before = _live(capi)
    with pytest.raises(capi.EigenexError, match="one shard"):
        capi.Csr.spin_half(lb, *model)
    assert _live(capi) == before
    lb.close()
    ctx = capi.Context()
    before = _live(capi)
    S = capi.Csr.spin_half(ctx, *model)
    assert _live(capi)[0] == before[0] + 1  # the table is all an operator holds
    with pytest.raises(capi.EigenexError, match="complex"):
        capi.Basis(ctx, S, 64, 4, dtype=np.complex128)
    assert _live(capi)[0] == before[0] + 1
    b1, b2 = capi.Basis(ctx, S, 64, 4), capi.Basis(ctx, S, 64, 3)
    b1.upload(capi.VEC_W, np.ones(64))
    b1.lanczos_enqueue(3)
    b2.upload(capi.VEC_COL(0), np.ones(64))
    b2.kpm_moments(capi.VEC_COL(0), 8, 0.0, 50.0)  # the streaming path's extra vectors
    for h in (b1, b2, S):
        h.close()
    assert _live(capi) == before
    ctx.close()


def test_cpp_program_spin_chain(tmp_path):
    """tests/cpp/spin_chain_amd.cpp: SpinHalfModel and device::spinHalfOperator in a C++11 user program, built with -Wall -Wextra"""
    exe = str(tmp_path / "spin_chain_amd")
    lib = os.path.join(ROOT, "cmpt-eigenex_amd", "lib")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cmpt-eigenex_amd", "include"),
                           os.path.join(ROOT, "tests", "cpp", "spin_chain_amd.cpp"), "-o", exe, "-L", lib, "-leigenex_hip", "-Wl,-rpath," + lib])
    o = json.loads(subprocess.check_output([exe, "12"]).decode())
    print(o)
    assert o["sites"] == 12 and o["rows"] == 4096 and abs(o["norm"] - 1.0) < 1e-12
    assert abs(o["energy_matrix_free"] - o["energy_csr"]) <= 1e-10 * abs(o["energy_csr"])
    assert abs(o["energy_matrix_free"] + 5.387390917445) < 1e-9  # the periodic 12-site Heisenberg ring, E_0 = -5.387390917445...
    # converged to 1e-13 in the eigenvalue: the residual is about its square root times the spectral width, far below 1e-5
    assert o["residual"] < 1e-5
