"""Chebyshev filter on the device (eigenex_basis_set_filter / eigenex_filter_apply, the filtered Lanczos step driver) and
FilteredLanczosEigenSolver against the numpy restatement tests/filter_reference.py, the Lanczos oracle and LAPACK."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_reference as fr  # noqa: E402
from oracle import krylov_oracle as ko  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
DEGREES = (1, 2, 3, 40)
TAU = 0.3


@pytest.fixture(scope="module")
def capi():
    from cmpt_eigenex_amd import capi as c

    assert c.device_count() >= 1
    return c


def _laplacian_csr(n):
    from oracle import cref

    import scipy.sparse as sp

    rp, cl, vl = cref.laplacian3d(n)
    A = sp.csr_matrix((vl, cl, rp), shape=(n ** 3, n ** 3))
    A.sort_indices()
    return A


def _block_operator():
    """a small Hermitian block operator: sectors 5, 7, 4 with a dense diagonal block each and one coupled pair"""
    rng = np.random.RandomState(5)
    sizes = [5, 7, 4]
    blocks = {}
    for q, s in enumerate(sizes):
        B = rng.standard_normal((s, s))
        blocks[(q, q)] = B + B.T
    C01 = rng.standard_normal((5, 7))
    blocks[(0, 1)], blocks[(1, 0)] = C01, C01.T.copy()
    return sizes, blocks


_INPUTS = {}


def _input(name):
    """(scipy CSR, how to put it on the device) -- built once per module"""
    if name not in _INPUTS:
        if name == "chain1000":
            _INPUTS[name] = fr.anderson_chain(1000)
        elif name in ("chain257", "chain257_blocked"):
            _INPUTS[name] = fr.anderson_chain(257)
        elif name == "laplacian12":
            _INPUTS[name] = _laplacian_csr(12)
        elif name == "ztridiagonal":
            _INPUTS[name] = fr.hermitian_tridiagonal(300)
        elif name == "blocks":
            import scipy.sparse as sp

            sizes, blocks = _block_operator()
            off = np.concatenate([[0], np.cumsum(sizes)])
            D = np.zeros((off[-1], off[-1]))
            for (r, c), B in blocks.items():
                D[off[r]:off[r + 1], off[c]:off[c + 1]] = B
            A = sp.csr_matrix(D)
            A.sort_indices()
            _INPUTS[name] = A
    return _INPUTS[name]


def _upload(capi, ctx, name):
    A = _input(name)
    n = A.shape[0]
    if name == "laplacian12":
        return capi.Csr.laplacian3d(ctx, 12)
    if name == "chain257_blocked":
        return capi.Csr.upload(ctx, n, A.indptr, A.indices, A.data, column_blocks=2)
    if name == "blocks":
        sizes, blocks = _block_operator()
        return capi.Csr.upload_blocks(ctx, sizes, sizes, blocks)
    return capi.Csr.upload(ctx, n, A.indptr, A.indices, A.data)


def _filter_of(A, degree, tau=TAU):
    lo, hi = fr.gershgorin(A)
    c, h = 0.5 * (lo + hi), 0.5 * (hi - lo) * 1.01
    return fr.delta_coefficients(tau, c, h, degree), c, h


# The peak sits where the input has spectrum: at 0.3 the 12^3 Laplacian (band 0..12, few levels at its lower edge) gives the
# oracle's own Lanczos run on p(A) betas that fall from 2e-1 to 2e-4 within 20 steps -- a nearly invariant subspace, in which
# rounding decides the later coefficients and no two implementations agree to 1e-12; at the band centre they stay in [0.20, 0.31].
_TARGET = {"laplacian12": 6.0}
_REFS = {}


def _reference(name, degree):
    """x, p(A) x in long double and the float64 restatement's own error against it -- computed once, shared"""
    key = (name, degree)
    if key not in _REFS:
        A = _input(name)
        n = A.shape[0]
        cplx = np.iscomplexobj(A.data)
        rng = np.random.RandomState(17)
        x = rng.standard_normal(n) + (1j * rng.standard_normal(n) if cplx else 0.0)
        mu, c, h = _filter_of(A, degree, _TARGET.get(name, TAU))
        y64 = fr.apply_filter(fr.csr_rowsum_matmul(A.indptr, A.indices, A.data, A.data.dtype), x, mu, c, h)
        ld = np.clongdouble if cplx else np.longdouble
        yld = fr.apply_filter(fr.csr_rowsum_matmul(A.indptr, A.indices, A.data, ld), x.astype(ld), mu, c, h)
        _REFS[key] = (x, mu, c, h, yld, float(np.abs(y64.astype(ld) - yld).max()))
    return _REFS[key]


@pytest.mark.parametrize("shards", [1, 2, 3])
@pytest.mark.parametrize("name", ["chain1000", "chain257", "laplacian12", "chain257_blocked", "ztridiagonal", "blocks"])
def test_filter_apply_against_long_double(capi, name, shards):
    """device error <= 4 x the float64 restatement's own error against long double + 4 eps sum|mu| |x|_inf (the factor 4: another
    row-sum order)"""
    ctx = capi.Context(loopback_shards=shards) if shards > 1 else capi.Context()
    A = _upload(capi, ctx, name)
    n = _input(name).shape[0]
    b = capi.Basis(ctx, A, n, 3)
    for degree in DEGREES:
        x, mu, c, h, yld, err64 = _reference(name, degree)
        b.set_filter(mu, c, h)
        b.upload(capi.VEC_COL(0), x)
        b.filter_apply(capi.VEC_COL(0), capi.VEC_V)
        y = b.download(capi.VEC_V)
        err = float(np.abs(y.astype(yld.dtype) - yld).max())
        bound = 4 * err64 + 4 * EPS * np.abs(mu).sum() * np.abs(x).max()
        print(f"{name} shards={shards} degree={degree}: device error {err:.3e}, float64 restatement {err64:.3e}, bound {bound:.3e}")
        assert err <= bound
        np.testing.assert_array_equal(b.download(capi.VEC_COL(0)), x)  # the input is left alone
    b.close()
    A.close()
    ctx.close()


def _run_steps(capi, b, init, ncalls):
    b.clear()
    b.upload(capi.VEC_W, init)
    b.lanczos_enqueue(ncalls)
    st, alpha, beta = b.lanczos_state()
    return st, alpha, beta


def _set_filter_form(monkeypatch, b, form, mu, c, h):
    if form == "composed":
        monkeypatch.setenv("EIGENEX_NO_FUSED_FILTER", "1")
    else:
        monkeypatch.delenv("EIGENEX_NO_FUSED_FILTER", raising=False)
    b.set_filter(mu, c, h)  # the variable is read here


def _counted_filter_apply(capi, ctx, b, x):
    """y = p(A) x and the number of launches booked as operator work for it"""
    b.upload(capi.VEC_COL(0), x)
    ctx.profile_enable(True)
    ctx.profile_reset()
    b.filter_apply(capi.VEC_COL(0), capi.VEC_V)
    launches = ctx.profile_get(capi.K_SPMV)[0]
    ctx.profile_enable(False)
    return b.download(capi.VEC_V), launches


@pytest.mark.parametrize("name", ["chain1000", "chain257", "laplacian12"])
def test_fused_and_composed_paths_give_the_same_bits(capi, name, monkeypatch):
    """and the fused path is the one taken: one operator launch per degree on these one-pass real CSR inputs (plain and
    row-coded), against the operator and k_cheb_combine per degree of the composed path"""
    degree = 40
    ctx = capi.Context()
    A = _upload(capi, ctx, name)
    assert A.encoding() == ("row_codes" if name == "laplacian12" else "plain")
    n = _input(name).shape[0]
    b = capi.Basis(ctx, A, n, 14)
    x, mu, c, h, _, _ = _reference(name, degree)
    out = {}
    for form in ("fused", "composed"):
        _set_filter_form(monkeypatch, b, form, mu, c, h)
        y, launches = _counted_filter_apply(capi, ctx, b, x)
        assert launches == (degree if form == "fused" else 2 * degree)
        st, alpha, beta = _run_steps(capi, b, x, 12)
        assert st.nvec == 12 and st.stopped == 0
        out[form] = (y, alpha, beta)
    for u, v in zip(out["fused"], out["composed"]):
        np.testing.assert_array_equal(u, v)
    b.close()
    A.close()
    ctx.close()


@pytest.mark.parametrize("name", ["chain1000", "chain257"])
def test_fused_path_follows_the_cache_policy_knob(capi, name, monkeypatch):
    """eigenex_basis_tune's bit 1 (non-temporal val/col streams) selects another instantiation of the plain CSR kernels, of the
    fused one too: the same bits as the composed path under that policy and as the default policy, one launch per degree"""
    degree = 40
    ctx = capi.Context()
    A = _upload(capi, ctx, name)
    n = _input(name).shape[0]
    b = capi.Basis(ctx, A, n, 3)
    x, mu, c, h, _, _ = _reference(name, degree)
    _set_filter_form(monkeypatch, b, "fused", mu, c, h)
    y_default, _ = _counted_filter_apply(capi, ctx, b, x)
    b.tune(flags=2)
    out = {}
    for form in ("fused", "composed"):
        _set_filter_form(monkeypatch, b, form, mu, c, h)
        out[form], launches = _counted_filter_apply(capi, ctx, b, x)
        assert launches == (degree if form == "fused" else 2 * degree)
    np.testing.assert_array_equal(out["fused"], out["composed"])
    np.testing.assert_array_equal(out["fused"], y_default)
    b.close()
    A.close()
    ctx.close()


@pytest.mark.parametrize("shards", [1, 2])
@pytest.mark.parametrize("name", ["chain257", "laplacian12"])
def test_filtered_lanczos_steps_against_the_oracle(capi, name, shards):
    degree, ncalls = 40, 20
    Asp = _input(name)
    n = Asp.shape[0]
    x, mu, c, h, _, _ = _reference(name, degree)
    matmul = fr.csr_rowsum_matmul(Asp.indptr, Asp.indices, Asp.data, np.float64)
    bo = ko.LanczosBaseOracle()
    bo.matmul = lambda v: fr.apply_filter(matmul, v, mu, c, h)
    bo.matrix_height = n
    bo.initial_vector = x
    for _ in range(ncalls):
        assert bo.update_lanczos_steps()
    assert min(bo.beta) > 0.1 * max(bo.beta)  # a well-conditioned recurrence (see _TARGET)
    ctx = capi.Context(loopback_shards=shards) if shards > 1 else capi.Context()
    A = _upload(capi, ctx, name)
    b = capi.Basis(ctx, A, n, ncalls + 1)
    b.set_filter(mu, c, h)
    ctx.trace(True)
    st, alpha, beta = _run_steps(capi, b, x, ncalls)
    ops = ctx.trace_get()
    assert (st.nvec, st.nalpha, st.nbeta, st.stopped) == (ncalls, ncalls, ncalls - 1, 0)
    print(f"{name} shards={shards}: max |alpha - oracle| {np.abs(alpha - bo.alpha).max():.3e}, |beta - oracle| {np.abs(beta - bo.beta).max():.3e}")
    np.testing.assert_allclose(alpha, bo.alpha, rtol=0, atol=1e-12)
    np.testing.assert_allclose(beta, bo.beta, rtol=0, atol=1e-12)
    halos = sum(1 for op, _ in ops if op == capi.COLL_HALO)
    assert halos == (degree * ncalls if shards > 1 else 0)  # one neighbour exchange per degree and application
    for k in range(ncalls):
        np.testing.assert_allclose(b.download(capi.VEC_COL(k)), bo.lanczosvectors[k], rtol=0, atol=1e-10)
    b.close()
    A.close()
    ctx.close()


def test_recorded_batches_follow_the_filter(capi):
    name = "laplacian12"
    ctx = capi.Context()
    A = _upload(capi, ctx, name)
    n = _input(name).shape[0]
    b = capi.Basis(ctx, A, n, 8)
    x, mu, c, h, _, _ = _reference(name, 3)
    b.set_filter(mu, c, h)
    first = _run_steps(capi, b, x, 6)
    again = _run_steps(capi, b, x, 6)
    assert b.graph_info()["graphs"] >= 1
    np.testing.assert_array_equal(first[1], again[1])
    np.testing.assert_array_equal(first[2], again[2])
    mu2 = mu * np.linspace(1.0, 2.0, mu.size)
    b.set_filter(mu2, c, h)
    assert b.graph_info()["graphs"] == 0
    other = _run_steps(capi, b, x, 6)
    matmul = fr.csr_rowsum_matmul(_input(name).indptr, _input(name).indices, _input(name).data, np.float64)
    u0 = x / np.linalg.norm(x)
    np.testing.assert_allclose(other[1][0], u0 @ fr.apply_filter(matmul, u0, mu2, c, h), rtol=0, atol=1e-12)
    assert abs(other[1][0] - first[1][0]) > 1e-3
    b.close()
    A.close()
    ctx.close()


def test_errors_leave_the_state_usable(capi):
    name = "chain257"
    Asp = _input(name)
    n = Asp.shape[0]
    ctx = capi.Context()
    x, mu, c, h, _, _ = _reference(name, 3)
    hb = capi.Basis(ctx, None, n, 4)
    hb.set_host_operator(lambda v: Asp @ v)
    with pytest.raises(capi.EigenexError):
        hb.set_filter(mu, c, h)  # a filter needs a device operator
    st, a_host, _ = _run_steps(capi, hb, x, 3)
    assert st.nvec == 3
    hb.close()
    A = _upload(capi, ctx, name)
    b = capi.Basis(ctx, A, n, 8)
    plain = _run_steps(capi, b, x, 6)
    np.testing.assert_allclose(plain[1][:3], a_host, rtol=0, atol=1e-12)
    for bad in (dict(mu=mu, center=c, halfwidth=0.0), dict(mu=mu, center=c, halfwidth=-1.0), dict(mu=mu, center=c, halfwidth=h, degree=-1),
                dict(mu=None, center=c, halfwidth=h, degree=2)):
        with pytest.raises(capi.EigenexError):
            b.set_filter(**bad)
    with pytest.raises(capi.EigenexError):
        b.filter_apply(capi.VEC_COL(0), capi.VEC_V)  # no filter set
    b.set_filter(mu, c, h)
    b.clear()
    b.upload(capi.VEC_W, x)
    with pytest.raises(capi.EigenexError):
        b.arnoldi_enqueue(2)
    b.configure(0.25, 1e-12, 1, capi.ORTHO_BATCHED)
    with pytest.raises(capi.EigenexError):
        b.lanczos_enqueue(2)
    with pytest.raises(capi.EigenexError):
        b.filter_apply(capi.VEC_COL(0), capi.VEC_W)
    b.configure(0.0, 1e-12, 1, capi.ORTHO_BATCHED)
    filtered = _run_steps(capi, b, x, 6)
    assert filtered[0].nvec == 6 and abs(filtered[1][0] - plain[1][0]) > 1e-3
    b.set_filter(None)
    after = _run_steps(capi, b, x, 6)
    np.testing.assert_array_equal(after[1], plain[1])  # plain Lanczos as before any filter
    np.testing.assert_array_equal(after[2], plain[2])
    b.close()
    A.close()
    ctx.close()


def _solve(capi, Asp, ctx, dtype, tau, degree, m, nev, init, **kw):
    from cmpt_eigenex_amd import solver

    n = Asp.shape[0]
    A = capi.Csr.upload(ctx, n, Asp.indptr, Asp.indices, Asp.data)
    es = solver.FilteredLanczosEigenSolver(dtype)
    es.setDeviceOperator(A)
    es.set(numberOfEigenvalues=nev, maxBasisSize=m, target=tau, filterDegree=degree, spectralRange=fr.gershgorin(Asp), initialVector=init, **kw)
    es.compute()
    r = es.results()
    log = es.log()
    es.close()
    A.close()
    return r, log


def _check_pairs(Asp, r, tau, nev):
    want = fr.nearest(Asp, tau, nev)
    X = r["eigenvectors"]
    true_res = np.array([np.linalg.norm(Asp @ X[:, e] - r["eigenvalues"][e] * X[:, e]) for e in range(nev)])
    print("eigenvalue error %.3e, true residuals %.3e (reported %.3e), restarts %d, applications %d" %
          (np.abs(r["eigenvalues"] - want).max(), true_res.max(), r["residuals"].max(), r["restarts"], r["operatorApplications"]))
    assert r["info_name"] == "Success" and r["neig"] == nev
    np.testing.assert_allclose(r["eigenvalues"], want, rtol=0, atol=1e-9)
    assert true_res.max() <= 1e-6 and r["residuals"].max() <= 1e-6
    np.testing.assert_allclose(r["residuals"], true_res, rtol=0, atol=1e-10)
    assert np.all(np.diff(np.abs(r["eigenvalues"] - tau)) >= 0)
    np.testing.assert_allclose(np.linalg.norm(X, axis=0), 1.0, atol=1e-12)
    for e in range(nev):
        z = X[np.flatnonzero(X[:, e])[0], e]
        assert abs(np.imag(z)) < 1e-13 and np.real(z) > 0


def test_solver_anderson_chain(capi):
    """residual 1e-10 in p over a p-gap of about 1e-2 gives an angle of 1e-8; times |A|, with a margin: 1e-6; the
    restatement reaches 1e-14 / 1e-15"""
    Asp = _input("chain1000")
    init = np.random.RandomState(11).standard_normal(1000)
    ctx = capi.Context()
    r, _ = _solve(capi, Asp, ctx, np.float64, TAU, 200, 60, 4, init)
    _check_pairs(Asp, r, TAU, 4)
    ctx.close()


def test_solver_anderson_grid_on_two_shards(capi):
    Asp = fr.anderson3d()
    init = np.random.RandomState(11).standard_normal(Asp.shape[0])
    ctx = capi.Context(loopback_shards=2)
    r, _ = _solve(capi, Asp, ctx, np.float64, TAU, 100, 60, 4, init)
    _check_pairs(Asp, r, TAU, 4)
    ctx.close()


def test_solver_with_restarts(capi):
    """m = 24 on the 6 x 7 x 8 model, degree 100: the restatement needs four restarts and converges"""
    Asp = fr.anderson3d()
    n = Asp.shape[0]
    init = np.random.RandomState(11).standard_normal(n)
    lo, hi = fr.gershgorin(Asp)
    ref = fr.filtered_lanczos(lambda x: Asp @ x, n, init, TAU, lo, hi, 100, 4, 24)
    print("restatement: restarts %d, eigenvalue error %.3e, residuals %.3e" % (ref["restarts"], np.abs(ref["eigenvalues"] - fr.nearest(Asp, TAU, 4)).max(), ref["residuals"].max()))
    assert ref["restarts"] >= 2 and ref["log"] == ["converged"]
    np.testing.assert_allclose(ref["eigenvalues"], fr.nearest(Asp, TAU, 4), rtol=0, atol=1e-9)
    ctx = capi.Context()
    r, log = _solve(capi, Asp, ctx, np.float64, TAU, 100, 24, 4, init)
    assert r["restarts"] >= 2 and "INFO      thick-restart lanczos converged with tolerance" in log
    _check_pairs(Asp, r, TAU, 4)
    ctx.close()


def test_solver_complex_hermitian(capi):
    Asp = _input("ztridiagonal")
    rng = np.random.RandomState(11)
    init = rng.standard_normal(300) + 1j * rng.standard_normal(300)
    ctx = capi.Context()
    r, _ = _solve(capi, Asp, ctx, np.complex128, TAU, 200, 60, 4, init)
    _check_pairs(Asp, r, TAU, 4)
    ctx.close()


def test_cpp_program_filtered_lanczos(tmp_path):
    """tests/cpp/filtered_lanczos_amd.cpp: the class as a C++11 user program on the Anderson chain"""
    exe = str(tmp_path / "filtered_lanczos_amd")
    lib = os.path.join(ROOT, "cmpt-eigenex_amd", "lib")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cmpt-eigenex_amd", "include"),
                           os.path.join(ROOT, "tests", "cpp", "filtered_lanczos_amd.cpp"), "-o", exe, "-L", lib, "-leigenex_hip", "-Wl,-rpath," + lib])
    Asp = _input("chain1000")
    diag = tmp_path / "diag.txt"
    np.savetxt(diag, Asp.diagonal(), fmt="%.17g")
    out = json.loads(subprocess.check_output([exe, str(diag), "0.3", "200", "60", "4"], timeout=120).decode())
    want = fr.nearest(Asp, 0.3, 4)
    print("C++ program: eigenvalue error %.3e, residuals %.3e" % (np.abs(np.array(out["eigenvalues"]) - want).max(), max(out["residuals"])))
    assert out["info"] == 0
    np.testing.assert_allclose(out["eigenvalues"], want, rtol=0, atol=1e-9)
    assert max(out["residuals"]) <= 1e-6
    assert out["invalid_without_range"] == 3
