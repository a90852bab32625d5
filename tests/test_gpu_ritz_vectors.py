"""Ritz vectors and Krylov combinations against the extended-precision reference (tests/ritz_reference.py).

k_ritz<8, true> (X = V S and the column norms), k_ritz<16, false> (the thick-restart combination), k_ritz_combine (complex
coefficients), k_first_nonzero / k_scale_columns and the host's ritz_finish (phase and normalisation, lanczos.hpp:806-816,
arnoldi.hpp:854-865) are compared entry by entry with rr.bound:
  a. constructed bases: local row counts around the 4-row / 4096-entry chunks, odd local sizes, 1-8 loopback shards,
     every coefficient chunking (8 real, 4 complex per pass, nvec unrolled by 4), host strides, phase and scale edges,
     eigenex_krylov_combine raw;
  b. bases the step kernels wrote (odd local sizes: the padding rows must stay zero);
  c. the thick-restart combination;
  d. the BASELINE sizes (128^3 Lanczos, 10^6 x 32 Arnoldi, 512^3 Lanczos).
All inputs are seeded."""
import time

import numpy as np
import pytest

from oracle import cref
from oracle import krylov_oracle as ko
from tests import ritz_reference as rr

pytestmark = pytest.mark.gpu

U = rr.U


@pytest.fixture(scope="module")
def capi():
    from cmpt_eigenex_amd import capi as m

    assert m.device_count() >= 1
    return m


def _ctx(capi, shards):
    return capi.Context(loopback_shards=shards) if shards > 1 else capi.Context()


def _identity(capi, ctx, n, cplx):
    rp = np.arange(n + 1, dtype=np.int32)
    return capi.Csr.upload(ctx, n, rp, np.arange(n, dtype=np.int32), np.ones(n, np.complex128 if cplx else np.float64))


def _rand(rng, shape, cplx):
    x = rng.standard_normal(shape)
    return x + 1j * rng.standard_normal(shape) if cplx else x


def _check(X, V, S, raw=False, where=""):
    """X (device) against the reference of V S: entry-wise bound; the first non-zero entry: same index, same sign,
    |imag| <= 4u.  Returns the reference."""
    x_ld = rr.combine(V, S)
    ref = x_ld.astype(np.complex128 if np.iscomplexobj(x_ld) else np.float64) if raw else rr.finish(x_ld)
    assert X.shape == ref.shape, where
    assert not np.isnan(X).any(), where
    factors = None if raw else [rr.norm_factor(x_ld[:, e]) for e in range(ref.shape[1])]
    tol = rr.bound(V, S, ref, raw=raw, factors=factors)
    bad = np.argwhere(np.abs(X - ref) > tol)
    assert bad.size == 0, f"{where}: {len(bad)} entries outside the bound, first {bad[0]}: {X[tuple(bad[0])]} vs {ref[tuple(bad[0])]}"
    if not raw:
        for e in range(ref.shape[1]):
            i = rr.first_hit(ref[:, e])
            assert rr.first_hit(X[:, e]) == i, (where, e)
            if i >= 0:
                assert np.sign(np.real(X[i, e])) == np.sign(np.real(ref[i, e])) != 0, (where, e)
                assert abs(np.imag(X[i, e])) <= 4 * U, (where, e)
    return ref


# ---- a. constructed bases --------------------------------------------------------------------------------------------
SIZES = [1, 2, 3, 1023, 1024, 1025, 2049, 4097 * 16 + 1]
SHARDS = [1, 2, 3, 8]
CASES = [(n, p) for n in SIZES for p in SHARDS if p <= n]
CAP = 12


def _basis(capi, n, shards, cplx, seed, cap=CAP):
    rng = np.random.default_rng(seed)
    ctx = _ctx(capi, shards)
    A = _identity(capi, ctx, n, cplx)
    b = capi.Basis(ctx, A, n, cap)
    V = _rand(rng, (cap, n), cplx)
    for c in range(cap):
        b.upload(capi.VEC_COL(c), V[c])
    return ctx, b, V, rng


@pytest.mark.parametrize("n, shards", CASES)
def test_real_coefficients_every_chunking(capi, n, shards):
    """real S on a real basis: nvec across the unroll by 4, nev across the 8-column passes; host strides"""
    ctx, b, V, rng = _basis(capi, n, shards, False, 100 + n + shards)
    for nvec in (0, 1, 3, 4, 5, 9, CAP):
        for nev in (1, 7, 8, 9, 16, 17):
            S = rng.standard_normal((nvec, nev))
            _check(b.ritz_vectors(nvec, S), V, S, where=f"nvec={nvec} nev={nev}")
    # lds > nvec (NaN rows behind S must not be read) and ldx > n_rows (the gap rows must not be written)
    S = rng.standard_normal((5, 9))
    X = b.ritz_vectors(5, S, lds=8, ldx=n + 5)
    _check(X, V, S, where="strides")
    assert X.base is not None and X.base.shape == (n + 5, 9) and np.isnan(X.base[n:]).all()
    ctx.close()


@pytest.mark.parametrize("n, shards", CASES)
@pytest.mark.parametrize("cplx_basis", [False, True])
def test_complex_coefficients_and_complex_basis(capi, n, shards, cplx_basis):
    """complex S on a real and on a complex basis (4 columns per pass), real S on a complex basis"""
    ctx, b, V, rng = _basis(capi, n, shards, cplx_basis, 200 + n + shards + cplx_basis)
    for nvec in (1, 4, 5, CAP):
        for nev in (1, 3, 4, 5, 8, 9):
            S = _rand(rng, (nvec, nev), True)
            _check(b.ritz_vectors(nvec, S), V, S, where=f"complex S nvec={nvec} nev={nev}")
    if cplx_basis:
        for nvec, nev in ((3, 9), (CAP, 17)):
            S = rng.standard_normal((nvec, nev))
            _check(b.ritz_vectors(nvec, S), V, S, where=f"real S nvec={nvec} nev={nev}")
    S = _rand(rng, (7, 5), True)
    X = b.ritz_vectors(7, S, lds=11, ldx=n + 3)
    _check(X, V, S, where="complex strides")
    assert np.isnan(X.base[n:]).all()
    ctx.close()


@pytest.mark.parametrize("n, shards", [(3, 1), (1025, 3), (2049, 2), (4097 * 16 + 1, 1), (4097 * 16 + 1, 8)])
@pytest.mark.parametrize("cplx", [False, True])
def test_krylov_combine_raw(capi, n, shards, cplx):
    """eigenex_krylov_combine: V C as it is, real and complex C, ncols across 4 and 8"""
    ctx, b, V, rng = _basis(capi, n, shards, cplx, 300 + n + shards + cplx)
    for ncols in (1, 3, 4, 5, 8, 9):
        for nvec in (4, 9):
            C = rng.standard_normal((nvec, ncols)) * 10.0 ** rng.integers(-3, 4, (1, ncols))
            _check(b.krylov_combine(nvec, C), V, C, raw=True, where=f"real C {ncols}")
            Cz = _rand(rng, (nvec, ncols), True)
            _check(b.krylov_combine(nvec, Cz), V, Cz, raw=True, where=f"complex C {ncols}")
    X = b.krylov_combine(5, rng.standard_normal((5, 3)), ldc=9, ldx=n + 2)
    assert np.isnan(X.base[n:]).all() and not np.isnan(X).any()
    ctx.close()


def _phase_basis(rng, n, k, nvec, cplx):
    """columns whose rows 0..k-1 are zero in every column (+0.0 or -0.0), random after"""
    V = _rand(rng, (nvec, n), cplx)
    V[:, :k] = 0.0
    return V


@pytest.mark.parametrize("n, shards", [(1, 1), (2, 2), (1025, 3), (2049, 8), (4097 * 16 + 1, 1), (4097 * 16 + 1, 3),
                                       (4097 * 16 + 1, 8)])
def test_phase_selection(capi, n, shards):
    """the first entry with |z| > 0 in global row order decides the phase: on the last shard, past local entry 4096,
    negative, behind -0.0, subnormal, purely imaginary; an all-zero column stays zero"""
    nvec = 6
    rb_last, re_last = capi.partition(n, shards, shards - 1)
    for cplx in (False, True):
        rng = np.random.default_rng(400 + n + shards + cplx)
        ctx = _ctx(capi, shards)
        b = capi.Basis(ctx, _identity(capi, ctx, n, cplx), n, nvec)
        starts = {rb_last}
        if re_last - rb_last > 5000:
            starts.add(rb_last + 5000)  # past the first 4096-entry chunk of the last shard
        if n > 4200:
            starts.add(4200)
        for k in sorted(starts):
            for kind in ("random", "negative", "negzero", "subnormal", "imaginary", "zero"):
                if kind == "imaginary" and not cplx:
                    continue
                V = _phase_basis(rng, n, k, nvec, cplx)
                S = rng.standard_normal((nvec, 3))
                if kind == "negative":  # x[k] = -sum S^2 < 0 in every column: only column 0 of V is non-zero there
                    V[:, k] = 0.0
                    V[0, k] = -1.5
                    S[0] = np.abs(S[0]) + 0.1
                elif kind == "negzero":
                    V[:, :k] = -0.0
                elif kind == "subnormal":  # x[k] = -5e-324 and x[k+1] > 0: the subnormal decides the sign
                    V[:, k] = 0.0
                    V[0, k] = -5e-324
                    S[0] = 1.0
                    if k + 1 < n:
                        V[:, k + 1] = 0.0
                        V[1, k + 1] = 1.0
                        S[1] = 1.0
                elif kind == "imaginary":
                    V[:, k] = 0.0
                    V[0, k] = 2j
                elif kind == "zero":
                    S[:, 1] = 0.0
                for c in range(nvec):
                    b.upload(capi.VEC_COL(c), V[c])
                X = b.ritz_vectors(nvec, S)
                ref = _check(X, V, S, where=f"{kind} k={k} cplx={cplx}")
                if kind == "zero":
                    assert np.all(X[:, 1] == 0)
                else:
                    for e in range(3):
                        first = rr.first_hit(ref[:, e])
                        assert first >= k, (kind, first, k)
                        if kind != "subnormal":  # (5e-324 / ||x|| may round to zero)
                            assert first == k and np.real(X[k, e]) > 0
                if kind == "subnormal" and k + 1 < n:
                    assert np.all(np.real(X[k + 1]) < 0)  # phase -1 from the subnormal entry
        ctx.close()


@pytest.mark.parametrize("n, shards", [(3, 1), (1025, 3), (4097 * 16 + 1, 8)])
def test_scale_edges(capi, n, shards):
    """squares that underflow (column returned unnormalised, phase applied) and overflow (zeros), as Eigen's normalized()"""
    for cplx in (False, True):
        ctx, b, V, rng = _basis(capi, n, shards, cplx, 500 + n + shards + cplx, cap=6)
        S = rng.standard_normal((6, 5))
        for scale in (1e-200, 1e200):
            Ss = S * scale
            X = b.ritz_vectors(6, Ss)
            ref = _check(X, V, Ss, where=f"scale {scale}")
            if scale > 1:
                assert np.all(X == 0) and np.all(ref == 0)
            else:
                assert np.abs(X).max() < 1e-190
            Sz = Ss * (1 + 1j)
            _check(b.ritz_vectors(6, Sz), V, Sz, where=f"complex scale {scale}")
        ctx.close()


# ---- b. bases the step kernels wrote ----------------------------------------------------------------------------------
def _hermitian_laplacian(n):
    """the 3-D Laplacian with +-0.3i added to its off-diagonal entries (Hermitian)"""
    rp, col, val = cref.laplacian3d(n)
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    z = val.astype(np.complex128) + 0.3j * np.sign(col - rows)
    return rp, col, z


def _lanczos(capi, ctx, A, N, m, cap, cplx, seed):
    b = capi.Basis(ctx, A, N, cap, dtype=np.complex128 if cplx else np.float64)
    rng = np.random.default_rng(seed)
    b.upload(capi.VEC_W, _rand(rng, N, cplx))
    b.lanczos_enqueue(m + 1)
    st, alpha, beta = b.lanczos_state()
    assert (st.nvec, st.nalpha, st.stopped) == (m + 1, m + 1, 0)
    V = np.stack([b.download(capi.VEC_COL(c)) for c in range(m + 1)])
    return b, alpha, beta, V


@pytest.mark.parametrize("shards", [1, 2, 3, 8])
@pytest.mark.parametrize("op", ["row_codes", "plain", "hermitian"])
def test_ritz_vectors_of_fused_lanczos_bases(capi, shards, op, monkeypatch):
    """Lanczos m = 40 on 11^3 (1,331 rows: odd local sizes): all 40 Ritz vectors against combine(V, S) of the downloaded
    columns.  The step kernels wrote these columns, padding rows included; a non-zero padding row shows in the norm."""
    n, m = 11, 40
    N = n ** 3
    if op == "plain":
        monkeypatch.setenv("EIGENEX_NO_ROW_CODES", "1")
    ctx = _ctx(capi, shards)
    if op == "hermitian":
        A = capi.Csr.upload(ctx, N, *_hermitian_laplacian(n))
    else:
        A = capi.Csr.upload(ctx, N, *cref.laplacian3d(n))
        assert A.encoding() == ("plain" if op == "plain" else "row_codes")
    b, alpha, beta, V = _lanczos(capi, ctx, A, N, m, m + 1, op == "hermitian", 600 + shards)
    theta, S = ko.tridiagonal_eigh(alpha[:m], beta[: m - 1])
    _check(b.ritz_vectors(m, S), V, S, where=f"{op} shards={shards}")
    ctx.close()


# ---- c. thick-restart combination ------------------------------------------------------------------------------------
@pytest.mark.parametrize("nkeep", [1, 15, 16, 17, 33, 40])
@pytest.mark.parametrize("shards", [1, 3])
@pytest.mark.parametrize("cplx", [False, True])
def test_restart_combination(capi, nkeep, shards, cplx):
    n, m = 11, 40
    N = n ** 3
    ctx = _ctx(capi, shards)
    A = capi.Csr.upload(ctx, N, *(_hermitian_laplacian(n) if cplx else cref.laplacian3d(n)))
    b, alpha, beta, V = _lanczos(capi, ctx, A, N, m, m + 1 + nkeep, cplx, 700 + nkeep + shards)
    theta, S = ko.tridiagonal_eigh(alpha[:m], beta[: m - 1])
    Sk = np.ascontiguousarray(S[:, :nkeep])
    coupling = beta[m - 1] * S[m - 1, nkeep - 1]
    b.lanczos_restart(Sk, coupling)
    st, alpha2, beta2 = b.lanczos_state()
    assert (st.nvec, st.nalpha, st.nbeta, st.stopped) == (nkeep + 1, nkeep + 1, nkeep, 0)
    W = np.stack([b.download(capi.VEC_COL(c)) for c in range(nkeep + 1)])
    _check(W[:nkeep].T, V[:m], Sk, raw=True, where=f"restart nkeep={nkeep}")
    np.testing.assert_array_equal(W[nkeep].view(np.float64), V[m].view(np.float64))  # bit for bit, nkeep == m included
    assert alpha2[nkeep] == alpha[m] and beta2[nkeep - 1] == coupling
    ctx.close()


# ---- d. BASELINE sizes -----------------------------------------------------------------------------------------------
def _apply(capi, b, x):
    """A x on the device (x uploaded to VEC_W, applied into VEC_V); complex x on a real operator: parts separately"""
    if np.iscomplexobj(x) and not b.is_complex:
        return _apply(capi, b, np.ascontiguousarray(x.real)) + 1j * _apply(capi, b, np.ascontiguousarray(x.imag))
    b.upload(capi.VEC_W, x)
    b.apply(capi.VEC_W, capi.VEC_V)
    return b.download(capi.VEC_V)


def test_c2_laplacian128_ritz_vectors(capi):
    from cmpt_eigenex_amd import solver

    n, m = 128, 50
    N = n ** 3
    ctx = capi.Context()
    A = capi.Csr.laplacian3d(ctx, n)
    b, alpha, beta, V = _lanczos(capi, ctx, A, N, m, m + 1, False, 2)
    theta, S = ko.tridiagonal_eigh(alpha[:m], beta[: m - 1])
    for cols in (np.arange(8), np.arange(m - 8, m)):
        Se = np.ascontiguousarray(S[:, cols])
        X = b.ritz_vectors(m, Se)
        _check(X, V, Se, where="C2")
        for j, e in enumerate(cols):
            r = np.linalg.norm(_apply(capi, b, np.ascontiguousarray(X[:, j])) - theta[e] * X[:, j])
            assert abs(r - beta[m - 1] * abs(S[m - 1, e])) <= 1e-10 * 12.0, (e, r)
    es = solver.LanczosEigenSolver()
    es.setDeviceOperator(A).set(minIterations=m, maxIterations=m, maxEigenvalues=8, initialVector=V[0])
    es.compute()
    Xs = es.results()["eigenvectors"]
    assert Xs.shape == (N, 8)
    for e in range(8):
        assert abs(np.linalg.norm(Xs[:, e]) - 1.0) < 1e-13
        assert Xs[rr.first_hit(Xs[:, e]), e] > 0
    assert np.abs(Xs.T @ Xs - np.eye(8)).max() <= 1e-10
    es.close()
    ctx.close()


def test_c3_random_csr_arnoldi_complex_ritz_vectors(capi):
    from cmpt_eigenex_amd import synthetic

    N, m = 1_000_000, 80
    rowptr, col, val = synthetic.random_csr32(N, 12345)
    ctx = capi.Context()
    A = capi.Csr.upload(ctx, N, rowptr, col, val)
    b = capi.Basis(ctx, A, N, m)
    b.upload(capi.VEC_W, np.random.default_rng(3).standard_normal(N))
    b.arnoldi_enqueue(m)
    st, H = b.arnoldi_state()
    assert (st.nvec, st.stopped) == (m, 0)
    lam, Y = np.linalg.eig(H)
    order = np.argsort(-np.abs(lam))
    pos = [i for i in order if lam[i].imag > 0][:4]
    partner = [int(np.flatnonzero((lam == np.conj(lam[i])) & (np.arange(m) != i))[0]) for i in pos]
    real = [i for i in order if lam[i].imag == 0][:1]
    sel = pos + partner + real  # 9 columns: three passes of 4, the conjugate of each pair in the next pass
    assert len(sel) == 9
    Se = np.asfortranarray(Y[:, sel])
    V = np.stack([b.download(capi.VEC_COL(c)) for c in range(m)])
    X = b.ritz_vectors(m, Se)
    _check(X, V, Se, where="C3")
    for j in range(4):  # the split into V s_re / V s_im, the norm and the phase are symmetric under s_im -> -s_im
        np.testing.assert_array_equal(X[:, 4 + j], np.conj(X[:, j]))
    for j, e in enumerate(sel):
        r = np.linalg.norm(_apply(capi, b, X[:, j]) - lam[e] * X[:, j])
        assert abs(r - st.residue * abs(Y[m - 1, e])) <= 1e-10 * max(1.0, np.abs(lam).max()), (e, r)
    ctx.close()


def test_c4_laplacian512_ritz_vectors(capi):
    t0 = time.perf_counter()
    n, m = 512, 100
    N = n ** 3
    ctx = capi.Context()
    try:
        A = capi.Csr.laplacian3d(ctx, n)
        b = capi.Basis(ctx, A, N, m + 1)
    except capi.EigenexError as e:  # pragma: no cover
        pytest.skip(f"not enough device memory for 512^3: {e}")
    b.upload(capi.VEC_W, np.random.default_rng(20240601).standard_normal(N))
    b.lanczos_enqueue(m + 1)
    st, alpha, beta = b.lanczos_state()
    assert (st.nvec, st.stopped) == (m + 1, 0)
    theta, S = ko.tridiagonal_eigh(alpha[:m], beta[: m - 1])
    cols = [0, m - 1]
    Se = np.ascontiguousarray(S[:, cols])
    X = b.ritz_vectors(m, Se)  # 2 x 1 GB on the host
    for j in range(2):
        assert abs(np.linalg.norm(X[:, j]) - 1.0) < 1e-12
        assert X[rr.first_hit(X[:, j]), j] > 0
    assert abs(X[:, 0] @ X[:, 1]) < 1e-10
    for j, e in enumerate(cols):
        r = np.linalg.norm(_apply(capi, b, np.ascontiguousarray(X[:, j])) - theta[e] * X[:, j])
        assert abs(r - beta[m - 1] * abs(S[m - 1, e])) <= 1e-10 * 12.0, (e, r)
    # a row sample against combine: the norm of V s from the Gram matrix of the basis (dots on the device)
    rows = np.unique(np.concatenate([np.arange(4096), np.arange(N - 4096, N),
                                     np.random.default_rng(4).choice(N, 65536, replace=False)]))
    G = np.stack([b.dots(capi.VEC_COL(c), 0, 1, m) for c in range(m)])
    Vs = np.empty((m, rows.size))
    for c in range(m):
        Vs[c] = b.download(capi.VEC_COL(c))[rows]
    x_ld = rr.combine(Vs, Se)
    Gl, Sl = G.astype(np.longdouble), Se.astype(np.longdouble)
    factors = [1 / np.sqrt(Sl[:, j] @ Gl @ Sl[:, j]) for j in range(2)]
    assert rr.first_hit(x_ld[:, 0]) == 0 and rr.first_hit(x_ld[:, 1]) == 0
    ref = np.stack([(x_ld[:, j] * factors[j] * np.sign(x_ld[0, j])).astype(np.float64) for j in range(2)], axis=1)
    tol = rr.bound(Vs, Se, ref, factors=factors)
    assert np.all(np.abs(X[rows] - ref) <= tol)
    ctx.close()
    print(f"C4 Ritz vector test: {time.perf_counter() - t0:.1f} s")
