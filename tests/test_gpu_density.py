"""Chebyshev moments on the device (eigenex_kpm_moments, eigenex_kpm_trace_moments, eigenex_vec_random_signs) and
SpectralDensitySolver against the numpy restatement tests/density_reference.py.  Inputs: those of tests/test_gpu_filter.py
and a 5-row matrix."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import density_reference as dr  # noqa: E402
import filter_reference as fr  # noqa: E402
import test_gpu_filter as tf  # noqa: E402  (its inputs and how they go to the device)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
N_MOMENTS = (1, 2, 3, 4, 5, 64, 65)
NAMES = ["chain257", "chain1000", "laplacian12", "chain257_blocked", "blocks", "ztridiagonal", "five"]
ROUNDED = ("blocks",)  # operator kernels whose row sums are not the restatement's, rounding for rounding


@pytest.fixture(scope="module")
def capi():
    from cmpt_eigenex_amd import capi as c

    assert c.device_count() >= 1
    return c


def _input(name):
    if name == "five":
        import scipy.sparse as sp

        A = sp.diags([[0.4, -0.2, 0.1, 0.7, -0.5], [-1.0, 0.5, -0.25, 2.0], [-1.0, 0.5, -0.25, 2.0]], [0, 1, -1]).tocsr()
        A.sort_indices()
        return A
    return tf._input(name)


def _upload(capi, ctx, name):
    if name == "five":
        A = _input(name)
        return capi.Csr.upload(ctx, 5, A.indptr, A.indices, A.data)
    return tf._upload(capi, ctx, name)


_REFS = {}


def _reference(name):
    """x, (center, halfwidth), the float64 restatement's t_0 .. t_32, its own error against long double per degree -- once"""
    if name not in _REFS:
        A = _input(name)
        n = A.shape[0]
        cplx = np.iscomplexobj(A.data)
        rng = np.random.RandomState(17)
        x = rng.standard_normal(n) + (1j * rng.standard_normal(n) if cplx else 0.0)
        c, h = dr.widened(*fr.gershgorin(A))
        d = dr.applications(max(N_MOMENTS))
        ts = dr.chebyshev_vectors(dr.device_matmul(A), x, c, h, d)
        ld = np.clongdouble if cplx else np.longdouble
        tl = dr.chebyshev_vectors(fr.csr_rowsum_matmul(A.indptr, A.indices, A.data, ld), x.astype(ld), c, h, d)
        err64 = [float(np.abs(a.astype(ld) - b).max()) for a, b in zip(ts, tl)]
        _REFS[name] = (x, c, h, ts, err64)
    return _REFS[name]


def _vector_bound(name, k):
    """|t_k(device) - t_k(restatement)|: 0 where the two round alike, else the bound of test_filter_apply_against_long_double
    (4 x the restatement's own error against long double + 4 eps |x|_inf; the factor 4: another row-sum order)"""
    if name not in ROUNDED:
        return 0.0
    x, _, _, _, err64 = _reference(name)
    return dr.rounded_vector_bound(err64[k], x)


def _rounded(name):
    """what density_reference's checks take: None where the device rounds like the restatement, else the bound of vector k"""
    return (lambda k: _vector_bound(name, k)) if name in ROUNDED else None


def _moment_bounds(name, ts, n_moments):
    return dr.moment_bounds(ts, n_moments, _rounded(name))


def _check_moments(label, mu, name, ts, n_moments):
    dr.check_moments(label, mu, ts, n_moments, _rounded(name))


def _check_vector(label, name, got, ts, d):
    dr.check_vector(label, got, ts[d], _vector_bound(name, d) if name in ROUNDED else None)


@pytest.mark.parametrize("shards", [1, 2, 3])
@pytest.mark.parametrize("name", NAMES)
def test_moments_and_last_vector_against_the_restatement(capi, name, shards):
    """EIGENEX_VEC_V = t_d of the float64 restatement bit for bit, every moment within the dot-product bound; between shards one
    neighbour exchange per application and one all-reduce per run; the input is left alone"""
    ctx = capi.Context(loopback_shards=shards) if shards > 1 else capi.Context()
    A = _upload(capi, ctx, name)
    x, c, h, ts, _ = _reference(name)
    b = capi.Basis(ctx, A, x.size, 3)
    b.upload(capi.VEC_COL(0), x)
    for nm in N_MOMENTS:
        d = dr.applications(nm)
        ctx.trace(True)
        mu = b.kpm_moments(capi.VEC_COL(0), nm, c, h)
        ops = ctx.trace_get()
        ctx.trace(False)
        label = f"{name} shards={shards}"
        _check_vector(label, name, b.download(capi.VEC_V), ts, d)
        _check_moments(label, mu, name, ts, nm)
        halos = sum(1 for op, _ in ops if op == capi.COLL_HALO)
        reduces = [cnt for op, cnt in ops if op == capi.COLL_ALLREDUCE]
        assert halos == (d if shards > 1 else 0)
        assert reduces == ([2 * (d + 1)] if shards > 1 else [])
    np.testing.assert_array_equal(b.download(capi.VEC_COL(0)), x)
    b.close()
    A.close()
    ctx.close()


def _counted_moments(capi, ctx, b, nm, c, h):
    ctx.profile_enable(True)
    ctx.profile_reset()
    mu = b.kpm_moments(capi.VEC_COL(0), nm, c, h)
    launches, _, nbytes = ctx.profile_get(capi.K_SPMV)
    ctx.profile_enable(False)
    return mu, b.download(capi.VEC_V), launches, nbytes


@pytest.mark.parametrize("name", ["chain1000", "chain257", "laplacian12"])
def test_fused_and_streaming_forms(capi, name, monkeypatch):
    """the same bits in t_d, moments of both within the bound (their partial sums are grouped differently), either form the same
    bits when repeated; the fused form is one launch per application, the streaming form two"""
    nm = 65
    d = dr.applications(nm)
    ctx = capi.Context()
    A = _upload(capi, ctx, name)
    assert A.encoding() == ("row_codes" if name == "laplacian12" else "plain")
    x, c, h, ts, _ = _reference(name)
    b = capi.Basis(ctx, A, x.size, 3)
    b.upload(capi.VEC_COL(0), x)
    out = {}
    for form in ("fused", "streaming"):
        if form == "streaming":
            monkeypatch.setenv("EIGENEX_NO_FUSED_FILTER", "1")
        else:
            monkeypatch.delenv("EIGENEX_NO_FUSED_FILTER", raising=False)
        mu, td, launches, nbytes = _counted_moments(capi, ctx, b, nm, c, h)
        mu2, td2, _, _ = _counted_moments(capi, ctx, b, nm, c, h)
        assert launches == (d if form == "fused" else 2 * d)
        np.testing.assert_array_equal(mu, mu2)
        np.testing.assert_array_equal(td, td2)
        _check_moments(f"{name} {form}", mu, name, ts, nm)
        out[form] = (mu, td, nbytes)
    np.testing.assert_array_equal(out["fused"][1], out["streaming"][1])
    np.testing.assert_array_equal(out["fused"][1], ts[d])
    # booked traffic: per application the operator + 24 N bytes fused (16 N in the first), + 16 N and 32 N (24 N) streaming
    n = x.size
    assert out["streaming"][2] - out["fused"][2] == pytest.approx(24.0 * n * d)
    b.tune(flags=2)  # non-temporal val/col streams: another instantiation of the fused kernels, the same bits
    monkeypatch.delenv("EIGENEX_NO_FUSED_FILTER", raising=False)
    mu_nt, td_nt, launches, _ = _counted_moments(capi, ctx, b, nm, c, h)
    assert launches == d
    np.testing.assert_array_equal(td_nt, out["fused"][1])
    np.testing.assert_array_equal(mu_nt, out["fused"][0])
    b.close()
    A.close()
    ctx.close()


@pytest.mark.parametrize("shards", [1, 2, 3])
@pytest.mark.parametrize("name", ["chain1000", "ztridiagonal", "five"])
def test_random_signs_equal_the_numpy_hash(capi, name, shards):
    """entry for entry, so the same vector under every sharding; imaginary parts 0"""
    ctx = capi.Context(loopback_shards=shards) if shards > 1 else capi.Context()
    A = _upload(capi, ctx, name)
    n = _input(name).shape[0]
    b = capi.Basis(ctx, A, n, 3)
    for seed, stream, ref in ((0, 0, capi.VEC_COL(1)), (2006, 5, capi.VEC_W), (2 ** 64 - 1, 2 ** 63 + 11, capi.VEC_V)):
        b.random_signs(ref, seed, stream)
        np.testing.assert_array_equal(b.download(ref), dr.random_signs(seed, stream, n, b.dtype))
    with pytest.raises(capi.EigenexError):
        b.random_signs(capi.VEC_COL(7), 1, 1)
    b.close()
    A.close()
    ctx.close()


@pytest.mark.parametrize("shards", [1, 2])
@pytest.mark.parametrize("name", ["chain257", "laplacian12", "ztridiagonal"])
def test_trace_moments_equal_a_loop_of_single_runs(capi, name, shards):
    ctx = capi.Context(loopback_shards=shards) if shards > 1 else capi.Context()
    A = _upload(capi, ctx, name)
    _, c, h, _, _ = _reference(name)
    n = _input(name).shape[0]
    b = capi.Basis(ctx, A, n, 3)
    for nm in (1, 2, 5, 64):
        ctx.trace(True)
        each = b.kpm_trace_moments(nm, 3, 41, 7, c, h)
        ops = ctx.trace_get()
        ctx.trace(False)
        assert sum(1 for op, _ in ops if op == capi.COLL_ALLREDUCE) == (1 if shards > 1 else 0)
        assert sum(1 for op, _ in ops if op == capi.COLL_HALO) == (3 * dr.applications(nm) if shards > 1 else 0)
        last = b.download(capi.VEC_V)
        for i in range(3):
            b.random_signs(capi.VEC_COL(0), 41, 7 + i)
            mu = b.kpm_moments(capi.VEC_COL(0), nm, c, h)
            np.testing.assert_array_equal(each[i], mu / n)
        np.testing.assert_array_equal(last, b.download(capi.VEC_V))  # t_d of the last vector
        np.testing.assert_array_equal(each[:, 0], 1.0)
    b.close()
    A.close()
    ctx.close()


def test_filter_stays_in_force_and_errors_leave_the_state_usable(capi):
    name = "chain257"
    Asp = _input(name)
    n = Asp.shape[0]
    ctx = capi.Context()
    x, c, h, ts, _ = _reference(name)
    fx, fmu, fc, fh, _, _ = tf._reference(name, 40)
    hb = capi.Basis(ctx, None, n, 4)
    hb.set_host_operator(lambda v: Asp @ v)
    hb.upload(capi.VEC_COL(0), x)
    with pytest.raises(capi.EigenexError):
        hb.kpm_moments(capi.VEC_COL(0), 5, c, h)  # the moments need a device operator
    with pytest.raises(capi.EigenexError):
        hb.kpm_trace_moments(5, 2, 1, 0, c, h)
    assert tf._run_steps(capi, hb, x, 3)[0].nvec == 3  # the state still steps
    hb.close()
    A = _upload(capi, ctx, name)
    b = capi.Basis(ctx, A, n, 8)
    b.set_filter(fmu, fc, fh)
    b.upload(capi.VEC_COL(0), fx)
    b.filter_apply(capi.VEC_COL(0), capi.VEC_COL(1))
    before = b.download(capi.VEC_COL(1))
    b.upload(capi.VEC_COL(2), x)
    mu = b.kpm_moments(capi.VEC_COL(2), 65, c, h)
    for bad in (dict(n_moments=0, center=c, halfwidth=h), dict(n_moments=-3, center=c, halfwidth=h), dict(n_moments=5, center=c, halfwidth=0.0),
                dict(n_moments=5, center=c, halfwidth=-1.0)):
        with pytest.raises(capi.EigenexError):
            b.kpm_moments(capi.VEC_COL(2), **bad)
    with pytest.raises(capi.EigenexError):
        b.kpm_trace_moments(5, 0, 1, 0, c, h)
    with pytest.raises(capi.EigenexError):
        b.kpm_moments(capi.VEC_COL(99), 5, c, h)
    assert capi.lib().eigenex_kpm_moments(b.h, capi.VEC_COL(2), 5, c, h, None) != 0  # mu == NULL
    np.testing.assert_array_equal(b.kpm_moments(capi.VEC_COL(2), 65, c, h), mu)
    b.filter_apply(capi.VEC_COL(0), capi.VEC_COL(1))
    np.testing.assert_array_equal(b.download(capi.VEC_COL(1)), before)  # the filter is still the one that was set
    filtered = tf._run_steps(capi, b, fx, 6)
    b.set_filter(None)
    plain = tf._run_steps(capi, b, fx, 6)
    assert filtered[0].nvec == 6 and abs(filtered[1][0] - plain[1][0]) > 1e-3
    c2 = capi.Basis(ctx, A, n, 8)  # a state that never had a filter: the moments bring their own work vectors, then a filter finds them
    c2.upload(capi.VEC_COL(2), x)
    np.testing.assert_array_equal(c2.kpm_moments(capi.VEC_COL(2), 65, c, h), mu)
    c2.set_filter(fmu, fc, fh)
    c2.upload(capi.VEC_COL(0), fx)
    c2.filter_apply(capi.VEC_COL(0), capi.VEC_COL(1))
    np.testing.assert_array_equal(c2.download(capi.VEC_COL(1)), before)
    c2.close()
    b.close()
    A.close()
    ctx.close()


def test_solver_counts_against_the_restatement(capi):
    """SpectralDensitySolver on the 1000-site chain, M = 257, R = 8, seed 2006: the count on the four quantile windows equals the
    restatement's count from the same +-1 vectors.  No statistics: the vectors are identical, so the bound is the moments' bound
    (test above) carried through the linear form, |w_k| bound_k summed, plus the rounding of the M-term sum and of the mean."""
    from cmpt_eigenex_amd import solver

    M, R, seed, name = 257, 8, 2006, "chain1000"
    Asp = _input(name)
    n = Asp.shape[0]
    lam = np.linalg.eigvalsh(Asp.toarray())
    lo, hi = fr.gershgorin(Asp)
    c, h = dr.widened(lo, hi)
    matmul = dr.device_matmul(Asp)
    refs, bnds = [], []
    for i in range(R):
        ts = dr.chebyshev_vectors(matmul, dr.random_signs(seed, i, n), c, h, dr.applications(M))
        _, bounds, ref = _moment_bounds(name, ts, M)
        refs.append((ref / n).astype(np.float64))
        bnds.append(bounds / n + EPS * np.abs(refs[-1]))
    mu_ref = np.mean(refs, axis=0)
    mu_bound = np.mean(bnds, axis=0) + R * EPS * np.abs(refs).mean(axis=0)
    ctx = capi.Context()
    A = _upload(capi, ctx, name)
    sd = solver.SpectralDensitySolver(np.float64)
    sd.setDeviceOperator(A)
    sd.set(spectralRange=(lo, hi), moments=M, randomVectors=R, seed=seed)
    sd.compute()
    r = sd.results()
    assert r["info_name"] == "Success" and r["nmoments"] == M and r["nvectors"] == R and r["operatorApplications"] == R * (M // 2)
    assert (r["center"], r["halfwidth"]) == (c, h)
    assert np.all(np.abs(r["moments"] - mu_ref) <= mu_bound) and r["moments"][0] == 1.0
    se = np.std(r["momentsOfEachVector"], axis=0, ddof=1) / np.sqrt(R)
    np.testing.assert_allclose(r["momentsStandardError"], se, rtol=1e-12, atol=1e-18)
    g = dr.jackson(M)
    for qa, qb in dr.QUANTILE_WINDOWS:
        a, b_, true = dr.quantile_window(lam, qa, qb, lo, hi)
        terms = dr.count_terms(mu_ref, c, h, a, b_)
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.where(mu_ref != 0, terms / mu_ref, 0.0)
        w[mu_ref == 0] = 2.0 * g[mu_ref == 0]  # |coefficient| <= 2 g_k / (k pi) <= 2 g_k
        bound = n * (np.abs(w) * mu_bound).sum() + 2 * M * EPS * n * np.abs(terms).sum()
        got, ref = sd.eigenvalueCount(a, b_), dr.count(mu_ref, c, h, a, b_, n)
        err = sd.eigenvalueCountStandardError(a, b_)
        print(f"[{qa}, {qb}]: {true} eigenvalues; device {got:.6f} +- {err:.3f}, restatement {ref:.6f}: difference {abs(got - ref):.3e}, bound {bound:.3e}")
        assert abs(got - ref) <= bound
        each = np.array([dr.count(m, c, h, a, b_, n) for m in r["momentsOfEachVector"]])
        assert err == pytest.approx(each.std(ddof=1) / np.sqrt(R), rel=1e-9)
    d = sd.energyWindow(c, 10.0)
    assert abs(sd.eigenvalueCount(c - d, c + d) - 10.0) < 1e-9
    np.testing.assert_allclose(sd.density([0.3, -1.0]), [dr.density(r["moments"], c, h, 0.3), dr.density(r["moments"], c, h, -1.0)], rtol=1e-12)
    sd.continueToCompute()
    r2 = sd.results()
    assert r2["nvectors"] == 2 * R
    np.testing.assert_array_equal(r2["momentsOfEachVector"][:R], r["momentsOfEachVector"])
    assert np.abs(r2["momentsOfEachVector"][R:] - r["momentsOfEachVector"]).max() > 1e-3  # new streams
    # the local density of a given vector: one run, no error bars
    v = np.random.RandomState(3).standard_normal(n)
    sd.set(initialVector=v)
    sd.compute()
    r3 = sd.results()
    ts = dr.chebyshev_vectors(matmul, v, c, h, dr.applications(M))
    _, bounds, ref = _moment_bounds(name, ts, M)
    assert r3["nvectors"] == 1 and np.all(r3["momentsStandardError"] == 0) and sd.eigenvalueCountStandardError(-1.0, 1.0) == 0.0
    assert np.all(np.abs(r3["moments"] - (ref / ref[0]).astype(np.float64)) <= (bounds + np.abs(ref).astype(np.float64) * bounds[0] / float(ref[0])) / float(ref[0]) + 2 * EPS * np.abs(r3["moments"]))
    sd.close()
    A.close()
    ctx.close()


def test_cpp_program_window_feeds_the_filtered_solver(tmp_path):
    """tests/cpp/spectral_density_amd.cpp: energyWindow at the centre of the Anderson chain for count = 10, then
    FilteredLanczosEigenSolver for 10 eigenvalues: all inside twice that half-width.  The factor 2 checked with the restatements
    on the CPU first: for seeds 1, 2, 3, 2006 (M = 257, R = 8) the 10th-nearest eigenvalue lies at 0.93, 0.94, 1.02, 0.85 of the
    half-width, so 2 has room."""
    exe = str(tmp_path / "spectral_density_amd")
    lib = os.path.join(ROOT, "cmpt-eigenex_amd", "lib")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cmpt-eigenex_amd", "include"),
                           os.path.join(ROOT, "tests", "cpp", "spectral_density_amd.cpp"), "-o", exe, "-L", lib, "-leigenex_hip", "-Wl,-rpath," + lib])
    Asp = _input("chain1000")
    diag = tmp_path / "diag.txt"
    np.savetxt(diag, Asp.diagonal(), fmt="%.17g")
    out = json.loads(subprocess.check_output([exe, str(diag), "257", "8", "2006", "10", "200", "100"], timeout=120).decode())
    lam = np.array(out["eigenvalues"])
    want = fr.nearest(Asp, out["tau"], 10)
    print("C++ program: half-width %.6f, farthest eigenvalue at %.6f (%.2f of it), eigenvalue error %.3e" %
          (out["delta"], np.abs(lam - out["tau"]).max(), np.abs(lam - out["tau"]).max() / out["delta"], np.abs(np.sort(lam) - np.sort(want)).max()))
    assert out["info"] == 0 and out["invalid_without_range"] == 3 and out["solver_info"] == 0
    assert out["mu0"] == 1.0 and out["vectors_after_continue"] == 16 and out["applications"] == 16 * 128
    assert abs(out["count_in_window"] - 10.0) < 1e-9 and out["count_error"] > 0
    assert lam.size == 10 and np.all(np.abs(lam - out["tau"]) <= 2.0 * out["delta"])
    np.testing.assert_allclose(np.sort(lam), np.sort(want), rtol=0, atol=1e-9)
