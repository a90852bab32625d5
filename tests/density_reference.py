"""numpy restatement of the kernel polynomial method of spectral_density.hpp / eigenex_kpm_moments: the random-sign hash, the
Chebyshev recurrence in float64 (the device's order of operations) and in np.longdouble, the two-moments-per-application
identity, the Jackson factors, density, eigenvalue count and energy window.  Shared by tests/test_density_host.py and
tests/test_gpu_density.py."""
from __future__ import annotations

import numpy as np

from filter_reference import csr_rowsum_matmul  # noqa: F401  (the long double reference of the callers)

_G = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


def _mix(z):
    """the splitmix64 finaliser on uint64 arrays (arithmetic modulo 2^64)"""
    z = np.asarray(z, np.uint64).copy()
    z ^= z >> np.uint64(30)
    z *= _M1
    z ^= z >> np.uint64(27)
    z *= _M2
    z ^= z >> np.uint64(31)
    return z


def random_signs(seed, stream, n, dtype=np.float64):
    """entry `row` = -1 where bit 63 of mix((key ^ row) + G) is set, else +1; key = mix((mix(seed + G) ^ stream) + G)"""
    with np.errstate(over="ignore"):
        seed, stream = np.array([seed], np.uint64), np.array([stream], np.uint64)
        key = _mix((_mix(seed + _G) ^ stream) + _G)
        h = _mix((key ^ np.arange(n, dtype=np.uint64)) + _G)
    return np.where((h >> np.uint64(63)) != 0, -1.0, 1.0).astype(dtype)


def applications(n_moments):
    return n_moments // 2  # ceil((n_moments - 1) / 2)


def _sequential_row_sums(prod, rowptr):
    """sum of every row's products from 0.0 in stored order, one rounded addition at a time (np.add.reduceat adds the first
    product to the sum of the others: another association)"""
    rowptr = np.asarray(rowptr, np.int64)
    length = np.diff(rowptr)
    s = np.zeros(length.size, prod.dtype)
    for j in range(int(length.max()) if length.size else 0):
        here = j < length
        s[here] = s[here] + prod[rowptr[:-1][here] + j]
    return s


def device_matmul(A):
    """x -> A x in float64, one rounded operation at a time in the device's order: every product rounded, then added to the
    row's sum in stored order starting from 0.0.  filter_reference.csr_rowsum_matmul keeps serving the long double reference;
    in float64 its np.add.reduceat associates a row as p0 + (p1 + p2 + ...), which is not the order of the operator kernels
    and moves last bits.  Complex: (re, im) of each product as ar*br - ai*bi and ar*bi + ai*br, every partial product rounded
    (numpy's own complex multiply may contract them), the parts summed separately."""
    rowptr, col = np.asarray(A.indptr, np.int64), A.indices
    if not np.iscomplexobj(A.data):
        val = np.asarray(A.data, np.float64)
        return lambda x: _sequential_row_sums(val * x[col], rowptr)
    vr, vi = A.data.real.copy(), A.data.imag.copy()

    def matmul(x):
        xr, xi = x.real[col], x.imag[col]
        pr = vr * xr - vi * xi
        pi = vr * xi + vi * xr
        return _sequential_row_sums(pr, rowptr) + 1j * _sequential_row_sums(pi, rowptr)

    return matmul


def chebyshev_vectors(matmul, x, center, halfwidth, d):
    """t_0 .. t_d of the recurrence of eigenex_kpm_moments in the precision of x and matmul: a = A t_k - center t_k,
    t_1 = (1/h) a, t_{k+1} = (2/h) a - t_{k-1}, every product rounded before it is added"""
    real = np.float64 if x.dtype in (np.float64, np.complex128) else np.longdouble
    c1, c2 = real(1.0) / real(halfwidth), real(2.0) / real(halfwidth)
    if real is np.float64:  # the factors the device forms on the host, in double
        c1, c2 = np.float64(1.0 / halfwidth), np.float64(2.0 / halfwidth)
    shift = real(-center)
    ts = [x]
    for k in range(d):
        t = ts[-1]
        a = matmul(t)
        if shift != 0:
            a = a + shift * t
        ts.append(c1 * a if k == 0 else c2 * a - ts[-2])
    return ts


def moments_from_vectors(ts, n_moments, dot):
    """mu_0 = <t0,t0>, mu_1 = <t1,t0>, mu_2k = 2 <t_k,t_k> - mu_0, mu_2k+1 = 2 <t_k+1,t_k> - mu_1 with the given real dot"""
    mu = []
    for k in range(n_moments):
        if k == 0:
            mu.append(dot(ts[0], ts[0]))
        elif k == 1:
            mu.append(dot(ts[1], ts[0]))
        elif k % 2 == 0:
            mu.append(2 * dot(ts[k // 2], ts[k // 2]) - mu[0])
        else:
            mu.append(2 * dot(ts[k // 2 + 1], ts[k // 2]) - mu[1])
    return np.array(mu)


def as_doubles(t):
    """a vector as the device sees it: complex entries as interleaved (re, im) doubles"""
    t = np.ascontiguousarray(t)
    return t.view(np.float64) if t.dtype == np.complex128 else (t.view(np.longdouble) if t.dtype == np.clongdouble else t)


def real_dot_longdouble(a, b):
    """Re<a, b> = the plain dot of the interleaved doubles, in long double"""
    return (as_doubles(a).astype(np.longdouble) * as_doubles(b).astype(np.longdouble)).sum()


def abs_dot(a, b):
    return float((np.abs(as_doubles(a)).astype(np.longdouble) * np.abs(as_doubles(b)).astype(np.longdouble)).sum())


# ---- the checks of a device run against the float64 restatement (tests/test_gpu_density.py and the suites that borrow them) -------
EPS = np.finfo(np.float64).eps


def rounded_vector_bound(err64, x):
    """|t_k(device) - t_k(restatement)| where the operator kernel adds a row in another order than the restatement: the bound of
    test_filter_apply_against_long_double, 4 x the restatement's own error against long double (err64) + 4 eps |x|_inf"""
    return 4 * err64 + 4 * EPS * np.abs(x).max()


def moment_bounds(ts, n_moments, vector_bound=None):
    """reference moments (long double dots of the float64 vectors) and the bound of each: a float64 dot of n terms in any order
    errs by at most n eps sum|a_i b_i|, so  |mu_dev - mu_ref| <= 2 (2 n eps sum|t_i||t'_i|) + n eps |mu_0 or mu_1| + eps |mu|,
    and for mu_0, mu_1 themselves n eps sum|a_i b_i| + eps |mu|.  vector_bound(k), where the device's vectors are only close
    to the restatement's (None: they are equal): the dots move by at most dt' sum|t| + dt sum|t'| more."""
    vb = vector_bound or (lambda k: 0.0)
    ref = moments_from_vectors(ts, n_moments, real_dot_longdouble)
    n = as_doubles(ts[0]).size
    one = np.ones(n)
    bounds = []
    for k in range(n_moments):
        a, b = (ts[k // 2], ts[k // 2]) if k % 2 == 0 else (ts[k // 2 + 1], ts[k // 2])
        ka, kb = (k // 2, k // 2) if k % 2 == 0 else (k // 2 + 1, k // 2)
        moved = vb(ka) * abs_dot(one, b) + vb(kb) * abs_dot(one, a)
        if k < 2:
            bnd = n * EPS * abs_dot(a, b) + EPS * abs(float(ref[k])) + moved
        else:
            moved0 = 2 * vb(0) * abs_dot(one, ts[0]) if vector_bound is not None else 0.0
            bnd = 2 * (2 * n * EPS * abs_dot(a, b)) + n * EPS * abs(float(ref[k % 2])) + EPS * abs(float(ref[k])) + 2 * moved + moved0
        bounds.append(bnd)
    return ref.astype(np.float64), np.array(bounds), ref


def check_moments(label, mu, ts, n_moments, vector_bound=None):
    ref64, bounds, ref = moment_bounds(ts, n_moments, vector_bound)
    err = np.abs(mu.astype(np.longdouble) - ref).astype(np.float64)
    worst = int(np.argmax(err / np.maximum(bounds, 1e-300)))
    print(f"{label} n_moments={n_moments}: worst moment {worst}: device error {err[worst]:.3e}, bound {bounds[worst]:.3e} (mu = {ref64[worst]:.6e})")
    assert np.all(err <= bounds)


def check_vector(label, got, t_d, bound=None):
    """the device's Chebyshev vector against the restatement's t_d: bit for bit (bound None), or within the bound"""
    if bound is None:
        np.testing.assert_array_equal(got, t_d)
        return
    e = float(np.abs(got - t_d).max())
    print(f"{label}: device error {e:.3e}, bound {bound:.3e}")
    assert e <= bound


def exact_moments(lam, center, halfwidth, M):
    """mu_k = mean_i cos(k arccos x_i) of the scaled eigenvalues: tr T_k / N"""
    th = np.arccos(np.clip((np.asarray(lam, np.longdouble) - center) / halfwidth, -1, 1))
    return np.array([np.cos(k * th).mean() for k in range(M)]).astype(np.float64)


def jackson(M):
    k = np.arange(M, dtype=np.float64)
    q = np.pi / (M + 1)
    return ((M - k + 1) * np.cos(q * k) + np.sin(q * k) / np.tan(q)) / (M + 1)


def density_terms(mu, center, halfwidth, E):
    """the M terms of the damped series at E and the common factor: density = factor * sum(terms)"""
    mu = np.asarray(mu, np.float64)
    M = mu.size
    x = (E - center) / halfwidth
    th = np.arccos(x)
    k = np.arange(M)
    terms = np.where(k == 0, 1.0, 2.0) * jackson(M) * mu * np.cos(k * th)
    return terms, 1.0 / (np.pi * np.sqrt(1.0 - x * x) * halfwidth)


def density(mu, center, halfwidth, E):
    x = (E - center) / halfwidth
    if not (-1.0 < x < 1.0):
        return 0.0
    terms, f = density_terms(mu, center, halfwidth, E)
    return float(terms.sum() * f)


def count_terms(mu, center, halfwidth, a, b):
    """the M terms of the fraction of states in [a, b]"""
    mu = np.asarray(mu, np.float64)
    M = mu.size
    tha = np.arccos(np.clip((a - center) / halfwidth, -1, 1))
    thb = np.arccos(np.clip((b - center) / halfwidth, -1, 1))
    k = np.arange(1, M)
    g = jackson(M)
    first = g[0] * mu[0] * (tha - thb) / np.pi
    rest = 2.0 * g[1:] * mu[1:] * (np.sin(k * tha) - np.sin(k * thb)) / (k * np.pi)
    return np.concatenate([[first], rest])


def count(mu, center, halfwidth, a, b, N):
    if not b > a:
        return 0.0
    return float(N * count_terms(mu, center, halfwidth, a, b).sum())


def window(mu, center, halfwidth, tau, want, N):
    """the half-width delta with count(tau - delta, tau + delta) = want: bisection down to neighbouring doubles"""
    lo, hi = 0.0, max(tau - (center - halfwidth), (center + halfwidth) - tau)
    if not hi > 0 or not want > 0:
        return 0.0
    if count(mu, center, halfwidth, tau - hi, tau + hi, N) <= want:
        return hi
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if not lo < mid < hi:
            break
        if count(mu, center, halfwidth, tau - mid, tau + mid, N) < want:
            lo = mid
        else:
            hi = mid
    return hi


def widened(lo, hi):
    """(center, halfwidth) of SpectralDensitySolver for setSpectralRange(lo, hi)"""
    return 0.5 * (lo + hi), 0.5 * (hi - lo) * 1.01


QUANTILE_WINDOWS = ((0.10, 0.40), (0.45, 0.55), (0.0, 0.50), (0.70, 1.0))


def quantile_window(lam, qa, qb, lo, hi):
    """[a, b] whose ends sit half-way between neighbouring eigenvalues at the quantiles qa, qb of the sorted spectrum (the ends of
    the spectral range at 0 and 1), and the number of eigenvalues inside"""
    lam = np.sort(np.asarray(lam))
    n = lam.size
    ia, ib = int(round(qa * n)), int(round(qb * n))
    a = lo if ia <= 0 else 0.5 * (lam[ia - 1] + lam[ia])
    b = hi if ib >= n else 0.5 * (lam[ib - 1] + lam[ib])
    return float(a), float(b), int(((lam > a) & (lam < b)).sum())
