"""Extended-precision reference for Ritz vectors and Krylov combinations (lanczos.hpp:798-816, arnoldi.hpp:841-865).

combine(V, S) forms X = sum_m S[m, e] V[m] in long double, one column at a time, m ascending.  finish(x) applies the
reference's phase fix and Eigen's normalized() in that precision and rounds to float64 at the end.  bound(V, S, x) is
the per-entry tolerance a correct fp64 kernel meets.  V is given as basis columns: V[m] is column m (an array of rows).
"""
import numpy as np

U = 2.0 ** -53  # unit roundoff of float64

assert np.finfo(np.longdouble).nmant >= 63, "the Ritz reference needs an 80-bit (or wider) long double"


def _ld(cplx):
    return np.clongdouble if cplx else np.longdouble


def combine(V_cols, S):
    """X[:, e] = sum_m S[m, e] * V[m] in long double (complex long double if V or S is complex); shape (rows, nev).
    V_cols may hold more columns than S has rows (the rows count is taken from V_cols[0])."""
    S = np.asarray(S)
    if S.ndim == 1:
        S = S[:, None]
    nvec, nev = S.shape
    nrows = len(V_cols[0]) if len(V_cols) else 0
    if np.iscomplexobj(S) and len(V_cols) and not np.iscomplexobj(V_cols[0]):  # real basis: the two parts apart
        return combine(V_cols, S.real) + 1j * combine(V_cols, S.imag)
    cplx = np.iscomplexobj(S) or (len(V_cols) > 0 and np.iscomplexobj(V_cols[0]))
    T = _ld(cplx)
    acc = [np.zeros(nrows, T) for _ in range(nev)]
    Sl = S.astype(T)
    for m in range(nvec):
        vm = np.asarray(V_cols[m]).astype(T)
        for e in range(nev):
            acc[e] += Sl[m, e] * vm
    return np.stack(acc, axis=1) if nev else np.zeros((nrows, 0), T)


def _first_nonzero(x):
    nz = np.flatnonzero(np.abs(x) > 0)
    return int(nz[0]) if nz.size else -1


def norm_factor(x):
    """The factor normalized() multiplies column x by, with fp64's semantics: a squared norm that is 0 in float64
    leaves the column alone (factor 1), one that overflows divides it by inf (factor 0)."""
    x64 = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    with np.errstate(over="ignore"):
        sq64 = np.sum(np.abs(x64) ** 2)
    if sq64 == 0:
        return np.longdouble(1)
    if np.isinf(sq64):
        return np.longdouble(0)
    return np.longdouble(1) / np.sqrt(np.sum(np.abs(x) ** 2))


def finish(x):
    """(1 / phase) * normalized(x) for one column (or each column of a 2-D array), in long double, rounded to
    float64 / complex128.  phase = value / |value| of the first entry with |value| > 0."""
    x = np.asarray(x)
    if x.ndim == 2:
        cols = [finish(x[:, e]) for e in range(x.shape[1])]
        dt = np.complex128 if np.iscomplexobj(x) else np.float64
        return np.stack(cols, axis=1) if cols else np.zeros(x.shape, dt)
    cplx = np.iscomplexobj(x)
    x = x.astype(_ld(cplx))
    i = _first_nonzero(x)
    phase = x[i] / np.abs(x[i]) if i >= 0 else _ld(cplx)(1)
    y = np.conj(phase) * (x * norm_factor(x)) if cplx else (x * norm_factor(x)) / phase
    return y.astype(np.complex128 if cplx else np.float64)


def bound(V_cols, S, x_ref, raw=False, factors=None):
    """Per-entry tolerance, shape of x_ref: (nvec + 8) u (sum_m |S_me| |V_mr|) / ||x_e|| + 8 u |x_ref_r|.
    raw: for eigenex_krylov_combine's unnormalised output (no division by the norm).  factors: norm_factor() of each
    whole column, when V_cols holds only a sample of the rows."""
    S = np.asarray(S)
    if S.ndim == 1:
        S = S[:, None]
    nvec, nev = S.shape
    x_ref = np.asarray(x_ref).reshape(-1, nev)
    mag = np.zeros(x_ref.shape, np.float64)
    aS = np.abs(S)
    for m in range(nvec):
        av = np.abs(np.asarray(V_cols[m]))
        for e in range(nev):
            mag[:, e] += aS[m, e] * av
    if not raw:
        if factors is None:
            x = combine(V_cols, S)
            factors = [norm_factor(x[:, e]) for e in range(nev)]
        for e in range(nev):
            mag[:, e] *= float(factors[e])
    return (nvec + 8) * U * mag + 8 * U * np.abs(x_ref)


def first_hit(x):
    """Index of the first entry with |x| > 0 (-1 if none)."""
    return _first_nonzero(np.asarray(x))
