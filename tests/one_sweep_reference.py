"""numpy restatements (fp64) of the two re-orthogonalisation schemes of a Lanczos step, written the same way so that they
can be held against each other, and of the small terms of the one-sweep scheme (csrc/lag_terms.hpp).

batched(): the two-sweep scheme.  Step k forms w0 = (v - alpha_k u_k) - beta_{k-1} u_{k-1}, sweeps the basis once for
h = V^T w0 and a second time for w = w0 - V h.

one_sweep(): one sweep per step, corrected for lag.  The sweep of step k takes the dots d = V^T w0 of the RAW w0, and in the
same pass applies the coefficients of the PREVIOUS step to the column the operator has already used (u_k = u~_k - V c), and the
part of the error that is known beforehand to w (w = w0 - V f).  With T the tridiagonal matrix so far and a' = u~_k . A u~_k:

    f[0..k)  = (T[(k+1) x k] c - a' c),   da = 2 c[k-1] beta[k-1],   f[k] = (T c)[k] - da,   alpha_k = a' - da
    h = d - f,   beta_k = |w|,   c_next = h / beta_k

A plain one-step lag (f = 0, da = 0) is unstable: c_{k+1} ~ (T - alpha I) c_k / beta grows geometrically.  The guard: when
max |c_next| > 2^-27 the dropped c^2 terms matter (close to a breakdown, where beta is tiny); the pending vector is then
re-orthogonalised with the two-sweep pass before the operator uses it, and c_next = 0.

Every sum over basis columns runs in ascending column order, as the kernel's does."""
import numpy as np

GUARD = 2.0 ** -27


def laplacian3d(n):
    """7-point Laplacian on an n^3 grid, Dirichlet boundary, as a matrix-free product (6 on the diagonal, -1 to the neighbours)."""

    def apply(x):
        g = x.reshape(n, n, n)
        y = 6.0 * g
        y[1:, :, :] -= g[:-1, :, :]
        y[:-1, :, :] -= g[1:, :, :]
        y[:, 1:, :] -= g[:, :-1, :]
        y[:, :-1, :] -= g[:, 1:, :]
        y[:, :, 1:] -= g[:, :, :-1]
        y[:, :, :-1] -= g[:, :, 1:]
        return y.reshape(-1)

    return apply


def diagonal(d):
    d = np.asarray(d, dtype=np.float64)
    return lambda x: d * x


def tridiagonal_csr(n, diag=2.0, off=-1.0):
    """(diag + 0.01 (i mod 7)) on the diagonal, off beside it, as CSR (rowptr, col, val): the operator of the tile-edge cases"""
    i = np.arange(n)
    rows = np.concatenate([i[1:], i, i[:-1]])
    cols = np.concatenate([i[:-1], i, i[1:]])
    vals = np.concatenate([np.full(n - 1, off), diag + 0.01 * (i % 7), np.full(n - 1, off)])
    order = np.lexsort((cols, rows))
    rowptr = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(rows, minlength=n), out=rowptr[1:])
    return rowptr, cols[order].astype(np.int32), vals[order]


def csr_apply(rowptr, col, val):
    row = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
    return lambda x: np.bincount(row, weights=val * x[col], minlength=rowptr.size - 1)


def lag_terms(k, alpha, beta, c, a_raw):
    """f (length k+1) and da of step k from the series so far (alpha[0..k), beta[0..k)), the pending coefficients c (length k)
    and the raw a'.  The order of the additions is the one csrc/lag_terms.hpp uses per entry."""
    f = np.zeros(k + 1)
    da = 0.0
    if k == 0:
        return f, da
    for i in range(k + 1):  # T[(k+1) x k] c: column j of T reaches entry i = j+1, j, j-1; per entry in the order j = i-1, i, i+1
        s = 0.0
        if 1 <= i and i - 1 < k:
            s += beta[i - 1] * c[i - 1]
        if i < k:
            s += alpha[i] * c[i]
        if i + 1 < k:
            s += beta[i] * c[i + 1]
        if i < k:
            s -= a_raw * c[i]
        f[i] = s
    da = 2.0 * c[k - 1] * beta[k - 1]
    f[k] -= da
    return f, da


def batched(apply, x, m, shift=0.0, threshold=1e-12):
    """m steps of the two-sweep scheme.  Returns alpha (m+1, or fewer after a breakdown), beta, V (columns as rows)."""
    nrm = np.sqrt(x @ x)
    V = [x * (1.0 / nrm)]
    v = apply(V[0]) + shift * V[0]
    alpha, beta = [V[0] @ v], []
    for k in range(m):
        w0 = v - alpha[k] * V[k]
        if k > 0:
            w0 = w0 - beta[k - 1] * V[k - 1]
        h = [V[j] @ w0 for j in range(k + 1)]
        w = w0.copy()
        for j in range(k + 1):
            w -= h[j] * V[j]
        nrm = np.sqrt(w @ w)
        beta.append(nrm)
        if nrm <= threshold:
            break
        V.append(w * (1.0 / nrm))
        v = apply(V[-1]) + shift * V[-1]
        alpha.append(V[-1] @ v)
    return np.array(alpha), np.array(beta), np.array(V)


def one_sweep(apply, x, m, shift=0.0, threshold=1e-12, guard=GUARD, use_f=True, use_da=True, trace=None):
    """m steps of the one-sweep scheme, closed at the end (every column corrected, alpha corrected).
    Returns alpha, beta, V (columns as rows), the number of repairs, max |c| seen."""
    W = x.astype(np.float64).copy()
    scale = 1.0 / np.sqrt(W @ W)
    U = []
    ut = W * scale
    v = apply(ut) + shift * ut
    a_raw = ut @ v
    alpha, beta = [], []
    c = np.zeros(0)
    repairs, cmax = 0, 0.0
    stopped = False
    for k in range(m):
        ut = W * scale
        w0 = v - a_raw * ut
        if k > 0:
            w0 = w0 - beta[k - 1] * U[k - 1]
        f, da = lag_terms(k, alpha, beta, c, a_raw)
        if not use_f:
            f[:k] = 0.0
            f[k] = -da if k > 0 else 0.0
        if not use_da:
            if k > 0:
                f[k] += da
            da = 0.0
        alpha.append(a_raw - da)
        u, w, d = ut.copy(), w0.copy(), np.zeros(k + 1)
        for j in range(k):
            d[j] = U[j] @ w0
            u -= c[j] * U[j]
            w -= f[j] * U[j]
        d[k] = u @ w0
        w -= f[k] * u
        U.append(u)
        W = w
        nrm = np.sqrt(W @ W)
        h = d - f
        c = h / nrm if nrm > threshold else np.zeros(k + 1)
        if trace is not None:
            trace.append(dict(k=k, f=f.copy(), da=da, d=d.copy(), h=h.copy(), c=c.copy(), a_raw=a_raw))
        if c.size:
            cmax = max(cmax, float(np.abs(c).max()))
        if guard is not None and c.size and np.abs(c).max() > guard:
            repairs += 1
            hh = [U[j] @ W for j in range(k + 1)]
            for j in range(k + 1):
                W = W - hh[j] * U[j]
            nrm = np.sqrt(W @ W)
            c = np.zeros(k + 1)
        beta.append(nrm)
        if nrm <= threshold:
            stopped = True
            break
        scale = 1.0 / nrm
        ut = W * scale
        v = apply(ut) + shift * ut
        a_raw = ut @ v
    if not stopped:  # close: the newest column and its alpha
        k = len(U)
        u = ut.copy()
        for j in range(k):
            u -= c[j] * U[j]
        U.append(u)
        alpha.append(a_raw - (2.0 * c[k - 1] * beta[k - 1] if (k > 0 and use_da) else 0.0))
    return np.array(alpha), np.array(beta), np.array(U), repairs, cmax


def orthogonality(V):
    return float(np.abs(V @ V.T - np.eye(V.shape[0])).max())


def start_vector(n, seed=1234):
    return np.random.default_rng(seed).standard_normal(n)


def guard_start(n=60, small=1e-11):
    x = np.full(n, small)
    x[[3, 17, 29, 41, 53]] = 1.0
    return x
