"""A local, extended-precision check of Krylov steps, independent of the library: numpy longdouble / clongdouble on the host.

The operator is given by its CSR rows (rowptr, col, val) and a shift, which may be complex; the steps by the downloaded columns
u_0 .. u_k (as rows of U) and the recorded coefficients.  Every step is checked on its own, from the columns as they were stored:
hu = (H + shift) u_j in extended precision, r = hu - sum_{i <= j} (u_i^H hu) u_i, and then

  Lanczos (full re-orthogonalisation, interval 1)    Arnoldi (H = Basis.arnoldi_projected())
    |alpha_j - Re(u_j^H hu)|     <= bound              |H[i, j] - u_i^H hu|          <= bound   (i <= j)
    |beta_j - |r||               <= bound              |H[j + 1, j] - |r||           <= bound
    max |beta_j u_{j+1} - r|     <= bound              max |H[j + 1, j] u_{j+1} - r| <= bound

  max |U^H U - I| <= (n + k) eps
  bound = (n + k) eps (|H|_1 + |shift|),  |H|_1 the largest column sum of |val|, k the number of columns

which is the rounding of one application plus one combination (the form of _lowest in tests/test_gpu_spin_momentum.py).  Rounding
does not compound from step to step, so the bound does not depend on the number of steps; a wrong gathered element, scale, phase
or shift is of the order of the entries of u, ten orders of magnitude outside.  np.add.reduceat sums the rows from the starts
of the non-empty ones (an empty row's start is the next non-empty row's, so leaving it out cuts the products at the same
places); an empty row's sum is zero, so that (H + shift) u is shift u there.

Also the fp64 recurrences that tests/test_krylov_local_reference_host.py runs through the check beside those of
tests/one_sweep_reference.py (which are real): a two-sweep Lanczos for complex vectors and a plain Arnoldi with one or two
Gram-Schmidt passes."""
from __future__ import annotations

import numpy as np

EPS = float(np.finfo(np.float64).eps)
LD, CLD = np.longdouble, np.clongdouble


def norm1(n, col, val):
    """the largest column sum of |val| (0 for an operator without entries: a column that no row stores sums to zero)"""
    if n == 0 or np.size(val) == 0:
        return 0.0
    return float(np.bincount(np.asarray(col, np.int64), weights=np.abs(val), minlength=n).max())


def row_sums(prod, rowptr):
    """the sum of every row's products, zero for a row without entries"""
    rowptr = np.asarray(rowptr, np.int64)
    filled = rowptr[1:] > rowptr[:-1]
    if filled.all():
        return np.add.reduceat(prod, rowptr[:-1])
    out = np.zeros(filled.size, prod.dtype)
    if filled.any():
        out[filled] = np.add.reduceat(prod, rowptr[:-1][filled])
    return out


def bound(n, k, h1, shift):
    return (n + k) * EPS * (h1 + abs(complex(shift)))


def _wide(*arrays_and_scalars):
    """longdouble when everything is real, clongdouble else"""
    return CLD if any(np.iscomplexobj(a) for a in arrays_and_scalars) else LD


def applied(rows, shift, u, T=None):
    """(H + shift) u in extended precision"""
    rowptr, col, val = rows
    T = T or _wide(val, u, np.asarray(shift))
    u = np.asarray(u).astype(T)
    prod = np.asarray(val).astype(T) * u[np.asarray(col, np.int64)]
    return row_sums(prod, rowptr) + T(shift) * u


class Report(dict):
    """err_diag (alpha, or the column of H), err_norm (beta, or the coupling), err_vec (the next column), bound, ortho, ortho_bound"""

    def worst(self):
        return max(self["err_diag"], self["err_norm"], self["err_vec"])

    def ratio(self):
        if self["bound"] == 0.0:  # a zero operator without a shift: every product is an exact zero
            return 0.0 if self.worst() == 0.0 else float("inf")
        return self.worst() / self["bound"]

    def ok(self):
        return self.worst() <= self["bound"] and self["ortho"] <= self["ortho_bound"]

    def line(self, what=""):
        return (f"{what}: coefficient error {self['err_diag']:.3e}, norm error {self['err_norm']:.3e}, vector error {self['err_vec']:.3e}, "
                f"bound {self['bound']:.3e} (ratio {self.ratio():.3e}); orthogonality {self['ortho']:.3e}, bound {self['ortho_bound']:.3e}")


def _orthogonality(U, T):
    Uw = U.astype(T)
    return float(np.abs(Uw.conj() @ Uw.T - np.eye(U.shape[0])).max()) if U.shape[0] else 0.0


def _step(rows, shift, U, j, T):
    """hu, the coefficients u_i^H hu (i <= j) and r of step j"""
    hu = applied(rows, shift, U[j], T)
    Uw = U[: j + 1].astype(T)
    c = Uw.conj() @ hu
    return hu, c, hu - c @ Uw


def _norm(r):
    return np.sqrt((np.abs(r) ** 2).sum())


def check_lanczos(rows, shift, U, alpha, beta):
    """U: the stored columns as rows (k x n); alpha, beta: the recorded series.  Step j is checked as far as it was recorded:
    alpha_j for j < len(alpha) (and j < k), beta_j for j < len(beta), column j + 1 for j + 1 < k."""
    U = np.asarray(U)
    k, n = U.shape
    rowptr, col, val = rows
    T = _wide(val, U, np.asarray(shift))
    rep = Report(err_diag=0.0, err_norm=0.0, err_vec=0.0, bound=bound(n, k, norm1(n, col, val), shift), ortho=_orthogonality(U, T), ortho_bound=(n + k) * EPS)
    for j in range(min(k, len(alpha))):
        hu, c, r = _step(rows, shift, U, j, T)
        rep["err_diag"] = max(rep["err_diag"], float(abs(LD(alpha[j]) - c[j].real)))
        if j < len(beta):
            rep["err_norm"] = max(rep["err_norm"], float(abs(LD(beta[j]) - _norm(r))))
            if j + 1 < k:
                rep["err_vec"] = max(rep["err_vec"], float(np.abs(LD(beta[j]) * U[j + 1].astype(T) - r).max()))
    return rep


def check_arnoldi(rows, shift, U, H, residue=None, w=None):
    """U: the stored columns as rows (k x n); H: the projected matrix, (k + 1) x k or larger, whose coupling H[j + 1, j] the device
    writes when step j + 1 begins: for the last column the coupling is `residue` and the next column, unnormalised, is `w`
    (either may be None: not checked)."""
    U, H = np.asarray(U), np.asarray(H)
    k, n = U.shape
    rowptr, col, val = rows
    T = _wide(val, U, H, np.asarray(shift))
    rep = Report(err_diag=0.0, err_norm=0.0, err_vec=0.0, bound=bound(n, k, norm1(n, col, val), shift), ortho=_orthogonality(U, T), ortho_bound=(n + k) * EPS)
    for j in range(min(k, H.shape[1])):
        hu, c, r = _step(rows, shift, U, j, T)
        rep["err_diag"] = max(rep["err_diag"], float(np.abs(H[: j + 1, j].astype(T) - c).max()))
        if j + 1 < k:
            coupling = H[j + 1, j]
            rep["err_norm"] = max(rep["err_norm"], float(abs(T(coupling) - _norm(r))))
            rep["err_vec"] = max(rep["err_vec"], float(np.abs(T(coupling) * U[j + 1].astype(T) - r).max()))
        else:
            if residue is not None:
                rep["err_norm"] = max(rep["err_norm"], float(abs(LD(residue) - _norm(r))))
            if w is not None:
                rep["err_vec"] = max(rep["err_vec"], float(np.abs(np.asarray(w).astype(T) - r).max()))
    return rep


def dense_to_csr(A):
    """(rowptr, col, val) of a dense matrix: the non-zero entries and every diagonal entry, so that no row is empty"""
    A = np.asarray(A)
    keep = (A != 0) | np.eye(A.shape[0], dtype=bool)
    rowptr = np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.int64)
    return rowptr, np.nonzero(keep)[1].astype(np.int32), A[keep]


def csr_matmul(rows):
    """x -> H x in fp64 (complex when val or x is)"""
    rowptr, col, val = rows
    return lambda x: row_sums(val * x[col], rowptr)


# ---- fp64 recurrences, written like one_sweep_reference.batched --------------------------------------------------------------
def lanczos_fp64(apply, x, m, shift=0.0, threshold=1e-12, scaled_input=True, alpha_of=None):
    """m steps of the two-sweep Lanczos scheme for real or complex vectors.  Returns alpha, beta, V (columns as rows).
    scaled_input = False and alpha_of are the faults of tests/test_krylov_local_reference_host.py: the operator applied to the
    unnormalised vector while the column is normalised; alpha computed by alpha_of(u, v) instead of Re(u^H v)."""
    alpha_of = alpha_of or (lambda u, v: np.vdot(u, v).real)
    nrm = np.sqrt(np.vdot(x, x).real)
    raw = x
    V = [x * (1.0 / nrm)]

    def op(raw, u):
        t = u if scaled_input else raw
        return apply(t) + shift * t

    v = op(raw, V[0])
    alpha, beta = [alpha_of(V[0], v)], []
    for k in range(m):
        w0 = v - alpha[k] * V[k]
        if k > 0:
            w0 = w0 - beta[k - 1] * V[k - 1]
        h = [np.vdot(V[j], w0) for j in range(k + 1)]
        w = w0.copy()
        for j in range(k + 1):
            w -= h[j] * V[j]
        nrm = np.sqrt(np.vdot(w, w).real)
        beta.append(nrm)
        if nrm <= threshold:
            break
        V.append(w * (1.0 / nrm))
        v = op(w, V[-1])
        alpha.append(alpha_of(V[-1], v))
    return np.array(alpha), np.array(beta), np.array(V)


def arnoldi_fp64(apply, x, m, shift=0.0, passes=1, threshold=1e-12, scaled_input=True):
    """m calls of a plain Arnoldi step with `passes` classical Gram-Schmidt passes.  Returns V (columns as rows, at most m), the
    projected matrix ((nvec + 1) x nvec, every coupling but the last filled in), the last residue and the last unnormalised w."""
    w = np.asarray(x)
    residue = np.sqrt(np.vdot(w, w).real)
    V, cols, couplings = [], [], []
    for k in range(m):
        if residue <= threshold or k >= w.size:
            break
        if k > 0:
            couplings.append(residue)  # written when step k begins
        u = w * (1.0 / residue)
        V.append(u)
        t = u if scaled_input else w
        v = apply(t) + shift * t
        h = np.zeros(k + 1, v.dtype)
        w = v.copy()
        for _ in range(passes):
            d = np.array([np.vdot(V[j], w) for j in range(k + 1)])
            for j in range(k + 1):
                w = w - d[j] * V[j]
            h = h + d
        cols.append(h)
        residue = np.sqrt(np.vdot(w, w).real)
    nv = len(V)
    H = np.zeros((nv + 1, nv), cols[0].dtype if cols else np.float64)
    for k, h in enumerate(cols):
        H[: k + 1, k] = h
    for k, c in enumerate(couplings):
        H[k + 1, k] = c
    return np.array(V), H, residue, w
