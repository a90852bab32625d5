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
Gram-Schmidt passes.

The general step (library.hip: enq_orthogonalize over a column set first / stride / count followed by nq orthogonalizing vectors)
has the same check with the scheme restated: lanczos_columns, check_lanczos_general and check_arnoldi_general below, and the
fp64 recurrences lanczos_general_fp64 and arnoldi_general_fp64, which take the number-only faults (FAULTS) that
tests/test_general_step_reference_host.py shows the check to reject.

Restarted states (eigenex_lanczos_restart, eigenex_arnoldi_restart): check_lanczos and check_arnoldi take first = nkeep, the kept
columns have the relations check_kept_lanczos and check_kept_arnoldi (their bound is derived above them), and thick_restart_fp64 and
krylov_schur_fp64 are the fp64 recurrences with the number-only faults RESTART_FAULTS that
tests/test_restart_step_reference_host.py shows the checks to reject."""
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


def check_lanczos(rows, shift, U, alpha, beta, first=0):
    """U: the stored columns as rows (k x n); alpha, beta: the recorded series.  Step j is checked as far as it was recorded:
    alpha_j for j < len(alpha) (and j < k), beta_j for j < len(beta), column j + 1 for j + 1 < k.  first: the steps j < first are
    skipped (a restarted state: the columns below nkeep are Ritz vectors, and the series below nkeep are not defined);
    orthogonality is still taken over every column and the bound is the same."""
    U = np.asarray(U)
    k, n = U.shape
    rowptr, col, val = rows
    T = _wide(val, U, np.asarray(shift))
    rep = Report(err_diag=0.0, err_norm=0.0, err_vec=0.0, bound=bound(n, k, norm1(n, col, val), shift), ortho=_orthogonality(U, T), ortho_bound=(n + k) * EPS)
    for j in range(first, min(k, len(alpha))):
        hu, c, r = _step(rows, shift, U, j, T)
        rep["err_diag"] = max(rep["err_diag"], float(abs(LD(alpha[j]) - c[j].real)))
        if j < len(beta):
            rep["err_norm"] = max(rep["err_norm"], float(abs(LD(beta[j]) - _norm(r))))
            if j + 1 < k:
                rep["err_vec"] = max(rep["err_vec"], float(np.abs(LD(beta[j]) * U[j + 1].astype(T) - r).max()))
    return rep


def check_arnoldi(rows, shift, U, H, residue=None, w=None, first=0):
    """U: the stored columns as rows (k x n); H: the projected matrix, (k + 1) x k or larger, whose coupling H[j + 1, j] the device
    writes when step j + 1 begins: for the last column the coupling is `residue` and the next column, unnormalised, is `w`
    (either may be None: not checked).  first: the steps j < first are skipped (a restarted state: first = nkeep; column
    j >= nkeep of H is still compared on every row i <= j, the rows below nkeep are ordinary coefficients)."""
    U, H = np.asarray(U), np.asarray(H)
    k, n = U.shape
    rowptr, col, val = rows
    T = _wide(val, U, H, np.asarray(shift))
    rep = Report(err_diag=0.0, err_norm=0.0, err_vec=0.0, bound=bound(n, k, norm1(n, col, val), shift), ortho=_orthogonality(U, T), ortho_bound=(n + k) * EPS)
    for j in range(first, min(k, H.shape[1])):
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


# ---- the general step: a column set first / stride / count followed by nq orthogonalizing vectors ---------------------------------
# library.hip: enq_orthogonalize.  Every step is still checked on its own from the stored columns; what is restated is which vectors
# the step projects out and in which form.  With S vectors m_i in the step's set, c_i the coefficients of every pass and w0 the
# vector the passes start from,
#   bound_j = (n + k + nq) eps (|H|_1 + |shift|) max(1, sum_i |c_i| / |w0|_2)
# (the combination r = w0 - sum c_i m_i rounds every product c_i m_i; for an orthonormal set the factor is at most sqrt(S) per pass,
# and it is 1 on every case of the pass-mode suites within that factor).  Orthogonality is asserted only where the scheme promises
# it: every column against every column and every orthogonalizing vector, interval 1, orthonormal Q.
BATCHED, SEQUENTIAL, TWICE, ADAPTIVE = 0, 1, 2, 3  # capi.ORTHO_*
ETA2 = 0.5  # the adaptive scheme takes its second pass when |r_1|^2 < ETA2 |w0|^2 (library.hip: InlineDecide.eta2)


def lanczos_columns(k, interval, nq):
    """(the basis columns, the number of orthogonalizing vectors) that Lanczos step k, with k + 1 existing columns, projects out:
    library.hip, lanczos_columns"""
    if interval <= 0:
        return [], 0
    kmod = (k + 1) % interval
    return list(range(kmod, k + 1, interval)), (nq if kmod == 0 else 0)


def _q_rows(Q, n, dtype=None):
    Q = np.zeros((0, n)) if Q is None or len(Q) == 0 else np.asarray(Q)
    assert Q.ndim == 2 and Q.shape[1] == n
    return Q if dtype is None else Q.astype(dtype)


def _norm2(r):
    return (np.abs(r) ** 2).sum()


def _passes(w0, M, mode):
    """Gram-Schmidt of w0 against the rows of M in the scheme's form, in the precision of its arguments.  Sequential: one
    projection after another in the order of the rows.  Returns r, the coefficients summed over the passes, sum |c_i| over every
    pass, and |r_1|^2 / |w0|^2 after the first classical pass (None: sequential, no vector, or w0 = 0)."""
    S = M.shape[0]
    csum = np.zeros(S, w0.dtype)
    if S == 0:
        return w0, csum, LD(0), None
    if mode == SEQUENTIAL:
        r, cabs = w0.copy(), LD(0)
        for i in range(S):
            c = (M[i].conj() * r).sum()
            r = r - c * M[i]
            csum[i], cabs = c, cabs + abs(c)
        return r, csum, cabs, None
    c = M.conj() @ w0
    r = w0 - c @ M
    csum, cabs = csum + c, np.abs(c).sum()
    before, after = _norm2(w0), _norm2(r)
    if mode == TWICE or (mode == ADAPTIVE and after < LD(ETA2) * before):
        c = M.conj() @ r
        r = r - c @ M
        csum, cabs = csum + c, cabs + np.abs(c).sum()
    return r, csum, cabs, (float(after / before) if before > 0 else None)


def _start_mode(mode):
    """the start vector has no norm from before the pass: the adaptive scheme deflates it twice (library.hip: Before::Unknown)"""
    return TWICE if mode == ADAPTIVE else mode


class GeneralReport(Report):
    """Report with a bound per step: steps = [(j, err_diag, err_norm, err_vec, bound, S)], ratio() the worst error / bound over the
    steps (step_ratio) and the start vector (start_ratio); err_* and bound are those of the worst step; decisions =
    |r_1|^2 / |w0|^2 per Arnoldi step"""

    def ratio(self):
        return max(self["step_ratio"], self["start_ratio"])

    def ok(self):
        return self.ratio() <= 1.0 and self["ortho"] <= self["ortho_bound"]

    def line(self, what=""):
        return (f"{what}: worst step {self['worst_step']} ({self['worst_set']} vectors): coefficient error {self['err_diag']:.3e}, norm error "
                f"{self['err_norm']:.3e}, vector error {self['err_vec']:.3e}, bound {self['bound']:.3e}; start vector {self['err_start']:.3e}, bound "
                f"{self['start_bound']:.3e}; ratio {self.ratio():.3e}; orthogonality {self['ortho']:.3e}, bound {self['ortho_bound']:.3e}")

    def _ratio(self, err, bound):
        return err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))

    def add(self, j, err_diag, err_norm, err_vec, bound, S):
        self["steps"].append((j, err_diag, err_norm, err_vec, bound, S))
        ratio = self._ratio(max(err_diag, err_norm, err_vec), bound)
        if ratio >= self["step_ratio"]:
            self.update(step_ratio=ratio, worst_step=j, worst_set=S, err_diag=err_diag, err_norm=err_norm, err_vec=err_vec, bound=bound)

    def start(self, u0, r0, x0, nq):
        """column 0 against the deflated start vector: max | |r_0| u_0 - r_0 | <= (n + nq) eps |x0|_2"""
        self["err_start"] = float(np.abs(_norm(r0) * u0 - r0).max())
        self["start_bound"] = (x0.size + nq) * EPS * float(_norm(x0))
        self["start_ratio"] = self._ratio(self["err_start"], self["start_bound"])


def _general_report(n, k, Uw, Qw, x0, mode, orthonormal):
    rep = GeneralReport(err_diag=0.0, err_norm=0.0, err_vec=0.0, bound=0.0, step_ratio=0.0, start_ratio=0.0, worst_step=-1, worst_set=0, steps=[], decisions=[],
                        err_start=0.0, start_bound=0.0, ortho=0.0, ortho_bound=(n + k) * EPS)
    if x0 is not None and k > 0:
        x0w = np.asarray(x0).astype(Uw.dtype)
        rep.start(Uw[0], _passes(x0w, Qw, _start_mode(mode))[0], x0w, Qw.shape[0])
    if orthonormal and k > 0:
        rep["ortho"] = float(np.abs(Uw.conj() @ Uw.T - np.eye(k)).max())
        if Qw.shape[0]:
            rep["ortho"] = max(rep["ortho"], float(np.abs(Qw.conj() @ Uw.T).max()))
    return rep


def check_lanczos_general(rows, shift, U, Q, alpha, beta, interval=1, mode=BATCHED, x0=None, orthonormal=False):
    """check_lanczos for any interval, nq orthogonalizing vectors (the rows of Q) and any scheme.  Step j: hu = (H + shift) u_j,
    w0 = hu - alpha_j u_j - beta_{j-1} u_{j-1} with the recorded coefficients, r = w0 with lanczos_columns(j, interval, nq)
    projected out in the scheme's form: batched one classical pass, twice a second one on r, sequential one vector after another
    (columns ascending, then the orthogonalizing vectors), adaptive as batched (a pass with a recurrence is never adaptive).
    x0: the start vector, for the check of column 0.  orthonormal: Q is orthonormal, so that interval 1 promises orthogonality."""
    U = np.asarray(U)
    k, n = U.shape
    rowptr, col, val = rows
    T = _wide(val, U, np.asarray(shift), *([] if Q is None else [np.asarray(Q)]), *([] if x0 is None else [np.asarray(x0)]))
    Uw, Qw = U.astype(T), _q_rows(Q, n, T)
    nq = Qw.shape[0]
    base = (n + k + nq) * EPS * (norm1(n, col, val) + abs(complex(shift)))
    rep = _general_report(n, k, Uw, Qw, x0, mode, orthonormal and interval == 1)
    step_mode = BATCHED if mode == ADAPTIVE else mode
    for j in range(min(k, len(alpha))):
        hu = applied(rows, shift, U[j], T)
        err_diag = float(abs(LD(alpha[j]) - (Uw[j].conj() * hu).sum().real))
        err_norm, err_vec, factor, S = 0.0, 0.0, 1.0, 0
        if j < len(beta):
            w0 = hu - T(alpha[j]) * Uw[j]
            if j > 0:
                w0 = w0 - T(beta[j - 1]) * Uw[j - 1]
            cols, nqu = lanczos_columns(j, interval, nq)
            M = np.concatenate([Uw[np.asarray(cols, np.int64)], Qw[:nqu]])
            r, _, cabs, _ = _passes(w0, M, step_mode)
            S, nw = M.shape[0], _norm(w0)
            factor = max(1.0, float(cabs / nw)) if nw > 0 else 1.0
            err_norm = float(abs(LD(beta[j]) - _norm(r)))
            if j + 1 < k:
                err_vec = float(np.abs(LD(beta[j]) * Uw[j + 1] - r).max())
        rep.add(j, err_diag, err_norm, err_vec, base * factor, S)
    return rep


def check_arnoldi_general(rows, shift, U, Q, H, residue=None, w=None, mode=BATCHED, x0=None, orthonormal=False):
    """check_arnoldi with nq orthogonalizing vectors and any scheme.  Step j: w0 = hu, the set is the columns 0 .. j and every
    orthogonalizing vector (sequential: those first); adaptive takes the second pass exactly when |r_1|^2 < 0.5 |hu|^2 in
    extended precision; H[:j + 1, j] is the sum of the passes' coefficients of the basis columns.  The report's decisions are
    |r_1|^2 / |hu|^2 per step."""
    U, H = np.asarray(U), np.asarray(H)
    k, n = U.shape
    rowptr, col, val = rows
    T = _wide(val, U, H, np.asarray(shift), *([] if Q is None else [np.asarray(Q)]), *([] if x0 is None else [np.asarray(x0)]))
    Uw, Qw = U.astype(T), _q_rows(Q, n, T)
    nq = Qw.shape[0]
    base = (n + k + nq) * EPS * (norm1(n, col, val) + abs(complex(shift)))
    rep = _general_report(n, k, Uw, Qw, x0, mode, orthonormal)
    for j in range(min(k, H.shape[1])):
        hu = applied(rows, shift, U[j], T)
        M, basis = (np.concatenate([Qw, Uw[: j + 1]]), slice(nq, None)) if mode == SEQUENTIAL else (np.concatenate([Uw[: j + 1], Qw]), slice(0, j + 1))
        r, csum, cabs, decision = _passes(hu, M, mode)
        rep["decisions"].append(decision)
        nw = _norm(hu)
        factor = max(1.0, float(cabs / nw)) if nw > 0 else 1.0
        err_diag = float(np.abs(H[: j + 1, j].astype(T) - csum[basis]).max())
        err_norm, err_vec = 0.0, 0.0
        if j + 1 < k:
            coupling = T(H[j + 1, j])
            err_norm = float(abs(coupling - _norm(r)))
            err_vec = float(np.abs(coupling * Uw[j + 1] - r).max())
        else:
            if residue is not None:
                err_norm = float(abs(LD(residue) - _norm(r)))
            if w is not None:
                err_vec = float(np.abs(np.asarray(w).astype(T) - r).max())
        rep.add(j, err_diag, err_norm, err_vec, base * factor, M.shape[0])
    return rep


# ---- the fp64 recurrences of the general step, with the faults the check must reject ----------------------------------------------
FAULTS = (
    "first_plus_one",      # the column set's `first` moved by one (a column beyond the newest is left out)
    "drop_newest",         # the newest selected column left out
    "q_every_step",        # Lanczos: the orthogonalizing vectors used on every step
    "q_no_step",           # the orthogonalizing vectors used on no step after the start
    "q_reversed",          # sequential: the orthogonalizing vectors projected in reverse order
    "q_first_flip",        # sequential: orthogonalizing vectors first where they come last, and the other way round
    "skip_second",         # twice: the second pass omitted
    "eta_quarter",         # adaptive: the decision taken with 0.25
    "always_second",       # adaptive: the second pass always taken
    "never_second",        # adaptive: the second pass never taken
    "no_conj_q",           # complex: the conjugate dropped on the orthogonalizing vectors' dots
    "swap_budget",         # a set beyond the dots budget: the coefficients at budget - 1 and budget exchanged
    "start_not_deflated",  # the start vector not deflated
)


def _gs64(w0, B, Qm, mode, q_first, fault=None, budget=None):
    """fp64 Gram-Schmidt of w0 against the rows of B (basis columns) and Qm (orthogonalizing vectors) as the device orders them.
    Returns w and the coefficients of the rows of B summed over the passes."""
    nb, S = B.shape[0], B.shape[0] + Qm.shape[0]
    if S == 0:
        return w0.copy(), np.zeros(0, w0.dtype)
    M = np.concatenate([B, Qm]).astype(w0.dtype)

    def dots(w):
        c = M.conj() @ w
        if fault == "no_conj_q":
            c[nb:] = M[nb:] @ w
        if fault == "swap_budget" and budget is not None and S > budget:
            c[[budget - 1, budget]] = c[[budget, budget - 1]]
        return c

    if mode == SEQUENTIAL:
        qs = list(range(nb, S))
        if fault == "q_reversed":
            qs.reverse()
        order = qs + list(range(nb)) if q_first != (fault == "q_first_flip") else list(range(nb)) + qs
        w, h = w0.copy(), np.zeros(S, w0.dtype)
        for i in order:
            h[i] = M[i] @ w if (fault == "no_conj_q" and i >= nb) else np.vdot(M[i], w)
            w = w - h[i] * M[i]
        return w, h[:nb]
    c = dots(w0)
    w = w0 - c @ M
    h = c.copy()
    if mode == TWICE:
        second = fault != "skip_second"
    elif mode == ADAPTIVE:
        eta2 = 0.25 if fault == "eta_quarter" else ETA2
        second = fault == "always_second" or (fault != "never_second" and np.vdot(w, w).real < eta2 * np.vdot(w0, w0).real)
    else:
        second = False
    if second:
        c = dots(w)
        w = w - c @ M
        h = h + c
    return w, h[:nb]


def _start64(x, Qa, mode, fault, budget):
    """the start vector deflated by Q in the scheme's form (library.hip: enq_initial_vector)"""
    dtype = np.result_type(np.asarray(x).dtype, Qa.dtype, np.float64)
    w = np.asarray(x).astype(dtype)
    if Qa.shape[0] and fault != "start_not_deflated":
        w, _ = _gs64(w, Qa[:0], Qa, _start_mode(mode), True, fault, budget)
    return w


def lanczos_general_fp64(apply, x, m, shift=0.0, interval=1, Q=None, mode=BATCHED, fault=None, budget=None, threshold=1e-12):
    """lanczos_fp64 (m steps: alpha of m + 1, beta of m, m + 1 columns) with the general column set, nq orthogonalizing vectors
    (rows of Q), the scheme and one of FAULTS.  budget: the vectors one dots launch takes (swap_budget)."""
    n = np.asarray(x).size
    Qa = _q_rows(Q, n)
    nq = Qa.shape[0]
    step_mode = BATCHED if mode == ADAPTIVE else mode
    w = _start64(x, Qa, mode, fault, budget)
    nrm = np.sqrt(np.vdot(w, w).real)
    V = [w * (1.0 / nrm)]
    v = apply(V[0]) + shift * V[0]
    alpha, beta = [np.vdot(V[0], v).real], []
    for k in range(m):
        w0 = v - alpha[k] * V[k]
        if k > 0:
            w0 = w0 - beta[k - 1] * V[k - 1]
        cols, nqu = lanczos_columns(k, interval, nq)
        if fault == "first_plus_one":
            cols = [c + 1 for c in cols if c + 1 <= k]
        elif fault == "drop_newest":
            cols = cols[:-1]
        elif fault == "q_every_step":
            nqu = nq
        elif fault == "q_no_step":
            nqu = 0
        B = np.array([V[c] for c in cols]).reshape(len(cols), n)
        w, _ = _gs64(w0, B, Qa[:nqu], step_mode, False, fault, budget)
        nrm = np.sqrt(np.vdot(w, w).real)
        beta.append(nrm)
        if nrm <= threshold:
            break
        V.append(w * (1.0 / nrm))
        v = apply(V[-1]) + shift * V[-1]
        alpha.append(np.vdot(V[-1], v).real)
    return np.array(alpha), np.array(beta), np.array(V)


def arnoldi_general_fp64(apply, x, m, shift=0.0, Q=None, mode=BATCHED, fault=None, budget=None, threshold=1e-12):
    """arnoldi_fp64 (m calls) with nq orthogonalizing vectors, the scheme and one of FAULTS"""
    n = np.asarray(x).size
    Qa = _q_rows(Q, n)
    w = _start64(x, Qa, mode, fault, budget)
    residue = np.sqrt(np.vdot(w, w).real)
    V, cols, couplings = [], [], []
    for k in range(m):
        if residue <= threshold or k >= n:
            break
        if k > 0:
            couplings.append(residue)
        V.append(w * (1.0 / residue))
        v = apply(V[-1]) + shift * V[-1]
        sel = list(range(k + 1))
        if fault == "first_plus_one":
            sel = sel[1:]
        elif fault == "drop_newest":
            sel = sel[:-1]
        B = np.array([V[c] for c in sel]).reshape(len(sel), n)
        w, h = _gs64(v, B, Qa[:0] if fault == "q_no_step" else Qa, mode, True, fault, budget)
        col = np.zeros(k + 1, v.dtype)
        col[sel] = h
        cols.append(col)
        residue = np.sqrt(np.vdot(w, w).real)
    nv = len(V)
    H = np.zeros((nv + 1, nv), cols[0].dtype if cols else np.float64)
    for k, h in enumerate(cols):
        H[: k + 1, k] = h
    for k, c in enumerate(couplings):
        H[k + 1, k] = c
    return np.array(V), H, residue, w


# ---- restarted states: eigenex_lanczos_restart (thick restart) and eigenex_arnoldi_restart (Krylov-Schur) ---------------------
# A restart keeps the columns Y = V_m C (C = S, eigenvectors of T_m, or Q, an orthonormal basis of an invariant subspace of H_m) and
# continues with ordinary steps from column nkeep on.  The steps behind it are checked as before with first = nkeep.  The kept
# columns were made by no step, but they inherit a relation from the steps of the cycle before:
#
#   Lanczos    (H + shift) y_e = theta_e y_e + s_e u_m,               s_e = beta_{m-1} S[m-1, e]
#   Arnoldi    (H + shift) Y   = Y B_top + w q_last^T,                q_last = Q[m-1, :], w the unnormalised residual
#
# Derivation of the bound.  Every old step j holds (H + shift) v_j = sum_i T_ij v_i + f_j with a local error |f_j| <= bound
# (the check above), and y_e = sum_j C_je v_j.  So (H + shift) y_e - sum_i (T C)_ie v_i - (coupling) = sum_j C_je f_j, which is
# at most bound * sum_j |C_je| entry by entry; forming y_e itself rounds once more per entry (the "1 +"; tests/ritz_reference.py
# holds that part to its own bound); and T C = C diag(theta) (or C B_top) holds to the small eigenproblem's residual m eps |T|,
# which multiplies columns of norm one and is below n eps |H|_1, already inside `bound`.  Hence
#
#   kept bound = (n + k) eps (|H|_1 + |shift|) (1 + max_e sum_j |C_je|),     k = m + 1 columns of the cycle before
#
# (sum_j |C_je| <= sqrt(m) for a unit column).  A restart of a restarted state inherits the same relation: its old columns
# y_e satisfy it in place of a step's, within the same order.
class KeptReport(dict):
    """err, bound and the factor 1 + max_e sum_j |C_je| of a kept relation"""

    def ratio(self):
        if self["bound"] == 0.0:
            return 0.0 if self["err"] == 0.0 else float("inf")
        return self["err"] / self["bound"]

    def ok(self):
        return self["err"] <= self["bound"]

    def line(self, what=""):
        return f"{what}: kept relation {self['err']:.3e}, bound {self['bound']:.3e} (factor {self['factor']:.3f}, ratio {self.ratio():.3e})"


def _kept_report(err, rows, shift, n, coef, nkeep):
    rowptr, col, val = rows
    if coef is None:  # the weights are not known: as if every kept column were one old column
        factor, k = 2.0, nkeep + 1
    else:
        coef = np.asarray(coef)
        factor, k = 1.0 + float(np.abs(coef).sum(0).max()), coef.shape[0] + 1
    return KeptReport(err=float(err), factor=factor, bound=bound(n, k, norm1(n, col, val), shift) * factor)


def check_kept_lanczos(rows, shift, Y, u, theta, s, coef=None):
    """max_e max |(H + shift) y_e - theta_e y_e - s_e u| in extended precision.  Y: the kept columns as rows (nkeep x n), u: the
    residual direction (column nkeep after the restart), theta: their Ritz values, s: their couplings beta_{m-1} S[m-1, e];
    coef = S (m x nkeep) gives the bound its factor (derivation above)."""
    Y, u = np.asarray(Y), np.asarray(u)
    nkeep, n = Y.shape
    T = _wide(rows[2], Y, u, np.asarray(shift))
    uw, err = u.astype(T), 0.0
    for e in range(nkeep):
        r = applied(rows, shift, Y[e], T) - LD(theta[e]) * Y[e].astype(T) - LD(s[e]) * uw
        err = max(err, float(np.abs(r).max()))
    return _kept_report(err, rows, shift, n, coef, nkeep)


def check_kept_arnoldi(rows, shift, Y, B_top, w, q_last, coef=None):
    """max |(H + shift) Y - Y B_top - w q_last^T| in extended precision.  Y: the kept columns as rows (nkeep x n), B_top: nkeep x
    nkeep, w: the unnormalised residual the restart leaves untouched, q_last = Q[m-1, :] (not conjugated); coef = Q (m x nkeep)
    gives the bound its factor (derivation above)."""
    Y, B_top, w, q_last = np.asarray(Y), np.asarray(B_top), np.asarray(w), np.asarray(q_last)
    nkeep, n = Y.shape
    T = _wide(rows[2], Y, B_top, w, q_last, np.asarray(shift))
    Yw, ww, Bw, err = Y.astype(T), w.astype(T), B_top.astype(T), 0.0
    for e in range(nkeep):
        r = applied(rows, shift, Y[e], T) - Bw[:, e] @ Yw - T(q_last[e]) * ww
        err = max(err, float(np.abs(r).max()))
    return _kept_report(err, rows, shift, n, coef, nkeep)


RESTART_FAULTS = (
    "alpha_from_previous",         # Lanczos: alpha[nkeep] taken from alpha[m - 1]
    "residual_column_previous",    # Lanczos: column nkeep is u_{m-1}
    "stale_v",                     # Lanczos: the operator output kept is that of the last kept Ritz vector, not of u_m
    "second_chunk_repeats_first",  # kept vector E + e built from the coefficients of vector e (E = 16; complex Arnoldi: 8)
    "last_basis_column_dropped",   # Y = V[:m - 1] C[:m - 1]
    "kept_columns_not_projected",  # the first step orthogonalises against the columns >= nkeep - 1 only
    "coupling_overwritten",        # Arnoldi: H[nkeep, nkeep - 1] set to the residue by the first step
    "coupling_row_conjugated",     # complex Arnoldi: row nkeep of B stored as its conjugate
)


def _kept_columns(V, C, fault, chunk):
    """Y = C^T V (V: the old columns as rows, C: m x nkeep) with the faults of the combination.  Summed in extended precision and
    rounded once: the bound of tests/ritz_reference.py is a tight one ((m + 8) u sum |C||V| + 8 u |y| per entry), of which a plain
    fp64 sum of 24 products uses 0.07 to 0.12 somewhere among 30 000 entries whatever the input; rounded once, at most 1/16."""
    C = np.array(C)
    T = _wide(C, V)
    if fault == "second_chunk_repeats_first":
        for e in range(chunk, C.shape[1]):
            C[:, e] = C[:, e - chunk]
    if fault == "last_basis_column_dropped":
        C[-1] = 0.0
    return (C.T.astype(T) @ np.asarray(V).astype(T)).astype(np.result_type(C.dtype, np.asarray(V).dtype))


def _mode64(mode):
    return BATCHED if mode == ADAPTIVE else mode  # Lanczos: a pass with a recurrence is never adaptive


def _lanczos_extend64(apply, shift, V, v, alpha, beta, upto, mode_of, threshold, narrow_at=None):
    """Lanczos steps k = len(V) - 1 .. upto - 1 (full re-orthogonalisation) on lists that grow in place; returns the last v"""
    for k in range(len(V) - 1, upto):
        w0 = v - alpha[k] * V[k]
        if k > 0:
            w0 = w0 - beta[k - 1] * V[k - 1]
        lo = k - 1 if narrow_at == k else 0
        w, _ = _gs64(w0, np.array(V[lo: k + 1]), np.zeros((0, w0.size), w0.dtype), _mode64(mode_of(k)), False)
        nrm = np.sqrt(np.vdot(w, w).real)
        beta.append(nrm)
        if nrm <= threshold:
            break
        V.append(w * (1.0 / nrm))
        v = apply(V[-1]) + shift * V[-1]
        alpha.append(np.vdot(V[-1], v).real)
    return v


def restart_T(theta, s, alpha, beta, m):
    """the projected matrix of a restarted cycle as the front-end builds it (thick_restart_lanczos.hpp): diag(theta), the border
    s in row and column nkeep, and the tridiagonal tail from alpha[nkeep ..] and beta[nkeep ..]; nothing of the series below nkeep"""
    nkeep = len(theta)
    T = np.zeros((m, m))
    T[np.arange(nkeep), np.arange(nkeep)] = theta
    if 0 < nkeep < m:
        T[nkeep, :nkeep] = T[:nkeep, nkeep] = s
    for j in range(nkeep, m):
        T[j, j] = alpha[j]
        if j + 1 < m:
            T[j + 1, j] = T[j, j + 1] = beta[j]
    return T


def thick_restart_fp64(apply, x, m, nkeep, cycles=1, shift=0.0, first=TWICE, rest=BATCHED, fault=None, kept=None, threshold=1e-12):
    """What the device holds after m + 1 Lanczos calls (scheme `rest`) and then after each of `cycles` thick restarts keeping
    nkeep Ritz vectors (kept: their indices in ascending Ritz values, default the lowest nkeep) followed by m - nkeep calls, the
    first in the scheme `first`, the others in `rest`.  Returns a list: [0] = dict(alpha, beta, U); [c] = dict(V: the columns
    before the restart, theta, S (m x nkeep), s, coupling_last, Y: the nkeep + 1 columns right after it, alpha, beta, U: after the
    steps).  The series below nkeep are left stale as the device leaves them.  fault: one of RESTART_FAULTS, in every restart."""
    x = np.asarray(x)
    nrm = np.sqrt(np.vdot(x, x).real)
    V = [x * (1.0 / nrm)]
    v = apply(V[0]) + shift * V[0]
    alpha, beta = [np.vdot(V[0], v).real], []
    v = _lanczos_extend64(apply, shift, V, v, alpha, beta, m, lambda k: rest, threshold)
    out = [dict(alpha=np.array(alpha), beta=np.array(beta), U=np.array(V))]
    T = restart_T([], [], alpha, beta, m)
    sel = np.arange(nkeep) if kept is None else np.asarray(kept)
    for _ in range(cycles):
        Vold = np.array(V)
        theta_all, S_all = np.linalg.eigh(T)
        theta, S = theta_all[sel], np.ascontiguousarray(S_all[:, sel])
        s = beta[m - 1] * S[m - 1]
        Y = _kept_columns(Vold[:m], S, fault, 16)
        u = Vold[m - 1] if fault == "residual_column_previous" else Vold[m]
        if fault == "stale_v":
            v = apply(Y[nkeep - 1]) + shift * Y[nkeep - 1]
        a_m = alpha[m - 1] if fault == "alpha_from_previous" else alpha[m]
        alpha, beta = list(alpha[:nkeep]) + [a_m], list(beta[: nkeep - 1]) + [s[nkeep - 1]]
        V = list(Y) + [u]
        after = np.array(V)
        v = _lanczos_extend64(apply, shift, V, v, alpha, beta, m, lambda k: first if k == nkeep else rest, threshold,
                              nkeep if fault == "kept_columns_not_projected" else None)
        out.append(dict(V=Vold, theta=theta, S=S, s=s, coupling_last=s[nkeep - 1], Y=after, alpha=np.array(alpha), beta=np.array(beta), U=np.array(V)))
        if nkeep == m or len(V) < m + 1:  # the whole of T was kept (u_m then couples to every column, which no front-end asks
            break                         # for): one restart; or a breakdown (a fault's): nothing to restart from
        T = restart_T(theta, s, alpha, beta, m)
    return out


def krylov_schur_fp64(apply, x, m, nkeep, cycles=1, shift=0.0, first=BATCHED, rest=BATCHED, fault=None, threshold=1e-12, basis=None):
    """What the device holds after m Arnoldi calls and then after each of `cycles` Krylov-Schur restarts keeping nkeep vectors
    (basis(H_m, nkeep, residue) -> k, Q, B, theta; default krylov_schur_reference.restart_basis, which may move k by one for a
    conjugate pair on the cut) followed by m - k calls, the first in the scheme `first`, the others in `rest`.  Returns a list:
    [0] = dict(U, H, residue, w); [c] = dict(V: the columns before the restart, k, Q, B, w0, residue0 (untouched by the restart),
    Y: the k columns right after it, U, H, residue, w: after the steps).  fault: one of RESTART_FAULTS, in every restart."""
    if basis is None:
        from krylov_schur_reference import restart_basis as basis
    V, H, residue, w = arnoldi_general_fp64(apply, x, m, shift, None, rest, None, None, threshold)
    out = [dict(U=V, H=H, residue=residue, w=w)]
    cplx = np.iscomplexobj(V)
    for _ in range(cycles):
        Vold, w0, residue0 = V, w, residue
        k, Q, B, _ = basis(H[:m], nkeep, residue)
        Y = _kept_columns(Vold, Q, fault, 8 if cplx else 16)
        Hn = np.zeros((m + 1, m), H.dtype)
        Hn[: k + 1, :k] = B
        if fault == "coupling_row_conjugated":
            Hn[k, :k] = np.conj(B[k])
        cols = list(Y)
        for j in range(k, m):
            if j > k or fault == "coupling_overwritten":
                Hn[j, j - 1] = residue  # written when step j begins; the first step after a restart leaves B's entry
            cols.append(w * (1.0 / residue))
            hv = apply(cols[-1]) + shift * cols[-1]
            lo = k - 1 if (fault == "kept_columns_not_projected" and j == k) else 0
            w, h = _gs64(hv, np.array(cols[lo:]), np.zeros((0, hv.size), hv.dtype), first if j == k else rest, True)
            Hn[lo: j + 1, j] = h
            residue = np.sqrt(np.vdot(w, w).real)
        V, H = np.array(cols), Hn
        out.append(dict(V=Vold, k=k, Q=Q, B=B, w0=w0, residue0=residue0, Y=Y, U=V, H=H, residue=residue, w=w))
    return out
