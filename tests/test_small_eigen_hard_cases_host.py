"""The six host dense eigen-solvers of small_eigen.hpp (tridiagonal, symmetric, hermitian, hessenberg, hessenberg_real_values,
general) on matrices that are hard for them, held to a backward-error criterion computed in np.longdouble.  No GPU.

The criterion, for every routine that returns vectors (columns normalised to unit length, ||A||_1 the largest absolute column sum):
    max |A x_k - lambda_k x_k| <= n eps ||A||_1
and for tridiagonal, symmetric and hermitian also
    max |X^H X - I| <= n eps             (the columns as returned)
    |lambda - lambda_LAPACK| <= n eps ||A||_1   against numpy.linalg.eigvalsh (symmetric and hermitian).
Every case prints its residual and orthogonality as fractions of these bounds before it asserts (profiles/small_eigen_hard_cases.md
holds them).  Values-only results: the sum of the values against the trace within n^2 eps ||A||_1 (the values are the exact ones of
A + E with |E| within the criterion, and a trace moves by at most n max|E_ii|), and hessenberg_real_values against hessenberg as
multisets at 1e-6 of the matrix's scale, the tolerance of tests/test_cabi_and_host_logic.py.  The spectra of the non-normal matrices
(Frank, companion, the defective bidiagonal one) are ill-conditioned, so they are not compared with LAPACK's; the defective matrix
(one Jordan block of order 10: a perturbation of eps moves its eigenvalue by eps^(1/10) = 0.03) is held to residual and trace alone.

tridiagonal, symmetric, hessenberg and hessenberg_real_values are reached through solver.py, which raises EigenexError when the
routine returns false; hermitian and general through tests/cpp/small_eigen_hard_cases.cpp, built once as it is and once with
AddressSanitizer + UBSan.  On the commit before the column-tail fix of symmetric(), the 3 x 3 cases with t <= 1e-8, the T + E cases,
the corner case of hermitian and the silent results of symmetric and general at 2^-600 fail; see the profile note for the figures."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spin_rdm_reference as rr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
CLD = np.clongdouble
EPS = float(np.finfo(np.float64).eps)
PROGRAM_MODES = ("hermitian", "hermitian_values", "general", "general_values", "hessenberg")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g

    g.build()
    from cmpt_eigenex_amd import capi, solver

    return capi, solver


def _compile(tmp, name, extra):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", *extra, "-I", os.path.join(ROOT, "cmpt-eigenex_amd", "include"),
                           os.path.join(ROOT, "tests", "cpp", "small_eigen_hard_cases.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """run(mode, A) -> (ok, values, vectors or None) through the stand-alone program, with a time limit of a few seconds"""
    tmp = tmp_path_factory.mktemp("small_eigen_hard_cases")
    exe = _compile(tmp, "small_eigen_hard_cases", [])
    count = [0]

    def run(mode, A, exe=exe):
        assert mode in PROGRAM_MODES
        A = np.asarray(A, np.complex128)
        n = A.shape[0]
        count[0] += 1
        path = str(tmp / f"matrix_{count[0]}.txt")
        with open(path, "w") as f:
            f.write(f"{mode} {n}\n")
            f.writelines(f"{float(e.real)!r} {float(e.imag)!r}\n" for e in A.T.ravel())  # column-major
        out = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=10)
        assert out.returncode == 0 and not out.stderr, (out.returncode, out.stderr.decode()[-2000:])
        return _parse(out.stdout.decode(), mode, n) + (out.stdout,)

    run.tmp = tmp
    return run


def _parse(text, mode, n):
    ok, values, vectors = [ln.split() for ln in text.splitlines()]
    assert (ok[0], values[0], vectors[0]) == ("ok", "values", "vectors")
    v = np.array([float(x) for x in values[1:]])
    if not mode.startswith("hermitian"):
        v = v[0::2] + 1j * v[1::2]
    assert v.size == n
    x = np.array([float(t) for t in vectors[1:]])
    X = None
    if not mode.endswith("_values"):
        X = (x[0::2] + 1j * x[1::2]).reshape(n, n).T  # column-major -> [row, col]
    else:
        assert x.size == 0
    return int(ok[1]) == 1, v, X


# ---------------------------------------------------------------------------------------------------------------------------
# the criterion
# ---------------------------------------------------------------------------------------------------------------------------
def norm1(A):
    return np.abs(np.asarray(A).astype(CLD)).sum(axis=0).max() if np.asarray(A).size else LD(0)


def fractions(A, values, X, orthonormal, product=None):
    """(max |A x - lambda x| / (n eps ||A||_1), max |X^H X - I| / (n eps) or None), in np.longdouble; nan where the result is not
    finite or a column is zero, which no assertion below lets pass.  product(U): A U in long double for a matrix with a structure
    (the dense product of order 400 takes seconds)"""
    A, X, lam = np.asarray(A).astype(CLD), np.asarray(X).astype(CLD), np.asarray(values).astype(CLD)
    n = A.shape[0]
    with np.errstate(all="ignore"):
        unit = X / np.sqrt((np.abs(X) ** 2).sum(axis=0))
        res = np.abs((A @ unit if product is None else product(unit)) - unit * lam).max()
        bound = n * LD(EPS) * norm1(A)
        rf = float(res / bound) if bound > 0 else (0.0 if res == 0 else float("inf"))
        of = float(np.abs(X.conj().T @ X - np.eye(n)).max() / (n * LD(EPS))) if orthonormal else None
    return rf, of


def holds(routine, family, A, values, X, orthonormal, lapack=None, product=None):
    """assert the criterion; prints the fractions first"""
    n = np.asarray(A).shape[0]
    rf, of = fractions(A, values, X, orthonormal, product)
    lf = None
    if lapack is not None:
        bound = n * LD(EPS) * norm1(A)
        diff = np.abs(np.asarray(values).astype(LD) - np.asarray(lapack).astype(LD)).max()
        lf = float(diff / bound) if bound > 0 else (0.0 if diff == 0 else float("inf"))
    print(f"FRACTION {routine} {family} n={n} residual={rf:.3g} orthogonality={'-' if of is None else format(of, '.3g')} "
          f"lapack={'-' if lf is None else format(lf, '.3g')}")
    assert rf <= 1.0, f"{routine} {family}: residual {rf:.3g} of n eps ||A||_1"
    assert of is None or of <= 1.0, f"{routine} {family}: orthogonality {of:.3g} of n eps"
    assert lf is None or lf <= 1.0, f"{routine} {family}: eigenvalues off LAPACK's by {lf:.3g} of n eps ||A||_1"
    return rf, of


def trace_holds(routine, family, A, values):
    """|sum lambda - tr A| <= n^2 eps ||A||_1"""
    A = np.asarray(A).astype(CLD)
    n = A.shape[0]
    off = np.abs(np.asarray(values).astype(CLD).sum() - np.trace(A))
    bound = n * n * LD(EPS) * norm1(A)
    print(f"TRACE {routine} {family} n={n} off={float(off / bound) if bound > 0 else float(off):.3g} of n^2 eps ||A||_1")
    assert off <= bound, f"{routine} {family}: the values add up to the trace + {float(off):.3e}, bound {float(bound):.3e}"


def same_multiset(got, want, tol, label):
    want = list(want)
    assert len(got) == len(want)
    for v in got:
        k = int(np.argmin([abs(v - r) for r in want]))
        d = abs(v - want.pop(k))
        assert d <= tol, f"{label}: {v} is {d:.3e} from its nearest partner, tolerance {tol:.3e}"


def eigvalsh(A, scale=1.0):
    """LAPACK's eigenvalues of A * scale, taken of A: scale is a power of two where A * scale would strain LAPACK itself"""
    return np.linalg.eigvalsh(np.asarray(A)) * scale


# ---------------------------------------------------------------------------------------------------------------------------
# the families
# ---------------------------------------------------------------------------------------------------------------------------
def wilkinson21():
    return np.abs(np.arange(21) - 10.0), np.ones(20)


def lanczos_t(steps=400):
    """T of `steps` Lanczos steps without re-orthogonalisation on diag(linspace(0, 1, 200), 3, 5): the two outliers converge within a
    few steps and come back as ghost copies, more than twenty of each: clusters of eigenvalues equal to rounding"""
    d = np.concatenate([np.linspace(0.0, 1.0, 200), [3.0, 5.0]])
    v = np.random.default_rng(7).standard_normal(d.size)
    v /= np.linalg.norm(v)
    before, b, alpha, beta = np.zeros_like(v), 0.0, [], []
    for _ in range(steps):
        w = d * v - b * before
        a = float(w @ v)
        w -= a * v
        b = float(np.linalg.norm(w))
        alpha.append(a), beta.append(b)
        before, v = v, w / b
    return np.array(alpha), np.array(beta[:-1])


def tridiagonal_families():
    d, e = wilkinson21()
    glued_e = np.concatenate([np.concatenate([e, [1e-8]]) for _ in range(5)])[:-1]
    graded = 10.0 ** -np.arange(30)
    clement = np.sqrt(np.arange(1, 50) * (50.0 - np.arange(1, 50)))
    out = {
        "wilkinson21": (d, e),
        "wilkinson21_x5_glued_1e-8": (np.tile(d, 5), glued_e),
        "graded_down_1e-29": (graded, 0.5 * graded[1:]),
        "graded_up_1e-29": (graded[::-1].copy(), 0.5 * graded[1:][::-1]),
        "clement50": (np.zeros(50), clement),
        "lanczos_ghosts400": lanczos_t(),
        "wilkinson21_x1e200": (d * 1e200, e * 1e200),
        "wilkinson21_x1e-200": (d * 1e-200, e * 1e-200),
        "zeros5": (np.zeros(5), np.zeros(4)),
    }
    return out


def dense_tridiagonal(d, e):
    return np.diag(d) + np.diag(e, 1) + np.diag(e, -1)


def tridiagonal_product(d, e):
    """U -> T U in long double, row by row of the three diagonals"""
    d, e = np.asarray(d).astype(LD)[:, None], np.asarray(e).astype(LD)[:, None]

    def product(U):
        out = d * U
        out[1:] += e * U[:-1]
        out[:-1] += e * U[1:]
        return out

    return product


def three_by_three(t):
    return np.array([[2.0, 1.0, t], [1.0, 3.0, 0.5], [t, 0.5, 4.0]])


def arrowhead():
    """the projected matrix of a thick restart: 5 Ritz values, their couplings to the first new vector (1e-12 .. 1e-9 for the
    converged ones next to 0.2 .. 0.5), and a tridiagonal tail of 4"""
    A = np.diag([-2.0, -1.5, -1.1, -0.7, -0.2, 0.3, 0.8, 1.1, 1.9])
    for i, s in enumerate([1e-12, 0.3, 1e-10, 0.5, 1e-9]):
        A[5, i] = A[i, 5] = s
    for i, b in zip(range(5, 8), [0.4, 0.2, 0.45]):
        A[i + 1, i] = A[i, i + 1] = b
    return A


def with_spectrum(lam, seed):
    Q = np.linalg.qr(np.random.default_rng(seed).standard_normal((len(lam), len(lam))))[0]
    A = (Q * lam) @ Q.T
    return (A + A.T) / 2


def repeated_exactly():
    """H D H^T / 8 with the Hadamard matrix of order 8 and small integers in D: every entry is a multiple of 1/8, the matrix is
    exact and its eigenvalues are 1, 1, 1, 2, 2, 5, 5, 5"""
    h2 = np.array([[1.0, 1.0], [1.0, -1.0]])
    H = np.kron(np.kron(h2, h2), h2)
    lam = np.array([1.0, 1, 1, 2, 2, 5, 5, 5])
    A = (H * lam) @ H.T / 8
    assert np.array_equal(A * 8, np.round(A * 8)) and np.array_equal(A, A.T)
    return A, lam


def sparse40():
    rng = np.random.default_rng(40)
    A = np.tril(rng.standard_normal((40, 40)))
    A[np.tril(rng.random((40, 40)) < 1 / 3, -1)] = 0.0
    return A + np.tril(A, -1).T


def column_tails40():
    """a tridiagonal matrix of order 40 whose entries below the sub-diagonal are 1e-9 .. 1e-13 of it, a third of them zero: every
    column meets the decision that symmetric() got wrong"""
    rng = np.random.default_rng(41)
    low = np.tril(rng.standard_normal((40, 40)) * 10.0 ** -rng.integers(9, 14, (40, 40)), -2)
    low[rng.random((40, 40)) < 1 / 3] = 0.0
    return dense_tridiagonal(rng.standard_normal(40), 1.0 + rng.random(39)) + low + low.T


def symmetric_families():
    out = {f"three_t={t:g}": three_by_three(t) for t in (1e-3, 1e-7, 1e-8, 1e-9, 1e-12)}
    out.update({"t_plus_e8": rr.t_plus_e(8), "t_plus_e64": rr.t_plus_e(64), "arrowhead9": arrowhead(), "repeated8": repeated_exactly()[0],
                "sparse40": sparse40(), "column_tails40": column_tails40()})
    out.update({f"decades16_d{d}": with_spectrum(np.logspace(0, -16, d), 50 + d) for d in (8, 16, 64)})
    return out


def hermitian_corner(t=1e-9):
    A = three_by_three(0.0).astype(np.complex128)
    A[2, 0], A[0, 2] = -1j * t, 1j * t
    return A


def degenerate_levels():
    """D = diag(1 x 4, 2 x 3, 5 x 3) / 4 between two Householder reflectors I - v v^H / 4 with eight entries of modulus 1 each:
    every entry is a Gaussian integer over 1024, so the matrix is exact and the three levels are exactly degenerate"""
    lam = np.array([1.0] * 4 + [2.0] * 3 + [5.0] * 3) / 4
    v1 = np.array([1, 1j, -1, -1j, 1, 1j, 1, -1j, 0, 0])
    v2 = np.array([0, 0, 1, 1, 1j, -1, -1j, 1j, 1, -1])
    A = np.diag(lam).astype(np.complex128)
    for v in (v1, v2):
        P = np.eye(10) - np.outer(v, v.conj()) / 4
        A = P @ A @ P
    assert np.array_equal(A * 1024, np.round(A * 1024)) and np.array_equal(A, A.conj().T)
    return A, lam


def hermitian_families():
    return {"corner_1e-9i": hermitian_corner(), "identity6": np.eye(6, dtype=np.complex128), "degenerate_4_3_3": degenerate_levels()[0],
            "t_plus_e8_z": rr.t_plus_e(8, True), "t_plus_e64_z": rr.t_plus_e(64, True)}


def frank(n=12):
    i, j = np.indices((n, n))
    return np.where(j >= i - 1, n - np.maximum(i, j), 0).astype(np.float64)


def companion12():
    """of prod (x - i), i = 1 .. 12, upper Hessenberg: the coefficients are integers below 2^53"""
    c = np.poly(np.arange(1.0, 13.0))
    assert np.array_equal(c, np.round(c)) and np.abs(c).max() < 2.0 ** 53
    C = np.diag(np.ones(11), -1)
    C[0, :] = -c[1:]
    return C


def rotation_blocks():
    """four 2 x 2 rotations on the diagonal (complex pairs on the unit circle), coupled above the blocks"""
    rng = np.random.default_rng(8)
    A = np.triu(0.5 * rng.standard_normal((8, 8)), 2)
    for b, th in enumerate((0.3, 1.1, 1.1, 2.9)):
        c, s = np.cos(th), np.sin(th)
        A[2 * b:2 * b + 2, 2 * b:2 * b + 2] = [[c, -s], [s, c]]
    return A


def random_hessenberg(n, seed, complex_entries=False):
    rng = np.random.default_rng(seed)
    H = rng.standard_normal((n, n)) + (1j * rng.standard_normal((n, n)) if complex_entries else 0.0)
    return np.triu(H, -1)


# (matrix, the scale its values are compared at, compare hessenberg_real_values with hessenberg as multisets)
def hessenberg_families():
    H30 = random_hessenberg(30, 30)
    return {"defective_bidiagonal10": (np.eye(10) + np.diag(np.ones(9), -1), 1.0, False), "frank12": (frank(), 1.0, True),
            "companion12": (companion12(), 1.0, True), "rotation_blocks8": (rotation_blocks(), 1.0, True),
            "random30_x1e150": (H30 * 1e150, 1e150, True), "random30_x1e-150": (H30 * 1e-150, 1e-150, True)}


def general_families():
    rng = np.random.default_rng(31)
    G = rng.standard_normal((30, 30)) + 1j * rng.standard_normal((30, 30))
    D = 10.0 ** -np.arange(30)
    return {"random30": G, "random30_x1e150": G * 1e150, "graded_dgd30": D[:, None] * G * D[None, :]}


# ---------------------------------------------------------------------------------------------------------------------------
# tridiagonal
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", sorted(tridiagonal_families()))
def test_tridiagonal(built, family):
    _, solver = built
    d, e = tridiagonal_families()[family]
    vals, vecs = solver.tridiagonal_eigen(d, e)
    holds("tridiagonal", family, dense_tridiagonal(d, e), vals, vecs, True, product=tridiagonal_product(d, e))
    assert np.all(np.diff(vals) >= 0)
    alone, _ = solver.tridiagonal_eigen(d, e, vectors=False)
    assert alone.tobytes() == vals.tobytes()  # the vectors do not steer the iteration
    if family == "zeros5":
        assert not vals.any() and np.array_equal(vecs, np.eye(5))
    if family == "clement50":  # the spectrum is -49, -47, .., 49
        assert np.abs(vals - np.arange(-49.0, 50.0, 2.0)).max() <= 50 * EPS * float(norm1(dense_tridiagonal(d, e)))


# ---------------------------------------------------------------------------------------------------------------------------
# symmetric
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", sorted(symmetric_families()))
def test_symmetric(built, family):
    _, solver = built
    A = symmetric_families()[family]
    vals, vecs = solver.symmetric_eigen(A)
    holds("symmetric", family, A, vals, vecs, True, lapack=eigvalsh(A))
    assert np.all(np.diff(vals) >= 0)
    if family == "repeated8":
        assert np.abs(vals - repeated_exactly()[1]).max() <= 8 * EPS * float(norm1(A))


# ---------------------------------------------------------------------------------------------------------------------------
# hermitian (through the program)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", sorted(hermitian_families()))
def test_hermitian(program, family):
    A = hermitian_families()[family]
    ok, vals, X, _ = program("hermitian", A)
    assert ok, "hermitian returned false: it kept fewer than n vectors, or the iteration did not converge"
    holds("hermitian", family, A, vals, X, True, lapack=eigvalsh(A))
    assert np.all(np.diff(vals) >= 0)
    ok, alone, none, _ = program("hermitian_values", A)
    assert ok and none is None and alone.tobytes() == vals.tobytes()
    if family == "degenerate_4_3_3":
        assert np.abs(vals - degenerate_levels()[1]).max() <= 10 * EPS * float(norm1(A))
    if family == "identity6":
        assert np.array_equal(vals, np.ones(6))


# ---------------------------------------------------------------------------------------------------------------------------
# hessenberg and hessenberg_real_values
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", sorted(hessenberg_families()))
def test_hessenberg_and_real_values(built, family):
    _, solver = built
    H, scale, compare = hessenberg_families()[family]
    vals, vecs = solver.hessenberg_eigen(H)
    holds("hessenberg", family, H, vals, vecs, False)
    assert np.abs(np.linalg.norm(vecs, axis=0) - 1.0).max() <= H.shape[0] * EPS
    trace_holds("hessenberg", family, H, vals)
    alone, _ = solver.hessenberg_eigen(H, vectors=False)
    assert alone.tobytes() == vals.tobytes()
    real = solver.hessenberg_values_real(H)
    trace_holds("hessenberg_real_values", family, H, real)
    pairs = real[real.imag != 0]
    assert pairs.size % 2 == 0 and np.all(pairs[0::2].imag > 0) and np.array_equal(pairs[1::2], pairs[0::2].conj())
    if compare:
        same_multiset(real / scale, vals / scale, 1e-6, f"hessenberg_real_values {family} against hessenberg")
    if family == "rotation_blocks8":  # block triangular: the spectrum is the blocks', exp(+-i theta)
        want = [np.exp(s * 1j * th) for th in (0.3, 1.1, 1.1, 2.9) for s in (1, -1)]
        same_multiset(real, want, 1e-6, "hessenberg_real_values rotation_blocks8 against exp(+-i theta)")


# ---------------------------------------------------------------------------------------------------------------------------
# general (through the program)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", sorted(general_families()))
def test_general(program, family):
    A = general_families()[family]
    ok, vals, X, _ = program("general", A)
    assert ok
    holds("general", family, A, vals, X, False)
    assert np.abs(np.linalg.norm(X, axis=0) - 1.0).max() <= A.shape[0] * EPS
    trace_holds("general", family, A, vals)
    ok, alone, none, _ = program("general_values", A)
    assert ok and none is None and alone.tobytes() == vals.tobytes()


def test_general_passes_a_hessenberg_matrix_through(program):
    """no reflector is applied to a matrix that is already Hessenberg: the bytes of hessenberg()"""
    for H in (random_hessenberg(12, 32, True), frank().astype(np.complex128), random_hessenberg(12, 33, True) * 2.0 ** 600):
        one, two = program("general", H), program("hessenberg", H)
        assert one[3] == two[3] and one[0]
        holds("general", "already_hessenberg", H, one[1], one[2], False)


# ---------------------------------------------------------------------------------------------------------------------------
# scale: A * 2^+-600.  Either the criterion holds, or the routine returns false.
# ---------------------------------------------------------------------------------------------------------------------------
SCALES = [("2^600", 2.0 ** 600), ("2^-600", 2.0 ** -600)]


def _wrapped(capi, call):
    """(True, result) or (False, None) when the routine returned false (the wrapper raises)"""
    try:
        return True, call()
    except capi.EigenexError:
        return False, None


@pytest.mark.parametrize("label,scale", SCALES)
def test_scale_tridiagonal(built, label, scale):
    capi, solver = built
    d, e = wilkinson21()
    ok, r = _wrapped(capi, lambda: solver.tridiagonal_eigen(d * scale, e * scale))
    print(f"SCALE tridiagonal {label} ok={ok}")
    if ok:
        holds("tridiagonal", "wilkinson21_x" + label, dense_tridiagonal(d, e) * scale, r[0], r[1], True)


@pytest.mark.parametrize("label,scale", SCALES)
def test_scale_symmetric(built, label, scale):
    capi, solver = built
    A = sparse40()[:12, :12]
    ok, r = _wrapped(capi, lambda: solver.symmetric_eigen(A * scale))
    print(f"SCALE symmetric {label} ok={ok}")
    if ok:
        holds("symmetric", "sparse12_x" + label, A * scale, r[0], r[1], True, lapack=eigvalsh(A, scale))


@pytest.mark.parametrize("label,scale", SCALES)
def test_scale_hermitian(program, label, scale):
    A = rr.t_plus_e(8, True) + 0.25j * (np.tril(np.ones((8, 8)), -1) - np.triu(np.ones((8, 8)), 1))
    ok, vals, X, _ = program("hermitian", A * scale)
    print(f"SCALE hermitian {label} ok={ok}")
    if ok:
        holds("hermitian", "t_plus_e8_z_x" + label, A * scale, vals, X, True, lapack=eigvalsh(A, scale))


@pytest.mark.parametrize("label,scale", SCALES)
def test_scale_hessenberg_and_real_values(built, label, scale):
    capi, solver = built
    H = random_hessenberg(12, 34)
    ok, r = _wrapped(capi, lambda: solver.hessenberg_eigen(H * scale))
    print(f"SCALE hessenberg {label} ok={ok}")
    if ok:
        holds("hessenberg", "random12_x" + label, H * scale, r[0], r[1], False)
        trace_holds("hessenberg", "random12_x" + label, H * scale, r[0])
    ok, real = _wrapped(capi, lambda: solver.hessenberg_values_real(H * scale))
    print(f"SCALE hessenberg_real_values {label} ok={ok}")
    if ok:  # against the values of the matrix at its own scale, which the criterion holds above (test_hessenberg_..: random30)
        trace_holds("hessenberg_real_values", "random12_x" + label, H * scale, real)
        at_one, vecs = solver.hessenberg_eigen(H)
        holds("hessenberg", "random12", H, at_one, vecs, False)
        same_multiset(real / scale, at_one, 1e-6, f"hessenberg_real_values x {label} against hessenberg at scale 1")


@pytest.mark.parametrize("label,scale", SCALES)
def test_scale_general(program, label, scale):
    A = general_families()["random30"][:12, :12]
    ok, vals, X, _ = program("general", A * scale)
    print(f"SCALE general {label} ok={ok}")
    if ok:
        holds("general", "random12_x" + label, A * scale, vals, X, False)
        trace_holds("general", "random12_x" + label, A * scale, vals)


# ---------------------------------------------------------------------------------------------------------------------------
# entries that are not finite: false, and an end
# ---------------------------------------------------------------------------------------------------------------------------
CHILD = r"""
import sys
import numpy as np
from cmpt_eigenex_amd import capi, solver
rng = np.random.default_rng(9)
for bad in (float("nan"), float("inf")):
    d, e = rng.standard_normal(8), rng.standard_normal(7)
    S = rng.standard_normal((8, 8)); S = S + S.T
    H = np.triu(rng.standard_normal((8, 8)), -1)
    calls = []
    for at in (0, 5):  # an entry of the diagonal alone deflates at once: no sweep ever looks at it
        dd, ee = d.copy(), e.copy()
        dd[at] = bad
        calls.append(("tridiagonal_diag", lambda dd=dd: solver.tridiagonal_eigen(dd, e)))
        calls.append(("tridiagonal_diag_alone", lambda dd=dd: solver.tridiagonal_eigen(dd, np.zeros(7))))
        ee[at] = bad
        calls.append(("tridiagonal_sub", lambda ee=ee: solver.tridiagonal_eigen(d, ee, vectors=False)))
    Sb = S.copy(); Sb[6, 2] = Sb[2, 6] = bad
    calls.append(("symmetric", lambda: solver.symmetric_eigen(Sb)))
    Sd = np.diag(d); Sd[3, 3] = bad
    calls.append(("symmetric_diagonal", lambda: solver.symmetric_eigen(Sd)))
    for r, c in ((3, 5), (4, 3), (7, 7)):
        Hb = H.copy(); Hb[r, c] = bad
        calls.append(("hessenberg", lambda Hb=Hb: solver.hessenberg_eigen(Hb)))
        calls.append(("hessenberg_values", lambda Hb=Hb: solver.hessenberg_eigen(Hb, vectors=False)))
        calls.append(("hessenberg_real_values", lambda Hb=Hb: solver.hessenberg_values_real(Hb)))
    for name, call in calls:
        try:
            call()
            print(name, bad, "true")
        except capi.EigenexError:
            print(name, bad, "false")
        sys.stdout.flush()
print("done")
"""


def test_non_finite_entries_through_the_wrappers(built):
    """in a child process with a time limit: a routine that span on a NaN would otherwise take the test run with it"""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=15)
    lines = r.stdout.decode().splitlines()
    assert r.returncode == 0 and lines and lines[-1] == "done", (lines[-3:], r.stderr.decode()[-2000:])
    assert len(lines) == 2 * (6 + 2 + 9) + 1
    assert [ln for ln in lines[:-1] if not ln.endswith(" false")] == []


def test_non_finite_entries_through_the_program(program):
    rng = np.random.default_rng(10)
    G = rng.standard_normal((8, 8)) + 1j * rng.standard_normal((8, 8))
    A = G + G.conj().T
    for bad in (float("nan"), float("inf"), complex(0.0, float("nan")), complex(0.0, float("-inf"))):
        for r, c in ((5, 1), (4, 4) if isinstance(bad, float) else (6, 0)):
            Ab = A.copy()
            Ab[r, c] = bad  # the lower triangle: hermitian() does not look at the upper one
            for mode in ("hermitian", "hermitian_values"):
                assert not program(mode, Ab)[0], (mode, bad, r, c)
            Gb = G.copy()
            Gb[r, c] = bad
            for mode in ("general", "general_values"):
                assert not program(mode, Gb)[0], (mode, bad, r, c)
    Hb = np.triu(G, -1)
    Hb[2, 6] = float("nan")
    assert not program("general", Hb)[0] and not program("hessenberg", Hb)[0]


# ---------------------------------------------------------------------------------------------------------------------------
# the criterion rejects a wrong answer
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_criterion_rejects_a_perturbed_answer():
    """numpy's own eigenpairs pass; one eigenvalue moved by 1e-10 ||A||_1, or one vector entry by 1e-9, does not"""
    A = sparse40()[:12, :12]
    vals, X = np.linalg.eigh(A)
    holds("numpy.eigh", "sparse12", A, vals, X, True, lapack=eigvalsh(A))
    faults = []
    for k in (0, 5, 11):
        moved = vals.copy()
        moved[k] += 1e-10 * float(norm1(A))
        faults.append((f"value {k}", moved, X))
        bent = X.copy()
        bent[(3 * k) % 12, k] += 1e-9
        faults.append((f"vector {k}", vals, bent))
    for what, v, V in faults:
        rf, of = fractions(A, v, V, True)
        print(f"REJECT {what}: residual {rf:.3g}, orthogonality {of:.3g}")
        with pytest.raises(AssertionError):
            holds("numpy.eigh", "sparse12 with a wrong " + what, A, v, V, True)
        if what.startswith("value"):
            assert rf > 1.0
            with pytest.raises(AssertionError):
                holds("numpy.eigh", "sparse12 with a wrong " + what, A, v, X, True, lapack=eigvalsh(A))
        else:
            assert rf > 1.0 and of > 1.0
    G = general_families()["random30"][:12, :12]
    w, V = np.linalg.eig(G)
    holds("numpy.eig", "random12", G, w, V, False)
    moved = w.copy()
    moved[4] += 1e-10 * float(norm1(G))
    bent = V.copy()
    bent[7, 4] += 1e-9
    for v, Z in ((moved, V), (w, bent)):
        with pytest.raises(AssertionError):
            holds("numpy.eig", "random12 with a fault", G, v, Z, False)
    with pytest.raises(AssertionError):
        trace_holds("numpy.eig", "random12 with a wrong value", G, w + np.where(np.arange(12) == 4, 1e-10 * float(norm1(G)), 0.0))
    nan = vals.copy()
    nan[2] = np.nan
    with pytest.raises(AssertionError):
        holds("numpy.eigh", "sparse12 with a NaN", A, nan, X, True)


# ---------------------------------------------------------------------------------------------------------------------------
# the program under AddressSanitizer + UBSan
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_program_under_sanitizers(program):
    """the same stand-alone program built with -fsanitize=address,undefined, on one matrix of every family that goes through it
    and on every routine of the header it reaches: the flags and the values of the plain build, and nothing on stderr"""
    exe = _compile(program.tmp, "small_eigen_hard_cases_sanitize", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    cases = [("hermitian", A) for A in hermitian_families().values()] + [("general", A) for A in general_families().values()]
    cases += [("hermitian_values", rr.t_plus_e(8, True)), ("general_values", general_families()["random30"]), ("hessenberg", frank().astype(np.complex128)),
              ("general", frank().astype(np.complex128)), ("hermitian", rr.t_plus_e(8, True) * 2.0 ** -600), ("general", general_families()["random30"] * 2.0 ** 600),
              ("hermitian", np.zeros((0, 0))), ("general", np.zeros((0, 0))), ("hermitian", np.ones((1, 1))), ("general", np.ones((1, 1))),
              ("general", np.zeros((5, 5)))]
    bad = general_families()["random30"][:6, :6].copy()
    bad[4, 1] = np.nan
    cases += [("hermitian", bad), ("general", bad)]
    for mode, A in cases:
        plain, checked = program(mode, A), program(mode, A, exe=exe)
        assert plain[0] == checked[0], mode
        if plain[0]:
            n = A.shape[0]
            assert np.abs(plain[1] - checked[1]).max(initial=0.0) <= n * EPS * float(norm1(A)), mode
