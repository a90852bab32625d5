"""Momentum sectors of up to 48 sites on the device (eigenex_spin_momentum64_upload(_z); kernels.hip: k_spin_momentum_spmv<E, uint64_t>)
and diagonal correlations in the momentum basis (eigenex_spin_momentum_measure; k_spin_momentum_measure<E, Word>).  The reference for
operator outputs is the plain-CSR upload (column_blocks = 0) of eigenex_spin_momentum64_csr's rows: the kernel adds a row's
products in that stored order, so y is compared with np.array_equal.  Shapes (L, n_up, cell), each at m in {0, 1, N/2}: (34,2,1), 17
rows; (36,3,1), 199; (36,4,1), 1641, past one tile; (40,4,1), 2290; (48,3,1), bits up to 47; (36,4,2), a cell with its own
couplings, a bond across bit 32 and a cell-periodic hz.  (36,5,1) at k = 0, 10472 rows on 41 tiles, and (40,6,1) at k = 0, 95988
rows on 375 tiles, run with one operator workgroup per CU (tune(2, 1, 0)); a device with fewer workgroups than tiles takes the
tile loop round."""
import ctypes as C
import itertools
import json
import os
import subprocess
import sys
from math import comb

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spin_momentum64_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
LD = np.longdouble
SHAPES = [(34, 2, 1), (36, 3, 1), (36, 4, 1), (40, 4, 1), (48, 3, 1), (36, 4, 2)]
LAYOUT = "matrix_free_spin_momentum64"


@pytest.fixture(scope="module")
def mods():
    from cmpt_eigenex_amd import capi, solver

    assert capi.device_count() >= 1
    return capi, solver


def _momenta(L, cell):
    N = L // cell
    return sorted({0, 1, N // 2})


def _model(L, cell):
    """(bonds, hz)"""
    return (ref.xxz_ring(L, 1.0, 0.7), None) if cell == 1 else ref.cell_model(L, cell)


def _is_real(L, cell, m):
    return m == 0 or 2 * m == L // cell


def _vector(n, cplx, seed):
    rs = np.random.RandomState(seed)
    return rs.standard_normal(n) + 1j * rs.standard_normal(n) if cplx else rs.standard_normal(n)


# ---- 1. the operator ----
def _apply_case(capi, ctx, M, A, n, x, big, es_complex):
    """one matrix-free handle against one CSR handle: y bit for bit at two shifts, with and without the dot; the dot; x unchanged"""
    bm, ba = capi.Basis(ctx, M, n, 2), capi.Basis(ctx, A, n, 2)
    assert bm.is_complex == es_complex == ba.is_complex
    if big:
        for b in (bm, ba):
            b.tune(2, 1, 0)  # one operator workgroup per CU
    for b in (bm, ba):
        b.upload(capi.VEC_COL(0), x)
    for shift in (0.0, -0.37):
        dot = bm.apply(capi.VEC_COL(0), capi.VEC_V, shift, want_dot=True)
        ba.apply(capi.VEC_COL(0), capi.VEC_V, shift)
        ym, ya = bm.download(capi.VEC_V), ba.download(capi.VEC_V)
        assert np.array_equal(ym, ya), f"shift={shift}: {np.count_nonzero(ym != ya)} of {n} rows differ, max {np.abs(ym - ya).max():.3e}"
        assert np.abs(ym).max() > 0
        if es_complex:
            xr, xi, yr, yi = (v.astype(LD) for v in (x.real, x.imag, ym.real, ym.imag))
            want = complex((xr * yr + xi * yi).sum(), (xr * yi - xi * yr).sum())  # conj(x) . y
        else:
            want = complex((x.astype(LD) * ym.astype(LD)).sum(), 0.0)
        bound = n * EPS * float((np.abs(x).astype(LD) * np.abs(ym).astype(LD)).sum())
        assert abs(complex(dot).real - want.real) <= bound and abs(complex(dot).imag - want.imag) <= bound
        bm.apply(capi.VEC_COL(0), capi.VEC_COL(1), shift)  # without the dot: the same y
        assert bm.download(capi.VEC_COL(1)).tobytes() == ym.tobytes()
    assert bm.download(capi.VEC_COL(0)).tobytes() == x.tobytes()  # the input column is unchanged
    for b in (bm, ba):
        b.close()


CASES = [(L, n_up, cell, m, False) for (L, n_up, cell) in SHAPES for m in _momenta(L, cell)] + [(36, 5, 1, 0, True), (40, 6, 1, 0, True)]


@pytest.mark.parametrize("L,n_up,cell,m,big", CASES)
def test_apply_equals_the_csr_upload_of_the_rows(mods, L, n_up, cell, m, big):
    capi, _ = mods
    bonds, hz = _model(L, cell)
    n = capi.spin_momentum64_dim(L, n_up, m, cell)
    if big:
        assert n == ref.necklace_count(L, n_up) and n > 40 * 256
    rowptr, col, val = capi.spin_momentum64_csr(L, n_up, m, bonds, hz, cell)
    assert rowptr.size == n + 1 and col.min() >= 0 and col.max() < n
    ctx = capi.Context()
    x = _vector(n, True, L + n_up + 7 * m)
    Z = capi.Csr.spin_half_momentum64(ctx, L, n_up, m, bonds, hz, cell, complex_states=True)
    A = capi.Csr.upload(ctx, n, rowptr, col, val, column_blocks=0)
    assert Z.layout() == LAYOUT and Z.encoding() == "plain" and Z.is_complex and A.layout() == "csr" and A.is_complex
    assert Z.info() == dict(n_global=n, n_local=n, nnz_local=0, n_halo_local=0)
    assert Z.spin_momentum_geometry() == (L, n_up, cell, m)
    _apply_case(capi, ctx, Z, A, n, x, big, True)
    for h in (Z, A):
        h.close()
    if _is_real(L, cell, m):
        assert not val.imag.any() and not np.signbit(val.imag).any()  # every imaginary part is +0
        R = capi.Csr.spin_half_momentum64(ctx, L, n_up, m, bonds, hz, cell)
        Ar = capi.Csr.upload(ctx, n, rowptr, col, np.ascontiguousarray(val.real), column_blocks=0)
        assert R.layout() == LAYOUT and not R.is_complex and Ar.layout() == "csr"
        _apply_case(capi, ctx, R, Ar, n, np.ascontiguousarray(x.real), big, False)
        for h in (R, Ar):
            h.close()
    ctx.close()


@pytest.mark.parametrize("L,n_up,momenta", [(12, 6, (0, 1, 6)), (16, 8, (0, 1, 8)), (24, 12, (0,))])
def test_the_64_bit_handle_equals_the_32_bit_handle(mods, L, n_up, momenta):
    capi, _ = mods
    bonds, hz = _model(L, 1)
    ctx = capi.Context()
    for m in momenta:
        n = capi.spin_momentum_dim(L, n_up, m)
        assert capi.spin_momentum64_dim(L, n_up, m) == n
        for cplx in ((True, False) if _is_real(L, 1, m) else (True,)):
            W = capi.Csr.spin_half_momentum64(ctx, L, n_up, m, bonds, hz, complex_states=cplx)
            N = capi.Csr.spin_half_momentum(ctx, L, n_up, m, bonds, hz, complex_states=cplx)
            assert W.layout() == LAYOUT and N.layout() == "matrix_free_spin_momentum"
            x = _vector(n, cplx, 3 + m)
            ys = []
            for op in (W, N):
                b = capi.Basis(ctx, op, n, 2)
                b.upload(capi.VEC_COL(0), x)
                out = []
                for shift in (0.0, -0.37):
                    dot = b.apply(capi.VEC_COL(0), capi.VEC_V, shift, want_dot=True)
                    out.append((b.download(capi.VEC_V), dot))
                ys.append(out)
                b.close()
            for (yw, dw), (yn, dn) in zip(*ys):
                assert yw.tobytes() == yn.tobytes() and dw == dn and np.abs(yw).max() > 0, (L, m, cplx)
            for h in (W, N):
                h.close()
    ctx.close()


@pytest.mark.parametrize("L,n_up,cell", [(36, 3, 1), (36, 4, 1), (36, 4, 2), (48, 3, 1)])
def test_real_handle_equals_the_complex_handle_part_by_part(mods, L, n_up, cell):
    capi, _ = mods
    bonds, hz = _model(L, cell)
    ctx = capi.Context()
    for m in (0, L // cell // 2):
        n = capi.spin_momentum64_dim(L, n_up, m, cell)
        R = capi.Csr.spin_half_momentum64(ctx, L, n_up, m, bonds, hz, cell)
        Z = capi.Csr.spin_half_momentum64(ctx, L, n_up, m, bonds, hz, cell, complex_states=True)
        br, bz = capi.Basis(ctx, R, n, 2), capi.Basis(ctx, Z, n, 2)
        x = _vector(n, True, 3 + m)
        bz.upload(capi.VEC_COL(0), x)
        for shift in (0.0, -0.37):
            parts = []
            for part in (x.real, x.imag):
                br.upload(capi.VEC_COL(0), np.ascontiguousarray(part))
                br.apply(capi.VEC_COL(0), capi.VEC_V, shift)
                parts.append(br.download(capi.VEC_V))
            bz.apply(capi.VEC_COL(0), capi.VEC_V, shift)
            yz = bz.download(capi.VEC_V)
            assert np.array_equal(yz.real, parts[0]) and np.array_equal(yz.imag, parts[1]), (m, shift)
        for h in (br, bz, R, Z):
            h.close()
    ctx.close()


# ---- 2. Krylov steps, the filter and the moments ----
@pytest.mark.parametrize("m,cplx", [(1, True), (0, False), (18, False)])
def test_lanczos_steps_match_the_csr_backed_state(mods, m, cplx):
    """(36,4), 1641 rows: the tolerances of tests/test_gpu_spin_momentum.py's test of the same name"""
    capi, _ = mods
    L, n_up = 36, 4
    bonds, hz = _model(L, 1)
    n = capi.spin_momentum64_dim(L, n_up, m)
    rowptr, col, val = capi.spin_momentum64_csr(L, n_up, m, bonds, hz)
    ctx = capi.Context()
    M = capi.Csr.spin_half_momentum64(ctx, L, n_up, m, bonds, hz, complex_states=cplx)
    A = capi.Csr.upload(ctx, n, rowptr, col, val if cplx else np.ascontiguousarray(val.real), column_blocks=0)
    steps = 20
    init = _vector(n, cplx, 5)
    out = []
    for op in (M, A):
        b = capi.Basis(ctx, op, n, steps + 2)
        b.upload(capi.VEC_W, init)
        b.lanczos_enqueue(steps + 1)
        st, alpha, beta = b.lanczos_state()
        assert (st.nvec, st.iterations, st.stopped) == (steps + 1, steps, 0)
        V = np.stack([b.download(capi.VEC_COL(c)) for c in range(steps + 1)])
        out.append((alpha, beta, V))
        b.close()
    print(f"m={m}: alpha differs by {np.abs(out[0][0] - out[1][0]).max():.3e}, beta by {np.abs(out[0][1] - out[1][1]).max():.3e}")
    np.testing.assert_allclose(out[0][0], out[1][0], rtol=0, atol=5e-11)
    np.testing.assert_allclose(out[0][1], out[1][1], rtol=0, atol=5e-11)
    for _, _, V in out:
        assert np.abs(V.conj() @ V.T - np.eye(steps + 1)).max() < 1e-12
    for h in (M, A, ctx):
        h.close()


PASS_HANDLES = [("momentum", 36, 4, 1, 0, False), ("momentum", 36, 4, 1, 18, False), ("momentum", 36, 4, 1, 1, True), ("momentum", 36, 4, 2, 17, True)]


@pytest.fixture(scope="module")
def pass_handles(mods):
    """(matrix-free handle, plain-CSR handle, rows, n) of PASS_HANDLES, built once for all their schemes"""
    capi, _ = mods
    ctx = capi.Context()
    cache = {}

    def get(h):
        if h not in cache:
            _, L, n_up, cell, m, cplx = h
            bonds, hz = _model(L, cell)
            rowptr, col, val = capi.spin_momentum64_csr(L, n_up, m, bonds, hz, cell)
            rows = (rowptr, col, np.ascontiguousarray(val if cplx else val.real))
            n = rowptr.size - 1
            M = capi.Csr.spin_half_momentum64(ctx, L, n_up, m, bonds, hz, cell, complex_states=cplx)
            A = capi.Csr.upload(ctx, n, *rows, column_blocks=0)
            assert M.layout() == LAYOUT and A.layout() == "csr" and n > 256
            cache[h] = (M, A, rows, n)
        return ctx, cache[h]

    yield get
    for M, A, _, _ in cache.values():
        M.close()
        A.close()
    ctx.close()


def _pass_cases():
    import test_gpu_spin_krylov_passes as kp

    return [(h, s) for h in PASS_HANDLES for s in kp.SCHEMES if h[5] or not kp.SCHEMES[s][4]]


@pytest.mark.parametrize("h,scheme", _pass_cases(), ids=lambda v: v if isinstance(v, str) else f"{v[1]}_{v[2]}_{v[3]}_m{v[4]}_{'z' if v[5] else 'r'}")
def test_steps_match_the_csr_backed_state_in_every_pass_mode(mods, pass_handles, h, scheme):
    """The schemes of tests/test_gpu_spin_krylov_passes.py (its SCHEMES, _lanczos and _arnoldi: the one-sweep and the two-sweep
    Lanczos step, with and without the stored column, the Arnoldi step with and without kPassSelfNorm, split batches, a complex
    shift) on 64-bit momentum handles past one tile, each against the same calls on the CSR-backed state of the same rows: the
    same (nvec, iterations, stopped) and series lengths, and the coefficients and the columns within the 5e-11 of
    test_lanczos_steps_match_the_csr_backed_state.  The local check of that file is printed, not asserted: its orthogonality bound
    (n + k) eps is a property of the step scheme on the operator, the same for both states, and the single-pass Arnoldi step
    exceeds it on the three-magnon spectrum of (36,4) on the CSR-backed state too."""
    import krylov_local_reference as kl
    import test_gpu_spin_krylov_passes as kp

    capi, _ = mods
    ctx, (M, A, rows, n) = pass_handles(h)
    lanczos, mode_name, batches, shifts, _ = kp.SCHEMES[scheme]
    mode = getattr(capi, mode_name)
    x = _vector(n, h[5], 7)
    run = kp._lanczos if lanczos else kp._arnoldi
    for shift in shifts:
        open_bases = []
        try:
            got, bm = run(capi, ctx, M, n, x, batches, shift, mode, kp.CALLS + 1)
            open_bases.append(bm)
            want, ba = run(capi, ctx, A, n, x, batches, shift, mode, kp.CALLS + 1)
            open_bases.append(ba)
            calls = sum(batches)
            assert got["state"] == want["state"] and got["lengths"] == want["lengths"], (scheme, shift, got["state"], want["state"])
            assert got["state"][0] == calls and got["state"][2] == 0
            for key in ("alpha", "beta") if lanczos else ("H",):
                np.testing.assert_allclose(got[key], want[key], rtol=0, atol=5e-11)
            if not lanczos:
                assert abs(got["residue"] - want["residue"]) <= 5e-11
            np.testing.assert_allclose(got["U"], want["U"], rtol=0, atol=5e-11)
            rep = kl.check_lanczos(rows, shift, got["U"], got["alpha"], got["beta"]) if lanczos else kl.check_arnoldi(rows, shift, got["U"], got["H"], got["residue"], got["w"])
            print(rep.line(f"{h} scheme {scheme} shift={shift}"))
        finally:
            for b in open_bases:  # before the fixture closes the context the states live on
                b.close()


def test_filter_and_moments_equal_the_complex_csr_backed_state(mods):
    capi, _ = mods
    import filter_reference as fr

    L, n_up, m = 36, 4, 1
    bonds, hz = _model(L, 1)
    n = capi.spin_momentum64_dim(L, n_up, m)
    rowptr, col, val = capi.spin_momentum64_csr(L, n_up, m, bonds, hz)
    c, h = 0.0, 1.01 * float(np.add.reduceat(np.abs(val), rowptr[:-1]).max())
    ctx = capi.Context()
    Z = capi.Csr.spin_half_momentum64(ctx, L, n_up, m, bonds, hz, complex_states=True)
    A = capi.Csr.upload(ctx, n, rowptr, col, val, column_blocks=0)
    x = _vector(n, True, 9)
    mu = fr.delta_coefficients(-0.3 * h, c, h, 7)
    out = []
    for op in (Z, A):
        b = capi.Basis(ctx, op, n, 2)
        b.upload(capi.VEC_COL(0), x)
        b.set_filter(mu, c, h)
        b.filter_apply(capi.VEC_COL(0), capi.VEC_COL(1))
        y = b.download(capi.VEC_COL(1))
        b.set_filter(None)
        out.append((y, b.kpm_moments(capi.VEC_COL(0), 16, c, h), b.download(capi.VEC_V)))
        b.close()
    assert np.abs(out[1][0]).max() > 0 and np.array_equal(out[0][0], out[1][0])
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])
    for hd in (Z, A, ctx):
        hd.close()


def test_filter_of_the_real_state_equals_the_csr_backed_state(mods):
    """(36,4) at m = 0: filter_apply bit for bit; the CSR kernel takes the Chebyshev step in its epilogue, the momentum kernel stores
    y and k_cheb_combine follows"""
    capi, _ = mods
    import filter_reference as fr

    L, n_up, m = 36, 4, 0
    bonds, hz = _model(L, 1)
    n = capi.spin_momentum64_dim(L, n_up, m)
    rowptr, col, val = capi.spin_momentum64_csr(L, n_up, m, bonds, hz)
    c, h = 0.0, 1.01 * float(np.add.reduceat(np.abs(val), rowptr[:-1]).max())
    ctx = capi.Context()
    R = capi.Csr.spin_half_momentum64(ctx, L, n_up, m, bonds, hz)
    A = capi.Csr.upload(ctx, n, rowptr, col, np.ascontiguousarray(val.real), column_blocks=0)
    x = _vector(n, False, 19)
    mu = fr.delta_coefficients(-0.3 * h, c, h, 7)
    ys = []
    for op in (R, A):
        b = capi.Basis(ctx, op, n, 2)
        b.upload(capi.VEC_COL(0), x)
        b.set_filter(mu, c, h)
        b.filter_apply(capi.VEC_COL(0), capi.VEC_COL(1))
        ys.append(b.download(capi.VEC_COL(1)))
        b.close()
    assert np.abs(ys[1]).max() > 0 and ys[0].tobytes() == ys[1].tobytes()
    for hd in (R, A, ctx):
        hd.close()


# ---- 3. spectra ----
def _sector_h1(L, n_up, bonds, hz):
    """max column sum of |H| over the Sz sector (H is symmetric), without the matrix: |diagonal| + sum of |jxy| / 2 over the bonds whose
    spins differ, per state"""
    states = np.fromiter((sum(1 << i for i in c) for c in itertools.combinations(range(L), n_up)), np.uint64, comb(L, n_up))
    d, off = np.zeros(states.size), np.zeros(states.size)
    for i, j, jz, jxy in bonds:
        differ = (((states >> np.uint64(i)) ^ (states >> np.uint64(j))) & np.uint64(1)).astype(bool)
        d += np.where(differ, -jz * 0.25, jz * 0.25)
        off += np.where(differ, abs(jxy) * 0.5, 0.0)
    if hz is not None:
        for i in range(L):
            d += np.where(((states >> np.uint64(i)) & np.uint64(1)).astype(bool), hz[i] * 0.5, -hz[i] * 0.5)
    return float((np.abs(d) + off).max())


def _lowest(solver, op, n, H1, dtype, seed=1):
    """tests/test_gpu_spin_momentum.py's _lowest: the lowest Ritz pair after min(120, n) steps and its bound, |beta s| of T plus
    (n + steps) eps |H|_1"""
    m = min(120, n)
    es = solver.LanczosEigenSolver(dtype=dtype)
    es.setDeviceOperator(op).set(minIterations=m, maxIterations=m, maxEigenvalues=1, initialVector=solver.random_vector(seed, n, dtype))
    es.compute()
    r = es.results()
    it = r["iterations"]
    alpha, beta = np.asarray(r["alpha"]).real, np.asarray(r["beta"]).real
    T = np.diag(alpha[:it]) + np.diag(beta[: it - 1], 1) + np.diag(beta[: it - 1], -1)
    _, S = np.linalg.eigh(T)
    bound = abs(beta[it - 1] * S[it - 1, 0]) + (n + it) * EPS * H1
    value, vector = float(np.real(r["eigenvalues"][0])), np.array(r["eigenvectors"][:, 0])
    es.close()
    return value, vector, bound


def _check_levels(mods, L, n_up, momenta):
    capi, solver = mods
    bonds, hz = _model(L, 1)
    H1 = _sector_h1(L, n_up, bonds, hz)
    ctx = capi.Context()
    levels = {}
    for m in momenta:
        real = _is_real(L, 1, m)
        n = capi.spin_momentum64_dim(L, n_up, m)
        M = capi.Csr.spin_half_momentum64(ctx, L, n_up, m, bonds, hz, complex_states=not real)
        value, _, bound = _lowest(solver, M, n, H1, np.float64 if real else np.complex128)
        M.close()
        want = np.linalg.eigvalsh(ref.dense_block(L, n_up, 1, m, bonds, hz))[0]
        print(f"({L},{n_up}) m={m}: {n} rows, E = {value:.13f}, dense {want:.13f}, error {abs(value - want):.3e}, bound {bound:.3e}")
        assert abs(value - want) <= bound
        levels[m] = (value, bound)
    ctx.close()
    return levels


def test_lowest_level_of_every_momentum_at_36_3(mods):
    levels = _check_levels(mods, 36, 3, range(36))
    for m in range(1, 36):
        assert abs(levels[m][0] - levels[36 - m][0]) <= 2 * max(levels[m][1], levels[36 - m][1])  # H(N - m) = conj H(m)


@pytest.mark.parametrize("m", [0, 1, 20])
def test_lowest_level_at_40_4(mods, m):
    _check_levels(mods, 40, 4, [m])


# ---- 4. diagonal correlations ----
def _masks(L):
    """sites, pairs (across bit 32 where the ring has it), a three-site string and the mask of all sites: 40 masks and three sweeps
    beyond 30 sites, 25 masks and two sweeps at 16"""
    top = L - 1
    masks = [1 << i for i in (0, 1, L // 2, top)] + [1 | 1 << r for r in range(1, min(31, L))] + [1 | 1 << top, 1 << (L // 2) | 1 << top]
    return masks + [1 << 2 | 1 << (L // 2 + 1) | 1 << top, (1 << L) - 1, 1 | 1 << 1, 1 << 1 | 1 << 2]


def _check_measure(capi, b, ref_col, L, n_up, m, cell, x, states, label):
    """the device sums against the host definition and against extended precision, within the bound tests/test_gpu_spin_measure.py
    uses: n eps sum |terms| for a sum of n terms in any grouping (twice that between two roundings of it)"""
    masks = _masks(L)
    n = x.size
    diag, norm2 = b.spin_momentum_measure(ref_col, masks)
    host, hnorm = capi.spin_momentum_measure_host(L, n_up, m, x, masks, cell)
    reps = [(int(s), 0) for s in states]
    c = ref.orbit_sums(reps, L, cell, masks).astype(LD)
    w = np.abs(x).astype(LD) ** 2
    want, mag = (c * w).sum(1), (np.abs(c) * w).sum(1)
    worst = 0.0
    for t in range(len(masks)):
        assert abs(LD(diag[t]) - want[t]) <= n * EPS * mag[t], (label, t)
        assert abs(diag[t] - host[t]) <= 2 * n * EPS * float(mag[t]), (label, t)
        worst = max(worst, float(abs(LD(diag[t]) - want[t]) / (n * EPS * mag[t])))
    assert abs(LD(norm2) - w.sum()) <= n * EPS * w.sum() and abs(norm2 - hnorm) <= 2 * n * EPS * hnorm
    print(f"{label}: largest error / bound = {worst:.3e}")
    # identical bytes on a second call; a term does not depend on the masks around it; norm2 alone
    again, n2 = b.spin_momentum_measure(ref_col, masks)
    assert again.tobytes() == diag.tobytes() and n2 == norm2
    for t in (0, 15, 16, len(masks) - 7, len(masks) - 1):
        alone, n2 = b.spin_momentum_measure(ref_col, [masks[t]])
        assert alone[0] == diag[t] and n2 == norm2
        around, _ = b.spin_momentum_measure(ref_col, masks[5:9] + [masks[t]] + masks[20:37])
        assert around[4] == diag[t]
    none, n2 = b.spin_momentum_measure(ref_col, [])
    assert none.size == 0 and n2 == norm2
    assert b.download(ref_col).tobytes() == x.tobytes()


@pytest.mark.parametrize("L,n_up,cell,m,cplx,wide", [(36, 3, 1, 0, False, True), (36, 3, 1, 1, True, True), (36, 4, 2, 9, False, True), (48, 3, 1, 24, True, True),
                                                     (16, 8, 1, 0, False, False), (16, 8, 1, 1, True, False), (16, 8, 1, 8, True, True),
                                                     (36, 5, 1, 0, False, True)])
def test_measure_equals_the_host_definition(mods, L, n_up, cell, m, cplx, wide):
    capi, _ = mods
    bonds, hz = _model(L, cell)
    ctx = capi.Context()
    make = capi.Csr.spin_half_momentum64 if wide else capi.Csr.spin_half_momentum
    M = make(ctx, L, n_up, m, bonds, hz, cell, complex_states=cplx)
    states, _ = capi.spin_momentum64_states(L, n_up, m, cell)
    n = states.size
    b = capi.Basis(ctx, M, n, 2)
    if n > 10000:
        b.tune(2, 1, 0)
    x = _vector(n, cplx, 21 + m)
    b.upload(capi.VEC_COL(1), x)
    _check_measure(capi, b, capi.VEC_COL(1), L, n_up, m, cell, x, states, f"({L},{n_up},{cell}) m={m} {'wide' if wide else 'narrow'}")
    for h in (b, M, ctx):
        h.close()


def test_ground_state_correlations_agree_with_expand_then_spin_measure(mods):
    """(16,8): the Lanczos ground vector of the 32-bit momentum handle at k = 0, measured in the momentum basis, against the same
    vector expanded into the Sz sector and measured by eigenex_spin_measure: <Sz_i Sz_j> = diag{i,j} / (4 norm2) on either side,
    within dim_sector eps"""
    capi, solver = mods
    L, n_up = 16, 8
    bonds = ref.xxz_ring(L, 1.0, 1.0)
    nd = comb(L, n_up)
    ctx = capi.Context()
    M = capi.Csr.spin_half_momentum(ctx, L, n_up, 0, bonds)
    S = capi.Csr.spin_half_sector(ctx, L, n_up, bonds)
    n = capi.spin_momentum_dim(L, n_up, 0)
    _, x0, _ = _lowest(solver, M, n, 1.0, np.float64)
    x0 = np.ascontiguousarray(x0.real)
    bm, bd = capi.Basis(ctx, M, n, 1), capi.Basis(ctx, S, nd, 1)
    bm.upload(capi.VEC_COL(0), x0)
    sites = [1 << i for i in range(L)]
    pairs = [(1 << i) | (1 << j) for i in range(L) for j in range(i + 1, L)]
    diag, norm2 = bm.spin_momentum_measure(capi.VEC_COL(0), sites + pairs)
    bm.spin_momentum_expand(capi.VEC_COL(0), bd, capi.VEC_COL(0))
    sdiag, _, snorm = bd.spin_measure(capi.VEC_COL(0), sites + pairs, [])
    mine, theirs = diag[L:] / (4 * L * norm2), sdiag[L:] / (4 * snorm)
    print(f"<Sz_0 Sz_r> = {mine[: L - 1]}; largest difference {np.abs(mine - theirs).max():.3e}, bound {nd * EPS:.3e}")
    assert np.abs(mine - theirs).max() <= nd * EPS
    assert np.abs(diag[:L] / (2 * L * norm2) - sdiag[:L] / (2 * snorm)).max() <= nd * EPS and np.abs(diag[:L]).max() <= nd * EPS * L * norm2
    assert abs(3 * mine[0] - (-0.4463935225)) < 1e-6  # <S_0 . S_1> = E_0 / L of the 16-site Heisenberg ring
    for h in (bm, bd, M, S, ctx):
        h.close()


def test_a_measurement_between_two_batches_changes_nothing(mods):
    capi, _ = mods
    L, n_up, m = 36, 4, 0
    bonds, hz = _model(L, 1)
    n = capi.spin_momentum64_dim(L, n_up, m)
    ctx = capi.Context()
    M = capi.Csr.spin_half_momentum64(ctx, L, n_up, m, bonds, hz)
    init = _vector(n, False, 5)
    runs = []
    for measured in (False, True):
        b = capi.Basis(ctx, M, n, 10)
        b.upload(capi.VEC_W, init)
        b.lanczos_enqueue(4)
        if measured:
            diag, norm2 = b.spin_momentum_measure(capi.VEC_COL(2), _masks(L))
            assert abs(norm2 - 1.0) <= n * EPS and np.abs(diag).max() > 0
        b.lanczos_enqueue(4)
        st, alpha, beta = b.lanczos_state()
        assert (st.nvec, st.iterations, st.stopped) == (8, 7, 0)
        runs.append((alpha.tobytes(), beta.tobytes(), b"".join(b.download(capi.VEC_COL(c)).tobytes() for c in range(8)), b.download(capi.VEC_W).tobytes()))
        b.close()
    assert runs[0] == runs[1]
    for h in (M, ctx):
        h.close()


# ---- 5. refusals ----
def _live(capi):
    v = [C.c_int64() for _ in range(3)]
    assert capi.lib().eigenex_debug_allocations(*[C.byref(x) for x in v]) == 0
    return v[0].value, v[1].value


def test_refusals_on_the_device(mods):
    capi, _ = mods
    L, n_up = 36, 3
    bonds, hz = _model(L, 1)
    lb = capi.Context(loopback_shards=2)
    before = _live(capi)
    with pytest.raises(capi.EigenexError, match="eigenex_spin_momentum64_upload: .*one shard"):
        capi.Csr.spin_half_momentum64(lb, L, n_up, 0, bonds)
    assert _live(capi) == before
    lb.close()
    ctx = capi.Context()
    before = _live(capi)
    with pytest.raises(capi.EigenexError, match="eigenex_spin_momentum64_upload: real states take a real momentum only"):
        capi.Csr.spin_half_momentum64(ctx, L, n_up, 1, bonds)
    with pytest.raises(capi.EigenexError, match="n_sites must be 2..48"):
        capi.Csr.spin_half_momentum64(ctx, 49, n_up, 0, ref.xxz_ring(49))
    assert _live(capi) == before
    R = capi.Csr.spin_half_momentum64(ctx, L, n_up, 0, bonds)
    Z = capi.Csr.spin_half_momentum64(ctx, L, n_up, 1, bonds, complex_states=True)
    assert _live(capi)[0] == before[0] + 6  # the view, the representatives and the buckets are all an operator holds
    assert R.spin_momentum_geometry() == (L, n_up, 1, 0) and Z.spin_momentum_geometry() == (L, n_up, 1, 1)
    n, nz = capi.spin_momentum64_dim(L, n_up, 0), capi.spin_momentum64_dim(L, n_up, 1)
    br, bz = capi.Basis(ctx, R, n, 2), capi.Basis(ctx, Z, nz, 2)
    br.upload(capi.VEC_COL(0), np.ones(n))
    bz.upload(capi.VEC_COL(0), np.ones(nz, np.complex128))
    S = capi.Csr.spin_half_sector(ctx, 12, 6, ref.xxz_ring(12))
    bs = capi.Basis(ctx, S, comb(12, 6), 1)
    bs.upload(capi.VEC_COL(0), np.ones(comb(12, 6)))
    live = _live(capi)

    def refused(match, call, *args):
        with pytest.raises(capi.EigenexError, match=match) as e:
            call(*args)
        assert str(e.value).startswith("eigenex error -4:")  # EIGENEX_ERR_STATE
        assert _live(capi) == live  # before anything is allocated

    not_spin = "is not a matrix-free spin operator"
    for op in (R, Z):
        refused("eigenex_spin_geometry: the operator " + not_spin, op.spin_geometry)
    for b in (br, bz):
        refused("eigenex_spin_momentum_expand: .*no Sz-sector operator exists beyond 32 sites.*eigenex_spin_momentum_upload", b.spin_momentum_expand,
                capi.VEC_COL(0), bs, capi.VEC_COL(0))
        refused("eigenex_spin_measure: the operator of this state " + not_spin, b.spin_measure, capi.VEC_COL(0), [1], [3])
        refused("eigenex_spin_rdm: the operator of this state " + not_spin, b.spin_rdm, capi.VEC_COL(0), 0x0F)
        refused("eigenex_spin_rdm_z: the operator of this state " + not_spin, b.spin_rdm_z, capi.VEC_COL(0), 0x0F)
        refused("eigenex_spin_site_apply: the operator of a state " + not_spin, b.spin_site_apply, capi.VEC_COL(0), b, capi.VEC_COL(1), 0, np.ones(L))
        refused("eigenex_spin_site_apply_z: the operator of a state " + not_spin, b.spin_site_apply_z, capi.VEC_COL(0), b, capi.VEC_COL(1), 0, np.ones(L))
    refused("eigenex_spin_momentum_measure: the operator of this state is not a momentum-sector operator", bs.spin_momentum_measure, capi.VEC_COL(0), [1])
    for b in (br, bz):
        for masks, what in (([1, 1 << 36], "a mask names a site outside 0..n_sites-1"), ([1, 0], "a mask is zero"), ([1] * 1025, "n_diag must be 0..1024")):
            with pytest.raises(capi.EigenexError, match="eigenex_spin_momentum_measure: " + what) as e:
                b.spin_momentum_measure(capi.VEC_COL(0), masks)
            assert str(e.value).startswith("eigenex error -1:")  # EIGENEX_ERR_ARG
            assert _live(capi) == live
        diag, norm2 = b.spin_momentum_measure(capi.VEC_COL(0), [1 << 35])
        assert norm2 == float(b.n_rows) and _live(capi) == live  # the scratch of a call is gone after it
    for h in (br, bz, bs, R, Z, S):
        h.close()
    assert _live(capi) == before
    ctx.close()


# ---- 6. the C++ interface ----
def test_cpp_program_spin_momentum64(tmp_path):
    """tests/cpp/spin_momentum64_amd.cpp: SpinHalfModel's momentum64 calls, device::spinHalfMomentum64Operator behind
    LanczosEigenSolver<double> and SpinMomentumCorrelationSolver in a C++11 user program, built with -Wall -Wextra: the ground
    state of the 36-site Heisenberg ring with 3 sites up at k = 0 and its correlations"""
    exe = str(tmp_path / "spin_momentum64_amd")
    lib = os.path.join(ROOT, "cmpt-eigenex_amd", "lib")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cmpt-eigenex_amd", "include"),
                           os.path.join(ROOT, "tests", "cpp", "spin_momentum64_amd.cpp"), "-o", exe, "-L", lib, "-leigenex_hip", "-Wl,-rpath," + lib])
    text = subprocess.check_output([exe, "36", "3"]).decode()
    print(text)
    assert "SPIN MOMENTUM64 OK" in text
    o = json.loads(text.splitlines()[0])
    bonds = ref.xxz_ring(36, 1.0, 1.0)
    want = np.linalg.eigvalsh(ref.dense_block(36, 3, 1, 0, bonds))[0]
    assert o["sites"] == 36 and o["n_up"] == 3 and o["dim"] == 199 and o["first_state"] == 7 and o["first_period"] == 36
    assert abs(o["energy"] - want) <= 1e-10 * abs(want) and abs(o["energy_csr"] - want) <= 1e-10 * abs(want)
    assert o["layout"] == 8 and o["expand_refused"] == 1 and o["sites_49_refused"] == 1
    # translation invariance and the sum rules of a state with fixed Sz: <Sz_i> = (2 n_up - L) / (2 L), sum_j <Sz_0 Sz_j> = Sz_total <Sz_0>
    sz = (2 * 3 - 36) / (2.0 * 36)
    assert abs(o["magnetisation_0"] - sz) <= 1e-12 and abs(o["zz_00"] - 0.25) <= 1e-12
    assert abs(o["zz_row_sum"] - (3 - 18) * sz) <= 1e-11 and abs(o["structure_factor_0"] - (3 - 18) ** 2 / 36.0) <= 1e-10
    assert abs(o["string_all_sites"] - (-1.0) ** 33) <= 1e-12
