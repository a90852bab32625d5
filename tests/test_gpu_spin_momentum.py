"""The matrix-free spin-1/2 operator in a momentum sector (eigenex_spin_momentum_upload(_z); kernels.hip: k_spin_momentum_spmv<E>,
k_spin_momentum_expand<E>) on the device.  The reference for operator outputs is the plain-CSR upload (column_blocks = 0) of
eigenex_spin_momentum_csr's rows: the kernel adds a row's products in that stored order, so y is compared with np.array_equal.
Shapes (L, n_up, cell), each at m in {0, 1, N/2 (N even), N - 1}: (4,2,1), rows 2 and 1; (8,4,1); (12,6,1), one ragged tile and
periods 2, 4, 6, 12, also with 24 bonds (three batches of flip terms); (13,6,1), a prime ring; (12,6,2) and (12,4,3), cells with
their own couplings, a bond across the split of the state word and a cell-periodic hz; (16,8,1), four tiles; (31,2,1), (32,2,1),
(32,3,1), (32,31,1), bits 30 and 31 and rotations across the word; (24,12,1) at m = 0 and 5 with one operator workgroup per CU
(441 tiles on 256 workgroups: the tile loop goes round)."""
import ctypes as C
import json
import os
import subprocess
import sys
from math import comb

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spin_momentum_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
LD = np.longdouble
SHAPES = [(4, 2, 1), (8, 4, 1), (12, 6, 1), (13, 6, 1), (12, 6, 2), (12, 4, 3), (16, 8, 1), (31, 2, 1), (32, 2, 1), (32, 3, 1), (32, 31, 1)]


@pytest.fixture(scope="module")
def mods():
    from cmpt_eigenex_amd import capi, solver

    assert capi.device_count() >= 1
    return capi, solver


def _momenta(L, cell):
    N = L // cell
    return sorted({0, 1 % N, N - 1} | ({N // 2} if N % 2 == 0 else set()))


def _model(L, cell, name="ring"):
    """(bonds, hz)"""
    if name == "ring24":
        return ref.xxz_ring(L, 1.0, 0.7, reach=(1, 2)), None
    if cell == 1:
        return ref.xxz_ring(L, 1.0, 0.7), None  # jz != jxy
    return ref.cell_model(L, cell)


CASES = [(L, n_up, cell, m, "ring") for (L, n_up, cell) in SHAPES for m in _momenta(L, cell)]
CASES += [(12, 6, 1, m, "ring24") for m in _momenta(12, 1)]
CASES += [(24, 12, 1, 0, "ring"), (24, 12, 1, 5, "ring")]


def _is_real(L, cell, m):
    return m == 0 or 2 * m == L // cell


def _apply_case(capi, ctx, M, A, n, x, big, es_complex):
    """one matrix-free handle against one CSR handle: y bit for bit at two shifts, with and without the dot; the dot; x unchanged"""
    bm, ba = capi.Basis(ctx, M, n, 2), capi.Basis(ctx, A, n, 2)
    assert bm.is_complex == es_complex == ba.is_complex
    if big:
        for b in (bm, ba):
            b.tune(2, 1, 0)  # 256 workgroups for 441 tiles
    for b in (bm, ba):
        b.upload(capi.VEC_COL(0), x)
    for shift in (0.0, -0.37):
        dot = bm.apply(capi.VEC_COL(0), capi.VEC_V, shift, want_dot=True)
        ba.apply(capi.VEC_COL(0), capi.VEC_V, shift)
        ym, ya = bm.download(capi.VEC_V), ba.download(capi.VEC_V)
        assert np.array_equal(ym, ya), f"shift={shift}: {np.count_nonzero(ym != ya)} of {n} rows differ, max {np.abs(ym - ya).max():.3e}"
        if es_complex:
            xr, xi, yr, yi = (v.astype(LD) for v in (x.real, x.imag, ym.real, ym.imag))
            want = complex((xr * yr + xi * yi).sum(), (xr * yi - xi * yr).sum())  # conj(x) . y
        else:
            want = complex((x.astype(LD) * ym.astype(LD)).sum(), 0.0)
        bound = n * EPS * float((np.abs(x).astype(LD) * np.abs(ym).astype(LD)).sum())
        print(f"shift={shift} complex={es_complex}: dot error {abs(complex(dot) - want):.3e}, bound {bound:.3e}")
        assert abs(complex(dot).real - want.real) <= bound and abs(complex(dot).imag - want.imag) <= bound
        bm.apply(capi.VEC_COL(0), capi.VEC_COL(1), shift)  # without the dot: the same y
        assert bm.download(capi.VEC_COL(1)).tobytes() == ym.tobytes()
    assert bm.download(capi.VEC_COL(0)).tobytes() == x.tobytes()  # the input column is unchanged
    for b in (bm, ba):
        b.close()


@pytest.mark.parametrize("L,n_up,cell,m,name", CASES)
def test_apply_equals_the_csr_upload_of_the_rows(mods, L, n_up, cell, m, name):
    capi, _ = mods
    bonds, hz = _model(L, cell, name)
    n = capi.spin_momentum_dim(L, n_up, m, cell)
    rowptr, col, val = capi.spin_momentum_csr(L, n_up, m, bonds, hz, cell)
    assert rowptr.size == n + 1 and col.min() >= 0 and col.max() < n
    ctx = capi.Context()
    rs = np.random.RandomState(L + n_up + 7 * m)
    x = rs.standard_normal(n) + 1j * rs.standard_normal(n)
    Z = capi.Csr.spin_half_momentum(ctx, L, n_up, m, bonds, hz, cell, complex_states=True)
    A = capi.Csr.upload(ctx, n, rowptr, col, val, column_blocks=0)
    assert Z.layout() == "matrix_free_spin_momentum" and Z.encoding() == "plain" and Z.is_complex and A.layout() == "csr" and A.is_complex
    assert Z.info() == dict(n_global=n, n_local=n, nnz_local=0, n_halo_local=0)
    assert Z.spin_momentum_geometry() == (L, n_up, cell, m)
    _apply_case(capi, ctx, Z, A, n, x, L == 24, True)
    for h in (Z, A):
        h.close()
    if _is_real(L, cell, m):
        assert not val.imag.any() and not np.signbit(val.imag).any()  # every imaginary part is +0
        R = capi.Csr.spin_half_momentum(ctx, L, n_up, m, bonds, hz, cell)
        Ar = capi.Csr.upload(ctx, n, rowptr, col, np.ascontiguousarray(val.real), column_blocks=0)
        assert R.layout() == "matrix_free_spin_momentum" and not R.is_complex and Ar.layout() == "csr"
        _apply_case(capi, ctx, R, Ar, n, np.ascontiguousarray(x.real), L == 24, False)
        for h in (R, Ar):
            h.close()
    ctx.close()


@pytest.mark.parametrize("L,n_up,cell", [(8, 4, 1), (12, 6, 1), (12, 6, 2), (16, 8, 1), (32, 3, 1)])
def test_real_handle_equals_the_complex_handle_part_by_part(mods, L, n_up, cell):
    capi, _ = mods
    bonds, hz = _model(L, cell)
    ctx = capi.Context()
    for m in (0, L // cell // 2):
        n = capi.spin_momentum_dim(L, n_up, m, cell)
        R = capi.Csr.spin_half_momentum(ctx, L, n_up, m, bonds, hz, cell)
        Z = capi.Csr.spin_half_momentum(ctx, L, n_up, m, bonds, hz, cell, complex_states=True)
        br, bz = capi.Basis(ctx, R, n, 2), capi.Basis(ctx, Z, n, 2)
        rs = np.random.RandomState(3 + m)
        x = rs.standard_normal(n) + 1j * rs.standard_normal(n)
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


@pytest.mark.parametrize("m,cplx", [(1, True), (0, False)])
def test_lanczos_steps_match_the_csr_backed_state(mods, m, cplx):
    capi, _ = mods
    L, n_up = 12, 6
    bonds, hz = _model(L, 1)
    n = capi.spin_momentum_dim(L, n_up, m)
    rowptr, col, val = capi.spin_momentum_csr(L, n_up, m, bonds, hz)
    ctx = capi.Context()
    M = capi.Csr.spin_half_momentum(ctx, L, n_up, m, bonds, hz, complex_states=cplx)
    A = capi.Csr.upload(ctx, n, rowptr, col, val if cplx else np.ascontiguousarray(val.real), column_blocks=0)
    steps = 20
    rs = np.random.RandomState(5)
    init = rs.standard_normal(n) + 1j * rs.standard_normal(n) if cplx else rs.standard_normal(n)
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


def _lowest(solver, op, n, H1, dtype, seed=1):
    """the lowest Ritz pair after the solver's fixed work of 120 steps -- a Krylov space has at most n dimensions, so min(120, n) --
    and its bound: the estimate |beta s| of T plus the rounding of one application and one combination, (n + m) eps |H|_1"""
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


@pytest.fixture(scope="module")
def spectra(mods):
    """(L, n_up, cell) -> (levels [(value, bound)] per momentum, the sector operator's (value, bound), the m = 0 ground vector)"""
    capi, solver = mods
    out = {}
    ctx = capi.Context()
    for (L, n_up, cell) in ((12, 6, 1), (12, 6, 2)):
        bonds, hz = _model(L, cell)
        N = L // cell
        H1 = float(np.abs(ref.dense_sector(L, n_up, bonds, hz)).sum(0).max())
        levels, x0 = [], None
        for m in range(N):
            real = _is_real(L, cell, m)
            M = capi.Csr.spin_half_momentum(ctx, L, n_up, m, bonds, hz, cell, complex_states=not real)
            value, vector, bound = _lowest(solver, M, capi.spin_momentum_dim(L, n_up, m, cell), H1, np.float64 if real else np.complex128)
            levels.append((value, bound))
            if m == 0:
                x0 = vector
            M.close()
        S = capi.Csr.spin_half_sector(ctx, L, n_up, bonds, hz)
        sv, _, sb = _lowest(solver, S, comb(L, n_up), H1, np.float64)
        S.close()
        out[(L, n_up, cell)] = (levels, (sv, sb), x0, H1)
    ctx.close()
    return out


@pytest.mark.parametrize("L,n_up,cell", [(12, 6, 1), (12, 6, 2)])
def test_lowest_level_of_every_momentum(spectra, L, n_up, cell):
    bonds, hz = _model(L, cell)
    N = L // cell
    levels, (sector_value, sector_bound), _, _ = spectra[(L, n_up, cell)]
    for m in range(N):
        want = np.linalg.eigvalsh(ref.dense_block(L, n_up, cell, m, bonds, hz))[0]
        value, bound = levels[m]
        print(f"({L},{n_up},{cell}) m={m}: E = {value:.13f}, dense {want:.13f}, error {abs(value - want):.3e}, bound {bound:.3e}")
        assert abs(value - want) <= bound
    for m in range(1, N):
        assert abs(levels[m][0] - levels[N - m][0]) <= 2 * max(levels[m][1], levels[N - m][1])  # H(N - m) = conj H(m)
    best = min(range(N), key=lambda m: levels[m][0])
    print(f"ground momentum {best}: {levels[best][0]:.13f}; sector operator {sector_value:.13f}")
    assert abs(levels[best][0] - sector_value) <= levels[best][1] + sector_bound


EXPAND_SHAPES = [(4, 2, 1), (12, 6, 1), (12, 6, 2), (12, 4, 3), (13, 6, 1), (16, 8, 1), (31, 2, 1), (32, 3, 1), (32, 31, 1)]


@pytest.mark.parametrize("L,n_up,cell", EXPAND_SHAPES)
def test_expand_equals_the_host_definition(mods, L, n_up, cell):
    capi, _ = mods
    bonds, hz = _model(L, cell)
    nd = comb(L, n_up)
    ctx = capi.Context()
    S = {False: capi.Csr.spin_half_sector(ctx, L, n_up, bonds, hz), True: capi.Csr.spin_half_sector(ctx, L, n_up, bonds, hz, complex_states=True)}
    for m in _momenta(L, cell):
        n = capi.spin_momentum_dim(L, n_up, m, cell)
        rs = np.random.RandomState(11 + m)
        for cplx in ((True, False) if _is_real(L, cell, m) else (True,)):
            x = rs.standard_normal(n) + 1j * rs.standard_normal(n) if cplx else rs.standard_normal(n)
            M = capi.Csr.spin_half_momentum(ctx, L, n_up, m, bonds, hz, cell, complex_states=cplx)
            bm, bd = capi.Basis(ctx, M, n, 1), capi.Basis(ctx, S[cplx], nd, 2)
            bm.upload(capi.VEC_COL(0), x)
            norm2 = bm.spin_momentum_expand(capi.VEC_COL(0), bd, capi.VEC_COL(1))
            y = bd.download(capi.VEC_COL(1))
            want = capi.spin_momentum_expand_host(L, n_up, m, x, cell)
            assert y.tobytes() == want.tobytes(), (m, cplx, np.count_nonzero(y != want))
            host = float((np.abs(want).astype(LD) ** 2).sum())
            assert abs(norm2 - host) <= nd * EPS * host
            assert abs(host - float((np.abs(x).astype(LD) ** 2).sum())) <= 8 * EPS * host  # expand preserves the norm: four roundings per entry
            again = bm.spin_momentum_expand(capi.VEC_COL(0), bd, capi.VEC_COL(1))
            assert again == norm2 and bd.download(capi.VEC_COL(1)).tobytes() == y.tobytes()  # two calls, identical bytes
            assert bm.download(capi.VEC_COL(0)).tobytes() == x.tobytes()
            for h in (bm, bd, M):
                h.close()
    for h in (*S.values(), ctx):
        h.close()


def test_expanded_ground_vector_in_the_sector(mods, spectra):
    """the m = 0 ground vector of (12,6,1), expanded, is an eigenvector of the sector operator to the bound of the spectrum test, and
    its correlations are translation invariant: the expanded entries of one orbit are the same bits, so sums over translated terms
    differ by the order of summation alone, dim eps norm2"""
    capi, _ = mods
    L, n_up, cell = 12, 6, 1
    bonds, hz = _model(L, cell)
    levels, _, x0, H1 = spectra[(L, n_up, cell)]
    nd = comb(L, n_up)
    ctx = capi.Context()
    M = capi.Csr.spin_half_momentum(ctx, L, n_up, 0, bonds, hz, cell)
    S = capi.Csr.spin_half_sector(ctx, L, n_up, bonds, hz)
    bm, bd = capi.Basis(ctx, M, x0.size, 1), capi.Basis(ctx, S, nd, 2)
    bm.upload(capi.VEC_COL(0), np.ascontiguousarray(x0.real))
    norm2 = bm.spin_momentum_expand(capi.VEC_COL(0), bd, capi.VEC_COL(0))
    y = bd.download(capi.VEC_COL(0))
    H = ref.dense_sector(L, n_up, bonds, hz)
    residual = np.linalg.norm(H @ y - levels[0][0] * y)
    bound = levels[0][1] + (nd + 120) * EPS * H1
    print(f"expanded ground vector: residual {residual:.3e}, bound {bound:.3e}, norm2 {norm2:.15f}")
    assert residual <= bound
    sites = [1 << i for i in range(L)]
    pairs = [(1 << i) | (1 << ((i + r) % L)) for r in range(1, L // 2 + 1) for i in range(L)]
    diag, flip, n2 = bd.spin_measure(capi.VEC_COL(0), sites + pairs, pairs)
    tol = nd * EPS * n2
    assert np.abs(diag[:L] - diag[0]).max() <= tol  # <Sz_i> does not depend on i
    zz, xy = diag[L:].reshape(L // 2, L), flip.reshape(L // 2, L)
    ss_r = zz / 4 + xy / 2  # <S_i . S_{i+r}> norm2, row r - 1
    print(f"<S_0.S_r> = {ss_r[:, 0] / n2}")
    assert np.abs(ss_r - ss_r[:, :1]).max() <= tol
    for h in (bm, bd, M, S, ctx):
        h.close()


def test_filter_and_moments_equal_the_complex_csr_backed_state(mods):
    capi, _ = mods
    import filter_reference as fr

    L, n_up, m = 12, 6, 1
    bonds, hz = _model(L, 1)
    n = capi.spin_momentum_dim(L, n_up, m)
    rowptr, col, val = capi.spin_momentum_csr(L, n_up, m, bonds, hz)
    c, h = 0.0, 1.01 * float(np.add.reduceat(np.abs(val), rowptr[:-1]).max())
    ctx = capi.Context()
    Z = capi.Csr.spin_half_momentum(ctx, L, n_up, m, bonds, hz, complex_states=True)
    A = capi.Csr.upload(ctx, n, rowptr, col, val, column_blocks=0)
    rs = np.random.RandomState(9)
    x = rs.standard_normal(n) + 1j * rs.standard_normal(n)
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


def _live(capi):
    v = [C.c_int64() for _ in range(3)]
    assert capi.lib().eigenex_debug_allocations(*[C.byref(x) for x in v]) == 0
    return v[0].value, v[1].value


def test_refusals_on_the_device(mods):
    capi, _ = mods
    L, n_up = 8, 4
    bonds, hz = _model(L, 1)
    lb = capi.Context(loopback_shards=2)
    before = _live(capi)
    with pytest.raises(capi.EigenexError, match="one shard"):
        capi.Csr.spin_half_momentum(lb, L, n_up, 0, bonds)
    assert _live(capi) == before
    lb.close()
    ctx = capi.Context()
    before = _live(capi)
    with pytest.raises(capi.EigenexError, match="real momentum"):
        capi.Csr.spin_half_momentum(ctx, L, n_up, 1, bonds)  # a real upload at a complex momentum
    assert _live(capi) == before
    R = capi.Csr.spin_half_momentum(ctx, L, n_up, 0, bonds)
    Z = capi.Csr.spin_half_momentum(ctx, L, n_up, 1, bonds, complex_states=True)
    assert _live(capi)[0] == before[0] + 6  # the view, the representatives and the buckets are all an operator holds
    n, nz = capi.spin_momentum_dim(L, n_up, 0), capi.spin_momentum_dim(L, n_up, 1)
    br, bz = capi.Basis(ctx, R, n, 2), capi.Basis(ctx, Z, nz, 2)
    br.upload(capi.VEC_COL(0), np.ones(n))
    bz.upload(capi.VEC_COL(0), np.ones(nz, np.complex128))
    live = _live(capi)
    for op in (R, Z):
        with pytest.raises(capi.EigenexError, match="eigenex_spin_geometry: the operator is not a matrix-free spin operator"):
            op.spin_geometry()
    not_spin = "is not a matrix-free spin operator"
    for b in (br, bz):
        with pytest.raises(capi.EigenexError, match="eigenex_spin_measure: the operator of this state " + not_spin):
            b.spin_measure(capi.VEC_COL(0), [1], [3])
        with pytest.raises(capi.EigenexError, match="eigenex_spin_rdm: the operator of this state " + not_spin):
            b.spin_rdm(capi.VEC_COL(0), 0x0F)
        with pytest.raises(capi.EigenexError, match="eigenex_spin_rdm_z: the operator of this state " + not_spin):
            b.spin_rdm_z(capi.VEC_COL(0), 0x0F)
        with pytest.raises(capi.EigenexError, match="eigenex_spin_site_apply: the operator of a state " + not_spin):
            b.spin_site_apply(capi.VEC_COL(0), b, capi.VEC_COL(1), 0, np.ones(L))
        with pytest.raises(capi.EigenexError, match="eigenex_spin_site_apply_z: the operator of a state " + not_spin):
            b.spin_site_apply_z(capi.VEC_COL(0), b, capi.VEC_COL(1), 0, np.ones(L))
    S = capi.Csr.spin_half_sector(ctx, L, n_up, bonds)
    Sz = capi.Csr.spin_half_sector(ctx, L, n_up, bonds, complex_states=True)
    S3 = capi.Csr.spin_half_sector(ctx, L, 3, bonds)
    F = capi.Csr.spin_half(ctx, L, bonds)
    bs, bsz, bs3, bf = capi.Basis(ctx, S, comb(L, n_up), 1), capi.Basis(ctx, Sz, comb(L, n_up), 1), capi.Basis(ctx, S3, comb(L, 3), 1), capi.Basis(ctx, F, 1 << L, 1)
    live = _live(capi)
    for src, dst, what in ((br, bs3, "n_sites or n_up"), (br, bsz, "scalar type"), (bz, bs, "scalar type"), (br, bf, "not a sector operator"),
                           (br, br, "not a sector operator"), (bs, bs, "not a momentum-sector operator")):
        with pytest.raises(capi.EigenexError, match=what) as e:
            src.spin_momentum_expand(capi.VEC_COL(0), dst, capi.VEC_COL(0))
        assert str(e.value).startswith("eigenex error -4:")  # EIGENEX_ERR_STATE
        assert _live(capi) == live  # refused before anything is allocated
    assert br.spin_momentum_expand(capi.VEC_COL(0), bs, capi.VEC_COL(0)) > 0
    for h in (br, bz, bs, bsz, bs3, bf, R, Z, S, Sz, S3, F):
        h.close()
    assert _live(capi) == before
    ctx.close()


def test_cpp_program_spin_momentum(tmp_path):
    """tests/cpp/spin_momentum_amd.cpp: SpinHalfModel's momentum calls and device::spinHalfMomentumOperator behind
    LanczosEigenSolver<double> and LanczosEigenSolver<std::complex<double>> in a C++11 user program, built with -Wall -Wextra: the
    lowest level of every momentum of the 12-site Heisenberg ring at n_up = 6"""
    exe = str(tmp_path / "spin_momentum_amd")
    lib = os.path.join(ROOT, "cmpt-eigenex_amd", "lib")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cmpt-eigenex_amd", "include"),
                           os.path.join(ROOT, "tests", "cpp", "spin_momentum_amd.cpp"), "-o", exe, "-L", lib, "-leigenex_hip", "-Wl,-rpath," + lib])
    o = json.loads(subprocess.check_output([exe, "12", "6"]).decode())
    print(o)
    assert o["sites"] == 12 and o["n_up"] == 6 and o["invariant"] == 1 and o["open_chain_invariant"] == 0
    assert sum(o["dims"]) == 924 and o["dims"][0] == len(ref.representatives(12, 6, 1, 0)) and o["first_state"] == 63 and o["first_period"] == 12
    levels = o["levels"]
    assert abs(levels[0] - (-5.387390917445)) < 1e-9 and abs(o["energy_csr_k0"] - levels[0]) <= 1e-10 * abs(levels[0])
    assert min(levels) == levels[0] and o["imag_k0"] == 0.0 and o["real_upload_of_complex_momentum_refused"] == 1
    bonds = ref.xxz_ring(12, 1.0, 1.0)
    for m in range(12):
        want = np.linalg.eigvalsh(ref.dense_block(12, 6, 1, m, bonds))[0]
        assert abs(levels[m] - want) <= 1e-10 * abs(want), m
