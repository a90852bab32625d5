"""The matrix-free spin-1/2 operators for complex states (eigenex_spin_upload_z, eigenex_spin_sector_upload_z; kernels.hip:
k_spin_spmv<..., SpinZ>, k_spin_measure<..., SpinZ>) on the device.

An application to x = a + ib is held against two references: the existing real kernel applied to a and to b (np.array_equal:
each part is the real kernel's sum, only the sign of a zero may differ and only with a shift), and the complex plain-CSR upload
(val + 0j) of eigenex_spin_csr's / eigenex_spin_sector_csr's rows.  The dot conj(x) . y is within n eps sum |x||y| of the long
double sum.  Shapes (L, n_up): (4,2); (6,0), the diagonal alone; (10,5), one ragged tile; (11,5), two tiles, with the 64-bond
model; (31,2), (32,2), (32,31), bits 30 and 31; (20,10) with one operator workgroup per CU (722 tiles: the tile loop goes round);
the full space of 2, 9 and 12 sites with a transverse field.  Then 20 complex Lanczos steps against the complex-CSR-backed state,
the measurement of complex states, the Chebyshev filter and moments (supported: the streaming form is correct for a complex
state; held against the complex CSR upload), and the refusals."""
import ctypes as C
import os
import sys
from math import comb

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spin_evolution_reference as er  # noqa: E402
import spin_measure_reference as mr  # noqa: E402
import spin_reference as sr  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
LD = np.longdouble
SECTOR_SHAPES = [(4, 2), (6, 0), (10, 5), (11, 5), (31, 2), (32, 2), (32, 31), (20, 10)]
FULL_SHAPES = [2, 9, 12]


@pytest.fixture(scope="module")
def mods():
    from cmpt_eigenex_amd import capi, solver

    assert capi.device_count() >= 1
    return capi, solver


def _models(L, n_up):
    """name -> (n_sites, n_up, bonds, hz, hx); n_up = None: the full space, every model with a transverse field"""
    if n_up is None:
        full = sr.models(L)
        return {name: (L, None) + tuple(full[name][1:]) for name in ("fields", "random40_fields")}
    if L == 20:
        rng = np.random.RandomState(20)
        return {"periodic_fields": (L, n_up, sr.chain(L, 1.0, 0.7, periodic=True) + [(3, 12, 0.4, 0.0), (5, 19, 0.0, 0.6), (9, 10, 0.3, -0.8)], rng.standard_normal(L), None)}
    full = sr.models(L)
    m = {name: (L, n_up, full[name][1], full[name][2], None) for name in ("periodic", "fields")}
    m["top_bond"] = (L, n_up, [(0, L - 1, 0.9, -1.3)] + sr.chain(L, 0.5, 1.0)[: max(L - 2, 0)], None, None)
    if (L, n_up) == (11, 5):
        m["b64"] = (L, n_up, sr.random_bonds(L, 64, 64), np.linspace(-1.0, 1.0, L), None)
    return m


CASES = [(L, n_up, name) for (L, n_up) in SECTOR_SHAPES + [(L, None) for L in FULL_SHAPES] for name in _models(L, n_up)]


def _rows(L, n_up):
    return 1 << L if n_up is None else comb(L, n_up)


def _handles(capi, ctx, model, csr=True):
    """(complex matrix-free handle, real matrix-free handle, complex plain-CSR handle or None, n)"""
    L, n_up, bonds, hz, hx = model
    n = _rows(L, n_up)
    if n_up is None:
        Z = capi.Csr.spin_half(ctx, L, bonds, hz, hx, complex_states=True)
        R = capi.Csr.spin_half(ctx, L, bonds, hz, hx)
        rows = capi.spin_csr(L, bonds, hz, hx) if csr else None
    else:
        Z = capi.Csr.spin_half_sector(ctx, L, n_up, bonds, hz, complex_states=True)
        R = capi.Csr.spin_half_sector(ctx, L, n_up, bonds, hz)
        rows = capi.spin_sector_csr(L, n_up, bonds, hz) if csr else None
    A = None
    if rows is not None:
        rowptr, col, val = rows
        A = capi.Csr.upload(ctx, n, rowptr, col, val.astype(np.complex128), column_blocks=0)
        assert A.layout() == "csr" and A.is_complex
    assert Z.is_complex and Z.layout() == R.layout() == ("matrix_free_spin" if n_up is None else "matrix_free_spin_sector")
    assert Z.encoding() == R.encoding() and Z.info() == R.info() and Z.spin_geometry() == R.spin_geometry()
    return Z, R, A, n


@pytest.mark.parametrize("L,n_up,name", CASES)
def test_apply_equals_the_real_kernel_on_each_part_and_the_complex_csr(mods, L, n_up, name):
    capi, _ = mods
    ctx = capi.Context()
    Z, R, A, n = _handles(capi, ctx, _models(L, n_up)[name])
    bz, br, ba = capi.Basis(ctx, Z, n, 2), capi.Basis(ctx, R, n, 3), capi.Basis(ctx, A, n, 2)
    assert bz.is_complex and not br.is_complex
    if L == 20:
        for b in (bz, br, ba):
            b.tune(2, 1, 0)  # 256 workgroups for 722 tiles
    rs = np.random.RandomState(L + (n_up or 0))
    x = rs.standard_normal(n) + 1j * rs.standard_normal(n)
    bz.upload(capi.VEC_COL(0), x)
    ba.upload(capi.VEC_COL(0), x)
    for shift in (0.0, -0.37):
        parts = []
        for part in (x.real, x.imag):
            br.upload(capi.VEC_COL(0), part)
            br.apply(capi.VEC_COL(0), capi.VEC_V, shift)
            parts.append(br.download(capi.VEC_V))
        want = parts[0] + 1j * parts[1]
        dot = bz.apply(capi.VEC_COL(0), capi.VEC_V, shift, want_dot=True)
        yz = bz.download(capi.VEC_V)
        assert np.array_equal(yz, want), f"{name} ({L},{n_up}) shift={shift}: {np.count_nonzero(yz != want)} rows differ from the real kernel, max {np.abs(yz - want).max():.3e}"
        if shift == 0.0:
            assert yz.tobytes() == want.tobytes()  # without a shift not even the sign of a zero differs
        ba.apply(capi.VEC_COL(0), capi.VEC_V, shift)
        ya = ba.download(capi.VEC_V)
        assert np.array_equal(yz, ya), f"{name} ({L},{n_up}) shift={shift}: {np.count_nonzero(yz != ya)} rows differ from the complex CSR"
        xr, xi, yr, yi = (v.astype(LD) for v in (x.real, x.imag, yz.real, yz.imag))
        ref = complex((xr * yr + xi * yi).sum(), (xr * yi - xi * yr).sum())  # conj(x) . y
        # each part is a sum of 2 n products bounded row by row by |x||y|: (2 n)(eps / 2) sum |x||y| to first order
        bound = n * EPS * float((np.abs(x).astype(LD) * np.abs(yz).astype(LD)).sum())
        print(f"{name} ({L},{n_up}) shift={shift}: dot error {abs(dot - ref):.3e}, bound {bound:.3e}")
        assert abs(dot.real - ref.real) <= bound and abs(dot.imag - ref.imag) <= bound
        bz.apply(capi.VEC_COL(0), capi.VEC_COL(1), shift)  # without the dot: the same y
        assert bz.download(capi.VEC_COL(1)).tobytes() == yz.tobytes()
    assert bz.download(capi.VEC_COL(0)).tobytes() == x.tobytes()  # x is left alone
    for h in (bz, br, ba, Z, R, A, ctx):
        h.close()


def test_complex_shift_is_a_complex_multiply_added_last(mods):
    """eigenex_basis_configure_z on a complex spin state: the Lanczos step's operator application uses (H + shift) with a complex
    shift; one step's alpha is <u|H + shift|u>"""
    capi, _ = mods
    ctx = capi.Context()
    model = _models(10, 5)["fields"]
    Z, R, A, n = _handles(capi, ctx, model)
    x = er.vector_z(10, 5, seed=4)
    out = []
    for op in (Z, A):
        b = capi.Basis(ctx, op, n, 4)
        b.configure(shift=0.3 - 0.2j)
        b.upload(capi.VEC_W, x)
        b.arnoldi_enqueue(3)
        st, H = b.arnoldi_state()
        out.append((H, np.stack([b.download(capi.VEC_COL(c)) for c in range(3)])))
        b.close()
    np.testing.assert_allclose(out[0][0], out[1][0], rtol=0, atol=5e-11)
    np.testing.assert_allclose(out[0][1], out[1][1], rtol=0, atol=5e-11)
    for h in (Z, R, A, ctx):
        h.close()


def test_lanczos_steps_match_the_complex_csr_backed_state(mods):
    capi, _ = mods
    ctx = capi.Context()
    Z, R, A, n = _handles(capi, ctx, (12, 6, sr.chain(12, periodic=True), None, None))
    m = 20
    init = er.vector_z(12, 6, seed=5)
    out = []
    for op in (Z, A):
        b = capi.Basis(ctx, op, n, m + 2)
        b.upload(capi.VEC_W, init)
        b.lanczos_enqueue(m + 1)
        st, alpha, beta = b.lanczos_state()
        assert (st.nvec, st.iterations, st.stopped) == (m + 1, m, 0)
        V = np.stack([b.download(capi.VEC_COL(c)) for c in range(m + 1)])
        out.append((alpha, beta, V))
        b.close()
    print(f"alpha differs by {np.abs(out[0][0] - out[1][0]).max():.3e}, beta by {np.abs(out[0][1] - out[1][1]).max():.3e}")
    np.testing.assert_allclose(out[0][0], out[1][0], rtol=0, atol=5e-11)
    np.testing.assert_allclose(out[0][1], out[1][1], rtol=0, atol=5e-11)
    for _, _, V in out:
        assert np.abs(V.conj() @ V.T - np.eye(m + 1)).max() < 1e-12
    for h in (Z, R, A, ctx):
        h.close()


MEASURE_SHAPES = [(4, 2), (6, 0), (10, 5), (11, 5), (31, 2), (32, 2), (32, 31), (2, None), (9, None), (12, None)]


@pytest.mark.parametrize("L,n_up", MEASURE_SHAPES)
def test_measure_of_complex_states(mods, L, n_up):
    capi, _ = mods
    ctx = capi.Context()
    name = "fields"
    Z, R, _, n = _handles(capi, ctx, _models(L, n_up)[name], csr=False)
    diag_masks, flip_masks = mr.term_lists(L, n_up)
    x = er.vector_z(L, n_up)
    bz, br = capi.Basis(ctx, Z, n, 1), capi.Basis(ctx, R, n, 1)
    bz.upload(capi.VEC_COL(0), x)
    got = bz.spin_measure(capi.VEC_COL(0), diag_masks, flip_masks)
    ref = er.check_z(f"device_z ({L},{n_up})", L, n_up, x, diag_masks, flip_masks, got)
    # against the host definition: the same sums in another grouping, so twice the bound at most
    host = capi.spin_measure_host_z(L, n_up, x, diag_masks, flip_masks)
    for out, hst, mag in ((got[0], host[0], ref[3]), (got[1], host[1], ref[4]), ([got[2]], [host[2]], [ref[5]])):
        for t in range(len(out)):
            assert abs(LD(out[t]) - LD(hst[t])) <= 2 * n * EPS * mag[t]
    again = bz.spin_measure(capi.VEC_COL(0), diag_masks, flip_masks)
    assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes() and again[2] == got[2]
    assert bz.download(capi.VEC_COL(0)).tobytes() == x.tobytes()
    # a real vector stored as complex: the real kernel's numbers
    xr = mr.vector(L, n_up)
    bz.upload(capi.VEC_COL(0), xr.astype(np.complex128))
    br.upload(capi.VEC_COL(0), xr)
    zc, rc = bz.spin_measure(capi.VEC_COL(0), diag_masks, flip_masks), br.spin_measure(capi.VEC_COL(0), diag_masks, flip_masks)
    assert np.array_equal(zc[0], rc[0]) and np.array_equal(zc[1], rc[1]) and zc[2] == rc[2]
    for h in (bz, br, Z, R, ctx):
        h.close()


def _range(val, rowptr):
    return 0.0, 1.01 * float(np.add.reduceat(np.abs(val), rowptr[:-1]).max())


def test_filter_and_moments_equal_the_complex_csr_backed_state(mods):
    """eigenex_basis_set_filter, eigenex_filter_apply, eigenex_kpm_moments and eigenex_kpm_trace_moments are supported on a complex
    spin state: both states take the streaming form of the Chebyshev step (real coefficients on interleaved doubles) behind
    operator outputs that are equal as numbers, so vectors and moments are equal as numbers too"""
    capi, _ = mods
    import filter_reference as fr

    ctx = capi.Context()
    model = (11, 5, sr.random_bonds(11, 40, 77), np.random.RandomState(111).standard_normal(11), None)
    Z, R, A, n = _handles(capi, ctx, model)
    rowptr, col, val = capi.spin_sector_csr(*model[:4])
    c, h = _range(val, rowptr)
    x = er.vector_z(11, 5, seed=9)
    for degree in (1, 2, 7, 24):
        mu = fr.delta_coefficients(-0.3 * h, c, h, degree)
        ys = []
        for op in (Z, A):
            b = capi.Basis(ctx, op, n, 2)
            b.upload(capi.VEC_COL(0), x)
            b.set_filter(mu, c, h)
            b.filter_apply(capi.VEC_COL(0), capi.VEC_COL(1))
            ys.append(b.download(capi.VEC_COL(1)))
            b.close()
        assert np.abs(ys[1]).max() > 0 and np.array_equal(ys[0], ys[1]), degree
    # the filter against numpy: p(H) x with the dense sector matrix, both parts
    import spin_sector_reference as ss

    Hd = ss.dense(*model[:4])
    t_prev, t_cur = x, (Hd @ x - c * x) / h
    acc = mu[0] * x + mu[1] * t_cur
    for k in range(2, 25):
        t_prev, t_cur = t_cur, 2.0 * (Hd @ t_cur - c * t_cur) / h - t_prev
        acc = acc + mu[k] * t_cur
    assert np.abs(ys[0] - acc).max() <= 1e-12 * np.abs(acc).max() * 25
    for nm in (1, 2, 5, 64, 65):
        out = []
        for op in (Z, A):
            b = capi.Basis(ctx, op, n, 2)
            b.upload(capi.VEC_COL(0), x)
            out.append((b.kpm_moments(capi.VEC_COL(0), nm, c, h), b.download(capi.VEC_V), b.kpm_trace_moments(nm, 3, 7, 11, c, h)))
            b.close()
        assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2]), nm
    for hd in (Z, R, A, ctx):
        hd.close()


def _live(capi):
    v = [C.c_int64() for _ in range(3)]
    assert capi.lib().eigenex_debug_allocations(*[C.byref(x) for x in v]) == 0
    return v[0].value, v[1].value


def test_refusals_and_no_allocation_left_behind(mods):
    capi, _ = mods
    L, n_up, bonds, hz = 6, 3, sr.chain(6, 0.8, 1.1), np.random.RandomState(106).standard_normal(6)
    lb = capi.Context(loopback_shards=2)
    before = _live(capi)
    for make in (lambda: capi.Csr.spin_half_sector(lb, L, n_up, bonds, hz, complex_states=True), lambda: capi.Csr.spin_half(lb, L, bonds, hz, complex_states=True)):
        with pytest.raises(capi.EigenexError, match="one shard"):
            make()
    assert _live(capi) == before
    lb.close()
    ctx = capi.Context()
    before = _live(capi)
    Zs = capi.Csr.spin_half_sector(ctx, L, n_up, bonds, hz, complex_states=True)
    Zf = capi.Csr.spin_half(ctx, L, bonds, hz, np.full(L, 0.2), complex_states=True)
    Rs = capi.Csr.spin_half_sector(ctx, L, n_up, bonds, hz)
    assert _live(capi)[0] == before[0] + 3 + 1 + 3  # the same tables as the real handles
    assert Zs.spin_geometry() == Rs.spin_geometry() == (L, n_up) and Zf.spin_geometry()[0] == L
    with pytest.raises(capi.EigenexError, match="scalar type"):
        capi.Basis(ctx, Zs, 20, 4, dtype=np.float64)  # is_complex = 0 on a complex handle
    with pytest.raises(capi.EigenexError, match="a matrix-free spin operator is real"):
        capi.Basis(ctx, Rs, 20, 4, dtype=np.complex128)  # the existing refusal, unchanged
    held = _live(capi)
    bs, bf, br = capi.Basis(ctx, Zs, 20, 3), capi.Basis(ctx, Zf, 64, 3), capi.Basis(ctx, Rs, 20, 3)
    assert bs.is_complex and bf.is_complex
    bs.upload(capi.VEC_COL(0), er.vector_z(6, 3))
    bf.upload(capi.VEC_COL(0), er.vector_z(6, None))
    live = _live(capi)
    for b, mask in ((bs, 0b000111), (bf, 0b000011)):
        with pytest.raises(capi.EigenexError, match="real states only") as e:
            b.spin_rdm(capi.VEC_COL(0), mask)
        assert "eigenex_spin_rdm" in str(e.value)
        for kind in (0, 1, 2):
            with pytest.raises(capi.EigenexError, match="real states only") as e:
                b.spin_site_apply(capi.VEC_COL(0), b, capi.VEC_COL(1), kind, np.ones(L))
            assert "eigenex_spin_site_apply" in str(e.value)
        assert _live(capi) == live
    with pytest.raises(capi.EigenexError, match="real states only"):  # a real source and a complex destination
        br.spin_site_apply(capi.VEC_COL(0), bs, capi.VEC_COL(1), 0, np.ones(L))
    assert _live(capi) == live
    for h in (bs, bf, br):
        h.close()
    assert _live(capi) == held
    for h in (Zs, Zf, Rs):
        h.close()
    assert _live(capi) == before
    ctx.close()
