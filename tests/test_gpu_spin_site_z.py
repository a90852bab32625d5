"""The site operators of complex states on the device (eigenex_spin_site_apply_z, kernels.hip: k_spin_site_apply<SECTOR, SpinZ>)
against the host definition (eigenex_spin_site_apply_host_z), bit for bit in y: the kernel performs the definition's operations
in the definition's order.  norm2 is a sum of non-negative terms in another grouping, so it stays within rows * 2^-52 relative
of the host's, and is the same bits from call to call.  Shapes, those of tests/test_gpu_spin_site.py: the smallest sector; odd
and even L; one-row sources and destinations; a partial last tile with three site batches; bit 31; the full space; (20,10), 722
tiles, on the default grid and on one workgroup per CU, where the persistent tile loop goes round.  Coefficients: both signs in
both parts, some zeros, all zero, and real ones -- handed over without imaginary parts and with zeros for them -- whose result is,
part by part, the REAL kernel's on that part of x.  Then Z in place, x only read, a complex Lanczos run that does not notice a call
between its batches, and the refusals with their codes and the allocations they leave behind (none).  NOT part of the reference
project."""
import ctypes as C
import gc
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spin_dynamics_reference as dr  # noqa: E402
import spin_reference as sr  # noqa: E402
import spin_site_z_reference as zr  # noqa: E402

pytestmark = pytest.mark.gpu
ALL = (dr.Z, dr.PLUS, dr.MINUS)
# (L, n_up or None, kinds).  Above L = 20 a sector has n_up <= 1 or >= L - 1: no test allocates more than a few MB.
SHAPES = [(4, 2, ALL), (9, 4, ALL), (11, 5, ALL), (13, 1, ALL), (17, 8, ALL), (20, 10, ALL), (32, 1, (dr.MINUS,)), (32, 31, (dr.PLUS,)), (6, 0, (dr.PLUS,)),
          (6, 6, (dr.MINUS,)), (3, None, ALL), (8, None, ALL), (14, None, ALL)]


@pytest.fixture(scope="module")
def capi():
    from cmpt_eigenex_amd import capi as c

    assert c.device_count() >= 1
    return c


def _operator(capi, ctx, L, n_up, complex_states=True):
    bonds = sr.chain(L, 1.0, 0.7, periodic=True)
    if n_up is None:
        return capi.Csr.spin_half(ctx, L, bonds, complex_states=complex_states)
    return capi.Csr.spin_half_sector(ctx, L, n_up, bonds, complex_states=complex_states)


def _rows(capi, L, n_up):
    return 1 << L if n_up is None else capi.spin_sector_dim(L, n_up)


def counts(capi):
    v = [C.c_int64() for _ in range(3)]
    assert capi.lib().eigenex_debug_allocations(*[C.byref(x) for x in v]) == 0
    return tuple(x.value for x in v)


@pytest.mark.parametrize("L,n_up,kinds", SHAPES)
def test_kernel_equals_the_host_definition(capi, L, n_up, kinds):
    ctx = capi.Context()
    n = _rows(capi, L, n_up)
    src_op, real_op = _operator(capi, ctx, L, n_up), _operator(capi, ctx, L, n_up, complex_states=False)
    src, real_src = capi.Basis(ctx, src_op, n, 2), capi.Basis(ctx, real_op, n, 2)
    x = zr.complex_vector(n, 11 * L + (n_up or 0))
    src.upload(capi.VEC_COL(0), x)
    real_src.upload(capi.VEC_COL(0), np.ascontiguousarray(x.real))
    real_src.upload(capi.VEC_COL(1), np.ascontiguousarray(x.imag))
    for kind in kinds:
        up = dr.dst_up(n_up, kind)
        nd = _rows(capi, L, up)
        dst_op = src_op if up == n_up else _operator(capi, ctx, L, up)
        real_dst_op = real_op if up == n_up else _operator(capi, ctx, L, up, complex_states=False)
        dst, real_dst = capi.Basis(ctx, dst_op, nd, 1), capi.Basis(ctx, real_dst_op, nd, 1)
        grids = ("default", "one per CU") if (L, n_up) == (20, 10) else ("default",)
        for grid in grids:
            if grid == "one per CU":
                dst.tune(2, 1, 0)  # 256 workgroups for 722 tiles (657 and 657 for the flips): the tile loop goes round
                real_dst.tune(2, 1, 0)
            for which in (("zeros",) if n > 20000 else ("both signs", "zeros", "none")):
                c = zr.coefficients(L, which)
                want, want_n2 = capi.spin_site_apply_host_z(L, n_up, kind, c, x)
                dst.upload(capi.VEC_W, np.full(nd, -7.0 - 7.0j))
                n2 = src.spin_site_apply_z(capi.VEC_COL(0), dst, capi.VEC_W, kind, c)
                got = dst.download(capi.VEC_W)
                assert got.shape == want.shape == (nd,)
                assert got.tobytes() == want.tobytes(), (L, n_up, kind, which, grid, int(np.flatnonzero(got != want)[0]))
                print(f"({L},{n_up}) kind {kind} {which} {grid}: norm2 {n2!r}, host {want_n2!r}, difference / bound "
                      f"{abs(n2 - want_n2) / max(nd * dr.EPS * want_n2, 1e-300):.3f}")
                assert abs(n2 - want_n2) <= nd * dr.EPS * want_n2
                if which == "none":
                    assert n2 == 0.0 and not got.any()
                else:
                    assert n2 > 0.0
                again = src.spin_site_apply_z(capi.VEC_COL(0), dst, capi.VEC_W, kind, c)
                assert again == n2 and dst.download(capi.VEC_W).tobytes() == got.tobytes()  # the same bits from call to call
            # real coefficients: the real kernel on the real and on the imaginary part of x
            c = zr.coefficients(L, "zeros").real.copy()
            parts = []
            for col in (0, 1):
                real_src.spin_site_apply(capi.VEC_COL(col), real_dst, capi.VEC_W, kind, c)
                parts.append(real_dst.download(capi.VEC_W))
            for imaginary in (False, True):  # coef_im NULL, then all zero
                dst.upload(capi.VEC_W, np.full(nd, -7.0 - 7.0j))
                n2 = src.spin_site_apply_z(capi.VEC_COL(0), dst, capi.VEC_W, kind, c, imaginary=imaginary)
                got = dst.download(capi.VEC_W)
                assert got.real.tobytes() == parts[0].tobytes() and got.imag.tobytes() == parts[1].tobytes(), (L, n_up, kind, grid, imaginary)
                assert abs(n2 - float(np.vdot(got, got).real)) <= 2 * nd * dr.EPS * n2
        if kind == dr.Z:  # in place equals out of place; any vector reference will do
            c = zr.coefficients(L, "both signs")
            want, _ = capi.spin_site_apply_host_z(L, n_up, kind, c, x)
            src.upload(capi.VEC_COL(1), x)
            n2_in = src.spin_site_apply_z(capi.VEC_COL(1), src, capi.VEC_COL(1), dr.Z, c)
            n2_out = src.spin_site_apply_z(capi.VEC_COL(0), src, capi.VEC_V, dr.Z, c)
            assert src.download(capi.VEC_COL(1)).tobytes() == want.tobytes() and src.download(capi.VEC_V).tobytes() == want.tobytes() and n2_in == n2_out
        for h in (dst, real_dst):
            h.close()
        if dst_op is not src_op:
            dst_op.close()
            real_dst_op.close()
    assert src.download(capi.VEC_COL(0)).tobytes() == x.tobytes()  # x is only read
    for h in (src, real_src, src_op, real_op, ctx):
        h.close()


def test_full_space_flip_between_two_vectors_of_one_state(capi):
    """dst == src in the full space with different vectors is the call as usual"""
    L = 8
    ctx = capi.Context()
    op = _operator(capi, ctx, L, None)
    b = capi.Basis(ctx, op, 1 << L, 2)
    x = zr.complex_vector(1 << L, 2)
    c = zr.coefficients(L, "both signs")
    b.upload(capi.VEC_COL(0), x)
    for kind in (dr.PLUS, dr.MINUS):
        n2 = b.spin_site_apply_z(capi.VEC_COL(0), b, capi.VEC_COL(1), kind, c)
        want, want_n2 = capi.spin_site_apply_host_z(L, None, kind, c, x)
        assert b.download(capi.VEC_COL(1)).tobytes() == want.tobytes() and abs(n2 - want_n2) <= (1 << L) * dr.EPS * want_n2
    for h in (b, op, ctx):
        h.close()


def _lanczos(capi, interrupt):
    L, n_up, steps = 12, 6, 20
    ctx = capi.Context()
    S = capi.Csr.spin_half_sector(ctx, L, n_up, sr.chain(L, periodic=True), complex_states=True)
    D = capi.Csr.spin_half_sector(ctx, L, n_up - 1, sr.chain(L, periodic=True), complex_states=True)
    n = capi.spin_sector_dim(L, n_up)
    b = capi.Basis(ctx, S, n, steps + 2)
    other, down = capi.Basis(ctx, S, n, 1), capi.Basis(ctx, D, capi.spin_sector_dim(L, n_up - 1), 1)
    b.upload(capi.VEC_W, zr.complex_vector(n, 5))
    if interrupt:
        b.lanczos_enqueue(steps // 2)
        c = zr.coefficients(L, "both signs")
        assert b.spin_site_apply_z(capi.VEC_COL(3), down, capi.VEC_W, dr.MINUS, c) > 0.0
        assert b.spin_site_apply_z(capi.VEC_COL(3), other, capi.VEC_W, dr.Z, c) > 0.0
        b.lanczos_enqueue(steps - steps // 2)
    else:
        b.lanczos_enqueue(steps)
    st, alpha, beta = b.lanczos_state()
    out = (alpha.tobytes(), beta.tobytes(), (st.nvec, st.iterations, st.nalpha, st.nbeta, st.stopped, st.calls_true), b.download(capi.VEC_W).tobytes())
    for h in (b, other, down, S, D, ctx):
        h.close()
    return out


def test_a_complex_lanczos_run_does_not_notice_a_call_between_its_batches(capi):
    whole, cut = _lanczos(capi, False), _lanczos(capi, True)
    assert whole[2][0] == 20 and whole == cut


def test_refusals_and_allocations(capi):
    gc.collect()  # handles that earlier tests dropped without closing go now, not in the middle of the counting
    before = counts(capi)[:2]
    ctx, ctx2 = capi.Context(), capi.Context()
    L = 6
    bonds = sr.chain(L)
    Z = dict(complex_states=True)
    S3, S4, S6, F = (capi.Csr.spin_half_sector(ctx, L, 3, bonds, **Z), capi.Csr.spin_half_sector(ctx, L, 4, bonds, **Z),
                     capi.Csr.spin_half_sector(ctx, L, 6, bonds, **Z), capi.Csr.spin_half(ctx, L, bonds, **Z))
    S7 = capi.Csr.spin_half_sector(ctx, 7, 4, sr.chain(7), **Z)
    T4 = capi.Csr.spin_half_sector(ctx2, L, 4, bonds, **Z)
    R3, R4 = capi.Csr.spin_half_sector(ctx, L, 3, bonds), capi.Csr.spin_half_sector(ctx, L, 4, bonds)  # real states
    rowptr, col, val = capi.spin_sector_csr(L, 4, bonds)
    A = capi.Csr.upload(ctx, 15, rowptr, col, val.astype(np.complex128), column_blocks=0)
    b3, b4, b6, bf, b7 = capi.Basis(ctx, S3, 20, 2), capi.Basis(ctx, S4, 15, 2), capi.Basis(ctx, S6, 1, 1), capi.Basis(ctx, F, 64, 2), capi.Basis(ctx, S7, 35, 1)
    t4, ba, r3, r4 = capi.Basis(ctx2, T4, 15, 1), capi.Basis(ctx, A, 15, 1), capi.Basis(ctx, R3, 20, 1), capi.Basis(ctx, R4, 15, 1)
    bh = capi.Basis(ctx, None, 15, 1)
    bh.set_host_operator(lambda v: v)
    x = np.arange(1.0, 21.0) - 1j * np.arange(21.0, 41.0)
    fill = np.full(15, -7.0 + 3.0j)
    b3.upload(capi.VEC_COL(0), x)
    b4.upload(capi.VEC_W, fill)
    ok, inf = np.full(L, 1.0 + 2.0j), np.full(L, 1.0 + 1.0j)
    inf[1] = complex(1.0, np.inf)
    dp = C.POINTER(C.c_double)
    okp = np.ones(32).ctypes.data_as(dp)
    ARG, STATE = -1, -4
    held = counts(capi)[:2]
    cases = [
        ("belong together", ARG, (b3, 0, b3, 1, dr.PLUS, ok)),        # mismatched geometries: PLUS needs (6,4)
        ("belong together", ARG, (b3, 0, b4, capi.VEC_W, dr.Z, ok)),
        ("belong together", ARG, (b3, 0, b4, capi.VEC_W, dr.MINUS, ok)),
        ("belong together", ARG, (b3, 0, b7, capi.VEC_W, dr.PLUS, ok)),  # other sites
        ("belong together", ARG, (b3, 0, bf, 0, dr.PLUS, ok)),         # a sector into the full space
        ("belong together", ARG, (bf, 0, b4, 0, dr.PLUS, ok)),
        ("different contexts", STATE, (b3, 0, t4, capi.VEC_W, dr.PLUS, ok)),
        ("not a matrix-free spin operator", STATE, (b3, 0, ba, capi.VEC_W, dr.PLUS, ok)),  # a CSR-backed state
        ("not a matrix-free spin operator", STATE, (ba, 0, b4, capi.VEC_W, dr.MINUS, ok)),
        ("host callback", STATE, (b3, 0, bh, capi.VEC_W, dr.PLUS, ok)),
        ("complex states only.*eigenex_spin_site_apply\\b", STATE, (r3, 0, r4, capi.VEC_W, dr.PLUS, ok)),   # two real states
        ("complex states only.*eigenex_spin_site_apply\\b", STATE, (r3, 0, b4, capi.VEC_W, dr.PLUS, ok)),   # a real source
        ("complex states only.*eigenex_spin_site_apply\\b", STATE, (b3, 0, r4, capi.VEC_W, dr.PLUS, ok)),   # a real destination
        ("reads what it would write", ARG, (bf, 0, bf, 0, dr.PLUS, ok)),  # y_ref == x_ref for a full-space flip
        ("reads what it would write", ARG, (bf, capi.VEC_W, bf, capi.VEC_W, dr.MINUS, ok)),
        ("destination sector", ARG, (b6, 0, b6, 0, dr.PLUS, ok)),       # S+ of the sector with every site up
        ("kind", ARG, (b3, 0, b4, capi.VEC_W, 3, ok)),
        ("not finite", ARG, (b3, 0, b4, capi.VEC_W, dr.PLUS, inf)),       # in the imaginary part
        ("not finite", ARG, (b3, 0, b4, capi.VEC_W, dr.PLUS, inf.imag.astype(np.complex128))),  # in the real part
        ("bad vector reference", ARG, (b3, 2, b4, capi.VEC_W, dr.PLUS, ok)),
        ("bad vector reference", ARG, (b3, 0, b4, 2, dr.PLUS, ok)),
    ]
    for word, code, (src, xr, dst, yr, kind, coef) in cases:
        with pytest.raises(capi.EigenexError, match=word) as e:
            src.spin_site_apply_z(xr, dst, yr, kind, coef)
        assert f"eigenex error {code}:" in str(e.value), (word, str(e.value))
        assert counts(capi)[:2] == held, word  # no live allocation is left behind, and none went away
    with pytest.raises(capi.EigenexError, match="real states only.*eigenex_spin_site_apply_z"):  # the real call names the complex one
        b3.spin_site_apply(0, b4, capi.VEC_W, dr.PLUS, np.ones(L))
    assert capi.lib().eigenex_spin_site_apply_z(None, 0, b4.h, 0, 1, okp, okp, None) == ARG
    assert capi.lib().eigenex_spin_site_apply_z(b3.h, 0, None, 0, 1, okp, okp, None) == ARG
    assert capi.lib().eigenex_spin_site_apply_z(b3.h, 0, b4.h, capi.VEC_W, 1, None, okp, None) == ARG and "NULL" in capi.lib().eigenex_last_error().decode()
    assert counts(capi)[:2] == held
    assert b4.download(capi.VEC_W).tobytes() == fill.tobytes()  # nothing above wrote anything
    # the call the refusals were variations of; norm2 and coef_im may be NULL; its scratch is gone when it returns
    want, want_n2 = capi.spin_site_apply_host_z(L, 3, dr.PLUS, ok, x)
    assert b3.spin_site_apply_z(0, b4, capi.VEC_W, dr.PLUS, ok) == want_n2 and b4.download(capi.VEC_W).tobytes() == want.tobytes()  # integers: exact
    assert capi.lib().eigenex_spin_site_apply_z(b3.h, 0, b4.h, capi.VEC_W, 1, okp, None, None) == 0
    assert counts(capi)[:2] == held
    for h in (b3, b4, b6, bf, b7, t4, ba, r3, r4, bh, S3, S4, S6, S7, F, T4, R3, R4, A, ctx, ctx2):
        h.close()
    assert counts(capi)[:2] == before  # none after destroy
