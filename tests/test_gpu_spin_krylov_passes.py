"""The two matrix-free spin kernels (kernels.hip: k_spin_spmv<SECTOR, E>, k_spin_momentum_spmv<E>) as the Krylov steps use them,
past one tile.  eigenex_apply, which the other spin suites pin bit for bit, launches them with scale = NULL, u_out = NULL,
pass_flags = 0, shift_im = 0 and a control block that is always zero; a Lanczos or Arnoldi step (library.hip: enq_apply) sets a
scale (the input is normalised inside the kernel), stores the column or not, writes alpha or norm partial sums, sets
kPassSelfNorm in the adaptive Arnoldi step, may carry a complex shift, and reads the live ctrl->stopped.

Every case runs a few step calls on the matrix-free handle and gives the downloaded state to tests/krylov_local_reference.py,
with the CSR rows of the library's host writers (capi.spin_csr, spin_sector_csr, spin_momentum_csr; the host suites hold those
against independent numpy).  The assertion is the local check: every step within (n + k) eps (|H|_1 + |shift|) of the
extended-precision step from the stored columns, max |U^H U - I| <= (n + k) eps.  The same calls on the CSR-backed state
(column_blocks = 0) give the diagnostic print of the trajectory differences and the (nvec, iterations, stopped) to equal.

Schemes, eight calls each (a batch of four or more is captured as a graph):
  a        lanczos_enqueue, default: real handles take the one-sweep step (u_out NULL, scale set), complex ones the two-sweep step
  b_twice  lanczos_enqueue, ORTHO_BATCHED_TWICE   } real handles take the two-sweep step with store_u; no repair and no pending
  b_seq    lanczos_enqueue, ORTHO_SEQUENTIAL      } close show that the one-sweep path was not taken
  c        arnoldi_enqueue, default (no partials)
  d        arnoldi_enqueue, ORTHO_BATCHED_ADAPTIVE (kPassSelfNorm)
  a_split, d_split   a and d as two batches of four
  e_c, e_d complex handles: c and d with the shift 0.3 - 0.2i
a .. d run at shift 0 and -0.37.

Measured ratios error / bound: profiles/spin_krylov_passes.md."""
import os
import sys
from math import comb

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import krylov_local_reference as kl  # noqa: E402
from krylov_pass_runs import CALLS, SCHEMES, SHIFT_Z, SHIFTS  # noqa: E402,F401
from krylov_pass_runs import arnoldi as _arnoldi, columns as _columns, lanczos as _lanczos, state as _state, two_sweeps_forced as _two_sweeps_forced  # noqa: E402
import spin_momentum_reference as mref  # noqa: E402
import spin_reference as sr  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    from cmpt_eigenex_amd import capi, solver

    assert capi.device_count() >= 1
    return capi, solver


# ---- handles ---------------------------------------------------------------------------------------------------------------------
# (kind, L, n_up, cell, m, complex states)
def _momentum_handles(L, n_up, cell):
    N = L // cell
    return [("momentum", L, n_up, cell, 0, False), ("momentum", L, n_up, cell, N // 2, False), ("momentum", L, n_up, cell, 1, True),
            ("momentum", L, n_up, cell, N - 1, True), ("momentum", L, n_up, cell, 0, True)]


HANDLES = [("full", 10, None, None, None, False), ("full", 10, None, None, None, True),
           ("sector", 11, 5, None, None, False), ("sector", 11, 5, None, None, True),
           ("sector", 12, 6, None, None, False), ("sector", 12, 6, None, None, True)]
HANDLES += _momentum_handles(16, 8, 1) + _momentum_handles(12, 6, 2)
BIG_HANDLES = [("momentum", 24, 12, 1, 5, True), ("momentum", 24, 12, 1, 0, False), ("sector", 20, 10, None, None, False), ("full", 17, None, None, None, False)]
TINY_HANDLES = [("momentum", 4, 2, 1, 0, False), ("momentum", 4, 2, 1, 2, False), ("momentum", 4, 2, 1, 1, True),
                ("sector", 6, 0, None, None, False), ("sector", 6, 0, None, None, True)]


def _id(h):
    kind, L, n_up, cell, m, cplx = h
    shape = {"full": f"L{L}", "sector": f"{L}_{n_up}", "momentum": f"{L}_{n_up}_{cell}_m{m}"}[kind]
    return f"{kind}_{shape}_{'z' if cplx else 'r'}"


def _model(h):
    """(bonds, hz, hx) of a handle"""
    kind, L, n_up, cell, m, cplx = h
    if kind == "momentum":
        bonds, hz = (mref.xxz_ring(L, 1.0, 0.7), None) if cell == 1 else mref.cell_model(L, cell)
        return bonds, hz, None
    if L == 17:  # the large shape of tests/test_gpu_spin_operator.py
        rng = np.random.RandomState(17)
        return (sr.chain(L, 1.0, 0.7, periodic=True) + [(3, 12, 0.4, 0.0), (5, 16, 0.0, 0.6)], rng.standard_normal(L),
                np.where(np.arange(L) % 3 == 0, rng.standard_normal(L), 0.0))
    if L == 20:  # the large shape of tests/test_gpu_spin_sector.py
        rng = np.random.RandomState(20)
        return sr.chain(L, 1.0, 0.7, periodic=True) + [(3, 12, 0.4, 0.0), (5, 19, 0.0, 0.6), (9, 10, 0.3, -0.8)], rng.standard_normal(L), None
    _, bonds, hz, hx = sr.models(L)["fields"]
    return bonds, hz, (hx if kind == "full" else None)


_ROWS = {}


def _rows(capi, h):
    """(rowptr, col, val) from the library's host writer, val in the handle's scalar type; computed once per operator"""
    kind, L, n_up, cell, m, cplx = h
    key = h[:5]
    if key not in _ROWS:
        bonds, hz, hx = _model(h)
        if kind == "full":
            _ROWS[key] = capi.spin_csr(L, bonds, hz, hx)
        elif kind == "sector":
            _ROWS[key] = capi.spin_sector_csr(L, n_up, bonds, hz)
        else:
            _ROWS[key] = capi.spin_momentum_csr(L, n_up, m, bonds, hz, cell)
    rowptr, col, val = _ROWS[key]
    if cplx:
        return rowptr, col, np.ascontiguousarray(val, np.complex128)
    assert not np.iscomplexobj(val) or not val.imag.any()
    return rowptr, col, np.ascontiguousarray(val.real)


def _operators(capi, ctx, h):
    """(matrix-free handle, plain-CSR handle, rows, n)"""
    kind, L, n_up, cell, m, cplx = h
    bonds, hz, hx = _model(h)
    rows = _rows(capi, h)
    n = rows[0].size - 1
    if kind == "full":
        M, layout = capi.Csr.spin_half(ctx, L, bonds, hz, hx, complex_states=cplx), "matrix_free_spin"
        assert n == 1 << L
    elif kind == "sector":
        M, layout = capi.Csr.spin_half_sector(ctx, L, n_up, bonds, hz, complex_states=cplx), "matrix_free_spin_sector"
        assert n == comb(L, n_up)
    else:
        M, layout = capi.Csr.spin_half_momentum(ctx, L, n_up, m, bonds, hz, cell, complex_states=cplx), "matrix_free_spin_momentum"
        assert n == capi.spin_momentum_dim(L, n_up, m, cell)
    A = capi.Csr.upload(ctx, n, *rows, column_blocks=0)
    assert M.layout() == layout and A.layout() == "csr" and M.is_complex == cplx == A.is_complex
    return M, A, rows, n


def _start(n, cplx, seed):
    rs = np.random.RandomState(seed)
    return rs.standard_normal(n) + 1j * rs.standard_normal(n) if cplx else rs.standard_normal(n)


# ---- runs --------------------------------------------------------------------------------------------------------------------------
# the schemes and the two runners: tests/krylov_pass_runs.py, shared with tests/test_gpu_layout_krylov_passes.py


def _run_scheme(capi, ctx, h, ops, scheme, batches=None, capacity=CALLS + 1, big=False, seed=7):
    """one scheme on one handle at each of its shifts: the local check asserted on the matrix-free state, the CSR-backed state as the
    diagnostic; returns the worst ratio"""
    M, A, rows, n = ops
    lanczos, mode_name, default_batches, shifts, _ = SCHEMES[scheme]
    batches = batches or default_batches
    mode = getattr(capi, mode_name)
    cplx = h[5]
    x = _start(n, cplx, seed)
    worst = 0.0
    for shift in shifts:
        run = _lanczos if lanczos else _arnoldi
        got, bm = run(capi, ctx, M, n, x, batches, shift, mode, capacity, big)
        ref, ba = run(capi, ctx, A, n, x, batches, shift, mode, capacity, big)
        calls = sum(batches)
        label = f"{_id(h)} n={n} scheme {scheme} shift={shift}"
        assert got["state"] == ref["state"] and got["lengths"] == ref["lengths"], (label, got["state"], ref["state"])
        if lanczos:
            assert got["state"] == (calls, calls - 1, 0) and got["lengths"] == (calls, calls - 1), (label, got["state"], got["lengths"])
            print(f"{label}: against the CSR-backed state alpha differs by {np.abs(got['alpha'] - ref['alpha']).max():.3e}, "
                  f"beta by {np.abs(got['beta'] - ref['beta']).max():.3e}, columns by {np.abs(got['U'] - ref['U']).max():.3e}")
            one_sweep = mode == capi.ORTHO_BATCHED and not cplx and not _two_sweeps_forced()
            if not one_sweep:  # the two-sweep step (on real handles with store_u)
                assert got["repairs"] == 0 and not got["pending"], label
            elif "EIGENEX_EAGER_CLOSE" not in os.environ:
                assert got["pending"], label  # the batch of one-sweep steps has left its newest column for later
            rep = kl.check_lanczos(rows, shift, got["U"], got["alpha"], got["beta"])
        else:
            assert got["state"][0] == calls and got["state"][2] == 0 and got["lengths"][0] == calls, (label, got["state"], got["lengths"])
            print(f"{label}: against the CSR-backed state H differs by {np.abs(got['H'] - ref['H']).max():.3e}, "
                  f"the residue by {abs(got['residue'] - ref['residue']):.3e}, columns by {np.abs(got['U'] - ref['U']).max():.3e}")
            rep = kl.check_arnoldi(rows, shift, got["U"], got["H"], got["residue"], got["w"])
        print(rep.line(label))
        print(f"RATIO {'big-' if big else ''}{h[0]} {'complex' if cplx else 'real'} {scheme} {rep.ratio():.3e} ortho {rep['ortho'] / rep['ortho_bound']:.3e}")
        assert rep.ok(), rep.line(label)
        worst = max(worst, rep.ratio())
        bm.close()
        ba.close()
    return worst


@pytest.fixture(scope="module")
def handles(mods):
    """the operators of HANDLES, built once for all their schemes"""
    capi, _ = mods
    ctx = capi.Context()
    cache = {}

    def get(h):
        if h not in cache:
            cache[h] = _operators(capi, ctx, h)
        return ctx, cache[h]

    yield get
    for M, A, _, _ in cache.values():
        M.close()
        A.close()
    ctx.close()


STEP_CASES = [(h, scheme) for h in HANDLES for scheme in SCHEMES if h[5] or not SCHEMES[scheme][4]]  # a complex shift needs a complex state


@pytest.mark.parametrize("h,scheme", STEP_CASES, ids=[f"{_id(h)}-{scheme}" for h, scheme in STEP_CASES])
def test_steps_pass_the_local_check(mods, handles, h, scheme):
    capi, _ = mods
    ctx, ops = handles(h)
    _run_scheme(capi, ctx, h, ops, scheme)


# ---- the tile loop going round inside a step ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_handles(mods):
    capi, _ = mods
    ctx = capi.Context()
    cache = {}

    def get(h):
        for other in [k for k in cache if k != h]:  # one large operator at a time
            for op in cache.pop(other)[:2]:
                op.close()
        if h not in cache:
            cache[h] = _operators(capi, ctx, h)
        return ctx, cache[h]

    yield get
    for M, A, _, _ in cache.values():
        M.close()
        A.close()
    ctx.close()


@pytest.mark.parametrize("scheme", ["a", "d"])
@pytest.mark.parametrize("h", BIG_HANDLES, ids=_id)
def test_steps_with_the_tile_loop_going_round(mods, big_handles, h, scheme):
    """one operator workgroup per CU (tune(2, 1, 0)) on 441, 722 and 512 tiles: every workgroup takes more than one tile inside a
    step, with the scale, the partial sums and (d) kPassSelfNorm.  Four calls, a basis of six columns."""
    capi, _ = mods
    ctx, ops = big_handles(h)
    _run_scheme(capi, ctx, h, ops, scheme, batches=(4,), capacity=6, big=True)


# ---- breakdown -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", TINY_HANDLES, ids=_id)
def test_breakdown_stops_the_steps(mods, h):
    """sectors of two rows and of one row: the recurrence ends (beta or the residue at rounding level, or a full Krylov space), the
    device sets ctrl->stopped and every later operator launch returns at once.  Six Lanczos calls and six Arnoldi calls (default
    and adaptive) on a basis of eight columns: the state and the lengths of the series equal those of the CSR-backed state, the
    steps before the stop pass the local check, and two further Lanczos calls leave the series and the columns byte for byte."""
    capi, _ = mods
    ctx = capi.Context()
    M, A, rows, n = _operators(capi, ctx, h)
    assert n <= 2
    cplx = h[5]
    x = _start(n, cplx, 11)
    got, bm = _lanczos(capi, ctx, M, n, x, (6,), 0.0, capi.ORTHO_BATCHED, 8)
    ref, ba = _lanczos(capi, ctx, A, n, x, (6,), 0.0, capi.ORTHO_BATCHED, 8)
    print(f"{_id(h)} lanczos: state {got['state']}, lengths {got['lengths']}, alpha {got['alpha']}, beta {got['beta']}")
    assert got["state"] == ref["state"] and got["lengths"] == ref["lengths"], (got["state"], ref["state"], got["lengths"], ref["lengths"])
    assert got["state"][2] == 1 and got["state"][0] == n  # stopped, with as many vectors as the space has dimensions
    rep = kl.check_lanczos(rows, 0.0, got["U"], got["alpha"], got["beta"])
    print(rep.line(f"{_id(h)} lanczos"))
    print(f"RATIO tiny-{h[0]} {'complex' if cplx else 'real'} a {rep.ratio():.3e} ortho {rep['ortho'] / rep['ortho_bound']:.3e}")
    assert rep.ok(), rep.line(_id(h))
    work = [bm.download(capi.VEC_W), bm.download(capi.VEC_V)]
    bm.lanczos_enqueue(2)
    st, alpha, beta = bm.lanczos_state()
    assert _state(st) == got["state"] and (st.nalpha, st.nbeta) == got["lengths"]
    assert alpha.tobytes() == got["alpha"].tobytes() and beta.tobytes() == got["beta"].tobytes()
    assert _columns(capi, bm, st.nvec).tobytes() == got["U"].tobytes()
    assert bm.download(capi.VEC_W).tobytes() == work[0].tobytes() and bm.download(capi.VEC_V).tobytes() == work[1].tobytes()
    bm.close()
    ba.close()
    for mode, name in ((capi.ORTHO_BATCHED, "c"), (capi.ORTHO_BATCHED_ADAPTIVE, "d")):
        got, bm = _arnoldi(capi, ctx, M, n, x, (6,), 0.0, mode, 8)
        ref, ba = _arnoldi(capi, ctx, A, n, x, (6,), 0.0, mode, 8)
        print(f"{_id(h)} arnoldi {name}: state {got['state']}, lengths {got['lengths']}, residue {got['residue']:.3e}")
        assert got["state"] == ref["state"] and got["lengths"] == ref["lengths"], (got["state"], ref["state"], got["lengths"], ref["lengths"])
        assert got["state"][2] == 1 and got["state"][0] == n
        rep = kl.check_arnoldi(rows, 0.0, got["U"], got["H"], got["residue"], got["w"])
        print(rep.line(f"{_id(h)} arnoldi {name}"))
        print(f"RATIO tiny-{h[0]} {'complex' if cplx else 'real'} {name} {rep.ratio():.3e} ortho {rep['ortho'] / rep['ortho_bound']:.3e}")
        assert rep.ok(), rep.line(_id(h))
        bm.close()
        ba.close()
    for hd in (M, A, ctx):
        hd.close()


# ---- filter and moments on momentum handles past one tile -------------------------------------------------------------------------
def _range(rows):
    rowptr, _, val = rows
    return 0.0, 1.01 * float(np.add.reduceat(np.abs(val), rowptr[:-1]).max())


def test_filter_and_moments_equal_the_complex_csr_backed_state_on_four_tiles(mods):
    """(16,8,1) at m = 1, 800 rows: tests/test_gpu_spin_momentum.py's comparison on 75 rows, with four busy workgroups"""
    capi, _ = mods
    import filter_reference as fr

    h = ("momentum", 16, 8, 1, 1, True)
    ctx = capi.Context()
    Z, A, rows, n = _operators(capi, ctx, h)
    assert n > 3 * 256
    c, hw = _range(rows)
    x = _start(n, True, 9)
    mu = fr.delta_coefficients(-0.3 * hw, c, hw, 7)
    out = []
    for op in (Z, A):
        b = capi.Basis(ctx, op, n, 2)
        b.upload(capi.VEC_COL(0), x)
        b.set_filter(mu, c, hw)
        b.filter_apply(capi.VEC_COL(0), capi.VEC_COL(1))
        y = b.download(capi.VEC_COL(1))
        b.set_filter(None)
        out.append((y, b.kpm_moments(capi.VEC_COL(0), 16, c, hw), b.download(capi.VEC_V)))
        b.close()
    assert np.abs(out[1][0]).max() > 0 and np.array_equal(out[0][0], out[1][0])
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])
    for hd in (Z, A, ctx):
        hd.close()


def test_filter_and_moments_of_the_real_momentum_state_on_four_tiles(mods):
    """(16,8,1) at m = 0, 810 rows.  filter_apply bit for bit against the CSR-backed state: the CSR kernel takes the Chebyshev step in
    its epilogue, the momentum kernel stores y and k_cheb_combine follows (the argument of tests/test_gpu_spin_sector.py).
    kpm_moments: the last Chebyshev vector equals the float64 restatement over the CSR rows bit for bit, every moment is within
    the dot-product bound of tests/test_gpu_density.py."""
    capi, _ = mods
    import density_reference as dr
    import filter_reference as fr
    import scipy.sparse as sp
    import test_gpu_density as td

    h = ("momentum", 16, 8, 1, 0, False)
    ctx = capi.Context()
    R, A, rows, n = _operators(capi, ctx, h)
    assert n > 3 * 256
    c, hw = _range(rows)
    x = _start(n, False, 19)
    mu = fr.delta_coefficients(-0.3 * hw, c, hw, 7)
    ys = []
    for op in (R, A):
        b = capi.Basis(ctx, op, n, 2)
        b.upload(capi.VEC_COL(0), x)
        b.set_filter(mu, c, hw)
        b.filter_apply(capi.VEC_COL(0), capi.VEC_COL(1))
        ys.append(b.download(capi.VEC_COL(1)))
        b.close()
    assert np.abs(ys[1]).max() > 0 and ys[0].tobytes() == ys[1].tobytes()
    rowptr, col, val = rows
    ts = dr.chebyshev_vectors(dr.device_matmul(sp.csr_matrix((val, col, rowptr), shape=(n, n))), x, c, hw, dr.applications(16))
    b = capi.Basis(ctx, R, n, 2)
    b.upload(capi.VEC_COL(0), x)
    got = b.kpm_moments(capi.VEC_COL(0), 16, c, hw)
    np.testing.assert_array_equal(b.download(capi.VEC_V), ts[dr.applications(16)])
    td._check_moments("spin momentum (16,8,1) m=0", got, "spin", ts, 16)
    for hd in (b, R, A, ctx):
        hd.close()
