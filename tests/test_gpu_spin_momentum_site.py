"""Site operators between momentum sectors on the device (eigenex_spin_momentum_site_apply(_z); kernels.hip:
k_spin_momentum_site_apply<E, Word>).  y is held against the host definition eigenex_spin_momentum_site_apply_host with
np.array_equal -- the kernel walks the same terms in the same order -- and norm2 within n eps norm2 (its partial sums are grouped by
workgroup).  Independent of the definition: the commutator with the Heisenberg Hamiltonian through the existing operator handles,
valid beyond 32 sites, and the static structure factor against eigenex_spin_momentum_measure.  Shapes (L, n_up, cell), each at
every (m, p) with m in {0, 1, N/2} and p in {0, 1, N/2, N - 1}: (8,4,1), periods 1..8 and rows of one sector only; (12,6,1);
(12,5,2); (16,8,1), 810 rows, past one tile; with 64-bit states (36,3,1), (36,4,1), (48,3,1), (36,4,2).  S+ from (36,4,1) to
(36,5,1) at k = 0, 10472 rows on 41 tiles, and S- from (20,10,1) to (20,9,1) run with one operator workgroup per CU (tune(2, 1, 0))."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spin_momentum64_reference as ref64  # noqa: E402
import spin_momentum_site_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
LD, CLD = np.longdouble, np.clongdouble
KINDS = (ref.Z, ref.PLUS, ref.MINUS)
SHAPES = [(8, 4, 1, False), (12, 6, 1, False), (12, 5, 2, False), (16, 8, 1, False), (36, 3, 1, True), (36, 4, 1, True), (48, 3, 1, True), (36, 4, 2, True)]
ARG, STATE = -1, -4


@pytest.fixture(scope="module")
def capi():
    from cmpt_eigenex_amd import capi as c

    assert c.device_count() >= 1
    return c


def _model(L, cell):
    """(bonds, hz)"""
    return (ref64.xxz_ring(L, 1.0, 0.7), None) if cell == 1 else ref64.cell_model(L, cell)


def _is_real(N, m):
    return m == 0 or 2 * m == N


def _momenta(L, cell):
    N = L // cell
    return [(m, p) for m in sorted({0, 1, N // 2}) for p in sorted({0, 1, N // 2, N - 1})]


def _vector(n, cplx, seed):
    rs = np.random.RandomState(seed)
    return rs.standard_normal(n) + 1j * rs.standard_normal(n) if cplx else rs.standard_normal(n)


class Sectors:
    """the operator handles and states of one ring on one context, one per (n_up, momentum, element), made when first asked for"""

    def __init__(self, capi, L, cell, wide, columns=2, tune=False):
        self.capi, self.L, self.cell, self.wide, self.columns, self.tune = capi, L, cell, wide, columns, tune
        self.ctx = capi.Context()
        self.bonds, self.hz = _model(L, cell)
        self.made, self.dims = {}, {}

    def dim(self, n_up, m):
        if not 0 <= n_up <= self.L:
            return 0
        if (n_up, m) not in self.dims:
            try:
                self.dims[n_up, m] = self.capi.spin_momentum64_dim(self.L, n_up, m, self.cell)
            except self.capi.EigenexError:
                self.dims[n_up, m] = 0  # an empty sector
        return self.dims[n_up, m]

    def state(self, n_up, m, cplx):
        key = (n_up, m, cplx)
        if key not in self.made:
            make = self.capi.Csr.spin_half_momentum64 if self.wide else self.capi.Csr.spin_half_momentum
            op = make(self.ctx, self.L, n_up, m, self.bonds, self.hz, self.cell, complex_states=cplx)
            b = self.capi.Basis(self.ctx, op, self.dim(n_up, m), self.columns)
            if self.tune:
                b.tune(2, 1, 0)  # one operator workgroup per CU
            self.made[key] = (op, b)
        return self.made[key][1]

    def close(self):
        for op, b in self.made.values():
            b.close()
            op.close()
        self.ctx.close()


def _check_call(capi, S, n_up, m, kind, cc, p, cplx, seed, y_ref=None):
    """one device call against the host definition; returns the number of rows of the destination, 0 where a sector is missing"""
    L, cell = S.L, S.cell
    up2, m2 = ref.destination(L, n_up, cell, m, kind, p)
    n_src, n_dst = S.dim(n_up, m), S.dim(up2, m2)
    if not (n_src and n_dst):
        return 0
    y_ref = capi.VEC_W if y_ref is None else y_ref
    src, dst = S.state(n_up, m, cplx), S.state(up2, m2, cplx)
    x = _vector(n_src, cplx, seed)
    src.upload(capi.VEC_COL(0), x)
    norm2 = src.spin_momentum_site_apply(capi.VEC_COL(0), dst, y_ref, kind, cc, p)
    y = dst.download(y_ref)
    want, wnorm = capi.spin_momentum_site_apply_host(L, n_up, m, kind, cc, p, x, cell)
    what = (L, n_up, cell, m, p, kind, cplx)
    assert y.dtype == want.dtype and np.array_equal(y, want), (what, int(np.count_nonzero(y != want)), float(np.abs(y - want).max()))
    assert abs(norm2 - wnorm) <= n_dst * EPS * wnorm, what
    assert src.download(capi.VEC_COL(0)).tobytes() == x.tobytes(), what  # x is unchanged
    return n_dst


# ---- 1. the device equals the host ----
@pytest.mark.parametrize("L,n_up,cell,wide", SHAPES)
def test_device_equals_the_host_definition(capi, L, n_up, cell, wide):
    S = Sectors(capi, L, cell, wide)
    N = L // cell
    rs = np.random.RandomState(L + n_up + cell)
    seen = set()
    for m, p in _momenta(L, cell):
        real = _is_real(N, m) and _is_real(N, (m - p) % N)
        for kind in KINDS:
            cz = rs.standard_normal(cell) + 1j * rs.standard_normal(cell)
            if _check_call(capi, S, n_up, m, kind, cz, p, True, 3 * m + p):
                seen.add((kind, "z"))
            if real:  # real coefficients: on two complex states, and the real form on two real states
                cr = rs.standard_normal(cell)
                _check_call(capi, S, n_up, m, kind, cr, p, True, 5 * m + p)
                if _check_call(capi, S, n_up, m, kind, cr, p, False, 7 * m + p):
                    seen.add((kind, "d"))
    assert seen == {(k, e) for k in KINDS for e in "zd"}
    S.close()


@pytest.mark.parametrize("L,n_up,kind,wide,p,cplx", [(36, 4, ref.PLUS, True, 0, False), (36, 4, ref.PLUS, True, 1, True), (20, 10, ref.MINUS, False, 0, False),
                                                     (20, 10, ref.MINUS, False, 1, True), (20, 10, ref.Z, False, 10, False)])
def test_many_tiles_with_one_workgroup_per_cu(capi, L, n_up, kind, wide, p, cplx):
    S = Sectors(capi, L, 1, wide, tune=True)
    n_dst = _check_call(capi, S, n_up, 0, kind, [0.75 - 0.5j] if cplx else [0.75], p, cplx, 11)
    assert n_dst > 8000 and (L != 36 or p != 0 or n_dst == 10472 == ref64.necklace_count(36, 5))
    S.close()


# ---- 2. side effects and repeatability ----
def test_repeatable_in_place_and_any_destination_vector(capi):
    L, n_up, cell, m = 12, 5, 2, 1
    S = Sectors(capi, L, cell, False, columns=3)
    src = S.state(n_up, m, True)
    n = S.dim(n_up, m)
    x = _vector(n, True, 2)
    cc = [0.5 - 0.25j, 1.5 + 0.125j]
    src.upload(capi.VEC_COL(0), x)
    # Z with p = 0 on one state: into another vector, then in place
    n2 = src.spin_momentum_site_apply(capi.VEC_COL(0), src, capi.VEC_COL(1), ref.Z, cc, 0)
    want, wnorm = capi.spin_momentum_site_apply_host(L, n_up, m, ref.Z, cc, 0, x, cell)
    assert np.array_equal(src.download(capi.VEC_COL(1)), want) and n2 > 0 and abs(n2 - wnorm) <= n * EPS * wnorm
    assert src.download(capi.VEC_COL(0)).tobytes() == x.tobytes()
    n2b = src.spin_momentum_site_apply(capi.VEC_COL(0), src, capi.VEC_COL(0), ref.Z, cc, 0)
    assert src.download(capi.VEC_COL(0)).tobytes() == want.tobytes() and n2b == n2
    # a second call gives identical bytes, in the intended vector and in a column
    src.upload(capi.VEC_COL(0), x)
    for kind, p in ((ref.MINUS, 1), (ref.PLUS, 5), (ref.Z, 3)):
        up2, m2 = ref.destination(L, n_up, cell, m, kind, p)
        dst = S.state(up2, m2, True)
        first = src.spin_momentum_site_apply(capi.VEC_COL(0), dst, capi.VEC_W, kind, cc, p)
        y = dst.download(capi.VEC_W)
        again = src.spin_momentum_site_apply(capi.VEC_COL(0), dst, capi.VEC_COL(2), kind, cc, p)
        assert again == first and dst.download(capi.VEC_COL(2)).tobytes() == y.tobytes() and np.abs(y).max() > 0
        assert dst.download(capi.VEC_W).tobytes() == y.tobytes() and src.download(capi.VEC_COL(0)).tobytes() == x.tobytes()
    S.close()


# ---- 3. the commutator with the Heisenberg Hamiltonian ----
def _csr_apply(rowptr, col, val, x):
    """(H x, number of entries of each row, sum of the moduli of each row's products) in longdouble"""
    prod = val.astype(CLD) * np.asarray(x).astype(CLD)[col]
    rows = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
    y, mod = np.zeros(rowptr.size - 1, CLD), np.zeros(rowptr.size - 1, LD)
    np.add.at(y, rows, prod)
    np.add.at(mod, rows, np.abs(prod))
    return y, np.diff(rowptr), mod


@pytest.mark.parametrize("L,n_up,wide", [(16, 8, False), (36, 4, True)])
@pytest.mark.parametrize("m", [0, 1])
def test_total_lowering_operator_commutes_with_the_heisenberg_ring(capi, L, n_up, wide, m):
    """O = sum_i S-_i (p = 0, cc = 1) commutes with H at Jz = Jxy: H_{n_up-1,k} (O x) against O (H_{n_up,k} x), both on the
    device.  Per element at most (T_H + T_O + 8) eps sum|terms|: T_H the entries of the row of H_{n_up-1,k}, T_O the terms of the
    row of O, both the row's own counts from the two-step reference; the sum is that of the moduli of all products of the two-step
    evaluation in longdouble.  Two orders of evaluation are compared and each has its own sum of moduli (H after O, O after H);
    the difference of the two results is bounded by the larger of the two, which is the one taken."""
    cplx = m != 0
    bonds = ref64.xxz_ring(L, 1.0, 1.0)
    ctx = capi.Context()
    make = capi.Csr.spin_half_momentum64 if wide else capi.Csr.spin_half_momentum
    n_src, n_dst = capi.spin_momentum64_dim(L, n_up, m), capi.spin_momentum64_dim(L, n_up - 1, m)
    Hs, Hd = make(ctx, L, n_up, m, bonds, complex_states=cplx), make(ctx, L, n_up - 1, m, bonds, complex_states=cplx)
    bs, bd = capi.Basis(ctx, Hs, n_src, 2), capi.Basis(ctx, Hd, n_dst, 2)
    x = _vector(n_src, cplx, 40 + m)
    bs.upload(capi.VEC_COL(0), x)
    bs.spin_momentum_site_apply(capi.VEC_COL(0), bd, capi.VEC_COL(0), ref.MINUS, [1.0], 0)
    bd.apply(capi.VEC_COL(0), capi.VEC_V)
    h_o_x = bd.download(capi.VEC_V)
    bs.apply(capi.VEC_COL(0), capi.VEC_V)
    bs.spin_momentum_site_apply(capi.VEC_V, bd, capi.VEC_COL(1), ref.MINUS, [1.0], 0)
    o_h_x = bd.download(capi.VEC_COL(1))
    # the two-step reference
    csr_s, csr_d = capi.spin_momentum64_csr(L, n_up, m, bonds), capi.spin_momentum64_csr(L, n_up - 1, m, bonds)
    ox, _, ox_mod = ref.apply(L, n_up, 1, m, ref.MINUS, [1.0], 0, x)
    want_a, th_d, _ = _csr_apply(*csr_d, ox)
    _, _, mod_a = _csr_apply(csr_d[0], csr_d[1], np.abs(csr_d[2]), ox_mod)
    hx, th_s, hx_mod = _csr_apply(*csr_s, x)
    want_b, t_o, _ = ref.apply(L, n_up, 1, m, ref.MINUS, [1.0], 0, hx)
    _, _, mod_b = ref.apply(L, n_up, 1, m, ref.MINUS, [1.0], 0, hx_mod)
    assert np.abs(want_a - want_b).max() <= 1e-15 * float(np.abs(want_a).max())  # the reference commutes
    bound = (th_d + t_o + 8) * EPS * np.maximum(mod_a, mod_b).astype(np.float64)
    err = np.abs(h_o_x - o_h_x)
    print(f"({L},{n_up}) m={m}: largest error / bound = {float((err / bound).max()):.3e}; |H O x| up to {np.abs(h_o_x).max():.3e}")
    assert np.all(err <= bound) and np.abs(h_o_x).max() > 0.1
    assert np.all(np.abs(h_o_x - want_a.astype(np.complex128)) <= bound)
    for h in (bs, bd, Hs, Hd, ctx):
        h.close()


# ---- 4. the sum rule against the diagonal correlations ----
@pytest.mark.parametrize("L,n_up,wide", [(16, 8, False), (36, 4, True)])
def test_static_structure_factor_equals_the_fourier_sum_of_the_correlations(capi, L, n_up, wide):
    """norm2(Sz_q x) / norm2(x) = sum_d e^{2 pi i qIndex d / L} C(d), C(0) = 1/4, C(d) = <sigma_0 sigma_d> / 4 from
    eigenex_spin_momentum_measure, for a random complex x at m = 1.  Bound n eps (W + L / 4): n eps relative on each of the two
    non-negative sums, n eps / 4 on each of the L correlators."""
    m = 1
    S = Sectors(capi, L, 1, wide)
    n = S.dim(n_up, m)
    src = S.state(n_up, m, True)
    x = _vector(n, True, 9)
    src.upload(capi.VEC_COL(0), x)
    diag, x2 = src.spin_momentum_measure(capi.VEC_COL(0), [1 | (1 << d) for d in range(1, L)])
    corr = np.concatenate([[0.25], diag / (4.0 * L * x2)])
    for q in (1, L // 2):
        dst = S.state(n_up, (m - q) % L, True)
        cc = [np.exp(2j * np.pi * q * 0 / L) / np.sqrt(L)]
        y2 = src.spin_momentum_site_apply(capi.VEC_COL(0), dst, capi.VEC_W, ref.Z, cc, q % L)
        W = y2 / x2
        want = np.sum(np.exp(2j * np.pi * q * np.arange(L) / L) * corr)
        print(f"({L},{n_up}) q={q}: S(q) = {W:.15f}, from the correlations {want.real:.15f}, bound {n * EPS * (W + L / 4):.3e}")
        assert abs(W - want) <= n * EPS * (W + L / 4) and W > 1e-3
    S.close()


# ---- 5. what is refused ----
def test_state_errors_and_argument_errors(capi):
    L, n_up = 12, 5
    bonds = ref64.xxz_ring(L, 1.0, 0.7)
    ctx, other = capi.Context(), capi.Context()

    def state(make, up, m, cplx, c=ctx):
        op = make(c, L, up, m, bonds, complex_states=cplx)
        return op, capi.Basis(c, op, capi.spin_momentum64_dim(L, up, m), 2)

    narrow, wide = capi.Csr.spin_half_momentum, capi.Csr.spin_half_momentum64
    held = [state(narrow, 5, 0, False), state(narrow, 4, 0, False), state(narrow, 5, 0, True), state(narrow, 4, 0, True), state(wide, 4, 0, True),
            state(narrow, 4, 0, True, other), state(narrow, 5, 6, True), state(narrow, 6, 0, True)]
    r5, r4, z5, z4, w4, o4, z5pi, z6 = (b for _, b in held)
    sector = capi.Csr.spin_half_sector(ctx, L, 4, bonds, complex_states=True)
    s4 = capi.Basis(ctx, sector, capi.spin_sector_dim(L, 4), 2)
    z5.upload(capi.VEC_COL(0), _vector(z5.n_rows, True, 1))
    r5.upload(capi.VEC_COL(0), _vector(r5.n_rows, False, 1))
    before = z4.download(capi.VEC_W)
    real_call, z_call = "eigenex_spin_momentum_site_apply: ", "eigenex_spin_momentum_site_apply_z: "
    cases = [
        # mixed real and complex states: the message names the other call
        (STATE, z_call + "complex states only.*real states take eigenex_spin_momentum_site_apply", (z5, z4, False), (ref.MINUS, [1.0], 0), r4),
        (STATE, real_call + "real states only.*eigenex_spin_momentum_site_apply_z", (r5, r4, False), (ref.MINUS, [1.0], 0), z4),
        # mixed word widths, a handle that is no momentum handle, two contexts
        (STATE, z_call + "one operator has 32-bit states .* and the other 64-bit states", (z5, w4, True), (ref.MINUS, [1.0], 0), None),
        (STATE, z_call + "the operator of a state is not a momentum-sector operator.*eigenex_spin_site_apply", (z5, s4, True), (ref.MINUS, [1.0], 0), None),
        (STATE, z_call + "the two states live on different contexts", (z5, o4, True), (ref.MINUS, [1.0], 0), None),
        # aliasing: one state serves Z with p = 0 only
        (STATE, z_call + "the destination must be a different state", (z5, z5, True), (ref.MINUS, [1.0], 0), None),
        (STATE, z_call + "the destination must be a different state", (z5, z5, True), (ref.Z, [1.0], 6), None),
        # arguments
        (ARG, z_call + "kind must be EIGENEX_SPIN_SITE_Z, _PLUS or _MINUS", (z5, z4, True), (3, [1.0], 0), None),
        (ARG, z_call + "p must be 0..n_sites/cell - 1", (z5, z4, True), (ref.MINUS, [1.0], 12), None),
        (ARG, z_call + "a coefficient is not finite", (z5, z4, True), (ref.MINUS, [np.nan], 0), None),
        (ARG, z_call + "a coefficient is not finite", (z5, z4, True), (ref.MINUS, [1j * np.inf], 0), None),
        (ARG, z_call + "source and destination do not belong together", (z5, z4, True), (ref.PLUS, [1.0], 0), None),
        (ARG, z_call + "source and destination do not belong together", (z5, z4, True), (ref.MINUS, [1.0], 1), None),
        (ARG, z_call + "source and destination do not belong together", (z5, z5pi, True), (ref.Z, [1.0], 5), None),
    ]
    for code, what, (src, dst, _), (kind, cc, p), swap in cases:
        a, b = (src, dst) if swap is None else (src, swap)
        with pytest.raises(capi.EigenexError, match="eigenex error %d: %s" % (code, what)):
            a.spin_momentum_site_apply(capi.VEC_COL(0), b, capi.VEC_W, kind, cc, p)
    assert z4.download(capi.VEC_W).tobytes() == before.tobytes()  # a refused call writes nothing
    # the destination n_up outside 0..L: S+ of the sector with every site up
    full_op, full = state(narrow, L, 0, True)
    with pytest.raises(capi.EigenexError, match="eigenex error -1: " + z_call + "the destination sector lies outside 0..n_sites"):
        full.spin_momentum_site_apply(capi.VEC_COL(0), z4, capi.VEC_W, ref.PLUS, [1.0], 0)
    # the Sz-sector calls keep refusing momentum handles, and now say where to go
    for call in (z5.spin_site_apply_z, ):
        with pytest.raises(capi.EigenexError, match="eigenex error -4: eigenex_spin_site_apply_z: .*not a matrix-free spin operator.*eigenex_spin_momentum_site_apply"):
            call(capi.VEC_COL(0), z4, capi.VEC_W, ref.MINUS, np.ones(L))
    with pytest.raises(capi.EigenexError, match="eigenex error -4: eigenex_spin_site_apply: .*not a matrix-free spin operator.*eigenex_spin_momentum_site_apply"):
        r5.spin_site_apply(capi.VEC_COL(0), r4, capi.VEC_W, ref.MINUS, np.ones(L))
    # what is allowed next to what was refused: Z at p = pi between two states, and S+ up
    assert z5.spin_momentum_site_apply(capi.VEC_COL(0), z5pi, capi.VEC_W, ref.Z, [1.0], 6) > 0
    assert z5.spin_momentum_site_apply(capi.VEC_COL(0), z6, capi.VEC_W, ref.PLUS, [1.0], 0) > 0
    for b in (s4, full):
        b.close()
    for op, b in held:
        b.close()
        op.close()
    for h in (sector, full_op, ctx, other):
        h.close()


# ---- 6. the solver: S^zz(q, w) of the 12-site Heisenberg ring ----
def _dense_sector(L, n_up, bonds):
    """(states, H) of the Sz sector from the full-space model, dense"""
    states = [s for s in range(1 << L) if bin(s).count("1") == n_up]
    index = {s: r for r, s in enumerate(states)}
    H = np.zeros((len(states), len(states)))
    for r, s in enumerate(states):
        for i, j, jz, jxy in bonds:
            if ((s >> i) ^ (s >> j)) & 1:
                H[r, r] -= jz / 4
                H[index[s ^ (1 << i) ^ (1 << j)], r] += jxy / 2
            else:
                H[r, r] += jz / 4
    return np.array(states), H


@pytest.fixture(scope="module")
def ring12(capi):
    """the ground state of the 12-site Heisenberg ring: from LanczosEigenSolver at k = 0 in the momentum basis, and the dense
    diagonalisation of the whole (12, 6) sector, computed once and left unchanged"""
    from cmpt_eigenex_amd import solver

    L, n_up = 12, 6
    bonds = ref64.xxz_ring(L, 1.0, 1.0)
    ctx = capi.Context()
    op = capi.Csr.spin_half_momentum(ctx, L, n_up, 0, bonds)
    n = capi.spin_momentum_dim(L, n_up, 0)
    es = solver.LanczosEigenSolver(dtype=np.float64)
    es.setDeviceOperator(op).set(minIterations=n, maxIterations=n, maxEigenvalues=1, initialVector=solver.random_vector(1, n, np.float64))
    es.compute()
    r = es.results()
    e0, x = float(np.real(r["eigenvalues"][0])), np.ascontiguousarray(np.real(r["eigenvectors"][:, 0]))
    es.close()
    states, H = _dense_sector(L, n_up, bonds)
    levels, vectors = np.linalg.eigh(H)
    assert abs(levels[0] - e0) <= 1e-12 * abs(e0) and levels[1] - levels[0] > 0.1
    return dict(L=L, n_up=n_up, bonds=bonds, ctx=ctx, op=op, n=n, e0=e0, x=x, states=states, levels=levels, vectors=vectors, solver=solver)


@pytest.mark.parametrize("q_index", [6, 1])
def test_structure_factor_of_the_heisenberg_ring_against_dense_diagonalisation(capi, ring12, q_index):
    """computeStructureFactorZ(qIndex) at qIndex = 6 (q = pi: the real path) and 1 (the complex path): the first four moments within
    1e-10 and spectrum(w, 0.1) within 1e-9 of its maximum of the dense diagonalisation of the full (12, 6) sector, the bounds
    tests/test_gpu_spin_dynamics.py asserts; totalWeight() against the static structure factor from the diagonal correlations
    (what SpinMomentumCorrelationSolver evaluates) within the sum-rule bound n eps (W + L / 4)."""
    g = ring12
    L, solver = g["L"], g["solver"]
    ds = solver.SpinMomentumDynamicsSolver()
    ds.setModel(g["ctx"], L, g["bonds"], g["n_up"], 0).setState(g["x"]).setStateEnergy(g["e0"]).setLanczosSteps(100)
    ds.computeStructureFactorZ(q_index)
    r = ds.results()
    assert r["info_name"] == "Success", ds.log()
    assert r["complexRun"] == (0 if q_index == 6 else 1) and r["destinationMomentum"] == (L - q_index) % L and r["destinationSitesUp"] == g["n_up"]
    assert r["destinationDimension"] == capi.spin_momentum_dim(L, g["n_up"], (L - q_index) % L) and 0 < r["npoles"] <= r["destinationDimension"]
    # the dense reference: |<n| Sz_q |0>|^2 at E_n - E_0
    psi = g["vectors"][:, 0]
    sz = np.array([[0.5 if (s >> i) & 1 else -0.5 for i in range(L)] for s in g["states"]])
    phi = (sz @ (np.exp(2j * np.pi * q_index * np.arange(L) / L) / np.sqrt(L))) * psi
    w = np.abs(g["vectors"].T @ phi) ** 2
    poles = g["levels"] - g["levels"][0]
    for k in range(4):
        want = float(np.sum(w * poles ** k))
        print(f"q_index={q_index} moment {k}: {ds.moment(k):.15f} against {want:.15f}")
        assert abs(ds.moment(k) - want) <= 1e-10
    omega = np.linspace(-0.5, 6.0, 131)
    dense = np.array([np.sum(w * (0.1 / np.pi) / ((o - poles) ** 2 + 0.01)) for o in omega])
    got = ds.spectrum(omega, 0.1)
    print(f"q_index={q_index}: largest spectrum difference {np.abs(got - dense).max():.3e} of a maximum {dense.max():.3e}")
    assert np.abs(got - dense).max() <= 1e-9 * dense.max() and dense.max() > 0.1
    assert abs(np.sum(r["weights"]) - r["totalWeight"]) <= 1e-12 and np.all(np.diff(r["poles"]) >= 0) and r["poles"][0] > 0.1
    # the sum rule
    b = capi.Basis(g["ctx"], g["op"], g["n"], 1)
    b.upload(capi.VEC_COL(0), g["x"])
    diag, x2 = b.spin_momentum_measure(capi.VEC_COL(0), [1 | (1 << d) for d in range(1, L)])
    b.close()
    corr = np.concatenate([[0.25], diag / (4.0 * L * x2)])
    static = float(np.real(np.sum(np.exp(2j * np.pi * q_index * np.arange(L) / L) * corr)))
    W = r["totalWeight"]
    print(f"q_index={q_index}: totalWeight {W:.15f}, static {static:.15f}, bound {g['n'] * EPS * (W + L / 4):.3e}")
    assert abs(W - static) <= g["n"] * EPS * (W + L / 4)
    ds.close()


def test_solver_refusals_and_other_kinds(capi, ring12):
    g = ring12
    L, solver = g["L"], g["solver"]
    ds = solver.SpinMomentumDynamicsSolver()
    ds.setModel(g["ctx"], L, g["bonds"], g["n_up"], 0).setState(g["x"]).setStateEnergy(g["e0"]).setLanczosSteps(100)
    for what, args in (("the momentum index p of the site operator must be", (0, [1.0], L)), ("no site operator", (3, [1.0], 0)),
                       ("needs one coefficient per site of the cell", (0, [1.0, 1.0], 0)), ("is not finite of the cell", (0, [np.nan], 0))):
        ds.setSiteOperator(*args).compute()
        assert ds.results()["info_name"] == "InvalidInput" and what in ds.log()[-1], ds.log()
    # S-_q at q = pi from the singlet ground state: the triplet weight, all of it at positive energies; total = <S+_-q S-_q>
    ds.setSiteOperator(2, [1.0 / np.sqrt(L)], L // 2).compute()
    r = ds.results()
    assert r["info_name"] == "Success" and r["destinationSitesUp"] == g["n_up"] - 1 and r["destinationMomentum"] == L // 2 and r["complexRun"] == 0
    z = solver.SpinMomentumDynamicsSolver()
    z.setModel(g["ctx"], L, g["bonds"], g["n_up"], 0).setState(g["x"]).setStateEnergy(g["e0"]).setLanczosSteps(100).computeStructureFactorZ(L // 2)
    # SU(2): <S+_-q S-_q> = 2 <Sz_-q Sz_q> in a singlet, and the spectra coincide
    assert abs(r["totalWeight"] - 2 * z.results()["totalWeight"]) <= 1e-10 and abs(ds.moment(1) - 2 * z.moment(1)) <= 1e-9
    # a complex state of the same sector runs the complex path and gives the same response
    c = solver.SpinMomentumDynamicsSolver()
    c.setModel(g["ctx"], L, g["bonds"], g["n_up"], 0).setState(g["x"] * np.exp(0.3j)).setStateEnergy(g["e0"]).setLanczosSteps(100).computeStructureFactorZ(L // 2)
    assert c.results()["complexRun"] == 1 and abs(c.moment(0) - z.moment(0)) <= 1e-10 and abs(c.moment(2) - z.moment(2)) <= 1e-9
    for s in (ds, z, c):
        s.close()


def test_header_class_in_a_user_program(capi, ring12, tmp_path):
    """tests/cpp/spin_momentum_dynamics_amd.cpp: SpinMomentumDynamicsSolver in a C++11 user program built with -Wall -Wextra, the
    same ring, both paths, held against the same dense diagonalisation"""
    import json
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, lib = str(tmp_path / "spin_momentum_dynamics_amd"), os.path.join(root, "cmpt-eigenex_amd", "lib")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-I", os.path.join(root, "include"), "-I", os.path.join(root, "cmpt-eigenex_amd", "include"),
                           os.path.join(root, "tests", "cpp", "spin_momentum_dynamics_amd.cpp"), "-o", exe, "-L", lib, "-leigenex_hip", "-Wl,-rpath," + lib])
    text = subprocess.check_output([exe, "12", "100"]).decode()
    print(text)
    assert "SPIN MOMENTUM DYNAMICS OK" in text
    o = json.loads(text.splitlines()[0])
    g = ring12
    L = g["L"]
    assert o["sites"] == L and o["dim"] == g["n"] and abs(o["energy"] - g["e0"]) <= 1e-11
    psi, poles = g["vectors"][:, 0], g["levels"] - g["levels"][0]
    sz = np.array([[0.5 if (s >> i) & 1 else -0.5 for i in range(L)] for s in g["states"]])
    for key, q in (("q0", L // 2), ("q1", 1)):
        w = np.abs(g["vectors"].T @ ((sz @ (np.exp(2j * np.pi * q * np.arange(L) / L) / np.sqrt(L))) * psi)) ** 2
        for k in range(4):
            assert abs(o[key]["m%d" % k] - float(np.sum(w * poles ** k))) <= 1e-10
        dense = float(np.sum(w * (0.1 / np.pi) / ((1.0 - poles) ** 2 + 0.01)))
        assert abs(o[key]["spectrum_1"] - dense) <= 1e-9 * max(dense, 0.1)
        assert o[key]["complex"] == (0 if q == L // 2 else 1) and o[key]["dst_momentum"] == (L - q) % L
