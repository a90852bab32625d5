"""The kernels that read a stored operator (library.hip: launch_operator) as the Krylov steps use them, past one tile.
eigenex_apply, which the layout suites pin bit for bit, launches them with scale = NULL, u_out = NULL, pass_flags = 0,
shift_im = 0 and a control block that is always zero; a Lanczos or Arnoldi step (enq_apply) sets a scale (the input is normalised
inside the kernel), stores the column or not, writes alpha or norm partial sums, sets kPassSelfNorm in the adaptive Arnoldi step,
may carry a complex shift, and reads the live ctrl->stopped.

Every case makes eight step calls on a state of nine columns and gives the downloaded state to tests/krylov_local_reference.py
with the host rows of tests/layout_pass_cases.py: every step within (n + k) eps (|H|_1 + |shift|) of the extended-precision step
from the stored columns, max |U^H U - I| <= (n + k) eps (tests/test_layout_pass_cases_host.py holds the fp64 recurrences to a
tenth of that on the same rows).  The same calls on the plain-CSR state (column_blocks = 0) give the (nvec, iterations, stopped)
and the series lengths to equal and the diagnostic print of the trajectory differences.  Row codes, 64-bit row pointers and
column-blocked passes keep the plain kernel's 256-row tiles and grid: their columns, coefficients, residue and work vectors equal
the plain-CSR state's bit for bit in every scheme.

Schemes: tests/krylov_pass_runs.py.  Lanczos schemes run on the symmetric / Hermitian operator of a family, Arnoldi schemes on the
general one.  Branch of launch_operator against case, measured ratios and the seeded faults: profiles/layout_krylov_passes.md."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import krylov_local_reference as kl  # noqa: E402
import layout_pass_cases as lc  # noqa: E402
from krylov_pass_runs import CALLS, SCHEMES, arnoldi, columns, lanczos, two_sweeps_forced  # noqa: E402

pytestmark = pytest.mark.gpu
CAPACITY = CALLS + 1


@pytest.fixture(scope="module")
def mods():
    from cmpt_eigenex_amd import capi, solver

    assert capi.device_count() >= 1
    return capi, solver


class _Handles:
    """contexts by (shards, halo overlap) and operators by (context, family, kind, layout), built once for the module; every state
    a case creates is registered here and closed before its operator and its context"""

    def __init__(self, capi):
        self.capi, self.ctxs, self.ops, self.bases = capi, {}, {}, []

    def ctx(self, shards=1, overlap=None):
        key = (shards, overlap)
        if key not in self.ctxs:
            c = self.capi.Context(loopback_shards=shards) if shards > 1 else self.capi.Context()
            if overlap is not None:
                assert c.set_halo_overlap(overlap) == overlap
            self.ctxs[key] = c
        return self.ctxs[key]

    def op(self, family, kind, layout, shards=1, overlap=None):
        key = (shards, overlap, family, kind, layout)
        if key not in self.ops:
            A = lc.upload(self.capi, self.ctx(shards, overlap), family, kind, layout)
            self.ops[key] = A
            want = ("upload", 0, "csr", "plain", 1, False) if layout == "plain" else lc.LAYOUTS[layout]
            assert (A.layout(), A.encoding(), A.column_blocks()) == want[2:5], (key, A.layout(), A.encoding(), A.column_blocks())
            assert bool(getattr(A, "is_complex", False)) == lc.is_complex(family)
        return self.ops[key]

    def register(self, b):
        self.bases.append(b)

    def close_bases(self):
        for b in self.bases:
            b.close()
        self.bases.clear()

    def close(self):
        self.close_bases()
        for A in self.ops.values():
            A.close()
        for c in self.ctxs.values():
            c.close()


@pytest.fixture(scope="module")
def handles(mods):
    h = _Handles(mods[0])
    yield h
    h.close()


@pytest.fixture(autouse=True)
def _states_closed(handles):
    yield
    handles.close_bases()  # also when the test failed: basis, then (at the end of the module) operator, then context


def _one_sweep(capi, mode, cplx, shards):
    return mode == capi.ORTHO_BATCHED and not cplx and shards == 1 and not two_sweeps_forced()


def _same_bits(label, got, ref, keys):
    for k in keys:
        assert np.asarray(got[k]).tobytes() == np.asarray(ref[k]).tobytes(), f"{label}: {k} differs from the plain-CSR state"


def _run_scheme(handles, family, layout, scheme, batches=None, capacity=CAPACITY, big=False, shards=1, overlap=None, tag=""):
    """one scheme on one operator at each of its shifts: the local check asserted on the state of the layout, the plain-CSR state
    driven with the same calls as the diagnostic (and bit for bit where the library promises it)"""
    capi = handles.capi
    is_lanczos, mode_name, default_batches, shifts, _ = SCHEMES[scheme]
    batches = batches or default_batches
    mode = getattr(capi, mode_name)
    kind = "sym" if is_lanczos else "gen"
    rows = lc.rows(family, kind)
    n = rows[0].size - 1
    cplx = lc.is_complex(family)
    ctx = handles.ctx(shards, overlap)
    M, A = handles.op(family, kind, layout, shards, overlap), handles.op(family, kind, "plain", shards, overlap)
    x = lc.start(family)
    bitwise = layout != "plain" and lc.LAYOUTS[layout][5]
    run = lanczos if is_lanczos else arnoldi
    calls = sum(batches)
    for shift in shifts:
        got, bm = run(capi, ctx, M, n, x, batches, shift, mode, capacity, big, prepare=handles.register)
        ref, ba = run(capi, ctx, A, n, x, batches, shift, mode, capacity, big, prepare=handles.register)
        label = f"{tag}{family} {layout} n={n} scheme {scheme} shift={shift}"
        assert got["state"] == ref["state"] and got["lengths"] == ref["lengths"], (label, got["state"], ref["state"])
        if is_lanczos:
            got["w"], ref["w"], got["v"], ref["v"] = bm.download(capi.VEC_W), ba.download(capi.VEC_W), bm.download(capi.VEC_V), ba.download(capi.VEC_V)
            assert got["state"] == (calls, calls - 1, 0) and got["lengths"] == (calls, calls - 1), (label, got["state"], got["lengths"])
            print(f"{label}: against the plain-CSR state alpha differs by {np.abs(got['alpha'] - ref['alpha']).max():.3e}, "
                  f"beta by {np.abs(got['beta'] - ref['beta']).max():.3e}, columns by {np.abs(got['U'] - ref['U']).max():.3e}")
            if not _one_sweep(capi, mode, cplx, shards):  # the two-sweep step (on real handles with store_u)
                assert got["repairs"] == 0 and not got["pending"], label
            elif "EIGENEX_EAGER_CLOSE" not in os.environ:
                assert got["pending"], label  # the batch of one-sweep steps has left its newest column for later
            rep = kl.check_lanczos(rows, shift, got["U"], got["alpha"], got["beta"])
            keys = ("U", "alpha", "beta", "w", "v")
        else:
            assert got["state"][0] == calls and got["state"][2] == 0 and got["lengths"][0] == calls, (label, got["state"], got["lengths"])
            print(f"{label}: against the plain-CSR state H differs by {np.abs(got['H'] - ref['H']).max():.3e}, "
                  f"the residue by {abs(got['residue'] - ref['residue']):.3e}, columns by {np.abs(got['U'] - ref['U']).max():.3e}")
            rep = kl.check_arnoldi(rows, shift, got["U"], got["H"], got["residue"], got["w"])
            keys = ("U", "H", "residue", "w")
        print(rep.line(label))
        print(f"RATIO {tag}{family} {layout} {scheme} shift={shift} {rep.ratio():.3e} ortho {rep['ortho'] / rep['ortho_bound']:.3e}")
        assert rep.ok(), rep.line(label)
        if bitwise:
            _same_bits(label, got, ref, keys)
        handles.close_bases()


def _schemes_of(family):
    return [s for s in SCHEMES if lc.is_complex(family) or not SCHEMES[s][4]]  # a complex shift needs a complex state


STEPS = [(f, lay, s) for f, lay in lc.STEP_CASES for s in _schemes_of(f)]


@pytest.mark.parametrize("family,layout,scheme", STEPS, ids=[f"{f}-{lay}-{s}" for f, lay, s in STEPS])
def test_steps_pass_the_local_check(handles, family, layout, scheme):
    _run_scheme(handles, family, layout, scheme)


# ---- loopback shards: interior and boundary tile lists, the neighbour exchange beside or in front of the operator ------------------
SHARDED = [(f, lay, ov, s) for f, lay in lc.SHARD_CASES for ov in ((True, False) if (f, lay) == ("band9001", "csr") else (None,))
           for s in ("a", "b_twice", "c", "d")]


@pytest.mark.parametrize("family,layout,overlap,scheme", SHARDED, ids=[f"{f}-{lay}-{'default' if ov is None else 'overlap' if ov else 'serial'}-{s}" for f, lay, ov, s in SHARDED])
def test_steps_on_three_loopback_shards(handles, family, layout, overlap, scheme):
    """9,001 rows in three shards of about 12 tiles.  Plain CSR on the banded operator has interior and boundary tile lists (the
    partial dots of the two launches side by side), once with the neighbour exchange beside the interior rows and once in
    front of the operator; on the uniformly random columns every tile is a boundary tile; 70,001 rows keep three input slices per shard, so the column-sorted tiles stay eligible; split
    tiles of 256 rows and dense blocks cut by the shard boundaries.  No layout falls back: op() asserts layout()."""
    _run_scheme(handles, family, layout, scheme, shards=3, overlap=overlap, tag="shards3-")


# ---- the tile loop going round inside a step ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["a", "d"])
@pytest.mark.parametrize("family,layout", lc.TILE_LOOP_CASES, ids=[f"{f}-{lay}" for f, lay in lc.TILE_LOOP_CASES])
def test_steps_with_the_tile_loop_going_round(handles, family, layout, scheme):
    """one operator workgroup per CU (tune(2, 1, 0)) on 274 tiles of 256 rows (plain, three column-blocked passes): the grid is
    smaller than the tile count, so the tile loop goes round with the scale, the partial sums and (d) kPassSelfNorm.  The
    column-sorted layout has 69 tiles of 1024 rows here, fewer than workgroups: its case holds the smaller grid (other partial
    sums per workgroup, idle workgroups), not a second trip round the loop"""
    _run_scheme(handles, family, layout, scheme, big=True, tag="big-")


# ---- breakdown inside a batch --------------------------------------------------------------------------------------------------------
def _sentinel(n, cplx):
    s = np.cos(np.arange(n) * 0.37) + 3.0
    return s + 0.5j * s if cplx else s


def _breakdown(handles, family, layout, shards=1):
    """a start vector on the five rows that are coupled to nothing else: eight calls in one batch, Lanczos and Arnoldi (default and
    adaptive), against the plain-CSR state on one shard driven with the same calls"""
    capi = handles.capi
    rows = lc.rows(family, "sym")
    n = rows[0].size - 1
    cplx = lc.is_complex(family)
    ctx_m, ctx_a = handles.ctx(shards), handles.ctx()
    M, A = handles.op(family, "sym", layout, shards), handles.op(family, "sym", "plain")
    x = lc.start(family, support=lc.SUPPORT)
    sentinel = _sentinel(n, cplx)
    bitwise = shards == 1 and lc.LAYOUTS[layout][5]
    tag = f"breakdown-{'shards3-' if shards > 1 else ''}"
    label = f"{tag}{family} {layout}"

    def prepare(b):
        handles.register(b)
        for c in range(CAPACITY):
            b.upload(capi.VEC_COL(c), sentinel)

    def untouched(b, nvec):
        for c in range(nvec, CAPACITY):
            assert b.download(capi.VEC_COL(c)).tobytes() == np.ascontiguousarray(sentinel, b.dtype).tobytes(), f"{label}: column {c} was written after the stop"

    for mode, name in ((capi.ORTHO_BATCHED, "a"), (capi.ORTHO_BATCHED, "c"), (capi.ORTHO_BATCHED_ADAPTIVE, "d")):
        run = lanczos if name == "a" else arnoldi
        got, bm = run(capi, ctx_m, M, n, x, (CALLS,), 0.0, mode, CAPACITY, prepare=prepare)
        ref, ba = run(capi, ctx_a, A, n, x, (CALLS,), 0.0, mode, CAPACITY, prepare=prepare)
        print(f"{label} {name}: state {got['state']}, lengths {got['lengths']}, " + (f"beta {got['beta']}" if name == "a" else f"residue {got['residue']:.3e}"))
        assert got["state"] == ref["state"] and got["lengths"] == ref["lengths"], (label, name, got["state"], ref["state"], got["lengths"], ref["lengths"])
        assert got["state"][2] == 1 and got["state"][0] == lc.SUPPORT, (label, name, got["state"])
        if name == "a":
            got["w"], ref["w"], got["v"], ref["v"] = bm.download(capi.VEC_W), ba.download(capi.VEC_W), bm.download(capi.VEC_V), ba.download(capi.VEC_V)
            rep = kl.check_lanczos(rows, 0.0, got["U"], got["alpha"], got["beta"])
            keys = ("U", "alpha", "beta", "w", "v")
        else:
            rep = kl.check_arnoldi(rows, 0.0, got["U"], got["H"], got["residue"], got["w"])
            keys = ("U", "H", "residue", "w")
        print(rep.line(f"{label} {name}"))
        print(f"RATIO {tag}{family} {layout} {name} shift=0.0 {rep.ratio():.3e} ortho {rep['ortho'] / rep['ortho_bound']:.3e}")
        assert rep.ok(), rep.line(f"{label} {name}")
        untouched(bm, got["state"][0])
        untouched(ba, ref["state"][0])
        if bitwise:
            _same_bits(f"{label} {name}", got, ref, keys)
        handles.close_bases()


@pytest.mark.parametrize("family,layout", lc.BREAKDOWN_CASES, ids=[f"{f}-{lay}" for f, lay in lc.BREAKDOWN_CASES])
def test_breakdown_inside_a_batch(handles, family, layout):
    """the recurrence ends after five columns, the device sets ctrl->stopped inside the batch and every later operator launch of the
    batch returns at once: the state and the lengths of the series equal the plain-CSR state's, the steps before the stop pass the
    local check, the columns beyond nvec are the sentinel that was uploaded before the batch, and the layouts that promise the
    plain kernel's bits keep them up to the stop"""
    _breakdown(handles, family, layout)


@pytest.mark.parametrize("family,layout", lc.SHARD_BREAKDOWN_CASES, ids=[f"{f}-{lay}" for f, lay in lc.SHARD_BREAKDOWN_CASES])
def test_breakdown_inside_a_batch_on_three_loopback_shards(handles, family, layout):
    """the same through the interior and boundary tile lists: two operator launches per application, a control block per shard,
    and a start vector that lives on the first shard alone, so that the other two learn of the stop through the reduction inside
    the captured batch.  The state to equal is that of the plain-CSR operator on one shard."""
    _breakdown(handles, family, layout, shards=3)


# ---- filter and moments off the epilogue path --------------------------------------------------------------------------------------
FILTER_CASES = [("s40000_4", "sorted"), ("r9001", "split")]
_FILTER_REFS = {}


def _filter_reference(family):
    """x, the filter of degree 12, p(A) x in long double with the float64 restatement's own error against it, the float64
    Chebyshev vectors t_0 .. t_8 in the device's order with their own errors -- once per operator"""
    import density_reference as dr
    import filter_reference as fr
    import scipy.sparse as sp

    if family not in _FILTER_REFS:
        rowptr, col, val = lc.rows(family, "sym")
        n = rowptr.size - 1
        S = sp.csr_matrix((val, col, rowptr), shape=(n, n))
        x = np.random.RandomState(17).standard_normal(n)
        lo, hi = fr.gershgorin(S)
        c, h = dr.widened(lo, hi)
        mu = fr.delta_coefficients(0.3 * h + c, c, h, 12)
        ld = np.longdouble
        y64 = fr.apply_filter(fr.csr_rowsum_matmul_any_rows(rowptr, col, val, np.float64), x, mu, c, h)
        yld = fr.apply_filter(fr.csr_rowsum_matmul_any_rows(rowptr, col, val, ld), x.astype(ld), mu, c, h)
        d = dr.applications(16)
        ts = dr.chebyshev_vectors(dr.device_matmul(S), x, c, h, d)
        tl = dr.chebyshev_vectors(fr.csr_rowsum_matmul_any_rows(rowptr, col, val, ld), x.astype(ld), c, h, d)
        _FILTER_REFS[family] = dict(x=x, c=c, h=h, mu=mu, yld=yld, err64=float(np.abs(y64.astype(ld) - yld).max()), ts=ts,
                                    terr64=[float(np.abs(a.astype(ld) - b).max()) for a, b in zip(ts, tl)])
    return _FILTER_REFS[family]


@pytest.mark.parametrize("family,layout", FILTER_CASES, ids=[f"{f}-{lay}" for f, lay in FILTER_CASES])
def test_filter_apply_behind_k_cheb_combine(handles, family, layout):
    """eigenex_filter_apply of degree 12 where the operator kernel has no epilogue for the Chebyshev step (filter_in_epilogue is
    false): the operator stores y and k_cheb_combine follows.  The bound of tests/test_gpu_filter.py: device error <= 4 x the
    float64 restatement's own error against long double + 4 eps sum|mu| |x|_inf."""
    capi = handles.capi
    r = _filter_reference(family)
    n = r["x"].size
    b = capi.Basis(handles.ctx(), handles.op(family, "sym", layout), n, 3)
    handles.register(b)
    b.set_filter(r["mu"], r["c"], r["h"])
    b.upload(capi.VEC_COL(0), r["x"])
    b.filter_apply(capi.VEC_COL(0), capi.VEC_V)
    y = b.download(capi.VEC_V)
    err = float(np.abs(y.astype(np.longdouble) - r["yld"]).max())
    bound = 4 * r["err64"] + 4 * kl.EPS * np.abs(r["mu"]).sum() * np.abs(r["x"]).max()
    print(f"{family} {layout} degree=12: device error {err:.3e}, float64 restatement {r['err64']:.3e}, bound {bound:.3e}")
    assert np.abs(y).max() > 0 and err <= bound
    np.testing.assert_array_equal(b.download(capi.VEC_COL(0)), r["x"])  # the input is left alone


@pytest.mark.parametrize("family,layout", FILTER_CASES, ids=[f"{f}-{lay}" for f, lay in FILTER_CASES])
def test_kpm_moments_behind_k_cheb_moments(handles, family, layout):
    """eigenex_kpm_moments, 16 moments, on the same two layouts: the operator stores y and k_cheb_moments follows.  The checks and
    bounds of tests/test_gpu_density.py (tests/density_reference.py: check_vector, check_moments): the column-sorted tiles add a
    row in stored order, so the last Chebyshev vector equals the float64 restatement bit for bit; the split tiles re-associate a
    row's sum and take the bounds of the operators that round otherwise."""
    import density_reference as dr

    capi = handles.capi
    r = _filter_reference(family)
    vector_bound = (lambda k: dr.rounded_vector_bound(r["terr64"][k], r["x"])) if layout == "split" else None
    n, d = r["x"].size, len(r["ts"]) - 1
    b = capi.Basis(handles.ctx(), handles.op(family, "sym", layout), n, 3)
    handles.register(b)
    b.upload(capi.VEC_COL(0), r["x"])
    mu = b.kpm_moments(capi.VEC_COL(0), 16, r["c"], r["h"])
    dr.check_vector(f"{family} {layout} t_{d}", b.download(capi.VEC_V), r["ts"][d], vector_bound(d) if vector_bound else None)
    dr.check_moments(f"{family} {layout}", mu, r["ts"], 16, vector_bound)
    np.testing.assert_array_equal(b.download(capi.VEC_COL(0)), r["x"])
