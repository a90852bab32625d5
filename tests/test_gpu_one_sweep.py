"""The one-sweep Lanczos step (k_sweep, k_lag_terms, the guard's repair pass; csrc/lag_terms.hpp) on the device.

One shard with a device operator, real data, the batched scheme against every column, no deflation vectors, no filter and no
thick restart re-orthogonalises a step in ONE sweep of the basis; the coefficients a sweep finds are applied one step late and
the known part of that lag is taken out beforehand (tests/one_sweep_reference.py restates the scheme).  Held against the C
oracle, against the restatement at the tile edges, bit for bit across batch schedules and the launch switches (child processes:
the switches are read once per process), against the two-sweep step (EIGENEX_TWO_SWEEPS=1), and through the guard."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import cref
from tests import one_sweep_cases as cases

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import one_sweep_reference as osr  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = (
    ("default", {}),
    ("no_inline_fin", {"EIGENEX_NO_INLINE_FIN": "1"}),
    ("no_graphs", {"EIGENEX_NO_GRAPHS": "1"}),
    ("no_inline_fin_no_graphs", {"EIGENEX_NO_INLINE_FIN": "1", "EIGENEX_NO_GRAPHS": "1"}),
    ("two_sweeps", {"EIGENEX_TWO_SWEEPS": "1"}),
)


@pytest.fixture(scope="module")
def capi():
    from cmpt_eigenex_amd import capi as m

    assert m.device_count() >= 1
    return m


@contextlib.contextmanager
def _state(capi, operator, N, cap, nq=0):
    """(context, basis) of a fresh state; closed in the order basis, operator, context whatever the test does"""
    ctx = capi.Context()
    A = b = None
    try:
        A = operator(ctx)
        b = capi.Basis(ctx, A, N, cap, nq)
        yield ctx, b
    finally:
        if b is not None:
            b.close()
        if A is not None:
            A.close()
        ctx.close()


def _columns(capi, b, n):
    return np.stack([b.download(capi.VEC_COL(c)) for c in range(n)])


def _relation_residual(capi, b, k, alpha, beta, shift=0.0):
    """|| A u_k - beta_{k-1} u_{k-1} - alpha_k u_k - beta_k u_{k+1} ||, as tests/test_gpu_fullsize.py computes it"""
    b.apply(capi.VEC_COL(k), capi.VEC_V, shift)
    first = k - 1 if k > 0 else 0
    h = ([beta[k - 1]] if k > 0 else []) + [alpha[k], beta[k]]
    return np.sqrt(b.update(capi.VEC_V, first, 1, len(h), np.array(h)))


@pytest.mark.parametrize("n, m, shift", [(16, 40, 0.0), (14, 30, 0.3)])
def test_against_the_oracle_and_the_basis(capi, n, m, shift):
    N = n ** 3
    rowptr, col, val = cref.laplacian3d(n)
    init = np.random.default_rng(n).standard_normal(N)
    ref = cref.CLanczos(rowptr, col, val, init, cap=m + 2, shift=shift)
    assert ref.run(m + 1) == m + 1
    with _state(capi, lambda ctx: capi.Csr.laplacian3d(ctx, n), N, m + 1) as (ctx, b):
        b.configure(shift, 1e-12, 1, capi.ORTHO_BATCHED)
        b.upload(capi.VEC_W, init)
        b.lanczos_enqueue(m + 1)
        st, alpha, beta = b.lanczos_state()
        assert (st.nvec, st.iterations, st.nalpha, st.nbeta, st.stopped) == (m + 1, m, m + 1, m, 0)
        V = _columns(capi, b, m + 1)
        repairs = b.repairs()
        residuals = [_relation_residual(capi, b, k, alpha, beta, shift) for k in (0, 1, m // 2, m - 1)]
    orth = np.abs(V @ V.T - np.eye(m + 1)).max()
    dv = np.abs(V - ref.V[: m + 1]).max()
    print(f"{n}^3 m={m}: |dalpha| {np.abs(alpha - ref.alpha).max():.2e} |dbeta| {np.abs(beta - ref.beta).max():.2e} "
          f"orthogonality {orth:.2e} |dV| {dv:.2e} repairs {repairs} relation residuals {max(residuals):.2e}")
    np.testing.assert_allclose(alpha, ref.alpha, rtol=0, atol=1e-12)
    np.testing.assert_allclose(beta, ref.beta, rtol=0, atol=1e-12)
    assert orth < 1e-13 and dv < 1e-9
    assert repairs == 0
    assert max(residuals) < 1e-12 * 12.0


def _cus():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.mark.parametrize("N", [63, 2048, 2049, 4097, 70001, "several tiles per workgroup"])
def test_tile_edges_against_the_restatement(capi, N):
    """rows that end inside, at and one behind a 2048-row tile, and (2 CUs + 1) tiles + 38 rows on a grid of one workgroup per CU"""
    m = 12
    several = isinstance(N, str)
    if several:
        N = (2 * _cus() + 1) * 2048 + 38
    rowptr, col, val = osr.tridiagonal_csr(N)
    init = np.random.default_rng(N).standard_normal(N)
    a_ref, b_ref, V_ref, repairs, _ = osr.one_sweep(osr.csr_apply(rowptr, col, val), init, m)
    with _state(capi, lambda ctx: capi.Csr.upload(ctx, N, rowptr, col, val, column_blocks=0), N, m + 1) as (ctx, b):
        if several:
            b.tune(1, 4, 0)
        b.upload(capi.VEC_W, init)
        b.lanczos_enqueue(m + 1)
        st, alpha, beta = b.lanczos_state()
        assert (st.nvec, st.stopped) == (m + 1, 0) and repairs == 0 and b.repairs() == 0
        V = _columns(capi, b, m + 1)
    print(f"N={N}: |dalpha| {np.abs(alpha - a_ref).max():.2e} |dbeta| {np.abs(beta - b_ref).max():.2e} |dV| {np.abs(V - V_ref).max():.2e}")
    np.testing.assert_allclose(alpha, a_ref, rtol=0, atol=1e-12)
    np.testing.assert_allclose(beta, b_ref, rtol=0, atol=1e-12)
    assert np.abs(V - V_ref).max() < 1e-9
    assert np.abs(V @ V.T - np.eye(m + 1)).max() < 1e-13


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """configuration -> {key: array}; after a child that did not exit normally no further child is started"""
    d = tmp_path_factory.mktemp("one_sweep")
    res, failure = {}, None
    for name, extra in CONFIGS:
        env = {k: v for k, v in os.environ.items() if not k.startswith("EIGENEX_")}
        env.update(extra)
        out = str(d / (name + ".npz"))
        try:
            r = subprocess.run([sys.executable, "-m", "tests.one_sweep_cases", out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        except subprocess.TimeoutExpired as e:
            failure = "%s: timed out\n%s" % (name, (e.stderr or b"")[-4000:])
            break
        if r.returncode != 0:
            failure = "%s: exit status %d\n%s" % (name, r.returncode, r.stderr[-4000:])
            break
        with np.load(out) as z:
            res[name] = {k: z[k] for k in z.files}
    res["_failure"] = failure
    return res


def _need(runs, *names):
    missing = [n for n in names if n not in runs]
    if missing:
        pytest.fail("no results for %s: %s" % (", ".join(missing), runs["_failure"]))
    return [runs[n] for n in names]


@pytest.mark.parametrize("case", list(cases.CASES))
def test_schedules_and_switches_give_the_same_bits(runs, case):
    """alpha, beta, every column, W, the state and the repair counter: identical wherever the batches are cut, with and without
    inline finalisers, with and without recorded graphs"""
    data = _need(runs, *[c[0] for c in CONFIGS[:4]])
    ref = {k.split("/", 2)[2]: v for k, v in data[0].items() if k.startswith(case + "/whole/")}
    assert set(ref) == {"alpha", "beta", "state", "V", "W"} and ref["state"][0] == cases.CASES[case][1]
    for (name, _), d in zip(CONFIGS[:4], data):
        for sched in cases.schedules(cases.CASES[case][1]):
            for k, v in ref.items():
                got = d["%s/%s/%s" % (case, sched, k)]
                assert got.shape == v.shape and np.array_equal(got, v), "%s %s %s differs: max %s" % (name, sched, k, np.abs(got - v).max())


@pytest.mark.parametrize("case", list(cases.CASES))
def test_two_sweep_switch_agrees(runs, case):
    one, two = _need(runs, "default", "two_sweeps")
    for k in ("alpha", "beta"):
        a, b = one["%s/whole/%s" % (case, k)], two["%s/whole/%s" % (case, k)]
        print(case, k, np.abs(a - b).max())
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-13)
    assert not np.array_equal(one[case + "/whole/W"], two[case + "/whole/W"])  # the switch did change the path


def _guard_case(small):
    N = 4099
    d = 1.0 + (np.arange(N) % 60)
    rows = np.array([j + 60 * ((j * 17) % 68) for j in range(60)])
    rows[16] = 4096  # the third tile has rows 4096..4098 only
    assert np.array_equal(rows % 60, np.arange(60)) and rows.max() < N and (rows < 2048).any() and ((rows >= 2048) & (rows < 4096)).any()
    x = np.zeros(N)
    x[rows] = osr.guard_start(60, small)
    return N, d, x


@pytest.mark.parametrize("small, repaired", [(1e-11, True), (1e-6, False)])
def test_guard_close_to_a_breakdown(capi, small, repaired):
    """diag(1 + i mod 60) with a start vector on 60 rows, one per residue: the 60-row case of the restatement, five rows at 1.0
    and the rest tiny, so that beta_4 is tiny but above the threshold and the lagged coefficients are no longer small"""
    N, d, x = _guard_case(small)
    m = 20
    rowptr = np.arange(N + 1, dtype=np.int32)
    col = np.arange(N, dtype=np.int32)
    ref = cref.CLanczos(rowptr, col, d, x, cap=m + 2)
    assert ref.run(m + 1) == m + 1
    with _state(capi, lambda ctx: capi.Csr.upload(ctx, N, rowptr, col, d, column_blocks=0), N, m + 1) as (ctx, b):
        b.upload(capi.VEC_W, x)
        b.lanczos_enqueue(m + 1)
        st, alpha, beta = b.lanczos_state()
        V = _columns(capi, b, st.nvec)
        repairs = b.repairs()
    assert not V[:, x == 0].any()  # every other row stays exactly zero
    orth = np.abs(V @ V.T - np.eye(st.nvec)).max()
    print(f"small={small}: repairs {repairs} orthogonality {orth:.2e} |dalpha| {np.abs(alpha - ref.alpha).max():.2e} "
          f"|dbeta| {np.abs(beta - ref.beta).max():.2e} min beta {beta.min():.2e}")
    assert st.nvec == m + 1
    assert (repairs >= 1) if repaired else (repairs == 0)
    assert orth <= 1e-14
    np.testing.assert_allclose(alpha, ref.alpha, rtol=0, atol=1e-12)
    np.testing.assert_allclose(beta, ref.beta, rtol=0, atol=1e-12)


def test_breakdown_in_a_two_dimensional_invariant_subspace(capi):
    N = 3000
    d = 1.0 + (np.arange(N) % 60)
    rowptr, col = np.arange(N + 1, dtype=np.int32), np.arange(N, dtype=np.int32)
    x = np.zeros(N)
    x[[5, 2071]] = 1.0, -0.5
    ref = cref.CLanczos(rowptr, col, d, x, cap=10)
    ref.run(6)
    with _state(capi, lambda ctx: capi.Csr.upload(ctx, N, rowptr, col, d, column_blocks=0), N, 9) as (ctx, b):
        b.upload(capi.VEC_W, x)
        b.lanczos_enqueue(6)
        st, alpha, beta = b.lanczos_state()
    assert st.stopped == 1 and (st.nvec, st.iterations, st.nalpha, st.nbeta) == (ref.nvec, ref.iterations, ref.alpha.size, ref.beta.size) == (2, 1, 2, 2)
    assert beta[-1] <= 1e-12
    np.testing.assert_allclose(alpha, ref.alpha, rtol=0, atol=1e-12)
    np.testing.assert_allclose(beta[:-1], ref.beta[:-1], rtol=0, atol=1e-12)


def _launches(capi, prepare, calls):
    """(update launches, dots launches, dots bytes, state) of one batch of `calls` calls on a state of nine vectors"""
    n = 12
    N = n ** 3
    nq = prepare.get("nq", 0)
    with _state(capi, lambda ctx: capi.Csr.laplacian3d(ctx, n), N, 40, nq) as (ctx, b):
        b.configure(0.0, 1e-12, prepare.get("interval", 1), capi.ORTHO_BATCHED)
        for q in range(nq):
            e = np.zeros(N)
            e[q] = 1.0
            b.upload(capi.VEC_ORTHO(q), e)
        b.upload(capi.VEC_W, np.random.default_rng(5).standard_normal(N))
        b.lanczos_enqueue(9)
        if prepare.get("restart"):
            st, alpha, beta = b.lanczos_state()
            k = st.nvec - 1
            T = np.diag(alpha[:k]) + np.diag(beta[: k - 1], 1) + np.diag(beta[: k - 1], -1)
            S = np.linalg.eigh(T)[1][:, :3]
            b.lanczos_restart(S, beta[k - 1] * S[k - 1, 2])
        ctx.profile_enable(True)
        ctx.profile_reset()
        b.lanczos_enqueue(calls)
        st = b.lanczos_state()[0]
        upd, dots = ctx.profile_get(capi.K_UPDATE), ctx.profile_get(capi.K_DOTS)
        ctx.profile_enable(False)
    return upd[0], dots[0], dots[2], st


def test_other_states_keep_the_two_sweep_step(capi):
    """through the profile: a one-sweep call books the sweep and the (unarmed) repair update as two update launches and a closing
    pass per batch, and its only dots launch (the repair's) books no bytes; a two-sweep call books one of each, with bytes"""
    calls = 4
    upd, dots, dots_bytes, st = _launches(capi, {}, calls)
    assert (upd, dots, dots_bytes) == (2 * calls + 1, calls, 0.0) and st.stopped == 0
    for prepare in ({"restart": True}, {"nq": 1}, {"interval": 3}):
        upd, dots, dots_bytes, st = _launches(capi, prepare, calls)
        assert upd == calls and dots_bytes > 0.0 and st.stopped == 0, prepare
