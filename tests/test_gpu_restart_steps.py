"""Restarted Lanczos and Arnoldi states, step by step and in every transition: the state that eigenex_lanczos_restart or
eigenex_arnoldi_restart has rewritten is what ThickRestartLanczosEigenSolver, FilteredLanczosEigenSolver and KrylovSchurEigenSolver
hold for nearly their whole run, and it runs code of its own: t_restarted takes a real one-shard state off the one-sweep step and
is a bit of the step-graph key, eigenex_basis_clear puts the one-sweep step back, eigenex_basis_clone copies the flag and
Ctrl::keep_coupling, eigenex_basis_reserve moves a projected matrix with a full block in it, the first Arnoldi step behind a restart
must leave the coupling row alone, and the first Lanczos step meets components of order one along every kept column.

Every case of tests/restart_step_cases.py makes its calls (the runners of tests/krylov_pass_runs.py, with the restarts of
restart_step_cases between the batches), and after every restart and the steps behind it holds
  the counters and series lengths; column nkeep, alpha[nkeep] and beta[nkeep - 1] (Lanczos), W, the residue and H == B (Arnoldi)
  bit for bit;
  the combination Y = V C within the unchanged bound of tests/ritz_reference.py;
  the kept relation within its bound (tests/krylov_local_reference.py: check_kept_lanczos, check_kept_arnoldi);
  the local step check from first = nkeep with the module's unchanged bound, orthogonality of all columns within (n + k) eps.
tests/test_restart_step_reference_host.py holds the fp64 recurrence of every case to a tenth of these and shows every fault of
kl.RESTART_FAULTS a hundred times outside.  The host builds each cycle's T as the front-end does and reads nothing of the device's
series below nkeep (stale by design) except the echo of coupling_last.

Also: which step ran before and behind a restart and after clear(); clone() and reserve() of a restarted state; three cycles whose
second and third replay the first's recorded graph; three schedules of the calls behind a restart, bit for bit; a breakdown behind
a restart.  Measured ratios, the seeded device faults and the file's time: profiles/restart_steps.md."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import krylov_local_reference as kl  # noqa: E402
import restart_step_cases as rc  # noqa: E402
from krylov_pass_runs import arnoldi_state, lanczos_state, two_sweeps_forced  # noqa: E402

pytestmark = pytest.mark.gpu

M, N = rc.M, rc.N
CAP = 2 * M + 1  # a Lanczos restart keeping m needs (m + 1) + m columns
ERR_STATE = -4   # include/eigenex_hip.h


@pytest.fixture(scope="module")
def mods():
    from cmpt_eigenex_amd import capi, solver

    assert capi.device_count() >= 1
    return capi, solver


class _Handles:
    """contexts by shards and operators by (shards, kind, complex), built once for the module; every state a test creates is
    registered here and closed before its operator and its context"""

    def __init__(self, capi, solver):
        self.capi, self.solver, self.ctxs, self.ops, self.bases = capi, solver, {}, {}, []

    def ctx(self, shards):
        if shards not in self.ctxs:
            self.ctxs[shards] = self.capi.Context(loopback_shards=shards) if shards > 1 else self.capi.Context()
        return self.ctxs[shards]

    def op(self, c):
        key = (c["shards"], c["kind"], c["cplx"])
        if key not in self.ops:
            self.ops[key] = rc.upload(self.capi, self.ctx(c["shards"]), c)
        return self.ops[key]

    def register(self, b):
        self.bases.append(b)
        return b

    def basis(self, c, capacity=CAP, start=True):
        """a state of the case with its settings and (start) its start vector"""
        b = self.register(self.capi.Basis(self.ctx(c["shards"]), self.op(c), N, capacity))
        b.configure(shift=c["shift"], ortho_mode=getattr(self.capi, rc.SCHEMES[c["scheme"]][1]))
        if c["fusion"] is not None:
            b.set_alpha_fusion(c["fusion"])
        if start:
            b.upload(self.capi.VEC_W, rc.inputs(c["kind"], c["cplx"])[1])
        return b

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
    h = _Handles(*mods)
    yield h
    h.close()


@pytest.fixture(autouse=True)
def _states_closed(handles):
    yield
    handles.close_bases()


def _same(a, b, keys, what):
    for key in keys:
        assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), f"{what}: {key} differs"


LANCZOS_KEYS = ("state", "lengths", "alpha", "beta", "U", "pending", "repairs")
ARNOLDI_KEYS = ("state", "lengths", "H", "residue", "U", "w")


def _lanczos_first(handles, c, capacity=CAP):
    """the unrestarted run: m + 1 calls in the scheme of the later calls; (state, basis, the host's T)"""
    b = handles.basis(c, capacity)
    b.lanczos_enqueue(M + 1)
    prev = lanczos_state(handles.capi, b)
    assert prev["state"] == (M + 1, M, 0) and prev["lengths"] == (M + 1, M), (c["name"], prev["state"], prev["lengths"])
    return prev, b, kl.restart_T([], [], prev["alpha"], prev["beta"], M)


def _lanczos_cycle(handles, c, b, prev, T, i=1, batches=None):
    """one restart and the calls behind it with every assertion of a restarted Lanczos state; (cycle, the next T)"""
    k = c["nkeep"]
    cy, after, T = rc.lanczos_restart(handles.capi, b, c, prev, T, batches)
    it = prev["state"][1]
    assert after["state"] == (k + 1, it, 0) and after["lengths"] == (k + 1, k), (c["name"], i, after["state"], after["lengths"])
    assert after["U"][k].tobytes() == prev["U"][M].tobytes(), f"{c['name']}: column nkeep is not u_m bit for bit"
    assert after["alpha"][k] == prev["alpha"][M] and after["beta"][k - 1] == cy["coupling_last"]
    got = cy["got"]
    calls = sum(rc.batches_behind(c, M - k) if batches is None else batches)
    assert got["state"] == (k + 1 + calls, it + calls, 0) and got["lengths"] == (k + 1 + calls, k + calls), (c["name"], i, got["state"], got["lengths"])
    assert got["beta"][k - 1] == cy["coupling_last"]  # the echo, bit for bit: all that is asserted of coupling_last
    assert got["U"][: k + 1].tobytes() == after["U"].tobytes()  # the steps leave the kept columns alone
    if calls == M - k:
        r = rc.check_cycle(c, cy)
        print("RATIO " + rc.line(c["name"], i, r))
        print(r["step"].line(c["name"]) + "\n" + r["kept"].line(c["name"]))
        assert r["comb"] <= 1.0, rc.line(c["name"], i, r)
        assert r["kept"].ok(), r["kept"].line(c["name"])
        assert r["step"].ok(), r["step"].line(c["name"])
    return cy, T


def _arnoldi_first(handles, c, capacity=CAP):
    b = handles.basis(c, capacity)
    b.arnoldi_enqueue(M)
    prev = arnoldi_state(handles.capi, b)
    assert prev["state"] == (M, M, 0) and prev["lengths"][0] == M, (c["name"], prev["state"], prev["lengths"])
    return prev, b


def _hessenberg_behind(H, k):
    """nothing below B in the kept columns, nothing below the subdiagonal behind them"""
    return not H[k + 1:, :k].any() and all(not H[j + 2:, j].any() for j in range(k, H.shape[1]))


def _arnoldi_cycle(handles, c, b, prev, i=1, batches=None):
    """one restart and the calls behind it with every assertion of a restarted Arnoldi state"""
    cy, after = rc.arnoldi_restart(handles.capi, handles.solver, b, c, prev, batches)
    k, Q, B, it = cy["k"], cy["Q"], cy["B"], prev["state"][1]
    assert i > 1 or k == c["nkeep"], (c["name"], k)  # (a conjugate pair on the cut may move a later cycle's by one)
    assert after["state"] == (k, it, 0) and after["lengths"][0] == k, (c["name"], i, after["state"], after["lengths"])
    assert after["H"].tobytes() == np.asarray(B, after["H"].dtype).tobytes(), f"{c['name']}: H is not B bit for bit"
    assert after["residue"] == prev["residue"] and after["w"].tobytes() == prev["w"].tobytes(), f"{c['name']}: W or the residue moved"
    got = cy["got"]
    calls = sum(rc.batches_behind(c, M - k) if batches is None else batches)
    assert got["state"] == (k + calls, it + calls, 0) and got["lengths"][0] == k + calls, (c["name"], i, got["state"], got["lengths"])
    H = got["H"]
    assert H[: k + 1, :k].tobytes() == np.asarray(B, H.dtype).tobytes(), f"{c['name']}: the steps behind the restart changed B"
    assert H[k, k - 1] == B[k, k - 1] == prev["residue"] * Q[M - 1, k - 1], f"{c['name']}: the coupling entry did not survive"
    assert _hessenberg_behind(H, k), c["name"]
    assert got["U"][:k].tobytes() == after["U"].tobytes()
    if k + calls == M:
        r = rc.check_cycle(c, cy)
        print("RATIO " + rc.line(c["name"], i, r))
        print(r["step"].line(c["name"]) + "\n" + r["kept"].line(c["name"]))
        assert r["comb"] <= 1.0, rc.line(c["name"], i, r)
        assert r["kept"].ok(), r["kept"].line(c["name"])
        assert r["step"].ok(), r["step"].line(c["name"])
    return cy


def _graphs(b):
    return b.graph_info()["graphs"]


LANCZOS_ONE = [c["name"] for c in rc.LANCZOS_GRID + rc.LANCZOS_EDGES + rc.LANCZOS_SHIFT]
ARNOLDI_ONE = [c["name"] for c in rc.ARNOLDI_GRID]


@pytest.mark.parametrize("name", LANCZOS_ONE)
def test_lanczos_steps_behind_a_restart(handles, name):
    c = rc.BY_NAME[name]
    prev, b, T = _lanczos_first(handles, c)
    _lanczos_cycle(handles, c, b, prev, T)


@pytest.mark.parametrize("name", ARNOLDI_ONE)
def test_arnoldi_steps_behind_a_restart(handles, name):
    c = rc.BY_NAME[name]
    prev, b = _arnoldi_first(handles, c)
    _arnoldi_cycle(handles, c, b, prev)


@pytest.mark.parametrize("name", [c["name"] for c in rc.LANCZOS_CYCLES + rc.ARNOLDI_CYCLES])
def test_three_cycles_replay_the_first_cycles_graph(handles, name):
    """the same nkeep and the same batch sizes in every cycle: the second and third restart replay the graph the first recorded,
    over a basis whose contents have changed, and every cycle passes the checks of the first"""
    c = rc.BY_NAME[name]
    graphs = []
    if c["kind"] == "lanczos":
        prev, b, T = _lanczos_first(handles, c)
        before = _graphs(b)
        for i in range(1, c["cycles"] + 1):
            cy, T = _lanczos_cycle(handles, c, b, prev, T, i)
            prev = cy["got"]
            graphs.append(_graphs(b))
    else:
        prev, b = _arnoldi_first(handles, c)
        before, keeps = _graphs(b), []
        for i in range(1, c["cycles"] + 1):
            cy = _arnoldi_cycle(handles, c, b, prev, i)
            prev = cy["got"]
            keeps.append(cy["k"])
            graphs.append(_graphs(b))
    print(f"GRAPHS {name}: {before} after the first run, {graphs} after the cycles" + (f", kept {keeps}" if c["kind"] == "arnoldi" else ""))
    if c["kind"] == "lanczos" or len(set(keeps)) == 1:  # (an Arnoldi cycle that kept one more has another batch size)
        assert graphs[1] == graphs[0] and graphs[2] == graphs[0], (name, before, graphs)
    if before > 0:  # this state records its batches at all (one context without a communicator, graphs not turned off)
        assert graphs[0] > before, (name, before, graphs)  # a restarted batch is not the unrestarted one's graph


def _schedules(calls):
    return ((calls,), (1, calls - 1), (1,) * calls)


@pytest.mark.parametrize("name", [c["name"] for c in rc.LANCZOS_SPLITS])
def test_lanczos_batches_behind_a_restart_give_the_same_bits(handles, name):
    c = rc.BY_NAME[name]
    runs = []
    for batches in _schedules(M - c["nkeep"]):
        prev, b, T = _lanczos_first(handles, c)
        cy, _ = _lanczos_cycle(handles, c, b, prev, T, batches=batches)
        runs.append(cy["got"])
        handles.close_bases()
    for other, batches in zip(runs[1:], _schedules(M - c["nkeep"])[1:]):
        _same(runs[0], other, ("state", "lengths", "alpha", "beta", "U"), f"{name}: one batch against {batches}")


@pytest.mark.parametrize("name", [c["name"] for c in rc.ARNOLDI_SPLITS])
def test_arnoldi_batches_behind_a_restart_give_the_same_bits(handles, name):
    c = rc.BY_NAME[name]
    runs = []
    for batches in _schedules(M - c["nkeep"]):
        prev, b = _arnoldi_first(handles, c)
        cy = _arnoldi_cycle(handles, c, b, prev, batches=batches)  # (the coupling entry is asserted in each)
        runs.append(cy["got"])
        handles.close_bases()
    for other, batches in zip(runs[1:], _schedules(M - c["nkeep"])[1:]):
        _same(runs[0], other, ARNOLDI_KEYS, f"{name}: one batch against {batches}")


def test_a_restart_takes_the_one_sweep_step_away_and_clear_puts_it_back(handles):
    """a real one-shard ORTHO_BATCHED state: the one-sweep step leaves its newest column pending at the end of a batch; behind a
    restart the two-sweep step runs (nothing pending, no repair booked); after clear() and the same start vector the run is that
    of a fresh state of the same capacity, pending close and repairs included"""
    capi = handles.capi
    c = rc.BY_NAME["lr-batched-k7-s1"]
    prev, b, T = _lanczos_first(handles, c)
    if not two_sweeps_forced():
        assert prev["pending"], "the unrestarted state did not take the one-sweep step"
    cy, _ = _lanczos_cycle(handles, c, b, prev, T)
    assert not cy["got"]["pending"] and cy["got"]["repairs"] == prev["repairs"]
    b.clear()
    b.upload(capi.VEC_W, rc.inputs("lanczos", False)[1])
    b.lanczos_enqueue(M + 1)
    again = lanczos_state(capi, b)
    fresh, _, _ = _lanczos_first(handles, c)
    _same(fresh, again, LANCZOS_KEYS, "after clear() against a fresh state")
    assert again["pending"] == prev["pending"]


@pytest.mark.parametrize("name", ["ar-adaptive-k17-s1", "az-default-k9-s3"])
def test_clear_of_a_restarted_arnoldi_state_starts_from_nothing(handles, name):
    """the full block a restart left in the projected matrix is gone: the new run's matrix is Hessenberg and the run is a fresh
    state's"""
    capi = handles.capi
    c = rc.BY_NAME[name]
    prev, b = _arnoldi_first(handles, c)
    _arnoldi_cycle(handles, c, b, prev)
    b.clear()
    b.upload(capi.VEC_W, rc.inputs("arnoldi", c["cplx"])[1])
    b.arnoldi_enqueue(M)
    again = arnoldi_state(capi, b)
    assert _hessenberg_behind(again["H"], 0), name
    fresh, _ = _arnoldi_first(handles, c)
    _same(fresh, again, ARNOLDI_KEYS, "after clear() against a fresh state")
    # and the step behind a restart of the cleared state leaves the coupling alone again
    _arnoldi_cycle(handles, c, b, again)


@pytest.mark.parametrize("name", ["lr-front-k7-s1", "lz-front-k17-s3f"])
def test_clone_of_a_restarted_lanczos_state(handles, name):
    capi = handles.capi
    c = rc.BY_NAME[name]
    prev, b, T = _lanczos_first(handles, c)
    cy, _ = _lanczos_cycle(handles, c, b, prev, T, batches=())  # the restart alone
    twin = handles.register(b.clone())
    restarted = lanczos_state(capi, b)
    _same(restarted, lanczos_state(capi, twin), LANCZOS_KEYS, f"{name}: the clone")
    states = []
    for s in (b, twin):
        rc.enqueue_behind(capi, s, c, rc.batches_behind(c, M - c["nkeep"]), s.lanczos_enqueue)
        states.append(lanczos_state(capi, s))
    _same(states[0], states[1], LANCZOS_KEYS, f"{name}: the steps on the clone")
    cy.update(alpha=states[1]["alpha"], beta=states[1]["beta"], U=states[1]["U"])
    r = rc.check_cycle(c, cy)
    print("RATIO " + rc.line(name + " clone", 1, r))
    assert r["comb"] <= 1.0 and r["kept"].ok() and r["step"].ok(), rc.line(name, 1, r)
    # restart the clone a second time: the original's columns stay
    _lanczos_cycle(handles, c, twin, states[1], rc.next_T(cy), 2)
    _same(states[0], lanczos_state(capi, b), LANCZOS_KEYS, f"{name}: the original after the clone's second restart")


@pytest.mark.parametrize("name", ["ar-default-k7-s1", "az-adaptive-k9-s3"])
def test_clone_of_a_restarted_arnoldi_state(handles, name):
    """keep_coupling travels in Ctrl: the clone's first step leaves the coupling entry as the original's does"""
    capi = handles.capi
    c = rc.BY_NAME[name]
    prev, b = _arnoldi_first(handles, c)
    k, Q, B, _ = handles.solver.krylov_schur_basis(prev["H"][:M], c["nkeep"], prev["residue"])
    b.arnoldi_restart(Q, B)
    twin = handles.register(b.clone())
    _same(arnoldi_state(capi, b), arnoldi_state(capi, twin), ARNOLDI_KEYS, f"{name}: the clone")
    states = []
    for s in (b, twin):
        rc.enqueue_behind(capi, s, c, rc.batches_behind(c, M - k), s.arnoldi_enqueue)
        states.append(arnoldi_state(capi, s))
    _same(states[0], states[1], ARNOLDI_KEYS, f"{name}: the steps on the clone")
    assert states[1]["H"][k, k - 1] == prev["residue"] * Q[M - 1, k - 1] and states[1]["H"][: k + 1, :k].tobytes() == np.asarray(B, states[1]["H"].dtype).tobytes()
    _arnoldi_cycle(handles, c, twin, states[1], 2)
    _same(states[0], arnoldi_state(capi, b), ARNOLDI_KEYS, f"{name}: the original after the clone's second restart")


@pytest.mark.parametrize("name", ["lr-batched-k17-s1", "lz-front-k7-s3u"])
def test_reserve_of_a_restarted_lanczos_state(handles, name):
    """reserve to a larger capacity, then continue: the bits of a state created at that capacity and taken through the same calls"""
    capi = handles.capi
    c = rc.BY_NAME[name]
    big = CAP + 15
    states, cycles = [], []
    for capacity in (CAP, big):
        prev, b, T = _lanczos_first(handles, c, capacity)
        cy, _ = _lanczos_cycle(handles, c, b, prev, T, batches=())
        if capacity != big:
            restarted = lanczos_state(capi, b)
            b.reserve(big)
            _same(restarted, lanczos_state(capi, b), LANCZOS_KEYS, f"{name}: reserve moved the state")
        rc.enqueue_behind(capi, b, c, rc.batches_behind(c, M - c["nkeep"]), b.lanczos_enqueue)
        states.append(lanczos_state(capi, b))
        cycles.append(cy)
    _same(states[0], states[1], LANCZOS_KEYS, f"{name}: reserved against created at {big}")
    cy = cycles[0]
    cy.update(alpha=states[0]["alpha"], beta=states[0]["beta"], U=states[0]["U"])
    r = rc.check_cycle(c, cy)
    print("RATIO " + rc.line(name + " reserved", 1, r))
    assert r["comb"] <= 1.0 and r["kept"].ok() and r["step"].ok(), rc.line(name, 1, r)


@pytest.mark.parametrize("name", ["ar-default-k17-s1", "az-adaptive-k3-s3"])
def test_reserve_of_a_restarted_arnoldi_state(handles, name):
    """the projected matrix moves to a new leading dimension with a full block in it: the same on the old extent, zero beyond
    (seen through the steps that follow, which write the Hessenberg part of their columns only)"""
    capi = handles.capi
    c = rc.BY_NAME[name]
    big = CAP + 15
    states = []
    for capacity in (CAP, big):
        prev, b = _arnoldi_first(handles, c, capacity)
        k, Q, B, _ = handles.solver.krylov_schur_basis(prev["H"][:M], c["nkeep"], prev["residue"])
        b.arnoldi_restart(Q, B)
        if capacity != big:
            restarted = arnoldi_state(capi, b)
            b.reserve(big)
            _same(restarted, arnoldi_state(capi, b), ARNOLDI_KEYS, f"{name}: reserve moved the state")
            reserved = (prev, k, Q, B)
        rc.enqueue_behind(capi, b, c, rc.batches_behind(c, M - k), b.arnoldi_enqueue)
        states.append(arnoldi_state(capi, b))
    _same(states[0], states[1], ARNOLDI_KEYS, f"{name}: reserved against created at {big}")
    prev, k, Q, B = reserved
    H = states[0]["H"]
    assert H[: k + 1, :k].tobytes() == np.asarray(B, H.dtype).tobytes() and _hessenberg_behind(H, k)
    cy = dict(V=prev["U"], k=k, Q=Q, B=B, w0=prev["w"], residue0=prev["residue"], Y=restarted["U"], **{key: states[0][key] for key in ("U", "H", "residue", "w")})
    r = rc.check_cycle(c, cy)
    print("RATIO " + rc.line(name + " reserved", 1, r))
    assert r["comb"] <= 1.0 and r["kept"].ok() and r["step"].ok(), rc.line(name, 1, r)


def test_breakdown_behind_a_restart(handles):
    """a diagonal operator with twelve values on twelve rows (every tile) and a start vector on those rows: 8 calls, a restart
    keeping 3, then 12 calls in one batch.  The state stops with twelve columns, the last beta is at most the threshold (the
    library compares the norm itself: fin_norm_apply), the calls behind the breakdown are no-ops (the columns from twelve on hold
    the sentinel written beforehand; the restart's scratch columns m + 1 .. m + nkeep = 8 .. 10 lie below twelve here and were
    columns again), and a restart of the stopped state is refused and changes nothing."""
    capi = handles.capi
    rows, x = rc.breakdown_inputs()
    ctx = handles.ctx(1)
    op = capi.Csr.upload(ctx, N, *rows)
    try:
        cap, threshold = 24, 1e-12
        b = handles.register(capi.Basis(ctx, op, N, cap))
        b.configure(shift=0.0, threshold=threshold, ortho_mode=capi.ORTHO_BATCHED)
        sentinel = np.full(N, rc.SENTINEL)
        for col in range(cap):
            b.upload(capi.VEC_COL(col), sentinel)
        b.upload(capi.VEC_W, x)
        b.lanczos_enqueue(rc.BREAK_CALLS)
        prev = lanczos_state(capi, b)
        m, k = rc.BREAK_CALLS - 1, rc.BREAK_KEEP
        assert prev["state"] == (m + 1, m, 0)
        theta, S = np.linalg.eigh(kl.restart_T([], [], prev["alpha"], prev["beta"], m))
        S = np.ascontiguousarray(S[:, :k])
        b.lanczos_restart(S, prev["beta"][m - 1] * S[m - 1, k - 1])
        assert lanczos_state(capi, b)["state"] == (k + 1, m, 0)
        b.configure(shift=0.0, threshold=threshold, ortho_mode=capi.ORTHO_BATCHED_TWICE)
        b.lanczos_enqueue(1)
        b.configure(shift=0.0, threshold=threshold, ortho_mode=capi.ORTHO_BATCHED)
        b.lanczos_enqueue(rc.BREAK_BATCH)
        st, alpha, beta = b.lanczos_state()
        print(f"BREAKDOWN nvec {st.nvec} stopped {st.stopped} iterations {st.iterations} nalpha {st.nalpha} nbeta {st.nbeta} last beta {beta[-1]:.3e}")
        assert (st.nvec, st.stopped) == (rc.BREAK_D, 1) and (st.nalpha, st.nbeta) == (rc.BREAK_D, rc.BREAK_D)
        assert beta[-1] <= threshold and beta[k:-1].min() > 1e-3
        got = lanczos_state(capi, b)
        U = got["U"]
        assert np.abs(U @ U.T - np.eye(rc.BREAK_D)).max() <= (N + rc.BREAK_D) * kl.EPS
        assert not np.delete(U, rc.BREAK_ROWS, axis=1).any()  # the space of the twelve rows
        for col in range(rc.BREAK_D, cap):
            assert np.array_equal(b.download(capi.VEC_COL(col)), sentinel), f"column {col} was written behind the breakdown"
        Sf = np.asfortranarray(S)
        rcode = capi.lib().eigenex_lanczos_restart(b.h, k, Sf.ctypes.data_as(capi._dp), m, 0.25)
        assert rcode == ERR_STATE
        _same(got, lanczos_state(capi, b), LANCZOS_KEYS, "a refused restart")
    finally:
        handles.close_bases()
        op.close()
