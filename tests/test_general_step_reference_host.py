"""The cases of tests/general_step_cases.py on the host: what makes the assertion of tests/test_gpu_general_step_passes.py fair, and
what shows that it can fail.  No GPU, no library.

For every case the fp64 recurrence of tests/krylov_local_reference.py (lanczos_general_fp64, arnoldi_general_fp64: the general
column set, the orthogonalizing vectors, the scheme, the deflated start vector) passes the general local check at a ratio of at
most 0.1, orthogonality included where the scheme promises it.  An input on which it comes nearer would be replaced, not tolerated.

For every fault that applies to a case (general_step_cases.applicable_faults) the faulty fp64 state fails the check at a ratio of
at least 100; every fault of kl.FAULTS is caught by at least one case and no case is without a fault.

The adaptive Arnoldi cases that are there for the decision hold, by the extended-precision ratios |r_1|^2 / |hu|^2, at least two
steps whose second pass runs and two whose does not, none within 1e-3 of 0.5.  (The two adaptive chunk cases are there for the
launches of a chunked second pass: with a thousand orthonormal vectors in the set the second pass runs on every step.)

The restated selection rule is held against a plain transcription of the library's arithmetic, and the general check against
check_lanczos / check_arnoldi where both apply.  Measured ratios: profiles/general_step_passes.md."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import general_step_cases as gc  # noqa: E402
import krylov_local_reference as kl  # noqa: E402

ROOM = 0.1    # a reference recurrence that uses more than a tenth of the bound means another input
CAUGHT = 100  # a fault must be this far outside the bound on at least one step
_REFS = {}


def _reference(name):
    if name not in _REFS:
        _REFS[name] = gc.reference(gc.BY_NAME[name])
    return _REFS[name]


def _calls_made(c, st):
    return st["U"].shape[0] == c["calls"]


@pytest.mark.parametrize("name", list(gc.BY_NAME))
def test_fp64_recurrence_passes_with_room(name):
    c = gc.BY_NAME[name]
    rep, st = _reference(name)
    print(rep.line(name))
    print(f"HOST RATIO {name} {rep.ratio():.3e} steps {rep['step_ratio']:.3e} start {rep['start_ratio']:.3e} ortho {rep['ortho'] / rep['ortho_bound']:.3e}")
    assert _calls_made(c, st), (name, st["U"].shape)
    assert len(rep["steps"]) == c["calls"]
    assert rep.ok() and rep.ratio() <= ROOM and rep["ortho"] <= ROOM * rep["ortho_bound"], rep.line(name)
    assert c["nq"] == 0 or rep["start_bound"] > 0.0  # column 0 was checked


PAIRS = [(c["name"], f) for c in gc.CASES for f in c["faults"]]


@pytest.mark.parametrize("name,fault", PAIRS, ids=[f"{n}-{f}" for n, f in PAIRS])
def test_fault_is_caught(name, fault):
    c = gc.BY_NAME[name]
    rep, st = gc.reference(c, fault)
    print(rep.line(f"{name} with {fault}"))
    print(f"FAULT RATIO {name} {fault} {rep.ratio():.3e}")
    assert rep.ratio() >= CAUGHT and not rep.ok(), rep.line(f"{name} with {fault}")


def test_every_fault_has_a_case_and_every_case_a_fault():
    assert {f for c in gc.CASES for f in c["faults"]} == set(kl.FAULTS)
    assert all(c["faults"] for c in gc.CASES), [c["name"] for c in gc.CASES if not c["faults"]]
    assert all(set(c["faults"]) <= set(kl.FAULTS) for c in gc.CASES)


ADAPTIVE = [c["name"] for c in gc.CASES if c["kind"] == "arnoldi" and c["mode"] == "ORTHO_BATCHED_ADAPTIVE" and not c["budget"]]


@pytest.mark.parametrize("name", ADAPTIVE)
def test_adaptive_cases_hold_both_outcomes_clear_of_the_threshold(name):
    rep, _ = _reference(name)
    d = np.array(rep["decisions"], np.float64)
    print(f"{name}: |r_1|^2 / |hu|^2 per step {np.array2string(d, precision=4)}")
    assert d.size == gc.BY_NAME[name]["calls"] == gc.CALLS_ADAPTIVE
    assert np.count_nonzero(d < kl.ETA2) >= 2 and np.count_nonzero(d > kl.ETA2) >= 2
    assert np.abs(d - kl.ETA2).min() > 1e-3
    assert np.count_nonzero((d > 0.25) & (d < kl.ETA2)) >= 1  # a decision taken with 0.25 would differ


def test_the_table_holds_the_required_axes():
    """every value of every axis the suite is built on occurs, the pairs the device paths need included"""
    cs = gc.CASES
    have = lambda **kw: any(all(c[k] == v for k, v in kw.items()) for c in cs)  # noqa: E731
    for kind, op in (("lanczos", "sym"), ("lanczos", "herm"), ("arnoldi", "gen"), ("arnoldi", "zgen")):
        for mode in gc.MODES:
            assert have(kind=kind, mode=mode) and have(kind=kind, op=op), (kind, op, mode)
    for interval, nq in ((1, 2), (2, 0), (3, 2), (5, 3), (0, 2)):
        assert have(kind="lanczos", interval=interval, nq=nq, shards=1), (interval, nq)
    assert have(kind="lanczos", interval=2, nq=0, calls=gc.CALLS_GAP) and have(interval=3, calls=gc.CALLS_GAP) and have(interval=5, calls=gc.CALLS_GAP)
    for nq in (0, 2):
        assert have(kind="arnoldi", nq=nq)
    for q in ("orth", "skew"):
        assert have(kind="lanczos", q=q) and have(kind="arnoldi", q=q)
    for mode in ("ORTHO_BATCHED", "ORTHO_BATCHED_TWICE"):
        for fusion in (True, False):
            assert have(kind="lanczos", shards=3, mode=mode, fusion=fusion), (mode, fusion)
    assert have(kind="arnoldi", shards=3) and have(kind="arnoldi", shards=3, mode="ORTHO_BATCHED_ADAPTIVE")
    for layout in ("plain", "auto"):
        assert have(kind="lanczos", op="sym", shards=1, layout=layout) and have(kind="arnoldi", op="gen", shards=1, layout=layout)
    assert have(split=gc.SPLIT, kind="lanczos") and have(split=gc.SPLIT, kind="arnoldi")
    for c in cs:
        if c["budget"]:
            assert c["q"] == "orth" and c["n"] >= c["nq"] + 16 and c["budget"] < c["nq"] + c["calls"], c["name"]


def _c_lanczos_columns(k, interval, nq_total):
    """library.hip, lanczos_columns, line by line"""
    first = stride = count = nq = 0
    if interval <= 0:
        return first, 1, count, nq
    nk = k + 2
    kmod = (nk - 1) % interval
    first, stride = kmod, min(interval, 1 << 30)
    count = (nk - 1 - kmod + interval - 1) // interval if kmod < nk - 1 else 0
    nq = nq_total if kmod == 0 else 0
    return first, stride, count, nq


def test_lanczos_columns_restates_the_library_rule():
    for interval in (-1, 0, 1, 2, 3, 5, 7, 40):
        for k in range(30):
            first, stride, count, nq = _c_lanczos_columns(k, interval, 3)
            cols, nqu = kl.lanczos_columns(k, interval, 3)
            assert cols == [first + i * stride for i in range(count)] and nqu == nq, (interval, k)
            assert all(0 <= c <= k for c in cols)
    assert kl.lanczos_columns(4, 5, 3) == ([0], 3) and kl.lanczos_columns(3, 5, 3) == ([], 0)  # k = 3: kmod 4 > k, nothing
    assert kl.lanczos_columns(5, 3, 2) == ([0, 3], 2) and kl.lanczos_columns(6, 3, 2) == ([1, 4], 0)


def test_general_check_agrees_with_the_existing_one():
    """interval 1, no orthogonalizing vector, batched, on the states of the existing recurrences: the same orthogonality, a bound
    that is the existing one (with nq = 0) times max(1, sum |c_i| / |w0|) <= sqrt(S), and errors that differ from those of
    check_lanczos / check_arnoldi by less than a tenth of the bound (Lanczos: the general check removes the recurrence with the
    recorded coefficients first; Arnoldi: the same arithmetic, the same errors)"""
    def close(new, old, key, i):
        assert abs(max(s[i] for s in new["steps"]) - old[key]) <= ROOM * old["bound"], (key, new.line(), old.line())

    for op, n in (("sym", 300), ("herm", 200)):
        rows, x = gc.rows(op, n), gc.start(op, n)
        a, b, V = kl.lanczos_fp64(kl.csr_matmul(rows), x, 7, -0.3)
        old, new = kl.check_lanczos(rows, -0.3, V, a, b), kl.check_lanczos_general(rows, -0.3, V, None, a, b, x0=x, orthonormal=True)
        assert old.ok() and new.ok() and new.ratio() <= ROOM and new["ortho"] == old["ortho"] and new["ortho_bound"] == old["ortho_bound"]
        for key, i in (("err_diag", 1), ("err_norm", 2), ("err_vec", 3)):
            close(new, old, key, i)
        assert all(old["bound"] <= s[4] <= old["bound"] * np.sqrt(max(s[5], 1)) * (1 + 1e-6) for s in new["steps"])
    for op, n, shift in (("gen", 300, -0.37), ("zgen", 200, 0.3 - 0.2j)):
        rows, x = gc.rows(op, n), gc.start(op, n)
        for passes, mode in ((1, kl.BATCHED), (2, kl.TWICE)):
            V, H, residue, w = kl.arnoldi_fp64(kl.csr_matmul(rows), x, 8, shift, passes)
            old, new = kl.check_arnoldi(rows, shift, V, H, residue, w), kl.check_arnoldi_general(rows, shift, V, None, H, residue, w, mode, x, True)
            assert old.ok() and new.ok() and new.ratio() <= ROOM and new["ortho"] == old["ortho"]
            for key, i in (("err_diag", 1), ("err_norm", 2), ("err_vec", 3)):
                close(new, old, key, i)
            if passes == 1:
                assert [max(s[i] for s in new["steps"]) for i in (1, 2, 3)] == [old["err_diag"], old["err_norm"], old["err_vec"]]
            assert all(old["bound"] <= s[4] <= old["bound"] * np.sqrt(max(s[5], 1)) * (2 if passes == 2 else 1) * (1 + 1e-6) for s in new["steps"])


def test_skewed_vectors_overlap_by_three_tenths():
    for op, n in (("sym", gc.N), ("herm", gc.NZ)):
        for q, off in (("skew", 0.3), ("orth", 0.0)):
            Q = gc.ortho_vectors(op, n, 3, q)
            G = Q.conj() @ Q.T
            assert np.abs(np.diag(G) - 1.0).max() < 1e-13 and np.abs(np.abs(G - np.diag(np.diag(G))) - off * (1 - np.eye(3))).max() < 1e-13
