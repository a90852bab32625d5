"""The fused step finalisers against their separate-launch forms, bit for bit.

One shard with a plain CSR operator folds a step's small finalising launches into its big kernels: Lanczos takes alpha in k_dots
and beta, the breakdown test and the scale in k_spmv (InlineFin); the adaptive Arnoldi scheme takes the second-pass decision in
that pass's k_dots (InlineDecide), its second-stage sums in k_update (InlineReduce), and the start and the (deferred) end of a
step in the next operator kernel (InlineArnoldiBegin).  EIGENEX_NO_INLINE_FIN=1 restores k_reduce_fin, k_fin_norm,
k_reduce_decide, k_arnoldi_begin and k_arnoldi_tail, EIGENEX_NO_GRAPHS=1 plain launches instead of recorded step batches.
Both switches promise the same numbers, i.e. the same sums in the same order and the same decisions, so the
four combinations are compared with np.array_equal -- a tolerance against the fp64 oracle cannot see a dropped partial sum or
a different association.  The default configuration is anchored to the oracle as well, so that "all four agree" also means
"all four are right".  EIGENEX_DOTS_RED4=0 (the other k_dots reduction) is checked against a high-precision reference of the
same dot products.

The library reads the switches once per process: every configuration runs tests/variant_cases.py in a child process of its
own, one after the other, each once per session.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import variant_cases as vc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = (  # name, environment, case patterns (None: every case)
    ("default", {}, None),
    ("no_inline_fin", {"EIGENEX_NO_INLINE_FIN": "1"}, None),
    ("no_graphs", {"EIGENEX_NO_GRAPHS": "1"}, None),
    ("no_inline_fin_no_graphs", {"EIGENEX_NO_INLINE_FIN": "1", "EIGENEX_NO_GRAPHS": "1"}, None),
    ("dots_red4_off", {"EIGENEX_DOTS_RED4": "0"}, ["prim-*"]),
)
BITWISE = [c[0] for c in CONFIGS[:4]]
CHILD_TIMEOUT = 900


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """config name -> {key: array}.  Configurations run one after the other; after a child that did not exit normally no
    further child is started (the tests that need the missing results fail with the first child's error)."""
    d = tmp_path_factory.mktemp("variants")
    res, failure = {}, None
    for name, extra, only in CONFIGS:
        if failure:
            break
        env = {k: v for k, v in os.environ.items() if not k.startswith("EIGENEX_")}
        env.update(extra)
        out = str(d / (name + ".npz"))
        cmd = [sys.executable, "-m", "tests.variant_cases", out] + (["--only"] + only if only else [])
        try:
            r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired as e:
            failure = "%s: timed out after %d s\n%s" % (name, CHILD_TIMEOUT, (e.stderr or b"")[-4000:])
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


def _case_keys(data, case):
    return sorted(k for k in data if k.startswith(case + "/"))


def test_every_configuration_ran(runs):
    _need(runs, *[c[0] for c in CONFIGS])
    assert list(runs["default"]["_cases"]) == vc.all_case_names()


@pytest.mark.parametrize("case", vc.all_case_names())
def test_same_bits_with_and_without_inline_finalisers_and_graphs(runs, case):
    """every observable -- alpha/beta or H, state, residue, basis columns, Ritz vectors -- identical in all four configurations"""
    data = _need(runs, *BITWISE)
    keys = _case_keys(data[0], case)
    assert keys
    for name, d in zip(BITWISE[1:], data[1:]):
        assert _case_keys(d, case) == keys, name
        for k in keys:
            if k.endswith("/graphs"):
                continue  # what differs on purpose: the number of recorded batches
            assert data[0][k].shape == d[k].shape and np.array_equal(data[0][k], d[k]), (
                "%s differs under %s: max |diff| %s" % (k, name, _maxdiff(data[0][k], d[k])))


def _maxdiff(a, b):
    try:
        return float(np.abs(a.astype(np.complex128) - b.astype(np.complex128)).max()) if a.shape == b.shape else "shape %s/%s" % (a.shape, b.shape)
    except (TypeError, ValueError):
        return "n/a"


@pytest.mark.parametrize("base", list(vc.SOLVER_CASES))
def test_batch_schedules_and_replay_give_the_same_bits(runs, base):
    """one batch (recorded as a graph, then replayed), one call per batch, mixed batches: a step's end taken by the last call of
    its batch or deferred to the next call's operator kernel, alpha closed at the batch end or taken by the next dots -- same bits"""
    data = _need(runs, *BITWISE)
    for name, d in zip(BITWISE, data):
        ref = {k.split("/", 1)[1]: v for k, v in d.items() if k.startswith(base + "-whole/")}
        for k in [k for k in ref if k.endswith("_again")]:
            assert np.array_equal(ref[k], ref[k[: -len("_again")]]), "%s: %s second run differs (%s)" % (name, k, base)
        for sched in ("single", "mixed"):
            other = {k.split("/", 1)[1]: v for k, v in d.items() if k.startswith(base + "-" + sched + "/")}
            for k, v in other.items():
                if k == "graphs":
                    continue
                assert np.array_equal(ref[k], v), "%s: %s differs between schedules whole and %s (%s): %s" % (
                    name, k, sched, base, _maxdiff(ref[k], v))


@pytest.mark.parametrize("base", list(vc.SOLVER_CASES))
def test_cases_reach_their_paths(runs, base):
    """the layout each case is meant to cover, and recorded step graphs exactly where they are expected"""
    default, nog = _need(runs, "default", "no_graphs")
    cs = vc.SOLVER_CASES[base]
    for sched in vc.SCHEDULES:
        case = "%s-%s" % (base, sched)
        assert str(default[case + "/layout"]) == cs["layout"], case
        assert int(nog[case + "/graphs"]) == 0
        if sched == "single":
            assert int(default[case + "/graphs"]) == 0
        elif sched == "whole":
            assert int(default[case + "/graphs"]) == 1
        else:
            assert int(default[case + "/graphs"]) >= 1
    if base == "lz_big" or base == "ar_big":
        n = 85 ** 3
        assert (n + 2047) // 2048 > 256  # vector kernels: one workgroup per 2048-row tile, more tiles than 256 (strided sums)
    st = dict(zip(vc.STATE_FIELDS, default[base + "-whole/state"]))
    if base == "lz_breakdown":
        assert st["stopped"] == 1 and st["calls_true"] == 5 and st["nvec"] == 5
    if base in ("lz_full", "ar_full"):
        assert st["stopped"] == 1 and st["nvec"] == 40
    if base == "ar_cap":
        assert st["stopped"] == 0 and st["nvec"] == cs["cap"]
    if base == "ar_defl":
        assert (st["nvec"] + cs["nq"]) > 4096  # coefficients per step beyond kInlineReduceMaxCoef


@pytest.mark.parametrize("base", [b for b, c in vc.SOLVER_CASES.items() if not c["cplx"] and b != "ar_dgks"])
def test_default_configuration_matches_the_oracle(runs, base):
    """the C restatement of the reference's step loops (oracle/krylov_ref.c) at the suite's tolerances"""
    from oracle import cref

    (d,) = _need(runs, "default")
    cs = vc.SOLVER_CASES[base]
    rp, cl, vl, init, Q = vc.case_inputs(base)
    m = cs["m"]
    key = base + "-whole/"
    st = dict(zip(vc.STATE_FIELDS, d[key + "state"]))
    Qs = list(Q) if cs["nq"] else None
    if cs["kind"] == "lanczos":
        ref = cref.CLanczos(rp, cl, vl, init, cap=m + 1, shift=cs["shift"], Q=Qs, nthreads=4)
        ok = ref.run(m)
        assert st["calls_true"] == ok and st["stopped"] == int(ok < m)
        assert (st["nvec"], st["nalpha"], st["iterations"]) == (ref.nvec, ref.alpha.size, ref.iterations)
        beta = d[key + "beta"]
        if ref.nvec == rp.size - 1 and ref.beta[-1] > 1e-12:
            # full Krylov space: the oracle's driver stops in front of the next call (lanczosStepIsUtmost, lanczos.hpp:331-347),
            # updateLanczosSteps itself -- what lanczos_enqueue runs -- makes that call, records beta (rounding level) and breaks down
            assert beta.size == ref.beta.size + 1 and beta[-1] <= 1e-12
            beta = beta[:-1]
        assert d[key + "alpha"].shape == ref.alpha.shape and beta.shape == ref.beta.shape
        tol = 1e-11 if rp.size < 100_000 else 1e-10
        np.testing.assert_allclose(d[key + "alpha"], ref.alpha, rtol=0, atol=tol)
        np.testing.assert_allclose(beta, ref.beta, rtol=0, atol=tol)
    else:
        ref = cref.CArnoldi(rp, cl, vl, init, cap=m + 1, shift=cs["shift"], Q=Qs, nthreads=4)
        ok = ref.run(m)
        assert st["calls_true"] == ok and st["stopped"] == int(ok < m)
        assert (st["nvec"], st["iterations"]) == (ref.nvec, ref.iterations)
        H, H_ref = d[key + "H"], ref.hessenberg()
        assert H.shape == H_ref.shape
        scale = max(1.0, np.abs(H_ref).max())
        np.testing.assert_allclose(H, H_ref, rtol=0, atol=1e-10 * scale)
        assert abs(d[key + "residue"][0] - ref.residue) <= 1e-10 * scale


def test_dgks_case_keeps_orthogonality_and_the_top_ritz_value(runs):
    """ar_dgks runs the adaptive scheme past convergence, where it departs from the reference's single pass on purpose
    (test_arnoldi_orthogonality_when_ritz_values_converge): anchored by orthogonality and the exact top eigenvalue"""
    (d,) = _need(runs, "default")
    n = vc.SOLVER_CASES["ar_dgks"]["op"][1]
    V = d["ar_dgks-whole/V"]
    assert np.abs(V @ V.T - np.eye(V.shape[0])).max() < 1e-13
    lam_max = 3 * (2 - 2 * np.cos(n * np.pi / (n + 1)))
    ev = np.linalg.eigvals(d["ar_dgks-whole/H"])
    assert abs(ev.real.max() - lam_max) < 1e-10 and np.abs(ev.imag).max() < 1e-8


def _dots_exact(M, w):
    """conj(M) @ w in long double (each fp64 product is exact to far below the bound)"""
    Mr, Mi = M.real.astype(np.longdouble), (M.imag if np.iscomplexobj(M) else np.zeros_like(M.real)).astype(np.longdouble)
    wr, wi = w.real.astype(np.longdouble), (w.imag if np.iscomplexobj(w) else np.zeros_like(w.real)).astype(np.longdouble)
    re = Mr @ wr + Mi @ wi
    im = Mr @ wi - Mi @ wr
    return re.astype(np.float64) + 1j * im.astype(np.float64)


@pytest.mark.parametrize("case", list(vc.PRIM_CASES))
def test_dots_both_reductions_against_a_high_precision_reference(runs, case):
    """k_dots<C, R, D> with R = true (default) and R = false (EIGENEX_DOTS_RED4=0): |h - h_exact| <= 1e-13 ||m|| ||w||"""
    d, d0 = _need(runs, "default", "dots_red4_off")
    M, w = vc.prim_inputs(case)
    exact = _dots_exact(M, w)
    bound = 1e-13 * np.linalg.norm(M, axis=1) * np.linalg.norm(w)
    for name, data in (("default", d), ("dots_red4_off", d0)):
        h = data[case + "/h"]
        assert h.shape == (M.shape[0],)
        err = np.abs(h - exact)
        assert np.all(err <= bound), "%s: worst error / bound %.3g" % (name, (err / bound).max())
