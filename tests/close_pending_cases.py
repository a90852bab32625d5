"""Lanczos runs through the C ABI around batch ends of the one-sweep step, written to one .npz -- the child process of
tests/test_gpu_close_pending.py.

    python -m tests.close_pending_cases OUT.npz

A batch of one-sweep steps leaves its newest column to be written by whatever needs it next (eigenex_basis_close_pending).  The
library reads EIGENEX_EAGER_CLOSE and EIGENEX_NO_GRAPHS once per process, so one configuration is one process.  Every scenario
stores what its reader returned and the final state (alpha, beta, state fields with the repair counter, all columns, W) under
"<case>/<scenario>/<key>".  Importable without a GPU.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import one_sweep_cases as osc  # noqa: E402
from tests import sweep_bits_cases as sbc  # noqa: E402

NCALLS = 16
EXTRA = 8  # free columns: the scratch of a thick restart, room for the steps behind it
# name -> (operator, one workgroup per CU).  laplacian3d(17): 4913 rows = two full 2048-row tiles + 817 rows, row codes and inline
# finalisers; the tridiagonal operators of sweep_bits_cases: plain CSR, a tile of one row, an exact second tile + one row
CASES = {
    "lap17": (("lap", 17), False),
    "lap17_per_cu": (("lap", 17), True),
    "tri2049": sbc.CASES["tri2049"][0::2],
    "tri4097": sbc.CASES["tri4097"][0::2],
}
SCHEDULES = {"whole": [NCALLS], "ones": [1] * NCALLS, "mixed": osc.schedules(NCALLS)["mixed"]}
HEAD, TAIL = (5, 1, 2), (1, 4, 3)  # batches in front of a reader (the last one leaves the close pending) and behind it
assert sum(HEAD) + sum(TAIL) == NCALLS
READERS = ("download", "dots", "ritz", "clone", "reserve", "update", "restart", "configure", "clear")
CONFIGS = (("default", {}), ("eager", {"EIGENEX_EAGER_CLOSE": "1"}), ("no_graphs", {"EIGENEX_NO_GRAPHS": "1"}))
GUARD_CALLS = 21


def snapshot(b, out, key):
    from cmpt_eigenex_amd import capi

    st, alpha, beta = b.lanczos_state()
    out[key + "alpha"], out[key + "beta"] = alpha, beta
    out[key + "state"] = np.array([st.nvec, st.iterations, st.nalpha, st.nbeta, st.stopped, st.calls_true, b.repairs()], np.int64)
    out[key + "V"] = np.stack([b.download(capi.VEC_COL(c)) for c in range(st.nvec)])
    out[key + "W"] = b.download(capi.VEC_W)


def make(ctx, case):
    from tests import one_sweep_reference as osr
    from cmpt_eigenex_amd import capi

    (kind, size), per_cu = CASES[case]
    if kind == "lap":
        n, A = size ** 3, capi.Csr.laplacian3d(ctx, size)
    else:
        n, A = size, capi.Csr.upload(ctx, size, *osr.tridiagonal_csr(size), column_blocks=0)

    def state():
        b = capi.Basis(ctx, A, n, NCALLS + 1 + EXTRA)
        if per_cu:
            b.tune(1, 4, 0)
        b.upload(capi.VEC_W, osc.start(n))
        return b

    return n, A, state


def fixed_matrix(rows, cols, seed):
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((rows, cols)))
    return np.asfortranarray(q)


def run_reader(reader, b, n, out, key):
    """`b` has a close pending behind HEAD; returns the states to continue (and to snapshot in the end)"""
    from cmpt_eigenex_amd import capi

    nvec = sum(HEAD)
    states = [b]
    if reader == "download":
        out[key + "result"] = b.download(capi.VEC_COL(nvec - 1))
    elif reader == "dots":
        out[key + "result"] = b.dots(capi.VEC_W, 0, 1, nvec)
    elif reader == "ritz":
        out[key + "result"] = b.ritz_vectors(nvec, fixed_matrix(nvec, 3, 5))
    elif reader == "clone":
        states.append(b.clone())
    elif reader == "reserve":
        b.reserve(b.capacity + 7)
    elif reader == "update":
        h = 1e-3 * np.random.default_rng(7).standard_normal(nvec)
        out[key + "result"] = np.array(b.update(capi.VEC_W, 0, 1, nvec, h))
    elif reader == "restart":
        b.lanczos_restart(fixed_matrix(nvec - 1, 2, 9), 0.25)
    elif reader == "configure":
        b.configure(interval=2)  # the next step is a two-sweep step
    elif reader == "clear":
        b.clear()
        b.upload(capi.VEC_W, osc.start(n))
        for k in HEAD:
            b.lanczos_enqueue(k)
    else:
        raise ValueError(reader)
    return states


def run_case(ctx, case, out):
    n, A, state = make(ctx, case)
    for sched, batches in SCHEDULES.items():
        b = state()
        for k in batches:
            b.lanczos_enqueue(k)
        snapshot(b, out, "%s/sched_%s/" % (case, sched))
        b.close()
    for reader in READERS:
        key = "%s/read_%s/" % (case, reader)
        b = state()
        for k in HEAD:
            b.lanczos_enqueue(k)
        out[key + "pending_before"] = np.array(b.close_pending())
        states = run_reader(reader, b, n, out, key)
        out[key + "pending_after"] = np.array([s.close_pending() for s in states])
        for i, s in enumerate(states):
            for k in TAIL:
                s.lanczos_enqueue(k)
            snapshot(s, out, key + ("" if i == 0 else "copy_"))
            s.close()
    A.close()


def run_bytes(ctx, case, out):
    """one-call batches with the context's profile on (no recorded graphs then): bytes booked under K_UPDATE, the flag"""
    from cmpt_eigenex_amd import capi

    n, A, state = make(ctx, case)
    b = state()
    b.lanczos_enqueue(1)  # the start vector and alpha_0: no sweep yet
    ctx.profile_enable(True)
    ctx.profile_reset()
    flags = []
    s = 6
    for _ in range(s):
        b.lanczos_enqueue(1)
        flags.append(b.close_pending())
    b.lanczos_state()
    key = case + "/bytes/"
    out[key + "update_bytes"] = np.array(ctx.profile_get(capi.K_UPDATE)[2])
    out[key + "pending_after_batch"] = np.array(flags)
    out[key + "n_steps"] = np.array([n, s], np.int64)
    b.download(capi.VEC_COL(s))
    out[key + "pending_after_download"] = np.array(b.close_pending())
    out[key + "update_bytes_after_download"] = np.array(ctx.profile_get(capi.K_UPDATE)[2])
    ctx.profile_enable(False)
    b.close()
    A.close()


def run_graphs(ctx, case, out):
    """the same batches of >= 4 calls three times from the same state, a clear in between: recorded once, replayed twice"""
    from cmpt_eigenex_amd import capi

    n, A, state = make(ctx, case)
    b = state()
    for rep in range(3):
        if rep:
            b.clear()
            b.upload(capi.VEC_W, osc.start(n))
        for k in (5, 4, 7):
            b.lanczos_enqueue(k)
        snapshot(b, out, "%s/graphs_%d/" % (case, rep))
    out[case + "/graphs/count"] = np.array(b.graph_info()["graphs"])
    b.close()
    A.close()


def guard_operator(ctx):
    from tests import one_sweep_reference as osr
    from cmpt_eigenex_amd import capi

    n = 60
    A = capi.Csr.upload(ctx, n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), 1.0 + np.arange(n), column_blocks=0)
    return n, A, osr.guard_start(n, 1e-11)


def run_guard(ctx, out):
    """diag(1..60), five entries 1 and the rest 1e-11: a lagged coefficient leaves the guard's bound and a repair is armed.  One
    call per batch finds the call that armed it; then a batch is cut right behind that call."""
    from cmpt_eigenex_amd import capi

    n, A, x = guard_operator(ctx)

    def state():
        b = capi.Basis(ctx, A, n, GUARD_CALLS + 1)
        b.upload(capi.VEC_W, x)
        return b

    b = state()
    armed = -1
    for i in range(GUARD_CALLS):
        b.lanczos_enqueue(1)
        if armed < 0 and b.repairs() > 0:
            armed = i + 1  # calls made when the counter first moved
    snapshot(b, out, "guard/ones/")
    b.close()
    out["guard/armed_after_calls"] = np.array(armed)
    if 0 < armed < GUARD_CALLS:
        b = state()
        b.lanczos_enqueue(armed)
        out["guard/cut/pending"] = np.array(b.close_pending())
        out["guard/cut/repairs_at_cut"] = np.array(b.repairs())
        b.lanczos_enqueue(GUARD_CALLS - armed)
        snapshot(b, out, "guard/cut/")
        b.close()
    b = state()
    b.lanczos_enqueue(GUARD_CALLS)
    snapshot(b, out, "guard/whole/")
    b.close()
    A.close()


def run_config(name, out_path, timeout=300):
    """one configuration in a child process of its own -> {key: array}; raises RuntimeError if the child did not end normally"""
    import subprocess

    env = {k: v for k, v in os.environ.items() if not k.startswith("EIGENEX_")}
    env.update(dict(CONFIGS)[name])
    try:
        r = subprocess.run([sys.executable, "-m", "tests.close_pending_cases", out_path], cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as e:
        raise RuntimeError("%s: timed out\n%s" % (name, (e.stderr or b"")[-4000:]))
    if r.returncode != 0:
        raise RuntimeError("%s: exit status %d\n%s" % (name, r.returncode, r.stderr[-4000:]))
    with np.load(out_path) as z:
        return {k: z[k] for k in z.files}


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    from cmpt_eigenex_amd import capi

    ctx = capi.Context()
    out = {}
    for case in CASES:
        run_case(ctx, case, out)
        run_graphs(ctx, case, out)
    run_guard(ctx, out)
    run_bytes(ctx, "lap17", out)  # last: the profile stays off for everything above
    ctx.close()
    tmp = argv[0] + ".part.npz"
    np.savez(tmp, **out)
    os.replace(tmp, argv[0])
    print("%d cases -> %s" % (len(CASES), argv[0]))


if __name__ == "__main__":
    main()
