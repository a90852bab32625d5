"""The periodic spin-1/2 Heisenberg ring in momentum sectors of 64-bit states (eigenex_spin_momentum64_upload / _z), cell = 1.
Every step is a process of its own under a time limit of its own; the driver stops at the first step that fails.
  word32    (32,16), k = 0, real: upload time of both handles (enumeration included) and the time of one application on the
            32-bit and on the 64-bit handle in one process, alternating: the cost of the 64-bit word
  apply36   (36,18): upload time and time of one application at m = 0 (real), m = 18 (real) and m = 1 (complex)
  lanczos36 (36,18), m = 0, real states: Lanczos iterations per second at --m steps (the complex basis of m = 1, 4 GB a vector,
            is not run), then one eigenex_spin_momentum_measure of all 36 + 630 site and pair masks
  ground36  (36,18), k = 0: the lowest level after --ground-steps Lanczos steps, its energy per site and <Sz_0 Sz_r>
Times per application come from the library's own per-kernel profile (HIP events around every launch of eigenex_apply) after three
warm-up applications.  Lanczos, measure and upload: host clock around calls that end in a synchronise.
usage: python scripts/probe_spin_momentum64.py [--steps word32 apply36 lanczos36 ground36] [--m 50] [--ground-steps 90]
                                               [--applies 10] [--repeats 3] [--limit 600]"""
import argparse
import subprocess
import sys
import time

sys.path.insert(0, ".")

STEPS = ("word32", "apply36", "lanczos36", "ground36")
ap = argparse.ArgumentParser()
ap.add_argument("--steps", nargs="+", default=list(STEPS), choices=STEPS)
ap.add_argument("--step", choices=STEPS, help="run this one step in this process")
ap.add_argument("--m", type=int, default=50)
ap.add_argument("--ground-steps", type=int, default=90)
ap.add_argument("--applies", type=int, default=10)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--limit", type=float, default=600.0, help="seconds for each step")
ap.add_argument("--sites", type=int, default=36, help="the ring of the 36-site steps (a smaller one for a trial run)")
args = ap.parse_args()

if args.step is None:
    for step in args.steps:
        cmd = [sys.executable, sys.argv[0], "--step", step, "--m", str(args.m), "--ground-steps", str(args.ground_steps), "--applies", str(args.applies),
               "--repeats", str(args.repeats), "--sites", str(args.sites)]
        try:
            rc = subprocess.run(cmd, timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f"step {step} ended with status {rc}: nothing more is run", flush=True)
            sys.exit(rc)
    sys.exit(0)

import numpy as np  # noqa: E402

from cmpt_eigenex_amd import capi, solver  # noqa: E402

ctx = capi.Context()
L = args.sites


def ring(n):
    return [(i, (i + 1) % n, 1.0, 1.0) for i in range(n)]


def upload(make, n_sites, n_up, m, cplx, label):
    t0 = time.perf_counter()
    op = make(ctx, n_sites, n_up, m, ring(n_sites), complex_states=cplx)
    dt = time.perf_counter() - t0
    n = op.info()["n_global"]
    print(f"({n_sites},{n_up}) m={m} {label}: {n} rows, vector {8 * n * (2 if cplx else 1) / 1e9:.3f} GB, upload {dt:.2f} s (enumeration included)", flush=True)
    return op, n


def apply_time(b, count):
    """us per application from the profile of `count` applications"""
    ctx.profile_reset()
    ctx.profile_enable(True)
    for _ in range(count):
        b.apply(capi.VEC_COL(0), capi.VEC_V)
    launches, ms, by = ctx.profile_get(capi.K_SPMV)
    ctx.profile_enable(False)
    return ms * 1e3 / count


def state(op, n, columns=2):
    b = capi.Basis(ctx, op, n, columns)
    b.random_signs(capi.VEC_START, 1, 0)
    b.copy(capi.VEC_COL(0), capi.VEC_START)
    return b


if args.step == "word32":
    forms = {"32-bit": upload(capi.Csr.spin_half_momentum, 32, 16, 0, False, "32-bit"), "64-bit": upload(capi.Csr.spin_half_momentum64, 32, 16, 0, False, "64-bit")}
    states = {k: state(op, n) for k, (op, n) in forms.items()}
    for b in states.values():
        apply_time(b, 3)
    for rep in range(args.repeats):
        for name, b in states.items():
            us = apply_time(b, args.applies)
            print(f"(32,16) rep {rep} {name} apply: {us:11.1f} us = {us * 1e3 / forms[name][1]:8.4f} ns/row", flush=True)
elif args.step == "apply36":
    for m, cplx in ((0, False), (L // 2, False), (1, True)):
        op, n = upload(capi.Csr.spin_half_momentum64, L, L // 2, m, cplx, "complex" if cplx else "real")
        b = state(op, n)
        apply_time(b, 3)
        for rep in range(args.repeats):
            us = apply_time(b, args.applies)
            print(f"({L},{L // 2}) m={m} rep {rep} apply: {us:11.1f} us = {us * 1e3 / n:8.4f} ns/row", flush=True)
        b.close()
        op.close()
elif args.step == "lanczos36":
    op, n = upload(capi.Csr.spin_half_momentum64, L, L // 2, 0, False, "real")
    b = state(op, n, args.m + 2)
    for rep in range(args.repeats + 1):  # the first run has the first launches
        b.clear()
        b.copy(capi.VEC_W, capi.VEC_START)
        ctx.sync()
        t0 = time.perf_counter()
        b.lanczos_enqueue(args.m + 1)
        st, alpha, beta = b.lanczos_state()
        ctx.sync()
        dt = time.perf_counter() - t0
        assert st.iterations == args.m and st.stopped == 0
        print(f"({L},{L // 2}) m=0 run {rep} Lanczos m={args.m}: {args.m / dt:9.2f} iterations/s (alpha_0 = {alpha[0]:.12g})", flush=True)
    masks = [1 << i for i in range(L)] + [(1 << i) | (1 << j) for i in range(L) for j in range(i + 1, L)]
    for rep in range(args.repeats + 1):
        ctx.sync()
        t0 = time.perf_counter()
        diag, norm2 = b.spin_momentum_measure(capi.VEC_COL(1), masks)
        dt = time.perf_counter() - t0
        print(f"({L},{L // 2}) m=0 run {rep} measure of {len(masks)} masks: {dt * 1e3:9.2f} ms by the host clock (norm2 = {norm2:.15f})", flush=True)
elif args.step == "ground36":
    op, n = upload(capi.Csr.spin_half_momentum64, L, L // 2, 0, False, "real")
    es = solver.LanczosEigenSolver()
    es.setDeviceOperator(op).set(minIterations=args.ground_steps, maxIterations=args.ground_steps, maxEigenvalues=1, initialVector=solver.random_vector(1, n, np.float64))
    t0 = time.perf_counter()
    es.compute()
    r = es.results()
    dt = time.perf_counter() - t0
    it = r["iterations"]
    alpha, beta = np.asarray(r["alpha"]).real, np.asarray(r["beta"]).real
    T = np.diag(alpha[:it]) + np.diag(beta[: it - 1], 1) + np.diag(beta[: it - 1], -1)
    theta, S = np.linalg.eigh(T)
    e0 = float(np.real(r["eigenvalues"][0]))
    x = np.ascontiguousarray(np.real(r["eigenvectors"][:, 0]))
    es.close()
    print(f"({L},{L // 2}) k=0: E_0 = {e0:.12f} after {it} steps in {dt:.1f} s, E_0 / L = {e0 / L:.12f}, residual estimate {abs(beta[it - 1] * S[it - 1, 0]):.3e}", flush=True)
    b = capi.Basis(ctx, op, n, 1)
    b.upload(capi.VEC_COL(0), x)
    diag, norm2 = b.spin_momentum_measure(capi.VEC_COL(0), [1 | (1 << r) for r in range(1, L // 2 + 1)])
    for r, d in enumerate(diag, 1):
        print(f"({L},{L // 2}) k=0: <Sz_0 Sz_{r}> = {d / (4 * L * norm2):+.10f}", flush=True)
ctx.close()
