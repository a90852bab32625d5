"""Times the pieces of a dynamical spin correlation on the periodic spin-1/2 Heisenberg chain in the sector of n_up sites up, in
one process:
  (a) eigenex_spin_site_apply, kind Z, from a vector of the source state into the work vector of a second state on the same
      operator, and kind MINUS into the work vector of a state on the sector n_up - 1;
  (b) one eigenex_apply of the sector operator at the same size, beside them;
  (c) a whole SpinDynamicsSolver::computeStructureFactorZ(pi) at m Lanczos steps (upload of the state, both parts, the
      tridiagonal eigenproblems), from a random +-1 state with its energy given (no eigenstate is needed to time it).
Host clock around calls that end in a synchronise; one warm-up call of each, then --repeats timed ones, median, minimum and
maximum printed.  Every step runs under an alarm of its own: a step that hangs ends the process instead of holding the device.
usage: python scripts/probe_spin_dynamics.py [--sectors 24:12 28:14] [--repeats 5] [--steps 100] [--step-timeout 240]"""
import argparse
import signal
import sys
import time

sys.path.insert(0, ".")
import numpy as np

from cmpt_eigenex_amd import capi, solver


def pair(text):
    L, k = text.split(":")
    return int(L), int(k)


ap = argparse.ArgumentParser()
ap.add_argument("--sectors", type=pair, nargs="+", default=[(24, 12), (28, 14)])
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--step-timeout", type=int, default=240)
args = ap.parse_args()


def on_alarm(signum, frame):
    print("a step ran into its time limit: stopping", flush=True)
    sys.exit(3)


signal.signal(signal.SIGALRM, on_alarm)


def timed(label, call, ctx, repeats):
    """median, min, max in seconds of `repeats` calls after one warm-up call; each call under its own alarm"""
    times = []
    for rep in range(repeats + 1):
        signal.alarm(args.step_timeout)
        ctx.sync()
        t0 = time.perf_counter()
        call()
        ctx.sync()
        dt = time.perf_counter() - t0
        signal.alarm(0)
        if rep:
            times.append(dt)
    t = np.array(times)
    print(f"{label}: median {np.median(t) * 1e3:10.3f} ms (min {t.min() * 1e3:.3f}, max {t.max() * 1e3:.3f}, {repeats} calls)", flush=True)
    return float(np.median(t))


ctx = capi.Context()
for (L, n_up) in args.sectors:
    n, nd = capi.spin_sector_dim(L, n_up), capi.spin_sector_dim(L, n_up - 1)
    tag = f"({L},{n_up})"
    bonds = [(i, (i + 1) % L, 1.0, 1.0) for i in range(L)]
    c = np.cos(np.pi * np.arange(L)) / np.sqrt(L)
    print(f"{tag}: {n} rows, vector {8 * n / 1e9:.3f} GB; ({L},{n_up - 1}): {nd} rows", flush=True)
    S, D = capi.Csr.spin_half_sector(ctx, L, n_up, bonds), capi.Csr.spin_half_sector(ctx, L, n_up - 1, bonds)
    src, same, down = capi.Basis(ctx, S, n, 1), capi.Basis(ctx, S, n, 1), capi.Basis(ctx, D, nd, 1)
    src.random_signs(capi.VEC_COL(0), 1, 0)
    t_apply = timed(f"{tag} eigenex_apply of the sector operator", lambda: src.apply(capi.VEC_COL(0), capi.VEC_V, 0.0, want_dot=True), ctx, args.repeats)
    t_z = timed(f"{tag} eigenex_spin_site_apply Z", lambda: src.spin_site_apply(capi.VEC_COL(0), same, capi.VEC_W, capi.SPIN_SITE_Z, c), ctx, args.repeats)
    t_m = timed(f"{tag} eigenex_spin_site_apply MINUS -> ({L},{n_up - 1})", lambda: src.spin_site_apply(capi.VEC_COL(0), down, capi.VEC_W, capi.SPIN_SITE_MINUS, c),
                ctx, args.repeats)
    print(f"{tag}: Z / apply = {t_z / t_apply:.2f}, MINUS / apply = {t_m / t_apply:.2f}; bytes moved by Z: {16 * n / 1e9:.3f} GB, "
          f"{16 * n / 1e9 / t_z:.0f} GB/s over the whole call (host clock, with the call's allocations, table upload and synchronise)", flush=True)
    x = src.download(capi.VEC_COL(0))
    for h in (src, same, down):
        h.close()
    sd = solver.SpinDynamicsSolver().setModel(ctx, L, bonds, None, None, n_up).setState(x).setStateEnergy(0.0).setLanczosSteps(args.steps)
    t_sd = timed(f"{tag} computeStructureFactorZ(pi), m = {args.steps}", lambda: sd.computeStructureFactorZ(np.pi), ctx, max(1, args.repeats // 2))
    r = sd.results()
    print(f"{tag}: info {r['info_name']}, poles {r['npoles']}, total weight {r['totalWeight']!r}; whole solve / one apply = {t_sd / t_apply:.0f}", flush=True)
    sd.close()
    S.close()
    D.close()
ctx.close()
