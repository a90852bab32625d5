"""Times the site operators of complex states beside those of real states on the periodic spin-1/2 Heisenberg chain in the sector
of n_up sites up, and the two solvers built on them, in one process:
  (a) eigenex_spin_site_apply (real state, real coefficients L^{-1/2} cos(q i)) and eigenex_spin_site_apply_z (complex state,
      complex coefficients L^{-1/2} e^{iqi}, q = 2 pi 3 / L), kind Z into a second state on the same operator and kind MINUS into
      a state on the sector n_up - 1.  The host clock is around whole calls; the kernels' own times come from running this script
      under a kernel trace (--sites-only keeps that run short), where the four instantiations show under their own names;
  (b) with --solvers: one time point of SpinTimeCorrelationSolver with setMeasuredSites() (one evolve(dt) of both vectors and
      values()) beside one evolve(dt) of SpinTimeEvolutionSolver, from the Neel state, B = S-_0;
  (c) with --solvers: SpinDynamicsSolver::computeStructureFactorZSingleRun(pi) beside computeStructureFactorZ(pi) at --steps
      Lanczos steps, from a random +-1 state with its energy given.
One warm-up call of each, then --repeats timed ones, median, minimum and maximum printed.  Every step runs under an alarm of its
own: a step that hangs ends the process instead of holding the device.
With --summarize-trace FILE (no GPU) it reads the kernel trace (CSV) of such a run made with the same --sectors and --repeats and
prints, per sector and label, the kernel's own time: the dispatches of k_spin_site_apply in the order this script makes them, the
warm-up call of each label dropped.
usage: python scripts/probe_spin_site_z.py [--sectors 24:12 28:14] [--repeats 5] [--solvers 28:14] [--krylov 30] [--dt 0.05]
                                          [--steps 100] [--step-timeout 240] [--sites-only]"""
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
ap.add_argument("--solvers", type=pair, nargs="*", default=[])
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--krylov", type=int, default=30)
ap.add_argument("--dt", type=float, default=0.05)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--step-timeout", type=int, default=240)
ap.add_argument("--sites-only", action="store_true")
ap.add_argument("--summarize-trace", default=None)
args = ap.parse_args()

LABELS = ("real Z", "real MINUS", "complex Z", "complex MINUS", "complex Z, real coefficients")  # the order of the calls below

if args.summarize_trace:
    import csv

    with open(args.summarize_trace, newline="") as f:
        rows = [r for r in csv.DictReader(f) if "k_spin_site_apply" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = args.repeats + 1
    assert len(rows) == per * len(LABELS) * len(args.sectors), (len(rows), per, len(args.sectors))
    for i, (L, n_up) in enumerate(args.sectors):
        got = {}
        for j, label in enumerate(LABELS):
            block = rows[(i * len(LABELS) + j) * per:(i * len(LABELS) + j + 1) * per]
            names = {r["Kernel_Name"] for r in block}
            assert len(names) == 1 and (("SpinZ" in next(iter(names))) == label.startswith("complex")), names
            t = np.array([int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in block[1:]]) * 1e-6  # ms; the first is the warm-up
            got[label] = float(t.mean())
            print(f"({L},{n_up}) {label}: kernel {t.mean():.4f} ms (min {t.min():.4f}, max {t.max():.4f}, {t.size} dispatches)  {next(iter(names))[:60]}")
        print(f"({L},{n_up}) kernel time, complex / real: Z {got['complex Z'] / got['real Z']:.2f}, MINUS {got['complex MINUS'] / got['real MINUS']:.2f}; "
              f"complex Z with real coefficients / complex Z {got['complex Z, real coefficients'] / got['complex Z']:.2f}")
    sys.exit(0)


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
    q = 2 * np.pi * 3 / L
    cz = np.exp(1j * q * np.arange(L)) / np.sqrt(L)
    print(f"{tag}: {n} rows, real vector {8 * n / 1e9:.3f} GB, complex {16 * n / 1e9:.3f} GB; ({L},{n_up - 1}): {nd} rows", flush=True)
    out = {}
    for word, cplx, coef in (("real", False, cz.real.copy()), ("complex", True, cz)):
        S = capi.Csr.spin_half_sector(ctx, L, n_up, bonds, complex_states=cplx)
        D = capi.Csr.spin_half_sector(ctx, L, n_up - 1, bonds, complex_states=cplx)
        src, same, down = capi.Basis(ctx, S, n, 1), capi.Basis(ctx, S, n, 1), capi.Basis(ctx, D, nd, 1)
        src.random_signs(capi.VEC_COL(0), 1, 0)
        call = src.spin_site_apply_z if cplx else src.spin_site_apply
        out[word, "Z"] = timed(f"{tag} {word} Z", lambda: call(capi.VEC_COL(0), same, capi.VEC_W, capi.SPIN_SITE_Z, coef), ctx, args.repeats)
        out[word, "MINUS"] = timed(f"{tag} {word} MINUS -> ({L},{n_up - 1})", lambda: call(capi.VEC_COL(0), down, capi.VEC_W, capi.SPIN_SITE_MINUS, coef),
                                   ctx, args.repeats)
        if cplx:  # real coefficients on the complex state: the branch without the imaginary products
            out[word, "Z real coef"] = timed(f"{tag} complex Z, real coefficients", lambda: call(capi.VEC_COL(0), same, capi.VEC_W, capi.SPIN_SITE_Z, cz.real.copy()),
                                             ctx, args.repeats)
        for h in (src, same, down, S, D):
            h.close()
    print(f"{tag}: whole calls on the host clock, complex / real: Z {out['complex', 'Z'] / out['real', 'Z']:.2f}, "
          f"MINUS {out['complex', 'MINUS'] / out['real', 'MINUS']:.2f}", flush=True)

for (L, n_up) in ([] if args.sites_only else args.solvers):
    tag = f"({L},{n_up})"
    bonds = [(i, (i + 1) % L, 1.0, 1.0) for i in range(L)]
    neel = sum(1 << i for i in range(0, L, 2))
    source = np.zeros(L)
    source[0] = 1.0
    te = solver.SpinTimeEvolutionSolver().setModel(ctx, L, bonds, None, None, n_up=n_up).setKrylovDimension(args.krylov).setTolerance(1e-8).setProductState(neel)
    t_te = timed(f"{tag} SpinTimeEvolutionSolver::evolve({args.dt}), m = {args.krylov}", lambda: te.evolve(args.dt), ctx, max(1, args.repeats // 2))
    print(f"{tag}: info {te.info()}, applications {te.operatorApplications()}, bound {te.errorBound():.2e}", flush=True)
    te.close()
    tc = solver.SpinTimeCorrelationSolver().setModel(ctx, L, bonds, None, None, n_up=n_up).setKrylovDimension(args.krylov).setTolerance(1e-8)
    tc.setProductState(neel).setSourceOperator(capi.SPIN_SITE_MINUS, source).setMeasuredSites()
    signal.alarm(args.step_timeout)
    tc.values()  # the upload, both states and B psi_0 are set-up, not a time point
    signal.alarm(0)
    t_ev = timed(f"{tag} SpinTimeCorrelationSolver::evolve({args.dt}), both vectors", lambda: tc.evolve(args.dt), ctx, max(1, args.repeats // 2))
    t_val = timed(f"{tag} SpinTimeCorrelationSolver::values(), {L} measured sites", lambda: tc.values(), ctx, max(1, args.repeats // 2))
    print(f"{tag}: info {tc.info()}, applications {tc.operatorApplications()}, bound {tc.errorBound():.2e}; one time point / one evolution sub-step = "
          f"{(t_ev + t_val) / t_te:.2f} (values alone {t_val / t_te:.3f})", flush=True)
    tc.close()
    n = capi.spin_sector_dim(L, n_up)
    x = np.where(np.random.RandomState(1).randint(0, 2, n) > 0, 1.0, -1.0)
    sd = solver.SpinDynamicsSolver().setModel(ctx, L, bonds, None, None, n_up).setState(x).setStateEnergy(0.0).setLanczosSteps(args.steps)
    t_two = timed(f"{tag} computeStructureFactorZ(pi), m = {args.steps}", lambda: sd.computeStructureFactorZ(np.pi), ctx, max(1, args.repeats // 2))
    two = sd.results()
    t_one = timed(f"{tag} computeStructureFactorZSingleRun(pi), m = {args.steps}", lambda: sd.computeStructureFactorZSingleRun(np.pi), ctx, max(1, args.repeats // 2))
    one = sd.results()
    print(f"{tag}: two runs {two['info_name']}, {two['npoles']} poles, total weight {two['totalWeight']!r}; single run {one['info_name']}, {one['npoles']} poles, "
          f"total weight {one['totalWeight']!r}; single / two = {t_one / t_two:.2f}", flush=True)
    sd.close()
ctx.close()
