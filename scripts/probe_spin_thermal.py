"""The columns measurement behind the finite-temperature Lanczos solver next to its yardstick, in one process per run: a basis of
`count` columns of the periodic spin-1/2 Heisenberg chain in the sector of n_up sites up (random sign vectors), then
  (a) one eigenex_spin_measure_columns with 16 diagonal terms        -- one pass of the basis, no gathers;
  (b) one eigenex_spin_measure_columns with 16 diagonal + 16 flip terms -- one pass of the basis with all gathers;
  (c) one eigenex_dots of the same columns                            -- the same basis bytes, the yardstick;
  (d) with --compute: one whole ThermalLanczosSolver.compute() with all sites and pairs, R vectors, M steps.
Host clock around the calls; each ends in a synchronise.  Kernel times come from a kernel trace of a run of its own:

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/probe_spin_thermal.py --sectors 28:14 --once
    python scripts/probe_spin_thermal.py --summarize DIR --sectors 28:14

--once runs (a), (b), (c) exactly once each after first launches on two columns, so that the trace holds, in order, the launches of
(a), of (b) and of (c); --summarize adds up the durations of k_spin_measure_columns (first half: (a), second half: (b)) and of
k_dots, leaving out the first launches, and prints the ratios and the fraction of the HBM peak that the basis bytes imply.
usage: python scripts/probe_spin_thermal.py [--sectors 24:12 28:14] [--count 50] [--repeats 3] [--compute R M]"""
import argparse
import csv
import glob
import os
import sys
import time

sys.path.insert(0, ".")
import numpy as np

HBM_PEAK = 8.0e12  # bytes per second, MI355X


def pair(text):
    L, k = text.split(":")
    return int(L), int(k)


ap = argparse.ArgumentParser()
ap.add_argument("--sectors", type=pair, nargs="+", default=[(24, 12), (28, 14)])
ap.add_argument("--count", type=int, default=50)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--once", action="store_true")
ap.add_argument("--compute", type=int, nargs=2, metavar=("R", "M"))
ap.add_argument("--summarize", metavar="DIR")
args = ap.parse_args()
J = 4  # csrc/spin_measure_columns.hpp: kSpinMeasureColumns

if args.summarize:
    from math import comb

    (L, n_up), = args.sectors
    rows = []
    for path in glob.glob(os.path.join(args.summarize, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    per = -(-args.count // J)  # launches per call
    timed = [(s, d) for (s, d, name) in rows if "k_spin_measure_columns<" in name][-2 * per:]
    cols = [d for (_, d) in timed]
    dots = [d for (s, d, name) in rows if "k_dots" in name and s > timed[-1][0]]  # the call behind (b); the first launches came before (a)
    assert len(cols) == 2 * per and dots, (len(cols), per, len(dots))
    a, b, c = sum(cols[:per]) * 1e-9, sum(cols[per:]) * 1e-9, sum(dots) * 1e-9
    basis = 8.0 * comb(L, n_up) * args.count
    print(f"({L},{n_up}), {args.count} columns, basis {basis / 1e9:.2f} GB, kernel time from the trace")
    for name, t in (("16 diagonal terms", a), ("16 + 16 terms", b), ("eigenex_dots", c)):
        print(f"  {name:20s} {t * 1e3:9.3f} ms   basis bytes / time = {basis / t / 1e12:5.2f} TB/s = {100 * basis / t / HBM_PEAK:4.1f} % of the HBM peak"
              f"   ratio to eigenex_dots {t / c:5.2f}")
    sys.exit(0)

from cmpt_eigenex_amd import capi, solver

ctx = capi.Context()
for (L, n_up) in args.sectors:
    n = capi.spin_sector_dim(L, n_up)
    tag = f"({L},{n_up})"
    bonds = [(i, (i + 1) % L, 1.0, 1.0) for i in range(L)]
    S = capi.Csr.spin_half_sector(ctx, L, n_up, bonds)
    pair_masks = [(1 << i) | (1 << j) for i in range(L) for j in range(i + 1, L)]
    diag16, flip16 = pair_masks[:16], pair_masks[16:32]
    print(f"{tag}: {n} rows, {args.count} columns, basis {8 * n * args.count / 1e9:.2f} GB", flush=True)
    b = capi.Basis(ctx, S, n, args.count)
    for j in range(args.count):
        b.random_signs(capi.VEC_COL(j), 7, j)
    b.spin_measure_columns(capi.VEC_COL(0), 0, 2, diag16, flip16)  # first launches
    b.dots(capi.VEC_COL(0), 0, 1, 2)
    for rep in range(1 if args.once else args.repeats):
        t = []
        for call in (lambda: b.spin_measure_columns(capi.VEC_COL(0), 0, args.count, diag16, []),
                     lambda: b.spin_measure_columns(capi.VEC_COL(0), 0, args.count, diag16, flip16),
                     lambda: b.dots(capi.VEC_COL(0), 0, 1, args.count)):
            ctx.sync()
            t0 = time.perf_counter()
            call()
            t.append(time.perf_counter() - t0)
        print(f"{tag} rep {rep}, host clock: 16 diagonal terms {t[0] * 1e3:9.2f} ms, 16 + 16 terms {t[1] * 1e3:9.2f} ms, eigenex_dots {t[2] * 1e3:9.2f} ms; "
              f"ratios to eigenex_dots {t[0] / t[2]:.2f} and {t[1] / t[2]:.2f}", flush=True)
    b.close()
    if args.compute:
        R, M = args.compute
        th = solver.ThermalLanczosSolver().setDeviceOperator(S).set(lanczosSteps=M, randomVectors=R, seed=1)
        assert th.setAllSitesAndPairs() == "Success"
        ctx.sync()
        t0 = time.perf_counter()
        th.compute()
        dt = time.perf_counter() - t0
        r = th.results()
        print(f"{tag} compute(): R = {R}, M = {M}, {r['ndiag']} + {r['nflip']} observables: {dt:.2f} s ({r['info_name']}, {r['operatorApplications']} operator "
              f"applications); E(beta = 1) / L = {th.energy(1.0) / L:.6f} +- {th.standardError('energy', 1.0) / L:.6f}, "
              f"<S_0.S_1>(beta = 1) = {th.correlationSS(0, 1, 1.0):.6f}", flush=True)
        th.close()
    S.close()
ctx.close()
