#!/usr/bin/env python3
"""Fit the duration of each full-grid launch of a slab kernel in a rocprofv3 kernel trace against the step it belongs to:

    scripts/fit_sweep_launches.py TRACE.csv k_sweep [M]     (one-sweep step k streams k - 1 columns and moves k + 4 vectors)
    scripts/fit_sweep_launches.py TRACE.csv k_dots [M]      (EIGENEX_TWO_SWEEPS=1: step k reads k + 1 columns and three vectors)

The trace does not name k (its LDS column holds the static size only), so launches are taken in dispatch order and numbered
k = 0..M-1 within each solve of M steps (bench.py: M = 100); the closing pass and launches on fewer than 512 workgroups (the
repair pass, small operators) are left out.  Prints the least-squares slope (ms per step, that is per column), the intercept,
and the residuals by k as a markdown table (mean over the solves of the trace, with their extremes).
"""
import csv
import re
import sys
from collections import defaultdict

import numpy as np


def main():
    path, name = sys.argv[1], sys.argv[2]
    M = int(sys.argv[3]) if len(sys.argv) > 3 else 100
    rows = []
    for r in csv.DictReader(open(path)):
        kn = r["Kernel_Name"]
        m = re.search(r"\b%s<([^>]*)>" % name, kn)  # "void eigenex::(anonymous namespace)::k_sweep<false, true>(...)"
        if not m:
            continue
        if name == "k_sweep" and m.group(1).split(",")[0].strip() == "true":
            continue  # the closing pass
        if int(r["Grid_Size_X"]) < 512 * 256:
            continue  # the repair pass's launches and small operators
        rows.append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6))
    rows.sort()
    assert rows and len(rows) % M == 0, "%d launches are not whole solves of %d steps" % (len(rows), M)
    by_k = defaultdict(list)
    for i, (_, ms) in enumerate(rows):
        by_k[i % M].append(ms)
    ks = np.array(sorted(by_k))
    mean = np.array([np.mean(by_k[k]) for k in ks])
    lo = np.array([np.min(by_k[k]) for k in ks])
    hi = np.array([np.max(by_k[k]) for k in ks])
    fit = ks >= 8  # the first launches are not streaming yet
    slope, icpt = np.polyfit(ks[fit], mean[fit], 1)
    res = mean - (slope * ks + icpt)
    print("%s: %d launches, %d steps per solve, fit over k >= 8" % (name, len(rows), M))
    print("slope %.5f ms per step, intercept %.4f ms, rms residual %.4f ms, largest |residual| %.4f ms (k = %d)"
          % (slope, icpt, float(np.sqrt(np.mean(res[fit] ** 2))), float(np.abs(res[fit]).max()), int(ks[fit][np.abs(res[fit]).argmax()])))
    print("| k | launches | mean ms | min | max | residual ms |\n|---|---|---|---|---|---|")
    for k, m, a, b, r in zip(ks, mean, lo, hi, res):
        print("| %d | %d | %.4f | %.4f | %.4f | %+.4f |" % (k, len(by_k[k]), m, a, b, r))


if __name__ == "__main__":
    main()
