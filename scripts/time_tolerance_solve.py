"""A tolerance-driven Lanczos solve through solver.LanczosEigenSolver on an n^3 Laplacian: the case bench.py does not measure.
Beyond minIterations the solver enqueues batches of 1, 2, 4 or 8 calls (one call per batch once a step takes >= 2 ms), so every
step ends a batch; a tolerance that cannot be reached keeps it going to maxIterations.  Prints one JSON line.
usage: python scripts/time_tolerance_solve.py [n=256] [max_iterations=100] [solves=3]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from cmpt_eigenex_amd import capi, solver  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
m = int(sys.argv[2]) if len(sys.argv) > 2 else 100
solves = int(sys.argv[3]) if len(sys.argv) > 3 else 3
N = n ** 3
ctx = capi.Context()
A = capi.Csr.laplacian3d(ctx, n)
es = solver.LanczosEigenSolver()
es.setDeviceOperator(A).set(minIterations=1, maxIterations=m, tolerance=1e-300, computeEigenvectorsOn=0,
                            initialVector=solver.default_start_vector(N))
ts = []
for rep in range(solves + 1):  # the first one warms up
    ctx.sync()
    t0 = time.perf_counter()
    es.compute()
    ctx.sync()
    ts.append(time.perf_counter() - t0)
r = es.results()
print(json.dumps({"workload": "laplacian3d_%d_tolerance_driven_m%d" % (n, m), "iterations": r["iterations"], "nvec": r["nvec"],
                  "eager_close": "EIGENEX_EAGER_CLOSE" in os.environ, "ms_per_solve": [t * 1e3 for t in ts[1:]],
                  "ms_per_step": float(np.mean(ts[1:])) * 1e3 / max(r["iterations"], 1), "alpha_last": float(r["alpha"][-1])}))
es.close()
A.close()
ctx.close()
