"""Time per degree on the generated n^3 Laplacian, from the library's own per-kernel profile (HIP events around every launch):
a fused Chebyshev-moments degree (eigenex_kpm_moments), the filter's fused degree (eigenex_filter_apply) and a plain operator
application (eigenex_apply).  The first degree of either recurrence reads one vector less, so its share is taken out by running
two lengths and dividing the difference.
usage: python scripts/kpm_degree_time.py n [degrees] [repeats]"""
import sys

sys.path.insert(0, ".")
import numpy as np

from cmpt_eigenex_amd import capi

n = int(sys.argv[1])
d = int(sys.argv[2]) if len(sys.argv) > 2 else 40
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
N = n ** 3
PEAK = 8.0e12  # bytes/s
ctx = capi.Context()
A = capi.Csr.laplacian3d(ctx, n)
b = capi.Basis(ctx, A, N, 2)
b.random_signs(capi.VEC_COL(0), 1, 0)
center, half = 6.0, 6.0 * 1.01  # the spectrum of the 7-point Laplacian lies in [0, 12]
print(f"n={n} N={N} encoding={A.encoding()} degrees={d}", flush=True)


def profiled(fn):
    ctx.profile_reset()
    ctx.profile_enable(True)
    fn()
    cnt, ms, by = ctx.profile_get(capi.K_SPMV)
    ctx.profile_enable(False)
    return cnt, ms, by


def per_degree(run):
    """(ms, bytes) of one later degree: the difference of a run of d + 1 and a run of 1 degrees, over d"""
    c1, ms1, by1 = profiled(lambda: run(1))
    c2, ms2, by2 = profiled(lambda: run(d + 1))
    assert c1 == 1 and c2 == d + 1, (c1, c2)
    return (ms2 - ms1) / d, (by2 - by1) / d


def moments(k):
    b.kpm_moments(capi.VEC_COL(0), 2 * k + 1, center, half)


def filt(k):
    b.set_filter(np.full(k + 1, 1.0 / (k + 1)), center, half)
    b.filter_apply(capi.VEC_COL(0), capi.VEC_V)


def apply(k):
    for _ in range(k):
        b.apply(capi.VEC_COL(0), capi.VEC_V)


moments(2), filt(2), apply(2)  # allocations and first launches
for rep in range(reps):
    for name, run in (("moments degree (fused)", moments), ("filter degree (fused)", filt), ("operator application", apply)):
        ms, by = per_degree(run)
        print(f"rep {rep}: {name:24s} {ms * 1e3:9.1f} us  booked {by / N:6.1f} B/row  {by / (ms * 1e-3) / 1e12:6.3f} TB/s = {by / (ms * 1e-3) / PEAK:5.3f} of 8 TB/s", flush=True)
