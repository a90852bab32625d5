// The small terms of the one-sweep Lanczos step (kernels.hip: k_sweep, k_lag_terms; library.hip: lanczos_step_one_sweep),
// no HIP needed: shared by the kernels and by the host program tests/cpp/lag_terms_sanitize.cpp, which runs this file under
// AddressSanitizer + UBSan and holds it against the values of tests/one_sweep_reference.py.
//
// Step k re-orthogonalises against columns 0..k in ONE sweep of the basis.  The dots d = V^T w0 it takes are only complete at
// the end of the sweep, so they are applied one step late: c (length k) = the coefficients the PREVIOUS step found, still
// missing from column k, which the operator has already used raw.  What that lag does to w0 is known before the sweep, from
// the tridiagonal matrix T so far (alpha[0..k), beta[0..k)), c and the raw a' = u~_k . A u~_k:
//
//   f[i] = (T[(k+1) x k] c)[i] - a' c[i]   (i < k),      da = 2 c[k-1] beta[k-1],      f[k] = beta[k-1] c[k-1] - da
//   alpha_k = a' - da,        w = w0 - V f (inside the sweep),        h = d - f,        c_next = h / beta_k  (length k+1)
//
// Both f and da are needed: without f the coefficients obey c_{k+1} ~ (T - alpha I) c_k / beta and grow geometrically (1e-16 to
// 1e-6 in 40 steps of the 16^3 Laplacian); without da orthogonality is lost after ~100 steps.  c^2 terms are dropped, so the
// scheme needs |c| << sqrt(eps): beyond kLagGuard the pending vector is re-orthogonalised by the two-sweep pass instead.
//
// Every product is rounded before it is added (no contraction), so that every workgroup, the closing pass and the host arrive at
// the same bits.
#pragma once

#if defined(__HIPCC__)
#define EIGENEX_LAG_HD __host__ __device__
#else
#define EIGENEX_LAG_HD
#endif

namespace eigenex {

constexpr double kLagGuard = 7.450580596923828125e-09;  // 2^-27
constexpr int kSweepMaxCols = 1024;  // k_sweep keeps 6 doubles of LDS per column (4 per-wave sums, c, f): 48 KB

// first-order correction of alpha_k for the lag of column k; 0 at k == 0
EIGENEX_LAG_HD inline double lag_alpha_correction(int k, const double* beta, const double* c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (k <= 0) return 0.0;
  const double twice = 2.0 * c[k - 1];
  return twice * beta[k - 1];
}

// f[i], i <= k.  Column j of T reaches entries j+1, j, j-1; entry i adds them in the order j = i-1, i, i+1.
EIGENEX_LAG_HD inline double lag_f_entry(int i, int k, const double* alpha, const double* beta, const double* c, double a_raw, double da) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double s = 0.0;
  if (i >= 1 && i - 1 < k) {
    const double p = beta[i - 1] * c[i - 1];
    s += p;
  }
  if (i < k) {
    const double p = alpha[i] * c[i];
    s += p;
  }
  if (i + 1 < k) {
    const double p = beta[i] * c[i + 1];
    s += p;
  }
  if (i < k) {
    const double p = a_raw * c[i];
    s -= p;
  }
  if (i == k && k > 0) s -= da;
  return s;
}

// the coefficient of column i that the NEXT sweep applies to column k+1: (d - f) / beta_k; nothing is pending behind a breakdown
EIGENEX_LAG_HD inline double lag_next_coefficient(double d, double f, double beta_k, double threshold) {
  const double h = d - f;
  return beta_k > threshold ? h / beta_k : 0.0;
}

}  // namespace eigenex
