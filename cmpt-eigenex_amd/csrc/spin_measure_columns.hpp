// The observables of one real vector x against a set of columns V_j over the rows of a spin-1/2 operator (host side, no HIP): the
// definition, the argument check of the column range, the column chunk of the kernel (kernels.hip: k_spin_measure_columns) and
// the host evaluation.  Shared by the library (eigenex_spin_measure_columns, eigenex_spin_measure_columns_host) and by the host
// program tests/cpp/spin_measure_columns_sanitize.cpp, which runs this file under AddressSanitizer + UBSan.
//
// Rows, sigma_i(s), the two mask lists and their rules are those of spin_measure.hpp (spin_measure_error checks them).  For the
// columns j = 0 .. count - 1 a measurement yields the raw sums
//   diag[t * count + j] = sum_s (prod_{i in mask_t} sigma_i(s)) V_j(s) x_s                    = <V_j| prod sigma |x>
//   flip[t * count + j] = sum_s [sigma_a(s) != sigma_b(s)] V_j(s) x_{s ^ mask_t}              a two-bit mask {a, b}
//                                                                                             = <V_j| S+_a S-_b + S-_a S+_b |x>
//   flip[t * count + j] = sum_s V_j(s) x_{s ^ mask_t}                                         a one-bit mask {a}: the full space only
//                                                                                             = <V_j| 2 Sx_a |x>
// Every sum takes one fma per row, rows ascending: sum = fma(V_j(s), w_t(s), sum) with w_t(s) = (A_t x)(s), which is +-x_s or
// x_{s ^ mask} (or zero).  With V_j = x a diagonal sum has the fma chain of spin_measure_host's diag[t], bit for bit.
// These are the g_i = <v_i| A |v_0> of the finite-temperature Lanczos method when x is column 0 of a Lanczos basis.
#pragma once
#include <stdint.h>

#include <cmath>
#include <vector>

#include "spin_measure.hpp"

namespace eigenex {

// Columns per kernel launch (kernels.hip has the reasoning): a launch keeps 2 * kSpinMeasureChunk * kSpinMeasureColumns sums per lane
constexpr int kSpinMeasureColumns = 4;

// nullptr if columns [first, first + count) exist in a state that holds `held` columns, else what is wrong
inline const char* spin_measure_columns_error(int first, int count, int held) {
  if (count < 1) return "count must be at least 1";
  if (first < 0) return "first must not be negative";
  if ((int64_t)first + (int64_t)count > (int64_t)held) return "first + count exceeds the number of columns the state holds";
  return nullptr;
}

// The definition, evaluated: x has spin_measure_rows entries, column j is V + j * ldv (ldv >= rows); diag_out[n_diag * count] and
// flip_out[n_flip * count] are written where they are not NULL.  Rows ascending, one fma per term and column.
inline void spin_measure_columns_host(const SpinMeasureArgs& a, const double* x, const double* V, int64_t ldv, int count, double* diag_out,
                                      double* flip_out) {
  const bool sector = a.n_up != -1;
  const int64_t n = spin_measure_rows(a);
  SpinSectorTables t;
  if (sector && a.n_flip > 0) spin_sector_build_tables(a.n_sites, a.n_up, t);
  std::vector<double> dg((size_t)a.n_diag * (size_t)count, 0.0), fl((size_t)a.n_flip * (size_t)count, 0.0);
  for (int64_t r = 0; r < n; ++r) {
    const uint32_t s = sector ? spin_sector_unrank(a.n_sites, a.n_up, r) : (uint32_t)r;
    const double xs = x[r];
    for (int i = 0; i < a.n_diag; ++i) {
      const double w = spin_parity(~s & a.diag_masks[i]) ? -xs : xs;
      double* sum = dg.data() + (size_t)i * (size_t)count;
      for (int j = 0; j < count; ++j) sum[j] = std::fma(V[(int64_t)j * ldv + r], w, sum[j]);
    }
    for (int i = 0; i < a.n_flip; ++i) {
      const uint32_t m = a.flip_masks[i];
      if ((m & (m - 1)) != 0 && !spin_parity(s & m)) continue;  // a pair with equal spins has no entry
      const uint32_t s2 = s ^ m;
      const double w = x[sector ? (int64_t)spin_sector_rank(t, s2) : (int64_t)s2];
      double* sum = fl.data() + (size_t)i * (size_t)count;
      for (int j = 0; j < count; ++j) sum[j] = std::fma(V[(int64_t)j * ldv + r], w, sum[j]);
    }
  }
  for (size_t i = 0; i < dg.size() && diag_out; ++i) diag_out[i] = dg[i];
  for (size_t i = 0; i < fl.size() && flip_out; ++i) flip_out[i] = fl[i];
}

}  // namespace eigenex
