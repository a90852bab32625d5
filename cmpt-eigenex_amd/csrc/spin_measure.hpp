// Spin correlations of a real vector over the rows of a spin-1/2 operator (host side, no HIP): the definition, the argument
// check, the chunk table of the kernel (kernels.hip: k_spin_measure) and the host evaluation.  Shared by the library
// (eigenex_spin_measure, eigenex_spin_measure_host) and by the host program tests/cpp/spin_measure_sanitize.cpp, which runs this
// file under AddressSanitizer + UBSan.
//
// The rows are those of spin_model.hpp (n_up = -1: the full space, row s is state s) or of spin_sector.hpp (row r is the state
// of rank r among the states with n_up sites up).  sigma_i(s) = +1 if bit i of s is set, else -1.  A measurement is two lists of
// 32-bit site masks and yields raw, unnormalised sums over the rows:
//   norm2   = sum_s x_s^2
//   diag[t] = sum_s (prod_{i in mask} sigma_i(s)) x_s^2                   a mask of 1..n_sites bits: -1 where parity(~s & mask) is odd
//   flip[t] = sum_s [sigma_i(s) != sigma_j(s)] x_s x_{s ^ mask}           a two-bit mask {i, j}
//   flip[t] = sum_s x_s x_{s ^ mask}                                      a one-bit mask {i}: the full space only
// so that <Sz_i> = diag{i} / (2 norm2), <Sz_i Sz_j> = diag{i,j} / (4 norm2), <Sx_i> = flip{i} / (2 norm2) and
// <Sx_i Sx_j + Sy_i Sy_j> = flip{i,j} / (2 norm2).  Every sum takes one fma per row, rows ascending.
#pragma once
#include <stdint.h>

#include <cmath>
#include <vector>

#include "spin_sector.hpp"

namespace eigenex {

constexpr int kSpinMeasureMaxTerms = 1024;  // per list: all 496 pairs and 32 sites of L = 32 fit
// Terms of each list per kernel launch: 2 * 16 + 1 sums of 2 VGPRs each next to one batch of gathers stays far from spilling
constexpr int kSpinMeasureChunk = 16;
static_assert(kSpinMeasureChunk % kSpinBatch == 0, "the kernel takes a chunk's terms kSpinBatch at a time");

struct SpinMeasureArgs {
  int n_sites, n_up;  // n_up = -1: the full space
  int n_diag;
  const uint32_t* diag_masks;
  int n_flip;
  const uint32_t* flip_masks;
};

// nullptr if the measurement is valid, else what is wrong with it
inline const char* spin_measure_error(const SpinMeasureArgs& a) {
  const bool sector = a.n_up != -1;
  if (!sector && (a.n_sites < kSpinMinSites || a.n_sites > kSpinMaxSites)) return "n_sites must be 2..30 in the full space";
  if (sector && (a.n_sites < kSpinMinSites || a.n_sites > kSectorMaxSites)) return "n_sites must be 2..32";
  if (sector && (a.n_up < 0 || a.n_up > a.n_sites)) return "n_up must be 0..n_sites, or -1 for the full space";
  if (a.n_diag < 0 || a.n_diag > kSpinMeasureMaxTerms || a.n_flip < 0 || a.n_flip > kSpinMeasureMaxTerms) return "n_diag and n_flip must be 0..1024";
  if ((a.n_diag > 0 && !a.diag_masks) || (a.n_flip > 0 && !a.flip_masks)) return "a mask list is NULL but its count is not zero";
  const uint32_t outside = a.n_sites < 32 ? ~((uint32_t(1) << a.n_sites) - 1) : 0u;
  for (int t = 0; t < a.n_diag; ++t) {
    if (a.diag_masks[t] == 0) return "a mask is zero";
    if (a.diag_masks[t] & outside) return "a mask names a site outside 0..n_sites-1";
  }
  for (int t = 0; t < a.n_flip; ++t) {
    const uint32_t m = a.flip_masks[t];
    if (m == 0) return "a mask is zero";
    if (m & outside) return "a mask names a site outside 0..n_sites-1";
    const int bits = __builtin_popcount(m);
    if (bits > 2) return "a flip mask must have one or two bits";
    if (bits == 1 && sector) return "a one-bit flip mask (Sx) does not conserve total Sz: it has no meaning in a fixed-magnetisation sector";
  }
  return nullptr;
}

// What one launch of k_spin_measure receives (device memory; every lane reads the same entry): terms [k C, k C + C) of both
// lists, padded with mask 0 -- a zero diagonal mask (no site down) sums x^2 into a slot nobody reads, a zero flip mask never flips.
struct SpinMeasureChunk {
  int ndiag, nflip;  // live terms of this chunk, 0..kSpinMeasureChunk each
  uint32_t dmask[kSpinMeasureChunk], fmask[kSpinMeasureChunk];
};

// at least one chunk: norm2 is measured with empty lists too
inline int spin_measure_chunks(int n_diag, int n_flip) {
  const int most = n_diag > n_flip ? n_diag : n_flip;
  return most == 0 ? 1 : (most + kSpinMeasureChunk - 1) / kSpinMeasureChunk;
}

inline void spin_measure_build_chunks(const SpinMeasureArgs& a, std::vector<SpinMeasureChunk>& chunks) {
  chunks.assign((size_t)spin_measure_chunks(a.n_diag, a.n_flip), SpinMeasureChunk());
  for (size_t k = 0; k < chunks.size(); ++k) {
    SpinMeasureChunk& c = chunks[k];
    const int first = (int)k * kSpinMeasureChunk;
    c.ndiag = a.n_diag - first < 0 ? 0 : (a.n_diag - first < kSpinMeasureChunk ? a.n_diag - first : kSpinMeasureChunk);
    c.nflip = a.n_flip - first < 0 ? 0 : (a.n_flip - first < kSpinMeasureChunk ? a.n_flip - first : kSpinMeasureChunk);
    for (int t = 0; t < c.ndiag; ++t) c.dmask[t] = a.diag_masks[first + t];
    for (int t = 0; t < c.nflip; ++t) c.fmask[t] = a.flip_masks[first + t];
  }
}

// number of rows of a valid measurement's operator
inline int64_t spin_measure_rows(const SpinMeasureArgs& a) {
  return a.n_up == -1 ? int64_t(1) << a.n_sites : spin_sector_dim(a.n_sites, a.n_up);
}

// The definition, evaluated: x has spin_measure_rows entries; diag_out[n_diag], flip_out[n_flip] and norm2 are written where
// they are not NULL.  Rows ascending, one fma per term.
inline void spin_measure_host(const SpinMeasureArgs& a, const double* x, double* diag_out, double* flip_out, double* norm2) {
  const bool sector = a.n_up != -1;
  const int64_t n = spin_measure_rows(a);
  SpinSectorTables t;
  if (sector && a.n_flip > 0) spin_sector_build_tables(a.n_sites, a.n_up, t);
  std::vector<double> dg((size_t)a.n_diag, 0.0), fl((size_t)a.n_flip, 0.0);
  double nrm = 0.0;
  for (int64_t r = 0; r < n; ++r) {
    const uint32_t s = sector ? spin_sector_unrank(a.n_sites, a.n_up, r) : (uint32_t)r;
    const double xs = x[r];
    nrm = std::fma(xs, xs, nrm);
    for (int i = 0; i < a.n_diag; ++i) dg[(size_t)i] = std::fma(spin_parity(~s & a.diag_masks[i]) ? -xs : xs, xs, dg[(size_t)i]);
    for (int i = 0; i < a.n_flip; ++i) {
      const uint32_t m = a.flip_masks[i];
      if ((m & (m - 1)) != 0 && !spin_parity(s & m)) continue;  // a pair with equal spins has no entry
      const uint32_t s2 = s ^ m;
      fl[(size_t)i] = std::fma(xs, x[sector ? (int64_t)spin_sector_rank(t, s2) : (int64_t)s2], fl[(size_t)i]);
    }
  }
  for (int i = 0; i < a.n_diag && diag_out; ++i) diag_out[i] = dg[(size_t)i];
  for (int i = 0; i < a.n_flip && flip_out; ++i) flip_out[i] = fl[(size_t)i];
  if (norm2) *norm2 = nrm;
}

// The Hermitian definitions for a complex vector, x interleaved (re, im), 2 * spin_measure_rows doubles:
//   norm2   = sum_s |x_s|^2
//   diag[t] = sum_s (prod_{i in mask} sigma_i(s)) |x_s|^2
//   flip[t] = sum_s [predicate as above] Re(conj(x_s) x_{s ^ mask})
// so the normalisations above hold unchanged.  Rows ascending; every sum takes two fmas per row, the product of the real parts and
// then the product of the imaginary parts.  With every imaginary part +0 the sums are spin_measure_host's: fma(0, 0, a) is a.
inline void spin_measure_host_z(const SpinMeasureArgs& a, const double* x, double* diag_out, double* flip_out, double* norm2) {
  const bool sector = a.n_up != -1;
  const int64_t n = spin_measure_rows(a);
  SpinSectorTables t;
  if (sector && a.n_flip > 0) spin_sector_build_tables(a.n_sites, a.n_up, t);
  std::vector<double> dg((size_t)a.n_diag, 0.0), fl((size_t)a.n_flip, 0.0);
  double nrm = 0.0;
  for (int64_t r = 0; r < n; ++r) {
    const uint32_t s = sector ? spin_sector_unrank(a.n_sites, a.n_up, r) : (uint32_t)r;
    const double xr = x[2 * r], xi = x[2 * r + 1];
    nrm = std::fma(xr, xr, nrm);
    nrm = std::fma(xi, xi, nrm);
    for (int i = 0; i < a.n_diag; ++i) {
      const bool neg = spin_parity(~s & a.diag_masks[i]);
      dg[(size_t)i] = std::fma(neg ? -xr : xr, xr, dg[(size_t)i]);
      dg[(size_t)i] = std::fma(neg ? -xi : xi, xi, dg[(size_t)i]);
    }
    for (int i = 0; i < a.n_flip; ++i) {
      const uint32_t m = a.flip_masks[i];
      if ((m & (m - 1)) != 0 && !spin_parity(s & m)) continue;  // a pair with equal spins has no entry
      const uint32_t s2 = s ^ m;
      const int64_t r2 = sector ? (int64_t)spin_sector_rank(t, s2) : (int64_t)s2;
      fl[(size_t)i] = std::fma(xr, x[2 * r2], fl[(size_t)i]);
      fl[(size_t)i] = std::fma(xi, x[2 * r2 + 1], fl[(size_t)i]);
    }
  }
  for (int i = 0; i < a.n_diag && diag_out; ++i) diag_out[i] = dg[(size_t)i];
  for (int i = 0; i < a.n_flip && flip_out; ++i) flip_out[i] = fl[(size_t)i];
  if (norm2) *norm2 = nrm;
}

}  // namespace eigenex
