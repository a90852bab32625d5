// The spin-1/2 Hamiltonian of spin_model.hpp in one sector of fixed magnetisation (host side, no HIP): the states of n_sites
// sites with exactly n_up sites up, in ascending numerical order.  Row and column r is the rank of state s in that order;
// row r is row s = unrank(r) of the full-space definition at the top of spin_model.hpp -- the same terms, constants and order
// -- with every column s' replaced by rank(s').  A bond flip keeps the number of up spins, so every column is in the sector;
// a transverse field does not, so hx must be absent.  Shared by the library (eigenex_spin_sector_*) and by the host program
// tests/cpp/spin_sector_sanitize.cpp, which runs this file under AddressSanitizer + UBSan.
//
//   dim    = C(n_sites, n_up) <= C(32, 16) = 601,080,390 < 2^31: 32-bit columns hold for every sector of up to 32 sites
//   unrank : combinadic.  k = n_up; for p = n_sites-1 .. 0: if k > 0 and r >= C(p, k): set bit p, r -= C(p, k), --k
//   rank   : two tables (Lin tables).  With h = (n_sites + 1) / 2 low bits:  rank(s) = hi_base[s >> h] + lo_rank[s & (2^h - 1)]
//            lo_rank[lo] = rank of lo among the h-bit words of its own popcount
//            hi_base[hi] = number of sector states whose high part is below hi
#pragma once
#include <stdint.h>

#include <vector>

#include "spin_model.hpp"

namespace eigenex {

constexpr int kSectorMaxSites = 32;
static_assert(kSpinMaxBonds + kSectorMaxSites <= kSpinMaxTerms, "the diagonal table holds 64 bonds and hz on 32 sites");

// C(n, k) for 0 <= n, k <= 32 by Pascal's rule in 64 bits (the largest entry is C(32, 16): no sum overflows); 0 where k > n
struct SpinBinomials {
  uint64_t c[kSectorMaxSites + 1][kSectorMaxSites + 1];
  SpinBinomials() {
    for (int n = 0; n <= kSectorMaxSites; ++n)
      for (int k = 0; k <= kSectorMaxSites; ++k) c[n][k] = k == 0 ? 1 : (n == 0 ? 0 : c[n - 1][k - 1] + c[n - 1][k]);
  }
};

// The kernel's form of the sector (device memory, owned by the shard): the model's tables, and C(p, k) for the unranking --
// bit positions p = 0..31, k = 0..32 up spins still to place (0 where k > p: a state that must fill every remaining site).
// Every entry is below 2^32: C(31, 15).
struct SpinSectorView {
  SpinOperatorView model;  // no transverse field: every flip mask has two bits
  int n_up, h;             // h low bits index lo_rank, the n_sites - h bits above them index hi_base
  uint32_t lo_mask, pad;
  uint32_t binom[kSectorMaxSites][kSectorMaxSites + 1];
};

// the two rank tables of one sector: 2^h and 2^(n_sites - h) entries
struct SpinSectorTables {
  int n_sites = 0, n_up = 0, h = 0;
  std::vector<uint32_t> lo_rank, hi_base;
};

// nullptr if (model, n_up) describes a sector, else what is wrong with it
inline const char* spin_sector_error(const SpinModelArgs& a, int n_up) {
  if (const char* why = spin_model_error(a, kSectorMaxSites)) return why;
  if (n_up < 0 || n_up > a.n_sites) return "n_up must be 0..n_sites";
  if (a.hx)
    for (int i = 0; i < a.n_sites; ++i)
      if (a.hx[i] != 0.0) return "a transverse field (hx != 0) does not conserve Sz: the model has no fixed-magnetisation sector";
  return nullptr;
}

inline int64_t spin_sector_dim(int n_sites, int n_up) {
  static const SpinBinomials b;
  return n_sites < 0 || n_sites > kSectorMaxSites || n_up < 0 || n_up > n_sites ? 0 : (int64_t)b.c[n_sites][n_up];
}

// the state of rank r, 0 <= r < dim
inline uint32_t spin_sector_unrank(int n_sites, int n_up, int64_t r) {
  static const SpinBinomials b;
  uint32_t s = 0;
  uint64_t left = (uint64_t)r;
  int k = n_up;
  for (int p = n_sites - 1; p >= 0; --p)
    if (k > 0 && left >= b.c[p][k]) s |= uint32_t(1) << p, left -= b.c[p][k], --k;
  return s;
}

inline void spin_sector_build_tables(int n_sites, int n_up, SpinSectorTables& t) {
  static const SpinBinomials b;
  t.n_sites = n_sites, t.n_up = n_up, t.h = (n_sites + 1) / 2;
  const int hbits = n_sites - t.h;
  t.lo_rank.assign(size_t(1) << t.h, 0);
  t.hi_base.assign(size_t(1) << hbits, 0);
  uint32_t seen[kSectorMaxSites + 1] = {0};  // h-bit words met so far, by popcount
  for (uint32_t lo = 0; lo < t.lo_rank.size(); ++lo) t.lo_rank[lo] = seen[__builtin_popcount(lo)]++;
  uint64_t below = 0;
  for (uint32_t hi = 0; hi < t.hi_base.size(); ++hi) {
    t.hi_base[hi] = (uint32_t)below;
    const int need = n_up - __builtin_popcount(hi);  // up spins the low part has to hold
    if (need >= 0 && need <= t.h) below += b.c[t.h][need];
  }
}

// the rank of a state of the sector
inline uint32_t spin_sector_rank(const SpinSectorTables& t, uint32_t s) {
  return t.hi_base[s >> t.h] + t.lo_rank[s & ((uint32_t(1) << t.h) - 1)];
}

// the kernel's view of a valid sector (the model without its transverse field, which is absent or all zeros)
inline void spin_sector_build_view(const SpinModelArgs& a, int n_up, SpinSectorView& v) {
  static const SpinBinomials b;
  SpinModelArgs z = a;
  z.hx = nullptr;
  spin_build_view(z, v.model);
  v.n_up = n_up, v.h = (a.n_sites + 1) / 2, v.lo_mask = (uint32_t(1) << v.h) - 1, v.pad = 0;
  for (int p = 0; p < kSectorMaxSites; ++p)
    for (int k = 0; k <= kSectorMaxSites; ++k) v.binom[p][k] = (uint32_t)b.c[p][k];
}

// Rows [row_begin, row_begin + n_rows) of a valid sector (ranks) as CSR, the signature of spin_write_rows: rowptr[n_rows + 1]
// and *nnz always; col and val unless both are NULL.  Each row is written by spin_write_rows itself, as row unrank(r) of the
// full space, and its columns are then ranked: the sector CSR is the full-space CSR restricted to the sector, bit for bit.
inline void spin_sector_write_rows(const SpinModelArgs& a, const SpinSectorTables& t, int64_t row_begin, int64_t n_rows, int64_t* rowptr,
                                   int32_t* col, double* val, int64_t* nnz) {
  SpinModelArgs z = a;
  z.hx = nullptr;
  int64_t p = 0;
  rowptr[0] = 0;
  for (int64_t k = 0; k < n_rows; ++k) {
    const uint32_t s = spin_sector_unrank(t.n_sites, t.n_up, row_begin + k);
    int64_t one[2], count = 0;
    spin_write_rows(z, (int64_t)s, 1, one, col ? col + p : nullptr, col ? val + p : nullptr, &count);
    if (col)
      for (int64_t q = p; q < p + count; ++q) col[q] = (int32_t)spin_sector_rank(t, (uint32_t)col[q]);
    p += count;
    rowptr[k + 1] = p;
  }
  *nnz = p;
}

}  // namespace eigenex
