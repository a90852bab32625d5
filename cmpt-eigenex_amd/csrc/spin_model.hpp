// Spin-1/2 Hamiltonian on n_sites sites, full Hilbert space (host side, no HIP): the argument checks, the rows as CSR and the
// tables of the matrix-free kernel (kernels.hip: k_spin_spmv).  Shared by the library (eigenex_spin_csr, eigenex_spin_upload)
// and by the host program tests/cpp/spin_model_sanitize.cpp, which runs this file under AddressSanitizer + UBSan.
//
//   H = sum_b [ Jz_b Sz_i Sz_j + (Jxy_b/2)(S+_i S-_j + S-_i S+_j) ] + sum_i hz_i Sz_i + sum_i hx_i Sx_i
//
// Basis state s has site i up iff bit i of s is set.  Row s, in stored (= summation) order:
//   1. the diagonal, always stored, column s:  d = 0.0; for b ascending  d += (spins of bond b equal ? +1 : -1) * (Jz_b * 0.25);
//      for i ascending  d += (site i up ? +1 : -1) * (hz_i * 0.5)        -- plain additions of sign-flipped constants
//   2. for b ascending with Jxy_b != 0 and different spins on the bond:  value Jxy_b * 0.5, column s ^ (1<<i_b | 1<<j_b)
//   3. for i ascending with hx_i != 0:                                   value hx_i * 0.5,  column s ^ (1<<i)
#pragma once
#include <stdint.h>

#include <cmath>

namespace eigenex {

constexpr int kSpinMinSites = 2, kSpinMaxSites = 30, kSpinMaxBonds = 64, kSpinBatch = 8;
constexpr int kSpinMaxTerms = (kSpinMaxBonds + kSpinMaxSites + kSpinBatch - 1) / kSpinBatch * kSpinBatch;

// The kernel's form of the model (device memory, owned by the shard; every lane reads the same entry):
//   diagonal  d = 0.0, then for t < ndiag:  d += parity(s & dmask[t]) ? -dval[t] : dval[t]
//             bond b is (1<<i | 1<<j, Jz_b * 0.25): equal spins have even parity; field hz_i is (1<<i, -(hz_i * 0.5)): up is odd
//   flip t < nflip:  column s ^ fmask[t], value fval[t]; a two-bit mask (bond) only where parity(s & fmask[t]) is odd, a
//             one-bit mask (transverse field) on every row
// Both tables are padded with (mask 0, value 0.0) up to kSpinMaxTerms, a multiple of kSpinBatch: a zero mask never flips.
struct SpinOperatorView {
  int n_sites, ndiag, nflip, pad;
  uint32_t dmask[kSpinMaxTerms], fmask[kSpinMaxTerms];
  double dval[kSpinMaxTerms], fval[kSpinMaxTerms];
};

struct SpinModelArgs {
  int n_sites, n_bonds;
  const int32_t *site_i, *site_j;
  const double *jz, *jxy, *hz, *hx;  // hz, hx: n_sites entries or NULL
};

// nullptr if the model is valid, else what is wrong with it.  max_sites: 30 for the full space, 32 for a sector (spin_sector.hpp)
inline const char* spin_model_error(const SpinModelArgs& a, int max_sites = kSpinMaxSites) {
  if (a.n_sites < kSpinMinSites || a.n_sites > max_sites) return max_sites == kSpinMaxSites ? "n_sites must be 2..30" : "n_sites must be 2..32";
  if (a.n_bonds < 0 || a.n_bonds > kSpinMaxBonds) return "n_bonds must be 0..64";
  if (a.n_bonds > 0 && (!a.site_i || !a.site_j || !a.jz || !a.jxy)) return "site_i, site_j, jz or jxy is NULL";
  for (int b = 0; b < a.n_bonds; ++b) {
    if (a.site_i[b] < 0 || a.site_i[b] >= a.n_sites || a.site_j[b] < 0 || a.site_j[b] >= a.n_sites) return "a bond names a site outside 0..n_sites-1";
    if (a.site_i[b] == a.site_j[b]) return "a bond joins a site to itself";
    if (!std::isfinite(a.jz[b]) || !std::isfinite(a.jxy[b])) return "a coupling is not finite";
  }
  for (int i = 0; i < a.n_sites; ++i)
    if ((a.hz && !std::isfinite(a.hz[i])) || (a.hx && !std::isfinite(a.hx[i]))) return "a field is not finite";
  return nullptr;
}

inline void spin_build_view(const SpinModelArgs& a, SpinOperatorView& v) {
  v = SpinOperatorView();
  v.n_sites = a.n_sites;
  for (int b = 0; b < a.n_bonds; ++b) {
    const uint32_t m = (uint32_t(1) << a.site_i[b]) | (uint32_t(1) << a.site_j[b]);
    v.dmask[v.ndiag] = m, v.dval[v.ndiag++] = a.jz[b] * 0.25;
    if (a.jxy[b] != 0.0) v.fmask[v.nflip] = m, v.fval[v.nflip++] = a.jxy[b] * 0.5;
  }
  for (int i = 0; i < a.n_sites; ++i) {
    if (a.hz) v.dmask[v.ndiag] = uint32_t(1) << i, v.dval[v.ndiag++] = -(a.hz[i] * 0.5);
    if (a.hx && a.hx[i] != 0.0) v.fmask[v.nflip] = uint32_t(1) << i, v.fval[v.nflip++] = a.hx[i] * 0.5;
  }
}

inline int spin_parity(uint32_t x) {
  x ^= x >> 16, x ^= x >> 8, x ^= x >> 4, x ^= x >> 2, x ^= x >> 1;
  return (int)(x & 1u);
}

// Rows [row_begin, row_begin + n_rows) of a valid model as CSR: rowptr[n_rows + 1] (starting at 0) and *nnz always; col and val
// (global columns) unless both are NULL.  Written from the definition at the top, not from the kernel's tables.
inline void spin_write_rows(const SpinModelArgs& a, int64_t row_begin, int64_t n_rows, int64_t* rowptr, int32_t* col, double* val,
                            int64_t* nnz) {
  int64_t p = 0;
  rowptr[0] = 0;
  for (int64_t k = 0; k < n_rows; ++k) {
    const uint32_t s = (uint32_t)(row_begin + k);
    if (col) {
      double d = 0.0;
      for (int b = 0; b < a.n_bonds; ++b) {
        const double c = a.jz[b] * 0.25;
        d += (((s >> a.site_i[b]) ^ (s >> a.site_j[b])) & 1u) ? -c : c;
      }
      if (a.hz)
        for (int i = 0; i < a.n_sites; ++i) {
          const double c = a.hz[i] * 0.5;
          d += ((s >> i) & 1u) ? c : -c;
        }
      col[p] = (int32_t)s, val[p] = d;
    }
    ++p;
    for (int b = 0; b < a.n_bonds; ++b)
      if (a.jxy[b] != 0.0 && (((s >> a.site_i[b]) ^ (s >> a.site_j[b])) & 1u)) {
        if (col) col[p] = (int32_t)(s ^ ((uint32_t(1) << a.site_i[b]) | (uint32_t(1) << a.site_j[b]))), val[p] = a.jxy[b] * 0.5;
        ++p;
      }
    if (a.hx)
      for (int i = 0; i < a.n_sites; ++i)
        if (a.hx[i] != 0.0) {
          if (col) col[p] = (int32_t)(s ^ (uint32_t(1) << i)), val[p] = a.hx[i] * 0.5;
          ++p;
        }
    rowptr[k + 1] = p;
  }
  *nnz = p;
}

}  // namespace eigenex
