// The spin-1/2 Hamiltonian of spin_model.hpp in one momentum sector of one sector of fixed magnetisation (host side, no HIP).
// Shared by the library (eigenex_spin_momentum_*) and by the host program tests/cpp/spin_momentum_sanitize.cpp, which runs this
// file under AddressSanitizer + UBSan.
//
// Translation.  cell = a divides L = n_sites and 1 <= a <= L/2; N = L / a is the number of translations.  T moves site i to site
//   (i + a) mod L: on a state word a left rotation of the low L bits by a, ((s << a) | (s >> (L - a))) & site_mask, whose two
//   shifts are 1..31 for every L up to 32.
// Model.  Accepted if it conserves Sz (spin_sector_error) and is invariant under T: the multiset of (unordered bond, jz, jxy),
//   couplings compared bit for bit, maps onto itself, and hz[i] == hz[(i + a) mod L].  Otherwise refused with a message that names
//   the first bond or site that breaks the symmetry.
// Sector (L, n_up, cell, m), 0 <= m < N, k = 2 pi m / N.  A state s has orbit period R_s, the smallest R >= 1 with T^R s = s; it
//   divides N.  The representative of an orbit is its numerically smallest state.  The rows are the representatives a of the Sz
//   sector with (m R_a) mod N == 0, ascending; idx(a) is the row of a.  dim < 2^31 always.  A sector without such a state is refused.
// Basis.  |a(k)> = (sqrt(R_a) / N) sum_{r=0}^{N-1} e^{-ikr} T^r |a>.
// Row a of H_k, in stored (= summation) order:
//   1. the diagonal, always stored, column idx(a): the full-space diagonal d(a) of spin_model.hpp, the same constants in the same order
//   2. for b ascending over the bonds with jxy[b] != 0 and different spins on the bond: s' = a ^ mask_b; j* the smallest j >= 0
//      with T^j s' = rep(s'); l = (N - j*) mod N.  If (m R_s') mod N != 0 the term is absent, otherwise the value is c * phase[l]
//      at column idx(rep(s')), with c = (jxy[b] * 0.5) * ratio[R_a][R_s'], each product rounded, and value.re = c * phase.re,
//      value.im = c * phase.im
//   3. terms are never merged: two terms of a row that reach the same column stay two entries
//   ratio[p][q] = sqrt((double)p / (double)q);  phase[l] = e^{-2 pi i ((m l) mod N) / N}, exactly (1,0), (0,-1), (-1,0), (0,1)
//   where 4 ((m l) mod N) is a multiple of N;  inv_sqrt[q] = 1 / sqrt((double)q).  One function builds all three
//   (spin_momentum_build_tables), for the CSR writer, the upload and expand alike.
// A momentum is real when m == 0 or 2 m == N: every phase.im is then exactly 0 and H_k is real symmetric.
// expand maps a momentum vector x to the Sz-sector vector y: for every sector state s, with b = rep(s) = T^{j*} s,
//   y[rank(s)] = x[idx(b)] * phase[(N - j*) mod N] * inv_sqrt[R_b] if b is compatible with m, else 0.  The first product is a plain
//   complex multiply without contraction (of real vectors x * phase.re), the second scales each part.  It preserves the norm.
// Lookup idx(b): the ascending list reps[dim] and bucket[2^(L-h) + 1], h = (L + 1) / 2: bucket[hi] is the index of the first
//   representative whose high L - h bits are >= hi; idx(b) is the lower bound of b in reps[bucket[b >> h] .. bucket[(b >> h) + 1]).
//   The kernels search with a fixed trip count, steps = ceil(log2(largest bucket + 1)) (spin_rows.hpp: spin_momentum_index); the
//   functions in this file use std::lower_bound over the whole list and share nothing with that walk.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "spin_sector.hpp"

namespace eigenex {

constexpr int kMomentumMaxPeriod = kSectorMaxSites;             // N <= L <= 32
constexpr int kMomentumRatioPitch = kMomentumMaxPeriod + 1;     // ratio[p * pitch + q], 0 <= p, q <= 32 (row and column 0 unused)

// ratio, inv_sqrt and phase of one (N, m)
struct SpinMomentumTables {
  double ratio[kMomentumRatioPitch * kMomentumRatioPitch];
  double inv_sqrt[kMomentumRatioPitch];
  double phase_re[kMomentumMaxPeriod], phase_im[kMomentumMaxPeriod];
};

// The kernels' form of the sector (device memory, owned by the shard; reps and bucket are separate arrays)
struct SpinMomentumView {
  SpinOperatorView model;  // no transverse field: every flip mask has two bits
  int n_up, cell, n_trans, momentum;
  int h, steps;            // bucket index = state >> h; trip count of the search
  uint32_t site_mask;      // the low n_sites bits
  uint32_t compatible;     // bit R - 1: (momentum * R) mod n_trans == 0
  uint32_t first_rep, pad; // reps[0]: what a lane of expand without a compatible representative looks up
  SpinMomentumTables tab;
};

// the rows of one sector and their lookup
struct SpinMomentumBasis {
  int n_sites = 0, n_up = 0, cell = 0, n_trans = 0, momentum = 0, h = 0, steps = 0;
  std::vector<uint32_t> reps;    // ascending
  std::vector<uint8_t> period;   // of each representative
  std::vector<uint32_t> bucket;  // 2^(n_sites - h) + 1 entries
};

inline uint32_t spin_momentum_site_mask(int n_sites) { return 0xffffffffu >> (32 - n_sites); }

// T s
inline uint32_t spin_momentum_translate(uint32_t s, int n_sites, int cell) {
  return ((s << cell) | (s >> (n_sites - cell))) & spin_momentum_site_mask(n_sites);
}

// "" if (n_sites, n_up, cell, momentum) names a sector (that may still be empty), else what is wrong
inline std::string spin_momentum_geometry_error(int n_sites, int n_up, int cell, int momentum) {
  if (n_sites < kSpinMinSites || n_sites > kSectorMaxSites) return "n_sites must be 2..32";
  if (n_up < 0 || n_up > n_sites) return "n_up must be 0..n_sites";
  if (cell < 1 || n_sites % cell != 0) return "cell must be at least 1 and divide n_sites";
  if (cell > n_sites / 2) return "cell must be at most n_sites / 2: a translation by the whole ring is no symmetry to use";
  if (momentum < 0 || momentum >= n_sites / cell) return "momentum must be 0..n_sites/cell - 1";
  return "";
}

// "" if the model conserves Sz and is invariant under the translation by `cell` sites (a valid geometry is assumed)
inline std::string spin_momentum_invariance_error(const SpinModelArgs& a, int cell);
inline std::string spin_momentum_model_error(const SpinModelArgs& a, int n_up, int cell) {
  if (const char* why = spin_sector_error(a, n_up)) return why;
  return spin_momentum_invariance_error(a, cell);
}
// the invariance half of the check, of a model whose sites and bonds are valid: shared with spin_momentum64.hpp
inline std::string spin_momentum_invariance_error(const SpinModelArgs& a, int cell) {
  struct Bond {
    int lo, hi;
    uint64_t jz, jxy;
    bool operator==(const Bond& o) const { return lo == o.lo && hi == o.hi && jz == o.jz && jxy == o.jxy; }
  };
  const auto bits = [](double v) {
    uint64_t u;
    memcpy(&u, &v, 8);
    return u;
  };
  std::vector<Bond> bonds, moved;
  for (int b = 0; b < a.n_bonds; ++b) {
    const int i = a.site_i[b], j = a.site_j[b], ti = (i + cell) % a.n_sites, tj = (j + cell) % a.n_sites;
    bonds.push_back(Bond{std::min(i, j), std::max(i, j), bits(a.jz[b]), bits(a.jxy[b])});
    moved.push_back(Bond{std::min(ti, tj), std::max(ti, tj), bits(a.jz[b]), bits(a.jxy[b])});
  }
  for (int b = 0; b < a.n_bonds; ++b)  // T maps the multiset onto itself iff every bond and its image occur equally often
    if (std::count(bonds.begin(), bonds.end(), bonds[b]) != std::count(bonds.begin(), bonds.end(), moved[b]))
      return "the model is not invariant under the translation by cell sites: bond " + std::to_string(b) + " (sites " + std::to_string(a.site_i[b]) +
             ", " + std::to_string(a.site_j[b]) + ") has no image with the same couplings on sites " + std::to_string(moved[b].lo) + ", " +
             std::to_string(moved[b].hi);
  if (a.hz)
    for (int i = 0; i < a.n_sites; ++i)
      if (a.hz[i] != a.hz[(i + cell) % a.n_sites])
        return "the model is not invariant under the translation by cell sites: hz at site " + std::to_string(i) + " differs from hz at site " +
               std::to_string((i + cell) % a.n_sites);
  return "";
}

inline bool spin_momentum_is_real(int n_trans, int momentum) { return momentum == 0 || 2 * momentum == n_trans; }

// Walks the states of the Sz sector in ascending order and calls f(state) for each (Gosper's successor in 64 bits: no overflow at 32 sites)
template <class F>
inline void spin_momentum_for_each_state(int n_sites, int n_up, F f) {
  if (n_up == 0) {
    f(uint32_t(0));
    return;
  }
  const uint64_t end = uint64_t(1) << n_sites;
  for (uint64_t s = (uint64_t(1) << n_up) - 1; s < end;) {
    f((uint32_t)s);
    const uint64_t c = s & (~s + 1), r = s + c;
    s = (((r ^ s) >> 2) / c) | r;
  }
}

// Is s the smallest state of its orbit?  Rotates with an exit at the first smaller rotation; *period is set for a representative.
inline bool spin_momentum_is_representative(uint32_t s, int n_sites, int cell, int n_trans, int* period) {
  uint32_t t = s;
  for (int r = 1; r <= n_trans; ++r) {
    t = spin_momentum_translate(t, n_sites, cell);
    if (t < s) return false;
    if (t == s) {
      *period = r;
      return true;
    }
  }
  return false;  // not reached: T^N is the identity
}

// The rows of the sector of a valid geometry; returns their number.  basis == nullptr: the count alone, nothing is stored.
inline int64_t spin_momentum_build_basis(int n_sites, int n_up, int cell, int momentum, SpinMomentumBasis* basis) {
  const int n_trans = n_sites / cell;
  int64_t count = 0;
  if (basis) {
    *basis = SpinMomentumBasis();
    basis->n_sites = n_sites, basis->n_up = n_up, basis->cell = cell, basis->n_trans = n_trans, basis->momentum = momentum;
    basis->h = (n_sites + 1) / 2;
  }
  spin_momentum_for_each_state(n_sites, n_up, [&](uint32_t s) {
    int period = 0;
    if (!spin_momentum_is_representative(s, n_sites, cell, n_trans, &period) || (momentum * period) % n_trans != 0) return;
    ++count;
    if (basis) basis->reps.push_back(s), basis->period.push_back((uint8_t)period);
  });
  if (basis) {
    const size_t nb = size_t(1) << (n_sites - basis->h);
    basis->bucket.assign(nb + 1, 0);
    size_t i = 0, largest = 0;
    for (size_t hi = 0; hi <= nb; ++hi) {  // bucket[hi]: the first representative whose high bits are >= hi
      while (i < basis->reps.size() && (size_t)(basis->reps[i] >> basis->h) < hi) ++i;
      basis->bucket[hi] = (uint32_t)i;
      if (hi > 0) largest = std::max(largest, (size_t)(basis->bucket[hi] - basis->bucket[hi - 1]));
    }
    while ((size_t(1) << basis->steps) < largest + 1) ++basis->steps;  // ceil(log2(largest + 1))
  }
  return count;
}

inline void spin_momentum_build_tables(int n_trans, int momentum, SpinMomentumTables& t) {
  t = SpinMomentumTables();
  for (int p = 1; p <= kMomentumMaxPeriod; ++p)
    for (int q = 1; q <= kMomentumMaxPeriod; ++q) t.ratio[p * kMomentumRatioPitch + q] = std::sqrt((double)p / (double)q);
  for (int q = 1; q <= kMomentumMaxPeriod; ++q) t.inv_sqrt[q] = 1.0 / std::sqrt((double)q);
  for (int l = 0; l < n_trans; ++l) {
    const int q = (momentum * l) % n_trans;
    if ((4 * q) % n_trans == 0) {
      static const double re[4] = {1.0, 0.0, -1.0, 0.0}, im[4] = {0.0, -1.0, 0.0, 1.0};
      t.phase_re[l] = re[4 * q / n_trans], t.phase_im[l] = im[4 * q / n_trans];
    } else {
      const double angle = (6.283185307179586476925286766559 * (double)q) / (double)n_trans;  // 2 pi q / N
      t.phase_re[l] = std::cos(angle), t.phase_im[l] = -std::sin(angle);
    }
  }
}

// the kernels' view of a valid model on a built basis
inline void spin_momentum_build_view(const SpinModelArgs& a, const SpinMomentumBasis& b, SpinMomentumView& v) {
  SpinModelArgs z = a;
  z.hx = nullptr;
  spin_build_view(z, v.model);
  v.n_up = b.n_up, v.cell = b.cell, v.n_trans = b.n_trans, v.momentum = b.momentum, v.h = b.h, v.steps = b.steps;
  v.site_mask = spin_momentum_site_mask(b.n_sites);
  v.compatible = 0;
  for (int r = 1; r <= b.n_trans; ++r)
    if ((b.momentum * r) % b.n_trans == 0) v.compatible |= uint32_t(1) << (r - 1);
  v.first_rep = b.reps.empty() ? 0u : b.reps[0];
  v.pad = 0;
  spin_momentum_build_tables(b.n_trans, b.momentum, v.tab);
}

// the orbit of any state, from the definition: the representative, the smallest j >= 0 with T^j s = rep(s), and the period
struct SpinMomentumOrbit {
  uint32_t rep;
  int j, period;
};
inline SpinMomentumOrbit spin_momentum_orbit_host(uint32_t s, int n_sites, int cell) {
  SpinMomentumOrbit o = {s, 0, 0};
  uint32_t t = s;
  for (int r = 1;; ++r) {
    t = spin_momentum_translate(t, n_sites, cell);
    if (t == s) {
      o.period = r;
      return o;
    }
    if (t < o.rep) o.rep = t, o.j = r;
  }
}

// idx(b) of a representative of the sector, -1 for any other state
inline int64_t spin_momentum_row_of(const SpinMomentumBasis& b, uint32_t rep) {
  const auto it = std::lower_bound(b.reps.begin(), b.reps.end(), rep);
  return it != b.reps.end() && *it == rep ? (int64_t)(it - b.reps.begin()) : -1;
}

// Rows [row_begin, row_begin + n_rows) of a valid model as CSR, the signature of spin_write_rows with val interleaved (re, im):
// rowptr[n_rows + 1] and *nnz always; col and val unless both are NULL.  Written from the definition at the top.
inline void spin_momentum_write_rows(const SpinModelArgs& a, const SpinMomentumBasis& basis, const SpinMomentumTables& t, int64_t row_begin,
                                     int64_t n_rows, int64_t* rowptr, int32_t* col, double* val, int64_t* nnz) {
  const int L = basis.n_sites, N = basis.n_trans;
  int64_t p = 0;
  rowptr[0] = 0;
  for (int64_t k = 0; k < n_rows; ++k) {
    const uint32_t s = basis.reps[(size_t)(row_begin + k)];
    const int period = basis.period[(size_t)(row_begin + k)];
    if (col) {
      double d = 0.0;
      for (int b = 0; b < a.n_bonds; ++b) {
        const double c = a.jz[b] * 0.25;
        d += (((s >> a.site_i[b]) ^ (s >> a.site_j[b])) & 1u) ? -c : c;
      }
      if (a.hz)
        for (int i = 0; i < L; ++i) {
          const double c = a.hz[i] * 0.5;
          d += ((s >> i) & 1u) ? c : -c;
        }
      col[p] = (int32_t)(row_begin + k), val[2 * p] = d, val[2 * p + 1] = 0.0;
    }
    ++p;
    for (int b = 0; b < a.n_bonds; ++b)
      if (a.jxy[b] != 0.0 && (((s >> a.site_i[b]) ^ (s >> a.site_j[b])) & 1u)) {
        const uint32_t s2 = s ^ ((uint32_t(1) << a.site_i[b]) | (uint32_t(1) << a.site_j[b]));
        const SpinMomentumOrbit o = spin_momentum_orbit_host(s2, L, basis.cell);
        if ((basis.momentum * o.period) % N != 0) continue;
        if (col) {
          const int l = (N - o.j) % N;
          const double half = a.jxy[b] * 0.5;
          const double c = half * t.ratio[period * kMomentumRatioPitch + o.period];
          col[p] = (int32_t)spin_momentum_row_of(basis, o.rep);
          val[2 * p] = c * t.phase_re[l], val[2 * p + 1] = c * t.phase_im[l];
        }
        ++p;
      }
    rowptr[k + 1] = p;
  }
  *nnz = p;
}

// y = expand(x): x has basis.reps.size() entries, y C(n_sites, n_up), each one double (is_complex false; a real momentum) or an
// interleaved pair.  From the definition; the rank of a sector state is its place in the ascending walk.
inline void spin_momentum_expand_host(const SpinMomentumBasis& basis, const SpinMomentumTables& t, bool is_complex, const double* x, double* y) {
  const int L = basis.n_sites, N = basis.n_trans;
  int64_t rank = 0;
  spin_momentum_for_each_state(L, basis.n_up, [&](uint32_t s) {
#if defined(__clang__)
#pragma clang fp contract(off)  // a host compiler other than clang needs -ffp-contract=off, as for add_product_nofma
#endif
    const SpinMomentumOrbit o = spin_momentum_orbit_host(s, L, basis.cell);
    const int64_t row = (basis.momentum * o.period) % N == 0 ? spin_momentum_row_of(basis, o.rep) : -1;
    const int l = (N - o.j) % N;
    const double w = t.inv_sqrt[o.period];
    if (!is_complex) {
      y[rank] = row < 0 ? 0.0 : (x[row] * t.phase_re[l]) * w;
    } else if (row < 0) {
      y[2 * rank] = 0.0, y[2 * rank + 1] = 0.0;
    } else {
      const double xr = x[2 * row], xi = x[2 * row + 1];
      const double a = xr * t.phase_re[l], b = xi * t.phase_im[l], c = xr * t.phase_im[l], d = xi * t.phase_re[l];  // each product rounded
      const double re = a - b, im = c + d;
      y[2 * rank] = re * w, y[2 * rank + 1] = im * w;
    }
    ++rank;
  });
}

}  // namespace eigenex
