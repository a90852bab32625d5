// The momentum sectors of spin_momentum.hpp on rings of up to 48 sites: the same sector with 64-bit state words (host side, no
// HIP).  Shared by the library (eigenex_spin_momentum64_*, eigenex_spin_momentum_measure*) and by the host program
// tests/cpp/spin_momentum64_sanitize.cpp, which runs this file under AddressSanitizer + UBSan.
//
// Rows, basis, row contents, summation order, ratio, phase, inv_sqrt, the "real momentum" rule and the invariance check are the
// text at the top of spin_momentum.hpp, word for word.  Only the widths change:
//   n_sites 2..48, n_bonds 0..128 (a J1-J2 ring of 36 sites has 72), dim < 2^31 still; a state is a uint64_t, site i at bit i
//   the two shifts of a rotation are 1..47; `compatible` has 48 bits; the ratio pitch is 49
//   the bucket table has 2^(L - h) + 1 words with h = (L + 1) / 2, at most 2^24 + 1
//   the model's view has 64-bit masks and term tables for 128 bonds and 48 fields (SpinOperatorView64)
// For n_sites <= 32 and n_bonds <= 64 every function here returns what its 32-bit namesake returns.
//
// Enumeration.  The plain walk visits C(L, n_up) states, 9.1e9 at (36, 18).  Here the sector is cut by the top bits of the state
// into chunks that up to 16 threads take in turn and that are joined in ascending order, so the list is the plain walk's.  A chunk
// is skipped where its prefix p of tb bits alone shows that a rotation is smaller: for every multiple c of cell below tb, the
// top tb - c bits of T^(c/cell) s are the low tb - c bits of p and those of s are p >> c; if the first are smaller, no state of
// the chunk is a representative.  About one prefix in eight survives at cell = 1.
//
// Diagonal correlations (eigenex_spin_momentum_measure; kernels.hip: k_spin_momentum_measure<E, Word>).  In a momentum eigenstate
// x of the sector, <D> of a product D of sigma^z over a site mask needs no expansion: D is diagonal and distinct orbits are
// disjoint, so  <D> = sum_a |x_a|^2 (1/N) sum_{r<N} D(T^r a)  over the representatives a.  The raw sums are
//   norm2   = sum_a |x_a|^2                      one fma per row of a real x (x, x), two of a complex one (re, then im)
//   diag[t] = sum_a c_t(a) w_a                   one fma per row: fma((double)c_t(a), w_a, diag[t])
//   w_a     = x_a * x_a, of a complex element fma(im, im, re * re)
//   c_t(a)  = sum_{r<N} prod_{i in mask_t} sigma_i(T^r a), an integer in [-N, N]; sigma_i(s) = +1 if bit i of s is set, else -1
// rows ascending, so that <D_t> = diag[t] / (N norm2).  Masks are 64-bit; 1..1024 of them, none zero, none with a site >= n_sites.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <string>
#include <thread>
#include <vector>

#include "spin_measure.hpp"
#include "spin_momentum.hpp"

namespace eigenex {

constexpr int kMomentum64MaxSites = 48, kMomentum64MaxBonds = 128;
constexpr int kMomentum64MaxTerms = (kMomentum64MaxBonds + kMomentum64MaxSites + kSpinBatch - 1) / kSpinBatch * kSpinBatch;
constexpr int kMomentum64MaxPeriod = kMomentum64MaxSites;
constexpr int kMomentum64RatioPitch = kMomentum64MaxPeriod + 1;
constexpr int kMomentum64Threads = 16;
constexpr int64_t kMomentum64MaxDim = (int64_t(1) << 31) - 1;

// SpinOperatorView (spin_model.hpp) with 64-bit masks; no transverse field, so every flip mask has two bits
struct SpinOperatorView64 {
  int n_sites, ndiag, nflip, pad;
  uint64_t dmask[kMomentum64MaxTerms], fmask[kMomentum64MaxTerms];
  double dval[kMomentum64MaxTerms], fval[kMomentum64MaxTerms];
};

struct SpinMomentum64Tables {
  double ratio[kMomentum64RatioPitch * kMomentum64RatioPitch];
  double inv_sqrt[kMomentum64RatioPitch];
  double phase_re[kMomentum64MaxPeriod], phase_im[kMomentum64MaxPeriod];
};

struct SpinMomentum64View {
  SpinOperatorView64 model;
  int n_up, cell, n_trans, momentum;
  int h, steps;
  uint64_t site_mask, compatible, first_rep;
  SpinMomentum64Tables tab;
};

struct SpinMomentum64Basis {
  int n_sites = 0, n_up = 0, cell = 0, n_trans = 0, momentum = 0, h = 0, steps = 0;
  std::vector<uint64_t> reps;    // ascending
  std::vector<uint8_t> period;   // of each representative
  std::vector<uint32_t> bucket;  // 2^(n_sites - h) + 1 entries
};

inline uint64_t spin_momentum64_site_mask(int n_sites) { return ~uint64_t(0) >> (64 - n_sites); }

// T s
inline uint64_t spin_momentum64_translate(uint64_t s, int n_sites, int cell) {
  return ((s << cell) | (s >> (n_sites - cell))) & spin_momentum64_site_mask(n_sites);
}

inline std::string spin_momentum64_geometry_error(int n_sites, int n_up, int cell, int momentum) {
  if (n_sites < kSpinMinSites || n_sites > kMomentum64MaxSites) return "n_sites must be 2..48";
  if (n_up < 0 || n_up > n_sites) return "n_up must be 0..n_sites";
  if (cell < 1 || n_sites % cell != 0) return "cell must be at least 1 and divide n_sites";
  if (cell > n_sites / 2) return "cell must be at most n_sites / 2: a translation by the whole ring is no symmetry to use";
  if (momentum < 0 || momentum >= n_sites / cell) return "momentum must be 0..n_sites/cell - 1";
  return "";
}

// "" if the model is valid within the limits above and invariant under the translation (a valid geometry is assumed; the
// arguments carry no transverse field)
inline std::string spin_momentum64_model_error(const SpinModelArgs& a, int cell) {
  if (a.n_bonds < 0 || a.n_bonds > kMomentum64MaxBonds) return "n_bonds must be 0..128";
  if (a.n_bonds > 0 && (!a.site_i || !a.site_j || !a.jz || !a.jxy)) return "site_i, site_j, jz or jxy is NULL";
  for (int b = 0; b < a.n_bonds; ++b) {
    if (a.site_i[b] < 0 || a.site_i[b] >= a.n_sites || a.site_j[b] < 0 || a.site_j[b] >= a.n_sites) return "a bond names a site outside 0..n_sites-1";
    if (a.site_i[b] == a.site_j[b]) return "a bond joins a site to itself";
    if (!std::isfinite(a.jz[b]) || !std::isfinite(a.jxy[b])) return "a coupling is not finite";
  }
  for (int i = 0; i < a.n_sites; ++i)
    if (a.hz && !std::isfinite(a.hz[i])) return "a field is not finite";
  return spin_momentum_invariance_error(a, cell);
}

// Is s the smallest state of its orbit?  *period is set for a representative.
inline bool spin_momentum64_is_representative(uint64_t s, int n_sites, int cell, int n_trans, int* period) {
  uint64_t t = s;
  for (int r = 1; r <= n_trans; ++r) {
    t = spin_momentum64_translate(t, n_sites, cell);
    if (t < s) return false;
    if (t == s) {
      *period = r;
      return true;
    }
  }
  return false;  // not reached: T^N is the identity
}

// the chunks of the enumeration: tb top bits; a chunk is the prefix p, its states p << (L - tb) | q, q ascending
inline int spin_momentum64_prefix_bits(int n_sites) { return n_sites >= 20 ? 16 : 0; }
inline bool spin_momentum64_prefix_may_lead(uint32_t p, int tb, int cell) {
  for (int c = cell; c < tb; c += cell)
    if ((p >> c) > (p & ((uint32_t(1) << (tb - c)) - 1))) return false;
  return true;
}

// Calls f(state) for the states of chunk p in ascending order until f returns false (Gosper's successor on the low bits)
template <class F>
inline void spin_momentum64_for_each_in_chunk(int n_sites, int n_up, int tb, uint32_t p, F f) {
  const int lb = n_sites - tb, k = n_up - __builtin_popcount(p);
  if (k < 0 || k > lb) return;
  const uint64_t top = (uint64_t)p << lb;
  if (k == 0) {
    f(top);
    return;
  }
  const uint64_t end = uint64_t(1) << lb;
  for (uint64_t q = (uint64_t(1) << k) - 1; q < end;) {
    if (!f(top | q)) return;
    const uint64_t c = q & (~q + 1), r = q + c;
    q = (((r ^ q) >> 2) / c) | r;
  }
}

// The rows of the sector of a valid geometry; returns their number, or a number above kMomentum64MaxDim as soon as that many
// are known to exist (the basis is then not usable).  basis == nullptr: the count alone, nothing is stored.  with_lookup false:
// rows and periods only, bucket stays empty and steps 0 -- for the host functions, which search the whole list and would otherwise
// fill up to 2^24 + 1 words per call.
inline int64_t spin_momentum64_build_basis(int n_sites, int n_up, int cell, int momentum, SpinMomentum64Basis* basis, bool with_lookup = true) {
  const int n_trans = n_sites / cell, tb = spin_momentum64_prefix_bits(n_sites);
  const size_t n_chunks = size_t(1) << tb;
  std::vector<std::vector<uint64_t>> chunk_reps(basis ? n_chunks : 0);
  std::vector<std::vector<uint8_t>> chunk_period(basis ? n_chunks : 0);
  std::vector<int64_t> chunk_count(n_chunks, 0);
  std::atomic<size_t> next(0);
  std::atomic<int64_t> total(0);
  const auto work = [&]() {
    for (size_t p = next.fetch_add(1); p < n_chunks; p = next.fetch_add(1)) {
      if (total.load() > kMomentum64MaxDim) return;
      if (!spin_momentum64_prefix_may_lead((uint32_t)p, tb, cell)) continue;
      int64_t count = 0;
      spin_momentum64_for_each_in_chunk(n_sites, n_up, tb, (uint32_t)p, [&](uint64_t s) {
        int period = 0;
        if (!spin_momentum64_is_representative(s, n_sites, cell, n_trans, &period) || (momentum * period) % n_trans != 0) return true;
        ++count;
        if (basis) chunk_reps[p].push_back(s), chunk_period[p].push_back((uint8_t)period);
        return (count & 0xfffff) != 0 || total.load() + count <= kMomentum64MaxDim;
      });
      chunk_count[p] = count;
      total.fetch_add(count);
    }
  };
  unsigned n_threads = tb == 0 ? 1u : std::min<unsigned>(kMomentum64Threads, std::max(1u, std::thread::hardware_concurrency()));
  if (n_threads <= 1) {
    work();
  } else {
    std::vector<std::thread> pool;
    for (unsigned i = 0; i < n_threads; ++i) pool.emplace_back(work);
    for (std::thread& t : pool) t.join();
  }
  const int64_t count = total.load();
  if (!basis || count > kMomentum64MaxDim) return count;
  *basis = SpinMomentum64Basis();
  basis->n_sites = n_sites, basis->n_up = n_up, basis->cell = cell, basis->n_trans = n_trans, basis->momentum = momentum;
  basis->h = (n_sites + 1) / 2;
  basis->reps.reserve((size_t)count), basis->period.reserve((size_t)count);
  for (size_t p = 0; p < n_chunks; ++p) {  // ascending prefixes: the plain walk's order
    basis->reps.insert(basis->reps.end(), chunk_reps[p].begin(), chunk_reps[p].end());
    basis->period.insert(basis->period.end(), chunk_period[p].begin(), chunk_period[p].end());
    std::vector<uint64_t>().swap(chunk_reps[p]);
    std::vector<uint8_t>().swap(chunk_period[p]);
  }
  if (!with_lookup) return count;
  const size_t nb = size_t(1) << (n_sites - basis->h);
  basis->bucket.assign(nb + 1, 0);
  size_t i = 0, largest = 0;
  for (size_t hi = 0; hi <= nb; ++hi) {  // bucket[hi]: the first representative whose high bits are >= hi
    while (i < basis->reps.size() && (size_t)(basis->reps[i] >> basis->h) < hi) ++i;
    basis->bucket[hi] = (uint32_t)i;
    if (hi > 0) largest = std::max(largest, (size_t)(basis->bucket[hi] - basis->bucket[hi - 1]));
  }
  while ((size_t(1) << basis->steps) < largest + 1) ++basis->steps;  // ceil(log2(largest + 1))
  return count;
}

inline void spin_momentum64_build_tables(int n_trans, int momentum, SpinMomentum64Tables& t) {
  t = SpinMomentum64Tables();
  for (int p = 1; p <= kMomentum64MaxPeriod; ++p)
    for (int q = 1; q <= kMomentum64MaxPeriod; ++q) t.ratio[p * kMomentum64RatioPitch + q] = std::sqrt((double)p / (double)q);
  for (int q = 1; q <= kMomentum64MaxPeriod; ++q) t.inv_sqrt[q] = 1.0 / std::sqrt((double)q);
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

// the kernels' view of a valid model on a built basis: spin_build_view's tables with 64-bit masks
inline void spin_momentum64_build_view(const SpinModelArgs& a, const SpinMomentum64Basis& b, SpinMomentum64View& v) {
  v = SpinMomentum64View();
  SpinOperatorView64& o = v.model;
  o.n_sites = a.n_sites;
  for (int k = 0; k < a.n_bonds; ++k) {
    const uint64_t m = (uint64_t(1) << a.site_i[k]) | (uint64_t(1) << a.site_j[k]);
    o.dmask[o.ndiag] = m, o.dval[o.ndiag++] = a.jz[k] * 0.25;
    if (a.jxy[k] != 0.0) o.fmask[o.nflip] = m, o.fval[o.nflip++] = a.jxy[k] * 0.5;
  }
  if (a.hz)
    for (int i = 0; i < a.n_sites; ++i) o.dmask[o.ndiag] = uint64_t(1) << i, o.dval[o.ndiag++] = -(a.hz[i] * 0.5);
  v.n_up = b.n_up, v.cell = b.cell, v.n_trans = b.n_trans, v.momentum = b.momentum, v.h = b.h, v.steps = b.steps;
  v.site_mask = spin_momentum64_site_mask(b.n_sites);
  for (int r = 1; r <= b.n_trans; ++r)
    if ((b.momentum * r) % b.n_trans == 0) v.compatible |= uint64_t(1) << (r - 1);
  v.first_rep = b.reps.empty() ? 0u : b.reps[0];
  spin_momentum64_build_tables(b.n_trans, b.momentum, v.tab);
}

// the orbit of any state, from the definition
struct SpinMomentum64Orbit {
  uint64_t rep;
  int j, period;
};
inline SpinMomentum64Orbit spin_momentum64_orbit_host(uint64_t s, int n_sites, int cell) {
  SpinMomentum64Orbit o = {s, 0, 0};
  uint64_t t = s;
  for (int r = 1;; ++r) {
    t = spin_momentum64_translate(t, n_sites, cell);
    if (t == s) {
      o.period = r;
      return o;
    }
    if (t < o.rep) o.rep = t, o.j = r;
  }
}

// idx(b) of a representative of the sector, -1 for any other state
inline int64_t spin_momentum64_row_of(const SpinMomentum64Basis& b, uint64_t rep) {
  const auto it = std::lower_bound(b.reps.begin(), b.reps.end(), rep);
  return it != b.reps.end() && *it == rep ? (int64_t)(it - b.reps.begin()) : -1;
}

// spin_momentum_write_rows on the 64-bit basis, from the definition
inline void spin_momentum64_write_rows(const SpinModelArgs& a, const SpinMomentum64Basis& basis, const SpinMomentum64Tables& t, int64_t row_begin,
                                       int64_t n_rows, int64_t* rowptr, int32_t* col, double* val, int64_t* nnz) {
  const int L = basis.n_sites, N = basis.n_trans;
  int64_t p = 0;
  rowptr[0] = 0;
  for (int64_t k = 0; k < n_rows; ++k) {
    const uint64_t s = basis.reps[(size_t)(row_begin + k)];
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
        const uint64_t s2 = s ^ ((uint64_t(1) << a.site_i[b]) | (uint64_t(1) << a.site_j[b]));
        const SpinMomentum64Orbit o = spin_momentum64_orbit_host(s2, L, basis.cell);
        if ((basis.momentum * o.period) % N != 0) continue;
        if (col) {
          const int l = (N - o.j) % N;
          const double half = a.jxy[b] * 0.5;
          const double c = half * t.ratio[period * kMomentum64RatioPitch + o.period];
          col[p] = (int32_t)spin_momentum64_row_of(basis, o.rep);
          val[2 * p] = c * t.phase_re[l], val[2 * p + 1] = c * t.phase_im[l];
        }
        ++p;
      }
    rowptr[k + 1] = p;
  }
  *nnz = p;
}

// ---- diagonal correlations in the momentum basis (the definition is at the top) ----
struct SpinMomentumMeasureArgs {
  int n_sites, n_diag;
  const uint64_t* masks;
};

// nullptr if the mask list is valid: the limits and messages of spin_measure_error's diagonal list
inline const char* spin_momentum_measure_error(const SpinMomentumMeasureArgs& a) {
  if (a.n_diag < 0 || a.n_diag > kSpinMeasureMaxTerms) return "n_diag must be 0..1024";
  if (a.n_diag > 0 && !a.masks) return "a mask list is NULL but its count is not zero";
  const uint64_t outside = ~spin_momentum64_site_mask(a.n_sites);
  for (int t = 0; t < a.n_diag; ++t) {
    if (a.masks[t] == 0) return "a mask is zero";
    if (a.masks[t] & outside) return "a mask names a site outside 0..n_sites-1";
  }
  return nullptr;
}

// What one launch of k_spin_momentum_measure receives: masks [k C, k C + C), padded with 0 (a slot nobody reads)
struct SpinMomentumMeasureChunk {
  int ndiag, pad;
  uint64_t dmask[kSpinMeasureChunk];
};
inline void spin_momentum_measure_build_chunks(const SpinMomentumMeasureArgs& a, std::vector<SpinMomentumMeasureChunk>& chunks) {
  chunks.assign((size_t)spin_measure_chunks(a.n_diag, 0), SpinMomentumMeasureChunk());
  for (size_t k = 0; k < chunks.size(); ++k) {
    const int first = (int)k * kSpinMeasureChunk;
    chunks[k].ndiag = std::max(0, std::min(a.n_diag - first, kSpinMeasureChunk));
    for (int t = 0; t < chunks[k].ndiag; ++t) chunks[k].dmask[t] = a.masks[first + t];
  }
}

// The definition, evaluated over the rows of a built basis: x has one double (is_complex false) or an interleaved pair per row
inline void spin_momentum_measure_host(const SpinMomentum64Basis& b, const SpinMomentumMeasureArgs& a, bool is_complex, const double* x,
                                       double* diag_out, double* norm2) {
  std::vector<double> dg((size_t)a.n_diag, 0.0);
  double nrm = 0.0;
  for (size_t r = 0; r < b.reps.size(); ++r) {
    double w;
    if (is_complex) {
      const double xr = x[2 * r], xi = x[2 * r + 1];
      nrm = std::fma(xi, xi, std::fma(xr, xr, nrm));
      w = std::fma(xi, xi, xr * xr);
    } else {
      nrm = std::fma(x[r], x[r], nrm);
      w = x[r] * x[r];
    }
    for (int t = 0; t < a.n_diag; ++t) {
      int c = 0;
      uint64_t s = b.reps[r];
      for (int k = 0; k < b.n_trans; ++k) {
        uint64_t down = ~s & a.masks[t];  // sigma = -1 on the mask's down sites
        int parity = 0;
        for (; down; down &= down - 1) parity ^= 1;
        c += parity ? -1 : 1;
        s = spin_momentum64_translate(s, b.n_sites, b.cell);
      }
      dg[(size_t)t] = std::fma((double)c, w, dg[(size_t)t]);
    }
  }
  for (int t = 0; t < a.n_diag && diag_out; ++t) diag_out[t] = dg[(size_t)t];
  if (norm2) *norm2 = nrm;
}

}  // namespace eigenex
