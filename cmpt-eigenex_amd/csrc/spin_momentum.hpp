// The spin-1/2 Hamiltonian of spin_model.hpp in one momentum sector of one sector of fixed magnetisation (host side, no HIP),
// written once for both state words: Word = uint32_t (eigenex_spin_momentum_*, up to 32 sites) and Word = uint64_t
// (eigenex_spin_momentum64_*, eigenex_spin_momentum_measure*, up to 48 sites).  Shared by the library and by the host program
// tests/cpp/spin_momentum_sanitize.cpp, which runs this file under AddressSanitizer + UBSan for either word.
//
// Word.  A state is a Word, site i at bit i.  SpinWord<Word> (spin_rows.hpp) is the one description of what depends on the width:
//   kMaxSites 32 / 48; kMaxBonds 64 / 128 (a J1-J2 ring of 36 sites has 72); kMaxTerms 96 / 176, the term tables of the model's
//   view, SpinWord<Word>::Model: SpinOperatorView with 32-bit masks, SpinOperatorView64 with 64-bit ones for 128 bonds and 48 fields
//   kMaxPeriod = kMaxSites: `compatible` has that many bits; kRatioPitch 33 / 49; the two shifts of a rotation are 1..31 / 1..47
//   the bucket table has 2^(L - h) + 1 words with h = (L + 1) / 2, at most 2^16 + 1 / 2^24 + 1; dim < 2^31 for both
// For n_sites <= 32 and n_bonds <= 64 every function here returns the same for both words.
// Translation.  cell = a divides L = n_sites and 1 <= a <= L/2; N = L / a is the number of translations.  T moves site i to site
//   (i + a) mod L: on a state word a left rotation of the low L bits by a, ((s << a) | (s >> (L - a))) & site_mask.
// Model.  Accepted if it conserves Sz and is invariant under T: the multiset of (unordered bond, jz, jxy), couplings compared bit
//   for bit, maps onto itself, and hz[i] == hz[(i + a) mod L].  Otherwise refused with a message that names the first bond or site
//   that breaks the symmetry.  What comes before the invariance check differs per word (spin_momentum_limits_error): a 32-bit
//   sector is checked by spin_sector_error, a 64-bit one here, within the limits above; its arguments carry no transverse field.
// Sector (L, n_up, cell, m), 0 <= m < N, k = 2 pi m / N.  A state s has orbit period R_s, the smallest R >= 1 with T^R s = s; it
//   divides N.  The representative of an orbit is its numerically smallest state.  The rows are the representatives a of the Sz
//   sector with (m R_a) mod N == 0, ascending; idx(a) is the row of a.  A sector without such a state is refused.
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
//
// Enumeration.  The plain walk visits C(L, n_up) states, 9.1e9 at (36, 18).  Here the sector is cut by the top bits of the state
// into chunks that up to 16 threads take in turn and that are joined in ascending order, so the list is the plain walk's.  A chunk
// is skipped where its prefix p of tb bits alone shows that a rotation is smaller: for every multiple c of cell below tb, the
// top tb - c bits of T^(c/cell) s are the low tb - c bits of p and those of s are p >> c; if the first are smaller, no state of
// the chunk is a representative.  About one prefix in eight survives at cell = 1.  Below 20 sites there is one chunk, tb = 0, and
// the code is the plain walk on one thread.  spin_momentum_for_each_state, the plain walk itself, is kept for expand, which needs
// the rank of every state of the sector.
//
// Diagonal correlations (eigenex_spin_momentum_measure; kernels.hip: k_spin_momentum_measure<E, Word>).  In a momentum eigenstate
// x of the sector, <D> of a product D of sigma^z over a site mask needs no expansion: D is diagonal and distinct orbits are
// disjoint, so  <D> = sum_a |x_a|^2 (1/N) sum_{r<N} D(T^r a)  over the representatives a.  The raw sums are
//   norm2   = sum_a |x_a|^2                      one fma per row of a real x (x, x), two of a complex one (re, then im)
//   diag[t] = sum_a c_t(a) w_a                   one fma per row: fma((double)c_t(a), w_a, diag[t])
//   w_a     = x_a * x_a, of a complex element fma(im, im, re * re)
//   c_t(a)  = sum_{r<N} prod_{i in mask_t} sigma_i(T^r a), an integer in [-N, N]; sigma_i(s) = +1 if bit i of s is set, else -1
// rows ascending, so that <D_t> = diag[t] / (N norm2).  Masks are 64-bit for both words; 1..1024 of them, none zero, none with a
// site >= n_sites.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <string>
#include <thread>
#include <vector>

#include "spin_rows.hpp"

namespace eigenex {

constexpr int kMomentumThreads = 16;
constexpr int64_t kMomentumMaxDim = (int64_t(1) << 31) - 1;

// ratio, inv_sqrt and phase of one (N, m); ratio[p * pitch + q], 0 <= p, q <= kMaxPeriod (row and column 0 unused)
template <class Word>
struct SpinMomentumTablesOf {
  double ratio[SpinWord<Word>::kRatioPitch * SpinWord<Word>::kRatioPitch];
  double inv_sqrt[SpinWord<Word>::kRatioPitch];
  double phase_re[SpinWord<Word>::kMaxPeriod], phase_im[SpinWord<Word>::kMaxPeriod];
};

// The kernels' form of the sector (device memory, owned by the shard; reps and bucket are separate arrays).  It is
// value-initialised before it is filled, so the padding that goes to the device with it is zero.
template <class Word>
struct SpinMomentumViewOf {
  typename SpinWord<Word>::Model model;  // no transverse field: every flip mask has two bits
  int n_up, cell, n_trans, momentum;
  int h, steps;     // bucket index = state >> h; trip count of the search
  Word site_mask;   // the low n_sites bits
  Word compatible;  // bit R - 1: (momentum * R) mod n_trans == 0
  Word first_rep;   // reps[0]: what a lane of expand without a compatible representative looks up
  SpinMomentumTablesOf<Word> tab;
};

// the rows of one sector and their lookup
template <class Word>
struct SpinMomentumBasisOf {
  int n_sites = 0, n_up = 0, cell = 0, n_trans = 0, momentum = 0, h = 0, steps = 0;
  std::vector<Word> reps;        // ascending
  std::vector<uint8_t> period;   // of each representative
  std::vector<uint32_t> bucket;  // 2^(n_sites - h) + 1 entries; empty without the lookup
};

typedef SpinMomentumTablesOf<uint32_t> SpinMomentumTables;
typedef SpinMomentumTablesOf<uint64_t> SpinMomentum64Tables;
typedef SpinMomentumViewOf<uint32_t> SpinMomentumView;
typedef SpinMomentumViewOf<uint64_t> SpinMomentum64View;
typedef SpinMomentumBasisOf<uint32_t> SpinMomentumBasis;
typedef SpinMomentumBasisOf<uint64_t> SpinMomentum64Basis;

// what the kernels read does not move
static_assert(sizeof(SpinMomentumView) == 11848 && sizeof(SpinOperatorView) == 2320 && sizeof(SpinMomentumTables) == 9488, "32-bit view");
static_assert(offsetof(SpinMomentumView, n_up) == 2320 && offsetof(SpinMomentumView, site_mask) == 2344 && offsetof(SpinMomentumView, compatible) == 2348 &&
                  offsetof(SpinMomentumView, first_rep) == 2352 && offsetof(SpinMomentumView, tab) == 2360,
              "32-bit view");
static_assert(sizeof(SpinMomentum64View) == 26064 && sizeof(SpinOperatorView64) == 5648 && sizeof(SpinMomentum64Tables) == 20368, "64-bit view");
static_assert(offsetof(SpinMomentum64View, n_up) == 5648 && offsetof(SpinMomentum64View, site_mask) == 5672 && offsetof(SpinMomentum64View, compatible) == 5680 &&
                  offsetof(SpinMomentum64View, first_rep) == 5688 && offsetof(SpinMomentum64View, tab) == 5696,
              "64-bit view");

template <class Word>
inline Word spin_momentum_site_mask(int n_sites) {
  return Word(~Word(0)) >> (SpinWord<Word>::kBits - n_sites);
}

// T s
template <class Word>
inline Word spin_momentum_translate(Word s, int n_sites, int cell) {
  return ((s << cell) | (s >> (n_sites - cell))) & spin_momentum_site_mask<Word>(n_sites);
}

// "" if (n_sites, n_up, cell, momentum) names a sector (that may still be empty), else what is wrong
template <class Word>
inline std::string spin_momentum_geometry_error(int n_sites, int n_up, int cell, int momentum) {
  if (n_sites < kSpinMinSites || n_sites > SpinWord<Word>::kMaxSites) return "n_sites must be 2.." + std::to_string(SpinWord<Word>::kMaxSites);
  if (n_up < 0 || n_up > n_sites) return "n_up must be 0..n_sites";
  if (cell < 1 || n_sites % cell != 0) return "cell must be at least 1 and divide n_sites";
  if (cell > n_sites / 2) return "cell must be at most n_sites / 2: a translation by the whole ring is no symmetry to use";
  if (momentum < 0 || momentum >= n_sites / cell) return "momentum must be 0..n_sites/cell - 1";
  return "";
}

// The first half of the model check, per word (the last argument only selects it): nullptr if the model is valid within the
// word's limits and conserves Sz.  A valid geometry is assumed.
inline const char* spin_momentum_limits_error(const SpinModelArgs& a, int n_up, uint32_t) { return spin_sector_error(a, n_up); }
inline const char* spin_momentum_limits_error(const SpinModelArgs& a, int, uint64_t) {
  if (a.n_bonds < 0 || a.n_bonds > SpinWord<uint64_t>::kMaxBonds) return "n_bonds must be 0..128";
  if (a.n_bonds > 0 && (!a.site_i || !a.site_j || !a.jz || !a.jxy)) return "site_i, site_j, jz or jxy is NULL";
  for (int b = 0; b < a.n_bonds; ++b) {
    if (a.site_i[b] < 0 || a.site_i[b] >= a.n_sites || a.site_j[b] < 0 || a.site_j[b] >= a.n_sites) return "a bond names a site outside 0..n_sites-1";
    if (a.site_i[b] == a.site_j[b]) return "a bond joins a site to itself";
    if (!std::isfinite(a.jz[b]) || !std::isfinite(a.jxy[b])) return "a coupling is not finite";
  }
  for (int i = 0; i < a.n_sites; ++i)
    if (a.hz && !std::isfinite(a.hz[i])) return "a field is not finite";
  return nullptr;
}

// the second half, of a model whose sites and bonds are valid: "" if it is invariant under the translation by `cell` sites
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

// "" if the model is valid for the word, conserves Sz and is invariant under the translation (a valid geometry is assumed)
template <class Word>
inline std::string spin_momentum_model_error(const SpinModelArgs& a, int n_up, int cell) {
  if (const char* why = spin_momentum_limits_error(a, n_up, Word())) return why;
  return spin_momentum_invariance_error(a, cell);
}

inline bool spin_momentum_is_real(int n_trans, int momentum) { return momentum == 0 || 2 * momentum == n_trans; }

// Walks the states of the Sz sector in ascending order and calls f(state) for each (Gosper's successor in 64 bits: no overflow
// at 32 sites).  For expand; the rows come from spin_momentum_build_basis.
template <class Word, class F>
inline void spin_momentum_for_each_state(int n_sites, int n_up, F f) {
  if (n_up == 0) {
    f(Word(0));
    return;
  }
  const uint64_t end = uint64_t(1) << n_sites;
  for (uint64_t s = (uint64_t(1) << n_up) - 1; s < end;) {
    f((Word)s);
    const uint64_t c = s & (~s + 1), r = s + c;
    s = (((r ^ s) >> 2) / c) | r;
  }
}

// Is s the smallest state of its orbit?  Rotates with an exit at the first smaller rotation; *period is set for a representative.
template <class Word>
inline bool spin_momentum_is_representative(Word s, int n_sites, int cell, int n_trans, int* period) {
  Word t = s;
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

// the chunks of the enumeration: tb top bits; a chunk is the prefix p, its states p << (L - tb) | q, q ascending
inline int spin_momentum_prefix_bits(int n_sites) { return n_sites >= 20 ? 16 : 0; }
inline bool spin_momentum_prefix_may_lead(uint32_t p, int tb, int cell) {
  for (int c = cell; c < tb; c += cell)
    if ((p >> c) > (p & ((uint32_t(1) << (tb - c)) - 1))) return false;
  return true;
}

// Calls f(state) for the states of chunk p in ascending order until f returns false (Gosper's successor on the low bits)
template <class Word, class F>
inline void spin_momentum_for_each_in_chunk(int n_sites, int n_up, int tb, uint32_t p, F f) {
  const int lb = n_sites - tb, k = n_up - __builtin_popcount(p);
  if (k < 0 || k > lb) return;
  const uint64_t top = (uint64_t)p << lb;
  if (k == 0) {
    f((Word)top);
    return;
  }
  const uint64_t end = uint64_t(1) << lb;
  for (uint64_t q = (uint64_t(1) << k) - 1; q < end;) {
    if (!f((Word)(top | q))) return;
    const uint64_t c = q & (~q + 1), r = q + c;
    q = (((r ^ q) >> 2) / c) | r;
  }
}

// The rows of the sector of a valid geometry; returns their number, or a number above kMomentumMaxDim as soon as that many are
// known to exist (the basis is then not usable; 32 sites cannot get there).  basis == nullptr: the count alone, nothing is
// stored.  with_lookup false: rows and periods only, bucket stays empty and steps 0 -- for the host functions, which search the
// whole list and would otherwise fill up to 2^24 + 1 words per call.
template <class Word>
inline int64_t spin_momentum_build_basis(int n_sites, int n_up, int cell, int momentum, SpinMomentumBasisOf<Word>* basis, bool with_lookup = true) {
  const int n_trans = n_sites / cell, tb = spin_momentum_prefix_bits(n_sites);
  const size_t n_chunks = size_t(1) << tb;
  std::vector<std::vector<Word>> chunk_reps(basis ? n_chunks : 0);
  std::vector<std::vector<uint8_t>> chunk_period(basis ? n_chunks : 0);
  std::atomic<size_t> next(0);
  std::atomic<int64_t> total(0);
  const auto work = [&]() {
    for (size_t p = next.fetch_add(1); p < n_chunks; p = next.fetch_add(1)) {
      if (total.load() > kMomentumMaxDim) return;
      if (!spin_momentum_prefix_may_lead((uint32_t)p, tb, cell)) continue;
      int64_t count = 0;
      spin_momentum_for_each_in_chunk<Word>(n_sites, n_up, tb, (uint32_t)p, [&](Word s) {
        int period = 0;
        if (!spin_momentum_is_representative(s, n_sites, cell, n_trans, &period) || (momentum * period) % n_trans != 0) return true;
        ++count;
        if (basis) chunk_reps[p].push_back(s), chunk_period[p].push_back((uint8_t)period);
        return (count & 0xfffff) != 0 || total.load() + count <= kMomentumMaxDim;
      });
      total.fetch_add(count);
    }
  };
  const unsigned n_threads = tb == 0 ? 1u : std::min<unsigned>(kMomentumThreads, std::max(1u, std::thread::hardware_concurrency()));
  if (n_threads <= 1) {
    work();
  } else {
    std::vector<std::thread> pool;
    for (unsigned i = 0; i < n_threads; ++i) pool.emplace_back(work);
    for (std::thread& t : pool) t.join();
  }
  const int64_t count = total.load();
  if (!basis || count > kMomentumMaxDim) return count;
  *basis = SpinMomentumBasisOf<Word>();
  basis->n_sites = n_sites, basis->n_up = n_up, basis->cell = cell, basis->n_trans = n_trans, basis->momentum = momentum;
  basis->h = (n_sites + 1) / 2;
  basis->reps.reserve((size_t)count), basis->period.reserve((size_t)count);
  for (size_t p = 0; p < n_chunks; ++p) {  // ascending prefixes: the plain walk's order
    basis->reps.insert(basis->reps.end(), chunk_reps[p].begin(), chunk_reps[p].end());
    basis->period.insert(basis->period.end(), chunk_period[p].begin(), chunk_period[p].end());
    std::vector<Word>().swap(chunk_reps[p]);
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

template <class Word>
inline void spin_momentum_build_tables(int n_trans, int momentum, SpinMomentumTablesOf<Word>& t) {
  constexpr int kMaxPeriod = SpinWord<Word>::kMaxPeriod, kPitch = SpinWord<Word>::kRatioPitch;
  t = SpinMomentumTablesOf<Word>();
  for (int p = 1; p <= kMaxPeriod; ++p)
    for (int q = 1; q <= kMaxPeriod; ++q) t.ratio[p * kPitch + q] = std::sqrt((double)p / (double)q);
  for (int q = 1; q <= kMaxPeriod; ++q) t.inv_sqrt[q] = 1.0 / std::sqrt((double)q);
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

// The model's view of a valid model, per word: spin_build_view's tables without a transverse field; with 64-bit masks they are
// filled here, the same constants in the same order.
inline void spin_momentum_build_model(const SpinModelArgs& a, SpinOperatorView& v) {
  SpinModelArgs z = a;
  z.hx = nullptr;
  spin_build_view(z, v);
}
inline void spin_momentum_build_model(const SpinModelArgs& a, SpinOperatorView64& o) {
  o = SpinOperatorView64();
  o.n_sites = a.n_sites;
  for (int k = 0; k < a.n_bonds; ++k) {
    const uint64_t m = (uint64_t(1) << a.site_i[k]) | (uint64_t(1) << a.site_j[k]);
    o.dmask[o.ndiag] = m, o.dval[o.ndiag++] = a.jz[k] * 0.25;
    if (a.jxy[k] != 0.0) o.fmask[o.nflip] = m, o.fval[o.nflip++] = a.jxy[k] * 0.5;
  }
  if (a.hz)
    for (int i = 0; i < a.n_sites; ++i) o.dmask[o.ndiag] = uint64_t(1) << i, o.dval[o.ndiag++] = -(a.hz[i] * 0.5);
}

// the kernels' view of a valid model on a built basis
template <class Word>
inline void spin_momentum_build_view(const SpinModelArgs& a, const SpinMomentumBasisOf<Word>& b, SpinMomentumViewOf<Word>& v) {
  v = SpinMomentumViewOf<Word>();
  spin_momentum_build_model(a, v.model);
  v.n_up = b.n_up, v.cell = b.cell, v.n_trans = b.n_trans, v.momentum = b.momentum, v.h = b.h, v.steps = b.steps;
  v.site_mask = spin_momentum_site_mask<Word>(b.n_sites);
  for (int r = 1; r <= b.n_trans; ++r)
    if ((b.momentum * r) % b.n_trans == 0) v.compatible |= Word(1) << (r - 1);
  v.first_rep = b.reps.empty() ? Word(0) : b.reps[0];
  spin_momentum_build_tables(b.n_trans, b.momentum, v.tab);
}

// the orbit of any state, from the definition: the representative, the smallest j >= 0 with T^j s = rep(s), and the period
template <class Word>
struct SpinMomentumOrbitOf {
  Word rep;
  int j, period;
};
template <class Word>
inline SpinMomentumOrbitOf<Word> spin_momentum_orbit_host(Word s, int n_sites, int cell) {
  SpinMomentumOrbitOf<Word> o = {s, 0, 0};
  Word t = s;
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
template <class Word>
inline int64_t spin_momentum_row_of(const SpinMomentumBasisOf<Word>& b, Word rep) {
  const auto it = std::lower_bound(b.reps.begin(), b.reps.end(), rep);
  return it != b.reps.end() && *it == rep ? (int64_t)(it - b.reps.begin()) : -1;
}

// Rows [row_begin, row_begin + n_rows) of a valid model as CSR, the signature of spin_write_rows with val interleaved (re, im):
// rowptr[n_rows + 1] and *nnz always; col and val unless both are NULL.  Written from the definition at the top.
template <class Word>
inline void spin_momentum_write_rows(const SpinModelArgs& a, const SpinMomentumBasisOf<Word>& basis, const SpinMomentumTablesOf<Word>& t,
                                     int64_t row_begin, int64_t n_rows, int64_t* rowptr, int32_t* col, double* val, int64_t* nnz) {
  const int L = basis.n_sites, N = basis.n_trans;
  int64_t p = 0;
  rowptr[0] = 0;
  for (int64_t k = 0; k < n_rows; ++k) {
    const Word s = basis.reps[(size_t)(row_begin + k)];
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
        const Word s2 = s ^ ((Word(1) << a.site_i[b]) | (Word(1) << a.site_j[b]));
        const SpinMomentumOrbitOf<Word> o = spin_momentum_orbit_host(s2, L, basis.cell);
        if ((basis.momentum * o.period) % N != 0) continue;
        if (col) {
          const int l = (N - o.j) % N;
          const double half = a.jxy[b] * 0.5;
          const double c = half * t.ratio[period * SpinWord<Word>::kRatioPitch + o.period];
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
template <class Word>
inline void spin_momentum_expand_host(const SpinMomentumBasisOf<Word>& basis, const SpinMomentumTablesOf<Word>& t, bool is_complex, const double* x,
                                      double* y) {
  const int L = basis.n_sites, N = basis.n_trans;
  int64_t rank = 0;
  spin_momentum_for_each_state<Word>(L, basis.n_up, [&](Word s) {
#if defined(__clang__)
#pragma clang fp contract(off)  // a host compiler other than clang needs -ffp-contract=off, as for add_product_nofma
#endif
    const SpinMomentumOrbitOf<Word> o = spin_momentum_orbit_host(s, L, basis.cell);
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

// ---- diagonal correlations in the momentum basis (the definition is at the top) ----
struct SpinMomentumMeasureArgs {
  int n_sites, n_diag;
  const uint64_t* masks;
};

// nullptr if the mask list is valid: the limits and messages of spin_measure_error's diagonal list
inline const char* spin_momentum_measure_error(const SpinMomentumMeasureArgs& a) {
  if (a.n_diag < 0 || a.n_diag > kSpinMeasureMaxTerms) return "n_diag must be 0..1024";
  if (a.n_diag > 0 && !a.masks) return "a mask list is NULL but its count is not zero";
  const uint64_t outside = ~spin_momentum_site_mask<uint64_t>(a.n_sites);
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
static_assert(sizeof(SpinMomentumMeasureChunk) == 136, "what the kernels read does not move");
inline void spin_momentum_measure_build_chunks(const SpinMomentumMeasureArgs& a, std::vector<SpinMomentumMeasureChunk>& chunks) {
  chunks.assign((size_t)spin_measure_chunks(a.n_diag, 0), SpinMomentumMeasureChunk());
  for (size_t k = 0; k < chunks.size(); ++k) {
    const int first = (int)k * kSpinMeasureChunk;
    chunks[k].ndiag = std::max(0, std::min(a.n_diag - first, kSpinMeasureChunk));
    for (int t = 0; t < chunks[k].ndiag; ++t) chunks[k].dmask[t] = a.masks[first + t];
  }
}

// The definition, evaluated over the rows of a built basis: x has one double (is_complex false) or an interleaved pair per row
template <class Word>
inline void spin_momentum_measure_host(const SpinMomentumBasisOf<Word>& b, const SpinMomentumMeasureArgs& a, bool is_complex, const double* x,
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
      Word s = b.reps[r];
      for (int k = 0; k < b.n_trans; ++k) {
        uint64_t down = ~(uint64_t)s & a.masks[t];  // sigma = -1 on the mask's down sites
        int parity = 0;
        for (; down; down &= down - 1) parity ^= 1;
        c += parity ? -1 : 1;
        s = spin_momentum_translate(s, b.n_sites, b.cell);
      }
      dg[(size_t)t] = std::fma((double)c, w, dg[(size_t)t]);
    }
  }
  for (int t = 0; t < a.n_diag && diag_out; ++t) diag_out[t] = dg[(size_t)t];
  if (norm2) *norm2 = nrm;
}

}  // namespace eigenex
