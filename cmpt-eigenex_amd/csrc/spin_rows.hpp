// The row walk of the matrix-free spin-1/2 kernels (kernels.hip: k_spin_spmv<SECTOR, E> and k_spin_measure<SECTOR, E>, each
// written once for real (E = double) and complex (E = SpinZ) vectors, as k_spin_site_apply<SECTOR, E> is, and through spin_rdm_rows.hpp
// k_spin_rdm<SECTOR, TILE, E>; k_spin_measure_columns<SECTOR> for real vectors: spin_measure_columns_row; at the end of this file the walk of k_spin_momentum_spmv<E>, k_spin_momentum_expand<E> and
// k_spin_momentum_site_apply<E, Word>), shared by the device code and by the host replays
// tests/cpp/spin_{model,sector,measure,measure_columns,site,site_z,rdm,rdm_z,complex,momentum,momentum_site}_sanitize.cpp, which run it under AddressSanitizer +
// UBSan.  The kernels and the replays call THESE functions, so what a replay proves about them (every load inside its array, the
// state equal to spin_sector_unrank, the sums equal to the CSR row loop and to spin_measure_host bit for bit) holds for the
// kernels' rows as compiled.  No device construct in here: plain C++11.  spin_write_rows, spin_sector_unrank, spin_sector_rank
// and spin_measure_host do not use this file: they are written from the definitions and are what this walk is checked against.
//
// One row per lane.  The lane has its state s: the row number itself in the full space, the state of rank r in a sector
// (spin_unrank_row).  The diagonal is ALU work (spin_row_diagonal).  The off-diagonal terms are site masks taken kSpinBatch at a
// time, in three phases that the callers keep apart:
//   1. spin_flip_targets: which terms the row has (on[]) and the row each one reads (base[] + low[]).  A lane without the term keeps its
//      own state and so its own row, a line its wave has fetched anyway: no load is branched around where half the lanes diverge.
//      In a sector this is where the two rank tables are read, two 4-byte gathers per term.
//   2. all kSpinBatch loads of x (spin_gather), issued before the first product is added.
//   3. the products: spin_add_flips for the operator (rounded, then added, in table order: the CSR row loop's sum) or
//      spin_measure_flips for a measurement (one fma per term, a lane without the term adds x_s * 0).
// Every array has kSpinBatch entries and every loop over one a constant trip count: after unrolling and inlining a register array
// is only ever indexed by constants.
//
// The mask and value tables, which every lane reads at the same index, come as pointers to a batch's first entry.  All other
// memory is reached through accessor objects of the caller -- the kernels index raw pointers and LDS, the replays check first:
// binom(i) is C(p, k) at i = p * (kSectorMaxSites + 1) + k; tab.hi(i) and tab.lo(i) are hi_base and lo_rank; x(i) is the vector.
#pragma once
#include <stdint.h>

#include <cmath>

#include "spin_measure.hpp"
#include "spin_measure_columns.hpp"
#include "spmv_index.hpp"

#if defined(__clang__)
#define EIGENEX_UNROLL _Pragma("unroll")
#else
#define EIGENEX_UNROLL
#endif

namespace eigenex {

// Parity by population count, one instruction on the device.  Not spin_parity (spin_model.hpp), the folding form of the functions
// written from the definition: the walk shares no arithmetic with what it is checked against.
EIGENEX_HD bool spin_odd(uint32_t x) { return (__builtin_popcount(x) & 1) != 0; }
EIGENEX_HD bool spin_odd(uint64_t x) { return (__builtin_popcountll(x) & 1) != 0; }  // the 64-bit states of spin_momentum.hpp

// The state of rank r among the states of n_sites sites with n_up up (spin_sector.hpp: unrank), in 32-bit arithmetic: n_sites
// predicated steps, the same for every lane; k differs between lanes.  left and k end at 0 for every r below the dimension.
struct SpinUnranked {
  uint32_t s, left;
  int k;
};
template <class Binom>
EIGENEX_HD SpinUnranked spin_unrank_row(const Binom& binom, int n_sites, int n_up, uint32_t r) {
  SpinUnranked u = {0u, r, n_up};
  for (int p = n_sites - 1; p >= 0; --p) {
    const uint32_t c = binom(p * (kSectorMaxSites + 1) + u.k);
    const bool up = u.k > 0 && u.left >= c;
    u.s |= up ? uint32_t(1) << p : 0u;
    u.left -= up ? c : 0u;
    u.k -= up ? 1 : 0;
  }
  return u;
}

// The diagonal entry of row s from the (mask, constant) table of SpinOperatorView: plain additions of sign-flipped constants
EIGENEX_HD double spin_row_diagonal(const uint32_t* dmask, const double* dval, int ndiag, uint32_t s) {
  double d = 0.0;
  for (int t = 0; t < ndiag; ++t) {
    const double k = dval[t];
    d += spin_odd(s & dmask[t]) ? -k : k;
  }
  return d;
}
// ... of a 64-bit state from the 64-bit masks of SpinOperatorView64 (below): the same additions
EIGENEX_HD double spin_row_diagonal(const uint64_t* dmask, const double* dval, int ndiag, uint64_t s) {
  double d = 0.0;
  for (int t = 0; t < ndiag; ++t) {
    const double k = dval[t];
    d += spin_odd(s & dmask[t]) ? -k : k;
  }
  return d;
}

// Phase 1 of a batch of masks (mask[0 .. kSpinBatch)) on the row of state s.  One predicate for every caller: a one-bit mask (a
// transverse field, Sx) flips every row, a two-bit mask (a bond, a pair) the rows whose two spins differ, a zero mask (padding)
// never.  A sector has no one-bit masks (spin_sector_error and spin_measure_error refuse them: they leave the sector), so that
// half of the test, four scalar instructions per term, is compiled out there.  The row a term reads is base[t] + low[t]: the
// state itself and 0 in the full space, where tab, h and lo_mask are not looked at, hi_base[..] and lo_rank[..] in a sector.  The
// two words stay apart until the load (spin_gather), so that a load of x waits for its own table words and not for the batch's.
// Either of the two alone left k_spin_spmv<true> 1.3 - 2 % slower (profiles/spin_rows_refactor.md).
template <bool SECTOR, class Tables>
EIGENEX_HD void spin_flip_targets(const uint32_t* mask, uint32_t s, const Tables& tab, int h, uint32_t lo_mask, bool* on, uint32_t* base,
                                  uint32_t* low) {
  EIGENEX_UNROLL
  for (int t = 0; t < kSpinBatch; ++t) {
    const uint32_t m = mask[t];
    on[t] = (!SECTOR && __builtin_popcount(m) == 1) || __builtin_popcount(s & m) == 1;
    const uint32_t s2 = on[t] ? s ^ m : s;
    base[t] = SECTOR ? tab.hi(s2 >> h) : s2;
    low[t] = SECTOR ? tab.lo(s2 & lo_mask) : 0u;
  }
}

// An element of the vector is a double or, of an interleaved complex vector, a pair (re, im): x(i) of the caller's accessor
// returns one, which the kernels fill from one 8-byte or one 16-byte load.  The operator is real, so the lane's state, the
// diagonal and phase 1 above serve both parts of a complex element unchanged and once per row; phases 2 and 3 and the helpers
// below are written once per element.  Each part of a complex sum is the real walk's sum of that part: the same products, rounded
// and added in the same order.  E{} is the zero element of either.
struct SpinZ {
  double re, im;
};

// x * c and y + a * x with a real c and a, part by part, every product rounded before it is added
EIGENEX_HD double spin_scaled(double x, double c) { return x * c; }
EIGENEX_HD SpinZ spin_scaled(SpinZ x, double c) { return SpinZ{x.re * c, x.im * c}; }
EIGENEX_HD double spin_add_product(double y, double a, double x) { return add_product_nofma(y, a, x); }
EIGENEX_HD SpinZ spin_add_product(SpinZ y, double a, SpinZ x) { return SpinZ{add_product_nofma(y.re, a, x.re), add_product_nofma(y.im, a, x.im)}; }

// nrm + |x|^2: one fma, of a complex element the real part's, then the imaginary part's
EIGENEX_HD double spin_norm_add(double nrm, double x) { return std::fma(x, x, nrm); }
EIGENEX_HD double spin_norm_add(double nrm, SpinZ x) { return std::fma(x.im, x.im, std::fma(x.re, x.re, nrm)); }

// phase 2
template <class Vector, class E>
EIGENEX_HD void spin_gather(const Vector& x, const uint32_t* base, const uint32_t* low, E* xv) {
  EIGENEX_UNROLL
  for (int t = 0; t < kSpinBatch; ++t) xv[t] = x(base[t] + low[t]);
}

// phase 3 of the operator: yr + sum over the row's terms of fval[t] * (xv[t] * scale), every product rounded before it is added
EIGENEX_HD double spin_add_flips(double yr, const double* fval, const bool* on, const double* xv, double scale) {
  EIGENEX_UNROLL
  for (int t = 0; t < kSpinBatch; ++t)
    if (on[t]) yr = add_product_nofma(yr, fval[t], xv[t] * scale);
  return yr;
}
// ... of a complex vector: the same on each part
EIGENEX_HD SpinZ spin_add_flips(SpinZ yr, const double* fval, const bool* on, const SpinZ* xv, double scale) {
  EIGENEX_UNROLL
  for (int t = 0; t < kSpinBatch; ++t)
    if (on[t]) {
      yr.re = add_product_nofma(yr.re, fval[t], xv[t].re * scale);
      yr.im = add_product_nofma(yr.im, fval[t], xv[t].im * scale);
    }
  return yr;
}

// phase 3 of a measurement (spin_measure.hpp: flip[t]): one fma per term on every row
EIGENEX_HD void spin_measure_flips(double xs, const bool* on, const double* xv, double* fl) {
  EIGENEX_UNROLL
  for (int t = 0; t < kSpinBatch; ++t) fl[t] = std::fma(xs, on[t] ? xv[t] : 0.0, fl[t]);
}
// ... of a complex vector (flip[t] = Re(conj(x_s) x_{s ^ mask})): the real part's fma, then the imaginary part's
EIGENEX_HD void spin_measure_flips(SpinZ xs, const bool* on, const SpinZ* xv, double* fl) {
  EIGENEX_UNROLL
  for (int t = 0; t < kSpinBatch; ++t) {
    fl[t] = std::fma(xs.re, on[t] ? xv[t].re : 0.0, fl[t]);
    fl[t] = std::fma(xs.im, on[t] ? xv[t].im : 0.0, fl[t]);
  }
}

// a batch of diagonal terms of a measurement (spin_measure.hpp: diag[t]): the sign is the parity of the mask's down spins
EIGENEX_HD void spin_measure_diagonals(double xs, uint32_t s, const uint32_t* dmask, double* dg) {
  EIGENEX_UNROLL
  for (int t = 0; t < kSpinBatch; ++t) dg[t] = std::fma(spin_odd(~s & dmask[t]) ? -xs : xs, xs, dg[t]);
}
// ... of a complex vector (diag[t], sign |x_s|^2): real part, then imaginary part
EIGENEX_HD void spin_measure_diagonals(SpinZ xs, uint32_t s, const uint32_t* dmask, double* dg) {
  EIGENEX_UNROLL
  for (int t = 0; t < kSpinBatch; ++t) {
    const bool neg = spin_odd(~s & dmask[t]);
    dg[t] = std::fma(neg ? -xs.re : xs.re, xs.re, dg[t]);
    dg[t] = std::fma(neg ? -xs.im : xs.im, xs.im, dg[t]);
  }
}

// One row of a chunk's observables against kSpinMeasureColumns columns (spin_measure_columns.hpp; kernels.hip:
// k_spin_measure_columns<SECTOR>): the values w_t = (A_t x)(s) of a batch are formed once -- a sign times the row's own element
// xs, or the gathered x of phases 1 and 2 above, zero where the row has no entry -- and then meet every column's element v[j] in
// one fma each: sum[t * kSpinMeasureColumns + j] = fma(v[j], w_t, sum[..]).  A batch is skipped as a whole where the chunk has no
// term in it (ndiag and nflip are the same for every lane); a padded term (mask 0) sums into a slot nobody reads.
template <bool SECTOR, class Tables, class Vector>
EIGENEX_HD void spin_measure_columns_row(const uint32_t* dmask, int ndiag, const uint32_t* fmask, int nflip, uint32_t s, double xs, const Vector& x,
                                         const Tables& tab, int h, uint32_t lo_mask, const double* v, double* dg, double* fl) {
  EIGENEX_UNROLL
  for (int t0 = 0; t0 < kSpinMeasureChunk; t0 += kSpinBatch)
    if (t0 < ndiag) {
      EIGENEX_UNROLL
      for (int t = 0; t < kSpinBatch; ++t) {
        const double w = spin_odd(~s & dmask[t0 + t]) ? -xs : xs;
        EIGENEX_UNROLL
        for (int j = 0; j < kSpinMeasureColumns; ++j)
          dg[(t0 + t) * kSpinMeasureColumns + j] = std::fma(v[j], w, dg[(t0 + t) * kSpinMeasureColumns + j]);
      }
    }
  EIGENEX_UNROLL
  for (int t0 = 0; t0 < kSpinMeasureChunk; t0 += kSpinBatch)
    if (t0 < nflip) {
      bool on[kSpinBatch];
      uint32_t base[kSpinBatch], low[kSpinBatch];
      double xv[kSpinBatch];
      spin_flip_targets<SECTOR>(fmask + t0, s, tab, h, lo_mask, on, base, low);
      spin_gather(x, base, low, xv);
      EIGENEX_UNROLL
      for (int t = 0; t < kSpinBatch; ++t) {
        const double w = on[t] ? xv[t] : 0.0;
        EIGENEX_UNROLL
        for (int j = 0; j < kSpinMeasureColumns; ++j)
          fl[(t0 + t) * kSpinMeasureColumns + j] = std::fma(v[j], w, fl[(t0 + t) * kSpinMeasureColumns + j]);
      }
    }
}

// ---- a sum of site operators (spin_site.hpp; kernels.hip: k_spin_site_apply<SECTOR, E>), one row of the DESTINATION per lane ----
// The lane unranks its state s with the destination's n_up (spin_unrank_row).  Z is ALU work on the lane's own element
// (spin_site_weight).  PLUS and MINUS take the sites kSpinBatch at a time in the three phases above: spin_site_targets,
// spin_gather, spin_site_add.  The row has term i where bit i of `has` is set: has = s for PLUS (site i up in the row), ~s &
// site_mask for MINUS (down).  The flipped state s ^ 1<<i belongs to the SOURCE geometry and is ranked through the source's
// tables.  The fall-back of spin_flip_targets is not valid here: the lane's own state has the wrong number of up sites for those
// tables, so their sum may lie outside x.  A lane without the term ranks `fallback` instead, the lowest state of the source
// geometry: both table reads stay inside the tables, the row is 0, which every source vector has, no load is branched around,
// and spin_site_add does not look at what was loaded.
// The kernel is written once for both elements.  A complex vector has complex coefficients (cr, ci); real_coef, the same for every
// lane, says that every ci is zero, and then neither ci nor the products with it are looked at: each part of the result is the real
// walk's on that part of x, bit for bit (spin_site.hpp states the operations and their order).  SpinSiteCoefficients is what
// the table holds of either form for the sites from a batch's first on; the real overloads read `re` alone.
struct SpinSiteCoefficients {
  const double *re, *im;
  bool real_coef;
};

// w(s) of Z from the halved coefficients half[i] = c[i] * 0.5: plain additions of sign-flipped constants, sites ascending.  The
// state word is a parameter for the 64-bit representatives of a momentum sector (below); uint32_t is the function as it was.
template <class Word>
EIGENEX_HD double spin_site_weight(const double* half, int n_sites, Word s) {
  double w = 0.0;
  for (int i = 0; i < n_sites; ++i) {
    const double k = half[i];
    w += ((s >> i) & 1u) ? k : -k;
  }
  return w;
}

// phase 1 of the sites i0 .. i0 + kSpinBatch - 1 (i0 a multiple of kSpinBatch below n_sites, so every shift is below 32; a site at
// or above n_sites has no bit in `has`)
template <bool SECTOR, class Tables>
EIGENEX_HD void spin_site_targets(int i0, uint32_t s, uint32_t has, uint32_t fallback, const Tables& src_tab, int h, uint32_t lo_mask, bool* on,
                                  uint32_t* base, uint32_t* low) {
  EIGENEX_UNROLL
  for (int t = 0; t < kSpinBatch; ++t) {
    const uint32_t bit = uint32_t(1) << (i0 + t);
    on[t] = (has & bit) != 0;
    const uint32_t s2 = on[t] ? s ^ bit : fallback;
    base[t] = SECTOR ? src_tab.hi(s2 >> h) : s2;
    low[t] = SECTOR ? src_tab.lo(s2 & lo_mask) : 0u;
  }
}

// phase 3: one fma per term the row has, sites ascending; a lane without the term keeps its sum
EIGENEX_HD double spin_site_add(double yr, const double* coef, const bool* on, const double* xv) {
  EIGENEX_UNROLL
  for (int t = 0; t < kSpinBatch; ++t) yr = on[t] ? std::fma(coef[t], xv[t], yr) : yr;
  return yr;
}
// ... of a complex vector with complex coefficients: per term re += cr x.re, re -= ci x.im, im += cr x.im, im += ci x.re, one fma
// each; the second and the fourth not with real_coef
EIGENEX_HD SpinZ spin_site_add(SpinZ yr, const SpinSiteCoefficients& c, const bool* on, const SpinZ* xv) {
  if (c.real_coef) {
    EIGENEX_UNROLL
    for (int t = 0; t < kSpinBatch; ++t) {
      yr.re = on[t] ? std::fma(c.re[t], xv[t].re, yr.re) : yr.re;
      yr.im = on[t] ? std::fma(c.re[t], xv[t].im, yr.im) : yr.im;
    }
  } else {
    EIGENEX_UNROLL
    for (int t = 0; t < kSpinBatch; ++t) {
      yr.re = on[t] ? std::fma(-c.im[t], xv[t].im, std::fma(c.re[t], xv[t].re, yr.re)) : yr.re;
      yr.im = on[t] ? std::fma(c.im[t], xv[t].re, std::fma(c.re[t], xv[t].im, yr.im)) : yr.im;
    }
  }
  return yr;
}
EIGENEX_HD double spin_site_add(double yr, const SpinSiteCoefficients& c, const bool* on, const double* xv) { return spin_site_add(yr, c.re, on, xv); }

// Z: the row's weight, of a complex vector the pair (wr, wi) of the two halves of the halved coefficients (wi = 0.0 and not summed
// with real_coef), then its product with the row's own element, which the caller loads after the weight is formed.  The last
// argument of spin_site_weights only selects the element.
template <class Word>
EIGENEX_HD double spin_site_weights(const SpinSiteCoefficients& half, int n_sites, Word s, double) { return spin_site_weight(half.re, n_sites, s); }
template <class Word>
EIGENEX_HD SpinZ spin_site_weights(const SpinSiteCoefficients& half, int n_sites, Word s, SpinZ) {
  return SpinZ{spin_site_weight(half.re, n_sites, s), half.real_coef ? 0.0 : spin_site_weight(half.im, n_sites, s)};
}
EIGENEX_HD double spin_site_product(double w, bool, double x) { return w * x; }
EIGENEX_HD SpinZ spin_site_product(SpinZ w, bool real_coef, SpinZ x) {
  if (real_coef) return SpinZ{w.re * x.re, w.re * x.im};
  return SpinZ{std::fma(-w.im, x.im, w.re * x.re), std::fma(w.im, x.re, w.re * x.im)};
}

// ---- a momentum sector (spin_momentum.hpp; kernels.hip: k_spin_momentum_spmv<E> and k_spin_momentum_expand<E>) ----
// One row per lane; the lane's state is its representative reps[r], a coalesced load of the caller.  A bond flip s' = a ^ mask
// leaves the list of representatives, so phase 1 (spin_momentum_targets) runs the orbit of s' -- all n_trans rotations on every
// lane, no early exit: the trip count is the same for the whole wave -- and looks the representative up (spin_momentum_index).
// The search is a lower bound with the trip count `steps` of the upload, branch-free, in the bucket of the state's high bits.
// Every state it is given is a row of the sector, so the bucket is not empty and every probe lies inside it.  A lane without
// the term (the spins of the bond are equal, or the period of s' does not carry the momentum) searches for its own row's state
// under the rule of spin_flip_targets: no load is branched around.  The coefficient of a term is fval * ratio[ri] * phase[li],
// each product rounded (spin_momentum_value); ri = R_a * SpinWord<Word>::kRatioPitch + R_s' and li = (N - j*) mod N are valid table
// indices on every lane.  Phase 3 is the product form of the plain CSR kernels, so that an application equals the CSR upload of
// spin_momentum_write_rows' rows bit for bit: real  yr = add_product_nofma(yr, value.re, xv * scale);  complex  p =
// spin_cmul_nofma(value, x * scale), yr.re += p.re, yr.im += p.im, the diagonal (d, 0) included: k_spmv_z's stored-order sum.
// lk.reps(i) and lk.bucket(i) are the two arrays; tb.ratio(i), tb.phase_re(i), tb.phase_im(i), tb.inv_sqrt(i) the tables.
// The walk is written once for both state words, as the host side of spin_momentum.hpp is: Word = uint32_t (up to 32 sites) and
// Word = uint64_t (up to 48 sites; k_spin_momentum_spmv<E, uint64_t>).  SpinWord<Word> is the one description of what depends on
// the width: the bits, the population count, the limits of the ring and of the model, the longest period (a bit of `compatible`
// and an entry of the phase tables each), the pitch of the ratio table and the model's view, whose term tables hold kMaxTerms
// entries, a multiple of kSpinBatch.  The uint32_t instantiations are the functions this file had before the word became a
// parameter, expression for expression.
struct SpinOperatorView64;
template <class Word>
struct SpinWord;
template <>
struct SpinWord<uint32_t> {
  typedef SpinOperatorView Model;
  static constexpr int kBits = 32, kMaxSites = kSectorMaxSites, kMaxBonds = kSpinMaxBonds, kMaxTerms = kSpinMaxTerms;
  static constexpr int kMaxPeriod = kMaxSites, kRatioPitch = kMaxPeriod + 1;
  static EIGENEX_HD int popcount(uint32_t x) { return __builtin_popcount(x); }
};
template <>
struct SpinWord<uint64_t> {
  typedef SpinOperatorView64 Model;
  static constexpr int kBits = 64, kMaxSites = 48, kMaxBonds = 128, kMaxTerms = (kMaxBonds + kMaxSites + kSpinBatch - 1) / kSpinBatch * kSpinBatch;
  static constexpr int kMaxPeriod = kMaxSites, kRatioPitch = kMaxPeriod + 1;
  static EIGENEX_HD int popcount(uint64_t x) { return __builtin_popcountll(x); }
};
// SpinOperatorView (spin_model.hpp) with 64-bit masks; no transverse field, so every flip mask has two bits
struct SpinOperatorView64 {
  int n_sites, ndiag, nflip, pad;
  uint64_t dmask[SpinWord<uint64_t>::kMaxTerms], fmask[SpinWord<uint64_t>::kMaxTerms];
  double dval[SpinWord<uint64_t>::kMaxTerms], fval[SpinWord<uint64_t>::kMaxTerms];
};

template <class Word>
EIGENEX_HD Word spin_rotate(Word s, int n_sites, int cell, Word site_mask) {
  return ((s << cell) | (s >> (n_sites - cell))) & site_mask;  // both shifts are 1..31 (1..47 of a 64-bit word): cell <= n_sites / 2
}

// the representative of the orbit of s, the smallest j >= 0 with T^j s = rep and the period: n_trans rotations, always
template <class Word>
struct SpinOrbitOf {
  Word rep;
  int j, period;
};
typedef SpinOrbitOf<uint32_t> SpinOrbit;
template <class Word>
EIGENEX_HD SpinOrbitOf<Word> spin_orbit(Word s, int n_sites, int cell, int n_trans) {
  const Word site_mask = Word(~Word(0)) >> (SpinWord<Word>::kBits - n_sites);
  SpinOrbitOf<Word> o = {s, 0, n_trans};
  Word t = s;
  bool closed = false;
  for (int r = 1; r <= n_trans; ++r) {
    t = spin_rotate(t, n_sites, cell, site_mask);
    const bool smaller = t < o.rep;  // strictly: the first of equal rotations stays
    o.rep = smaller ? t : o.rep;
    o.j = smaller ? r : o.j;
    const bool first_return = !closed && t == s;
    o.period = first_return ? r : o.period;
    closed = closed || first_return;
  }
  return o;
}

// idx(b) of a representative b of the sector: the lower bound of b in its bucket, `steps` probes
template <class Lookup, class Word>
EIGENEX_HD uint32_t spin_momentum_index(const Lookup& lk, Word b, int h, int steps) {
  uint32_t base = lk.bucket((uint32_t)(b >> h));  // at most 24 bits are left of a 64-bit state
  uint32_t n = lk.bucket((uint32_t)(b >> h) + 1) - base;  // >= 1: b is in there
  for (int i = 0; i < steps; ++i) {
    const uint32_t half = n >> 1;
    const Word v = lk.reps(base + (half ? half - 1 : 0));
    base += (half && v < b) ? half : 0u;
    n -= half;
  }
  return base;
}

// phase 1 of a batch of bond masks on the row of representative s with period `period`
template <class Lookup, class Word>
EIGENEX_HD void spin_momentum_targets(const Word* mask, Word s, int period, int n_sites, int cell, int n_trans, Word compatible, int h, int steps,
                                      const Lookup& lk, bool* on, uint32_t* column, int* ri, int* li) {
  EIGENEX_UNROLL
  for (int t = 0; t < kSpinBatch; ++t) {
    const Word m = mask[t];
    const bool flips = SpinWord<Word>::popcount(s & m) == 1;  // two-bit masks only; a zero mask (padding) never
    const SpinOrbitOf<Word> o = spin_orbit(flips ? s ^ m : s, n_sites, cell, n_trans);
    on[t] = flips && ((compatible >> (o.period - 1)) & 1u) != 0;
    column[t] = spin_momentum_index(lk, on[t] ? o.rep : s, h, steps);
    ri[t] = period * SpinWord<Word>::kRatioPitch + o.period;
    li[t] = o.j == 0 ? 0 : n_trans - o.j;
  }
}

// phase 2
template <class Vector, class E>
EIGENEX_HD void spin_momentum_gather(const Vector& x, const uint32_t* column, E* xv) {
  EIGENEX_UNROLL
  for (int t = 0; t < kSpinBatch; ++t) xv[t] = x(column[t]);
}

// a * b of two complex numbers as a plain C multiply without contraction (kernels.hip: cmul_nofma)
EIGENEX_HD SpinZ spin_cmul_nofma(SpinZ a, SpinZ b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double rr = a.re * b.re, ii = a.im * b.im, ri = a.re * b.im, ir = a.im * b.re;
  return SpinZ{rr - ii, ri + ir};
}

// the stored value of a term: c = fval * ratio, then (c * phase.re, c * phase.im)
EIGENEX_HD SpinZ spin_momentum_value(double fval, double ratio, double phase_re, double phase_im) {
  const double c = fval * ratio;
  return SpinZ{c * phase_re, c * phase_im};
}

// one stored entry of a row added to its sum
EIGENEX_HD double spin_momentum_add(double yr, SpinZ value, double x, double scale) { return add_product_nofma(yr, value.re, x * scale); }
EIGENEX_HD SpinZ spin_momentum_add(SpinZ yr, SpinZ value, SpinZ x, double scale) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const SpinZ p = spin_cmul_nofma(value, spin_scaled(x, scale));
  return SpinZ{yr.re + p.re, yr.im + p.im};
}

// phase 3, in table order
template <class Tables, class E>
EIGENEX_HD E spin_momentum_add_flips(E yr, const double* fval, const Tables& tb, const bool* on, const int* ri, const int* li, const E* xv,
                                     double scale) {
  EIGENEX_UNROLL
  for (int t = 0; t < kSpinBatch; ++t)
    if (on[t]) yr = spin_momentum_add(yr, spin_momentum_value(fval[t], tb.ratio(ri[t]), tb.phase_re(li[t]), tb.phase_im(li[t])), xv[t], scale);
  return yr;
}

// expand (spin_momentum.hpp), one row of the DESTINATION (the Sz sector) per lane: the orbit of the lane's state s, the lookup of
// its representative -- `fallback`, the sector's first row, where the representative does not carry the momentum -- one gather and
// one product.  x * phase is the plain complex multiply (of a real vector x * phase.re), then each part times inv_sqrt[R].
EIGENEX_HD double spin_momentum_expanded(double x, double phase_re, double, double w) { return (x * phase_re) * w; }
EIGENEX_HD SpinZ spin_momentum_expanded(SpinZ x, double phase_re, double phase_im, double w) {
  const SpinZ p = spin_cmul_nofma(x, SpinZ{phase_re, phase_im});
  return SpinZ{p.re * w, p.im * w};
}
template <class Lookup, class Tables, class Vector, class E>
EIGENEX_HD E spin_momentum_expand_row(uint32_t s, int n_sites, int cell, int n_trans, uint32_t compatible, uint32_t fallback, int h, int steps,
                                      const Lookup& lk, const Tables& tb, const Vector& x, E zero) {
  const SpinOrbit o = spin_orbit(s, n_sites, cell, n_trans);
  const bool on = ((compatible >> (o.period - 1)) & 1u) != 0;
  const E xv = x(spin_momentum_index(lk, on ? o.rep : fallback, h, steps));
  const int l = o.j == 0 ? 0 : n_trans - o.j;
  return on ? spin_momentum_expanded(xv, tb.phase_re(l), tb.phase_im(l), tb.inv_sqrt(o.period)) : zero;
}

// Diagonal correlations in the momentum basis (spin_momentum.hpp; kernels.hip: k_spin_momentum_measure<E, Word>), one row
// per lane: w = |x_a|^2 of the row's own element, then for a batch of masks the integer c_t(a) = sum over all n_trans rotations
// T^r a of the product of sigma over the mask -- the full trip count on every lane -- and one fma per term.
EIGENEX_HD double spin_momentum_weight(double x) { return x * x; }
EIGENEX_HD double spin_momentum_weight(SpinZ x) { return std::fma(x.im, x.im, x.re * x.re); }
template <class Word>
EIGENEX_HD void spin_momentum_measure_diagonals(double w, Word s, const uint64_t* dmask, int n_sites, int cell, int n_trans, double* dg) {
  const Word site_mask = Word(~Word(0)) >> (SpinWord<Word>::kBits - n_sites);
  int c[kSpinBatch];
  EIGENEX_UNROLL
  for (int t = 0; t < kSpinBatch; ++t) c[t] = 0;
  Word state = s;
  for (int r = 0; r < n_trans; ++r) {
    EIGENEX_UNROLL
    for (int t = 0; t < kSpinBatch; ++t) c[t] += spin_odd(Word(~state & (Word)dmask[t])) ? -1 : 1;
    state = spin_rotate(state, n_sites, cell, site_mask);
  }
  EIGENEX_UNROLL
  for (int t = 0; t < kSpinBatch; ++t) dg[t] = std::fma((double)c[t], w, dg[t]);
}

// A sum of site operators between two momentum sectors (spin_momentum_site.hpp; kernels.hip: k_spin_momentum_site_apply<E, Word>),
// one row of the DESTINATION sector per lane: the lane's state is the destination's representative b = reps_dst[r], its period
// R_b comes from one orbit walk.  Everything that is looked up -- the list of representatives and its buckets (src), h, steps,
// `compatible`, the ratio and phase tables -- is the SOURCE sector's.  Z is one search and one product
// (spin_momentum_site_z_row).  PLUS and MINUS take the sites kSpinBatch at a time in the three phases of the operator walk: the
// row has term i where bit i of `has` is set (has = b for PLUS, ~b & site_mask for MINUS); the flipped state b ^ 1<<i is a state
// of the source's magnetisation, its orbit is walked -- n_trans rotations on every lane -- and its representative searched with
// the fixed trip count.  A lane without the term, or whose flipped state has a period that does not carry the source momentum,
// searches for `fallback`, the source's first row, and its sum ignores what it loaded: no load is branched around, and every
// state handed to spin_momentum_index is a row of the source list.  (The lane's own state will not do: it is a row of the
// other sector.)  A lane without the term walks the orbit of its own state, so that ri and li are valid table indices on
// every lane.  Phase 3 is spin_momentum_expanded on what was loaded -- x times the source phase, then times sqrt(R_b / R_s') --
// and the fmas of spin_site_add with the site's coefficient.
template <class Lookup, class Word>
EIGENEX_HD void spin_momentum_site_targets(int i0, Word s, Word has, int period, int n_sites, int cell, int n_trans, Word compatible, Word fallback,
                                           int h, int steps, const Lookup& src, bool* on, uint32_t* column, int* ri, int* li) {
  EIGENEX_UNROLL
  for (int t = 0; t < kSpinBatch; ++t) {
    const Word bit = Word(1) << (i0 + t);  // i0 < n_sites is a multiple of kSpinBatch: the shift is below the word's bits
    const bool term = (has & bit) != 0;
    const SpinOrbitOf<Word> o = spin_orbit(term ? Word(s ^ bit) : s, n_sites, cell, n_trans);
    on[t] = term && ((compatible >> (o.period - 1)) & 1u) != 0;
    column[t] = spin_momentum_index(src, on[t] ? o.rep : fallback, h, steps);
    ri[t] = period * SpinWord<Word>::kRatioPitch + o.period;
    li[t] = o.j == 0 ? 0 : n_trans - o.j;
  }
}

// phase 3, sites ascending
template <class Tables, class E>
EIGENEX_HD E spin_momentum_site_add(E yr, const SpinSiteCoefficients& c, const Tables& tb, const bool* on, const int* ri, const int* li, const E* xv) {
  E xt[kSpinBatch];
  EIGENEX_UNROLL
  for (int t = 0; t < kSpinBatch; ++t) xt[t] = spin_momentum_expanded(xv[t], tb.phase_re(li[t]), tb.phase_im(li[t]), tb.ratio(ri[t]));
  return spin_site_add(yr, c, on, xt);
}

// Z: w(b) x[idx_src(b)] where b is a row of the source sector too (its period carries the source momentum), else zero
template <class Lookup, class Vector, class Word, class E>
EIGENEX_HD E spin_momentum_site_z_row(Word s, int period, int n_sites, Word compatible, Word fallback, int h, int steps, const Lookup& src,
                                      const SpinSiteCoefficients& half, const Vector& x, E zero) {
  const bool on = ((compatible >> (period - 1)) & 1u) != 0;
  const E w = spin_site_weights(half, n_sites, s, zero);
  const E xv = x(spin_momentum_index(src, on ? s : fallback, h, steps));
  return on ? spin_site_product(w, half.real_coef, xv) : zero;
}

}  // namespace eigenex

// the index arithmetic of the reduced-density-matrix kernel (k_spin_rdm<SECTOR, TILE, E>), under the same rules
#include "spin_rdm_rows.hpp"
