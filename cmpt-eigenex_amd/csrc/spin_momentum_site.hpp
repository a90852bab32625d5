// A sum of single-site spin operators that carries a momentum, applied to a vector of one momentum sector of spin_momentum.hpp;
// the result lives in another momentum sector (host side, no HIP), written once for both state words as spin_momentum.hpp is:
// the definition, the argument check, the table of the kernel (kernels.hip: k_spin_momentum_site_apply<E, Word>) and the host
// evaluation.  Shared by the library (eigenex_spin_momentum_site_apply, _z and _host) and by the host program
// tests/cpp/spin_momentum_site_sanitize.cpp, which runs this file under AddressSanitizer + UBSan.  NOT part of the reference.
//
// The conventions are those of spin_momentum.hpp: L = n_sites, cell a, N = L / a, T moves site i to site (i + a) mod L, and
// |a(k)> = (sqrt(R_a) / N) sum_r e^{-ikr} T^r |a>, k = 2 pi m / N.
// Input.  The source sector (L, n_up, a, m); a kind (kSpinSiteZ / Plus / Minus of spin_site.hpp); an integer p in 0..N-1; a
//   complex cell coefficients cc[j] = (cell_re[j], cell_im[j]), cell_im NULL meaning zeros.
// Site coefficients.  They are never given per site: c[j + a r] = spin_cmul_nofma(cc[j], u[r]) for j < a, r < N, with
//   u[r] = (phase_re[r], -phase_im[r]) of spin_momentum_build_tables(N, p), i.e. u[r] = e^{+2 pi i ((p r) mod N) / N}, exactly
//   1, i, -1, -i at quarter turns.  half[i] = c[i] * 0.5, each part.  O = sum_i c[i] S^kind_i then obeys T O T^-1 = e^{-2 pi i p / N} O.
//   real_coef: every c[i].im == 0.0 (-0.0 counts as zero).
// Destination.  n_up' = n_up (Z), n_up + 1 (PLUS), n_up - 1 (MINUS); m' = (m - p + N) mod N.  (One magnon: sum_j e^{i theta j} Sz_j
//   takes k to k - theta.)  Both sectors must have rows.
// Row b of the destination, b a representative of the destination sector with period R_b.  "compatible with m": (m R) mod N == 0.
// All tables below (ratio, phase) are the SOURCE sector's, spin_momentum_build_tables(N, m); idx_src is the row in the source.
//   Z      if R_b is compatible with m:  y_b = spin_site_product(w(b), real_coef, x[idx_src(b)]), w(b) = the sum over i ascending
//          of +half[i] (site i up in b) or -half[i] (down), each part (spin_site.hpp: Z; the imaginary part not with real_coef);
//          otherwise y_b = 0.
//   PLUS, MINUS   y_b = 0, then for i ascending over the sites that are up (PLUS) or down (MINUS) in b:  s' = b ^ (1 << i),
//          rep(s') = T^{j*} s' with the smallest j* >= 0, l = (N - j*) mod N.  If R_s' is compatible with m:
//            xt = spin_momentum_expanded(x[idx_src(rep(s'))], phase[l], ratio[R_b][R_s'])
//               = (x * phase[l]) * sqrt((double)R_b / (double)R_s'), the product a plain complex multiply without contraction (of a
//                 real vector x * phase.re), then each part scaled;
//            y.re = fma(c.re, xt.re, y.re);  y.re = fma(-c.im, xt.im, y.re)   (the second not with real_coef)
//            y.im = fma(c.re, xt.im, y.im);  y.im = fma(c.im, xt.re, y.im)    (the second not with real_coef)
//          This is <b(k')| O |a(k)> = c[i] sqrt(R_b / R_s') phase[l], phase[l] = e^{i k j*}: the factor of a row of H_k.
//   norm2  = sum_b |y_b|^2: per row the fma of the real part, then that of the imaginary part, rows ascending.
// Why: expand (spin_momentum.hpp) writes psi(s) = x[idx(rep s)] phase[(N - j*) mod N] / sqrt(R_s); (O psi)(b) is the sum above over
// psi(s'), and the destination's coefficient of a representative is y_b = sqrt(R_b) (O psi)(b).  So
//   expand_dst(y) = (sum_i c[i] S^kind_i) expand_src(x),
// which tests/test_spin_momentum_site_host.py checks against eigenex_spin_site_apply_host_z for every kind.
// Real form.  When m, m' and every coefficient are real -- m and m' each 0 or N/2, cell_im NULL or zeros -- every phase is +-1 or 0
// and x, y may be real vectors: the real overloads of the same functions, i.e. each part of the complex result on its own.
#pragma once
#include <stdint.h>

#include <cmath>
#include <memory>
#include <string>

#include "spin_momentum.hpp"
#include "spin_site.hpp"

namespace eigenex {

constexpr int kMomentumSiteMaxSites = SpinWord<uint64_t>::kMaxSites;
static_assert(kMomentumSiteMaxSites % kSpinBatch == 0 && SpinWord<uint32_t>::kMaxSites % kSpinBatch == 0,
              "the kernel takes the sites kSpinBatch at a time over a table of kMomentumSiteMaxSites");

struct SpinMomentumSiteArgs {
  int n_sites, n_up, cell, momentum;  // the source sector
  int kind, p;
  const double *cell_re, *cell_im;  // `cell` entries each; cell_im may be NULL
};

inline int spin_momentum_site_dst_up(int n_up, int kind) { return kind == kSpinSiteZ ? n_up : (kind == kSpinSitePlus ? n_up + 1 : n_up - 1); }
inline int spin_momentum_site_dst_momentum(int n_trans, int momentum, int p) { return (momentum - p + n_trans) % n_trans; }

// "" if the call is valid for the word (both sectors may still be empty), else what is wrong with it
template <class Word>
inline std::string spin_momentum_site_error(const SpinMomentumSiteArgs& a) {
  const std::string geo = spin_momentum_geometry_error<Word>(a.n_sites, a.n_up, a.cell, a.momentum);
  if (!geo.empty()) return geo;
  if (a.kind != kSpinSiteZ && a.kind != kSpinSitePlus && a.kind != kSpinSiteMinus) return "kind must be EIGENEX_SPIN_SITE_Z, _PLUS or _MINUS";
  if (a.p < 0 || a.p >= a.n_sites / a.cell) return "p must be 0..n_sites/cell - 1";
  if (!a.cell_re) return "the cell coefficients are NULL";
  for (int j = 0; j < a.cell; ++j)
    if (!std::isfinite(a.cell_re[j]) || (a.cell_im && !std::isfinite(a.cell_im[j]))) return "a coefficient is not finite";
  const int want = spin_momentum_site_dst_up(a.n_up, a.kind);
  if (want < 0 || want > a.n_sites)
    return "the destination sector lies outside 0..n_sites: S+ of the sector with every site up, or S- of the one with every site down, is zero";
  return "";
}

// no imaginary part among the cell coefficients (-0.0 counts as zero)
inline bool spin_momentum_site_real_cell(const SpinMomentumSiteArgs& a) {
  for (int j = 0; a.cell_im && j < a.cell; ++j)
    if (a.cell_im[j] != 0.0) return false;
  return true;
}

// the real form applies: real vectors may be used
inline bool spin_momentum_site_is_real(const SpinMomentumSiteArgs& a) {
  const int n_trans = a.n_sites / a.cell;
  return spin_momentum_is_real(n_trans, a.momentum) && spin_momentum_is_real(n_trans, spin_momentum_site_dst_momentum(n_trans, a.momentum, a.p)) &&
         spin_momentum_site_real_cell(a);
}

// What k_spin_momentum_site_apply receives besides the source's view (device memory; every lane reads the same entry): the site
// coefficients and their halves, padded with 0.0 up to kMomentumSiteMaxSites, a multiple of kSpinBatch; first_rep, the state a lane
// without a term looks up, and compatible, both the SOURCE sector's, as 64-bit words for either state word.
struct SpinMomentumSiteTable {
  int kind, real_coef;
  uint64_t first_rep, compatible;
  double coef[kMomentumSiteMaxSites], coef_im[kMomentumSiteMaxSites], half[kMomentumSiteMaxSites], half_im[kMomentumSiteMaxSites];
};
static_assert(sizeof(SpinMomentumSiteTable) == 24 + 4 * 8 * 48, "what the kernels read does not move");

// the table of a valid call; first_rep is the source sector's first row.  The word only selects the phase tables' size.
template <class Word>
inline void spin_momentum_site_build_table(const SpinMomentumSiteArgs& a, Word first_rep, SpinMomentumSiteTable& t) {
  const int n_trans = a.n_sites / a.cell;
  t = SpinMomentumSiteTable();
  t.kind = a.kind, t.first_rep = first_rep;
  for (int r = 1; r <= n_trans; ++r)
    if ((a.momentum * r) % n_trans == 0) t.compatible |= uint64_t(1) << (r - 1);
  std::unique_ptr<SpinMomentumTablesOf<Word>> u(new SpinMomentumTablesOf<Word>());
  spin_momentum_build_tables(n_trans, a.p, *u);
  t.real_coef = 1;
  for (int r = 0; r < n_trans; ++r)
    for (int j = 0; j < a.cell; ++j) {
      const SpinZ c = spin_cmul_nofma(SpinZ{a.cell_re[j], a.cell_im ? a.cell_im[j] : 0.0}, SpinZ{u->phase_re[r], -u->phase_im[r]});
      const int i = j + a.cell * r;
      t.coef[i] = c.re, t.coef_im[i] = c.im, t.half[i] = c.re * 0.5, t.half_im[i] = c.im * 0.5;
      if (c.im != 0.0) t.real_coef = 0;
    }
}

// The definition, evaluated over the rows of two built bases of one (n_sites, cell) -- src the source sector, dst the destination
// as the definition wants it -- with the source's tables and the table of the call: x has one double (is_complex false; the real
// form) or an interleaved pair per row of src, y per row of dst; norm2 may be NULL.  y may be x for Z with p = 0 only.  Orbits and
// rows through spin_momentum_orbit_host and spin_momentum_row_of, not through the row walk of spin_rows.hpp.
template <class Word>
inline void spin_momentum_site_apply_host(const SpinMomentumBasisOf<Word>& src, const SpinMomentumBasisOf<Word>& dst, const SpinMomentumTablesOf<Word>& ts,
                                          const SpinMomentumSiteTable& tb, bool is_complex, const double* x, double* y, double* norm2) {
#if defined(__clang__)
#pragma clang fp contract(off)  // a host compiler other than clang needs -ffp-contract=off, as for add_product_nofma
#endif
  const int L = src.n_sites, N = src.n_trans, m = src.momentum;
  const bool real_coef = tb.real_coef != 0;
  double nrm = 0.0;
  for (size_t r = 0; r < dst.reps.size(); ++r) {
    const Word b = dst.reps[r];
    const int Rb = dst.period[r];
    double yre = 0.0, yim = 0.0;
    if (tb.kind == kSpinSiteZ) {
      const int64_t row = (m * Rb) % N == 0 ? spin_momentum_row_of(src, b) : -1;
      if (row >= 0) {
        double wr = 0.0, wi = 0.0;
        for (int i = 0; i < L; ++i) wr += ((b >> i) & 1u) ? tb.half[i] : -tb.half[i];
        for (int i = 0; !real_coef && i < L; ++i) wi += ((b >> i) & 1u) ? tb.half_im[i] : -tb.half_im[i];
        if (!is_complex) {
          yre = wr * x[row];
        } else {
          const double xre = x[2 * row], xim = x[2 * row + 1];
          yre = real_coef ? wr * xre : std::fma(-wi, xim, wr * xre);
          yim = real_coef ? wr * xim : std::fma(wi, xre, wr * xim);
        }
      }
    } else {
      for (int i = 0; i < L; ++i) {
        const bool up = ((b >> i) & 1u) != 0;
        if (up != (tb.kind == kSpinSitePlus)) continue;
        const SpinMomentumOrbitOf<Word> o = spin_momentum_orbit_host(Word(b ^ (Word(1) << i)), L, src.cell);
        if ((m * o.period) % N != 0) continue;
        const int64_t row = spin_momentum_row_of(src, o.rep);  // >= 0: a compatible representative of the source's magnetisation
        const int l = (N - o.j) % N;
        const double pr = ts.phase_re[l], pi = ts.phase_im[l], w = ts.ratio[Rb * SpinWord<Word>::kRatioPitch + o.period];
        if (!is_complex) {
          const double xt = (x[row] * pr) * w;
          yre = std::fma(tb.coef[i], xt, yre);
        } else {
          const double xre = x[2 * row], xim = x[2 * row + 1];
          const double p1 = xre * pr, p2 = xim * pi, p3 = xre * pi, p4 = xim * pr;  // each product rounded
          const double tre = (p1 - p2) * w, tim = (p3 + p4) * w;
          yre = std::fma(tb.coef[i], tre, yre);
          if (!real_coef) yre = std::fma(-tb.coef_im[i], tim, yre);
          yim = std::fma(tb.coef[i], tim, yim);
          if (!real_coef) yim = std::fma(tb.coef_im[i], tre, yim);
        }
      }
    }
    if (!is_complex) {
      y[r] = yre;
      nrm = std::fma(yre, yre, nrm);
    } else {
      y[2 * r] = yre, y[2 * r + 1] = yim;
      nrm = std::fma(yim, yim, std::fma(yre, yre, nrm));
    }
  }
  if (norm2) *norm2 = nrm;
}

}  // namespace eigenex
