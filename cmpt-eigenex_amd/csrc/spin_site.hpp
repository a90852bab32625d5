// A sum of single-site spin operators applied to a real or a complex vector over the rows of a spin-1/2 operator (host side, no
// HIP): the definition, the argument check, the table of the kernel (kernels.hip: k_spin_site_apply<SECTOR, E>) and the host
// evaluations.  Shared by the library (eigenex_spin_site_apply, eigenex_spin_site_apply_z and their _host definitions) and by the
// host programs tests/cpp/spin_site_sanitize.cpp and spin_site_z_sanitize.cpp, which run this file under AddressSanitizer +
// UBSan.  NOT part of the reference.
//
// The rows are those of spin_model.hpp (n_up = -1: the full space, row s is state s) or of spin_sector.hpp (row r is the state
// of rank r among the states with n_up sites up).  sigma_i(s) = +1 if bit i of s is set, else -1.  A site operator is a kind and
// n_sites real coefficients c[i]; x lives on the source geometry (n_sites, n_up_src), y on the destination's:
//   Z      y_r = w(s_r) * x_r;  w(s) = 0.0, then for i ascending  w += sigma_i(s) > 0 ? +(c[i] * 0.5) : -(c[i] * 0.5)
//          -- plain additions of sign-flipped constants, as for the operator's diagonal.  Destination = source.
//   PLUS   y = sum_i c[i] S+_i x.  Destination: the sector n_up_src + 1, or the full space if the source is the full space.
//          Row t of the destination, whose state is s_t:  y_t = 0.0, then for i ascending with site i UP in s_t
//          y_t = fma(c[i], x[row_src(s_t ^ 1<<i)], y_t)
//   MINUS  y = sum_i c[i] S-_i x: the same with "site i DOWN in s_t".  Destination: the sector n_up_src - 1, or the full space.
//   norm2  = sum_r y_r^2, one fma per row, rows ascending
// Of a complex vector (x and y interleaved (re, im), spin_site_apply_host_z) the coefficients are complex, c[i] = (cr[i], ci[i]);
// real_coef says that there is no imaginary part (coef_im NULL or all zero).  With wr = w of cr and wi = w of ci as above:
//   Z      real_coef:  y.re = wr * x.re                      y.im = wr * x.im
//          otherwise:  y.re = fma(-wi, x.im, wr * x.re)      y.im = fma(wi, x.re, wr * x.im)
//   PLUS, MINUS  y = (0.0, 0.0), then for i ascending over the terms the row has, with x the element the term reads,
//          y.re = fma(cr[i], x.re, y.re);  y.re = fma(-ci[i], x.im, y.re)  (not with real_coef)
//          y.im = fma(cr[i], x.im, y.im);  y.im = fma(ci[i], x.re, y.im)   (not with real_coef)
//   norm2  = sum_r |y_r|^2: per row the fma of the real part, then that of the imaginary part, rows ascending
// With real_coef each part of y is the real call on that part of x, bit for bit.
#pragma once
#include <stdint.h>

#include <cmath>
#include <vector>

#include "spin_sector.hpp"

namespace eigenex {

constexpr int kSpinSiteZ = 0, kSpinSitePlus = 1, kSpinSiteMinus = 2;  // EIGENEX_SPIN_SITE_* of eigenex_hip.h
static_assert(kSectorMaxSites % kSpinBatch == 0, "the kernel takes the sites kSpinBatch at a time over a table of kSectorMaxSites");

struct SpinSiteArgs {
  int n_sites, n_up_src;  // the source; n_up = -1: the full space
  int kind;
  const double* coef;     // n_sites entries
  int n_sites_dst, n_up_dst;  // the destination as the caller has it (spin_site_dst_up: as the kind wants it)
  const double* coef_im;      // the imaginary parts of complex coefficients (the _z calls); NULL: none
  // the real call's six members in their order, or all seven (constructors, so that a list of six stays complete)
  SpinSiteArgs(int n_sites_, int n_up_src_, int kind_, const double* coef_, int n_sites_dst_, int n_up_dst_, const double* coef_im_ = nullptr)
      : n_sites(n_sites_), n_up_src(n_up_src_), kind(kind_), coef(coef_), n_sites_dst(n_sites_dst_), n_up_dst(n_up_dst_), coef_im(coef_im_) {}
};

// the destination's n_up for a source and a kind (of a valid kind); may lie outside 0..n_sites, which spin_site_error refuses
inline int spin_site_dst_up(int n_up_src, int kind) {
  return n_up_src == -1 || kind == kSpinSiteZ ? n_up_src : (kind == kSpinSitePlus ? n_up_src + 1 : n_up_src - 1);
}

// nullptr if the call is valid, else what is wrong with it
inline const char* spin_site_error(const SpinSiteArgs& a) {
  if (a.kind != kSpinSiteZ && a.kind != kSpinSitePlus && a.kind != kSpinSiteMinus) return "kind must be EIGENEX_SPIN_SITE_Z, _PLUS or _MINUS";
  const bool sector = a.n_up_src != -1;
  if (!sector && (a.n_sites < kSpinMinSites || a.n_sites > kSpinMaxSites)) return "n_sites must be 2..30 in the full space";
  if (sector && (a.n_sites < kSpinMinSites || a.n_sites > kSectorMaxSites)) return "n_sites must be 2..32";
  if (sector && (a.n_up_src < 0 || a.n_up_src > a.n_sites)) return "n_up must be 0..n_sites, or -1 for the full space";
  if (!a.coef) return "coef is NULL";
  for (int i = 0; i < a.n_sites; ++i)
    if (!std::isfinite(a.coef[i]) || (a.coef_im && !std::isfinite(a.coef_im[i]))) return "a coefficient is not finite";
  const int want = spin_site_dst_up(a.n_up_src, a.kind);
  if (sector && (want < 0 || want > a.n_sites))
    return "the destination sector lies outside 0..n_sites: S+ of the sector with every site up, or S- of the one with every site down, is zero";
  if (a.n_sites_dst != a.n_sites || a.n_up_dst != want)
    return "source and destination do not belong together: Z keeps the geometry, PLUS needs the sector n_up + 1 and MINUS the sector n_up - 1 of the "
           "same sites (the full space goes to the full space)";
  return nullptr;
}

// rows of a valid geometry
inline int64_t spin_site_rows(int n_sites, int n_up) { return n_up == -1 ? int64_t(1) << n_sites : spin_sector_dim(n_sites, n_up); }

// What k_spin_site_apply receives (device memory; every lane reads the same entry): the coefficients and their halves, padded
// with 0.0 up to kSectorMaxSites, a multiple of kSpinBatch.  site_mask has the bits of the n_sites sites (MINUS: the row has term i
// where bit i of ~s & site_mask is set; spin_rows.hpp: spin_site_targets); fallback is the state a lane without the term ranks
// instead of its own, which has the wrong number of up sites for the source's tables -- the lowest state of the SOURCE geometry,
// whose row is 0.  The imaginary parts, their halves and real_coef come after what the real kernel reads, whose offsets so stay.
struct SpinSiteTable {
  int kind, n_sites;
  uint32_t site_mask, fallback;
  double coef[kSectorMaxSites], half[kSectorMaxSites];
  double coef_im[kSectorMaxSites], half_im[kSectorMaxSites];
  int real_coef;  // 1: coef_im is NULL or all zero
};

// no imaginary part among the n_sites coefficients (-0.0 counts as zero)
inline bool spin_site_real_coef(const SpinSiteArgs& a) {
  for (int i = 0; a.coef_im && i < a.n_sites; ++i)
    if (a.coef_im[i] != 0.0) return false;
  return true;
}

inline void spin_site_build_table(const SpinSiteArgs& a, SpinSiteTable& t) {
  t = SpinSiteTable();
  t.kind = a.kind, t.n_sites = a.n_sites;
  t.site_mask = a.n_sites < 32 ? (uint32_t(1) << a.n_sites) - 1 : ~uint32_t(0);
  t.fallback = a.n_up_src <= 0 ? 0u : (a.n_up_src < 32 ? (uint32_t(1) << a.n_up_src) - 1 : ~uint32_t(0));
  for (int i = 0; i < a.n_sites; ++i) t.coef[i] = a.coef[i], t.half[i] = a.coef[i] * 0.5;
  t.real_coef = spin_site_real_coef(a) ? 1 : 0;
  for (int i = 0; a.coef_im && i < a.n_sites; ++i) t.coef_im[i] = a.coef_im[i], t.half_im[i] = a.coef_im[i] * 0.5;
}

// The definition, evaluated: x has spin_site_rows(source) entries, y spin_site_rows(destination); norm2 may be NULL.  y may be x
// for Z only.  Ranks and unranks through spin_sector_rank / spin_sector_unrank, not through the row walk of spin_rows.hpp.
inline void spin_site_apply_host(const SpinSiteArgs& a, const double* x, double* y, double* norm2) {
  const bool sector = a.n_up_src != -1;
  const int64_t n = spin_site_rows(a.n_sites, a.n_up_dst);
  SpinSectorTables src;
  if (sector && a.kind != kSpinSiteZ) spin_sector_build_tables(a.n_sites, a.n_up_src, src);
  double nrm = 0.0;
  for (int64_t r = 0; r < n; ++r) {
    const uint32_t s = sector ? spin_sector_unrank(a.n_sites, a.n_up_dst, r) : (uint32_t)r;
    double yr = 0.0;
    if (a.kind == kSpinSiteZ) {
      double w = 0.0;
      for (int i = 0; i < a.n_sites; ++i) {
        const double k = a.coef[i] * 0.5;
        w += ((s >> i) & 1u) ? k : -k;
      }
      yr = w * x[r];
    } else {
      for (int i = 0; i < a.n_sites; ++i) {
        const bool up = ((s >> i) & 1u) != 0;
        if (up != (a.kind == kSpinSitePlus)) continue;
        const uint32_t s2 = s ^ (uint32_t(1) << i);
        yr = std::fma(a.coef[i], x[sector ? (int64_t)spin_sector_rank(src, s2) : (int64_t)s2], yr);
      }
    }
    y[r] = yr;
    nrm = std::fma(yr, yr, nrm);
  }
  if (norm2) *norm2 = nrm;
}

// The definition of a complex vector, evaluated: x and y interleaved (re, im), a.coef_im the imaginary coefficients or NULL.
// Ranks and unranks as spin_site_apply_host does.
inline void spin_site_apply_host_z(const SpinSiteArgs& a, const double* x, double* y, double* norm2) {
  const bool sector = a.n_up_src != -1, real_coef = spin_site_real_coef(a);
  const int64_t n = spin_site_rows(a.n_sites, a.n_up_dst);
  SpinSectorTables src;
  if (sector && a.kind != kSpinSiteZ) spin_sector_build_tables(a.n_sites, a.n_up_src, src);
  double nrm = 0.0;
  for (int64_t r = 0; r < n; ++r) {
    const uint32_t s = sector ? spin_sector_unrank(a.n_sites, a.n_up_dst, r) : (uint32_t)r;
    double yre = 0.0, yim = 0.0;
    if (a.kind == kSpinSiteZ) {
      double wr = 0.0, wi = 0.0;
      for (int i = 0; i < a.n_sites; ++i) {
        const double k = a.coef[i] * 0.5;
        wr += ((s >> i) & 1u) ? k : -k;
      }
      for (int i = 0; !real_coef && i < a.n_sites; ++i) {
        const double k = a.coef_im[i] * 0.5;
        wi += ((s >> i) & 1u) ? k : -k;
      }
      const double xre = x[2 * r], xim = x[2 * r + 1];
      yre = real_coef ? wr * xre : std::fma(-wi, xim, wr * xre);
      yim = real_coef ? wr * xim : std::fma(wi, xre, wr * xim);
    } else {
      for (int i = 0; i < a.n_sites; ++i) {
        const bool up = ((s >> i) & 1u) != 0;
        if (up != (a.kind == kSpinSitePlus)) continue;
        const uint32_t s2 = s ^ (uint32_t(1) << i);
        const int64_t q = sector ? (int64_t)spin_sector_rank(src, s2) : (int64_t)s2;
        const double xre = x[2 * q], xim = x[2 * q + 1];
        yre = std::fma(a.coef[i], xre, yre);
        if (!real_coef) yre = std::fma(-a.coef_im[i], xim, yre);
        yim = std::fma(a.coef[i], xim, yim);
        if (!real_coef) yim = std::fma(a.coef_im[i], xre, yim);
      }
    }
    y[2 * r] = yre, y[2 * r + 1] = yim;
    nrm = std::fma(yim, yim, std::fma(yre, yre, nrm));
  }
  if (norm2) *norm2 = nrm;
}

}  // namespace eigenex
