// What the three spin sanitizer programs (spin_model_sanitize.cpp, spin_sector_sanitize.cpp, spin_measure_sanitize.cpp) share:
// the failure counter, and the accessors with which they drive csrc/spin_rows.hpp -- the kernels' own row walk -- so that every
// load it makes is checked against its array (std::vector::at: a load outside throws, and the program dies).
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "spin_rows.hpp"

static int fails = 0;
#define EXPECT(c)                                                        \
  do {                                                                   \
    if (!(c)) {                                                          \
      std::fprintf(stderr, "FAILED %s:%d %s\n", __FILE__, __LINE__, #c); \
      ++fails;                                                           \
    }                                                                    \
  } while (0)

static inline bool same_bits(const std::vector<double>& a, const std::vector<double>& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), sizeof(double) * a.size()) == 0);
}

struct CheckedBinomials {  // SpinSectorView::binom, flattened as the kernels stage it
  std::vector<std::uint32_t> c;
  explicit CheckedBinomials(const eigenex::SpinSectorView& v) : c(&v.binom[0][0], &v.binom[0][0] + eigenex::kSectorMaxSites * (eigenex::kSectorMaxSites + 1)) {}
  std::uint32_t operator()(int i) const {
    const int cols = eigenex::kSectorMaxSites + 1;
    EXPECT(i >= 0 && i / cols < eigenex::kSectorMaxSites);  // p * cols + k: never before the table (k < 0 at p = 0) nor behind it
    return c.at(static_cast<std::size_t>(i));
  }
};

struct CheckedTables {  // default-constructed tables are empty: the full space must not look at them
  const eigenex::SpinSectorTables* t;
  std::uint32_t hi(std::uint32_t i) const { return t->hi_base.at(i); }
  std::uint32_t lo(std::uint32_t i) const { return t->lo_rank.at(i); }
};

struct CheckedVector {
  const std::vector<double>* x;
  double operator()(std::uint32_t i) const { return x->at(i); }
};

// between spin_flip_targets and the loads of x, on row r: a lane without the term reads its own element, a padding mask never flips
static inline void expect_targets(const std::uint32_t* mask, const bool* on, const std::uint32_t* base, const std::uint32_t* low, std::int64_t r) {
  for (int t = 0; t < eigenex::kSpinBatch; ++t) {
    if (!on[t]) EXPECT(base[t] + low[t] == static_cast<std::uint32_t>(r));
    if (mask[t] == 0) EXPECT(!on[t]);
  }
}

// The row sum of k_spin_spmv<SECTOR, E> (kernels.hip) on row r, whose state is s, before the shift, from the kernel's tables by
// the kernel's own functions, every load checked; xs(i) is element i of the vector, a double or a SpinZ.  The full space passes
// empty tables, h = 0 and lo_mask = 0.
template <bool SECTOR, class E, class Vector>
static E checked_operator_row_of(const eigenex::SpinOperatorView& m, const eigenex::SpinSectorTables& t, int h, std::uint32_t lo_mask, const Vector& xs,
                                 std::int64_t r, std::uint32_t s, double scale) {
  const CheckedTables tab{&t};
  const double d = eigenex::spin_row_diagonal(m.dmask, m.dval, m.ndiag, s);
  const E xr = eigenex::spin_scaled(xs(static_cast<std::uint32_t>(r)), scale);
  E yr = eigenex::spin_add_product(E{}, d, xr);
  for (int t0 = 0; t0 < m.nflip; t0 += eigenex::kSpinBatch) {
    EXPECT(t0 + eigenex::kSpinBatch <= eigenex::kSpinMaxTerms);
    bool on[eigenex::kSpinBatch];
    std::uint32_t base[eigenex::kSpinBatch], low[eigenex::kSpinBatch];
    E xv[eigenex::kSpinBatch];
    eigenex::spin_flip_targets<SECTOR>(m.fmask + t0, s, tab, h, lo_mask, on, base, low);
    expect_targets(m.fmask + t0, on, base, low, r);
    eigenex::spin_gather(xs, base, low, xv);
    yr = eigenex::spin_add_flips(yr, m.fval + t0, on, xv, scale);
  }
  return yr;
}

// ... of a real vector
template <bool SECTOR>
static double checked_operator_row(const eigenex::SpinOperatorView& m, const eigenex::SpinSectorTables& t, int h, std::uint32_t lo_mask,
                                   const std::vector<double>& x, std::int64_t r, std::uint32_t s, double scale) {
  return checked_operator_row_of<SECTOR, double>(m, t, h, lo_mask, CheckedVector{&x}, r, s, scale);
}
