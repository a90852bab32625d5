// Host code of the fixed-magnetisation spin-1/2 operator under AddressSanitizer + UBSan (device code cannot be sanitised on
// the GPU pool): csrc/spin_sector.hpp -- argument checks, binomials, unrank, the two rank tables, the sector rows, the
// kernel's view -- compiled into this program, and the sector calls of SpinHalfModel (spin_operator.hpp) on top of the
// library.  For every (L, n_up) with L <= 12: dim, unrank and rank against enumeration.  For chains, random and field models in
// those sectors and in the few-spin sectors of 31 and 32 sites: the rows go into exactly-sized arrays, the count-only call
// agrees with the full one, a row window equals its slice, the rows equal the full-space rows at the sector's states with ranked
// columns, and the row sum of k_spin_spmv<true> -- the kernel's own functions (csrc/spin_rows.hpp) run on its tables, every
// load checked against its array -- equals the CSR row loop bit for bit.
// Built and run by tests/test_spin_sector_host.py; prints SPIN SECTOR OK and exits 0 when every check holds.
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "cmpt/eigen_ex/spin_operator.hpp"
#include "spin_rows_checked.hpp"
#include "spin_sector.hpp"

using namespace cmpt::EigenEx;

struct Rows {
  std::vector<std::int64_t> rowptr;
  std::vector<std::int32_t> col;
  std::vector<double> val;
};

static eigenex::SpinModelArgs args_of(const SpinHalfModel& m) {
  return eigenex::SpinModelArgs{m.sites(), m.bonds(), m.siteI(), m.siteJ(), m.jz(), m.jxy(), m.fieldZ(), m.fieldX()};
}

static int popcount(std::uint32_t x) {
  int c = 0;
  for (; x; x &= x - 1) ++c;
  return c;
}

static Rows rows_of(const SpinHalfModel& m, const eigenex::SpinSectorTables& t, std::int64_t rb, std::int64_t nr) {
  const eigenex::SpinModelArgs a = args_of(m);
  Rows r;
  r.rowptr.assign(static_cast<std::size_t>(nr) + 1, -1);
  std::int64_t nnz = -1, nnz2 = -1;
  eigenex::spin_sector_write_rows(a, t, rb, nr, r.rowptr.data(), nullptr, nullptr, &nnz);
  const std::vector<std::int64_t> counted = r.rowptr;
  r.col.assign(static_cast<std::size_t>(nnz), -1);  // exactly sized: one entry too many is a heap overflow
  r.val.assign(static_cast<std::size_t>(nnz), 0.0);
  eigenex::spin_sector_write_rows(a, t, rb, nr, r.rowptr.data(), r.col.data(), r.val.data(), &nnz2);
  EXPECT(nnz == nnz2 && counted == r.rowptr && r.rowptr[0] == 0 && r.rowptr.back() == nnz);
  return r;
}

static void check_sector(const SpinHalfModel& m, int n_up, std::mt19937& rng) {
  const eigenex::SpinModelArgs a = args_of(m);
  EXPECT(eigenex::spin_sector_error(a, n_up) == nullptr);
  const int L = m.sites();
  const std::int64_t n = eigenex::spin_sector_dim(L, n_up);
  EXPECT(n == m.sectorRows(n_up));
  eigenex::SpinSectorTables t;
  eigenex::spin_sector_build_tables(L, n_up, t);
  EXPECT(t.h == (L + 1) / 2 && t.lo_rank.size() == (std::size_t(1) << t.h) && t.hi_base.size() == (std::size_t(1) << (L - t.h)));
  const Rows full = rows_of(m, t, 0, n);
  // the library: SpinHalfModel::toSectorCsr and sectorStates
  const HostCsr<double> lib = m.toSectorCsr(n_up);
  EXPECT(lib.n == n && lib.col == full.col && lib.val.size() == full.val.size() &&
         (full.val.empty() || std::memcmp(lib.val.data(), full.val.data(), sizeof(double) * full.val.size()) == 0));
  EXPECT(lib.rowptr.size() == full.rowptr.size());
  for (std::size_t i = 0; i < lib.rowptr.size() && i < full.rowptr.size(); ++i) EXPECT(lib.rowptr[i] == full.rowptr[i]);
  const std::vector<std::uint32_t> states = m.sectorStates(n_up);
  EXPECT(static_cast<std::int64_t>(states.size()) == n);
  // windows
  const std::int64_t windows[4][2] = {{0, 1}, {n / 3, n - n / 3}, {n - 1, 1}, {n, 0}};
  for (const auto& w : windows) {
    const Rows part = rows_of(m, t, w[0], w[1]);
    const std::int64_t p0 = full.rowptr[static_cast<std::size_t>(w[0])];
    for (std::int64_t k = 0; k <= w[1]; ++k) EXPECT(part.rowptr[static_cast<std::size_t>(k)] == full.rowptr[static_cast<std::size_t>(w[0] + k)] - p0);
    EXPECT(std::equal(part.col.begin(), part.col.end(), full.col.begin() + p0));
    EXPECT(part.val.empty() || std::memcmp(part.val.data(), full.val.data() + p0, sizeof(double) * part.val.size()) == 0);
  }
  // the kernel's tables against the CSR row loop, and the rows against the full-space rows at the same state
  std::unique_ptr<eigenex::SpinSectorView> v(new eigenex::SpinSectorView());
  eigenex::spin_sector_build_view(a, n_up, *v);
  const CheckedBinomials binom(*v);
  EXPECT(v->model.n_sites == L && v->n_up == n_up && v->h == t.h && v->model.ndiag <= eigenex::kSpinMaxTerms && v->model.nflip <= eigenex::kSpinMaxBonds);
  for (int i = v->model.nflip; i < eigenex::kSpinMaxTerms; ++i) EXPECT(v->model.fmask[i] == 0 && v->model.fval[i] == 0.0);
  for (int i = 0; i < v->model.nflip; ++i) EXPECT(popcount(v->model.fmask[i]) == 2);
  std::vector<double> x(static_cast<std::size_t>(n));
  std::uniform_real_distribution<double> u(-1.0, 1.0);
  for (auto& e : x) e = u(rng);
  const double scale = 0.73;
  eigenex::SpinModelArgs z = a;
  z.hx = nullptr;
  for (std::int64_t r = 0; r < n; ++r) {
    double sum = 0.0;
    for (std::int64_t p = full.rowptr[static_cast<std::size_t>(r)]; p < full.rowptr[static_cast<std::size_t>(r) + 1]; ++p) {
      const std::int32_t c = full.col[static_cast<std::size_t>(p)];
      EXPECT(c >= 0 && c < n);
      sum = sum + full.val[static_cast<std::size_t>(p)] * (x[static_cast<std::size_t>(c)] * scale);
    }
    const eigenex::SpinUnranked u = eigenex::spin_unrank_row(binom, L, n_up, static_cast<std::uint32_t>(r));  // the kernel's own unrank
    EXPECT(u.left == 0 && u.k == 0);
    const std::uint32_t s = u.s;
    const double k = checked_operator_row<true>(v->model, t, v->h, v->lo_mask, x, r, s, scale);
    EXPECT(std::memcmp(&k, &sum, sizeof(double)) == 0);
    EXPECT(s == states[static_cast<std::size_t>(r)] && s == eigenex::spin_sector_unrank(L, n_up, r) && popcount(s) == n_up);
    EXPECT(eigenex::spin_sector_rank(t, s) == static_cast<std::uint32_t>(r));
    EXPECT(r == 0 || states[static_cast<std::size_t>(r) - 1] < s);  // ascending
    if (L <= 30) {  // the full-space row of state s: the same entries, columns ranked
      std::int64_t rp[2], cnt = 0;
      eigenex::spin_write_rows(z, s, 1, rp, nullptr, nullptr, &cnt);
      std::vector<std::int32_t> fc(static_cast<std::size_t>(cnt), -1);
      std::vector<double> fv(static_cast<std::size_t>(cnt), 0.0);
      eigenex::spin_write_rows(z, s, 1, rp, fc.data(), fv.data(), &cnt);
      const std::int64_t p0 = full.rowptr[static_cast<std::size_t>(r)];
      EXPECT(cnt == full.rowptr[static_cast<std::size_t>(r) + 1] - p0);
      for (std::int64_t q = 0; q < cnt && p0 + q < static_cast<std::int64_t>(full.col.size()); ++q) {
        EXPECT(static_cast<std::uint32_t>(full.col[static_cast<std::size_t>(p0 + q)]) == eigenex::spin_sector_rank(t, static_cast<std::uint32_t>(fc[static_cast<std::size_t>(q)])));
        EXPECT(std::memcmp(&full.val[static_cast<std::size_t>(p0 + q)], &fv[static_cast<std::size_t>(q)], sizeof(double)) == 0);
      }
    }
  }
}

int main() {
  std::mt19937 rng(7);
  std::uniform_real_distribution<double> u(-1.5, 1.5);
  // dim, unrank and rank against enumeration, every sector up to 12 sites
  for (int L = 2; L <= 12; ++L)
    for (int n_up = 0; n_up <= L; ++n_up) {
      eigenex::SpinSectorTables t;
      eigenex::spin_sector_build_tables(L, n_up, t);
      std::int64_t r = 0;
      for (std::uint32_t s = 0; s < (std::uint32_t(1) << L); ++s)
        if (popcount(s) == n_up) {
          EXPECT(eigenex::spin_sector_unrank(L, n_up, r) == s && eigenex::spin_sector_rank(t, s) == static_cast<std::uint32_t>(r));
          ++r;
        }
      EXPECT(r == eigenex::spin_sector_dim(L, n_up));
    }
  EXPECT(eigenex::spin_sector_dim(32, 16) == 601080390 && eigenex::spin_sector_dim(30, 15) == 155117520 && eigenex::spin_sector_dim(32, 0) == 1);
  EXPECT(eigenex::spin_sector_unrank(32, 16, 601080389) == 0xFFFF0000u && eigenex::spin_sector_unrank(32, 16, 0) == 0x0000FFFFu);
  {  // the largest tables: rank of the last and first state of (32, 16)
    eigenex::SpinSectorTables t;
    eigenex::spin_sector_build_tables(32, 16, t);
    EXPECT(eigenex::spin_sector_rank(t, 0xFFFF0000u) == 601080389u && eigenex::spin_sector_rank(t, 0x0000FFFFu) == 0u);
    std::uniform_int_distribution<std::int64_t> pick(0, 601080389);
    for (int i = 0; i < 2000; ++i) {
      const std::int64_t r = pick(rng);
      EXPECT(eigenex::spin_sector_rank(t, eigenex::spin_sector_unrank(32, 16, r)) == static_cast<std::uint32_t>(r));
    }
  }
  for (int L : {2, 3, 5, 8, 9, 10}) {
    SpinHalfModel open = SpinHalfModel::chain(L, 1.0, 1.0, false), ring = SpinHalfModel::chain(L, 1.0, 0.7, true), r(L), f = SpinHalfModel::chain(L, 0.8, 1.1, false);
    for (int b = 0; b < 40; ++b) {
      const int i = static_cast<int>(rng() % L), j = (i + 1 + static_cast<int>(rng() % (L - 1))) % L;
      r.addBond(i, j, b % 5 == 4 ? 0.0 : u(rng), b % 3 == 2 ? 0.0 : u(rng));
      if (b == 0) r.addBond(j, i, u(rng), u(rng));  // the same pair again
    }
    for (int i = 0; i < L; ++i) f.setFieldZ(i, u(rng)), r.setFieldZ(i, u(rng)).setFieldX(i, 0.0);  // an all-zero transverse field is none
    for (int n_up = 0; n_up <= L; ++n_up) {
      check_sector(open, n_up, rng);
      check_sector(ring, n_up, rng);
      check_sector(r, n_up, rng);
      check_sector(f, n_up, rng);
    }
  }
  // bits 30 and 31: the few-spin sectors of 31 and 32 sites, bonds on the top sites and across the split of the rank tables
  for (int L : {31, 32}) {
    SpinHalfModel m = SpinHalfModel::chain(L, 1.0, 0.7, true);
    m.addBond(0, L - 1, 0.4, -1.3).addBond(L / 2 - 1, L / 2 + 1, 0.3, 0.6).addBond(L - 1, L - 2, 0.0, 0.9);
    for (int b = m.bonds(); b < 64; ++b) m.addBond(b % L, (b * 7 + 3) % L == b % L ? (b + 1) % L : (b * 7 + 3) % L, u(rng), u(rng));
    for (int i = 0; i < L; ++i) m.setFieldZ(i, u(rng));
    for (int n_up : {0, 1, 2, L - 2, L - 1, L}) check_sector(m, n_up, rng);
  }
  // argument errors: a message, nothing written
  {
    const std::int32_t si[1] = {0}, sj[1] = {1};
    const double one[1] = {1.0}, zero4[4] = {0.0, 0.0, 0.0, 0.0}, hx4[4] = {0.0, 0.0, 0.5, 0.0};
    typedef eigenex::SpinModelArgs A;
    EXPECT(eigenex::spin_sector_error(A{4, 1, si, sj, one, one, nullptr, nullptr}, 2) == nullptr);
    EXPECT(eigenex::spin_sector_error(A{4, 1, si, sj, one, one, zero4, zero4}, 2) == nullptr);
    EXPECT(eigenex::spin_sector_error(A{32, 1, si, sj, one, one, nullptr, nullptr}, 32) == nullptr);
    EXPECT(eigenex::spin_model_error(A{32, 1, si, sj, one, one, nullptr, nullptr}) != nullptr);  // the full space stops at 30
    EXPECT(eigenex::spin_sector_error(A{1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, 0) != nullptr);
    EXPECT(eigenex::spin_sector_error(A{33, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, 3) != nullptr);
    EXPECT(eigenex::spin_sector_error(A{4, 1, si, sj, one, one, nullptr, nullptr}, -1) != nullptr);
    EXPECT(eigenex::spin_sector_error(A{4, 1, si, sj, one, one, nullptr, nullptr}, 5) != nullptr);
    const char* why = eigenex::spin_sector_error(A{4, 1, si, sj, one, one, nullptr, hx4}, 2);
    EXPECT(why != nullptr && std::strstr(why, "transverse") != nullptr);
    EXPECT(eigenex::spin_sector_dim(33, 2) == 0 && eigenex::spin_sector_dim(8, 9) == 0 && eigenex::spin_sector_dim(8, -1) == 0);
    bool threw = false;
    try {
      SpinHalfModel(4).addBond(0, 1, 1.0, 1.0).setFieldX(2, 0.5).toSectorCsr(2);
    } catch (const LanczosException&) {
      threw = true;
    }
    EXPECT(threw);
    threw = false;
    try {
      SpinHalfModel(33).sectorRows(3);
    } catch (const LanczosException&) {
      threw = true;
    }
    EXPECT(threw);
  }
  if (fails) return 1;
  std::printf("SPIN SECTOR OK\n");
  return 0;
}
