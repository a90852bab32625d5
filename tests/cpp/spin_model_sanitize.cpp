// Host code of the spin-1/2 operator under AddressSanitizer + UBSan (device code cannot be sanitised on the GPU pool):
// csrc/spin_model.hpp -- argument checks, the CSR rows, the tables of the matrix-free kernel -- compiled into this
// program, and SpinHalfModel of spin_operator.hpp on top of the library's eigenex_spin_csr.  For open, periodic, random
// (zero couplings, a repeated pair), field and Ising-only models at L = 2..10: the rows go into exactly-sized arrays, the
// count-only call agrees with the full one, a row window equals its slice, the row sum of k_spin_spmv<false> -- the kernel's own
// functions (csrc/spin_rows.hpp) run on its tables -- equals the CSR row loop bit for bit, and every load they make stays inside
// the vector.
// Built and run by tests/test_spin_host.py; prints SPIN MODEL OK and exits 0 when every check holds.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "cmpt/eigen_ex/spin_operator.hpp"
#include "spin_model.hpp"
#include "spin_rows_checked.hpp"

using namespace cmpt::EigenEx;

struct Rows {
  std::vector<std::int64_t> rowptr;
  std::vector<std::int32_t> col;
  std::vector<double> val;
};

static eigenex::SpinModelArgs args_of(const SpinHalfModel& m) {
  return eigenex::SpinModelArgs{m.sites(), m.bonds(), m.siteI(), m.siteJ(), m.jz(), m.jxy(), m.fieldZ(), m.fieldX()};
}

static Rows rows_of(const SpinHalfModel& m, std::int64_t rb, std::int64_t nr) {
  const eigenex::SpinModelArgs a = args_of(m);
  Rows r;
  r.rowptr.assign(static_cast<std::size_t>(nr) + 1, -1);
  std::int64_t nnz = -1, nnz2 = -1;
  eigenex::spin_write_rows(a, rb, nr, r.rowptr.data(), nullptr, nullptr, &nnz);
  const std::vector<std::int64_t> counted = r.rowptr;
  r.col.assign(static_cast<std::size_t>(nnz), -1);  // exactly sized: one entry too many is a heap overflow
  r.val.assign(static_cast<std::size_t>(nnz), 0.0);
  eigenex::spin_write_rows(a, rb, nr, r.rowptr.data(), r.col.data(), r.val.data(), &nnz2);
  EXPECT(nnz == nnz2 && counted == r.rowptr && r.rowptr[0] == 0 && r.rowptr.back() == nnz);
  return r;
}

static void check_model(const SpinHalfModel& m, std::mt19937& rng) {
  const eigenex::SpinModelArgs a = args_of(m);
  EXPECT(eigenex::spin_model_error(a) == nullptr);
  const std::int64_t n = m.rows();
  const Rows full = rows_of(m, 0, n);
  // SpinHalfModel::toCsr (the library's eigenex_spin_csr) gives the same arrays
  const HostCsr<double> lib = m.toCsr();
  EXPECT(lib.n == n && lib.col == full.col && same_bits(lib.val, full.val));
  EXPECT(lib.rowptr.size() == full.rowptr.size());
  for (std::size_t i = 0; i < lib.rowptr.size() && i < full.rowptr.size(); ++i) EXPECT(lib.rowptr[i] == full.rowptr[i]);
  // windows
  const std::int64_t windows[4][2] = {{0, 1}, {n / 3, n - n / 3}, {n - 1, 1}, {n, 0}};
  for (const auto& w : windows) {
    const Rows part = rows_of(m, w[0], w[1]);
    const std::int64_t p0 = full.rowptr[static_cast<std::size_t>(w[0])];
    for (std::int64_t k = 0; k <= w[1]; ++k) EXPECT(part.rowptr[static_cast<std::size_t>(k)] == full.rowptr[static_cast<std::size_t>(w[0] + k)] - p0);
    EXPECT(std::equal(part.col.begin(), part.col.end(), full.col.begin() + p0));
    EXPECT(part.val.empty() || std::memcmp(part.val.data(), full.val.data() + p0, sizeof(double) * part.val.size()) == 0);
  }
  // the kernel's tables against the CSR row loop
  eigenex::SpinOperatorView v;
  eigenex::spin_build_view(a, v);
  EXPECT(v.n_sites == m.sites() && v.ndiag <= eigenex::kSpinMaxBonds + eigenex::kSpinMaxSites && v.nflip <= eigenex::kSpinMaxBonds + eigenex::kSpinMaxSites);
  for (int t = v.nflip; t < eigenex::kSpinMaxTerms; ++t) EXPECT(v.fmask[t] == 0 && v.fval[t] == 0.0);
  std::vector<double> x(static_cast<std::size_t>(n));
  std::uniform_real_distribution<double> u(-1.0, 1.0);
  for (auto& e : x) e = u(rng);
  const double scale = 0.73;
  for (std::int64_t s = 0; s < n; ++s) {
    double sum = 0.0;
    for (std::int64_t p = full.rowptr[static_cast<std::size_t>(s)]; p < full.rowptr[static_cast<std::size_t>(s) + 1]; ++p) {
      const std::int32_t c = full.col[static_cast<std::size_t>(p)];
      EXPECT(c >= 0 && c < n);
      sum = sum + full.val[static_cast<std::size_t>(p)] * (x[static_cast<std::size_t>(c)] * scale);
    }
    const double k = checked_operator_row<false>(v, eigenex::SpinSectorTables(), 0, 0u, x, s, static_cast<std::uint32_t>(s), scale);
    EXPECT(std::memcmp(&k, &sum, sizeof(double)) == 0);
  }
}

int main() {
  std::mt19937 rng(5);
  std::uniform_real_distribution<double> u(-1.5, 1.5);
  for (int L = 2; L <= 10; ++L) {
    check_model(SpinHalfModel::chain(L, 1.0, 1.0, false), rng);
    check_model(SpinHalfModel::chain(L, 1.0, 0.7, true), rng);
    SpinHalfModel r(L), f = SpinHalfModel::chain(L, 0.8, 1.1, false), ising(L);
    for (int b = 0; b < 40; ++b) {
      const int i = static_cast<int>(rng() % L), j = (i + 1 + static_cast<int>(rng() % (L - 1))) % L;
      r.addBond(i, j, b % 5 == 4 ? 0.0 : u(rng), b % 3 == 2 ? 0.0 : u(rng));
      if (b == 0) r.addBond(j, i, u(rng), u(rng));  // the same pair again
      if (b < 12) ising.addBond(i, j, u(rng), 0.0);
    }
    check_model(r, rng);
    for (int i = 0; i < L; ++i) {
      f.setFieldZ(i, u(rng));
      if (i % 2 == 0) f.setFieldX(i, u(rng));
      r.setFieldZ(i, u(rng)).setFieldX(i, u(rng));
      ising.setFieldZ(i, u(rng));
    }
    check_model(f, rng);
    check_model(r, rng);
    check_model(ising, rng);
    EXPECT(ising.toCsr().col.size() == static_cast<std::size_t>(ising.rows()));
  }
  {  // the largest tables: 64 bonds and both fields on 30 sites fit, with room for the last batch
    SpinHalfModel big(30);
    for (int b = 0; b < 64; ++b) big.addBond(b % 30, (b + 1 + b / 30) % 30, 1.0, 1.0);
    for (int i = 0; i < 30; ++i) big.setFieldZ(i, 0.5).setFieldX(i, 0.25);
    const eigenex::SpinModelArgs a = args_of(big);
    EXPECT(eigenex::spin_model_error(a) == nullptr);
    eigenex::SpinOperatorView v;
    eigenex::spin_build_view(a, v);
    EXPECT(v.ndiag == 94 && v.nflip == 94 && (v.nflip + eigenex::kSpinBatch - 1) / eigenex::kSpinBatch * eigenex::kSpinBatch <= eigenex::kSpinMaxTerms);
    const Rows top = rows_of(big, (std::int64_t(1) << 30) - 3, 3);  // rows next to 2^30: columns stay below it
    for (std::int32_t c : top.col) EXPECT(c >= 0 && c < (std::int32_t(1) << 30));
  }
  // argument errors: a message, nothing written
  {
    const std::int32_t si[2] = {0, 2}, sj[2] = {1, 2}, far[1] = {7};
    const double one[2] = {1.0, 1.0}, bad[1] = {std::numeric_limits<double>::quiet_NaN()};
    EXPECT(eigenex::spin_model_error(eigenex::SpinModelArgs{1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}) != nullptr);
    EXPECT(eigenex::spin_model_error(eigenex::SpinModelArgs{31, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}) != nullptr);
    EXPECT(eigenex::spin_model_error(eigenex::SpinModelArgs{4, 65, si, sj, one, one, nullptr, nullptr}) != nullptr);
    EXPECT(eigenex::spin_model_error(eigenex::SpinModelArgs{4, -1, si, sj, one, one, nullptr, nullptr}) != nullptr);
    EXPECT(eigenex::spin_model_error(eigenex::SpinModelArgs{4, 2, si, sj, one, one, nullptr, nullptr}) != nullptr);   // bond 1 joins 2 to 2
    EXPECT(eigenex::spin_model_error(eigenex::SpinModelArgs{4, 1, si, far, one, one, nullptr, nullptr}) != nullptr);  // site 7 of 4
    EXPECT(eigenex::spin_model_error(eigenex::SpinModelArgs{4, 1, si, sj, bad, one, nullptr, nullptr}) != nullptr);
    EXPECT(eigenex::spin_model_error(eigenex::SpinModelArgs{4, 1, si, sj, one, one, nullptr, nullptr}) == nullptr);
    EXPECT(eigenex::spin_model_error(eigenex::SpinModelArgs{4, 1, nullptr, sj, one, one, nullptr, nullptr}) != nullptr);
    bool threw = false;
    try {
      SpinHalfModel(4).addBond(1, 1, 1.0, 1.0).toCsr();
    } catch (const LanczosException&) {
      threw = true;
    }
    EXPECT(threw);
    threw = false;
    try {
      SpinHalfModel(4).setFieldX(4, 1.0);
    } catch (const LanczosException&) {
      threw = true;
    }
    EXPECT(threw);
  }
  if (fails) return 1;
  std::printf("SPIN MODEL OK\n");
  return 0;
}
