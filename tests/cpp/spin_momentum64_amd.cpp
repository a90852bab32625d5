// C++11 user program: the ground state at k = 0 of the periodic spin-1/2 Heisenberg ring of L sites (default 36) with n_up sites up
// (default 3) through device::spinHalfMomentum64Operator and LanczosEigenSolver<double>, the same level from the stored CSR
// (SpinHalfModel::toMomentum64Csr), and the state's diagonal correlations in the momentum basis (SpinMomentumCorrelationSolver, on
// the real state and on its complex copy).  Prints one JSON line, which tests/test_gpu_spin_momentum64.py reads, then an OK line.
// usage: spin_momentum64_amd [L [n_up]]
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "cmpt/eigen_ex/lanczos.hpp"
#include "cmpt/eigen_ex/spin_correlations.hpp"
#include "cmpt/eigen_ex/spin_operator.hpp"

using namespace cmpt::EigenEx;

static double lowest(std::shared_ptr<device::CsrOperator> op, Index n, DenseVector<double>* vector) {
  std::mt19937 random_engine(1);
  LanczosEigenSolver<double> es;
  es.setDeviceOperator(op);
  es.setTolerance(1.0e-13);
  es.setMaxIterations(400);
  es.setIndicesForConvergence({0});
  es.setInitialVector(es.lanczosBase().makeRandomVector(random_engine, n));
  es.setMaxEigenvalues(1);
  es.compute();
  if (vector) {
    *vector = DenseVector<double>(n);
    for (Index r = 0; r < n; ++r) (*vector)[r] = es.eigenvectors()(r, 0);
  }
  return es.eigenvalues()[0];
}

int main(int argc, char** argv) {
  const int L = argc > 1 ? std::atoi(argv[1]) : 36;
  const int nUp = argc > 2 ? std::atoi(argv[2]) : 3;
  try {
    const SpinHalfModel model = SpinHalfModel::chain(L, 1.0, 1.0, true);
    std::shared_ptr<device::Context> ctx = std::make_shared<device::Context>(0);
    const Index n = model.momentum64Dimension(nUp, 1, 0);
    std::vector<std::uint8_t> periods;
    const std::vector<std::uint64_t> states = model.momentum64States(nUp, 1, 0, &periods);
    std::shared_ptr<device::CsrOperator> op = device::spinHalfMomentum64Operator(ctx, model, nUp, 0);
    int layout = -1;
    device::check(eigenex_csr_layout(op->handle(), &layout), "eigenex_csr_layout");
    DenseVector<double> x;
    const double e = lowest(op, n, &x);
    const HostCsr<std::complex<double> > csr = model.toMomentum64Csr(nUp, 1, 0);
    std::vector<double> re(csr.val.size());
    for (std::size_t p = 0; p < csr.val.size(); ++p) re[p] = csr.val[p].real();
    const double e_csr = lowest(std::make_shared<device::CsrOperator>(ctx, csr.n, 0, csr.n, csr.rowptr.data(), csr.col.data(), re.data()), csr.n, nullptr);

    SpinMomentumCorrelationSolver cs;
    cs.setDeviceOperator(op).setState(x);
    cs.compute();
    if (cs.info() != Success) throw LanczosException("SpinMomentumCorrelationSolver::compute failed: " + cs.log().back());
    double row = 0.0, spread = 0.0;
    for (int j = 0; j < L; ++j) row += cs.szsz(0, j);
    for (int i = 0; i < L; ++i) spread = std::fmax(spread, std::fabs(cs.magnetisation()[i] - cs.magnetisation()[0]));
    const std::uint64_t all = ~std::uint64_t(0) >> (64 - L);
    const double string_all = cs.stringCorrelator(all);
    // the same state as a complex vector on the complex handle: the same numbers
    DenseVector<std::complex<double> > xz(n);
    for (Index r = 0; r < n; ++r) xz[r] = std::complex<double>(x[r], 0.0);
    SpinMomentumCorrelationSolver cz;
    cz.setDeviceOperator(device::spinHalfMomentum64Operator(ctx, model, nUp, 0, 1, true)).setState(xz);
    cz.compute();
    double differ = 0.0;
    for (int i = 0; i < L; ++i)
      for (int j = 0; j < L; ++j) differ = std::fmax(differ, std::fabs(cz.szsz(i, j) - cs.szsz(i, j)));

    bool expand_refused = false, too_large_refused = false;
    {
      detail::KrylovDevice dev;
      dev.create(ctx, op, n, 1, 0, false);
      expand_refused = eigenex_spin_momentum_expand(dev.handle(), EIGENEX_VEC_COL(0), dev.handle(), EIGENEX_VEC_COL(0), nullptr) == EIGENEX_ERR_STATE;
    }
    try {
      SpinHalfModel::chain(49, 1.0, 1.0, true).momentum64Dimension(3, 1, 0);
    } catch (const std::exception&) {
      too_large_refused = true;
    }
    std::printf("{\"sites\": %d, \"n_up\": %d, \"dim\": %ld, \"first_state\": %llu, \"first_period\": %d, \"layout\": %d, \"energy\": %.17g, \"energy_csr\": %.17g, "
                "\"magnetisation_0\": %.17g, \"magnetisation_spread\": %.3g, \"zz_00\": %.17g, \"zz_01\": %.17g, \"zz_row_sum\": %.17g, "
                "\"structure_factor_0\": %.17g, \"structure_factor_pi\": %.17g, \"string_all_sites\": %.17g, \"complex_differs\": %.3g, "
                "\"expand_refused\": %d, \"sites_49_refused\": %d}\n",
                L, nUp, static_cast<long>(n), static_cast<unsigned long long>(states.front()), static_cast<int>(periods.front()), layout, e, e_csr,
                cs.magnetisation()[0], spread, cs.szsz(0, 0), cs.szsz(0, 1), row, cs.structureFactorZ(0.0), cs.structureFactorZ(3.14159265358979323846),
                string_all, differ, expand_refused ? 1 : 0, too_large_refused ? 1 : 0);
    const bool ok = spread <= 1e-13 && differ <= 1e-13 && expand_refused && too_large_refused && std::fabs(e - e_csr) <= 1e-10 * std::fabs(e);
    std::printf(ok ? "SPIN MOMENTUM64 OK\n" : "SPIN MOMENTUM64 FAILED\n");
    return ok ? 0 : 1;
  } catch (const std::exception& e) {
    std::printf("{\"error\": \"%s\"}\n", e.what());
    return 1;
  }
}
