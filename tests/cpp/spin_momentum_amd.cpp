// C++11 user program: the lowest level of every momentum sector of the periodic spin-1/2 Heisenberg ring (L sites, default 12) in
// the sector of n_up sites up (default L/2), through device::spinHalfMomentumOperator: LanczosEigenSolver<double> at the real
// momenta (0 and L/2) and LanczosEigenSolver<std::complex<double>> at the others.  At k = 0 the stored CSR of the same sector
// (SpinHalfModel::toMomentumCsr, real there) is solved too.  Prints JSON: the dimension and the level of every momentum, the k = 0
// level from the CSR, and the first representative.  tests/test_gpu_spin_momentum.py reads it.
// usage: spin_momentum_amd [L [n_up]]
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "cmpt/eigen_ex/lanczos.hpp"
#include "cmpt/eigen_ex/spin_operator.hpp"

using namespace cmpt::EigenEx;

template <class Scalar>
static double lowest(std::shared_ptr<device::CsrOperator> op, Index n) {
  std::mt19937 random_engine(1);
  LanczosEigenSolver<Scalar> es;
  es.setDeviceOperator(op);
  es.setTolerance(1.0e-13);
  es.setMaxIterations(400);
  es.setIndicesForConvergence({0});
  es.setInitialVector(es.lanczosBase().makeRandomVector(random_engine, n));
  es.setMaxEigenvalues(1);
  es.compute();
  return es.eigenvalues()[0];
}

int main(int argc, char** argv) {
  const int L = argc > 1 ? std::atoi(argv[1]) : 12;
  const int nUp = argc > 2 ? std::atoi(argv[2]) : L / 2;
  try {
    const SpinHalfModel model = SpinHalfModel::chain(L, 1.0, 1.0, true);
    const bool invariant = model.translationInvariant(1), open_is = SpinHalfModel::chain(L, 1.0, 1.0, false).translationInvariant(1);
    std::shared_ptr<device::Context> ctx = std::make_shared<device::Context>(0);
    std::string dims, levels;
    for (int m = 0; m < L; ++m) {
      const Index n = model.momentumDimension(nUp, 1, m);
      const bool real = m == 0 || 2 * m == L;
      const double e = real ? lowest<double>(device::spinHalfMomentumOperator(ctx, model, nUp, m), n)
                            : lowest<std::complex<double> >(device::spinHalfMomentumOperator(ctx, model, nUp, m, 1, true), n);
      char buf[64];
      std::snprintf(buf, sizeof buf, "%s%ld", m ? ", " : "", static_cast<long>(n));
      dims += buf;
      std::snprintf(buf, sizeof buf, "%s%.17g", m ? ", " : "", e);
      levels += buf;
    }
    bool refused = false;  // a complex momentum with real states
    try {
      device::spinHalfMomentumOperator(ctx, model, nUp, 1);
    } catch (const std::exception&) {
      refused = true;
    }
    const HostCsr<std::complex<double> > csr = model.toMomentumCsr(nUp, 1, 0);
    std::vector<double> re(csr.val.size());
    double imag = 0.0;
    for (std::size_t p = 0; p < csr.val.size(); ++p) re[p] = csr.val[p].real(), imag += std::fabs(csr.val[p].imag());
    const double e_csr = lowest<double>(std::make_shared<device::CsrOperator>(ctx, csr.n, 0, csr.n, csr.rowptr.data(), csr.col.data(), re.data()), csr.n);
    std::vector<std::uint8_t> periods;
    const std::vector<std::uint32_t> states = model.momentumStates(nUp, 1, 0, &periods);
    std::printf("{\"sites\": %d, \"n_up\": %d, \"invariant\": %d, \"open_chain_invariant\": %d, \"dims\": [%s], \"levels\": [%s], \"energy_csr_k0\": %.17g, "
                "\"imag_k0\": %.3g, \"first_state\": %lu, \"first_period\": %d, \"real_upload_of_complex_momentum_refused\": %d}\n",
                L, nUp, invariant ? 1 : 0, open_is ? 1 : 0, dims.c_str(), levels.c_str(), e_csr, imag, static_cast<unsigned long>(states.front()),
                static_cast<int>(periods.front()), refused ? 1 : 0);
  } catch (const std::exception& e) {
    std::printf("{\"error\": \"%s\"}\n", e.what());
    return 1;
  }
  return 0;
}
