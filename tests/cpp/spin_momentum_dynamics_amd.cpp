// C++11 user program: Szz(q, w) of the ground state of the periodic spin-1/2 Heisenberg ring of L sites (default 12) at half
// filling, found at k = 0 through device::spinHalfMomentumOperator (device::spinHalfMomentum64Operator beyond 32 sites) and
// LanczosEigenSolver<double>, by SpinMomentumDynamicsSolver::computeStructureFactorZ(qIndex) at qIndex = L / 2 (the real run) and
// qIndex = 1 (the complex run), beside SpinMomentumCorrelationSolver's static structure factor of the same state.  Prints one JSON
// line, which tests/test_gpu_spin_momentum_site.py reads and checks against a dense diagonalisation, then an OK line.
// usage: spin_momentum_dynamics_amd [L [steps]]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "cmpt/eigen_ex/lanczos.hpp"
#include "cmpt/eigen_ex/spin_correlations.hpp"
#include "cmpt/eigen_ex/spin_momentum_dynamics.hpp"
#include "cmpt/eigen_ex/spin_operator.hpp"

using namespace cmpt::EigenEx;

int main(int argc, char** argv) {
  const int L = argc > 1 ? std::atoi(argv[1]) : 12;
  const int steps = argc > 2 ? std::atoi(argv[2]) : 100;
  const int nUp = L / 2;
  try {
    const SpinHalfModel model = SpinHalfModel::chain(L, 1.0, 1.0, true);
    std::shared_ptr<device::Context> ctx = std::make_shared<device::Context>(0);
    std::shared_ptr<device::CsrOperator> op = L <= 32 ? device::spinHalfMomentumOperator(ctx, model, nUp, 0) : device::spinHalfMomentum64Operator(ctx, model, nUp, 0);
    const Index n = static_cast<Index>(op->rows());
    std::mt19937 random_engine(1);
    LanczosEigenSolver<double> es;
    es.setDeviceOperator(op);
    es.setTolerance(1.0e-13);
    es.setMinIterations(std::min<Index>(n, 200));  // the whole Krylov space of a small sector: the vector, not only the level, is converged
    es.setMaxIterations(400);
    es.setIndicesForConvergence({0});
    es.setInitialVector(es.lanczosBase().makeRandomVector(random_engine, n));
    es.setMaxEigenvalues(1);
    es.compute();
    DenseVector<double> x(n);
    for (Index r = 0; r < n; ++r) x[r] = es.eigenvectors()(r, 0);
    const double e0 = es.eigenvalues()[0];

    SpinMomentumCorrelationSolver cs;
    cs.setDeviceOperator(op).setState(x);
    cs.compute();
    if (cs.info() != Success) throw LanczosException("SpinMomentumCorrelationSolver::compute failed: " + cs.log().back());

    SpinMomentumDynamicsSolver ds;
    ds.setModel(ctx, model, nUp, 0).setState(x).setStateEnergy(e0).setLanczosSteps(steps);
    std::string out = "{\"sites\": " + std::to_string(L) + ", \"dim\": " + std::to_string(static_cast<long>(n));
    char buf[512];
    std::snprintf(buf, sizeof buf, ", \"energy\": %.17g", e0);
    out += buf;
    bool ok = true;
    const int qs[2] = {L / 2, 1};
    for (int k = 0; k < 2; ++k) {
      const int q = qs[k];
      const Index poles = ds.computeStructureFactorZ(q);
      if (ds.info() != Success) throw LanczosException("computeStructureFactorZ failed: " + ds.log().back());
      const double stat = cs.structureFactorZ(6.283185307179586476925286766559 * q / L);
      std::snprintf(buf, sizeof buf,
                    ", \"q%d\": {\"poles\": %ld, \"complex\": %d, \"dst_momentum\": %d, \"dst_dim\": %ld, \"total\": %.17g, \"static\": %.17g, "
                    "\"m0\": %.17g, \"m1\": %.17g, \"m2\": %.17g, \"m3\": %.17g, \"spectrum_1\": %.17g, \"lowest_pole\": %.17g}",
                    k, static_cast<long>(poles), ds.complexRun() ? 1 : 0, ds.destinationMomentum(), static_cast<long>(ds.destinationDimension()), ds.totalWeight(),
                    stat, ds.moment(0), ds.moment(1), ds.moment(2), ds.moment(3), ds.spectrum(1.0, 0.1), poles > 0 ? ds.poles()[0] : 0.0);
      out += buf;
      ok = ok && poles > 0 && ds.complexRun() == (k == 1) && ds.destinationMomentum() == (L - q) % L && 
           std::fabs(ds.totalWeight() - stat) <= static_cast<double>(n) * 2.220446049250313e-16 * (ds.totalWeight() + L / 4.0);  // the sum-rule bound
    }
    // what is refused
    ds.setSiteOperator(EIGENEX_SPIN_SITE_Z, std::vector<std::complex<double> >(1, 1.0), L);
    ds.compute();
    ok = ok && ds.info() == InvalidInput;
    std::printf("%s}\n", out.c_str());
    std::printf(ok ? "SPIN MOMENTUM DYNAMICS OK\n" : "SPIN MOMENTUM DYNAMICS FAILED\n");
    return ok ? 0 : 1;
  } catch (const std::exception& e) {
    std::printf("{\"error\": \"%s\"}\n", e.what());
    return 1;
  }
}
