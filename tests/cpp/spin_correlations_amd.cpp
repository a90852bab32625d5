// C++11 user program: SpinCorrelationSolver on the periodic spin-1/2 Heisenberg ring (L sites, default 12).  The lowest level
// of the sectors nUp = L/2 and L/2 - 1 through LanczosEigenSolver<double> with the matrix-free sector operator, then the
// correlations of each eigenvector in one call.  Prints JSON: per sector the energy, <S^2>, the i = j values, the structure
// factor at q = 0 (which is (nUp - L/2)^2 / L for any state of the sector), sum_i <Sz_i>, the largest difference between the
// nearest-neighbour <S_i.S_j> and E/L; and whether a stored CSR operator, a zero state, a state of the wrong length and no
// operator at all end in InvalidInput with an ERROR line in the log.  tests/test_gpu_spin_measure.py reads it.
// usage: spin_correlations_amd [L]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "cmpt/eigen_ex/lanczos.hpp"
#include "cmpt/eigen_ex/spin_correlations.hpp"

using namespace cmpt::EigenEx;

static bool refused(const SpinCorrelationSolver& sc) {
  bool line = false;
  for (const std::string& l : sc.log()) line = line || l.compare(0, SpinCorrelationSolver::headERROR().size(), SpinCorrelationSolver::headERROR()) == 0;
  return sc.info() == InvalidInput && line;
}

int main(int argc, char** argv) {
  const int L = argc > 1 ? std::atoi(argv[1]) : 12;
  try {
    const SpinHalfModel model = SpinHalfModel::chain(L, 1.0, 1.0, true);
    std::shared_ptr<device::Context> ctx = std::make_shared<device::Context>(0);
    std::printf("{\"sites\": %d, \"sectors\": [", L);
    for (int pass = 0; pass < 2; ++pass) {
      const int nUp = L / 2 - pass;
      const Index n = model.sectorRows(nUp);
      std::shared_ptr<device::CsrOperator> op = device::spinHalfSectorOperator(ctx, model, nUp);
      std::mt19937 random_engine(1);
      LanczosEigenSolver<double> es;
      es.setDeviceOperator(op);
      es.setTolerance(1.0e-13);
      es.setMaxIterations(400);
      es.setComputeEigenvectorsOn(true);
      es.setIndicesForConvergence({0});
      es.setInitialVector(es.lanczosBase().makeRandomVector(random_engine, n));
      es.setMaxEigenvalues(1);
      es.compute();
      const double energy = es.eigenvalues()[0];
      DenseVector<double> x(n);
      for (Index r = 0; r < n; ++r) x[r] = 3.0 * es.eigenvectors().colData(0)[r];  // not normalised: the solver divides by <v|v>
      SpinCorrelationSolver sc;
      sc.setDeviceOperator(op).setState(x);
      sc.compute();
      double sumSz = 0.0, bondSpread = 0.0, diagonal = 0.0;
      for (int i = 0; i < L; ++i) {
        sumSz += sc.sz(i);
        bondSpread = std::fmax(bondSpread, std::fabs(sc.dot(i, (i + 1) % L) - energy / L));
        diagonal = std::fmax(diagonal, std::fabs(sc.szsz(i, i) - 0.25) + std::fabs(sc.sxy(i, i) - 0.5) + std::fabs(sc.dot(i, i) - 0.75) + std::fabs(sc.sx(i)));
      }
      std::printf("%s{\"n_up\": %d, \"rows\": %ld, \"info\": %d, \"sites_seen\": %d, \"n_up_seen\": %d, \"energy\": %.17g, \"s2\": %.17g, \"norm2\": %.17g, "
                  "\"sum_sz\": %.17g, \"sf0\": %.17g, \"sf0_expected\": %.17g, \"sf_pi\": %.17g, \"bond_spread\": %.6g, \"diagonal_error\": %.6g, "
                  "\"symmetric\": %d}",
                  pass ? ", " : "", nUp, static_cast<long>(n), static_cast<int>(sc.info() == Success), sc.sites(), sc.sitesUp(), energy, sc.totalSpinSquared(),
                  sc.normSquared(), sumSz, sc.structureFactorZ(0.0), (nUp - 0.5 * L) * (nUp - 0.5 * L) / L, sc.structureFactorZ(3.14159265358979323846), bondSpread,
                  diagonal, static_cast<int>(sc.szsz(1, 4) == sc.szsz(4, 1) && sc.sxy(0, L - 1) == sc.sxy(L - 1, 0)));
    }
    // the refusals
    const Index n = model.sectorRows(L / 2);
    const HostCsr<double> csr = model.toSectorCsr(L / 2);
    std::shared_ptr<device::CsrOperator> stored = std::make_shared<device::CsrOperator>(ctx, n, 0, n, csr.rowptr.data(), csr.col.data(), csr.val.data());
    std::shared_ptr<device::CsrOperator> spin = device::spinHalfSectorOperator(ctx, model, L / 2);
    DenseVector<double> ones(n), zero(n), shorter(n - 1);
    for (Index r = 0; r < n; ++r) ones[r] = 1.0, zero[r] = 0.0;
    for (Index r = 0; r + 1 < n; ++r) shorter[r] = 1.0;
    SpinCorrelationSolver a, b, c, d;
    a.setDeviceOperator(stored).setState(ones);
    a.compute();
    b.setDeviceOperator(spin).setState(zero);
    b.compute();
    c.setDeviceOperator(spin).setState(shorter);
    c.compute();
    d.setState(ones);
    d.compute();
    const bool refusedZero = refused(b);
    bool threw = false;
    try {
      (void)b.sz(0);
    } catch (const LanczosException&) {
      threw = true;
    }
    // the uniform state of the sector after the refusals: the same solver object computes again
    b.setState(ones);
    b.compute();
    std::printf("], \"refused_csr\": %d, \"refused_zero\": %d, \"refused_length\": %d, \"refused_no_operator\": %d, \"no_result_throws\": %d, "
                "\"uniform_info\": %d, \"uniform_sum_sz\": %.17g}\n",
                static_cast<int>(refused(a)), static_cast<int>(refusedZero), static_cast<int>(refused(c)), static_cast<int>(refused(d)), static_cast<int>(threw),
                static_cast<int>(b.info() == Success), b.sz(0) * L);
  } catch (const std::exception& e) {
    std::printf("{\"error\": \"%s\"}\n", e.what());
    return 1;
  }
  return 0;
}
