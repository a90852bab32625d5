// C++11 user program: SpinEntanglementSolver on the periodic spin-1/2 Heisenberg ring (L sites, default 12).  The ground state
// of the sector nUp = L/2 through LanczosEigenSolver<double> with the matrix-free sector operator, then the reduced density
// matrix of the sites 0 .. L/2 - 1 and of their complement in one call each.  Prints JSON: info, the blocks (sites up and
// dimension), the entropy of both cuts, the Renyi entropies, the trace of rho_A, the Schmidt rank; and whether a stored CSR
// operator, an empty subsystem, a site named twice, a state of the wrong length and no operator at all end in InvalidInput
// with an ERROR line in the log.  tests/test_gpu_spin_rdm.py reads it.
// usage: spin_entanglement_amd [L]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "cmpt/eigen_ex/lanczos.hpp"
#include "cmpt/eigen_ex/spin_entanglement.hpp"

using namespace cmpt::EigenEx;

static bool refused(const SpinEntanglementSolver& se) {
  bool line = false;
  for (const std::string& l : se.log()) line = line || l.compare(0, SpinEntanglementSolver::headERROR().size(), SpinEntanglementSolver::headERROR()) == 0;
  return se.info() == InvalidInput && line && se.blocks() == 0;
}

int main(int argc, char** argv) {
  const int L = argc > 1 ? std::atoi(argv[1]) : 12;
  try {
    const SpinHalfModel model = SpinHalfModel::chain(L, 1.0, 1.0, true);
    std::shared_ptr<device::Context> ctx = std::make_shared<device::Context>(0);
    const int nUp = L / 2;
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
    DenseVector<double> x(n);
    for (Index r = 0; r < n; ++r) x[r] = 3.0 * es.eigenvectors().colData(0)[r];  // not normalised: the solver divides by <v|v>
    std::vector<int> half, rest;
    for (int i = 0; i < L; ++i) (i < L / 2 ? half : rest).push_back(i);
    SpinEntanglementSolver se, sc;
    se.setDeviceOperator(op).setState(x).setSubsystem(half);
    se.compute();
    sc.setDeviceOperator(op).setState(x).setSubsystemMask(((std::uint32_t(1) << L) - 1) & ~((std::uint32_t(1) << (L / 2)) - 1));
    sc.compute();
    double trace = 0.0, asym = 0.0;
    std::printf("{\"sites\": %d, \"n_up\": %d, \"rows\": %ld, \"energy\": %.17g, \"info\": %d, \"blocks\": [", L, nUp, static_cast<long>(n), es.eigenvalues()[0],
                static_cast<int>(se.info() == Success));
    for (Index b = 0; b < se.blocks(); ++b) {
      const Index d = se.blockDimension(b);
      const std::vector<double>& rho = se.reducedDensityMatrix(b);
      for (Index i = 0; i < d; ++i) {
        trace += rho[static_cast<std::size_t>(i + i * d)];
        for (Index j = 0; j < d; ++j) asym = std::fmax(asym, std::fabs(rho[static_cast<std::size_t>(i + j * d)] - rho[static_cast<std::size_t>(j + i * d)]));
      }
      std::printf("%s[%d, %ld]", b ? ", " : "", se.blockSitesUp(b), static_cast<long>(d));
    }
    double sum2 = 0.0;
    for (double lam : se.spectrum()) sum2 += lam * lam;
    std::printf("], \"entropy\": %.17g, \"entropy_complement\": %.17g, \"trace\": %.17g, \"asymmetry\": %.6g, \"norm2\": %.17g, \"renyi2\": %.17g, "
                "\"renyi2_spectrum\": %.17g, \"renyi_half\": %.17g, \"renyi_near_one\": %.17g, \"eigenvalues\": %ld, \"schmidt_rank\": %ld, "
                "\"largest\": %.17g, \"sites_seen\": %d, \"n_up_seen\": %d, \"mask\": %u",
                se.entropy(), sc.entropy(), trace, asym, se.normSquared(), se.renyi2(), -std::log(sum2), se.renyi(0.5), se.renyi(1.0 + 1.0e-6),
                static_cast<long>(se.spectrum().size()), static_cast<long>(se.schmidtRank(1.0e-12)), se.spectrum()[0], se.sites(), se.sitesUp(),
                static_cast<unsigned>(se.subsystemMask()));
    // the refusals
    const HostCsr<double> csr = model.toSectorCsr(nUp);
    std::shared_ptr<device::CsrOperator> stored = std::make_shared<device::CsrOperator>(ctx, n, 0, n, csr.rowptr.data(), csr.col.data(), csr.val.data());
    DenseVector<double> ones(n), shorter(n - 1);
    for (Index r = 0; r < n; ++r) ones[r] = 1.0;
    for (Index r = 0; r + 1 < n; ++r) shorter[r] = 1.0;
    SpinEntanglementSolver a, b, c, d, e, f;
    a.setDeviceOperator(stored).setState(ones).setSubsystem(half);
    a.compute();
    b.setDeviceOperator(op).setState(ones).setSubsystem(std::vector<int>());
    b.compute();
    c.setDeviceOperator(op).setState(ones).setSubsystem({0, 1, 1});
    c.compute();
    d.setDeviceOperator(op).setState(shorter).setSubsystem(half);
    d.compute();
    e.setState(ones).setSubsystem(half);
    e.compute();
    f.setDeviceOperator(op).setState(ones).setSubsystemMask((std::uint32_t(1) << L) - 1);
    f.compute();
    const bool refusedEmpty = refused(b);
    bool threw = false;
    try {
      (void)b.reducedDensityMatrix(0);
    } catch (const LanczosException&) {
      threw = true;
    }
    // the uniform state after the refusal, one site: the same solver object computes again
    b.setSubsystem({L - 1});
    b.compute();
    std::printf(", \"refused_csr\": %d, \"refused_empty\": %d, \"refused_twice\": %d, \"refused_length\": %d, \"refused_no_operator\": %d, \"refused_all\": %d, "
                "\"no_result_throws\": %d, \"uniform_info\": %d, \"uniform_blocks\": %ld, \"uniform_entropy\": %.17g}\n",
                static_cast<int>(refused(a)), static_cast<int>(refusedEmpty), static_cast<int>(refused(c)), static_cast<int>(refused(d)), static_cast<int>(refused(e)),
                static_cast<int>(refused(f)), static_cast<int>(threw), static_cast<int>(b.info() == Success), static_cast<long>(b.blocks()), b.entropy());
  } catch (const std::exception& e) {
    std::printf("{\"error\": \"%s\"}\n", e.what());
    return 1;
  }
  return 0;
}
