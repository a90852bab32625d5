// C++11 user program: SpinDynamicsSolver on the periodic spin-1/2 Heisenberg ring, 12 sites, sector nUp = 6.  The ground state
// through LanczosEigenSolver<double> with the matrix-free sector operator, then Szz(q = pi, w) by the Lanczos continued fraction.
// Prints JSON: the energy, the lowest pole that carries weight (the triplet gap), the total weight and the static structure
// factor it must equal; and whether no model, a state of the wrong length, PLUS from the sector with every site up and a zero
// state end in InvalidInput with an ERROR line in the log.  Exits non-zero if the main computation ends in InvalidInput.
// NOT part of the reference.  tests/test_gpu_spin_dynamics.py reads it.
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "cmpt/eigen_ex/lanczos.hpp"
#include "cmpt/eigen_ex/spin_correlations.hpp"
#include "cmpt/eigen_ex/spin_dynamics.hpp"

using namespace cmpt::EigenEx;

static bool refused(const SpinDynamicsSolver& sd) {
  bool line = false;
  for (const std::string& l : sd.log()) line = line || l.compare(0, SpinDynamicsSolver::headERROR().size(), SpinDynamicsSolver::headERROR()) == 0;
  return sd.info() == InvalidInput && line && sd.poles().empty() && sd.totalWeight() == 0.0;
}

int main() {
  const int L = 12, nUp = 6;
  const double pi = 3.14159265358979323846;
  try {
    const SpinHalfModel model = SpinHalfModel::chain(L, 1.0, 1.0, true);
    std::shared_ptr<device::Context> ctx = std::make_shared<device::Context>(0);
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
    for (Index r = 0; r < n; ++r) x[r] = es.eigenvectors().colData(0)[r];

    SpinDynamicsSolver sd;
    sd.setModel(ctx, model, nUp).setState(x).setLanczosSteps(60);
    sd.computeStructureFactorZ(pi);
    if (sd.info() == InvalidInput) {
      for (const std::string& l : sd.log()) std::fprintf(stderr, "%s\n", l.c_str());
      return 2;
    }
    double lowest = 0.0, sum = 0.0;
    bool found = false;
    for (std::size_t k = 0; k < sd.poles().size(); ++k) sum += sd.weights()[k];
    for (std::size_t k = 0; k < sd.poles().size() && !found; ++k)
      if (sd.weights()[k] > 1e-12 * sum) lowest = sd.poles()[k], found = true;
    SpinCorrelationSolver sc;
    sc.setDeviceOperator(op).setState(x);
    sc.compute();

    SpinDynamicsSolver none;
    none.setState(x).setSiteOperator(EIGENEX_SPIN_SITE_Z, std::vector<double>(L, 1.0));
    none.compute();
    const bool refusedNoModel = refused(none);
    SpinDynamicsSolver bad;
    bad.setModel(ctx, model, nUp).setSiteOperator(EIGENEX_SPIN_SITE_MINUS, std::vector<double>(L, 1.0)).setState(DenseVector<double>(n - 1, 1.0));
    bad.compute();
    const bool refusedLength = refused(bad);
    bad.setState(DenseVector<double>(n, 0.0));
    bad.compute();
    const bool refusedZero = refused(bad);
    SpinDynamicsSolver top;
    top.setModel(ctx, model, L).setSiteOperator(EIGENEX_SPIN_SITE_PLUS, std::vector<double>(L, 1.0)).setState(DenseVector<double>(1, 1.0));
    top.compute();
    const bool refusedPlus = refused(top);

    std::printf("{\"sites\": %d, \"rows\": %ld, \"info\": %d, \"energy\": %.17g, \"lowest_pole\": %.17g, \"total_weight\": %.17g, "
                "\"static_structure_factor\": %.17g, \"poles\": %ld, \"spectrum_at_gap\": %.17g, \"refused_no_model\": %d, \"refused_length\": %d, "
                "\"refused_plus_from_full\": %d, \"refused_zero\": %d}\n",
                sd.sites(), static_cast<long>(n), static_cast<int>(sd.info() == Success), energy, lowest, sd.totalWeight(), sc.structureFactorZ(pi),
                static_cast<long>(sd.poles().size()), sd.spectrum(lowest, 0.1), static_cast<int>(refusedNoModel), static_cast<int>(refusedLength),
                static_cast<int>(refusedPlus), static_cast<int>(refusedZero));
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "spin_dynamics_amd: %s\n", e.what());
    return 1;
  }
}
