// ThermalLanczosSolver and ThermalEnsemble in a C++11 user program (-Wall -Wextra): the exact-trace case of
// tests/test_gpu_thermal_lanczos.py -- ring of 8 sites, Jz = 1, Jxy = 0.7, sector (8,4), the 70 unit vectors as samples, M = 70 -- and
// the ensemble of the sectors n_up <= 4.  Prints one JSON object with the figures the Python wrapper gives for the same case;
// the test holds them against dense diagonalisation.
#include <cmath>
#include <cstdio>
#include <vector>

#include "cmpt/eigen_ex/spin_operator.hpp"
#include "cmpt/eigen_ex/thermal_lanczos.hpp"

using namespace cmpt::EigenEx;

int main() {
  try {
    const int L = 8;
    const double betas[4] = {0.0, 0.5, 2.0, 10.0};
    const SpinHalfModel model = SpinHalfModel::chain(L, 1.0, 0.7, true);
    std::shared_ptr<device::Context> ctx = std::make_shared<device::Context>(0);
    ThermalEnsemble ensemble(L);
    std::printf("{");
    for (int nUp = 0; nUp <= L / 2; ++nUp) {
      const Index n = model.sectorRows(nUp);
      std::shared_ptr<device::CsrOperator> op = device::spinHalfSectorOperator(ctx, model, nUp);
      std::vector<double> unit(static_cast<std::size_t>(n) * static_cast<std::size_t>(n), 0.0);
      for (Index i = 0; i < n; ++i) unit[static_cast<std::size_t>(i) * static_cast<std::size_t>(n) + static_cast<std::size_t>(i)] = 1.0;
      ThermalLanczosSolver<double> th;
      th.setDeviceOperator(op).setLanczosSteps(n).setSampleVectors(unit.data(), n, n);
      const ComputationInfo masks = th.setAllSitesAndPairs();
      th.compute();
      ensemble.add(th, nUp == L / 2 ? 1.0 : 2.0, nUp - L / 2.0);
      if (nUp != L / 2) continue;
      std::printf("\"rows\": %lld, \"samples\": %lld, \"info\": %d, \"masks\": %d, \"applications\": %lld, \"sector\": [", static_cast<long long>(th.dimension()),
                  static_cast<long long>(th.samples()), static_cast<int>(th.info()), static_cast<int>(masks), static_cast<long long>(th.operatorApplications()));
      for (int b = 0; b < 4; ++b) {
        std::printf("%s{\"beta\": %.17g, \"logZ\": %.17g, \"E\": %.17g, \"C\": %.17g, \"S\": %.17g, \"zz\": [", b ? ", " : "", betas[b], th.logPartitionFunction(betas[b]),
                    th.energy(betas[b]), th.specificHeat(betas[b]), th.entropy(betas[b]));
        for (int i = 0, k = 0; i < L; ++i)
          for (int j = i + 1; j < L; ++j, ++k) std::printf("%s%.17g", k ? ", " : "", th.correlationZZ(i, j, betas[b]));
        std::printf("], \"xy\": [");
        for (int i = 0, k = 0; i < L; ++i)
          for (int j = i + 1; j < L; ++j, ++k) std::printf("%s%.17g", k ? ", " : "", th.correlationXY(i, j, betas[b]));
        std::printf("], \"energy_error\": %.17g}", th.standardError(ThermalQuantity::Energy, betas[b]));
      }
      std::printf("], ");
      // a complex solver takes no observables; a solver without an operator refuses to compute
      ThermalLanczosSolver<std::complex<double>> tz;
      ThermalLanczosSolver<double> none;
      none.compute();
      std::printf("\"complex_masks\": %d, \"no_operator\": %d, ", static_cast<int>(tz.setSpinObservables({1u}, {})), static_cast<int>(none.info()));
    }
    std::printf("\"ensemble\": [");
    for (int b = 0; b < 4; ++b)
      std::printf("%s{\"beta\": %.17g, \"logZ\": %.17g, \"E\": %.17g, \"C\": %.17g, \"S\": %.17g, \"chi\": %.17g, \"zz01\": %.17g}", b ? ", " : "", betas[b],
                  ensemble.logPartitionFunction(betas[b]), ensemble.energy(betas[b]), ensemble.specificHeat(betas[b]), ensemble.entropy(betas[b]),
                  ensemble.susceptibility(betas[b]), ensemble.observable(static_cast<std::size_t>(L), betas[b]) / 4);
    std::printf("]}\n");
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 1;
  }
}
