// C++11 user program: the entanglement of complex spin states through both classes.  (1) Two sites, one bond (Jz, Jxy), from
// |up down> in the sector (2,1): S_A(t) = -c^2 ln c^2 - s^2 ln s^2 with c = cos(Jxy t / 2), s = sin(Jxy t / 2), at three times, the
// last t = pi / (2 Jxy) where S = ln 2; from SpinTimeEvolutionSolver::entanglementEntropy and, for the downloaded state, from
// SpinEntanglementSolver on the operator for complex states.  (2) The Neel state of the open XXZ chain of 10 sites in the sector
// (10,5) after four calls of evolve(0.25), A = sites 0..4: entropy, Renyi-2 and spectrum by mask and by site list from the
// evolution solver, the same from SpinEntanglementSolver with the downloaded state, and the complement.  Prints JSON; whether an
// invalid subsystem is logged, a complex state on the operator for real states ends in InvalidInput, and reducedDensityMatrix of a
// complex state throws.  Exits non-zero if a computation that must succeed does not.
// NOT part of the reference.  tests/test_gpu_spin_rdm_z.py reads it.
#include <cmath>
#include <complex>
#include <cstdio>
#include <vector>

#include "cmpt/eigen_ex/spin_entanglement.hpp"
#include "cmpt/eigen_ex/spin_evolution.hpp"

using namespace cmpt::EigenEx;

template <class Solver>
static bool refused(const Solver& s) {
  bool line = false;
  for (const std::string& l : s.log()) line = line || l.compare(0, Solver::headERROR().size(), Solver::headERROR()) == 0;
  return s.info() == InvalidInput && line;
}

template <class Solver>
static int fail(const Solver& s, int code) {
  for (const std::string& l : s.log()) std::fprintf(stderr, "%s\n", l.c_str());
  return code;
}

int main() {
  try {
    std::shared_ptr<device::Context> ctx = std::make_shared<device::Context>(0);
    // (1)
    const double Jz = 0.6, Jxy = 1.3, kPi = 3.14159265358979323846;
    double closed_evolution = 0.0, closed_class = 0.0, s_last = 0.0, t_last = 0.0;
    {
      const SpinHalfModel two = SpinHalfModel::chain(2, Jz, Jxy, false);
      SpinTimeEvolutionSolver te;
      te.setModel(ctx, two, 1).setProductState(1u);  // site 0 up
      if (te.info() != Success) return fail(te, 2);
      if (te.entanglementEntropy(1u) != 0.0) return fail(te, 3);  // a product state
      std::shared_ptr<device::CsrOperator> op = device::spinHalfComplexOperator(ctx, two, 1);
      const double times[3] = {0.4, 1.1, kPi / (2.0 * Jxy)};
      for (int k = 0; k < 3; ++k) {
        if (te.evolve(times[k] - te.time()) < 1 || te.info() != Success) return fail(te, 4);
        const double t = te.time(), c2 = std::cos(Jxy * t / 2) * std::cos(Jxy * t / 2), s2 = std::sin(Jxy * t / 2) * std::sin(Jxy * t / 2);
        const double want = -c2 * std::log(c2) - s2 * std::log(s2);
        const double got = te.entanglementEntropy(std::vector<int>{0});
        if (te.info() != Success) return fail(te, 5);
        closed_evolution = std::max(closed_evolution, std::fabs(got - want));
        SpinEntanglementSolver se;
        se.setDeviceOperator(op).setState(te.state()).setSubsystemMask(1u).compute();
        if (se.info() != Success) return fail(se, 6);
        closed_class = std::max(closed_class, std::fabs(se.entropy() - want));
        s_last = got, t_last = t;
      }
    }
    // (2)
    const int L = 10, nUp = 5;
    const SpinHalfModel model = SpinHalfModel::chain(L, 0.6, 1.0, false);
    std::uint32_t neel = 0;
    for (int i = 0; i < L; i += 2) neel |= std::uint32_t(1) << i;
    SpinTimeEvolutionSolver te;
    te.setModel(ctx, model, nUp).setKrylovDimension(12).setTolerance(1e-9).setProductState(neel);
    if (te.info() != Success) return fail(te, 7);
    const double s0 = te.entanglementEntropy(0x1Fu);
    for (int k = 0; k < 4; ++k) {
      te.evolve(0.25);
      if (te.info() != Success) return fail(te, 8);
    }
    const double t_before = te.time(), bound_before = te.totalErrorBound();
    const Index applications_before = te.operatorApplications();
    const double s_mask = te.entanglementEntropy(0x1Fu), s_list = te.entanglementEntropy(std::vector<int>{0, 1, 2, 3, 4});
    const double s_complement = te.entanglementEntropy(0x3E0u), r2 = te.entanglementRenyi2(0x1Fu);
    const std::vector<double> lam = te.entanglementSpectrum(0x1Fu);
    if (te.info() != Success) return fail(te, 9);
    double sum = 0.0, sum2 = 0.0;
    bool descending = true;
    for (std::size_t i = 0; i < lam.size(); ++i) sum += lam[i], sum2 += lam[i] * lam[i], descending = descending && (i == 0 || lam[i] <= lam[i - 1]);
    const bool untouched = te.time() == t_before && te.totalErrorBound() == bound_before && te.operatorApplications() == applications_before;

    std::shared_ptr<device::CsrOperator> zop = device::spinHalfComplexOperator(ctx, model, nUp);
    SpinEntanglementSolver se;
    se.setDeviceOperator(zop).setState(te.state()).setSubsystem({0, 1, 2, 3, 4}).compute();
    if (se.info() != Success) return fail(se, 10);
    double trace = 0.0, asym = 0.0, diag_im = 0.0;
    for (Index n = 0; n < se.blocks(); ++n) {
      const std::vector<std::complex<double>>& rho = se.reducedDensityMatrixComplex(n);
      const Index d = se.blockDimension(n);
      for (Index i = 0; i < d; ++i) {
        trace += rho[static_cast<std::size_t>(i + i * d)].real();
        diag_im = std::max(diag_im, std::fabs(rho[static_cast<std::size_t>(i + i * d)].imag()));
        for (Index j = 0; j < d; ++j) asym = std::max(asym, std::abs(rho[static_cast<std::size_t>(i + j * d)] - std::conj(rho[static_cast<std::size_t>(j + i * d)])));
      }
    }
    bool real_block_throws = false;
    try {
      se.reducedDensityMatrix(0);
    } catch (const LanczosException&) {
      real_block_throws = true;
    }
    // invalid input: logged, not thrown
    te.entanglementEntropy(0u);
    const bool refused_zero = refused(te);
    te.entanglementEntropy(std::vector<int>{0, 0});
    const bool refused_twice = refused(te);
    te.entanglementSpectrum(0x3FFu);
    const bool refused_all = refused(te);
    SpinTimeEvolutionSolver none;
    none.entanglementEntropy(1u);
    SpinEntanglementSolver wrong;  // a complex state on the operator for real states
    wrong.setDeviceOperator(device::spinHalfSectorOperator(ctx, model, nUp)).setState(te.state()).setSubsystemMask(0x1Fu).compute();
    const bool still_works = te.entanglementEntropy(0x1Fu) == s_mask && te.info() == Success;

    std::printf("{\"closed_evolution\": %.3e, \"closed_class\": %.3e, \"s_last\": %.17g, \"t_last\": %.17g, \"s0\": %.17g, \"s_mask\": %.17g, \"s_list\": %.17g, "
                "\"s_complement\": %.17g, \"renyi2\": %.17g, \"renyi2_spectrum\": %.17g, \"eigenvalues\": %d, \"sum\": %.17g, \"descending\": %d, \"untouched\": %d, "
                "\"class_entropy\": %.17g, \"class_renyi2\": %.17g, \"class_blocks\": %d, \"class_norm2\": %.17g, \"trace\": %.17g, \"asymmetry\": %.3e, "
                "\"diagonal_imag\": %.3e, \"real_block_throws\": %d, \"refused_zero\": %d, \"refused_twice\": %d, \"refused_all\": %d, \"refused_no_state\": %d, "
                "\"refused_real_operator\": %d, \"still_works\": %d, \"total_bound\": %.3e}\n",
                closed_evolution, closed_class, s_last, t_last, s0, s_mask, s_list, s_complement, r2, -std::log(sum2), static_cast<int>(lam.size()), sum,
                descending ? 1 : 0, untouched ? 1 : 0, se.entropy(), se.renyi2(), static_cast<int>(se.blocks()), se.normSquared(), trace, asym, diag_im,
                real_block_throws ? 1 : 0, refused_zero ? 1 : 0, refused_twice ? 1 : 0, refused_all ? 1 : 0, refused(none) ? 1 : 0, refused(wrong) ? 1 : 0,
                still_works ? 1 : 0, te.totalErrorBound());
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 1;
  }
}
