// Dynamical spin correlations of a state of ONE MOMENTUM SECTOR by the Lanczos continued fraction, run in the small sector the
// operator leads to: O_q |v_k> lies in the sector k - q, so neither the state nor the m + 1 Lanczos columns ever take the size of
// the Sz sector.  At (32, 16) a real column is 150 MB where the Sz sector's is 4.8 GB, and beyond 32 sites no Sz-sector operator
// exists at all.
//
// NOT part of the reference.  The state |v> lives over the rows of the momentum sector (nUp, momentum, cell) of a SpinHalfModel
// (device::spinHalfMomentumOperator up to 32 sites, device::spinHalfMomentum64Operator above; the class picks the word).  O is a
// sum of site operators that carries a momentum (eigenex_spin_momentum_site_apply in eigenex_hip.h): a kind, `cell` complex cell
// coefficients cc[j] and an index p, with site coefficients c[j + cell r] = cc[j] e^{2 pi i p r / N}; it takes the sector
// (nUp, m) to (nUp, nUp + 1 or nUp - 1; (m - p) mod N), and the class builds that operator itself.  What follows the start vector
// -- the zero-response rule, the normalisation, m Lanczos steps, T = S diag(theta) S^T, poles and weights -- is
// SpinDynamicsSolver's (spin_frontend.hpp: detail::unitOrZero, detail::ContinuedFraction), and so are the results:
//   poles() p_n = theta_n - E0, weights() w_n = <phi|phi> / <v|v> S(0, n)^2, totalWeight(), moment(k), spectrum(w, eta).
// The run is a real one -- real operators and states, the library's default Lanczos scheme for them -- when m, the destination
// momentum, the state and every cell coefficient are real; otherwise the state is uploaded to a complex source handle and ONE
// complex fraction is run (there is no cos + sin pair here: the complex site coefficients are applied as they are).
//
// computeStructureFactorZ(qIndex) is Szz(q, w) at q = 2 pi qIndex / L for O = Sz_q = L^{-1/2} sum_r e^{iqr} Sz_r:
// cc[j] = L^{-1/2} e^{2 pi i qIndex j / L} (exactly +-1, +-i times L^{-1/2} at quarter turns) and p = qIndex mod N.
// totalWeight() is then the static structure factor, SpinMomentumCorrelationSolver::structureFactorZ(q).
//
// Out of scope: products of site operators; reflection and spin-inversion sectors; time evolution in momentum sectors; more than
// one GPU.
#pragma once

#include <cmath>
#include <complex>
#include <cstdint>
#include <string>
#include <vector>

#include "lanczos.hpp"
#include "spin_frontend.hpp"
#include "spin_operator.hpp"

namespace cmpt {
namespace EigenEx {

class SpinMomentumDynamicsSolver {
 public:
  using Index = EigenEx::Index;
  using VectorType = DenseVector<double>;
  using Complex = std::complex<double>;
  using ComplexVectorType = DenseVector<Complex>;

  static std::string headERROR() { return detail::CallLog::headERROR(); }
  static std::string headINFO() { return detail::CallLog::headINFO(); }

  SpinMomentumDynamicsSolver& setModel(const std::shared_ptr<device::Context>& ctx, const SpinHalfModel& model, int nUp, int momentum, int cell = 1) {
    ctx_ = ctx, model_ = model, nUp_ = nUp, momentum_ = momentum, cell_ = cell, haveModel_ = true;
    srcDev_.release(), dstDev_.release();  // the states go before their operators
    src_.reset(), dst_.reset();
    return *this;
  }
  // a host vector over the rows of the source momentum sector; it need not be normalised
  SpinMomentumDynamicsSolver& setState(const VectorType& v) {
    state_ = v, stateComplex_ = false;
    return *this;
  }
  SpinMomentumDynamicsSolver& setState(const ComplexVectorType& v) {
    stateZ_ = v, stateComplex_ = true;
    return *this;
  }
  SpinMomentumDynamicsSolver& setStateEnergy(double E0) {
    E0set_ = E0, haveE0_ = true;
    return *this;
  }
  // kind: EIGENEX_SPIN_SITE_Z, _PLUS or _MINUS; cellCoef: one complex coefficient per site of the cell; p: 0 .. N - 1
  SpinMomentumDynamicsSolver& setSiteOperator(int kind, const std::vector<Complex>& cellCoef, int p) {
    kind_ = kind, p_ = p;
    cellRe_.assign(cellCoef.size(), 0.0), cellIm_.assign(cellCoef.size(), 0.0);
    for (std::size_t j = 0; j < cellCoef.size(); ++j) cellRe_[j] = cellCoef[j].real(), cellIm_[j] = cellCoef[j].imag();
    return *this;
  }
  SpinMomentumDynamicsSolver& setLanczosSteps(Index m) {
    steps_ = m;
    return *this;
  }

  Index compute() {
    begin_("compute");
    if (!prepare_(kind_, p_, cellRe_, cellIm_)) return 0;
    run_(kind_, p_, cellRe_, cellIm_);
    finish_();
    return static_cast<Index>(poles_.size());
  }

  // Szz(q, w) at q = 2 pi qIndex / L (see the top of this file); the site operator that was set is not used
  Index computeStructureFactorZ(int qIndex) {
    begin_("computeStructureFactorZ");
    if (!haveModel_ || !ctx_) return invalid_("invalid input: no model (setModel)");
    const int L = model_.sites();
    if (L < 1 || cell_ < 1 || L % cell_ != 0) return invalid_("invalid input: the cell must divide the number of sites");
    const int q = ((qIndex % L) + L) % L;
    const double scale = 1.0 / std::sqrt(static_cast<double>(L));
    std::vector<double> re(static_cast<std::size_t>(cell_), 0.0), im(static_cast<std::size_t>(cell_), 0.0);
    for (int j = 0; j < cell_; ++j) {
      const int t = (q * j) % L;  // the phase is t / L of a turn
      if ((4 * t) % L == 0) {
        static const double c[4] = {1.0, 0.0, -1.0, 0.0}, s[4] = {0.0, 1.0, 0.0, -1.0};
        re[static_cast<std::size_t>(j)] = scale * c[4 * t / L], im[static_cast<std::size_t>(j)] = scale * s[4 * t / L];
      } else {
        const double angle = 6.283185307179586476925286766559 * static_cast<double>(t) / static_cast<double>(L);
        re[static_cast<std::size_t>(j)] = scale * std::cos(angle), im[static_cast<std::size_t>(j)] = scale * std::sin(angle);
      }
    }
    const int p = q % (L / cell_);
    if (!prepare_(EIGENEX_SPIN_SITE_Z, p, re, im)) return 0;
    run_(EIGENEX_SPIN_SITE_Z, p, re, im);
    finish_();
    return static_cast<Index>(poles_.size());
  }

  // ---- results (after a compute; empty / zero after InvalidInput or a zero response) ----
  const std::vector<double>& poles() const { return poles_; }  // ascending
  const std::vector<double>& weights() const { return weights_; }
  double totalWeight() const { return total_; }
  double stateEnergy() const { return E0_; }
  double stateNormSquared() const { return vv_; }
  double spectrum(double omega, double eta) const {
    const double pi = 3.14159265358979323846;
    double s = 0.0;
    for (std::size_t n = 0; n < poles_.size(); ++n) s += weights_[n] * (eta / pi) / ((omega - poles_[n]) * (omega - poles_[n]) + eta * eta);
    return s;
  }
  double moment(int k) const {
    double s = 0.0;
    for (std::size_t n = 0; n < poles_.size(); ++n) s += weights_[n] * std::pow(poles_[n], k);
    return s;
  }
  const std::vector<double>& lanczosAlpha() const { return fraction_.alpha(); }
  const std::vector<double>& lanczosBeta() const { return fraction_.beta(); }
  // of the last run: the sector the continued fraction ran in (-1 and 0 before one)
  int destinationSitesUp() const { return dstUp_; }
  int destinationMomentum() const { return dstMomentum_; }
  Index destinationDimension() const { return dstRows_; }
  bool complexRun() const { return complexRun_; }
  ComputationInfo info() const { return log_.info(); }
  const std::vector<std::string>& log() const { return log_.log(); }

 private:
  void begin_(const char* who) {
    log_.begin("SpinMomentumDynamicsSolver", who);
    poles_.clear(), weights_.clear(), fraction_.clear();
    total_ = 0.0, E0_ = 0.0, vv_ = 0.0;
    dstUp_ = -1, dstMomentum_ = -1, dstRows_ = 0;
  }
  Index invalid_(const std::string& what) {
    poles_.clear(), weights_.clear();
    total_ = 0.0;
    return log_.invalid(what);
  }
  static bool realMomentum_(int N, int m) { return m == 0 || 2 * m == N; }
  std::shared_ptr<device::CsrOperator> makeOperator_(int nUp, int m) const {
    return model_.sites() <= 32 ? device::spinHalfMomentumOperator(ctx_, model_, nUp, m, cell_, complexRun_)
                                : device::spinHalfMomentum64Operator(ctx_, model_, nUp, m, cell_, complexRun_);
  }

  // checks, the source operator, the state on the device, <v|v> and E0; false after invalid_()
  bool prepare_(int kind, int p, const std::vector<double>& re, const std::vector<double>& im) {
    if (!haveModel_ || !ctx_) return invalid_("invalid input: no model (setModel)"), false;
    const int L = model_.sites();
    if (cell_ < 1 || L % cell_ != 0) return invalid_("invalid input: the cell must divide the number of sites"), false;
    const int N = L / cell_;
    if (momentum_ < 0 || momentum_ >= N) return invalid_("invalid input: the momentum must be 0..sites/cell - 1"), false;
    if (kind != EIGENEX_SPIN_SITE_Z && kind != EIGENEX_SPIN_SITE_PLUS && kind != EIGENEX_SPIN_SITE_MINUS)
      return invalid_("invalid input: no site operator (setSiteOperator: EIGENEX_SPIN_SITE_Z, _PLUS or _MINUS)"), false;
    if (p < 0 || p >= N) return invalid_("invalid input: the momentum index p of the site operator must be 0..sites/cell - 1"), false;
    const std::string why = detail::checkCoefficients(re, &im, cell_, "the site operator");
    if (!why.empty()) return invalid_(why + " of the cell"), false;
    if (steps_ < 1) return invalid_("invalid input: setLanczosSteps needs at least one step"), false;
    if (detail::dstUp(nUp_, kind) < 0 || detail::dstUp(nUp_, kind) > L || nUp_ < 0)
      return invalid_("invalid input: the site operator leaves the sectors of the model (S+ of the sector with every site up, S- of the one with none)"), false;
    bool realCoef = true;
    for (double c : im) realCoef = realCoef && c == 0.0;
    const bool z = stateComplex_ || !realCoef || !realMomentum_(N, momentum_) || !realMomentum_(N, (momentum_ - p + N) % N);
    if (z != complexRun_) {  // the other scalar type: its own operators and states
      srcDev_.release(), dstDev_.release();
      src_.reset(), dst_.reset();
      complexRun_ = z;
    }
    try {
      if (!src_) src_ = makeOperator_(nUp_, momentum_);
    } catch (const LanczosException& e) {
      return invalid_(std::string("invalid input: the model has no such operator: ") + e.what()), false;
    }
    const Index n = static_cast<Index>(src_->rows());
    if ((stateComplex_ ? stateZ_.size() : state_.size()) != n)
      return invalid_("invalid input: the state must have one entry per row of the momentum sector (setState)"), false;
    if (!srcDev_.alive()) srcDev_.create(ctx_, src_, n, 1, 0, z);
    if (!z) {
      srcDev_.upload(EIGENEX_VEC_COL(0), state_);
    } else if (stateComplex_) {
      srcDev_.upload(EIGENEX_VEC_COL(0), stateZ_);
    } else {
      ComplexVectorType promoted(n);
      for (Index r = 0; r < n; ++r) promoted[r] = Complex(state_[r], 0.0);
      srcDev_.upload(EIGENEX_VEC_COL(0), promoted);
    }
    device::check(eigenex_spin_momentum_measure(srcDev_.handle(), EIGENEX_VEC_COL(0), 0, nullptr, nullptr, &vv_), "eigenex_spin_momentum_measure");
    if (!(vv_ > 0.0) || !std::isfinite(vv_)) return invalid_("invalid input: the state is zero (or not finite)"), false;
    if (haveE0_) {
      E0_ = E0set_;
    } else {
      double vHv[2] = {0.0, 0.0};  // a complex state's dot has two parts; <v|H|v> is the real one
      device::check(eigenex_apply(srcDev_.handle(), EIGENEX_VEC_COL(0), EIGENEX_VEC_V, 0.0, vHv), "eigenex_apply");
      E0_ = vHv[0] / vv_;
    }
    return true;
  }

  // one continued fraction: |phi> = O|v> into the work vector of the destination state, then the shared tail
  void run_(int kind, int p, const std::vector<double>& re, const std::vector<double>& im) {
    const int N = model_.sites() / cell_;
    const int up = detail::dstUp(nUp_, kind), m2 = (momentum_ - p + N) % N;
    if (!dst_ || up != dstOpUp_ || m2 != dstOpMomentum_) {
      dstDev_.release();  // the state goes before its operator
      dst_.reset();
      try {
        dst_ = makeOperator_(up, m2);
      } catch (const LanczosException& e) {
        if (std::string(e.what()).find("the sector is empty") == std::string::npos) throw;
        dstUp_ = up, dstMomentum_ = m2;
        return log_.note("the destination sector has no rows: the response is identically zero");
      }
      dstOpUp_ = up, dstOpMomentum_ = m2;
    }
    const Index n = static_cast<Index>(dst_->rows());
    const Index m = std::min<Index>(steps_, n);
    const int cap = static_cast<int>(m + 1);
    if (!dstDev_.alive() || dstDev_.capacity() < cap)
      dstDev_.create(ctx_, dst_, n, cap, 0, complexRun_);
    else
      device::check(eigenex_basis_clear(dstDev_.handle()), "eigenex_basis_clear");
    dstUp_ = up, dstMomentum_ = m2, dstRows_ = n;
    const detail::SiteApplication phi = detail::applyMomentumSiteOperatorToUnit(srcDev_.handle(), EIGENEX_VEC_COL(0), dstDev_.handle(), complexRun_, kind, p,
                                                                                model_.sites(), re, im, vv_);
    if (phi.outcome == detail::SiteApplication::NotFinite) return void(log_.failed("O|v> is not finite"));
    if (phi.zero()) return log_.note(phi.zeroNote("O|v>", "the response"));
    fraction_.run(dstDev_.handle(), m, phi.norm2, vv_, E0_, log_);
  }

  void finish_() { fraction_.finish(info() == Success, poles_, weights_, total_); }

  std::shared_ptr<device::Context> ctx_;
  SpinHalfModel model_;
  bool haveModel_ = false, haveE0_ = false;
  int nUp_ = -1, momentum_ = 0, cell_ = 1, kind_ = -1, p_ = 0;
  std::vector<double> cellRe_, cellIm_;
  VectorType state_;
  ComplexVectorType stateZ_;
  bool stateComplex_ = false, complexRun_ = false;
  Index steps_ = 100;
  double E0set_ = 0.0;

  std::shared_ptr<device::CsrOperator> src_, dst_;
  int dstOpUp_ = -2, dstOpMomentum_ = -1;
  detail::KrylovDevice srcDev_, dstDev_;

  detail::ContinuedFraction fraction_;
  std::vector<double> poles_, weights_;
  double total_ = 0.0, E0_ = 0.0, vv_ = 0.0;
  int dstUp_ = -1, dstMomentum_ = -1;
  Index dstRows_ = 0;
  detail::CallLog log_;
};

}  // namespace EigenEx
}  // namespace cmpt
