// Unequal-time correlations C_AB(t) = <psi_0| e^{iHt} A^dagger e^{-iHt} B |psi_0> / <psi_0|psi_0> of a state of a spin-1/2 model
// by Krylov propagation of two vectors, matrix-free and with nothing but scalars crossing to the host between time points: spin
// spreading <Sz_j(t) Sz_0(0)>, S(q, t), the Green's functions <S+_j(t) S-_0(0)>.
//
// NOT part of the reference.  One source operator B = sum_i b_i S^k_i and any number of measured operators A_n = sum_i a_{n,i}
// S^k_i of the same kind k (EIGENEX_SPIN_SITE_Z, _PLUS or _MINUS), all with complex coefficients.  With psi(t) = e^{-iHt} psi_0 and
// phi(t) = e^{-iHt} B psi_0,
//   C_n(t) = <A_n psi(t) | phi(t)>.
// psi lives in the work vector of a complex Krylov state on the SOURCE operator (device::spinHalfComplexOperator of the model's
// space or sector), phi in that of a state on the DESTINATION operator -- S-_i takes the sector nUp to nUp - 1, S+_i to nUp + 1;
// the class builds it itself, as SpinDynamicsSolver does.  Both are kept as unit vectors, psi_0 / |psi_0| and B psi_0 / |B psi_0|,
// and <B^dagger B> = |B psi_0|^2 / |psi_0|^2 (sourceNormSquared()) is multiplied back.  evolve(dt) advances both by the sub-steps
// of SpinTimeEvolutionSolver (spin_evolution.hpp: detail::krylovSubStep), each vector with its own step control and the error
// budget setTolerance per call.  values() then takes, per measured operator, one eigenex_spin_site_apply_z of psi(t) into a spare
// column of phi's state and one eigenex_dots with phi(t).
//
// setEigenstate(E0) declares psi_0 an eigenstate of energy E0: psi(t) = e^{-i E0 t} psi_0 is not evolved, only phi is -- the
// ground-state S(q, t) at half the cost.  A_n psi_0 is then formed once and kept in a column of its own if there are at most
// kKeptOperators measured operators (each costs a vector of the destination); beyond that it is formed again per time point.
//
// errorBound() bounds |delta C_n| for every n: max_n ||A_n|| * |B psi_0| * (eps_psi + eps_phi), where eps_psi and eps_phi
// (stateErrorBound(), sourceErrorBound()) are the accumulated sub-step bounds of the two unit vectors since t = 0 and
// ||A|| <= sum_i |a_i| / 2 for Z, sum_i |a_i| for the flips (operatorNormBound(n)).  Like errorBound() of the evolution it is a
// bound in exact arithmetic.
//
// A B psi_0 that vanishes -- by the rule of SpinDynamicsSolver: |B psi_0|^2 <= (L 2^-52 sum_i |b_i|)^2 (Z: half of it), with
// |b| = |Re b| + |Im b| -- gives an identically zero response with Success, and is logged.  Invalid input (an operator that
// leaves the sectors, a coefficient count other than the number of sites, coefficients that are not finite, a missing state or
// operator) is logged and not thrown: info() becomes InvalidInput.  A change of the state, the operators' kind or source, the
// Krylov dimension or the eigenstate declaration starts again at t = 0, and the call that does so logs it; measured operators may
// be added between time points unless they are kept columns (then it starts again too).  After an evolve() that ended in
// NumericalIssue the two vectors may stand at different times: evolve() and values() are refused (InvalidInput) until one of those
// changes sets the run up again.
//
// Out of scope: operators of different kinds in one run (A of another kind than B changes the sector of psi and of phi
// differently); products of site operators; finite temperature (static quantities: thermal_lanczos.hpp); more than one GPU.
#pragma once

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdint>
#include <string>
#include <vector>

#include "spin_evolution.hpp"

namespace cmpt {
namespace EigenEx {

class SpinTimeCorrelationSolver {
 public:
  using Index = EigenEx::Index;
  using Complex = std::complex<double>;
  using VectorType = DenseVector<Complex>;
  using RealVectorType = DenseVector<double>;
  using Coefficients = std::vector<Complex>;

  static constexpr int kKeptOperators = 4;
  static constexpr Index kMaxSubSteps = detail::kKrylovMaxSubSteps;

  static std::string headERROR() { return detail::CallLog::headERROR(); }
  static std::string headINFO() { return detail::CallLog::headINFO(); }

  // nUp = -1: the full space (up to 30 sites); else the sector of nUp sites up (up to 32 sites, no transverse field)
  SpinTimeCorrelationSolver& setModel(const std::shared_ptr<device::Context>& ctx, const SpinHalfModel& model, int nUp = -1) {
    ctx_ = ctx, model_ = model, nUp_ = nUp, haveModel_ = true, haveState_ = false;
    release_();
    ops_.reset();
    return *this;
  }
  SpinTimeCorrelationSolver& setKrylovDimension(Index m) {
    if (m != m_) prepared_ = false;
    m_ = m;
    return *this;
  }
  SpinTimeCorrelationSolver& setTolerance(double tol) {
    tol_ = tol;
    return *this;
  }
  // a host vector over the rows of the model's space or sector; it need not be normalised.  A new state is not an eigenstate
  // until setEigenstate says so.
  SpinTimeCorrelationSolver& setState(const VectorType& v) {
    psi0_ = v, haveState_ = true, productState_ = false, eigen_ = false, prepared_ = false;
    return *this;
  }
  SpinTimeCorrelationSolver& setState(const RealVectorType& v) {
    VectorType z(v.size());
    for (Index r = 0; r < v.size(); ++r) z[r] = Complex(v[r], 0.0);
    return setState(z);
  }
  // the basis state with site i up where bit i of `bits` is set; it must lie in the sector
  SpinTimeCorrelationSolver& setProductState(std::uint32_t bits) {
    bits_ = bits, haveState_ = true, productState_ = true, eigen_ = false, prepared_ = false;
    return *this;
  }
  SpinTimeCorrelationSolver& setEigenstate(double E0) {
    E0_ = E0, eigen_ = true, prepared_ = false;
    return *this;
  }
  // B: a kind and one complex coefficient per site; the measured operators have the same kind
  SpinTimeCorrelationSolver& setSourceOperator(int kind, const Coefficients& coef) {
    kind_ = kind, source_ = coef, haveSource_ = true, prepared_ = false;
    return *this;
  }
  SpinTimeCorrelationSolver& addMeasuredOperator(const Coefficients& coef) {
    if (kept_) prepared_ = false;
    measured_.push_back(coef);
    return *this;
  }
  SpinTimeCorrelationSolver& clearMeasuredOperators() {
    if (kept_) prepared_ = false;
    measured_.clear();
    return *this;
  }
  // A_j = S^k_j for every site j, replacing the measured operators
  SpinTimeCorrelationSolver& setMeasuredSites() {
    clearMeasuredOperators();
    const std::size_t L = static_cast<std::size_t>(haveModel_ ? model_.sites() : 0);
    for (std::size_t j = 0; j < L; ++j) {
      Coefficients c(L, Complex(0.0, 0.0));
      c[j] = Complex(1.0, 0.0);
      addMeasuredOperator(c);
    }
    return *this;
  }
  // A = B = Sz_q = L^{-1/2} sum_r e^{iqr} Sz_r, the site index taken as position: C(t) = S^zz(q, t)
  SpinTimeCorrelationSolver& setMomentumZ(double q) {
    const int L = haveModel_ ? model_.sites() : 0;
    Coefficients c(static_cast<std::size_t>(L));
    const double scale = L > 0 ? 1.0 / std::sqrt(static_cast<double>(L)) : 0.0;
    for (int r = 0; r < L; ++r) c[static_cast<std::size_t>(r)] = Complex(scale * std::cos(q * r), scale * std::sin(q * r));
    setSourceOperator(EIGENEX_SPIN_SITE_Z, c);
    clearMeasuredOperators();
    return addMeasuredOperator(c);
  }
  Index krylovDimension() const { return m_; }
  double tolerance() const { return tol_; }

  // psi <- exp(-i H dt) psi and phi <- exp(-i H dt) phi; returns the number of sub-steps of both (0 after an error: info(), log())
  Index evolve(double dt) {
    begin_("evolve");
    if (!prepare_()) return 0;
    if (!std::isfinite(dt)) return invalid_("invalid input: dt is not finite");
    if (!(tol_ > 0.0) || !std::isfinite(tol_)) return invalid_("invalid input: setTolerance needs a positive tolerance");
    Index steps = 0;
    if (zero_) log_.note(zeroNote_);
    if (!zero_) {
      // a failed call may leave the two vectors at different times: nothing is read from them until the run is set up again
      if ((!eigen_ && !advance_(psiDev_, psiRows_(), dt, epsPsi_, steps)) || !advance_(phiDev_, phiRows_(), dt, epsPhi_, steps)) {
        broken_ = true;
        return 0;
      }
    }
    time_ += dt;
    log_.note("sub-steps: " + std::to_string(steps) + ", accumulated bounds: " + std::to_string(epsPsi_) + " (state), " +
                   std::to_string(epsPhi_) + " (source)");
    return steps;
  }

  // C_n(t), one per measured operator (empty after an error)
  std::vector<Complex> values() {
    begin_("values");
    std::vector<Complex> out;
    if (!prepare_()) return out;
    const std::size_t K = measured_.size();
    for (std::size_t n = 0; n < K; ++n)
      if (!checkCoefficients_(measured_[n], "a measured operator")) return out;
    out.assign(K, Complex(0.0, 0.0));
    if (zero_) return log_.note(zeroNote_), out;
    const double amplitude = std::sqrt(bnorm2_);
    const Complex phase = eigen_ ? Complex(std::cos(E0_ * time_), std::sin(E0_ * time_)) : Complex(1.0, 0.0);  // conj of e^{-i E0 t}
    for (std::size_t n = 0; n < K; ++n) {
      const int column = spare_ + (kept_ ? static_cast<int>(n) : 0);
      if (!kept_) applyMeasured_(n, column);
      double h[2] = {0.0, 0.0};
      device::check(eigenex_dots(phiDev_.handle(), EIGENEX_VEC_W, column, 1, 1, 0, h), "eigenex_dots");
      out[n] = amplitude * phase * Complex(h[0], h[1]);
    }
    return out;
  }

  double time() const { return time_; }
  // <B^dagger B> = |B psi_0|^2 / |psi_0|^2 (0 before the first evolve() or values(), and for a vanishing B psi_0)
  double sourceNormSquared() const { return prepared_ && !zero_ ? bnorm2_ : 0.0; }
  double stateErrorBound() const { return epsPsi_; }
  double sourceErrorBound() const { return epsPhi_; }
  // sum_i |a_i| / 2 for Z, sum_i |a_i| for the flips
  double operatorNormBound(std::size_t n) const {
    double sum = 0.0;
    if (n < measured_.size())
      for (const Complex& a : measured_[n]) sum += std::abs(a);
    return kind_ == EIGENEX_SPIN_SITE_Z ? 0.5 * sum : sum;
  }
  double errorBound(std::size_t n) const { return operatorNormBound(n) * std::sqrt(sourceNormSquared()) * (epsPsi_ + epsPhi_); }
  double errorBound() const {
    double worst = 0.0;
    for (std::size_t n = 0; n < measured_.size(); ++n) worst = std::max(worst, errorBound(n));
    return worst;
  }
  Index operatorApplications() const { return applications_; }
  std::size_t measuredOperators() const { return measured_.size(); }
  int sites() const { return haveModel_ ? model_.sites() : 0; }
  int sitesUp() const { return nUp_; }
  ComputationInfo info() const { return log_.info(); }
  const std::vector<std::string>& log() const { return log_.log(); }

 private:
  void begin_(const char* who) { log_.begin("SpinTimeCorrelationSolver", who); }
  Index invalid_(const std::string& what) { return log_.invalid(what); }
  Index failed_(const std::string& what) { return log_.failed(what); }
  void release_() {
    psiDev_.release(), phiDev_.release();  // the states go before their operators
    prepared_ = false, kept_ = false;
  }
  Index psiRows_() const { return static_cast<Index>(ops_.src->rows()); }
  Index phiRows_() const { return static_cast<Index>(ops_.dst->rows()); }
  static void split_(const Coefficients& c, std::vector<double>& re, std::vector<double>& im) {
    re.assign(c.size(), 0.0), im.assign(c.size(), 0.0);
    for (std::size_t i = 0; i < c.size(); ++i) re[i] = c[i].real(), im[i] = c[i].imag();
  }
  bool checkCoefficients_(const Coefficients& c, const char* whose) {
    std::vector<double> re, im;
    split_(c, re, im);
    const std::string why = detail::checkCoefficients(re, &im, model_.sites(), whose);
    return why.empty() || (invalid_(why), false);
  }

  // A_n psi (the work vector of psi's state) into column `column` of phi's state
  void applyMeasured_(std::size_t n, int column) {
    std::vector<double> re, im;
    split_(measured_[n], re, im);
    device::check(eigenex_spin_site_apply_z(psiDev_.handle(), EIGENEX_VEC_W, phiDev_.handle(), EIGENEX_VEC_COL(column), kind_, re.data(), im.data(), nullptr),
                  "eigenex_spin_site_apply_z");
  }

  // exp(-i H dt) on the work vector of `dev` in sub-steps; adds their bounds to eps and their number to steps
  bool advance_(detail::KrylovDevice& dev, Index rows, double dt, double& eps, Index& steps) {
    Index mine = 0;
    const char* failure = detail::advanceInSubSteps(dev.handle(), rows, std::min<Index>(m_, rows), tol_, dt, applications_, mine,
                                                    [&eps](const detail::KrylovSubStep& step, double) { eps += step.bound; });
    if (failure) return failed_(failure), false;
    steps += mine;
    return true;
  }

  // the checks, the two operators, psi_0 and B psi_0 on the device at t = 0; true if that stands already; false after invalid_()
  bool prepare_() {
    if (prepared_ && broken_)
      return invalid_("invalid input: the last evolve() failed and left the two vectors at different times; set the state, the source operator "
                      "or the Krylov dimension again, which starts at t = 0"),
             false;
    if (prepared_) return true;
    kept_ = false;
    if (!haveModel_ || !ctx_) return invalid_("invalid input: no model (setModel)"), false;
    const int L = model_.sites();
    if (!haveState_) return invalid_("invalid input: no state (setState, setProductState)"), false;
    if (!haveSource_) return invalid_("invalid input: no source operator (setSourceOperator, setMomentumZ)"), false;
    if (kind_ != EIGENEX_SPIN_SITE_Z && kind_ != EIGENEX_SPIN_SITE_PLUS && kind_ != EIGENEX_SPIN_SITE_MINUS)
      return invalid_("invalid input: the kind of the source operator must be EIGENEX_SPIN_SITE_Z, _PLUS or _MINUS"), false;
    if (!checkCoefficients_(source_, "the source operator")) return false;
    for (const Coefficients& a : measured_)
      if (!checkCoefficients_(a, "a measured operator")) return false;
    if (m_ < 2) return invalid_("invalid input: setKrylovDimension needs at least 2"), false;
    if (eigen_ && !std::isfinite(E0_)) return invalid_("invalid input: the energy of setEigenstate is not finite"), false;
    const int up = detail::dstUp(nUp_, kind_);
    if (nUp_ >= 0 && (up < 0 || up > L))
      return invalid_("invalid input: the operators leave the sectors of the model (S+ of the sector with every site up, S- of the one with none)"), false;
    try {
      const auto make = [this](int nUp) { return device::spinHalfComplexOperator(ctx_, model_, nUp); };
      if (!ops_.src) ops_.src = make(nUp_);
      if (!ops_.keeps(nUp_, up)) phiDev_.release();  // here the old state goes before the new operator is built, not after
      ops_.destination(nUp_, up, make, [this] { phiDev_.release(); });
    } catch (const LanczosException& e) {
      return invalid_(std::string("invalid input: the model has no such operator: ") + e.what()), false;
    }
    // psi_0, normalised
    const Index n = psiRows_();
    VectorType u;
    std::string why;
    if (productState_) {
      const Index row = detail::productStateRow(L, nUp_, n, bits_, why);
      if (row < 0) return invalid_(why), false;
      u = VectorType(n, Complex(0.0, 0.0));
      u[row] = Complex(1.0, 0.0);
    } else {
      double nrm = 0.0;
      u = detail::normalised(psi0_, n, nrm, why);
      if (!why.empty()) return invalid_(why), false;
    }
    const std::size_t K = measured_.size();
    const bool keep = eigen_ && K >= 1 && K <= static_cast<std::size_t>(kKeptOperators);
    // psi: the run's columns (none for an eigenstate, which is not evolved).  phi: the run's columns and the spare ones behind them.
    const int capPsi = eigen_ ? 1 : static_cast<int>(std::min<Index>(m_, n) + 2);
    const Index nd = phiRows_();
    spare_ = static_cast<int>(std::min<Index>(m_, nd) + 1);
    const int capPhi = spare_ + (keep ? static_cast<int>(K) : 1);
    psiDev_.create(ctx_, ops_.src, n, capPsi, 0, true);
    phiDev_.create(ctx_, ops_.dst, nd, capPhi, 0, true);
    psiDev_.upload(EIGENEX_VEC_W, u);
    if (time_ != 0.0 || applications_ > 0)  // a setting changed in the middle of a run
      log_.note("the run starts again at t = 0 (it stood at t = " + std::to_string(time_) + "): time, bounds and counters are cleared");
    time_ = 0.0, epsPsi_ = 0.0, epsPhi_ = 0.0, applications_ = 0, zero_ = false, bnorm2_ = 0.0, broken_ = false;
    std::vector<double> re, im;
    split_(source_, re, im);
    // B psi_0 of the unit vector psi_0, to unit length unless it vanishes
    const detail::SiteApplication b = detail::applySiteOperatorToUnit(psiDev_.handle(), EIGENEX_VEC_W, phiDev_.handle(), true, kind_, L, re, &im, 1.0);
    if (b.outcome == detail::SiteApplication::NotFinite) return failed_("B|psi_0> is not finite"), false;
    if (b.zero()) {
      zeroNote_ = b.zeroNote("B|psi_0>", "the response");
      zero_ = true;
    } else {
      bnorm2_ = b.norm2;
      if (keep) {
        kept_ = true;
        for (std::size_t k = 0; k < K; ++k) applyMeasured_(k, spare_ + static_cast<int>(k));
      }
    }
    prepared_ = true;
    return true;
  }

  std::shared_ptr<device::Context> ctx_;
  SpinHalfModel model_;
  bool haveModel_ = false, haveState_ = false, haveSource_ = false, productState_ = false, eigen_ = false;
  int nUp_ = -1, kind_ = -1;
  std::uint32_t bits_ = 0;
  Index m_ = 30;
  double tol_ = 1e-10, E0_ = 0.0;
  VectorType psi0_;
  Coefficients source_;
  std::vector<Coefficients> measured_;

  detail::SectorPair ops_;
  detail::KrylovDevice psiDev_, phiDev_;
  bool prepared_ = false, zero_ = false, kept_ = false, broken_ = false;
  int spare_ = 0;
  double time_ = 0.0, bnorm2_ = 0.0, epsPsi_ = 0.0, epsPhi_ = 0.0;
  Index applications_ = 0;
  detail::CallLog log_;
  std::string zeroNote_;
};

}  // namespace EigenEx
}  // namespace cmpt
