// Dynamical spin correlations of a state of a spin-1/2 model by the Lanczos continued fraction (E. R. Gagliano and C. A.
// Balseiro, Phys. Rev. Lett. 59 (1987) 2999), matrix-free and without the start vector ever visiting the host.
//
// NOT part of the reference.  For a real state |v> over the rows of a SpinHalfModel (full space, or the sector of nUp sites up)
// with energy E0, and O a sum of site operators (a kind and real coefficients c_i: sum_i c_i Sz_i, sum_i c_i S+_i or
// sum_i c_i S-_i),
//   S_O(w) = sum_n |<n| O |v>|^2 delta(w - (E_n - E0)) / <v|v>
// compute() uploads v once, forms |phi> = O|v> on the device (eigenex_spin_site_apply) straight into the work vector of a
// state on the DESTINATION operator -- S-_i takes the sector nUp to nUp - 1, S+_i to nUp + 1; the class builds that operator
// itself --, runs m Lanczos steps from it in the library's default scheme and diagonalises the tridiagonal matrix
// (small_eigen.hpp): T = S diag(theta) S^T.  Then
//   poles()       p_n = theta_n - E0                  weights()   w_n = <phi|phi> / <v|v> * S(0, n)^2
//   totalWeight() = sum_n w_n = <O^dagger O>          moment(k)   = sum_n w_n p_n^k   (exact for k < 2 m: Gauss quadrature)
//   spectrum(w, eta) = sum_n w_n (eta / pi) / ((w - p_n)^2 + eta^2), the Lorentzian-broadened continued fraction
// If O|v> = 0 -- or no larger than the roundings of the application can make an exact zero, |O v|^2 <= (L 2^-52 sum_i |c_i|)^2
// <v|v>, as for sum_i Sz_i on a state of a sector with Sz = 0 when the partial sums of w(s) round -- the response is
// identically zero: Success, no poles.  Otherwise |phi> is scaled to unit length on the device before the run.  A breakdown (an invariant subspace is exhausted before m
// steps) ends the fraction where the state reports it; the poles are then exact.  Without setStateEnergy, E0 = <v|H|v> / <v|v>
// from one operator application.
//
// computeStructureFactorZ(q) is Szz(q, w) for O = Sz_q = L^{-1/2} sum_r e^{iqr} Sz_r, the site index taken as position (as
// SpinCorrelationSolver::structureFactorZ does).  Coefficients are real here, so it runs the cos part, c_i = L^{-1/2} cos(q i), and
// the sin part, c_i = L^{-1/2} sin(q i), and merges their poles: for a real state and a real Hamiltonian the cross terms
// <v|A (w - H)^{-1} B|v> - <v|B (w - H)^{-1} A|v> of O = A + iB cancel, so the response is the sum of the two real runs.  A part
// whose O|v> is zero is skipped.  totalWeight() then equals the static structureFactorZ(q).
//
// A complex run.  setSiteOperator with complex coefficients, or setState with a complex vector, switches compute() to the operators
// for complex states (device::spinHalfComplexOperator: the same real Hamiltonian) and to eigenex_spin_site_apply_z: |phi> = O|v>
// with complex c_i is formed on the device and ONE fraction is run from it; the Lanczos coefficients of a Hermitian operator are
// real, so everything after the run is as above.  computeStructureFactorZSingleRun(q) is Szz(q, w) with c_r = L^{-1/2} e^{iqr} in
// one such run -- half the operator applications of computeStructureFactorZ(q), whose poles and weights it does not reproduce one
// by one (one fraction of m steps stands for two), while moments, sum rule and broadened spectrum agree.  The real
// setSiteOperator, computeStructureFactorZ and what they return are untouched by this; computeStructureFactorZ(q) after setState
// with a complex vector is InvalidInput (its two real runs stand for a real state only) and names the single run.
//
// Out of scope: products of site operators as O; a basis-free three-term recurrence for
// very long fractions (the run keeps m + 1 columns, like every Lanczos run here); more than one GPU (the matrix-free spin
// operators are one shard); finite temperature (static quantities: thermal_lanczos.hpp).
#pragma once

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "lanczos.hpp"
#include "small_eigen.hpp"
#include "spin_frontend.hpp"
#include "spin_operator.hpp"

namespace cmpt {
namespace EigenEx {

class SpinDynamicsSolver {
 public:
  using Index = EigenEx::Index;
  using VectorType = DenseVector<double>;
  using Complex = std::complex<double>;
  using ComplexVectorType = DenseVector<Complex>;

  static std::string headERROR() { return detail::CallLog::headERROR(); }
  static std::string headINFO() { return detail::CallLog::headINFO(); }

  // nUp = -1: the full space (up to 30 sites); else the sector of nUp sites up (up to 32 sites, no transverse field)
  SpinDynamicsSolver& setModel(const std::shared_ptr<device::Context>& ctx, const SpinHalfModel& model, int nUp = -1) {
    ctx_ = ctx, model_ = model, nUp_ = nUp, haveModel_ = true;
    srcDev_.release(), dstDev_.release();  // the states go before their operators
    ops_.reset();
    return *this;
  }
  // a host vector over the source rows, e.g. a column of a solver's eigenvectors(); it need not be normalised
  SpinDynamicsSolver& setState(const VectorType& v) {
    state_ = v, stateComplex_ = false;
    return *this;
  }
  // a complex state: the run is a complex one (see the top of this file)
  SpinDynamicsSolver& setState(const ComplexVectorType& v) {
    stateZ_ = v, stateComplex_ = true;
    return *this;
  }
  SpinDynamicsSolver& setStateEnergy(double E0) {
    E0set_ = E0, haveE0_ = true;
    return *this;
  }
  // kind: EIGENEX_SPIN_SITE_Z, _PLUS or _MINUS; coef: one real coefficient per site
  SpinDynamicsSolver& setSiteOperator(int kind, const std::vector<double>& coef) {
    kind_ = kind, coef_ = coef, coefComplex_ = false;
    coefIm_.clear();
    return *this;
  }
  // one complex coefficient per site: the run is a complex one
  SpinDynamicsSolver& setSiteOperator(int kind, const std::vector<Complex>& coef) {
    kind_ = kind, coefComplex_ = true;
    coef_.assign(coef.size(), 0.0), coefIm_.assign(coef.size(), 0.0);
    for (std::size_t i = 0; i < coef.size(); ++i) coef_[i] = coef[i].real(), coefIm_[i] = coef[i].imag();
    return *this;
  }
  SpinDynamicsSolver& setLanczosSteps(Index m) {
    steps_ = m;
    return *this;
  }

  Index compute() {
    begin_("compute");
    const bool z = stateComplex_ || coefComplex_;
    const std::vector<double>* im = coefComplex_ ? &coefIm_ : nullptr;
    if (!prepare_(kind_, coef_, im, z)) return 0;
    run_(kind_, coef_, im, z);
    finish_();
    return static_cast<Index>(poles_.size());
  }

  // Szz(q, w): the cos part and the sin part of Sz_q, merged (see the top of this file); the site operator that was set is not used
  Index computeStructureFactorZ(double q) {
    begin_("computeStructureFactorZ");
    if (!haveModel_ || !ctx_) return invalid_("invalid input: no model (setModel)");
    const int L = model_.sites();
    if (L < 1) return invalid_("invalid input: the model has no sites");
    std::vector<double> c(static_cast<std::size_t>(L), 0.0);
    if (!prepare_(EIGENEX_SPIN_SITE_Z, c, nullptr, false)) return 0;
    const double scale = 1.0 / std::sqrt(static_cast<double>(L));
    for (int part = 0; part < 2 && info() == Success; ++part) {
      for (int i = 0; i < L; ++i) c[static_cast<std::size_t>(i)] = scale * (part == 0 ? std::cos(q * i) : std::sin(q * i));
      run_(EIGENEX_SPIN_SITE_Z, c, nullptr, false);
    }
    finish_();
    return static_cast<Index>(poles_.size());
  }

  // Szz(q, w) from ONE complex run with c_r = L^{-1/2} e^{iqr} (see the top of this file); a real state is taken as a complex one.
  // The site operator that was set is not used.
  Index computeStructureFactorZSingleRun(double q) {
    begin_("computeStructureFactorZSingleRun");
    if (!haveModel_ || !ctx_) return invalid_("invalid input: no model (setModel)");
    const int L = model_.sites();
    if (L < 1) return invalid_("invalid input: the model has no sites");
    std::vector<double> cr(static_cast<std::size_t>(L), 0.0), ci(static_cast<std::size_t>(L), 0.0);
    const double scale = 1.0 / std::sqrt(static_cast<double>(L));
    for (int i = 0; i < L; ++i) cr[static_cast<std::size_t>(i)] = scale * std::cos(q * i), ci[static_cast<std::size_t>(i)] = scale * std::sin(q * i);
    if (!prepare_(EIGENEX_SPIN_SITE_Z, cr, &ci, true)) return 0;
    run_(EIGENEX_SPIN_SITE_Z, cr, &ci, true);
    finish_();
    return static_cast<Index>(poles_.size());
  }

  // ---- results (after compute(); empty / zero after InvalidInput or a zero response) ----
  const std::vector<double>& poles() const { return poles_; }      // ascending
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
  // the coefficients of the last Lanczos run (of the sin part after computeStructureFactorZ, if it ran)
  const std::vector<double>& lanczosAlpha() const { return fraction_.alpha(); }
  const std::vector<double>& lanczosBeta() const { return fraction_.beta(); }
  int sites() const { return haveModel_ ? model_.sites() : 0; }
  int sitesUp() const { return nUp_; }
  ComputationInfo info() const { return log_.info(); }
  const std::vector<std::string>& log() const { return log_.log(); }

 private:
  void begin_(const char* who) {
    log_.begin("SpinDynamicsSolver", who);
    poles_.clear(), weights_.clear(), fraction_.clear();
    total_ = 0.0, E0_ = 0.0, vv_ = 0.0;
  }
  Index invalid_(const std::string& what) {
    poles_.clear(), weights_.clear();
    total_ = 0.0;
    return log_.invalid(what);
  }
  Index failed_(const std::string& what) { return log_.failed(what); }
  std::shared_ptr<device::CsrOperator> makeOperator_(int nUp) const {
    if (complexRun_) return device::spinHalfComplexOperator(ctx_, model_, nUp);
    return nUp < 0 ? device::spinHalfOperator(ctx_, model_) : device::spinHalfSectorOperator(ctx_, model_, nUp);
  }

  // checks, the source operator, the state on the device, <v|v> and E0; false after invalid_()
  // coefIm: the imaginary parts of complex coefficients or null; z: a complex run (complex operators, states and site kernel)
  bool prepare_(int kind, const std::vector<double>& coef, const std::vector<double>* coefIm, bool z) {
    if (!haveModel_ || !ctx_) return invalid_("invalid input: no model (setModel)"), false;
    const int L = model_.sites();
    if (kind != EIGENEX_SPIN_SITE_Z && kind != EIGENEX_SPIN_SITE_PLUS && kind != EIGENEX_SPIN_SITE_MINUS)
      return invalid_("invalid input: no site operator (setSiteOperator: EIGENEX_SPIN_SITE_Z, _PLUS or _MINUS)"), false;
    const std::string why = detail::checkCoefficients(coef, coefIm, L, "the site operator");
    if (!why.empty()) return invalid_(why), false;
    if (steps_ < 1) return invalid_("invalid input: setLanczosSteps needs at least one step"), false;
    if (!z && stateComplex_)  // only computeStructureFactorZ asks for a real run whatever was set: its cos + sin sum holds for real states
      return invalid_("invalid input: computeStructureFactorZ needs a real state; a complex one takes computeStructureFactorZSingleRun"), false;
    if (nUp_ >= 0 && (detail::dstUp(nUp_, kind) < 0 || detail::dstUp(nUp_, kind) > L))
      return invalid_("invalid input: the site operator leaves the sectors of the model (S+ of the sector with every site up, S- of the one with none)"), false;
    if (z != complexRun_) {  // the other scalar type: its own operators and states
      srcDev_.release(), dstDev_.release();
      ops_.reset();
      complexRun_ = z;
    }
    try {
      if (!ops_.src) ops_.src = makeOperator_(nUp_);
    } catch (const LanczosException& e) {
      return invalid_(std::string("invalid input: the model has no such operator: ") + e.what()), false;
    }
    const Index n = static_cast<Index>(ops_.src->rows());
    if ((stateComplex_ ? stateZ_.size() : state_.size()) != n)
      return invalid_("invalid input: the state must have one entry per row of the model's space or sector (setState)"), false;
    if (!srcDev_.alive()) srcDev_.create(ctx_, ops_.src, n, 1, 0, z);
    if (!z) {
      srcDev_.upload(EIGENEX_VEC_COL(0), state_);
    } else if (stateComplex_) {
      srcDev_.upload(EIGENEX_VEC_COL(0), stateZ_);
    } else {
      ComplexVectorType promoted(n);
      for (Index r = 0; r < n; ++r) promoted[r] = Complex(state_[r], 0.0);
      srcDev_.upload(EIGENEX_VEC_COL(0), promoted);
    }
    device::check(eigenex_spin_measure(srcDev_.handle(), EIGENEX_VEC_COL(0), 0, nullptr, 0, nullptr, nullptr, nullptr, &vv_), "eigenex_spin_measure");
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

  // one continued fraction: |phi> = O|v> into the work vector of the destination state, m Lanczos steps, poles and weights appended
  void run_(int kind, const std::vector<double>& coef, const std::vector<double>* coefIm, bool z) {
    ops_.destination(nUp_, detail::dstUp(nUp_, kind), [this](int nUp) { return makeOperator_(nUp); }, [this] { dstDev_.release(); });
    const Index n = static_cast<Index>(ops_.dst->rows());
    const Index m = std::min<Index>(steps_, n);
    const int cap = static_cast<int>(m + 1);
    if (!dstDev_.alive() || dstDevOp_ != ops_.dst.get() || dstDev_.capacity() < cap) {
      dstDev_.create(ctx_, ops_.dst, n, cap, 0, z);
      dstDevOp_ = ops_.dst.get();
    } else {
      device::check(eigenex_basis_clear(dstDev_.handle()), "eigenex_basis_clear");
    }
    // the run starts from the unit vector O|v> / |O v| (V, which the scaling passed through, is overwritten by the run's first
    // operator application)
    const detail::SiteApplication phi =
        detail::applySiteOperatorToUnit(srcDev_.handle(), EIGENEX_VEC_COL(0), dstDev_.handle(), z, kind, model_.sites(), coef, coefIm, vv_);
    if (phi.outcome == detail::SiteApplication::NotFinite) return void(failed_("O|v> is not finite"));
    if (phi.zero()) return log_.note(phi.zeroNote("O|v>", "this part of the response"));
    fraction_.run(dstDev_.handle(), m, phi.norm2, vv_, E0_, log_);  // the tail every continued fraction shares (spin_frontend.hpp)
  }

  void finish_() { fraction_.finish(info() == Success, poles_, weights_, total_); }

  std::shared_ptr<device::Context> ctx_;
  SpinHalfModel model_;
  bool haveModel_ = false, haveE0_ = false;
  int nUp_ = -1, kind_ = -1;
  std::vector<double> coef_, coefIm_;
  VectorType state_;
  ComplexVectorType stateZ_;
  bool stateComplex_ = false, coefComplex_ = false, complexRun_ = false;
  Index steps_ = 100;
  double E0set_ = 0.0;

  detail::SectorPair ops_;
  const device::CsrOperator* dstDevOp_ = nullptr;
  detail::KrylovDevice srcDev_, dstDev_;

  detail::ContinuedFraction fraction_;
  std::vector<double> poles_, weights_;
  double total_ = 0.0, E0_ = 0.0, vv_ = 0.0;
  detail::CallLog log_;
};

}  // namespace EigenEx
}  // namespace cmpt
