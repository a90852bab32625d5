// Spin correlations of a state of a matrix-free spin-1/2 operator (spin_operator.hpp), measured on the device in one call.
//
// NOT part of the reference.  For a real vector v over the rows of device::spinHalfOperator (full space) or
// device::spinHalfSectorOperator (nUp sites up), compute() measures every site and every pair i < j at once
// (eigenex_spin_measure: v streams past once per 16 terms, nothing is written but the sums) and keeps
//   sz(i)      = <Sz_i>                          sx(i)     = <Sx_i>   (zero in a sector, without any gather)
//   szsz(i, j) = <Sz_i Sz_j>                     sxy(i, j) = <Sx_i Sx_j + Sy_i Sy_j>
//   dot(i, j)  = <S_i . S_j> = szsz + sxy        (i = j: 1/4, 1/2 and 3/4)
// all normalised by <v|v>.  From these follow
//   totalSpinSquared()   = sum_ij <S_i . S_j> = S(S + 1) of an eigenstate of an SU(2)-symmetric model: which multiplet a level of
//                          a sector belongs to
//   structureFactorZ(q)  = (1/L) sum_ij cos(q (i - j)) <Sz_i Sz_j>, the site index taken as position
// The vector is a host vector (e.g. a column of a solver's eigenvectors()) and is uploaded by compute().
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

class SpinCorrelationSolver {
 public:
  using Index = EigenEx::Index;
  using VectorType = DenseVector<double>;

  static std::string headERROR() { return detail::CallLog::headERROR(); }
  static std::string headINFO() { return detail::CallLog::headINFO(); }

  SpinCorrelationSolver& setDeviceOperator(const std::shared_ptr<device::CsrOperator>& op) {
    op_ = op;
    height_ = op ? static_cast<Index>(op->rows()) : 0;
    return *this;
  }
  SpinCorrelationSolver& setState(const VectorType& v) {
    state_ = v;
    return *this;
  }
  Index matrixHeight() const { return height_; }
  int sites() const { return sites_; }
  int sitesUp() const { return nUp_; }  // -1: the full space
  double normSquared() const { return norm2_; }

  Index compute() {
    log_.begin("SpinCorrelationSolver", "compute");
    sites_ = 0, nUp_ = -1, norm2_ = 0.0;
    sz_.clear(), sx_.clear(), zz_.clear(), xy_.clear();
    if (!op_ || height_ <= 0 || eigenex_spin_geometry(op_->handle(), &sites_, &nUp_) != 0) {
      sites_ = 0;
      return invalid_("invalid input: a matrix-free spin operator (device::spinHalfOperator, device::spinHalfSectorOperator) is required");
    }
    if (static_cast<Index>(state_.size()) != height_) return invalid_("invalid input: the state must have one entry per row of the operator");
    const std::size_t L = static_cast<std::size_t>(sites_);
    std::vector<std::uint32_t> diag, flip;
    detail::appendSiteMasks(L, diag);
    detail::appendPairMasks(L, diag);
    flip.assign(diag.begin() + static_cast<std::ptrdiff_t>(L), diag.end());
    if (nUp_ < 0) flip.insert(flip.end(), diag.begin(), diag.begin() + static_cast<std::ptrdiff_t>(L));  // <Sx_i>: the full space only
    if (!dev_.alive() || devOp_ != op_.get()) {
      dev_.create(op_->context(), op_, height_, 1, 0, false);
      devOp_ = op_.get();
    }
    dev_.upload(EIGENEX_VEC_COL(0), state_);
    std::vector<double> d(diag.size(), 0.0), f(flip.size(), 0.0);
    device::check(eigenex_spin_measure(dev_.handle(), EIGENEX_VEC_COL(0), static_cast<int>(diag.size()), diag.data(), static_cast<int>(flip.size()),
                                       flip.data(), d.data(), f.data(), &norm2_),
                  "eigenex_spin_measure");
    if (!(norm2_ > 0.0) || !std::isfinite(norm2_)) return invalid_("invalid input: the state is zero (or not finite)");
    const std::size_t npairs = L * (L - 1) / 2;
    sz_.assign(L, 0.0), sx_.assign(L, 0.0);
    for (std::size_t i = 0; i < L; ++i) {
      sz_[i] = d[i] / (2.0 * norm2_);
      if (nUp_ < 0) sx_[i] = f[npairs + i] / (2.0 * norm2_);
    }
    zz_ = detail::pairMatrix(d.data() + L, L, 4.0 * norm2_, 0.25);
    xy_ = detail::pairMatrix(f.data(), L, 2.0 * norm2_, 0.5);
    log_.note("sites: " + std::to_string(sites_) + (nUp_ < 0 ? std::string(", full space") : ", sites up: " + std::to_string(nUp_)) +
                   ", terms measured: " + std::to_string(diag.size() + flip.size()));
    return 0;
  }

  // ---- results (after a successful compute(); a site outside 0..sites()-1 throws) ----
  double sz(int i) const { return sz_[site_(i)]; }
  double sx(int i) const { return sx_[site_(i)]; }
  double szsz(int i, int j) const { return zz_[site_(i) * static_cast<std::size_t>(sites_) + site_(j)]; }
  double sxy(int i, int j) const { return xy_[site_(i) * static_cast<std::size_t>(sites_) + site_(j)]; }
  double dot(int i, int j) const { return szsz(i, j) + sxy(i, j); }
  double totalSpinSquared() const {
    double s = 0.0;
    for (int i = 0; i < sites_ && !zz_.empty(); ++i)
      for (int j = 0; j < sites_; ++j) s += dot(i, j);
    return s;
  }
  double structureFactorZ(double q) const {
    double s = 0.0;
    for (int i = 0; i < sites_ && !zz_.empty(); ++i)
      for (int j = 0; j < sites_; ++j) s += std::cos(q * static_cast<double>(i - j)) * szsz(i, j);
    return sites_ > 0 ? s / static_cast<double>(sites_) : 0.0;
  }
  ComputationInfo info() const { return log_.info(); }
  const std::vector<std::string>& log() const { return log_.log(); }

 private:
  Index invalid_(const std::string& what) {
    sz_.clear(), sx_.clear(), zz_.clear(), xy_.clear();
    return log_.invalid(what);
  }
  std::size_t site_(int i) const {
    if (i < 0 || i >= sites_ || sz_.empty()) throw LanczosException("SpinCorrelationSolver: no result for this site (compute() first; sites are 0..sites()-1)");
    return static_cast<std::size_t>(i);
  }

  std::shared_ptr<device::CsrOperator> op_;
  const device::CsrOperator* devOp_ = nullptr;
  detail::KrylovDevice dev_;
  Index height_ = 0;
  VectorType state_;
  int sites_ = 0, nUp_ = -1;
  double norm2_ = 0.0;
  std::vector<double> sz_, sx_, zz_, xy_;
  detail::CallLog log_;
};

// Diagonal correlations of a state of a momentum-sector operator (device::spinHalfMomentumOperator or
// device::spinHalfMomentum64Operator, real or complex states), measured in the momentum basis without expanding the state
// (eigenex_spin_momentum_measure): for a momentum eigenstate, <D> of a product D of sigma^z is sum_a |x_a|^2 (1/N) sum_r D(T^r a)
// over the representatives a.  compute() measures every site and every pair at once and keeps
//   magnetisation()      <Sz_i>, one entry per site
//   correlationsZZ()     <Sz_i Sz_j> as an L x L matrix (the diagonal is 1/4)
//   structureFactorZ(q)  (1/L) sum_ij cos(q (i - j)) <Sz_i Sz_j>
// stringCorrelator(mask) measures one further product, <prod_{i in mask} sigma^z_i> (sigma = 2 Sz), on the uploaded state.  For a
// singlet of an SU(2)-symmetric model <S_i . S_j> = 3 <Sz_i Sz_j>.  Off-diagonal correlators are not measured in this basis.
class SpinMomentumCorrelationSolver {
 public:
  using Index = EigenEx::Index;

  static std::string headERROR() { return detail::CallLog::headERROR(); }
  static std::string headINFO() { return detail::CallLog::headINFO(); }

  SpinMomentumCorrelationSolver& setDeviceOperator(const std::shared_ptr<device::CsrOperator>& op) {
    op_ = op;
    height_ = op ? static_cast<Index>(op->rows()) : 0;
    return *this;
  }
  SpinMomentumCorrelationSolver& setState(const DenseVector<double>& v) {
    real_ = v, complex_ = DenseVector<std::complex<double> >(), isComplex_ = false, uploaded_ = false;
    return *this;
  }
  SpinMomentumCorrelationSolver& setState(const DenseVector<std::complex<double> >& v) {
    complex_ = v, real_ = DenseVector<double>(), isComplex_ = true, uploaded_ = false;
    return *this;
  }
  Index matrixHeight() const { return height_; }
  int sites() const { return sites_; }
  int sitesUp() const { return nUp_; }
  int cell() const { return cell_; }
  int momentum() const { return momentum_; }
  double normSquared() const { return norm2_; }

  Index compute() {
    log_.begin("SpinMomentumCorrelationSolver", "compute");
    sz_.clear(), zz_.clear();
    if (!prepare_()) return 0;
    const std::size_t L = static_cast<std::size_t>(sites_);
    std::vector<std::uint64_t> masks;
    detail::appendSiteMasks(L, masks);
    detail::appendPairMasks(L, masks);
    std::vector<double> d(masks.size(), 0.0);
    // at most 1024 masks per call: 48 sites have 1176
    for (std::size_t first = 0; first < masks.size(); first += 1024) {
      const int count = static_cast<int>(masks.size() - first < 1024 ? masks.size() - first : 1024);
      device::check(eigenex_spin_momentum_measure(dev_.handle(), EIGENEX_VEC_COL(0), count, masks.data() + first, d.data() + first, &norm2_),
                    "eigenex_spin_momentum_measure");
    }
    if (!(norm2_ > 0.0) || !std::isfinite(norm2_)) return invalid_("invalid input: the state is zero (or not finite)");
    const double n = static_cast<double>(sites_ / cell_) * norm2_;
    sz_.assign(L, 0.0);
    for (std::size_t i = 0; i < L; ++i) sz_[i] = d[i] / (2.0 * n);
    zz_ = detail::pairMatrix(d.data() + L, L, 4.0 * n, 0.25);
    log_.note("sites: " + std::to_string(sites_) + ", sites up: " + std::to_string(nUp_) + ", momentum: " + std::to_string(momentum_) +
                   ", terms measured: " + std::to_string(masks.size()));
    return 0;
  }

  // ---- results (after a successful compute()) ----
  const std::vector<double>& magnetisation() const { return sz_; }
  // row-major L x L
  const std::vector<double>& correlationsZZ() const { return zz_; }
  double szsz(int i, int j) const {
    if (i < 0 || i >= sites_ || j < 0 || j >= sites_ || zz_.empty())
      throw LanczosException("SpinMomentumCorrelationSolver: no result for this pair (compute() first; sites are 0..sites()-1)");
    return zz_[static_cast<std::size_t>(i) * static_cast<std::size_t>(sites_) + static_cast<std::size_t>(j)];
  }
  double structureFactorZ(double q) const {
    double s = 0.0;
    for (int i = 0; i < sites_ && !zz_.empty(); ++i)
      for (int j = 0; j < sites_; ++j) s += std::cos(q * static_cast<double>(i - j)) * szsz(i, j);
    return sites_ > 0 ? s / static_cast<double>(sites_) : 0.0;
  }
  // <prod_{i in mask} sigma^z_i> of the state, one further measurement (bit i of mask = site i); throws on an invalid mask or state
  double stringCorrelator(std::uint64_t mask) {
    log_.succeed();
    if (!prepare_()) throw LanczosException("SpinMomentumCorrelationSolver::stringCorrelator: " + log_.log().back());
    double d = 0.0;
    device::check(eigenex_spin_momentum_measure(dev_.handle(), EIGENEX_VEC_COL(0), 1, &mask, &d, &norm2_), "eigenex_spin_momentum_measure");
    return d / (static_cast<double>(sites_ / cell_) * norm2_);
  }
  ComputationInfo info() const { return log_.info(); }
  const std::vector<std::string>& log() const { return log_.log(); }

 private:
  // the geometry of the handle and the state on the device; false (and info() = InvalidInput) if either is unusable
  bool prepare_() {
    sites_ = 0, nUp_ = 0, cell_ = 1, momentum_ = 0;
    if (!op_ || height_ <= 0 || eigenex_spin_momentum_geometry(op_->handle(), &sites_, &nUp_, &cell_, &momentum_) != 0) {
      sites_ = 0;
      invalid_("invalid input: a momentum-sector operator (device::spinHalfMomentumOperator, device::spinHalfMomentum64Operator) is required");
      return false;
    }
    const Index size = isComplex_ ? static_cast<Index>(complex_.size()) : static_cast<Index>(real_.size());
    if (size != height_) {
      invalid_("invalid input: the state must have one entry per row of the operator");
      return false;
    }
    if (!dev_.alive() || devOp_ != op_.get() || devComplex_ != isComplex_) {
      dev_.create(op_->context(), op_, height_, 1, 0, isComplex_);
      devOp_ = op_.get(), devComplex_ = isComplex_, uploaded_ = false;
    }
    if (!uploaded_) {
      if (isComplex_)
        dev_.upload(EIGENEX_VEC_COL(0), complex_);
      else
        dev_.upload(EIGENEX_VEC_COL(0), real_);
      uploaded_ = true;
    }
    return true;
  }
  Index invalid_(const std::string& what) {
    sz_.clear(), zz_.clear();
    return log_.invalid(what);
  }

  std::shared_ptr<device::CsrOperator> op_;
  const device::CsrOperator* devOp_ = nullptr;
  detail::KrylovDevice dev_;
  Index height_ = 0;
  DenseVector<double> real_;
  DenseVector<std::complex<double> > complex_;
  bool isComplex_ = false, devComplex_ = false, uploaded_ = false;
  int sites_ = 0, nUp_ = 0, cell_ = 1, momentum_ = 0;
  double norm2_ = 0.0;
  std::vector<double> sz_, zz_;
  detail::CallLog log_;
};

}  // namespace EigenEx
}  // namespace cmpt
