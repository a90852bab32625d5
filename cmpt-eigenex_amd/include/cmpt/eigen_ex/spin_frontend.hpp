// What the spin front-end classes (SpinDynamicsSolver, SpinTimeEvolutionSolver, SpinTimeCorrelationSolver, SpinEntanglementSolver,
// SpinCorrelationSolver, SpinMomentumCorrelationSolver) share, written once.  The sub-step loop of the two evolving classes is
// detail::advanceInSubSteps, beside the sub-step it repeats (spin_evolution.hpp).
// NOT part of the reference.  Like every public header it calls the C ABI only (eigenex_hip.h).
#pragma once

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdint>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "lanczos.hpp"
#include "small_eigen.hpp"
#include "spin_operator.hpp"

namespace cmpt {
namespace EigenEx {
namespace detail {

// The log and info() of one call of a front-end class: begin() clears both, the refusals and failures append an ERROR line.
class CallLog {
 public:
  static std::string headERROR() { return std::string("ERROR     "); }
  static std::string headINFO() { return std::string("INFO      "); }

  void begin(const char* className, const char* who) {
    lines_.clear();
    note(std::string(className) + "::" + who + "(...) was called");
    info_ = Success;
  }
  void note(const std::string& what) { lines_.push_back(headINFO() + what); }
  Index invalid(const std::string& what) { return failed(what, InvalidInput); }
  Index failed(const std::string& what, ComputationInfo info = NumericalIssue) {
    lines_.push_back(headERROR() + what);
    info_ = info;
    return 0;
  }
  void succeed() { info_ = Success; }  // a further call on the results of the last one: its log stays
  ComputationInfo info() const { return info_; }
  const std::vector<std::string>& log() const { return lines_; }

 private:
  ComputationInfo info_ = Success;
  std::vector<std::string> lines_;
};

inline int popcount(std::uint32_t bits) {
  int c = 0;
  for (; bits; bits &= bits - 1) ++c;
  return c;
}
// bit i for every site i of the list; valid becomes false for a site outside 0..31 or named twice
inline std::uint32_t siteMask(const std::vector<int>& sites, bool& valid) {
  std::uint32_t mask = 0;
  for (int i : sites) {
    if (i < 0 || i > 31 || ((mask >> i) & 1u)) valid = false;
    else mask |= std::uint32_t(1) << i;
  }
  return mask;
}
// the sector a site operator of `kind` takes the sector nUp to (nUp = -1, the full space, stays).  A copy of the library's
// spin_site_dst_up on purpose: the public headers see the C ABI, not csrc/.
inline int dstUp(int nUp, int kind) { return nUp < 0 || kind == EIGENEX_SPIN_SITE_Z ? nUp : (kind == EIGENEX_SPIN_SITE_PLUS ? nUp + 1 : nUp - 1); }

// The row of the basis state with site i up where bit i of `bits` is set, among the `rows` rows of the full space (nUp = -1: the
// state itself) or of the sector of nUp sites up (the library's own ordering, eigenex_spin_sector_states: the states ascending,
// searched by bisection).  -1 and the refusal in `why` if the state is not there.
inline Index productStateRow(int sites, int nUp, Index rows, std::uint32_t bits, std::string& why) {
  if (sites < 32 && (bits >> sites) != 0u) return why = "invalid input: the product state names a site outside 0..sites-1", -1;
  if (nUp < 0) return static_cast<Index>(bits);
  if (popcount(bits) != nUp) return why = "invalid input: the product state does not lie in the sector (its number of up sites differs)", -1;
  Index lo = 0, hi = rows - 1;
  while (lo <= hi) {
    const Index mid = lo + (hi - lo) / 2;
    std::uint32_t s = 0;
    device::check(eigenex_spin_sector_states(sites, nUp, mid, 1, &s), "eigenex_spin_sector_states");
    if (s == bits) return mid;
    if (s < bits)
      lo = mid + 1;
    else
      hi = mid - 1;
  }
  return why = "invalid input: the product state was not found among the sector's states", -1;
}

// v / |v| and the norm; an empty vector and the refusal in `why` unless v has `rows` entries and a finite norm above zero
inline DenseVector<std::complex<double>> normalised(const DenseVector<std::complex<double>>& v, Index rows, double& norm, std::string& why) {
  typedef DenseVector<std::complex<double>> Vector;
  if (v.size() != rows) return why = "invalid input: the state must have one entry per row of the model's space or sector", Vector();
  norm = v.norm();
  if (!(norm > 0.0) || !std::isfinite(norm)) return why = "invalid input: the state is zero (or not finite)", Vector();
  Vector u(rows);
  for (Index r = 0; r < rows; ++r) u[r] = v[r] / norm;
  return u;
}

// The operator of the sector a state lives in (the caller builds src) and the one a site operator takes it to.  `make(up)`
// builds an operator; `release()` destroys the state that lives on the destination, which goes before its operator.
struct SectorPair {
  std::shared_ptr<device::CsrOperator> src, dst;

  void reset() { src.reset(), dst.reset(); }
  // whether destination(nUp, up, ...) keeps dst as it is: it is the source and is wanted again, or was built for `up`
  bool keeps(int nUp, int up) const { return up == nUp ? dst == src : (dst && dst != src && dstUp_ == up); }
  template <class Make, class Release>
  void destination(int nUp, int up, Make make, Release release) {
    if (!keeps(nUp, up)) {
      const std::shared_ptr<device::CsrOperator> fresh = up == nUp ? src : make(up);
      release();
      dst = fresh;
    }
    dstUp_ = up;
  }

 private:
  int dstUp_ = -2;
};

// the refusal of a coefficient list of `whose` operator (im: the imaginary parts, or null) that is not one finite number per site
inline std::string checkCoefficients(const std::vector<double>& re, const std::vector<double>* im, int sites, const char* whose) {
  if (static_cast<int>(re.size()) != sites || (im && im->size() != re.size())) return std::string("invalid input: ") + whose + " needs one coefficient per site";
  for (std::size_t i = 0; i < re.size(); ++i)
    if (!std::isfinite(re[i]) || (im && !std::isfinite((*im)[i]))) return std::string("invalid input: a coefficient of ") + whose + " is not finite";
  return std::string();
}

// O x of a sum of site operators O (a kind, one coefficient per site) and what became of it
struct SiteApplication {
  enum Outcome { NotFinite, ExactZero, RoundingZero, Unit } outcome;
  double norm2;  // |O x|^2
  bool zero() const { return outcome == ExactZero || outcome == RoundingZero; }
  // "O|v> = 0: this part of the response is identically zero" and its like, from the names of the vector and of the response
  std::string zeroNote(const char* vector, const char* response) const {
    return std::string(vector) + (outcome == ExactZero ? " = 0" : " vanishes within the rounding of its application") + ": " + response + " is identically zero";
  }
};
// y = O x from vector xRef of `src` into the work vector W of `dst` (eigenex_spin_site_apply, or _z for a complex run, where im may
// be null), x of squared norm xNorm2.  |y_r| <= L eps sum_i |c_i| |x| is what the roundings of the application alone can leave of
// an exact zero (Z: half of it; a complex coefficient counts |Re| + |Im|, which bounds what each part of a row sums): a y no
// larger is a zero, and W is left as it is.  Otherwise W is scaled to unit length -- through V, the scaling kernel is not an
// in-place one --, whatever the scale of the coefficients: the breakdown threshold of a Lanczos run is an absolute number.
// what became of y = O x in W of `dst`, |y|^2 in out.norm2, csum the sum of the moduli of the site coefficients: the zero rule
// and the scaling to unit length
inline SiteApplication unitOrZero(eigenex_basis_t dst, SiteApplication out, int kind, int sites, double csum, double xNorm2) {
  if (!std::isfinite(out.norm2)) return out.outcome = SiteApplication::NotFinite, out;
  const double noise = static_cast<double>(sites) * std::ldexp(1.0, -52) * csum * (kind == EIGENEX_SPIN_SITE_Z ? 0.5 : 1.0);
  if (out.norm2 <= noise * noise * xNorm2) return out.outcome = out.norm2 == 0.0 ? SiteApplication::ExactZero : SiteApplication::RoundingZero, out;
  device::check(eigenex_scale(dst, EIGENEX_VEC_V, EIGENEX_VEC_W, 1.0 / std::sqrt(out.norm2)), "eigenex_scale");
  device::check(eigenex_vec_copy(dst, EIGENEX_VEC_W, EIGENEX_VEC_V), "eigenex_vec_copy");
  return out;
}
inline SiteApplication applySiteOperatorToUnit(eigenex_basis_t src, int xRef, eigenex_basis_t dst, bool complexRun, int kind, int sites,
                                               const std::vector<double>& re, const std::vector<double>* im, double xNorm2) {
  SiteApplication out = {SiteApplication::Unit, 0.0};
  if (complexRun)
    device::check(eigenex_spin_site_apply_z(src, xRef, dst, EIGENEX_VEC_W, kind, re.data(), im ? im->data() : nullptr, &out.norm2), "eigenex_spin_site_apply_z");
  else
    device::check(eigenex_spin_site_apply(src, xRef, dst, EIGENEX_VEC_W, kind, re.data(), &out.norm2), "eigenex_spin_site_apply");
  double csum = 0.0;
  for (double c : re) csum += std::fabs(c);
  if (im)
    for (double c : *im) csum += std::fabs(c);
  return unitOrZero(dst, out, kind, sites, csum, xNorm2);
}

// The same between two momentum sectors (eigenex_spin_momentum_site_apply, or _z for a complex run): the operator is a kind, `cell`
// cell coefficients and the momentum index p (eigenex_hip.h), its site coefficients have the moduli of the cell's, once per
// translation, so the sum of their moduli is (sites / cell) times the cell's.
inline SiteApplication applyMomentumSiteOperatorToUnit(eigenex_basis_t src, int xRef, eigenex_basis_t dst, bool complexRun, int kind, int p, int sites,
                                                       const std::vector<double>& cellRe, const std::vector<double>& cellIm, double xNorm2) {
  SiteApplication out = {SiteApplication::Unit, 0.0};
  if (complexRun)
    device::check(eigenex_spin_momentum_site_apply_z(src, xRef, dst, EIGENEX_VEC_W, kind, p, cellRe.data(), cellIm.data(), &out.norm2),
                  "eigenex_spin_momentum_site_apply_z");
  else
    device::check(eigenex_spin_momentum_site_apply(src, xRef, dst, EIGENEX_VEC_W, kind, p, cellRe.data(), &out.norm2), "eigenex_spin_momentum_site_apply");
  double csum = 0.0;
  for (double c : cellRe) csum += std::fabs(c);
  for (double c : cellIm) csum += std::fabs(c);
  return unitOrZero(dst, out, kind, sites, csum * static_cast<double>(sites / static_cast<int>(cellRe.size())), xNorm2);
}

// What follows the start vector of a continued fraction, for every class that runs one (SpinDynamicsSolver,
// SpinMomentumDynamicsSolver): the unit vector phi / |phi| is in the work vector of `dst`, a state of capacity m + 1 on the
// destination operator; m Lanczos steps in the library's default scheme, T = S diag(theta) S^T (small_eigen.hpp), and the poles
// theta_n - E0 with the weights |phi|^2 / <v|v> S(0, n)^2 appended to what earlier parts of the response found.
class ContinuedFraction {
 public:
  void clear() { found_.clear(), alpha_.clear(), beta_.clear(), parts_ = 0.0; }
  // one part: norm2 = |phi|^2 before it was scaled, vv = <v|v>
  void run(eigenex_basis_t dst, Index m, double norm2, double vv, double E0, CallLog& log) {
    device::check(eigenex_lanczos_enqueue(dst, static_cast<int>(m)), "eigenex_lanczos_enqueue");
    eigenex_state_t st;
    alpha_.assign(static_cast<std::size_t>(m) + 4, 0.0), beta_.assign(static_cast<std::size_t>(m) + 4, 0.0);
    device::check(eigenex_lanczos_state(dst, &st, alpha_.data(), beta_.data()), "eigenex_lanczos_state");
    const int k = std::min<int>(st.nalpha, static_cast<int>(m));  // a breakdown leaves fewer: the fraction ends there
    if (k < 1) {
      log.failed("the start vector O|v> failed the breakdown threshold of the Lanczos run");
      alpha_.clear(), beta_.clear();
      return;
    }
    alpha_.resize(static_cast<std::size_t>(k)), beta_.resize(static_cast<std::size_t>(k - 1));
    std::vector<double> theta, S;
    if (!small_eigen::tridiagonal(alpha_.data(), beta_.data(), k, theta, &S)) return void(log.failed("the tridiagonal eigenproblem did not converge"));
    for (int j = 0; j < k; ++j) {
      const double s0 = S[static_cast<std::size_t>(j) * static_cast<std::size_t>(k)];  // row 0 of column j
      found_.push_back(std::make_pair(theta[static_cast<std::size_t>(j)] - E0, norm2 / vv * s0 * s0));
    }
    parts_ += norm2 / vv;
    log.note("lanczos steps: " + std::to_string(k) + (st.stopped ? " (breakdown: the fraction is complete)" : "") +
             ", <O^dagger O> of this part: " + std::to_string(norm2 / vv));
  }
  // the parts merged into ascending poles, if the call succeeded; what was found is dropped either way
  void finish(bool success, std::vector<double>& poles, std::vector<double>& weights, double& total) {
    if (success) {
      std::stable_sort(found_.begin(), found_.end(), [](const std::pair<double, double>& a, const std::pair<double, double>& b) { return a.first < b.first; });
      for (const auto& pw : found_) poles.push_back(pw.first), weights.push_back(pw.second);
      total = parts_;
    }
    found_.clear();
    parts_ = 0.0;
  }
  // the coefficients of the last run
  const std::vector<double>& alpha() const { return alpha_; }
  const std::vector<double>& beta() const { return beta_; }

 private:
  std::vector<std::pair<double, double>> found_;
  double parts_ = 0.0;
  std::vector<double> alpha_, beta_;
};

// The masks of the sites, and of the pairs i < j with i ascending and j ascending within i, appended to `masks`
template <class Word>
inline void appendSiteMasks(std::size_t L, std::vector<Word>& masks) {
  for (std::size_t i = 0; i < L; ++i) masks.push_back(Word(1) << i);
}
template <class Word>
inline void appendPairMasks(std::size_t L, std::vector<Word>& masks) {
  for (std::size_t i = 0; i < L; ++i)
    for (std::size_t j = i + 1; j < L; ++j) masks.push_back((Word(1) << i) | (Word(1) << j));
}
// the sums of the pair masks, raw[0 .. L (L - 1) / 2), as the symmetric L x L matrix raw / divisor with `diagonal` on its diagonal
inline std::vector<double> pairMatrix(const double* raw, std::size_t L, double divisor, double diagonal) {
  std::vector<double> out(L * L, 0.0);
  std::size_t k = 0;
  for (std::size_t i = 0; i < L; ++i) {
    out[i * L + i] = diagonal;
    for (std::size_t j = i + 1; j < L; ++j, ++k) out[i * L + j] = out[j * L + i] = raw[k] / divisor;
  }
  return out;
}

}  // namespace detail
}  // namespace EigenEx
}  // namespace cmpt
