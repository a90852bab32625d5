// Chebyshev-filtered Lanczos: the eigenpairs of a Hermitian device operator A nearest a target energy tau INSIDE the
// spectrum, without a linear solver.
//
// NOT part of the reference (versmc/cmpt-eigenex finds the edges of the spectrum only).  Lanczos runs on p(A), where
//   p(x) = sum_k mu_k T_k((x - center)/halfwidth)
// is the Jackson-damped Chebyshev expansion of a delta peak at tau (Weisse, Wellein, Alvermann, Fehske, Rev. Mod. Phys. 78
// (2006) 275, sec. II.C), normalised to p(tau) = 1: the eigenvalues of A nearest tau are the LARGEST of p(A), an edge of its
// spectrum, which the thick-restart Lanczos cycle of thick_restart_lanczos.hpp finds (it looks for the lowest end, so it is
// given -p).  The device applies p(A) as `degree` operator applications with the three-term update in the operator kernel's
// epilogue (eigenex_basis_set_filter).  The Ritz vectors of p(A) are then rotated by a Rayleigh-Ritz step in A itself:
// X^H A X through eigenex_apply, diagonalised, X rotated; eigenvalues and residuals are those of A.
//
// [lo, hi] (setSpectralRange, required) must contain the spectrum of A, e.g. the Gershgorin bounds of
// TripletsOperator::estimateEigenvalueRange(); it is widened by 1 % before use.
#pragma once

#include <algorithm>
#include <cmath>
#include <complex>
#include <vector>

#include "thick_restart_lanczos.hpp"

namespace cmpt {
namespace EigenEx {

// g_k of the Jackson kernel for an expansion of N moments, k < N (Weisse et al., eq. 71); shared with spectral_density.hpp
inline double jacksonFactor(int k, int N) {
  const double pi = 3.14159265358979323846;
  const double q = pi / (N + 1);
  return ((N - k + 1) * std::cos(q * k) + std::sin(q * k) / std::tan(q)) / (N + 1);
}

// mu_0..mu_degree of the Jackson-damped delta peak at tau on [center - halfwidth, center + halfwidth], p(tau) = 1
inline std::vector<double> chebyshevDeltaCoefficients(double tau, double center, double halfwidth, int degree) {
  const int N = degree + 1;  // number of moments
  const double a = std::min(1.0, std::max(-1.0, (tau - center) / halfwidth));
  const double th = std::acos(a);
  std::vector<double> mu(static_cast<std::size_t>(N));
  double at_tau = 0.0, lost = 0.0;  // p(tau) before normalisation, summed with Neumaier's compensation
  for (int k = 0; k < N; ++k) {
    const double g = jacksonFactor(k, N);
    const double t = std::cos(k * th);  // T_k(a)
    mu[static_cast<std::size_t>(k)] = (k == 0 ? 1.0 : 2.0) * g * t;
    const double term = mu[static_cast<std::size_t>(k)] * t, sum = at_tau + term;
    lost += std::abs(at_tau) >= std::abs(term) ? (at_tau - sum) + term : (term - sum) + at_tau;
    at_tau = sum;
  }
  at_tau += lost;
  for (double& m : mu) m /= at_tau;
  return mu;
}

template <class Scalar_>
class FilteredLanczosEigenSolver : public ThickRestartLanczosEigenSolver<Scalar_> {
  using Base = ThickRestartLanczosEigenSolver<Scalar_>;

 public:
  using Index = typename Base::Index;
  using Scalar = Scalar_;
  using RealScalar = typename Base::RealScalar;
  using MatrixType = typename Base::MatrixType;

  FilteredLanczosEigenSolver& setTarget(RealScalar tau) {
    tau_ = tau;
    return *this;
  }
  FilteredLanczosEigenSolver& setSpectralRange(RealScalar lo, RealScalar hi) {
    lo_ = lo;
    hi_ = hi;
    return *this;
  }
  FilteredLanczosEigenSolver& setFilterDegree(Index d) {
    degree_ = d;
    return *this;
  }
  RealScalar target() const { return tau_; }
  Index filterDegree() const { return degree_; }
  // eigenvalues(): of A, sorted by |lambda - tau| ascending; residuals(): ||A x - lambda x||; operatorApplications():
  // applications of A (degree per Lanczos step, plus the Rayleigh-Ritz step and the residuals)

  Index compute() {
    const double lo = static_cast<double>(lo_), hi = static_cast<double>(hi_), tau = static_cast<double>(tau_);
    if (!(hi > lo) || !(tau >= lo && tau <= hi) || degree_ < 1 || degree_ > (Index(1) << 20) || !this->op_ || this->shift_ != RealScalar(0)) {
      this->log_.clear();
      this->log_.push_back(Base::headINFO() + "FilteredLanczosEigenSolver::compute(...) was called");
      this->log_.push_back(Base::headERROR() +
                           "invalid input: setSpectralRange(lo, hi) with lo <= target <= hi, a filter degree >= 1, a device operator and no eigenvalue shift are required");
      this->eigenvalues_.resize(0);
      this->eigenvectors_.resize(0, 0);
      this->residuals_.resize(0);
      this->restarts_ = this->matvecs_ = 0;
      this->info_ = InvalidInput;
      return 0;
    }
    center_ = 0.5 * (lo + hi);
    half_ = 0.5 * (hi - lo) * 1.01;
    negmu_ = chebyshevDeltaCoefficients(tau, center_, half_, static_cast<int>(degree_));
    for (double& m : negmu_) m = -m;  // the cycle looks for the lowest end
    struct Restore {  // the Ritz vectors of p(A) are needed whatever the caller wants returned; put back on every way out
      bool& flag;
      bool value;
      ~Restore() { flag = value; }
    } wanted{this->vectorsOn_, this->vectorsOn_};
    this->vectorsOn_ = true;
    Base::compute();
    if (this->dev_.alive()) device::check(eigenex_basis_set_filter(this->dev_.handle(), 0, nullptr, 0.0, 1.0), "eigenex_basis_set_filter");
    this->matvecs_ *= degree_;
    if (this->info_ == InvalidInput || this->info_ == NumericalIssue || this->eigenvalues_.size() == 0) return 0;
    rayleighRitz_();
    if (!wanted.value) this->eigenvectors_.resize(0, 0);
    return 0;
  }

 protected:
  void stateReady_() override {
    device::check(eigenex_basis_set_filter(this->dev_.handle(), static_cast<int>(degree_), negmu_.data(), center_, half_), "eigenex_basis_set_filter");
  }

  void uploadColumns_(Index nw) {
    for (Index i = 0; i < nw; ++i) this->dev_.upload(EIGENEX_VEC_COL(i), this->eigenvectors_.col(i));
  }

  // X = the nw Ritz vectors of p(A) (orthonormal): G = X^H A X, G = S diag(lambda) S^H, X <- X S; then the true residuals
  void rayleighRitz_() {
    constexpr bool cplx = detail::IsComplex<Scalar>::value;
    constexpr int es = cplx ? 2 : 1;
    const Index nw = this->eigenvalues_.size();
    const int n = static_cast<int>(nw);
    eigenex_basis_t h = this->dev_.handle();
    uploadColumns_(nw);
    std::vector<double> G(static_cast<std::size_t>(es) * n * n);  // column j = X^H (A x_j)
    for (int j = 0; j < n; ++j) {
      device::check(eigenex_apply(h, EIGENEX_VEC_COL(j), EIGENEX_VEC_V, 0.0, nullptr), "eigenex_apply");
      device::check(eigenex_dots(h, EIGENEX_VEC_V, 0, 1, n, 0, G.data() + static_cast<std::size_t>(es) * n * j), "eigenex_dots");
    }
    auto g = [&](int r, int c) { return std::complex<double>(G[static_cast<std::size_t>(es) * (r + c * n)], cplx ? G[static_cast<std::size_t>(es) * (r + c * n) + 1] : 0.0); };
    // Hermitian part, as the real symmetric matrix [[Re, -Im], [Im, Re]] for complex scalars: every eigenvalue twice, the
    // eigenvectors (x_re; x_im); one vector per complex direction is kept
    const int nn = cplx ? 2 * n : n;
    std::vector<double> M(static_cast<std::size_t>(nn) * nn), vals, vecs;
    for (int c = 0; c < n; ++c)
      for (int r = 0; r < n; ++r) {
        const std::complex<double> z = 0.5 * (g(r, c) + std::conj(g(c, r)));
        M[static_cast<std::size_t>(r + c * nn)] = z.real();
        if (cplx) {
          M[static_cast<std::size_t>(r + n + (c + n) * nn)] = z.real();
          M[static_cast<std::size_t>(r + n + c * nn)] = z.imag();
          M[static_cast<std::size_t>(r + (c + n) * nn)] = -z.imag();
        }
      }
    small_eigen::symmetric(M, nn, vals, vecs);
    std::vector<std::vector<std::complex<double>>> S;
    std::vector<double> lambda;
    for (int k = 0; k < nn && static_cast<int>(S.size()) < n; ++k) {
      std::vector<std::complex<double>> z(static_cast<std::size_t>(n));
      for (int r = 0; r < n; ++r) z[static_cast<std::size_t>(r)] = std::complex<double>(vecs[static_cast<std::size_t>(r + k * nn)], cplx ? vecs[static_cast<std::size_t>(r + n + k * nn)] : 0.0);
      for (const auto& s : S) {
        std::complex<double> d = 0.0;
        for (int r = 0; r < n; ++r) d += std::conj(s[static_cast<std::size_t>(r)]) * z[static_cast<std::size_t>(r)];
        for (int r = 0; r < n; ++r) z[static_cast<std::size_t>(r)] -= d * s[static_cast<std::size_t>(r)];
      }
      double nrm = 0.0;
      for (const auto& x : z) nrm += std::norm(x);
      nrm = std::sqrt(nrm);
      if (nrm < 0.5) continue;  // the second copy of a direction already taken
      for (auto& x : z) x /= nrm;
      S.push_back(z);
      lambda.push_back(vals[static_cast<std::size_t>(k)]);
    }
    const int got = static_cast<int>(S.size());
    std::vector<int> order(static_cast<std::size_t>(got));
    for (int i = 0; i < got; ++i) order[static_cast<std::size_t>(i)] = i;
    const double tau = static_cast<double>(tau_);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return std::abs(lambda[static_cast<std::size_t>(x)] - tau) < std::abs(lambda[static_cast<std::size_t>(y)] - tau); });
    std::vector<double> Sre(static_cast<std::size_t>(n) * got), Sim(static_cast<std::size_t>(n) * got);
    this->eigenvalues_.resize(got);
    for (int e = 0; e < got; ++e) {
      const int k = order[static_cast<std::size_t>(e)];
      this->eigenvalues_[e] = static_cast<RealScalar>(lambda[static_cast<std::size_t>(k)]);
      for (int r = 0; r < n; ++r) {
        Sre[static_cast<std::size_t>(r + e * n)] = S[static_cast<std::size_t>(k)][static_cast<std::size_t>(r)].real();
        Sim[static_cast<std::size_t>(r + e * n)] = S[static_cast<std::size_t>(k)][static_cast<std::size_t>(r)].imag();
      }
    }
    // X S from the columns that hold X, normalised and phase-fixed like every other solver's vectors
    MatrixType X(this->dev_.localRows(), got);
    {
      detail::WideOut<Scalar> out(X.data(), X.size());
      if (cplx)
        device::check(eigenex_ritz_vectors_complex(h, n, got, Sre.data(), Sim.data(), n, out.data(), X.rows()), "eigenex_ritz_vectors_complex");
      else
        device::check(eigenex_ritz_vectors(h, n, got, Sre.data(), n, out.data(), X.rows()), "eigenex_ritz_vectors");
    }
    this->eigenvectors_ = X;
    // true residuals ||A x - lambda x||
    uploadColumns_(got);
    this->residuals_.resize(got);
    for (int j = 0; j < got; ++j) {
      double nrm2 = 0.0;
      device::check(eigenex_apply(h, EIGENEX_VEC_COL(j), EIGENEX_VEC_V, 0.0, nullptr), "eigenex_apply");
      device::check(eigenex_axpy2(h, EIGENEX_VEC_W, EIGENEX_VEC_V, static_cast<double>(this->eigenvalues_[j]), EIGENEX_VEC_COL(j), 0.0, EIGENEX_VEC_COL(j)), "eigenex_axpy2");
      device::check(eigenex_update(h, EIGENEX_VEC_W, 0, 1, 0, 0, nullptr, &nrm2), "eigenex_update");
      this->residuals_[j] = static_cast<RealScalar>(std::sqrt(std::max(nrm2, 0.0)));
    }
    this->matvecs_ += nw + got;
  }

  RealScalar tau_ = 0, lo_ = 0, hi_ = 0;
  Index degree_ = 200;
  double center_ = 0.0, half_ = 1.0;
  std::vector<double> negmu_;
};

}  // namespace EigenEx
}  // namespace cmpt
