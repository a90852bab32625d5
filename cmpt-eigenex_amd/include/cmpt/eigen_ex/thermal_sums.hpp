// Host arithmetic of the finite-temperature Lanczos method (Jaklic and Prelovsek, Phys. Rev. B 49, 5065 (1994); Adv. Phys. 49, 1
// (2000)): thermodynamic sums over the Ritz values of R Lanczos runs from random vectors.  No device code, no other header of
// this library: thermal_lanczos.hpp fills it, tests/cpp/thermal_sums_test.cpp runs it alone.
//
// A run from the normalised vector |r> with M steps gives the tridiagonal matrix T = S diag(theta) S^T.  Its sample is
//   theta_j               the Ritz values
//   w_j = S_1j^2          the weight |<r|psi_j>|^2 of Ritz vector j in |r>; sum_j w_j = 1
//   a_tj = S_1j sum_i S_ij g_ti    per observable t, with g_ti = <v_i| A_t |v_0>: a_tj = <r|psi_j><psi_j| A_t |r>
// With N the dimension of the space and R samples,
//   Z(beta)    = (N / R) sum_r sum_j w_j exp(-beta theta_j)
//   <H^k>      = (N / (R Z)) sum_r sum_j w_j theta_j^k exp(-beta theta_j)
//   <A_t>      = (N / (R Z)) sum_r sum_j a_tj exp(-beta theta_j)
//   E = <H>,  C = beta^2 (<H^2> - <H>^2),  F = -log Z / beta,  S = beta (E - F) = beta E + log Z
// The estimate is exact at beta = 0 for H^k with k <= M in expectation over the random vectors, and exact altogether when the
// vectors are an orthonormal basis and every run ends in a breakdown (the trace is then complete).  Every sum is taken
// relative to E_ref = min theta over the samples it runs over: each exponent is <= 0 and the largest is exactly 0, so nothing
// overflows and the sum cannot underflow to zero, whatever beta (theta_max - theta_min) is.
//
// standardError is the delete-one jackknife over the samples: the quantity recomputed R times, each time without one sample,
// err^2 = (R - 1) / R sum_i (f_(i) - mean_i f_(i))^2.  It measures the scatter between the random vectors for the ratio as a
// whole (numerator and Z are correlated, which the jackknife respects).  It does not cover the truncation at M steps, and at low
// temperature with few vectors it underestimates: there a few vectors with a large overlap with the ground state carry the sums,
// and R such samples say little about the distribution they come from.  With fewer than two samples it is NaN.
#pragma once

#include <cmath>
#include <cstddef>
#include <limits>
#include <stdexcept>
#include <utility>
#include <vector>

namespace cmpt {
namespace EigenEx {

struct ThermalSample {
  std::vector<double> theta, weight;     // M' entries each, M' <= M the steps the run took
  std::vector<std::vector<double>> a;    // a[t][j], one row of M' entries per observable
};

enum class ThermalQuantity { LogPartitionFunction, Energy, SpecificHeat, Entropy, FreeEnergy, Observable };

class ThermalSums {
 public:
  ThermalSums() : dimension_(0.0), observables_(0) {}

  void clear() {
    samples_.clear();
    dimension_ = 0.0, observables_ = 0;
  }
  // N, the number of states the random vectors live in
  void setDimension(double N) { dimension_ = N; }
  double dimension() const { return dimension_; }
  std::size_t samples() const { return samples_.size(); }
  std::size_t observables() const { return observables_; }
  const ThermalSample& sample(std::size_t r) const { return samples_.at(r); }

  void addSample(ThermalSample s) {
    if (s.theta.empty() || s.theta.size() != s.weight.size()) throw std::invalid_argument("ThermalSums: a sample needs as many weights as Ritz values, at least one");
    if (!samples_.empty() && s.a.size() != observables_) throw std::invalid_argument("ThermalSums: every sample must hold the same observables");
    for (const auto& row : s.a)
      if (row.size() != s.theta.size()) throw std::invalid_argument("ThermalSums: an observable needs one entry per Ritz value");
    observables_ = s.a.size();
    samples_.push_back(std::move(s));
  }

  // the smallest Ritz value of all samples
  double referenceEnergy() const { return reference_(samples_.size()); }

  double logPartitionFunction(double beta) const { return value(ThermalQuantity::LogPartitionFunction, beta); }
  double energy(double beta) const { return value(ThermalQuantity::Energy, beta); }
  double specificHeat(double beta) const { return value(ThermalQuantity::SpecificHeat, beta); }
  double entropy(double beta) const { return value(ThermalQuantity::Entropy, beta); }
  double freeEnergy(double beta) const { return value(ThermalQuantity::FreeEnergy, beta); }
  double observable(std::size_t t, double beta) const { return value(ThermalQuantity::Observable, beta, t); }

  double value(ThermalQuantity q, double beta, std::size_t t = 0) const { return evaluate_(q, beta, t, samples_.size()); }

  double standardError(ThermalQuantity q, double beta, std::size_t t = 0) const {
    const std::size_t R = samples_.size();
    if (R < 2) return std::numeric_limits<double>::quiet_NaN();
    std::vector<double> f(R);
    double mean = 0.0;
    for (std::size_t i = 0; i < R; ++i) mean += (f[i] = evaluate_(q, beta, t, i));
    mean /= static_cast<double>(R);
    double s = 0.0;
    for (std::size_t i = 0; i < R; ++i) s += (f[i] - mean) * (f[i] - mean);
    return std::sqrt(s * static_cast<double>(R - 1) / static_cast<double>(R));
  }

  // what ThermalEnsemble adds up over sectors: log Z, <H> and <H^2> - <H>^2 of this set of samples
  void moments(double beta, double* logZ, double* mean, double* variance) const {
    if (logZ) *logZ = logPartitionFunction(beta);
    if (mean) *mean = energy(beta);
    if (variance) *variance = beta != 0.0 ? specificHeat(beta) / (beta * beta) : variance0_();
  }

 private:
  // <H^2> - <H>^2 at beta = 0, where C = beta^2 (...) no longer holds it
  double variance0_() const {
    double m0 = 0.0, m1 = 0.0, var = 0.0;
    const double e0 = reference_(samples_.size());
    for (const ThermalSample& s : samples_)
      for (std::size_t j = 0; j < s.theta.size(); ++j) m0 += s.weight[j], m1 += s.weight[j] * (s.theta[j] - e0);
    for (const ThermalSample& s : samples_)
      for (std::size_t j = 0; j < s.theta.size(); ++j) var += s.weight[j] * (s.theta[j] - e0 - m1 / m0) * (s.theta[j] - e0 - m1 / m0);
    return var / m0;
  }

  double reference_(std::size_t skip) const {
    double e = std::numeric_limits<double>::infinity();
    for (std::size_t r = 0; r < samples_.size(); ++r)
      if (r != skip)
        for (double th : samples_[r].theta) e = th < e ? th : e;
    return e;
  }

  // over every sample but `skip` (skip = samples(): over all)
  double evaluate_(ThermalQuantity q, double beta, std::size_t t, std::size_t skip) const {
    const std::size_t used = samples_.size() - (skip < samples_.size() ? 1 : 0);
    if (used == 0) throw std::logic_error("ThermalSums: no sample");
    if (q == ThermalQuantity::Observable && t >= observables_) throw std::out_of_range("ThermalSums: no such observable");
    const double e0 = reference_(skip);
    double m0 = 0.0, m1 = 0.0, at = 0.0;  // sums of w, w (theta - e0) and a_t, each times exp(-beta (theta - e0))
    for (std::size_t r = 0; r < samples_.size(); ++r) {
      if (r == skip) continue;
      const ThermalSample& s = samples_[r];
      for (std::size_t j = 0; j < s.theta.size(); ++j) {
        const double d = s.theta[j] - e0, b = std::exp(-beta * d);
        m0 += s.weight[j] * b;
        m1 += s.weight[j] * d * b;
        if (q == ThermalQuantity::Observable) at += s.a[t][j] * b;
      }
    }
    const double logz = std::log(dimension_ / static_cast<double>(used)) + std::log(m0) - beta * e0;
    const double mean = m1 / m0;  // <H> - e0
    switch (q) {
      case ThermalQuantity::LogPartitionFunction: return logz;
      case ThermalQuantity::Energy: return e0 + mean;
      case ThermalQuantity::FreeEnergy: return -logz / beta;
      case ThermalQuantity::Entropy: return beta * (e0 + mean) + logz;
      case ThermalQuantity::Observable: return at / m0;
      case ThermalQuantity::SpecificHeat: break;
    }
    double var = 0.0;  // the variance about the mean, in a second pass: no difference of two large moments
    for (std::size_t r = 0; r < samples_.size(); ++r) {
      if (r == skip) continue;
      const ThermalSample& s = samples_[r];
      for (std::size_t j = 0; j < s.theta.size(); ++j) {
        const double d = s.theta[j] - e0;
        var += s.weight[j] * (d - mean) * (d - mean) * std::exp(-beta * d);
      }
    }
    return beta * beta * var / m0;
  }

  double dimension_;
  std::size_t observables_;
  std::vector<ThermalSample> samples_;
};

}  // namespace EigenEx
}  // namespace cmpt
