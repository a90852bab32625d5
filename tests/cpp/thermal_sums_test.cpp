// include/cmpt/eigen_ex/thermal_sums.hpp alone, in a stand-alone host program (no device, no library): a two-level system and a
// truncated harmonic ladder against their closed forms (evaluated in long double) within 50 eps relative, observables, sums
// that stay finite at beta (theta_max - theta_min) = 1e4, the jackknife error (zero for identical samples, the textbook
// value for a linear quantity) and the refusals.  Built with -fsanitize=address,undefined and run by
// tests/test_thermal_sums_host.py; prints THERMAL SUMS OK and exits 0 when every check holds.
#include <cmath>
#include <cstdio>
#include <limits>
#include <stdexcept>
#include <vector>

#include "cmpt/eigen_ex/thermal_sums.hpp"

using cmpt::EigenEx::ThermalQuantity;
using cmpt::EigenEx::ThermalSample;
using cmpt::EigenEx::ThermalSums;

static int fails = 0;
#define EXPECT(c)                                                        \
  do {                                                                   \
    if (!(c)) {                                                          \
      std::fprintf(stderr, "FAILED %s:%d %s\n", __FILE__, __LINE__, #c); \
      ++fails;                                                           \
    }                                                                    \
  } while (0)

static const double kEps = std::numeric_limits<double>::epsilon();
static double worst = 0.0;

// within 50 eps relative; `scale` > 1 widens the bound for a quantity whose error is absolute (see log Z below)
static bool close(double got, long double want, long double scale = 1) {
  const long double err = std::fabs(static_cast<long double>(got) - want), bound = 50 * kEps * std::fabs(want) * scale;
  if (bound > 0 && static_cast<double>(err / bound) > worst) worst = static_cast<double>(err / bound);
  if (err > bound) std::fprintf(stderr, "  got %.17g, closed form %.17Lg, error %.3Lg > %.3Lg\n", got, want, err, bound);
  return err <= bound;
}

// K equidistant levels 0, w, .., (K - 1) w, each once: one sample with the weights 1 / K in a space of K states.  K = 2 is the
// two-level system.  `copies` identical samples leave every quantity as it is.
static ThermalSums ladder(int K, double w, int copies) {
  ThermalSums s;
  s.setDimension(K);
  for (int c = 0; c < copies; ++c) {
    ThermalSample a;
    for (int j = 0; j < K; ++j) a.theta.push_back(j * w), a.weight.push_back(1.0 / K);
    a.a.push_back(a.theta);  // observable 0 is H itself: a_j = w_j theta_j
    for (int j = 0; j < K; ++j) a.a[0][j] = a.theta[j] * a.weight[j];
    s.addSample(a);
  }
  return s;
}

static void check_ladder(int K, double w, double beta, int copies) {
  const ThermalSums s = ladder(K, w, copies);
  typedef long double LD;
  const LD x = static_cast<LD>(beta) * static_cast<LD>(w), q = std::exp(-x), qK = std::exp(-x * K);
  // Z = (1 - q^K) / (1 - q); n(x) = 1 / (e^x - 1); E = w (n(x) - K n(K x)); C = x^2 (e^x n(x)^2 - K^2 e^(K x) n(K x)^2)
  const LD Z = -std::expm1(-x * K) / -std::expm1(-x);
  const LD n1 = 1 / std::expm1(x), nK = 1 / std::expm1(x * K);
  const LD E = static_cast<LD>(w) * (n1 - K * nK);
  const LD C = x * x * (n1 * n1 / q - static_cast<LD>(K) * K * nK * nK / qK);
  const LD S = std::log(Z) + static_cast<LD>(beta) * E;
  // log Z is the logarithm of a rounded Z: its error is a relative error of Z, so absolute where |log Z| < 1 (Z near 1); F likewise
  const LD logscale = std::fabs(std::log(Z)) > 1 ? 1 : 1 / std::fabs(std::log(Z));
  EXPECT(close(s.logPartitionFunction(beta), std::log(Z), logscale));
  EXPECT(close(std::exp(s.logPartitionFunction(beta)), Z));
  EXPECT(close(s.energy(beta), E));
  EXPECT(close(s.specificHeat(beta), C));
  EXPECT(close(s.entropy(beta), S));
  EXPECT(close(s.freeEnergy(beta), -std::log(Z) / static_cast<LD>(beta), logscale));
  EXPECT(close(s.observable(0, beta), E));  // a_j = w_j theta_j: the observable is H
  EXPECT(s.referenceEnergy() == 0.0 && s.samples() == static_cast<std::size_t>(copies) && s.observables() == 1);
  if (copies == 1) EXPECT(std::isnan(s.standardError(ThermalQuantity::Energy, beta)));
  if (copies == 2 || copies == 4) {  // the mean of 2 or 4 equal numbers is that number: exactly zero
    const ThermalQuantity all[] = {ThermalQuantity::LogPartitionFunction, ThermalQuantity::Energy, ThermalQuantity::SpecificHeat,
                                   ThermalQuantity::Entropy, ThermalQuantity::FreeEnergy, ThermalQuantity::Observable};
    for (ThermalQuantity qn : all) EXPECT(s.standardError(qn, beta) == 0.0);
  }
}

int main() {
  // two levels: Z = 1 + e^-x, E = gap / (e^x + 1), C = x^2 e^x / (e^x + 1)^2 -- the K = 2 case of the ladder's forms
  for (double beta : {0.3, 1.0, 4.0})
    for (int copies : {1, 2, 4}) check_ladder(2, 1.5, beta, copies);
  for (double beta : {0.5, 1.5})
    for (int copies : {1, 4}) check_ladder(30, 0.7, beta, copies);
  {  // the two-level forms written out, once
    const ThermalSums s = ladder(2, 1.5, 1);
    const long double x = 1.5L * 0.8L;
    EXPECT(close(s.energy(0.8), 1.5L / (std::exp(x) + 1)));
    EXPECT(close(s.specificHeat(0.8), x * x * std::exp(x) / ((std::exp(x) + 1) * (std::exp(x) + 1))));
    EXPECT(close(std::exp(s.logPartitionFunction(0.8)), 1 + std::exp(-x)));
    // beta = 0: Z = N, E the plain mean, C = 0, S = log N
    EXPECT(s.logPartitionFunction(0.0) == std::log(2.0) && s.energy(0.0) == 0.75 && s.specificHeat(0.0) == 0.0 && s.entropy(0.0) == std::log(2.0));
  }
  {  // beta (theta_max - theta_min) = 1e4, three samples, the lowest value in one of them alone: every sum and every
     // jackknife subset stays finite, and the lowest level is all that is left
    ThermalSums s;
    s.setDimension(1e6);
    for (int r = 0; r < 3; ++r) {
      ThermalSample a;
      for (int j = 0; j < 5; ++j) a.theta.push_back(-5000.0 + (r == 0 && j == 0 ? 0.0 : 2500.0 * j + 100.0 * r + 50.0)), a.weight.push_back(0.2);
      a.theta.back() = 5000.0;
      a.a.push_back(std::vector<double>(5, 0.2 * (r + 1)));
      s.addSample(a);
    }
    const ThermalQuantity all[] = {ThermalQuantity::LogPartitionFunction, ThermalQuantity::Energy, ThermalQuantity::SpecificHeat,
                                   ThermalQuantity::Entropy, ThermalQuantity::FreeEnergy, ThermalQuantity::Observable};
    for (double beta : {1.0, 50.0})
      for (ThermalQuantity q : all) EXPECT(std::isfinite(s.value(q, beta)) && std::isfinite(s.standardError(q, beta)));
    EXPECT(s.referenceEnergy() == -5000.0 && s.energy(1.0) == -5000.0 && s.specificHeat(1.0) >= 0.0 && s.specificHeat(1.0) < 1e-50);
    EXPECT(close(s.logPartitionFunction(1.0), std::log(1e6L / 3 * 0.2L) + 5000.0L));
    EXPECT(s.observable(0, 1.0) == 1.0);  // a / w of sample 0
  }
  {  // a quantity that is linear in the samples at beta = 0: <A> = mean of c_r; the jackknife is then the standard error of the mean
    ThermalSums s;
    s.setDimension(4);
    const double c[4] = {1.0, 2.0, 4.0, 9.0};
    for (double v : c) {
      ThermalSample a;
      a.theta.push_back(0.5), a.weight.push_back(1.0);
      a.a.push_back(std::vector<double>(1, v));
      s.addSample(a);
    }
    double mean = 4.0, var = 0.0;
    for (double v : c) var += (v - mean) * (v - mean);
    EXPECT(s.observable(0, 0.0) == mean);
    EXPECT(close(s.standardError(ThermalQuantity::Observable, 0.0), std::sqrt(static_cast<long double>(var) / (4 * 3))));
    EXPECT(s.standardError(ThermalQuantity::Energy, 0.7) == 0.0);
  }
  {  // refusals
    ThermalSums s;
    ThermalSample a;
    bool threw = false;
    try {
      s.addSample(a);
    } catch (const std::invalid_argument&) {
      threw = true;
    }
    EXPECT(threw);
    a.theta.push_back(1.0), a.weight.push_back(1.0);
    s.addSample(a);
    a.a.push_back(std::vector<double>(1, 1.0));
    threw = false;
    try {
      s.addSample(a);
    } catch (const std::invalid_argument&) {
      threw = true;
    }
    EXPECT(threw);
    threw = false;
    try {
      s.observable(0, 1.0);
    } catch (const std::out_of_range&) {
      threw = true;
    }
    EXPECT(threw);
    s.clear();
    threw = false;
    try {
      s.energy(1.0);
    } catch (const std::logic_error&) {
      threw = true;
    }
    EXPECT(threw);
  }
  if (fails) return 1;
  std::printf("largest error / (50 eps) = %.3f\nTHERMAL SUMS OK\n", worst);
  return 0;
}
