// csrc/lag_terms.hpp under AddressSanitizer + UBSan (tests/test_one_sweep_host.py builds and starts this program): per line of
// the input file one case  k a' beta_k da alpha[k] beta[k] c[k] f[k+1] d[k+1] c_next[k+1]  as hexadecimal doubles, written by
// the numpy restatement.  Every array is allocated at its exact size, the terms are formed the way k_sweep and k_lag_terms
// form them, and the results must be the restatement's bits.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "lag_terms.hpp"

static bool same(double a, double b) { return a == b || (std::isnan(a) && std::isnan(b)); }

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  std::string line;
  int ncases = 0;
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    std::istringstream ls(line);
    std::vector<double> v;
    std::string tok;
    while (ls >> tok) v.push_back(std::strtod(tok.c_str(), nullptr));
    if (v.size() < 4) return 3;
    const int k = (int)v[0];
    const double a_raw = v[1], beta_k = v[2], da_ref = v[3];
    if (v.size() != (size_t)(4 + 3 * k + 3 * (k + 1))) return 3;
    size_t at = 4;
    auto take = [&](int n) {
      std::vector<double> out(v.begin() + (std::ptrdiff_t)at, v.begin() + (std::ptrdiff_t)(at + (size_t)n));
      at += (size_t)n;
      return out;
    };
    const std::vector<double> alpha = take(k), beta = take(k), c = take(k), f_ref = take(k + 1), d = take(k + 1), cn_ref = take(k + 1);
    const double da = eigenex::lag_alpha_correction(k, beta.data(), c.data());
    if (!same(da, da_ref)) {
      std::printf("k=%d: da %a, restatement %a\n", k, da, da_ref);
      return 1;
    }
    for (int i = 0; i <= k; ++i) {
      const double f = eigenex::lag_f_entry(i, k, alpha.data(), beta.data(), c.data(), a_raw, da);
      if (!same(f, f_ref[(size_t)i])) {
        std::printf("k=%d: f[%d] %a, restatement %a\n", k, i, f, f_ref[(size_t)i]);
        return 1;
      }
      const double cn = eigenex::lag_next_coefficient(d[(size_t)i], f, beta_k, 1e-12);
      if (!same(cn, cn_ref[(size_t)i])) {
        std::printf("k=%d: c_next[%d] %a, restatement %a\n", k, i, cn, cn_ref[(size_t)i]);
        return 1;
      }
      if (eigenex::lag_next_coefficient(d[(size_t)i], f, 1e-13, 1e-12) != 0.0) return 1;  // nothing is pending behind a breakdown
    }
    ++ncases;
  }
  if (eigenex::kLagGuard != std::ldexp(1.0, -27)) return 1;
  std::printf("LAG TERMS OK %d cases\n", ncases);
  return 0;
}
