// Host-only checks of what the spin front-end classes share (cmpt/eigen_ex/spin_frontend.hpp), for AddressSanitizer + UBSan:
// productStateRow against a full listing of eigenex_spin_sector_states, siteMask, dstUp, normalised, checkCoefficients, the
// wording of a zero response, and the pair masks with their unpacking.  No GPU: every library call here is host code.
// NOT part of the reference.  tests/test_spin_frontend_host.py builds and runs it.
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "cmpt/eigen_ex/spin_frontend.hpp"

using namespace cmpt::EigenEx;
typedef std::complex<double> Complex;

#define REQUIRE(...)                                                              \
  do {                                                                            \
    if (!(__VA_ARGS__)) {                                                         \
      std::fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #__VA_ARGS__); \
      std::exit(1);                                                               \
    }                                                                             \
  } while (0)

static const char* const kSites = "invalid input: the product state names a site outside 0..sites-1";
static const char* const kSector = "invalid input: the product state does not lie in the sector (its number of up sites differs)";

// every state of the sector (L, nUp) returns its row; every other word of L bits is refused with the sector message
static void sector(int L, int nUp, Index rows) {
  std::vector<std::uint32_t> states(static_cast<std::size_t>(rows));
  REQUIRE(eigenex_spin_sector_states(L, nUp, 0, rows, states.data()) == 0);
  for (Index r = 0; r < rows; ++r) {
    std::string why;
    REQUIRE(detail::productStateRow(L, nUp, rows, states[static_cast<std::size_t>(r)], why) == r && why.empty());
  }
  if (L > 8) return;
  Index members = 0;
  for (std::uint32_t bits = 0; bits < (std::uint32_t(1) << L); ++bits) {
    std::string why;
    const Index row = detail::productStateRow(L, nUp, rows, bits, why);
    if (detail::popcount(bits) == nUp) {
      REQUIRE(row >= 0 && states[static_cast<std::size_t>(row)] == bits && why.empty());
      ++members;
    } else {
      REQUIRE(row == -1 && why == kSector);
    }
  }
  REQUIRE(members == rows);
}

int main() {
  sector(6, 3, 20);
  sector(5, 0, 1);
  sector(5, 5, 1);
  sector(32, 1, 32);  // sites = 32: no word has a bit above the sites, and the top bit is a state
  {
    std::string why;
    REQUIRE(detail::productStateRow(32, 1, 32, std::uint32_t(1) << 31, why) == 31 && why.empty());
    REQUIRE(detail::productStateRow(32, 1, 32, 3u, why) == -1 && why == kSector);
    why.clear();
    REQUIRE(detail::productStateRow(6, 3, 20, (std::uint32_t(1) << 6) | 3u, why) == -1 && why == kSites);  // three up, one outside
    why.clear();
    REQUIRE(detail::productStateRow(6, 3, 20, std::uint32_t(1) << 31, why) == -1 && why == kSites);
    why.clear();
    REQUIRE(detail::productStateRow(5, -1, 32, 32u, why) == -1 && why == kSites);
    why.clear();
    REQUIRE(detail::productStateRow(5, -1, 32, 21u, why) == 21 && why.empty());  // the full space: the state is the row
  }
  {
    bool valid = true;
    REQUIRE(detail::siteMask(std::vector<int>{0, 3, 31}, valid) == (1u | 8u | (std::uint32_t(1) << 31)) && valid);
    REQUIRE(detail::siteMask(std::vector<int>(), valid) == 0u && valid);
    REQUIRE(detail::siteMask(std::vector<int>{2, 2}, valid) == 4u && !valid);
    valid = true;
    REQUIRE(detail::siteMask(std::vector<int>{1, -1}, valid) == 2u && !valid);
    valid = true;
    REQUIRE(detail::siteMask(std::vector<int>{32, 5}, valid) == 32u && !valid);
    REQUIRE(detail::popcount(0u) == 0 && detail::popcount(0xffffffffu) == 32 && detail::popcount(0x80000001u) == 2);
  }
  {
    const int kinds[3] = {EIGENEX_SPIN_SITE_Z, EIGENEX_SPIN_SITE_PLUS, EIGENEX_SPIN_SITE_MINUS};
    for (int kind : kinds) REQUIRE(detail::dstUp(-1, kind) == -1);  // the full space stays
    REQUIRE(detail::dstUp(3, EIGENEX_SPIN_SITE_Z) == 3 && detail::dstUp(3, EIGENEX_SPIN_SITE_PLUS) == 4 && detail::dstUp(3, EIGENEX_SPIN_SITE_MINUS) == 2);
    REQUIRE(detail::dstUp(0, EIGENEX_SPIN_SITE_MINUS) == -1);  // below the sectors: the caller refuses it (nUp >= 0 and a result < 0)
    REQUIRE(detail::dstUp(6, EIGENEX_SPIN_SITE_PLUS) == 7);    // above them, at L = 6
  }
  {
    typedef DenseVector<Complex> Vector;
    const char* const zero = "invalid input: the state is zero (or not finite)";
    std::string why;
    double norm = -1.0;
    REQUIRE(detail::normalised(Vector(4, Complex(0.0, 0.0)), 4, norm, why).size() == 0 && why == zero);
    why.clear();
    REQUIRE(detail::normalised(Vector(4, Complex(std::numeric_limits<double>::quiet_NaN(), 0.0)), 4, norm, why).size() == 0 && why == zero);
    why.clear();
    REQUIRE(detail::normalised(Vector(4, Complex(0.0, std::numeric_limits<double>::infinity())), 4, norm, why).size() == 0 && why == zero);
    why.clear();
    REQUIRE(detail::normalised(Vector(3, Complex(1.0, 0.0)), 4, norm, why).size() == 0 &&
            why == "invalid input: the state must have one entry per row of the model's space or sector");
    why.clear();
    Vector v(4, Complex(0.0, 0.0));
    v[1] = Complex(3.0, 0.0), v[2] = Complex(0.0, -4.0);
    const Vector u = detail::normalised(v, 4, norm, why);
    REQUIRE(why.empty() && norm == 5.0 && u.size() == 4);
    REQUIRE(u[0] == Complex(0.0, 0.0) && u[1] == Complex(3.0 / 5.0, 0.0) && u[2] == Complex(0.0, -4.0 / 5.0) && u[3] == Complex(0.0, 0.0));
  }
  {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const std::vector<double> good(4, 0.5), shorter(3, 0.5), bad = {0.5, 0.5, nan, 0.5}, worse = {0.5, inf, 0.5, 0.5};
    REQUIRE(detail::checkCoefficients(good, nullptr, 4, "the site operator").empty());
    REQUIRE(detail::checkCoefficients(good, &good, 4, "the site operator").empty());
    REQUIRE(detail::checkCoefficients(shorter, nullptr, 4, "the site operator") == "invalid input: the site operator needs one coefficient per site");
    REQUIRE(detail::checkCoefficients(good, &shorter, 4, "a measured operator") == "invalid input: a measured operator needs one coefficient per site");
    REQUIRE(detail::checkCoefficients(bad, nullptr, 4, "the site operator") == "invalid input: a coefficient of the site operator is not finite");
    REQUIRE(detail::checkCoefficients(good, &worse, 4, "the source operator") == "invalid input: a coefficient of the source operator is not finite");
    const detail::SiteApplication exact = {detail::SiteApplication::ExactZero, 0.0}, rounding = {detail::SiteApplication::RoundingZero, 1e-40},
                                  unit = {detail::SiteApplication::Unit, 2.0};
    REQUIRE(exact.zero() && rounding.zero() && !unit.zero());
    REQUIRE(exact.zeroNote("O|v>", "this part of the response") == "O|v> = 0: this part of the response is identically zero");
    REQUIRE(rounding.zeroNote("B|psi_0>", "the response") == "B|psi_0> vanishes within the rounding of its application: the response is identically zero");
  }
  for (std::size_t L : {std::size_t(2), std::size_t(5)}) {
    // raw[k] names its pair: 100 i + j for the mask with bits i < j, so the unpacked matrix must hold it at (i, j) and (j, i)
    std::vector<std::uint32_t> masks;
    detail::appendSiteMasks(L, masks);
    REQUIRE(masks.size() == L);
    for (std::size_t i = 0; i < L; ++i) REQUIRE(masks[i] == std::uint32_t(1) << i);
    detail::appendPairMasks(L, masks);
    REQUIRE(masks.size() == L + L * (L - 1) / 2);
    std::vector<std::uint64_t> wide;
    detail::appendPairMasks(L, wide);
    std::vector<double> raw;
    for (std::size_t k = L; k < masks.size(); ++k) {
      REQUIRE(detail::popcount(masks[k]) == 2 && wide[k - L] == masks[k]);
      int i = 0, j = 31;
      while (!((masks[k] >> i) & 1u)) ++i;
      while (!((masks[k] >> j) & 1u)) --j;
      raw.push_back(2.0 * (100.0 * i + j));
    }
    const std::vector<double> out = detail::pairMatrix(raw.data(), L, 2.0, 0.25);
    REQUIRE(out.size() == L * L);
    for (std::size_t i = 0; i < L; ++i)
      for (std::size_t j = 0; j < L; ++j)
        REQUIRE(out[i * L + j] == (i == j ? 0.25 : 100.0 * static_cast<double>(i < j ? i : j) + static_cast<double>(i < j ? j : i)));
  }
  std::printf("SPIN FRONTEND OK\n");
  return 0;
}
