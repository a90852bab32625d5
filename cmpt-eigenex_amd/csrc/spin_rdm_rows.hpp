// The index arithmetic of the reduced-density-matrix kernel (kernels.hip: k_spin_rdm<SECTOR, TILE, E>; spin_rdm.hpp has the
// definition and the work table), shared by the device code and by the host replay tests/cpp/spin_rdm_replay.hpp under the
// rules of spin_rows.hpp, which includes this file: plain C++11, all memory reached through the caller's accessor objects
// (binom, tab.hi / tab.lo, x).  spin_rdm_host, spin_rdm_host_z and spin_rdm_deposit do not use this file: they are what it is
// checked against.
//
// A workgroup holds a tile of TILE rows a_i (and TILE rows a_j of the other tile of its pair) and takes the b's of its slice
// CHUNK at a time.  Per tile and per chunk the states dep_A(a) and dep_B(b) are formed ONCE (spin_rdm_party_state: unrank
// through the binomials with the party's own (sites, sites up), then deposit) and kept in LDS; the TILE x CHUNK panel elements
// are then loads of x at rank(dep_A(a) | dep_B(b)) (spin_rdm_element).  The two words are disjoint, so the two table indices of
// the union are the unions of the parties' indices: hi_base[(a_hi | b_hi)] + lo_rank[(a_lo | b_lo)].
//
// Padding: a row at or past d_k and a b at or past the slice's end are not live.  A lane that is not live ranks and loads
// `fallback`, the state of row 0 of the vector (the spin_site_targets rule: the lane's own words may lie outside the sector, so
// the sum of their table entries may lie outside x), and its element is 0.  No load is branched around and none leaves the
// vector or the rank tables.
#pragma once
#include "spin_rdm.hpp"

namespace eigenex {

// dep(w): bit j of w goes to the j-th lowest set bit of the mask, set bit by set bit (the mask is the same for every lane)
EIGENEX_HD uint32_t spin_deposit(uint32_t w, uint32_t mask) {
  uint32_t s = 0;
  for (uint32_t m = mask; m != 0; m &= m - 1, w >>= 1) s |= (w & 1u) ? (m & (0u - m)) : 0u;
  return s;
}

// The deposited state of index r of one party (n sites of `mask`, kk of them up in a sector; the word r itself in the full
// space).  A lane that is not live unranks index 0, which every party has: every read of the binomials stays where a live lane
// reads, and the caller does not use the state.
template <bool SECTOR, class Binom>
EIGENEX_HD uint32_t spin_rdm_party_state(const Binom& binom, int n, int kk, uint32_t mask, uint32_t r, bool live) {
  const uint32_t rr = live ? r : 0u;
  return spin_deposit(SECTOR ? spin_unrank_row(binom, n, kk, rr).s : rr, mask);
}

// Which element of a tile x chunk panel lane-slot e gathers: the rows run along consecutive e (along_a) or the b's do.  The
// kernel takes along_a for a 64-row tile where A owns site 0 (consecutive a are then consecutive or near rows of x) and the
// b's in every other case, as measured (profiles/spin_entanglement.md).
EIGENEX_HD void spin_rdm_panel_slot(bool along_a, int tile, int chunk, int e, int* row, int* bj) {
  *row = along_a ? e % tile : e / chunk;
  *bj = along_a ? e / tile : e % chunk;
}

// one panel element: x at the rank of (sa | sb), or 0 behind a load of row 0 where the lane is not live.  Of an interleaved
// complex vector one walk of the rank tables and one load serve both parts (x(i) is then the pair at row i, a 16-byte load on
// the device; SpinZ is spin_rows.hpp's pair).
// The element is what the accessor returns.
template <bool SECTOR, class Tables, class Vector>
EIGENEX_HD auto spin_rdm_element(const Tables& tab, const Vector& x, int h, uint32_t lo_mask, uint32_t sa, uint32_t sb, bool live, uint32_t fallback)
    -> decltype(x(0u)) {
  typedef decltype(x(0u)) E;
  const uint32_t s = live ? (sa | sb) : fallback;
  const uint32_t base = SECTOR ? tab.hi(s >> h) : s;
  const uint32_t low = SECTOR ? tab.lo(s & lo_mask) : 0u;
  const E v = x(base + low);
  return live ? v : E{};
}

// The shape of the panels of k_spin_rdm<SECTOR, TILE, E>, in elements: the b's staged at a time, the pitch of a b-major panel,
// where the column of b `bj` starts in it -- row `row` of that b lies at panel_column(bj) + row -- and the r-th of the four tile
// rows (columns) of the lane at position t of SIDE = TILE / 4 positions.  A double: 4 t + r and TILE + 2.  A pair: t + SIDE r
// and TILE + 1, and half as many b's (spin_rdm.hpp says why these and not the real kernel's).  The kernel and its replay read
// the shape from here and nowhere else.  (The row is added by the caller and not in here: with the whole sum in one function
// the compiler shares it between the two panels of a pair, another instruction stream than the one measured.)
template <class E, int TILE>
struct SpinRdmGeometry {
  static constexpr bool REAL = sizeof(E) == sizeof(double);
  static constexpr int SIDE = TILE / 4;
  static constexpr int CHUNK = TILE == kSpinRdmBigTile ? (REAL ? kSpinRdmBigChunk : kSpinRdmBigChunkZ) : (REAL ? kSpinRdmSmallChunk : kSpinRdmSmallChunkZ);
  static constexpr int PITCH = REAL ? TILE + 2 : TILE + 1;
  static constexpr int PANEL = CHUNK * PITCH;
  static EIGENEX_HD int panel_column(int bj) { return bj * PITCH; }
  static EIGENEX_HD int lane_row(int t, int r) { return REAL ? 4 * t + r : t + SIDE * r; }
};

// One term of an entry's chains, (re, im) += a * conj(b): one fma into re, of pairs four in the definition's order
// (spin_rdm_host_z).  The accumulators of both elements are kept as parts, each in an array of its own -- they are registers, and
// the compiler orders them as the arrays lie -- and a real vector leaves im at its +0.0.
EIGENEX_HD void spin_rdm_fma(double a, double b, double& re, double&) { re = std::fma(a, b, re); }
EIGENEX_HD void spin_rdm_fma(SpinZ a, SpinZ b, double& re, double& im) {
  re = std::fma(a.re, b.re, re);
  re = std::fma(a.im, b.im, re);
  im = std::fma(a.im, b.re, im);
  im = std::fma(-a.re, b.im, im);
}

// the entry (i, j) as it is stored, from its parts: the imaginary part of a diagonal entry is not the computed chain but +0.0
// (spin_rdm.hpp)
template <class E>
EIGENEX_HD E spin_rdm_entry(double re, double im, bool diagonal);
template <>
EIGENEX_HD double spin_rdm_entry<double>(double re, double, bool) {
  return re;
}
template <>
EIGENEX_HD SpinZ spin_rdm_entry<SpinZ>(double re, double im, bool diagonal) {
  return SpinZ{re, diagonal ? 0.0 : im};
}

// a + b part by part: the slices of an entry are added with plain adds
EIGENEX_HD double spin_sum(double a, double b) { return a + b; }
EIGENEX_HD SpinZ spin_sum(SpinZ a, SpinZ b) { return SpinZ{a.re + b.re, a.im + b.im}; }

}  // namespace eigenex
