// The index arithmetic of the reduced-density-matrix kernel (kernels.hip: k_spin_rdm<SECTOR, TILE>; spin_rdm.hpp has the
// definition and the work table), shared by the device code and by the host replay tests/cpp/spin_rdm_sanitize.cpp under the
// rules of spin_rows.hpp, which includes this file: plain C++11, all memory reached through the caller's accessor objects
// (binom, tab.hi / tab.lo, x).  spin_rdm_host and spin_rdm_deposit do not use this file: they are what it is checked against.
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

// one panel element: x at the rank of (sa | sb), or 0 behind a load of row 0 where the lane is not live
template <bool SECTOR, class Tables, class Vector>
EIGENEX_HD double spin_rdm_element(const Tables& tab, const Vector& x, int h, uint32_t lo_mask, uint32_t sa, uint32_t sb, bool live, uint32_t fallback) {
  const uint32_t s = live ? (sa | sb) : fallback;
  const uint32_t base = SECTOR ? tab.hi(s >> h) : s;
  const uint32_t low = SECTOR ? tab.lo(s & lo_mask) : 0u;
  const double v = x(base + low);
  return live ? v : 0.0;
}

// The same element of an interleaved complex vector (k_spin_rdm_z): one walk of the rank tables and one load serve both parts
// (x(i) is the pair at row i, a 16-byte load on the device; SpinZ is spin_rows.hpp's pair).
template <bool SECTOR, class Tables, class Vector>
EIGENEX_HD SpinZ spin_rdm_element_z(const Tables& tab, const Vector& x, int h, uint32_t lo_mask, uint32_t sa, uint32_t sb, bool live, uint32_t fallback) {
  const uint32_t s = live ? (sa | sb) : fallback;
  const uint32_t base = SECTOR ? tab.hi(s >> h) : s;
  const uint32_t low = SECTOR ? tab.lo(s & lo_mask) : 0u;
  const SpinZ v = x(base + low);
  return live ? v : SpinZ{0.0, 0.0};
}

// k_spin_rdm_z: the r-th of the four tile rows (columns) of the lane at position t of `side` = TILE / 4 positions, and where
// row `row` of b `bj` lies in a b-major panel of CHUNK * (TILE + 1) pairs (spin_rdm.hpp says why these and not the real
// kernel's 4 t + r and TILE + 2)
EIGENEX_HD int spin_rdm_lane_row_z(int side, int t, int r) { return t + side * r; }
EIGENEX_HD int spin_rdm_panel_index_z(int tile, int bj, int row) { return bj * (tile + 1) + row; }

}  // namespace eigenex
