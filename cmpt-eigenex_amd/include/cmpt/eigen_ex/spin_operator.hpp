// Spin-1/2 Hamiltonians of exact diagonalisation, applied matrix-free.
//
//   H = sum_b [ Jz_b Sz_i Sz_j + (Jxy_b/2)(S+_i S-_j + S-_i S+_j) ] + sum_i hz_i Sz_i + sum_i hx_i Sx_i
//
// on L sites, full Hilbert space 2^L; basis state s has site i up iff bit i of s is set.  Nobody stores this matrix: row s
// follows from the bits of s.  SpinHalfModel is the description (sites, bonds, fields); two ways onto the device:
//   device::spinHalfOperator   uploads the description alone (eigenex_spin_upload: a few hundred bytes); the kernel works
//                              out every row as it goes -- the default choice, and the only one that reaches L = 28..30
//   toCsr() + CsrOperator      the rows as stored CSR (eigenex_spin_csr: 12 bytes per entry, about L/2 + 1 entries per row)
// Both add a row's products in the same order (include/eigenex_hip.h has it) and give bit-identical operator applications.
//
// A model without a transverse field conserves total Sz, and its levels are found sector by sector: the states with nUp sites
// up, ascending, C(L, nUp) of them (L up to 32 here).  sectorRows / sectorStates / toSectorCsr describe one sector on the host,
// device::spinHalfSectorOperator applies it matrix-free (eigenex_spin_sector_upload).  Within a sector the SU(2) multiplets of
// the full space no longer repeat, so "the lowest k levels" can be asked of a Lanczos solver with one start vector.
//
// A model that is also invariant under the translation by `cell` sites splits further, into the L / cell momentum sectors of each
// Sz sector: the orbits of the translation, one row each, about L / cell times fewer rows.  translationInvariant /
// momentumDimension / momentumStates / toMomentumCsr describe one on the host, device::spinHalfMomentumOperator applies it
// matrix-free (eigenex_spin_momentum_upload).  Momentum 0 and half the number of translations are real symmetric and take real
// states; every other momentum is complex Hermitian and needs complex states.
#pragma once

#include <complex>
#include <limits>

#include "device.hpp"
#include "triplets_operator.hpp"

namespace cmpt {
namespace EigenEx {

class SpinHalfModel {
 public:
  explicit SpinHalfModel(int sites = 2) : sites_(sites) {}

  // nearest-neighbour chain: bonds (i, i+1), i = 0 .. L-2, and with `periodic` the bond (L-1, 0).  Jz = Jxy: Heisenberg.
  static SpinHalfModel chain(int L, double Jz, double Jxy, bool periodic) {
    SpinHalfModel m(L);
    for (int i = 0; i + 1 < L; ++i) m.addBond(i, i + 1, Jz, Jxy);
    if (periodic && L > 2) m.addBond(L - 1, 0, Jz, Jxy);
    return m;
  }

  // Jz Sz_i Sz_j + (Jxy/2)(S+_i S-_j + S-_i S+_j); the same pair may be added more than once
  SpinHalfModel& addBond(int i, int j, double Jz, double Jxy) {
    si_.push_back(i), sj_.push_back(j), jz_.push_back(Jz), jxy_.push_back(Jxy);
    return *this;
  }
  // hz Sz_i (longitudinal) and hx Sx_i (transverse) on one site; a field that is never set is absent
  SpinHalfModel& setFieldZ(int site, double hz) { return setField(hz_, site, hz); }
  SpinHalfModel& setFieldX(int site, double hx) { return setField(hx_, site, hx); }

  int sites() const { return sites_; }
  int bonds() const { return static_cast<int>(si_.size()); }
  Index rows() const { return sites_ >= 0 && sites_ < 62 ? Index(1) << sites_ : 0; }
  const std::int32_t* siteI() const { return si_.data(); }
  const std::int32_t* siteJ() const { return sj_.data(); }
  const double* jz() const { return jz_.data(); }
  const double* jxy() const { return jxy_.data(); }
  const double* fieldZ() const { return hz_.empty() ? nullptr : hz_.data(); }
  const double* fieldX() const { return hx_.empty() ? nullptr : hx_.data(); }

  // rows [row_begin, row_end) as CSR with global columns, in the stored order of eigenex_spin_csr (the diagonal first)
  HostCsr<double> toCsr(Index row_begin = 0, Index row_end = -1) const {
    if (row_end < 0) row_end = rows();
    HostCsr<double> m;
    m.n = rows();
    std::vector<std::int64_t> rp(static_cast<std::size_t>(row_end > row_begin ? row_end - row_begin : 0) + 1, 0);
    std::int64_t nnz = 0;
    device::check(eigenex_spin_csr(sites_, bonds(), siteI(), siteJ(), jz(), jxy(), fieldZ(), fieldX(), row_begin, row_end - row_begin,
                                   rp.data(), nullptr, nullptr, &nnz),
                  "eigenex_spin_csr");
    if (nnz > static_cast<std::int64_t>(std::numeric_limits<std::int32_t>::max()))
      throw LanczosException("SpinHalfModel::toCsr: more than 2^31 - 1 stored entries (use device::spinHalfOperator, or fewer rows)");
    m.col.assign(static_cast<std::size_t>(nnz), 0);
    m.val.assign(static_cast<std::size_t>(nnz), 0.0);
    device::check(eigenex_spin_csr(sites_, bonds(), siteI(), siteJ(), jz(), jxy(), fieldZ(), fieldX(), row_begin, row_end - row_begin,
                                   rp.data(), m.col.data(), m.val.data(), &nnz),
                  "eigenex_spin_csr");
    m.rowptr.assign(rp.begin(), rp.end());
    return m;
  }

  // the sector of nUp sites up: its dimension C(sites, nUp), its states in ascending order (row r of the sector is state
  // sectorStates(nUp)[r] of the full space), and rows [row_begin, row_end) of the sector matrix as CSR (columns are ranks)
  Index sectorRows(int nUp) const {
    std::int64_t dim = 0;
    device::check(eigenex_spin_sector_dim(sites_, nUp, &dim), "eigenex_spin_sector_dim");
    return static_cast<Index>(dim);
  }
  std::vector<std::uint32_t> sectorStates(int nUp) const {
    std::vector<std::uint32_t> s(static_cast<std::size_t>(sectorRows(nUp)), 0u);
    device::check(eigenex_spin_sector_states(sites_, nUp, 0, static_cast<std::int64_t>(s.size()), s.data()), "eigenex_spin_sector_states");
    return s;
  }
  HostCsr<double> toSectorCsr(int nUp, Index row_begin = 0, Index row_end = -1) const {
    if (row_end < 0) row_end = sectorRows(nUp);
    HostCsr<double> m;
    m.n = sectorRows(nUp);
    std::vector<std::int64_t> rp(static_cast<std::size_t>(row_end > row_begin ? row_end - row_begin : 0) + 1, 0);
    std::int64_t nnz = 0;
    device::check(eigenex_spin_sector_csr(sites_, nUp, bonds(), siteI(), siteJ(), jz(), jxy(), fieldZ(), fieldX(), row_begin,
                                          row_end - row_begin, rp.data(), nullptr, nullptr, &nnz),
                  "eigenex_spin_sector_csr");
    if (nnz > static_cast<std::int64_t>(std::numeric_limits<std::int32_t>::max()))
      throw LanczosException("SpinHalfModel::toSectorCsr: more than 2^31 - 1 stored entries (use device::spinHalfSectorOperator, or fewer rows)");
    m.col.assign(static_cast<std::size_t>(nnz), 0);
    m.val.assign(static_cast<std::size_t>(nnz), 0.0);
    device::check(eigenex_spin_sector_csr(sites_, nUp, bonds(), siteI(), siteJ(), jz(), jxy(), fieldZ(), fieldX(), row_begin,
                                          row_end - row_begin, rp.data(), m.col.data(), m.val.data(), &nnz),
                  "eigenex_spin_sector_csr");
    m.rowptr.assign(rp.begin(), rp.end());
    return m;
  }

  // Is the model invariant under the translation by `cell` sites and free of a transverse field, i.e. does it have momentum
  // sectors of that cell?  (eigenex_last_error says which bond or site breaks the symmetry.)
  bool translationInvariant(int cell = 1) const {
    for (double h : hx_)
      if (h != 0.0) return false;
    std::int64_t rp[1] = {0}, nnz = 0;
    return eigenex_spin_momentum_csr(sites_, 0, cell, 0, bonds(), siteI(), siteJ(), jz(), jxy(), fieldZ(), 0, 0, rp, nullptr, nullptr, &nnz) == 0;
  }
  // the momentum sector m (0 .. sites / cell - 1) of the sector of nUp sites up: its dimension, its representatives in ascending
  // order with their periods, and rows [row_begin, row_end) as CSR (values complex; all real at m = 0 and 2 m = sites / cell)
  Index momentumDimension(int nUp, int cell, int m) const {
    std::int64_t dim = 0;
    device::check(eigenex_spin_momentum_dim(sites_, nUp, cell, m, &dim), "eigenex_spin_momentum_dim");
    return static_cast<Index>(dim);
  }
  std::vector<std::uint32_t> momentumStates(int nUp, int cell, int m, std::vector<std::uint8_t>* periods = nullptr) const {
    std::vector<std::uint32_t> s(static_cast<std::size_t>(momentumDimension(nUp, cell, m)), 0u);
    if (periods) periods->assign(s.size(), 0);
    device::check(eigenex_spin_momentum_states(sites_, nUp, cell, m, 0, static_cast<std::int64_t>(s.size()), s.data(), periods ? periods->data() : nullptr),
                  "eigenex_spin_momentum_states");
    return s;
  }
  HostCsr<std::complex<double>> toMomentumCsr(int nUp, int cell, int m, Index row_begin = 0, Index row_end = -1) const {
    requireNoTransverseField("SpinHalfModel::toMomentumCsr");
    HostCsr<std::complex<double>> out;
    out.n = momentumDimension(nUp, cell, m);
    if (row_end < 0) row_end = out.n;
    std::vector<std::int64_t> rp(static_cast<std::size_t>(row_end > row_begin ? row_end - row_begin : 0) + 1, 0);
    std::int64_t nnz = 0;
    device::check(eigenex_spin_momentum_csr(sites_, nUp, cell, m, bonds(), siteI(), siteJ(), jz(), jxy(), fieldZ(), row_begin, row_end - row_begin,
                                            rp.data(), nullptr, nullptr, &nnz),
                  "eigenex_spin_momentum_csr");
    if (nnz > static_cast<std::int64_t>(std::numeric_limits<std::int32_t>::max()))
      throw LanczosException("SpinHalfModel::toMomentumCsr: more than 2^31 - 1 stored entries (use device::spinHalfMomentumOperator, or fewer rows)");
    out.col.assign(static_cast<std::size_t>(nnz), 0);
    out.val.assign(static_cast<std::size_t>(nnz), std::complex<double>(0.0, 0.0));
    device::check(eigenex_spin_momentum_csr(sites_, nUp, cell, m, bonds(), siteI(), siteJ(), jz(), jxy(), fieldZ(), row_begin, row_end - row_begin,
                                            rp.data(), out.col.data(), reinterpret_cast<double*>(out.val.data()), &nnz),
                  "eigenex_spin_momentum_csr");
    out.rowptr.assign(rp.begin(), rp.end());
    return out;
  }
  // The same sector on rings of up to 48 sites and 128 bonds, with 64-bit states (eigenex_spin_momentum64_*): what momentumDimension,
  // momentumStates and toMomentumCsr return for sites <= 32, and the only form beyond.  The enumeration is threaded; (36, 18) walks
  // 9.1e9 states.
  Index momentum64Dimension(int nUp, int cell, int m) const {
    std::int64_t dim = 0;
    device::check(eigenex_spin_momentum64_dim(sites_, nUp, cell, m, &dim), "eigenex_spin_momentum64_dim");
    return static_cast<Index>(dim);
  }
  std::vector<std::uint64_t> momentum64States(int nUp, int cell, int m, std::vector<std::uint8_t>* periods = nullptr) const {
    std::vector<std::uint64_t> s(static_cast<std::size_t>(momentum64Dimension(nUp, cell, m)), 0u);
    if (periods) periods->assign(s.size(), 0);
    device::check(eigenex_spin_momentum64_states(sites_, nUp, cell, m, 0, static_cast<std::int64_t>(s.size()), s.data(), periods ? periods->data() : nullptr),
                  "eigenex_spin_momentum64_states");
    return s;
  }
  HostCsr<std::complex<double>> toMomentum64Csr(int nUp, int cell, int m, Index row_begin = 0, Index row_end = -1) const {
    requireNoTransverseField("SpinHalfModel::toMomentum64Csr");
    HostCsr<std::complex<double>> out;
    out.n = momentum64Dimension(nUp, cell, m);
    if (row_end < 0) row_end = out.n;
    std::vector<std::int64_t> rp(static_cast<std::size_t>(row_end > row_begin ? row_end - row_begin : 0) + 1, 0);
    std::int64_t nnz = 0;
    device::check(eigenex_spin_momentum64_csr(sites_, nUp, cell, m, bonds(), siteI(), siteJ(), jz(), jxy(), fieldZ(), row_begin, row_end - row_begin,
                                              rp.data(), nullptr, nullptr, &nnz),
                  "eigenex_spin_momentum64_csr");
    if (nnz > static_cast<std::int64_t>(std::numeric_limits<std::int32_t>::max()))
      throw LanczosException("SpinHalfModel::toMomentum64Csr: more than 2^31 - 1 stored entries (use device::spinHalfMomentum64Operator, or fewer rows)");
    out.col.assign(static_cast<std::size_t>(nnz), 0);
    out.val.assign(static_cast<std::size_t>(nnz), std::complex<double>(0.0, 0.0));
    device::check(eigenex_spin_momentum64_csr(sites_, nUp, cell, m, bonds(), siteI(), siteJ(), jz(), jxy(), fieldZ(), row_begin, row_end - row_begin,
                                              rp.data(), out.col.data(), reinterpret_cast<double*>(out.val.data()), &nnz),
                  "eigenex_spin_momentum64_csr");
    out.rowptr.assign(rp.begin(), rp.end());
    return out;
  }
  // the momentum entry points take no transverse field: one that is set and not zero is an error here, not silently dropped
  void requireNoTransverseField(const char* who) const {
    for (double h : hx_)
      if (h != 0.0) throw LanczosException(std::string(who) + ": a transverse field (hx != 0) does not conserve Sz: the model has no momentum sector");
  }

 private:
  SpinHalfModel& setField(std::vector<double>& h, int site, double value) {
    if (site < 0 || site >= sites_) throw LanczosException("SpinHalfModel: site index out of range");
    if (h.empty()) h.assign(static_cast<std::size_t>(sites_), 0.0);
    h[static_cast<std::size_t>(site)] = value;
    return *this;
  }
  int sites_;
  std::vector<std::int32_t> si_, sj_;
  std::vector<double> jz_, jxy_, hz_, hx_;
};

namespace device {

// the model as a matrix-free device operator (one GPU, real states); every solver class takes it through setDeviceOperator
inline std::shared_ptr<CsrOperator> spinHalfOperator(std::shared_ptr<Context> ctx, const SpinHalfModel& model) {
  eigenex_csr_t h = nullptr;
  check(eigenex_spin_upload(ctx->handle(), model.sites(), model.bonds(), model.siteI(), model.siteJ(), model.jz(), model.jxy(),
                            model.fieldZ(), model.fieldX(), &h),
        "eigenex_spin_upload");
  return CsrOperator::adopt(std::move(ctx), h);
}

// the model in the sector of nUp sites up (sites() up to 32, no transverse field), matrix-free in the same way
inline std::shared_ptr<CsrOperator> spinHalfSectorOperator(std::shared_ptr<Context> ctx, const SpinHalfModel& model, int nUp) {
  eigenex_csr_t h = nullptr;
  check(eigenex_spin_sector_upload(ctx->handle(), model.sites(), nUp, model.bonds(), model.siteI(), model.siteJ(), model.jz(), model.jxy(),
                                   model.fieldZ(), model.fieldX(), &h),
        "eigenex_spin_sector_upload");
  return CsrOperator::adopt(std::move(ctx), h);
}

// the same two operators for complex states (eigenex_spin_upload_z, eigenex_spin_sector_upload_z): the same real Hamiltonian and
// tables; a state created on such a handle is complex.  nUp = -1: the full space.
inline std::shared_ptr<CsrOperator> spinHalfComplexOperator(std::shared_ptr<Context> ctx, const SpinHalfModel& model, int nUp = -1) {
  eigenex_csr_t h = nullptr;
  if (nUp < 0)
    check(eigenex_spin_upload_z(ctx->handle(), model.sites(), model.bonds(), model.siteI(), model.siteJ(), model.jz(), model.jxy(),
                                model.fieldZ(), model.fieldX(), &h),
          "eigenex_spin_upload_z");
  else
    check(eigenex_spin_sector_upload_z(ctx->handle(), model.sites(), nUp, model.bonds(), model.siteI(), model.siteJ(), model.jz(),
                                       model.jxy(), model.fieldZ(), model.fieldX(), &h),
          "eigenex_spin_sector_upload_z");
  return CsrOperator::adopt(std::move(ctx), h);
}

// the model in the momentum sector m of the sector of nUp sites up, under the translation by `cell` sites, matrix-free
// (eigenex_spin_momentum_upload; complexStates: eigenex_spin_momentum_upload_z).  Real states take m = 0 and 2 m = sites / cell
// only: any other momentum throws unless complexStates is set.  LanczosEigenSolver<double> and
// LanczosEigenSolver<std::complex<double>> take the handle through setDeviceOperator as they take the others.
inline std::shared_ptr<CsrOperator> spinHalfMomentumOperator(std::shared_ptr<Context> ctx, const SpinHalfModel& model, int nUp, int m, int cell = 1,
                                                             bool complexStates = false) {
  model.requireNoTransverseField("device::spinHalfMomentumOperator");
  eigenex_csr_t h = nullptr;
  if (complexStates)
    check(eigenex_spin_momentum_upload_z(ctx->handle(), model.sites(), nUp, cell, m, model.bonds(), model.siteI(), model.siteJ(), model.jz(),
                                         model.jxy(), model.fieldZ(), &h),
          "eigenex_spin_momentum_upload_z");
  else
    check(eigenex_spin_momentum_upload(ctx->handle(), model.sites(), nUp, cell, m, model.bonds(), model.siteI(), model.siteJ(), model.jz(),
                                       model.jxy(), model.fieldZ(), &h),
          "eigenex_spin_momentum_upload");
  return CsrOperator::adopt(std::move(ctx), h);
}

// ... on a ring of up to 48 sites, with 64-bit states (eigenex_spin_momentum64_upload(_z)).  SpinMomentumCorrelationSolver
// (spin_correlations.hpp) measures a state of either handle; no Sz-sector operator exists beyond 32 sites to expand into.
inline std::shared_ptr<CsrOperator> spinHalfMomentum64Operator(std::shared_ptr<Context> ctx, const SpinHalfModel& model, int nUp, int m, int cell = 1,
                                                               bool complexStates = false) {
  model.requireNoTransverseField("device::spinHalfMomentum64Operator");
  eigenex_csr_t h = nullptr;
  if (complexStates)
    check(eigenex_spin_momentum64_upload_z(ctx->handle(), model.sites(), nUp, cell, m, model.bonds(), model.siteI(), model.siteJ(), model.jz(),
                                           model.jxy(), model.fieldZ(), &h),
          "eigenex_spin_momentum64_upload_z");
  else
    check(eigenex_spin_momentum64_upload(ctx->handle(), model.sites(), nUp, cell, m, model.bonds(), model.siteI(), model.siteJ(), model.jz(),
                                         model.jxy(), model.fieldZ(), &h),
          "eigenex_spin_momentum64_upload");
  return CsrOperator::adopt(std::move(ctx), h);
}

}  // namespace device
}  // namespace EigenEx
}  // namespace cmpt
