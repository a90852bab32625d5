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
#pragma once

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

}  // namespace device
}  // namespace EigenEx
}  // namespace cmpt
