// Body of k_spmv, k_spmv_cheb and k_spmv_moments (kernels.hip), a list of statements #included inside these kernels.
// The includer defines, as parameters or as constants in front of the #include, every name the body uses:
//   LONG_ROWS, OFF, NT (template parameters)          -- as documented at k_spmv
//   rowptr, col_all, val_all,
//   x_ext, scale_ptr, shift, y, u_out, n, ntiles, partials, spmv_flags, pass, ctrl, fin (InlineFin), ab (InlineArnoldiBegin),
//   tile_list                                         -- the arguments of k_spmv, with their meaning there
//   CHEB (constexpr bool), ch (ChebStep)              -- CHEB: the epilogue takes a Chebyshev step from the row sum (cheb_store)
//                                                        instead of storing it to y and adding to the partial dot; ch is read
//                                                        only then
//   MOM (constexpr bool), mo (MomentStep)             -- MOM: the epilogue takes a moments step from the row sum (moment_store)
//                                                        and adds its two partial dots, partials[block] and
//                                                        partials[mo.pstride + block]; mo is read only then
// k_spmv_cheb passes y = partials = nullptr, pass = 0 and empty fin / ab as constants: the hooks, the carry and the partial dots
// fold away at compile time; k_spmv_moments passes y = u_out = nullptr, pass = 0 and empty fin / ab likewise.  A name added to the
// body has to be added to ALL includers (and to this list).
  // tile_list != nullptr: the launch covers the ntiles tiles tile_list[0 .. ntiles) instead of 0 .. ntiles (r3: the interior
  // rows of a shard run while the halo is still on its way, the tiles that read halo columns afterwards; library.hip)
  __shared__ double prod[kSpmvProdSlots];
  __shared__ double lds4[4];
  if (ctrl->stopped) return;
  double scale = (scale_ptr && !ab.ctrl) ? *scale_ptr : 1.0;
  if (ab.ctrl) {
    double res, nrm2b;
    int kb;
    const bool stop = arnoldi_begin_inline(ab, &scale, lds4, &res, &nrm2b, &kb);
    __syncthreads();  // everybody has read the control block before workgroup 0 changes it (other workgroups: the values written are the ones they derived)
    if (blockIdx.x == 0) arnoldi_begin_record(ab, stop, scale, res, nrm2b, kb);
    if (stop) return;
  }
  if (fin.partials) {  // beta_k, the breakdown test and the scale of the operator input (lanczos.hpp:429-439), taken here
    const double nrm2 = inline_fin_sum(fin, lds4);
    const double nrm = sqrt(nrm2);
    const bool stop = fin.mode == kFinInit ? nrm < fin.threshold : nrm <= fin.threshold;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      fin.out[0] = nrm2;
      fin_norm_apply(fin.ctrl, nrm2, fin.threshold, fin.mode, fin.series);
    }
    if (stop) return;
    scale = 1.0 / nrm;
  }
  const int tid = threadIdx.x;
  double dot = 0.0, dot2 = 0.0;  // dot2: MOM only
  constexpr bool nt = NT;  // flags: bit 0 = XCD-contiguous tiles, bit 1 = cache policy of the val/col streams (NT, chosen by the launcher)
  const TileRange tr = spmv_tiles(ntiles, spmv_flags & 1);
  // row pointers of a tile: fetched one tile ahead, so that their latency is not part of the chain
  // rowptr -> val/col -> x that every tile otherwise pays in sequence
  constexpr bool kWide = sizeof(OFF) > 4;
  auto tile_rows = [&](int64_t slot, int& rs, int& re, int& p0, int& p1, int64_t& base, int64_t& tile) {
    rs = re = p0 = p1 = 0;
    base = 0;
    tile = slot;
    if (slot >= tr.end) return;
    if (tile_list) tile = tile_list[slot];
    const int64_t r0 = tile * kSpmvRows, r = r0 + tid;
    const OFF first = rowptr[r0];
    if (kWide) base = (int64_t)first & ~(int64_t)3;
    if (r < n) {
      rs = (int)(rowptr[r] - (OFF)base);
      re = (int)(rowptr[r + 1] - (OFF)base);
    }
    const int64_t rend = (r0 + kSpmvRows < n) ? r0 + kSpmvRows : n;
    p0 = (int)(first - (OFF)base);
    p1 = (int)(rowptr[rend] - (OFF)base);
  };
  int rs, re, p0, p1;
  int64_t base, tile;
  tile_rows(tr.first, rs, re, p0, p1, base, tile);
  for (int64_t slot = tr.first; slot < tr.end; slot += tr.step) {
    const int64_t r = tile * kSpmvRows + tid;
    int nrs, nre, np0, np1;
    int64_t nbase, ntile;
    tile_rows(slot + tr.step, nrs, nre, np0, np1, nbase, ntile);
    const int32_t* __restrict__ col = col_all + base;
    const double* __restrict__ val = val_all + base;
    const int pa = spmv_aligned_start(p0);  // int4 / double2 loads
    double sum = ((pass & kPassCarry) && r < n) ? y[r] : 0.0;  // column-blocked: carry the row sum from pass to pass
    for (int cb = pa; cb < p1; cb += kSpmvChunk) {
      const int cend = spmv_chunk_end(cb, p1);
      // phase 1: a chunk is two rounds of 4 entries per lane; all six 16-byte loads are issued before
      // the first use, then the eight gathers.  Entries outside [p0, p1) are valid neighbours' entries
      // or the zero padding behind nnz; their products are written but never read.
      const SpmvLaneLoads ll = spmv_lane_loads(cb, cend, tid);
      const int q0 = ll.q0, q1 = ll.q1;
      const bool in0 = ll.in0, in1 = ll.in1;
      int4 ca = make_int4(0, 0, 0, 0), cbv = make_int4(0, 0, 0, 0);
      double2 a01 = make_double2(0.0, 0.0), a23 = a01, b01 = a01, b23 = a01;
      if (nt) {  // compile-time: a run-time branch here cost the plain path 6-8 % through its register allocation (r3)
        if (in0) {
          ca = nt_ld_i4(col + q0);
          a01 = nt_ld_d2(val + q0);
          a23 = nt_ld_d2(val + q0 + 2);
        }
        if (in1) {
          cbv = nt_ld_i4(col + q1);
          b01 = nt_ld_d2(val + q1);
          b23 = nt_ld_d2(val + q1 + 2);
        }
      } else {
        if (in0) {
          ca = *reinterpret_cast<const int4*>(col + q0);
          a01 = ld2(val + q0);
          a23 = ld2(val + q0 + 2);
        }
        if (in1) {
          cbv = *reinterpret_cast<const int4*>(col + q1);
          b01 = ld2(val + q1);
          b23 = ld2(val + q1 + 2);
        }
      }
      if (in0) {
        const double x0 = x_ext[ca.x] * scale, x1 = x_ext[ca.y] * scale;
        const double x2 = x_ext[ca.z] * scale, x3 = x_ext[ca.w] * scale;
        const int li = skew(q0 - cb);  // 4 consecutive entries never straddle a multiple of 32
        prod[li + 0] = a01.x * x0;
        prod[li + 1] = a01.y * x1;
        prod[li + 2] = a23.x * x2;
        prod[li + 3] = a23.y * x3;
      }
      if (in1) {
        const double x0 = x_ext[cbv.x] * scale, x1 = x_ext[cbv.y] * scale;
        const double x2 = x_ext[cbv.z] * scale, x3 = x_ext[cbv.w] * scale;
        const int li = skew(q1 - cb);
        prod[li + 0] = b01.x * x0;
        prod[li + 1] = b01.y * x1;
        prod[li + 2] = b23.x * x2;
        prod[li + 3] = b23.y * x3;
      }
      __syncthreads();
      // phase 2: stored order, multiply-then-add
      int lo, hi;
      spmv_row_window(rs, re, cb, cend, &lo, &hi);
      int p = lo;
      // long rows: sixteen LDS reads in flight, then the sixteen adds in stored order (a row of 256 entries spent its time waiting
      // for one read after the other: 413 -> 156 us at 30,000 rows x 256 contiguous columns, 41 -> 25 us at 100,000 x 64); rows
      // shorter than 16 entries in the chunk -- the stencils -- take the plain loop below as before
      for (; LONG_ROWS && p + 16 <= hi; p += 16) {
        double t[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) t[i] = prod[skew(p + i - cb)];
#pragma unroll
        for (int i = 0; i < 16; ++i) sum = sum + t[i];
      }
      for (; p < hi; ++p) sum = sum + prod[skew(p - cb)];
      __syncthreads();
    }
    if ((pass & kPassNotLast) && r < n) {
      y[r] = sum;
    } else if (r < n) {
      const double xr = x_ext[r] * scale;
      double yr = sum;
      if (shift != 0.0) yr = add_product_nofma(yr, shift, xr);  // lanczos.hpp:390-392
      if constexpr (MOM) {
        const double t = moment_store(mo, r, yr);
        dot = fma(t, t, dot);
        dot2 = fma(t, xr, dot2);
      } else if constexpr (CHEB) {
        cheb_store(ch, r, yr, xr);
        if (u_out) __builtin_nontemporal_store(xr, &u_out[r]);
      } else {
        __builtin_nontemporal_store(yr, &y[r]);  // results of a pass over the whole operator: nothing here reads them again
        if (u_out) __builtin_nontemporal_store(xr, &u_out[r]);
        dot = (pass & kPassSelfNorm) ? fma(yr, yr, dot) : fma(xr, yr, dot);
      }
    }
    rs = nrs, re = nre, p0 = np0, p1 = np1, base = nbase, tile = ntile;
  }
  if (partials) {
    dot = block_sum(dot, lds4);
    if (tid == 0) partials[blockIdx.x] = dot;
    if constexpr (MOM) {
      dot2 = block_sum(dot2, lds4);
      if (tid == 0) partials[mo.pstride + blockIdx.x] = dot2;
    }
  }
