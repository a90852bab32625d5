// Body of k_spmv_rows, k_spmv_rows_cheb and k_spmv_rows_moments (kernels.hip), a list of statements #included inside these kernels.
// The includer defines, as parameters or as constants in front of the #include, every name the body uses:
//   REC (template parameter: record bytes, 8 or 16), op (RowCodeView),
//   x_ext, scale_ptr, shift, y, u_out, n, ntiles, partials, spmv_flags, pass, ctrl, fin (InlineFin), ab (InlineArnoldiBegin),
//   tile_list                                         -- the arguments of k_spmv_rows, with their meaning there
//   CHEB (constexpr bool), ch (ChebStep)              -- CHEB: the epilogue takes a Chebyshev step from the row sum (cheb_store)
//                                                        instead of storing it to y and adding to the partial dot; ch is read
//                                                        only then
//   MOM (constexpr bool), mo (MomentStep)             -- MOM: the epilogue takes a moments step from the row sum (moment_store)
//                                                        and adds its two partial dots, partials[block] and
//                                                        partials[mo.pstride + block]; mo is read only then
// k_spmv_rows_cheb passes y = partials = nullptr, pass = 0 and empty fin / ab as constants: the hooks, the carry and the partial dots
// fold away at compile time; k_spmv_rows_moments passes y = u_out = nullptr, pass = 0 and empty fin / ab likewise.  A name added to the
// body has to be added to ALL includers (and to this list).
  constexpr int W = REC / 8, S = REC;  // 64-bit words and slots per record
  __shared__ double pal[kRowCodeMaxValues];
  __shared__ double lds4[4];
  if (ctrl->stopped) return;
  for (int i = threadIdx.x; i < op.npal; i += kBlock) pal[i] = op.pal[i];
  double scale = (scale_ptr && !ab.ctrl) ? *scale_ptr : 1.0;
  if (ab.ctrl) {
    double res, nrm2b;
    int kb;
    const bool stop = arnoldi_begin_inline(ab, &scale, lds4, &res, &nrm2b, &kb);
    __syncthreads();
    if (blockIdx.x == 0) arnoldi_begin_record(ab, stop, scale, res, nrm2b, kb);
    if (stop) return;
  }
  if (fin.partials) {  // as in k_spmv
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
  __syncthreads();  // the palette
  const int tid = threadIdx.x;
  double dot = 0.0, dot2 = 0.0;  // dot2: MOM only
  const TileRange tr = spmv_tiles(ntiles, spmv_flags & 1);
  auto tile_of = [&](int64_t slot) { return tile_list ? (int64_t)tile_list[slot] : slot; };
  // records exist for every row of every tile (rows behind n: all slots absent), so the loads need no row test
  uint64_t rec[W], nrec[W];
  int64_t tile = tr.first < tr.end ? tile_of(tr.first) : 0;
  if (tr.first < tr.end) row_code_load<REC>(op.rec, tile * kSpmvRows + tid, rec);
  for (int64_t slot = tr.first; slot < tr.end; slot += tr.step) {
    const int64_t r = tile * kSpmvRows + tid;
    // branch-free, so that all gathers are in flight at once: an absent slot (also every slot behind the table's) loads
    // x_ext[0] and its sum is dropped
    double xs[S];
#pragma unroll
    for (int s = 0; s < S; ++s) xs[s] = x_ext[row_code_byte(rec, s) != kRowCodeAbsent ? r + op.slots.off[s] : 0];
    // the next tile's record, behind the gathers
    const int64_t nslot = slot + tr.step;
    const int64_t ntile = nslot < tr.end ? tile_of(nslot) : 0;
    if (nslot < tr.end) row_code_load<REC>(op.rec, ntile * kSpmvRows + tid, nrec);
    double sum = 0.0;
#pragma unroll
    for (int s = 0; s < S; ++s) {  // stored order, multiply then add
      const unsigned c = row_code_byte(rec, s);
      const bool here = c != kRowCodeAbsent;
      const double t = add_product_nofma(sum, pal[here ? c : 0], xs[s] * scale);
      sum = here ? t : sum;
    }
    if (r < n) {
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
        __builtin_nontemporal_store(yr, &y[r]);
        if (u_out) __builtin_nontemporal_store(xr, &u_out[r]);
        dot = (pass & kPassSelfNorm) ? fma(yr, yr, dot) : fma(xr, yr, dot);
      }
    }
#pragma unroll
    for (int w = 0; w < W; ++w) rec[w] = nrec[w];
    tile = ntile;
  }
  if (partials) {
    dot = block_sum(dot, lds4);
    if (tid == 0) partials[blockIdx.x] = dot;
    if constexpr (MOM) {
      dot2 = block_sum(dot2, lds4);
      if (tid == 0) partials[mo.pstride + blockIdx.x] = dot2;
    }
  }
