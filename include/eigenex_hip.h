/* eigenex_hip.h -- C ABI of the MI355X (gfx950) Krylov step library.
 *
 * This is the drop-in boundary for the hot path of versmc/cmpt-eigenex: the
 * vector work that LanczosBase::updateLanczosSteps() (reference
 * include/cmpt/eigen_ex/lanczos.hpp:371-457) and ArnoldiBase::updateArnoldiSteps()
 * (include/cmpt/eigen_ex/arnoldi.hpp:312-392) perform through Eigen on host
 * vectors, plus a CSR realisation of the operator callback
 * (MatMulFunction, lanczos.hpp:116).  The header-only C++ solver classes in
 * cmpt-eigenex_amd/include/cmpt/eigen_ex/ call ONLY these entry points; a
 * reference maintainer would bind the same symbols.
 *
 * Conventions
 *   - plain C, opaque handles, no C++/torch types; every function returns an
 *     int status: 0 = ok, negative = error (eigenex_last_error() has the text).
 *   - scalars are fp64, real or complex: complex data (the *_z entry points, or any basis created
 *     complex) are interleaved (re, im) pairs, i.e. the memory layout of std::complex<double>,
 *     passed as double*; alpha, beta, norms, thresholds and the Lanczos shift are always real.
 *     Indices int32 (per-shard nnz < 2^31); sizes int64.
 *   - a context owns ONE HIP stream; every call on its handles is ordered on
 *     that stream.  Calls that return scalars/vectors to the host synchronise;
 *     the *_enqueue calls do not.
 *   - rows of the operator and of every Krylov vector are partitioned 1-D into
 *     contiguous shards (eigenex_partition).  A context created with
 *     eigenex_context_create owns one shard per process (RCCL over xGMI between
 *     processes); eigenex_context_create_loopback owns all shards of a
 *     partition in one process on one device (verification transport: the same
 *     kernels, halo lists and reduction points, device copies instead of RCCL).
 *   - host pointers passed to upload/download calls cover the rows this context
 *     owns: one shard in RCCL mode, all rows in loopback mode.
 *   - threading: like the reference's solver objects, handles are not thread-safe: use a context and
 *     everything created from it from one host thread at a time (eigenex_last_error() is per thread);
 *     different contexts may be driven from different threads.
 */
#ifndef EIGENEX_HIP_H
#define EIGENEX_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EIGENEX_VERSION 100

typedef struct eigenex_context_s* eigenex_context_t;
typedef struct eigenex_csr_s* eigenex_csr_t;     /* device CSR operator (row shards + halo plan) */
typedef struct eigenex_basis_s* eigenex_basis_t; /* Krylov state: basis slab V, work vectors, coefficients */
typedef struct eigenex_plan_s* eigenex_plan_t;   /* host-only plan of one row shard (no GPU needed) */

/* status codes */
enum {
  EIGENEX_OK = 0,
  EIGENEX_ERR_ARG = -1,     /* invalid argument */
  EIGENEX_ERR_HIP = -2,     /* HIP runtime error */
  EIGENEX_ERR_RCCL = -3,    /* RCCL error */
  EIGENEX_ERR_STATE = -4,   /* call not valid in the current state (e.g. capacity exhausted) */
  EIGENEX_ERR_NODEVICE = -5 /* no usable GPU */
};

/* orthogonalisation scheme used by the fused step functions */
enum {
  /* batched classical Gram-Schmidt: one pass of dots against all selected basis
   * vectors, one all-reduce, one update pass (north star: "batched dots + AXPY") */
  EIGENEX_ORTHO_BATCHED = 0,
  /* strictly sequential modified Gram-Schmidt, the reference's operation order
   * (lanczos.hpp:416-418, arnoldi.hpp:380-383): one dot + one axpy per vector */
  EIGENEX_ORTHO_SEQUENTIAL = 1,
  /* batched Gram-Schmidt applied twice per step ("twice is enough"): for steps whose coefficients are
   * not small, e.g. the first step after a thick restart; doubles the traffic over the basis */
  EIGENEX_ORTHO_BATCHED_TWICE = 2,
  /* batched Gram-Schmidt with a second pass only when the first one cancelled too much of the vector
   * (||w_after|| < ||w_before|| / sqrt 2, Daniel-Gragg-Kaufman-Stewart), decided ON THE DEVICE: the second-pass
   * kernels are always enqueued and return at once when not needed.  Meant for the Arnoldi step, whose vector
   * A q_k has O(1) components along the basis: a single classical pass loses orthogonality completely once Ritz
   * values converge (measured: |V^T V - I| = 1 on a 16^3 Laplacian at m = 150; the reference's modified
   * Gram-Schmidt: 0.43; this scheme and BATCHED_TWICE: 3e-16).  Lanczos steps (the three-term recurrence has
   * removed the large components already) treat it as BATCHED; where ||w_before|| is not at hand (host-callback
   * operators, the start vector's deflation) it acts as BATCHED_TWICE. */
  EIGENEX_ORTHO_BATCHED_ADAPTIVE = 3
};

/* vector references inside a basis (arguments named *_ref) */
#define EIGENEX_VEC_COL(c) ((int)(c))        /* basis vector c (lanczosvectors_[c] / arnoldivectors_[c]) */
#define EIGENEX_VEC_V (-1)                    /* v_: holds A*u (lanczos.hpp:237, arnoldi.hpp:185) */
#define EIGENEX_VEC_W (-2)                    /* work vector that feeds the operator (with halo space) */
#define EIGENEX_VEC_START (-3)                /* device-resident copy of initialVector_ (lanczos.hpp:158); survives clear */
#define EIGENEX_VEC_ORTHO(q) (-16 - (int)(q)) /* orthogonalizingVectors_[q] (lanczos.hpp:153) */

/* operator callback for operators that live in host code: the reference's
 * MatMulFunction  std::function<void(const Scalar*, Scalar*)>  (lanczos.hpp:116)
 * plus a user pointer. `out` must be fully overwritten. */
typedef void (*eigenex_matvec_fn)(const double* in, double* out, void* user);

/* ---- library ---------------------------------------------------------- */
int eigenex_version(void);
const char* eigenex_last_error(void);
int eigenex_device_count(int* count);

/* rows [*begin, *end) of shard `shard` out of `nshards` for n_global rows */
int eigenex_partition(int64_t n_global, int nshards, int shard, int64_t* begin, int64_t* end);

/* Halo plan of one row shard, host only (no GPU needed): given the shard's CSR
 * column indices (GLOBAL numbering) returns the sorted unique remote columns
 * (halo slot s holds global column halo_cols[s]) and per-owner counts.
 * Call with halo_cols == NULL to query *n_halo first.  Mirrors what
 * eigenex_csr_upload does internally; exposed for the CPU (gloo) tests. */
int eigenex_halo_plan(int64_t n_global, int nshards, int shard, int64_t nnz, const int32_t* col_global,
                      int64_t* n_halo, int32_t* halo_cols, int64_t* count_per_owner /* nshards */);

/* ---- shard plan on the host --------------------------------------------------
 * The host-side half of eigenex_csr_upload, callable without a GPU: local/halo column numbering, receive segments,
 * and -- once the owners have been told which rows are wanted (what exchange_send_lists_rccl ships over RCCL) -- the
 * send segments.  The sharded upload runs exactly this code; tests/test_multirank_gloo.py drives it across real
 * processes.  rowptr/col_global: the shard's rows as for eigenex_csr_upload (rowptr relative to the first row). */
int eigenex_plan_create(int64_t n_global, int nshards, int shard, const int32_t* rowptr, const int32_t* col_global,
                        eigenex_plan_t* out);
int eigenex_plan_destroy(eigenex_plan_t plan);
/* rows, padded rows (= index of the first halo slot), stored entries, halo slots, segments, rows to send (after the
 * eigenex_plan_add_request calls); any pointer may be NULL */
int eigenex_plan_sizes(eigenex_plan_t plan, int64_t* n_local, int64_t* n_pad, int64_t* nnz, int64_t* n_halo, int* n_recv,
                       int* n_send, int64_t* n_send_rows);
/* local column of every stored entry: [0, n_local) own rows, n_pad + s = halo slot s */
int eigenex_plan_local_columns(eigenex_plan_t plan, int32_t* lcol);
/* r3: the shard's 256-row tiles that read no halo column (interior) and those that read at least one (boundary), ascending --
 * the two launches of a plain CSR operator between shards: the interior tiles need nothing from the neighbour exchange and may
 * run beside it (eigenex_context_set_halo_overlap).  Either array may be NULL (counts only). */
int eigenex_plan_tiles(eigenex_plan_t plan, int32_t* interior, int64_t* n_interior, int32_t* boundary, int64_t* n_boundary);
/* global column of every halo slot (ascending: grouped by owner) */
int eigenex_plan_halo_columns(eigenex_plan_t plan, int32_t* cols_global);
/* receive segment i: halo slots [offset[i], offset[i]+count[i]) come from shard peer[i]; the request to that owner is
 * halo_columns[offset[i] .. offset[i]+count[i]) */
int eigenex_plan_recv_segments(eigenex_plan_t plan, int32_t* peer, int64_t* offset, int64_t* count);
/* install the request of shard `from_shard` (global row numbers this shard owns), in rank order as the upload does */
int eigenex_plan_add_request(eigenex_plan_t plan, int from_shard, const int32_t* rows_global, int64_t count);
/* send segment i: rows send_rows[offset[i] .. +count[i]) go to shard peer[i]; contig_start[i] >= 0 when they are the
 * consecutive local rows contig_start[i].. (sent straight out of the vector, no pack kernel) */
int eigenex_plan_send_segments(eigenex_plan_t plan, int32_t* peer, int64_t* offset, int64_t* count, int64_t* contig_start);
int eigenex_plan_send_rows(eigenex_plan_t plan, int32_t* local_rows);

/* Collectives that ONE call of the Lanczos step driver (eigenex_lanczos_enqueue) issues between shards, in order:
 * ops[i] = EIGENEX_COLL_ALLREDUCE with counts[i] doubles, or EIGENEX_COLL_HALO (neighbour exchange of the operator
 * input).  call_index counts calls since eigenex_basis_clear; *alpha_pending carries the state of the alpha fusion from
 * call to call (start with 0).  Host only; a GPU test holds it against eigenex_context_trace of the real driver. */
enum { EIGENEX_COLL_ALLREDUCE = 1, EIGENEX_COLL_HALO = 2 };
int eigenex_lanczos_collectives(int call_index, int last_in_batch, int* alpha_pending, int64_t interval, int n_ortho,
                                int ortho_mode, int alpha_fusion, int is_complex, int* ops, int* counts, int cap, int* n);

/* ---- context ---------------------------------------------------------- */
/* 128-byte RCCL unique id (rank 0 creates it, the host program broadcasts it). */
int eigenex_rccl_unique_id(void* id128);
/* one process per GPU: this process owns shard `rank` of `world_size`. rccl_id may be NULL iff world_size == 1 */
int eigenex_context_create(int device, int rank, int world_size, const void* rccl_id128, eigenex_context_t* out);
/* all `nshards` shards in this process on `device` (verification transport) */
int eigenex_context_create_loopback(int device, int nshards, eigenex_context_t* out);
int eigenex_context_destroy(eigenex_context_t ctx);
/* runs every RCCL call of the data path once on this context's communicator and stream (all-reduce,
 * all-gather, grouped send/recv ring) and checks the received values; collective. A context created
 * with world_size 1 AND a non-NULL rccl_id owns a 1-rank communicator for this purpose. */
int eigenex_context_selftest(eigenex_context_t ctx, int* ok);
int eigenex_context_sync(eigenex_context_t ctx);
int eigenex_context_info(eigenex_context_t ctx, int* rank, int* world_size, int* nshards_total, int* nshards_local);
/* Between shards the neighbour exchange of the operator input (no counterpart in the reference, which has no
 * collective code) runs on a second stream -- between real ranks on a communicator of its own, ncclCommSplit -- while the
 * operator is applied to the 256-row tiles that read no halo column; the tiles that do wait for it.  on = 0 puts the exchange
 * back in front of the operator on the compute stream: the same launches and the same bits, for comparison.  Returns 1 if the
 * overlap is on afterwards, 0 if off (also when asked for but unavailable: one shard, or no second communicator), < 0 on
 * error.  Between real ranks the first call with on != 0 creates the second communicator: it is COLLECTIVE (every rank
 * must make it).  Default: on for loopback contexts (EIGENEX_NO_HALO_OVERLAP=1 turns that off), OFF between real ranks
 * unless EIGENEX_HALO_OVERLAP=1 is set when the context is created. */
int eigenex_context_set_halo_overlap(eigenex_context_t ctx, int on);
/* what the RCCL communicator itself reports (ncclCommCount / ncclCommUserRank / ncclCommCuDevice): *comm_ranks = 0
 * when the context has no communicator (single GPU, loopback) */
int eigenex_context_comm_info(eigenex_context_t ctx, int* comm_ranks, int* comm_rank, int* comm_device);
/* record (on = 1: from now, forgetting earlier records) the collectives the step drivers enqueue on this context, and
 * read the record back: same encoding as eigenex_lanczos_collectives */
int eigenex_context_trace(eigenex_context_t ctx, int on);
int eigenex_context_trace_get(eigenex_context_t ctx, int* ops, int* counts, int cap, int* n);
/* test hooks, process-wide: the device and pinned-host buffers the library holds now (count, bytes) and the allocations it
 * has made since the process started; eigenex_debug_fail_allocation(n) makes the n-th allocation from now fail with
 * hipErrorOutOfMemory without calling the runtime (0: disarm) */
int eigenex_debug_allocations(int64_t* live, int64_t* live_bytes, int64_t* made);
int eigenex_debug_fail_allocation(int64_t nth);
/* the context's hipStream_t (as void*) */
void* eigenex_context_stream(eigenex_context_t ctx);

/* HIP-event timing of every kernel launch (for bench.py's roofline object).
 * kind: 0 = spmv, 1 = dots, 2 = update, 3 = small (reductions/finalisers), 4 = collectives+copies */
enum { EIGENEX_K_SPMV = 0, EIGENEX_K_DOTS = 1, EIGENEX_K_UPDATE = 2, EIGENEX_K_SMALL = 3, EIGENEX_K_COMM = 4, EIGENEX_K_RITZ = 5, EIGENEX_K_COUNT = 6 };
int eigenex_profile_enable(eigenex_context_t ctx, int on);
int eigenex_profile_reset(eigenex_context_t ctx);
/* synchronises; launches, summed milliseconds and summed algorithmic bytes of one kind */
int eigenex_profile_get(eigenex_context_t ctx, int kind, int64_t* launches, double* total_ms, double* total_bytes);

/* ---- operator ---------------------------------------------------------- */
/* CSR rows owned by this context (RCCL: rows [row_begin, row_begin+n_rows) must equal
 * eigenex_partition(n_global, world, rank); loopback: row_begin = 0, n_rows = n_global).
 * rowptr[n_rows+1] is relative to the first passed row, col holds GLOBAL column indices,
 * ascending within a row is not required.  Host arrays are copied. Collective in RCCL mode.
 * Replaces the user lambda behind setMatrixMultiplication (lanczos.hpp:179-188). */
int eigenex_csr_upload(eigenex_context_t ctx, int64_t n_global, int64_t row_begin, int64_t n_rows,
                       const int32_t* rowptr, const int32_t* col_global, const double* val, eigenex_csr_t* out);
/* the same with complex values: val_interleaved[2*nnz] = (re, im) pairs (Scalar = std::complex<double>,
 * the instantiation of the reference's own samples: src/samples/sample_lanczos2.cpp:14, sample_arnoldi.cpp:14) */
int eigenex_csr_upload_z(eigenex_context_t ctx, int64_t n_global, int64_t row_begin, int64_t n_rows,
                         const int32_t* rowptr, const int32_t* col_global, const double* val_interleaved,
                         eigenex_csr_t* out);
/* r3 -- the same with 64-bit row pointers: the reference's Index is 64-bit (lanczos.hpp:108-116), and one MI355X holds shards
 * of more than 2^31 stored entries (768^3: 3.2e9).  Real operators.  Shards below 2^31 - 16384 entries are stored exactly as
 * eigenex_csr_upload stores them (automatic layout included); larger ones as plain CSR with 64-bit row pointers on the
 * device (column indices stay 32-bit: local numbering).  Stands behind setMatrixMultiplication (lanczos.hpp:179) like the others. */
int eigenex_csr_upload64(eigenex_context_t ctx, int64_t n_global, int64_t row_begin, int64_t n_rows, const int64_t* rowptr,
                         const int32_t* col_global, const double* val, eigenex_csr_t* out);
/* Upload with an explicit column-blocking choice.  A column-blocked operator is applied in K passes, pass k
 * holding the entries whose column lies in the k-th slice of the operator input, so that a slice (<= ~2 MB) stays
 * in each XCD's L2 while it is gathered from: 1.5x on a random 32-per-row matrix of 10^6 rows (BASELINE config 3),
 * useless for stencils.  Each row's running sum is carried from pass to pass, so the result is bit-identical to
 * the single-pass row loop whenever the slices are met in stored order along every row (always true for rows
 * with ascending columns); otherwise the entries of a row are added slice by slice (rounding-level difference).
 *   column_blocks = -1  automatic (what eigenex_csr_upload[_z] do): another layout than plain CSR only if the input vector
 *                       exceeds L2, rows are long enough and the gathers are scattered; -3, -2 or blocked passes, in that
 *                       order of preference (the last two only when the result stays bit-identical)
 *   column_blocks = 0,1 never;  2..16: that many passes, unconditionally
 *   column_blocks = -2  column-sorted row tiles (the automatic mode's choice among the bit-identical layouts, real operators): the
 *                       entries of every (4096-row tile, 256 KB input slice) are stored sorted by column, so that the lanes
 *                       of a wave gather from shared 128-byte lines, with a 16-bit slot that restores the row order for
 *                       the sums; one launch, slices walked inside the kernel, bit-identical to the row loop.  Needs a
 *                       real operator with 2..64 slices whose rows meet the slices in stored order; error otherwise
 *   column_blocks = -3  split tiles (what the automatic mode takes, ahead of the column-sorted tiles, for every operator of
 *                       >= 123,000 rows per shard and >= 3e6 entries whose gathers would not coalesce in the plain kernel --
 *                       uniformly random columns, random columns inside a band, ...): one workgroup per (row tile, column group) adds
 *                       column-sorted entries into partial row sums in LDS, a second kernel adds the <= 8 partial sums of a
 *                       row in ascending group order.  The ONLY layout that re-associates a row's sum: y differs from the
 *                       row loop by a few ulp of sum |a_ij x_j| (products are still rounded before they are added), the
 *                       same bits on every run.  1.35x over the column-sorted tiles on BASELINE config 3.  Real and complex
 *                       operators (complex: tiles of 8192 rows; 1.2x over the column-blocked passes on config 3's pattern
 *                       with complex values).  1.3x .. 2.8x over the other layouts from N = 4e5 to 1.6e7 (profiles/r02_layouts.md);
 *                       error if a row has thousands of entries in one column group.  Setting the environment variable
 *                       EIGENEX_EXACT_ROW_SUMS keeps the automatic mode to the layouts that are bit-identical to the row loop */
int eigenex_csr_upload_ex(eigenex_context_t ctx, int64_t n_global, int64_t row_begin, int64_t n_rows,
                          const int32_t* rowptr, const int32_t* col_global, const double* val, int is_complex,
                          int column_blocks, eigenex_csr_t* out);
/* Block-sparse operator in the reference's BlockTensor<Scalar,2> layout (block_tensor.hpp:1193-1206):
 * one direct-sum partition per axis (row_sizes / col_sizes, both adding up to n_global) and dense column-major
 * blocks, block k = sector (qr[k], qc[k]) with leading dimension row_sizes[qr[k]]; absent blocks are zero, an index
 * pair may appear once.  Kept on the device as dense blocks (8 bytes per stored real entry + one column index per
 * block column, no per-entry index) and
 * applied by its own kernel with the summation order of the flattened CSR rows (block by block, columns
 * ascending), i.e. bit-identical to eigenex_csr_upload of the same matrix.  Every rank passes at least the blocks
 * of the sector rows that intersect its rows (others are ignored).  Collective in RCCL mode.  The handle is used
 * like any other operator handle. */
int eigenex_block_upload(eigenex_context_t ctx, int64_t n_global, int n_row_sectors, const int64_t* row_sizes,
                         int n_col_sectors, const int64_t* col_sizes, int64_t nblocks, const int64_t* qr,
                         const int64_t* qc, const double* const* blocks, eigenex_csr_t* out);
/* the same with complex blocks: (re, im) pairs, leading dimension row_sizes[qr[k]] entries */
int eigenex_block_upload_z(eigenex_context_t ctx, int64_t n_global, int n_row_sectors, const int64_t* row_sizes,
                           int n_col_sectors, const int64_t* col_sizes, int64_t nblocks, const int64_t* qr,
                           const int64_t* qc, const double* const* blocks_interleaved, eigenex_csr_t* out);
/* Matrix-free spin-1/2 Hamiltonian on n_sites sites (2..30), full Hilbert space n = 2^n_sites: nothing is stored but a table
 * of a few hundred bytes, row s is worked out from the bits of s by the kernel.  Basis state s has site i up iff bit i of
 * s is set, sigma_i(s) = +1 for up, -1 for down.
 *   H = sum_b [ jz[b] Sz_i Sz_j + (jxy[b]/2)(S+_i S-_j + S-_i S+_j) ] + sum_i hz[i] Sz_i + sum_i hx[i] Sx_i
 * with bond b = (site_i[b], site_j[b]), 0 <= n_bonds <= 64, site_i[b] != site_j[b] (a pair may appear more than once), hz and
 * hx n_sites entries each or NULL.  Row s is this list of entries, in this (summation) order:
 *   1. the diagonal, always stored, column s: d = 0.0; for b ascending d += (sigma_i sigma_j > 0 ? +1 : -1) * (jz[b] * 0.25);
 *      then for i ascending d += sigma_i * (hz[i] * 0.5) -- plain double additions of sign-flipped constants
 *   2. for b ascending with jxy[b] != 0 and different spins on the bond: value jxy[b] * 0.5, column s ^ (1<<i_b | 1<<j_b)
 *   3. for i ascending with hx[i] != 0: value hx[i] * 0.5, column s ^ (1<<i)
 * Products are rounded before they are added, so eigenex_apply is bit-identical to eigenex_csr_upload of eigenex_spin_csr's rows.
 * The handle is used like any other operator handle (layout EIGENEX_LAYOUT_MATRIX_FREE_SPIN, real states only).  Errors
 * (n_sites or n_bonds out of range, a site index out of range, a bond from a site to itself, a coupling or field that is not
 * finite, a context with more than one shard in total) are returned, with a message in eigenex_last_error.  Sharding a
 * matrix-free spin operator needs an exchange of whole vectors for bonds on the top bits: not built, the message says so. */
int eigenex_spin_upload(eigenex_context_t ctx, int n_sites, int n_bonds, const int32_t* site_i, const int32_t* site_j,
                        const double* jz, const double* jxy, const double* hz_or_null, const double* hx_or_null,
                        eigenex_csr_t* out);
/* The rows [row_begin, row_begin + n_rows) of the same model as CSR, in the stored order above: host code, no context, no
 * GPU.  rowptr[n_rows + 1] starts at 0, col holds global columns, *nnz = rowptr[n_rows].  col == val == NULL: only rowptr
 * and *nnz are filled.  This function is the definition the matrix-free kernel is held against. */
int eigenex_spin_csr(int n_sites, int n_bonds, const int32_t* site_i, const int32_t* site_j, const double* jz,
                     const double* jxy, const double* hz_or_null, const double* hx_or_null, int64_t row_begin,
                     int64_t n_rows, int64_t* rowptr, int32_t* col, double* val, int64_t* nnz);
/* The same Hamiltonian in one sector of fixed magnetisation: the states of n_sites sites (2..32) with exactly n_up sites up
 * (0..n_sites), in ascending numerical order.  Row and column r is the rank of a state in that order, dim = C(n_sites, n_up)
 * <= C(32, 16) < 2^31.  The model must conserve total Sz: hx is NULL or all zeros (else an error whose message names the
 * transverse field); every other check is that of eigenex_spin_upload.  Row r is row s = state(r) of the full-space
 * definition above -- the same entries, values and summation order -- with every column s' replaced by rank(s'): the sector
 * matrix is the full-space matrix restricted to the sector, bit for bit.
 *   eigenex_spin_sector_dim     dim
 *   eigenex_spin_sector_states  the states of ranks first .. first + count - 1 (to scatter a sector vector into the full space)
 *   eigenex_spin_sector_csr     rows [row_begin, row_begin + n_rows) (ranks) as CSR, arguments as eigenex_spin_csr
 * are host code: no context, no GPU.
 *   eigenex_spin_sector_upload  the matrix-free operator (layout EIGENEX_LAYOUT_MATRIX_FREE_SPIN_SECTOR, real states, a context
 *                               with one shard in total): the kernel unranks r and ranks every flipped state through two
 *                               tables of at most 2^16 32-bit words each; no row and no state is stored.  eigenex_apply is
 *                               bit-identical to eigenex_csr_upload of eigenex_spin_sector_csr's rows.  The model is checked
 *                               before the context is touched. */
int eigenex_spin_sector_dim(int n_sites, int n_up, int64_t* dim);
int eigenex_spin_sector_states(int n_sites, int n_up, int64_t first, int64_t count, uint32_t* states);
int eigenex_spin_sector_csr(int n_sites, int n_up, int n_bonds, const int32_t* site_i, const int32_t* site_j, const double* jz,
                            const double* jxy, const double* hz_or_null, const double* hx_or_null, int64_t row_begin,
                            int64_t n_rows, int64_t* rowptr, int32_t* col, double* val, int64_t* nnz);
int eigenex_spin_sector_upload(eigenex_context_t ctx, int n_sites, int n_up, int n_bonds, const int32_t* site_i,
                               const int32_t* site_j, const double* jz, const double* jxy, const double* hz_or_null,
                               const double* hx_or_null, eigenex_csr_t* out);
/* The same two matrix-free operators for COMPLEX states (real-time evolution exp(-iHt)|psi>): the same arguments, checks and
 * error messages (under their own names), the same layout and tables, the same real Hamiltonian; only the scalar type of the
 * handle is complex.  eigenex_basis_create on such a handle gives a complex state, eigenex_basis_create_ex(is_complex = 0) is
 * refused by the scalar-type check; a handle of eigenex_spin_upload / eigenex_spin_sector_upload keeps refusing is_complex = 1.
 * An application to x = a + ib (interleaved) is the real kernel's result on a and on b, the row walked once: each part has the
 * real kernel's products, rounded and added in its order (with a shift only the sign of a zero may differ); a complex shift
 * (eigenex_basis_configure_z) is a plain complex multiply added last.  The dot is conj(x) . y.  eigenex_spin_geometry,
 * eigenex_csr_info, eigenex_csr_layout and eigenex_csr_encoding answer as for the real handles.  On a complex spin state:
 *   eigenex_spin_measure                             the Hermitian sums, see below
 *   eigenex_spin_rdm_z                               the reduced density matrix M M^H, see below
 *   eigenex_spin_site_apply_z                        a sum of site operators with complex coefficients, see below
 *   eigenex_spin_rdm, eigenex_spin_site_apply        EIGENEX_ERR_STATE, "real states only", before anything is allocated
 *                                                    (the messages name eigenex_spin_rdm_z and eigenex_spin_site_apply_z)
 *   eigenex_basis_set_filter, eigenex_filter_apply,  supported: a complex state takes the streaming form of the Chebyshev step,
 *   eigenex_kpm_moments, eigenex_kpm_trace_moments   whose real coefficients act on both parts alike and whose dots are the real
 *                                                    parts of the Hermitian ones, which is all a Hermitian operator's moments
 *                                                    need; the operator kernel supplies (H - center) t_k, u_out and the scale as
 *                                                    every other complex operator kernel does.  Tested against the complex CSR
 *                                                    upload of the same rows. */
int eigenex_spin_upload_z(eigenex_context_t ctx, int n_sites, int n_bonds, const int32_t* site_i, const int32_t* site_j,
                          const double* jz, const double* jxy, const double* hz_or_null, const double* hx_or_null,
                          eigenex_csr_t* out);
int eigenex_spin_sector_upload_z(eigenex_context_t ctx, int n_sites, int n_up, int n_bonds, const int32_t* site_i,
                                 const int32_t* site_j, const double* jz, const double* jxy, const double* hz_or_null,
                                 const double* hx_or_null, eigenex_csr_t* out);
/* The same Hamiltonian in one MOMENTUM sector of a sector of fixed magnetisation.  NOT part of the reference.  The model must
 * conserve total Sz (no hx argument: a transverse field has no Sz sector) and be invariant under the translation T by `cell`
 * sites, site i -> (i + cell) mod n_sites: cell divides n_sites, 1 <= cell <= n_sites / 2, N = n_sites / cell translations.  The
 * multiset of (unordered bond, jz, jxy), couplings compared bit for bit, must map onto itself under T and hz[i] must equal
 * hz[(i + cell) mod n_sites]; otherwise EIGENEX_ERR_ARG with a message that names the first bond or site that breaks the
 * symmetry.  momentum = m in 0..N-1 stands for k = 2 pi m / N.
 *   rows      A state s has period R_s, the smallest R >= 1 with T^R s = s.  The rows are the numerically smallest states
 *             ("representatives") a of the orbits of the Sz sector with (m R_a) mod N == 0, ascending; dim < 2^31.  A sector
 *             without such a state (n_up = 0 at m = 1) is refused with EIGENEX_ERR_ARG and a message that says so.
 *   basis     |a(k)> = (sqrt(R_a) / N) sum_{r<N} e^{-ikr} T^r |a>
 *   row a     in stored (= summation) order: the diagonal d(a) of eigenex_spin_upload's definition, always stored, at column
 *             idx(a); then for b ascending over the bonds with jxy[b] != 0 and different spins on the bond, with s' = a ^ mask_b,
 *             j* the smallest j >= 0 with T^j s' = rep(s') and l = (N - j*) mod N: nothing if (m R_s') mod N != 0, else the
 *             value c * phase[l] at column idx(rep(s')), c = (jxy[b] * 0.5) * sqrt((double)R_a / (double)R_s') with each product
 *             rounded, phase[l] = e^{-2 pi i ((m l) mod N) / N} -- exactly 1, -i, -1, i where 4 ((m l) mod N) is a multiple of N
 *             -- value.re = c * phase.re, value.im = c * phase.im.  Terms are never merged: two terms of a row that reach the
 *             same column stay two entries.
 *   real      m == 0 or 2 m == N: every value.im is exactly 0 and the operator is real symmetric.  Real momenta may be used
 *             with real states, every other momentum needs complex states.
 *   expand    maps a momentum vector x to the vector y of the Sz sector (the rows of eigenex_spin_sector_upload): for a sector
 *             state s with b = rep(s) = T^{j*} s, y[rank(s)] = x[idx(b)] * phase[(N - j*) mod N] * (1 / sqrt((double)R_b)) if b
 *             is a row of the sector, else 0; the first product is a plain complex multiply (of a real vector x * phase.re), the
 *             second scales each part.  It preserves the norm, and H_sector expand(x) = expand(H_k x).
 *   eigenex_spin_momentum_dim     dim
 *   eigenex_spin_momentum_states  the representatives of rows first .. first + count - 1 and, unless NULL, their periods
 *   eigenex_spin_momentum_csr     rows [row_begin, row_begin + n_rows) as CSR, arguments as eigenex_spin_sector_csr but val holds
 *                                 interleaved (re, im) pairs: 2 * nnz doubles
 *   eigenex_spin_momentum_expand_host  expand in host code: x and y hold 1 (is_complex = 0; real momenta only) or 2 doubles per row
 * are host code: no context, no GPU.
 *   eigenex_spin_momentum_upload    the matrix-free operator for real states, real momenta only (layout
 *                                   EIGENEX_LAYOUT_MATRIX_FREE_SPIN_MOMENTUM, a context with one shard in total).  The device holds
 *                                   the ascending list of representatives, 4 bytes per row, and a table of 2^(n_sites / 2) + 1
 *                                   words that brackets the search for a column; a row's own state is one coalesced load, the
 *                                   orbit of every flipped state is walked in registers.  eigenex_apply is bit-identical to
 *                                   eigenex_csr_upload of the real parts of eigenex_spin_momentum_csr's rows.  eigenex_csr_info
 *                                   reports nnz_local = 0.
 *   eigenex_spin_momentum_upload_z  the same for complex states, any momentum: bit-identical to eigenex_csr_upload_z of
 *                                   eigenex_spin_momentum_csr's rows.  Lanczos, the Chebyshev filter and the KPM moments run on
 *                                   either handle as on every other operator.
 *   eigenex_spin_momentum_geometry  n_sites, n_up, cell and momentum of such a handle; EIGENEX_ERR_STATE for any other handle.
 *                                   Every output may be NULL.
 *   eigenex_spin_momentum_expand    expand on the device: x a vector of a state on a momentum handle, y a vector of a state on a
 *                                   handle of eigenex_spin_sector_upload(_z) of the same (n_sites, n_up), the same scalar type
 *                                   and the same context; anything else is EIGENEX_ERR_STATE before anything is allocated.  One
 *                                   launch, bit-identical to eigenex_spin_momentum_expand_host; norm2 = sum |y_r|^2 (may be NULL)
 *                                   is reduced in a fixed order without atomics.  Synchronises once.
 * All argument checks -- geometry, model, and a complex momentum given to eigenex_spin_momentum_upload -- happen before the context
 * is touched.  A row of a momentum handle is an orbit, not a state: eigenex_spin_geometry, eigenex_spin_measure, eigenex_spin_rdm(_z)
 * and eigenex_spin_site_apply(_z) refuse it as they refuse every handle that is not theirs; expand first, or apply site operators
 * in the momentum basis (eigenex_spin_momentum_site_apply, below). */
int eigenex_spin_momentum_dim(int n_sites, int n_up, int cell, int momentum, int64_t* dim);
int eigenex_spin_momentum_states(int n_sites, int n_up, int cell, int momentum, int64_t first, int64_t count, uint32_t* states,
                                 uint8_t* periods_or_null);
int eigenex_spin_momentum_csr(int n_sites, int n_up, int cell, int momentum, int n_bonds, const int32_t* site_i,
                              const int32_t* site_j, const double* jz, const double* jxy, const double* hz_or_null,
                              int64_t row_begin, int64_t n_rows, int64_t* rowptr, int32_t* col, double* val_interleaved, int64_t* nnz);
int eigenex_spin_momentum_upload(eigenex_context_t ctx, int n_sites, int n_up, int cell, int momentum, int n_bonds,
                                 const int32_t* site_i, const int32_t* site_j, const double* jz, const double* jxy,
                                 const double* hz_or_null, eigenex_csr_t* out);
int eigenex_spin_momentum_upload_z(eigenex_context_t ctx, int n_sites, int n_up, int cell, int momentum, int n_bonds,
                                   const int32_t* site_i, const int32_t* site_j, const double* jz, const double* jxy,
                                   const double* hz_or_null, eigenex_csr_t* out);
int eigenex_spin_momentum_geometry(eigenex_csr_t csr, int* n_sites, int* n_up, int* cell, int* momentum);
int eigenex_spin_momentum_expand(eigenex_basis_t src_basis, int x_ref, eigenex_basis_t dst_basis, int y_ref, double* norm2);
int eigenex_spin_momentum_expand_host(int n_sites, int n_up, int cell, int momentum, int is_complex, const double* x, double* y);
/* Momentum sectors of rings of up to 48 sites: the sector above with 64-bit state words.  NOT part of the reference.  Rows,
 * basis, row contents, summation order, the values, the "real momentum" rule and the invariance check are those of
 * eigenex_spin_momentum_upload, word for word; only the limits differ:
 *   n_sites 2..48; n_bonds 0..128 (a J1-J2 ring of 36 sites has 72); n_up, cell and momentum as above; dim < 2^31 still: a
 *   sector with more rows is refused with EIGENEX_ERR_ARG.  A state is a uint64_t with site i at bit i.
 * For n_sites <= 32 and n_bonds <= 64 the three host functions return what their 32-bit namesakes return, byte for byte.
 *   eigenex_spin_momentum64_dim, _states (uint64_t states), _csr   host code: no context, no GPU.  The enumeration cuts the Sz
 *                                   sector by the top 16 bits of the state into chunks that up to 16 threads take in turn, skips a
 *                                   chunk whose prefix alone shows a smaller rotation, and joins the chunks in ascending order:
 *                                   the list is the plain ascending walk's.
 *   eigenex_spin_momentum64_upload(_z)  the matrix-free operator (layout EIGENEX_LAYOUT_MATRIX_FREE_SPIN_MOMENTUM64, a context with
 *                                   one shard in total).  The device holds the representatives at 8 bytes per row and the bucket
 *                                   table, 2^(n_sites - (n_sites + 1) / 2) + 1 words, at most 2^24 + 1.  eigenex_apply is
 *                                   bit-identical to eigenex_csr_upload(_z) of eigenex_spin_momentum64_csr's rows.  All argument
 *                                   checks happen before the context is touched.  Lanczos, the Chebyshev filter and the KPM
 *                                   moments run on the handle as on every other operator.
 * eigenex_spin_momentum_geometry answers for these handles too.  eigenex_spin_momentum_expand refuses them with EIGENEX_ERR_STATE
 * before anything is allocated -- no Sz-sector operator exists beyond 32 sites; for n_sites <= 32 use eigenex_spin_momentum_upload
 * -- and eigenex_spin_geometry, eigenex_spin_measure, eigenex_spin_rdm(_z) and eigenex_spin_site_apply(_z) refuse them as they
 * refuse every handle that is not theirs. */
int eigenex_spin_momentum64_dim(int n_sites, int n_up, int cell, int momentum, int64_t* dim);
int eigenex_spin_momentum64_states(int n_sites, int n_up, int cell, int momentum, int64_t first, int64_t count, uint64_t* states,
                                   uint8_t* periods_or_null);
int eigenex_spin_momentum64_csr(int n_sites, int n_up, int cell, int momentum, int n_bonds, const int32_t* site_i,
                                const int32_t* site_j, const double* jz, const double* jxy, const double* hz_or_null,
                                int64_t row_begin, int64_t n_rows, int64_t* rowptr, int32_t* col, double* val_interleaved, int64_t* nnz);
int eigenex_spin_momentum64_upload(eigenex_context_t ctx, int n_sites, int n_up, int cell, int momentum, int n_bonds,
                                   const int32_t* site_i, const int32_t* site_j, const double* jz, const double* jxy,
                                   const double* hz_or_null, eigenex_csr_t* out);
int eigenex_spin_momentum64_upload_z(eigenex_context_t ctx, int n_sites, int n_up, int cell, int momentum, int n_bonds,
                                     const int32_t* site_i, const int32_t* site_j, const double* jz, const double* jxy,
                                     const double* hz_or_null, eigenex_csr_t* out);
/* Diagonal correlations of a vector x of a momentum sector, without expanding it.  NOT part of the reference.  For a product D of
 * sigma^z over a site mask and a momentum eigenstate x, <D> = sum_a |x_a|^2 (1/N) sum_{r<N} D(T^r a) over the representatives a:
 * D is diagonal and distinct orbits are disjoint, so no cross term appears.  (For a vector that is no momentum eigenstate the sums
 * below are still what is computed; they are then the expectation in the translation average of |x><x|.)  Raw sums, rows ascending:
 *   norm2       = sum_a |x_a|^2              one fma per row of a real x, two of a complex one (real part, then imaginary part)
 *   diag_out[t] = sum_a c_t(a) w_a           one fma per row, fma((double)c_t(a), w_a, diag_out[t]);
 *                                            w_a = x_a * x_a, of a complex element fma(im, im, re * re)
 *   c_t(a)      = sum_{r<N} prod_{i in mask_t} sigma_i(T^r a), an integer in [-N, N]; sigma_i(s) = +1 if bit i of s is set, else -1
 * so that <D_t> = diag_out[t] / (N norm2): <Sz_i Sz_j> = diag{i,j} / (4 N norm2), and for a singlet of an SU(2)-symmetric model
 * <S_i . S_j> = 3 <Sz_i Sz_j>.  masks: 0..1024 64-bit site masks (bit i = site i), none zero, none with a site >= n_sites
 * (EIGENEX_ERR_ARG); n_diag = 0 returns norm2 alone.
 *   eigenex_spin_momentum_measure_host  the definition in host code; x holds 1 (is_complex = 0) or 2 doubles per row of the
 *                                   sector (n_sites up to 48).
 *   eigenex_spin_momentum_measure   on the device, for a vector of a real or complex state on a handle of
 *                                   eigenex_spin_momentum_upload(_z) or eigenex_spin_momentum64_upload(_z); any other handle is
 *                                   EIGENEX_ERR_STATE.  16 masks per sweep: x and the representatives stream once per sweep, no
 *                                   vector is written, partial sums are reduced in a fixed order without atomics, so results are
 *                                   bit-reproducible and a term does not depend on the other masks of the call.  No vector,
 *                                   coefficient or recorded step batch of the state is touched.  Synchronises once. */
int eigenex_spin_momentum_measure(eigenex_basis_t basis, int x_ref, int n_diag, const uint64_t* masks, double* diag_out, double* norm2);
int eigenex_spin_momentum_measure_host(int n_sites, int n_up, int cell, int momentum, int is_complex, const double* x, int n_diag,
                                       const uint64_t* masks, double* diag_out, double* norm2);
/* A sum of site operators that carries a momentum, from one momentum sector into another, without expanding: O_q |psi_k> lies in
 * the sector k - q.  NOT part of the reference.  Conventions as above: L = n_sites, cell a, N = L / a, sector (L, n_up, a, m).
 *   input       the source sector, a kind (EIGENEX_SPIN_SITE_Z / _PLUS / _MINUS), p in 0..N-1 and `cell` complex cell coefficients
 *               cc[j] = (cell_re[j], cell_im[j]); cell_im NULL means zeros.
 *   sites       c[j + a r] = cc[j] * u[r] (a plain complex multiply without contraction), u[r] = e^{+2 pi i ((p r) mod N) / N}, taken
 *               from the phase table of momentum p: exactly 1, i, -1, -i at quarter turns.  O = sum_i c[i] S^kind_i obeys
 *               T O T^-1 = e^{-2 pi i p / N} O.  Site coefficients are never given one by one.
 *   destination n_up' = n_up (Z), n_up + 1 (PLUS), n_up - 1 (MINUS); m' = (m - p + N) mod N.  Both sectors must have rows.
 *   row b       of the destination, b a representative with period R_b; idx, ratio = sqrt(R / R') and phase are the SOURCE's.
 *               Z: y_b = w(b) x[idx(b)] if (m R_b) mod N == 0, else 0; w(b) as in eigenex_spin_site_apply(_z) from c[i] * 0.5.
 *               PLUS / MINUS: y_b = 0, then for i ascending over the sites up (PLUS) or down (MINUS) in b, with s' = b ^ (1 << i),
 *               T^{j*} s' = rep(s'), l = (N - j*) mod N, and only if (m R_s') mod N == 0:
 *               xt = (x[idx(rep(s'))] * phase[l]) * sqrt((double)R_b / (double)R_s') -- the product a plain complex multiply (of a real
 *               vector x * phase.re), then each part scaled -- and y_b takes eigenex_spin_site_apply_z's fmas with c[i]:
 *               y.re = fma(c.re, xt.re, y.re), y.re = fma(-c.im, xt.im, y.re), y.im = fma(c.re, xt.im, y.im), y.im = fma(c.im, xt.re,
 *               y.im), the second of each pair not when every c[i].im is zero.
 *   norm2       sum_b |y_b|^2, the fma of the real part, then of the imaginary part, rows ascending (may be NULL)
 *   identity    expand(y) = (sum_i c[i] S^kind_i) expand(x), with the per-site c[i] given to eigenex_spin_site_apply_z.
 *   real form   m and m' real momenta and every coefficient real: every phase is +-1 or 0 and x and y may be real vectors; each part
 *               of the complex result equals the real call on that part.
 *   eigenex_spin_momentum_site_apply_host  the definition in host code (n_sites 2..48; 32-bit states up to 32 sites, 64-bit
 *                                   above, with equal results): x holds 1 (is_complex = 0; the real form only) or 2 doubles per
 *                                   row of the source, y per row of the destination.  y may be x for Z with p = 0 only.
 *   eigenex_spin_momentum_site_apply     on the device, for two real states; cell_coef holds `cell` doubles.
 *   eigenex_spin_momentum_site_apply_z   on the device, for two complex states; cell_im may be NULL.
 *                                   src and dst are states of one context, both on handles of eigenex_spin_momentum_upload(_z) or
 *                                   both on handles of eigenex_spin_momentum64_upload(_z), with the same n_sites and cell and
 *                                   dst's (n_up, momentum) = (n_up', m'), all read from eigenex_spin_momentum_geometry; the two
 *                                   models need not agree.  The intended y_ref is EIGENEX_VEC_W of dst.  EIGENEX_ERR_STATE: a
 *                                   handle that is no momentum handle, two contexts, two word widths, a state of the other scalar
 *                                   type (the message names the other call), and dst == src for anything but Z with p = 0, where
 *                                   y may be x.  EIGENEX_ERR_ARG: a kind or p out of range, a non-finite coefficient, a
 *                                   destination n_up outside 0..n_sites, sectors that do not belong together.  All of it before
 *                                   anything is allocated.  One launch and a fixed-order reduction without atomics:
 *                                   y is bit-identical to the host function's.  Synchronises once.  No coefficient, counter or
 *                                   recorded step batch of either state is touched.
 * eigenex_spin_site_apply(_z) keep refusing momentum handles; their message names these calls. */
int eigenex_spin_momentum_site_apply(eigenex_basis_t src_basis, int x_ref, eigenex_basis_t dst_basis, int y_ref, int kind, int p,
                                     const double* cell_coef, double* norm2);
int eigenex_spin_momentum_site_apply_z(eigenex_basis_t src_basis, int x_ref, eigenex_basis_t dst_basis, int y_ref, int kind, int p,
                                       const double* cell_re, const double* cell_im, double* norm2);
int eigenex_spin_momentum_site_apply_host(int n_sites, int n_up_src, int cell, int momentum_src, int kind, int p, int is_complex,
                                          const double* cell_re, const double* cell_im, const double* x, double* y, double* norm2);
/* Spin correlations of a real vector x over the rows of a matrix-free spin operator, all terms in one sweep: x is read once
 * per 16 terms of each list and nothing is written but the sums.  A measurement is two lists of 32-bit site masks (bit i = site
 * i); with sigma_i(s) as above it yields the raw, unnormalised sums
 *   norm2       = sum_s x_s^2
 *   diag_out[t] = sum_s (prod_{i in mask} sigma_i(s)) x_s^2              a mask of 1..n_sites bits
 *   flip_out[t] = sum_s [sigma_i(s) != sigma_j(s)] x_s x_{s ^ mask}      a two-bit mask {i, j}
 *   flip_out[t] = sum_s x_s x_{s ^ mask}                                 a one-bit mask {i}: the full space only
 * from which <Sz_i> = diag{i} / (2 norm2), <Sz_i Sz_j> = diag{i,j} / (4 norm2), <Sx_i> = flip{i} / (2 norm2), <Sx_i Sx_j + Sy_i
 * Sy_j> = flip{i,j} / (2 norm2) and <S_i.S_j> = the sum of the last two; a diagonal mask of more bits is a string or parity
 * correlator.  At most 1024 masks per list; duplicates are allowed; empty lists are valid (norm2 alone).  An output pointer whose
 * count is zero may be NULL, norm2 may be NULL.  Errors (EIGENEX_ERR_ARG, message in eigenex_last_error): a zero mask, a site at
 * or above n_sites, a flip mask of neither one nor two bits, a one-bit flip mask in a sector (it does not conserve total Sz),
 * a count out of range, a NULL list with a count.
 *   eigenex_spin_measure       x = any vector reference of a state whose operator handle came from eigenex_spin_upload or
 *                              eigenex_spin_sector_upload: sites, sector and rank tables are the handle's.  Any other operator
 *                              or a host callback: EIGENEX_ERR_STATE.  Runs on the context's stream and synchronises once.  No
 *                              vector of the state, no coefficient, counter or recorded step batch is touched: a Lanczos run may
 *                              be measured between two batches and goes on as if nothing had happened.  No atomics: a result
 *                              depends on the launch grid (eigenex_basis_tune) only through the grouping of partial sums, not on
 *                              the other terms of the call, and is bit-reproducible from run to run.
 *   eigenex_spin_measure_host  the definition the kernel is held against, in host code: no context, no GPU.  n_up = -1: the
 *                              full space (n_sites 2..30, x has 2^n_sites entries); else the sector (n_sites 2..32, x has
 *                              C(n_sites, n_up) entries).  Rows ascending, one fma per term.
 *   complex states             on a state of eigenex_spin_upload_z / eigenex_spin_sector_upload_z, eigenex_spin_measure computes the
 *                              Hermitian sums norm2 = sum_s |x_s|^2, diag_out[t] = sum_s sign |x_s|^2 and flip_out[t] = sum_s
 *                              [predicate] Re(conj(x_s) x_{s ^ mask}), so the normalisations above stay valid; same chunks, same
 *                              fixed-order reduction without atomics.  eigenex_spin_measure_host_z is its host definition: x
 *                              interleaved (re, im), rows ascending, per term the fma of the real parts and then the fma of the
 *                              imaginary parts; with all imaginary parts +0 it returns eigenex_spin_measure_host's bytes.
 *   eigenex_spin_geometry     n_sites and n_up (-1: the full space) of a matrix-free spin operator handle; EIGENEX_ERR_STATE
 *                              for any other handle.  Either output may be NULL. */
int eigenex_spin_measure(eigenex_basis_t b, int x_ref, int n_diag, const uint32_t* diag_masks, int n_flip,
                         const uint32_t* flip_masks, double* diag_out, double* flip_out, double* norm2);
int eigenex_spin_measure_host(int n_sites, int n_up /* -1: full space */, const double* x, int n_diag,
                              const uint32_t* diag_masks, int n_flip, const uint32_t* flip_masks, double* diag_out,
                              double* flip_out, double* norm2);
int eigenex_spin_measure_host_z(int n_sites, int n_up /* -1: full space */, const double* x_interleaved, int n_diag,
                                const uint32_t* diag_masks, int n_flip, const uint32_t* flip_masks, double* diag_out,
                                double* flip_out, double* norm2);
int eigenex_spin_geometry(eigenex_csr_t csr, int* n_sites, int* n_up);
/* The observables of one real vector x against basis columns, <V_j| A_t |x>, for the mask lists and rules of eigenex_spin_measure.
 * With V_j the columns first .. first + count - 1 of the state, raw and unnormalised, rows ascending, one fma per row and sum:
 *   diag_out[t * count + j] = sum_s (prod_{i in mask_t} sigma_i(s)) V_j(s) x_s             <V_j| prod sigma |x>
 *   flip_out[t * count + j] = sum_s [sigma_a(s) != sigma_b(s)] V_j(s) x_{s ^ mask_t}       two bits: <V_j| S+_a S-_b + S-_a S+_b |x>
 *   flip_out[t * count + j] = sum_s V_j(s) x_{s ^ mask_t}                                  one bit, full space only: <V_j| 2 Sx_a |x>
 * With x = column 0 of a Lanczos basis these are the g_i = <v_i| A |v_0> that thermal expectation values by the finite-temperature
 * Lanczos method need; products of site operators, which eigenex_spin_site_apply does not form, are diagonal masks here.
 *   eigenex_spin_measure_columns       x_ref = any vector reference of the state, a basis column included; first and count
 *                              address basis columns as eigenex_dots does with stride 1: count >= 1, first >= 0, first + count <=
 *                              the capacity.  Needs a real state whose operator handle came from eigenex_spin_upload or
 *                              eigenex_spin_sector_upload; a complex state, a momentum handle, a stored operator or a host
 *                              callback is EIGENEX_ERR_STATE, and the message names the handles that are served.  The mask
 *                              errors are eigenex_spin_measure's (EIGENEX_ERR_ARG).  The basis streams past once per 16 terms of
 *                              the longer list; per row the state, the rank-table gathers and the gathered x are taken once for
 *                              every 4 columns.  Runs on the context's stream and synchronises once.  If a batch of one-sweep
 *                              steps has left its newest column pending (eigenex_basis_close_pending) and that column is x_ref or
 *                              lies in the range, it is closed first, as every other entry point would; nothing else of the
 *                              state changes: no vector, coefficient, counter or recorded batch.  No atomics: out[t][j] has
 *                              the same bits whatever other terms and columns share the call, and from run to run.
 *   eigenex_spin_measure_columns_host  the definition in host code: no context, no GPU.  x has the rows of (n_sites, n_up) as
 *                              for eigenex_spin_measure_host, column j is V + j * ldv, ldv >= rows.  With V_j = x a diagonal
 *                              sum has the bits of eigenex_spin_measure_host's diag_out[t]. */
int eigenex_spin_measure_columns(eigenex_basis_t b, int x_ref, int first, int count, int n_diag, const uint32_t* diag_masks,
                                 int n_flip, const uint32_t* flip_masks, double* diag_out, double* flip_out);
int eigenex_spin_measure_columns_host(int n_sites, int n_up /* -1: full space */, const double* x, const double* V, int64_t ldv,
                                      int count, int n_diag, const uint32_t* diag_masks, int n_flip, const uint32_t* flip_masks,
                                      double* diag_out, double* flip_out);
/* A sum of single-site spin operators applied to a real vector, y = O x: the start vector of a dynamical correlation function
 * (Lanczos continued fraction) formed on the device, also where O changes the magnetisation.  NOT part of the reference.  O is a
 * kind and n_sites real coefficients c[i]; x lives on the rows of the source geometry (n_sites, n_up_src; n_up = -1: the full
 * space), y on the destination's.  With sigma_i(s) as above:
 *   EIGENEX_SPIN_SITE_Z      O = sum_i c[i] Sz_i.  y_r = w(s_r) * x_r;  w(s) = 0.0, then for i ascending
 *                            w += sigma_i(s) > 0 ? +(c[i] * 0.5) : -(c[i] * 0.5)  -- plain additions of sign-flipped constants, as
 *                            for the operator's diagonal.  The destination geometry equals the source's.
 *   EIGENEX_SPIN_SITE_PLUS   O = sum_i c[i] S+_i.  Destination: the sector n_up_src + 1; the full space for the full space.  Row
 *                            t of the destination, with state s_t:  y_t = 0.0, then for i ascending with site i up in s_t
 *                            y_t = fma(c[i], x[row_src(s_t ^ 1<<i)], y_t)
 *   EIGENEX_SPIN_SITE_MINUS  O = sum_i c[i] S-_i: the same with "site i down in s_t".  Destination: the sector n_up_src - 1.
 *   norm2 = sum_r y_r^2 comes with every call (host: one fma per row, rows ascending; device: per-workgroup partial sums added in a
 *   fixed order, no atomics, bit-reproducible from run to run); it may be NULL.
 * Errors (EIGENEX_ERR_ARG, message in eigenex_last_error): a kind out of range, a coefficient that is not finite, a destination
 * sector outside 0..n_sites (S+ of the all-up sector, S- of the all-down one), geometries that do not belong together.
 *   eigenex_spin_site_apply       src and dst are states on the SAME context whose operator handles came from eigenex_spin_upload
 *                                 or eigenex_spin_sector_upload and whose geometries (eigenex_spin_geometry) fit the kind; dst may
 *                                 be src.  x_ref is a vector of src, y_ref one of dst; y_ref = EIGENEX_VEC_W of dst is the intended
 *                                 use: that is where a Lanczos run takes its start vector.  For Z, y may be x (in place); for PLUS
 *                                 and MINUS y == x (dst == src in the full space) is refused: the gather reads what it writes.
 *                                 Runs on the context's stream and synchronises once; touches no coefficient, counter or recorded
 *                                 step batch of either state.  Any other operator, a host callback or two different contexts:
 *                                 EIGENEX_ERR_STATE.  Everything is checked before anything is allocated.
 *   eigenex_spin_site_apply_host  the definition the kernel is held against, in host code: no context, no GPU.  x has the source's
 *                                 rows (2^n_sites, n_sites 2..30; or C(n_sites, n_up_src), n_sites 2..32), y the destination's. */
enum { EIGENEX_SPIN_SITE_Z = 0, EIGENEX_SPIN_SITE_PLUS = 1, EIGENEX_SPIN_SITE_MINUS = 2 };
int eigenex_spin_site_apply(eigenex_basis_t src, int x_ref, eigenex_basis_t dst, int y_ref, int kind,
                            const double* coef /* n_sites */, double* norm2 /* or NULL */);
int eigenex_spin_site_apply_host(int n_sites, int n_up_src /* -1: full space */, int kind, const double* coef,
                                 const double* x, double* y, double* norm2);
/* The same of a COMPLEX vector (interleaved (re, im)) with complex coefficients c[i] = (coef_re[i], coef_im[i]): O psi(t) of an
 * evolved state and the operators sum_r exp(iqr) S_r, formed on the device.  NOT part of the reference.  coef_im may be NULL;
 * real_coef = coef_im is NULL or every one of its n_sites entries is zero.  Kinds, geometries and rows are those above.  With
 * wr = w(s) of coef_re and wi = w(s) of coef_im as defined for EIGENEX_SPIN_SITE_Z above:
 *   Z            real_coef:  y.re = wr * x.re                   y.im = wr * x.im
 *                otherwise:  y.re = fma(-wi, x.im, wr * x.re)   y.im = fma(wi, x.re, wr * x.im)
 *   PLUS, MINUS  y = (0.0, 0.0), then for i ascending over the terms the row has, x being the element the term reads:
 *                y.re = fma(cr, x.re, y.re);  y.re = fma(-ci, x.im, y.re)   (the second not with real_coef)
 *                y.im = fma(cr, x.im, y.im);  y.im = fma(ci, x.re, y.im)    (the second not with real_coef)
 *   norm2 = sum_r |y_r|^2: per row the fma of the real part, then that of the imaginary part (device: fixed-order partial sums).
 * With real_coef each part of y is eigenex_spin_site_apply's result on that part of x, bit for bit.
 *   eigenex_spin_site_apply_z       both states are complex spin states (eigenex_spin_upload_z, eigenex_spin_sector_upload_z); a
 *                                   real state, or one real and one complex, is EIGENEX_ERR_STATE with a message that names
 *                                   eigenex_spin_site_apply.  Geometries, aliasing (y may be x for Z only), scratch, the one
 *                                   synchronisation and what is left untouched are those of eigenex_spin_site_apply; a coefficient
 *                                   of either part that is not finite is refused.
 *   eigenex_spin_site_apply_host_z  the definition the kernel is held against, in host code: x and y have 2 doubles per row. */
int eigenex_spin_site_apply_z(eigenex_basis_t src, int x_ref, eigenex_basis_t dst, int y_ref, int kind,
                              const double* coef_re /* n_sites */, const double* coef_im /* n_sites, or NULL */,
                              double* norm2 /* or NULL */);
int eigenex_spin_site_apply_host_z(int n_sites, int n_up_src /* -1: full space */, int kind, const double* coef_re,
                                   const double* coef_im /* or NULL */, const double* x, double* y, double* norm2);
/* The reduced density matrix rho_A of a real vector over the rows of a matrix-free spin-1/2 operator, on the device, without
 * downloading the vector: what the entanglement entropy, the Renyi entropies and the entanglement spectrum are taken from.  NOT
 * part of the reference.  The subsystem A is a 32-bit site mask mask_a (bit i = site i); nA = popcount(mask_a), nB = n_sites - nA,
 * mask_b = the other sites; dep_A(a) deposits the nA-bit word a into mask_a (bit j of a goes to the j-th lowest set bit), dep_B
 * likewise.
 *   full space   one block of d = 2^nA rows:  rho[a, a'] = sum_{b < 2^nB} x[dep_A(a) | dep_B(b)] * x[dep_A(a') | dep_B(b)]
 *   sector       rho_A is block-diagonal in the number k of up sites inside A: blocks k = max(0, n_up - nB) .. min(nA, n_up);
 *                block k has d_k = C(nA, k) rows, row i is the i-th nA-bit word with k bits set in ascending order, b runs over
 *                the C(nB, n_up - k) words of nB bits with n_up - k bits set in ascending order, and the element is
 *                x[rank(dep_A(a) | dep_B(b))]
 * The blocks are packed in ascending k, each a full d_k x d_k column-major matrix with both triangles stored; (i, j) and (j, i)
 * hold the same bits.  The sums are raw and unnormalised (the trace is sum_s x_s^2).  Errors (EIGENEX_ERR_ARG, message in
 * eigenex_last_error): a zero mask, a site at or above n_sites, a mask that leaves no site out, a geometry that
 * eigenex_spin_measure_host refuses, a block of more than 4096 rows (nA <= 12 in the full space, nA <= 14 in a sector), an
 * out_len that is not the layout's length.
 *   eigenex_spin_rdm_layout  host only, no context: the number of blocks, k of the first (0 in the full space), dims[n_blocks]
 *                            (at most 33) and offsets[n_blocks + 1] (at most 34; the last is the length of `out`).  Any output
 *                            may be NULL.
 *   eigenex_spin_rdm         x = any vector reference of a state whose operator handle came from eigenex_spin_upload or
 *                            eigenex_spin_sector_upload; any other operator or a host callback: EIGENEX_ERR_STATE.  out is host
 *                            memory of exactly the layout's length.  Runs on the context's stream and synchronises once.  No
 *                            vector of the state, no coefficient, counter or recorded step batch is touched.  No atomics: every
 *                            entry is the sum of its b range cut into slices, the slices added in ascending order; the number
 *                            of slices depends on the geometry, the mask and the launch grid (eigenex_basis_tune) alone, so two
 *                            calls return identical bytes.
 *   eigenex_spin_rdm_host    the definition the kernels are held against, in host code: no context, no GPU.  The b terms are
 *                            added in ascending order, one fma per term. */
int eigenex_spin_rdm_layout(int n_sites, int n_up /* -1: full space */, uint32_t mask_a, int* n_blocks, int* k_first,
                            int64_t* dims /* <= 33 */, int64_t* offsets /* <= 34 */);
int eigenex_spin_rdm(eigenex_basis_t b, int x_ref, uint32_t mask_a, double* out, int64_t out_len);
int eigenex_spin_rdm_host(int n_sites, int n_up /* -1: full space */, const double* x, uint32_t mask_a, double* out,
                          int64_t out_len);
/* The same for a COMPLEX vector x (interleaved (re, im) pairs): rho[i, j] = sum_b M[i, b] conj(M[j, b]) over the same blocks, with
 * the same layout, limits, argument check and messages (under these names).  out: the blocks packed in ascending k, each a full
 * column-major d_k x d_k matrix of interleaved (re, im) pairs; out_len = 2 * the layout's length.  Raw sums: the trace is
 * sum |x|^2.  The imaginary part of a diagonal entry is +0.0 and (j, i) holds the bits of (i, j) with the imaginary part negated.
 *   eigenex_spin_rdm_z       x = any vector reference of a COMPLEX state whose operator handle came from eigenex_spin_upload_z or
 *                            eigenex_spin_sector_upload_z.  EIGENEX_ERR_STATE: a real state (that is eigenex_spin_rdm), any other
 *                            operator, a host callback.  Everything else as eigenex_spin_rdm: the same plan and slices (the
 *                            scratch is twice the real call's), no atomics, nothing of the state touched, identical bytes from
 *                            two calls.
 *   eigenex_spin_rdm_host_z  the definition in host code: per entry i >= j one chain over ascending b of four fmas per term,
 *                            re += ar_i ar_j, re += ai_i ai_j, im += ai_i ar_j, im -= ar_i ai_j. */
int eigenex_spin_rdm_z(eigenex_basis_t b, int x_ref, uint32_t mask_a, double* out, int64_t out_len);
int eigenex_spin_rdm_host_z(int n_sites, int n_up /* -1: full space */, const double* x /* interleaved */, uint32_t mask_a,
                            double* out, int64_t out_len);
/* CSR that already lives in device memory of this context's GPU (e.g. tensors of a GPU framework: pass their
 * data pointers): copied device-to-device, never through the host, after a device-side check of the row pointers
 * and column indices.  Unsharded contexts only; rowptr_dev[0] = 0; columns are global = local indices. */
int eigenex_csr_upload_device(eigenex_context_t ctx, int64_t n, const int32_t* rowptr_dev, const int32_t* col_dev,
                              const double* val_dev, int is_complex, eigenex_csr_t* out);
/* passes of the (largest) local shard: 1 = not column-blocked */
int eigenex_csr_column_blocks(eigenex_csr_t csr, int* passes);
/* how the operator is stored on the device.  A layout chosen automatically never changes a result, with one exception:
 * EIGENEX_LAYOUT_SPLIT_TILES adds a row's products in another association (see column_blocks = -3) */
enum { EIGENEX_LAYOUT_CSR = 0, EIGENEX_LAYOUT_COLUMN_BLOCKED = 1, EIGENEX_LAYOUT_SORTED_TILES = 2, EIGENEX_LAYOUT_DENSE_BLOCKS = 3,
       EIGENEX_LAYOUT_SPLIT_TILES = 4, EIGENEX_LAYOUT_MATRIX_FREE_SPIN = 5 /* eigenex_spin_upload: nothing stored */,
       EIGENEX_LAYOUT_MATRIX_FREE_SPIN_SECTOR = 6 /* eigenex_spin_sector_upload: two rank tables, no rows */,
       EIGENEX_LAYOUT_MATRIX_FREE_SPIN_MOMENTUM = 7 /* eigenex_spin_momentum_upload: one representative per row and a bucket table */,
       EIGENEX_LAYOUT_MATRIX_FREE_SPIN_MOMENTUM64 = 8 /* eigenex_spin_momentum64_upload: the same with 64-bit states, up to 48 sites */ };
int eigenex_csr_layout(eigenex_csr_t csr, int* layout);
/* how the entries of an EIGENEX_LAYOUT_CSR operator are encoded.  EIGENEX_ENCODING_ROW_CODES: a real operator in one pass
 * whose rows use at most 16 column offsets (col - row, halo columns in local numbering) and at most 255 bitwise-distinct
 * values -- constant-coefficient stencils, graph Laplacians, adjacency matrices -- is stored as one 8- or 16-byte record per
 * row (a palette index per offset) instead of row pointers, columns and values; rows are still applied whole, in stored
 * order, with the same results bit for bit.  Chosen per shard by eigenex_csr_upload / eigenex_csr_upload64 (where the
 * automatic choice is plain CSR) and eigenex_csr_laplacian3d, never by eigenex_csr_upload_device; the environment variable
 * EIGENEX_NO_ROW_CODES, read per upload, keeps the plain form.  Reports ROW_CODES if any local shard is row-coded. */
enum { EIGENEX_ENCODING_PLAIN = 0, EIGENEX_ENCODING_ROW_CODES = 1 };
int eigenex_csr_encoding(eigenex_csr_t csr, int* encoding);
/* synthetic 7-point Laplacian on an n^3 grid generated on the device (BASELINE configs 2 and 4) */
int eigenex_csr_laplacian3d(eigenex_context_t ctx, int64_t n, eigenex_csr_t* out);
int eigenex_csr_destroy(eigenex_csr_t csr);
/* nnz_local counts STORED entries: 0 for a matrix-free spin operator */
int eigenex_csr_info(eigenex_csr_t csr, int64_t* n_global, int64_t* n_local, int64_t* nnz_local, int64_t* n_halo_local);

/* ---- Krylov state ------------------------------------------------------ */
/* capacity = maximum number of basis vectors (Lanczos with maxIterations m needs m+1,
 * Arnoldi m: SURVEY F8); n_ortho = size of orthogonalizingVectors_.
 * csr may be NULL: the operator is then a host callback (single shard only). */
int eigenex_basis_create(eigenex_context_t ctx, eigenex_csr_t csr, int64_t n_global, int capacity, int n_ortho,
                         eigenex_basis_t* out);
/* explicit scalar type (needed when csr == NULL: host-callback operator); with a csr it must match it.
 * eigenex_basis_create == eigenex_basis_create_ex with is_complex taken from the csr (real if csr == NULL). */
int eigenex_basis_create_ex(eigenex_context_t ctx, eigenex_csr_t csr, int64_t n_global, int capacity, int n_ortho,
                            int is_complex, eigenex_basis_t* out);
int eigenex_basis_is_complex(eigenex_basis_t b, int* is_complex);
int eigenex_basis_destroy(eigenex_basis_t b);
/* deep copy (same context, same operator handle): copying a solver object in the reference copies its vectors
 * (implicitly copyable classes, lanczos.hpp:104-105, :233-239); device-to-device, synchronises */
int eigenex_basis_clone(eigenex_basis_t src, eigenex_basis_t* out);
int eigenex_basis_set_host_operator(eigenex_basis_t b, eigenex_matvec_fn fn, void* user);
/* settings of LanczosBase/ArnoldiBase that the kernels need (lanczos.hpp:155-159) */
int eigenex_basis_configure(eigenex_basis_t b, double eigenvalue_shift, double threshold,
                            int64_t reorthogonalize_interval, int ortho_mode);
/* complex eigenvalueShift_ (ArnoldiBase, arnoldi.hpp:108: the shift is a Scalar there) */
int eigenex_basis_configure_z(eigenex_basis_t b, double shift_re, double shift_im, double threshold,
                              int64_t reorthogonalize_interval, int ortho_mode);
/* grow the basis slab to hold at least `capacity` vectors, keeping the state (the reference's
 * std::vector<VectorType>::push_back never runs out: lanczos.hpp:402, arnoldi.hpp:364) */
int eigenex_basis_reserve(eigenex_basis_t b, int capacity);
int eigenex_basis_capacity(eigenex_basis_t b, int* capacity);
/* tuning knobs: workgroups per CU of the persistent grids (slab kernels dots/update, SpMV; 1..16, defaults 2 and 4)
 * and `flags`, a bit set (default 0):
 *   bit 0  XCD-sliced tile order of the SpMV: within each step of the row frontier every XCD takes a contiguous eighth
 *          of the tiles (measured: no change on the 7-point stencil, -0.2 %..+0.6 %; cutting the whole row range into
 *          eight chunks, the first attempt, was 7 % slower)
 *   bit 1  non-temporal loads of the CSR value/column streams (+5 % on a random 32-per-row CSR, slower on stencils)
 * Results do not depend on the knobs beyond the summation order of the per-workgroup partial sums. */
int eigenex_basis_tune(eigenex_basis_t b, int vec_blocks_per_cu, int spmv_blocks_per_cu, int flags);
/* clearLanczosSteps()/clearArnoldiSteps(): forget vectors and coefficients, keep settings */
int eigenex_basis_clear(eigenex_basis_t b);
/* Lanczos between shards (more than one shard, batched schemes): by default alpha_{k+1} = u_{k+1}.v (lanczos.hpp:448) is not
 * all-reduced on its own after the operator but travels with the next step's dots (together with the Gram column
 * V^H u_{k+1}, from which h = V^H w0 is formed exactly): 2 instead of 3 all-reduces per step, results equal to rounding.
 * on = 0 restores one all-reduce per scalar.  Single-shard contexts are not affected. */
int eigenex_basis_set_alpha_fusion(eigenex_basis_t b, int on);
/* Recorded step batches (hipGraphs) of this state: how many are cached, their node count, and the node limit that applies
 * on the calling thread (hipGraphInstantiate recurses over a linear chain: the limit follows the stack that is left, see
 * library.hip).  Batches above the limit run as plain launches. */
int eigenex_basis_graph_info(eigenex_basis_t b, int* ngraphs, int64_t* nodes_total, int64_t* node_limit);
/* One-sweep Lanczos steps (one shard, device operator, real data, batched scheme against every column, no deflation vectors, no
 * filter, no thick restart; EIGENEX_TWO_SWEEPS=1 turns them off): how many steps since the last clear had their pending vector
 * re-orthogonalised by the two-sweep pass because a lagged coefficient exceeded 2^-27 (close to a breakdown).  Synchronises. */
int eigenex_basis_repairs(eigenex_basis_t b, int* repairs);
/* A batch of one-sweep Lanczos steps ends with complete alpha and beta, but writes the corrected form of its newest basis column
 * only when something other than a further one-sweep step touches the state: every call that takes the state does that first,
 * except eigenex_lanczos_enqueue (when a one-sweep step follows), eigenex_lanczos_state, eigenex_basis_repairs,
 * eigenex_basis_configure[_z], eigenex_basis_set_alpha_fusion, eigenex_basis_clear, eigenex_basis_destroy and the getters.
 * *pending = 1 while that column is still outstanding.  Results never depend on it; EIGENEX_EAGER_CLOSE=1 (read once per process)
 * writes the column at every batch end instead.  Does not synchronise. */
int eigenex_basis_close_pending(eigenex_basis_t b, int* pending);

/* host <-> device vectors (rows owned by this context) */
int eigenex_vec_upload(eigenex_basis_t b, int vec_ref, const double* host);
int eigenex_vec_download(eigenex_basis_t b, int vec_ref, double* host);
/* device-to-device copy dst = src (e.g. W = START before the first step: no PCIe traffic per solve) */
int eigenex_vec_copy(eigenex_basis_t b, int dst_ref, int src_ref);

/* ---- step primitives (each one parity-tested on its own; all synchronise) -- */
/* Complex bases: h / dot arguments hold (re, im) pairs (dots are conjugate-linear in the basis vector,
 * Eigen's a.dot(b) = sum conj(a_i) b_i); host vectors are interleaved.
 * y = A*x + shift*x ; if dot != NULL also *dot = x . y      (a1, a2, a3 of SURVEY 8a); works with a CSR/block
 * handle or, on an unsharded context, with the host callback of eigenex_basis_set_host_operator */
int eigenex_apply(eigenex_basis_t b, int x_ref, int y_ref, double shift, double* dot);
/* Chebyshev polynomial filter of a Hermitian device operator:  p(A) = sum_k mu[k] T_k((A - center)/halfwidth),  k <= degree,
 * mu real (mu[degree + 1] is copied).  While a filter is set, eigenex_lanczos_enqueue builds the Krylov space of p(A) instead of
 * A (alpha, beta and the basis are those of p(A): with a Jackson-damped delta peak at a target energy the eigenvalues of A
 * nearest the target become the largest of p(A)); eigenex_apply keeps meaning A itself.  [center - halfwidth, center +
 * halfwidth] must contain the spectrum of A.  degree = 0 removes the filter (mu may be NULL).  Setting or removing a filter
 * drops the recorded step batches of the state.  The first call allocates two more work vectors.
 * Per row and degree, every product rounded before it is added:  a = (A t_k)[i] + (-center) t_k[i];  t_1 = (1/halfwidth) a,
 * t_{k+1} = (2/halfwidth) a - t_{k-1};  acc_1 = mu[0] x + mu[1] t_1,  acc_{k+1} = acc_k + mu[k+1] t_{k+1}.  One-pass real CSR
 * operators (plain or row-coded) take this in the operator kernel's epilogue, all others in a streaming kernel behind the
 * operator: the same bits.  EIGENEX_NO_FUSED_FILTER in the environment, read by every call, selects the second form everywhere.
 * Between shards one application of p(A) issues `degree` neighbour exchanges.
 * EIGENEX_ERR_ARG: degree < 0, mu == NULL, halfwidth <= 0;  EIGENEX_ERR_STATE: the operator is a host callback.
 * With a filter set, eigenex_arnoldi_enqueue and a Lanczos step with a non-zero eigenvalue shift return EIGENEX_ERR_STATE. */
int eigenex_basis_set_filter(eigenex_basis_t b, int degree, const double* mu, double center, double halfwidth);
/* y = p(A) x with the filter of the state; synchronises; vector references as for eigenex_apply (x is copied into the operator
 * input vector W, y may not be W or x) */
int eigenex_filter_apply(eigenex_basis_t b, int x_ref, int y_ref);
/* Chebyshev moments of a Hermitian device operator (kernel polynomial method; Weisse et al., Rev. Mod. Phys. 78 (2006) 275):
 * mu[k] = <x| T_k((A - center)/halfwidth) |x>, k < n_moments (unnormalised; mu[0] = <x|x>).  ceil((n_moments-1)/2) operator
 * applications: with the recurrence of eigenex_basis_set_filter (t_0 = x, no accumulator) every application yields two
 * moments, mu_2k = 2 <t_k,t_k> - mu_0 and mu_2k+1 = 2 <t_k+1,t_k> - mu_1.  x is copied into W as for eigenex_filter_apply.  On
 * return EIGENEX_VEC_V holds t_d, the last Chebyshev vector formed (d applications).  The dot products stay on the device until
 * the end: one synchronisation.  Between shards: one neighbour exchange per application and ONE all-reduce of the moments
 * array at the end.  Independent of, and without effect on, a filter set on the state.  The two forms of the step (operator
 * kernel's epilogue / streaming kernel, EIGENEX_NO_FUSED_FILTER as for the filter) give the same bits in t_k; their moments are
 * each reproducible from run to run and differ from each other by rounding (other partial sums).  The first call allocates the
 * filter's second work vector (and the operator's output where the streaming form runs).
 * EIGENEX_ERR_ARG: n_moments < 1, mu == NULL, halfwidth <= 0, n_vectors < 1;  EIGENEX_ERR_STATE: the operator is a host callback. */
int eigenex_kpm_moments(eigenex_basis_t b, int x_ref, int n_moments, double center, double halfwidth, double* mu);
/* n_vectors runs of the above from +-1 vectors (seed, stream = first_stream + i): mu_each[i*n_moments + k], divided by N; one
 * synchronisation and one all-reduce for all of them */
int eigenex_kpm_trace_moments(eigenex_basis_t b, int n_moments, int n_vectors, uint64_t seed, uint64_t first_stream,
                              double center, double halfwidth, double* mu_each);
/* x[row] = +1 or -1 (imaginary part 0) from a counter-based hash of (seed, stream, global row): the same vector under every
 * sharding.  key = mix((mix(seed + G) ^ stream) + G), h = mix((key ^ row) + G) modulo 2^64, -1 where bit 63 of h is set;
 * G = 0x9E3779B97F4A7C15, mix = the splitmix64 finaliser (z ^= z >> 30, z *= 0xBF58476D1CE4E5B9, z ^= z >> 27,
 * z *= 0x94D049BB133111EB, z ^= z >> 31). */
int eigenex_vec_random_signs(eigenex_basis_t b, int x_ref, uint64_t seed, uint64_t stream);
/* h[i] = col(first + i*stride) . w, i < count, then h[count + q] = ortho(q) . w, q < n_ortho_used   (a5 dot half) */
int eigenex_dots(eigenex_basis_t b, int w_ref, int first, int stride, int count, int n_ortho_used, double* h);
/* w -= sum_i h[i]*col(first+i*stride) + sum_q h[count+q]*ortho(q); *nrm2 = ||w||^2   (a5 axpy half, a6) */
int eigenex_update(eigenex_basis_t b, int w_ref, int first, int stride, int count, int n_ortho_used, const double* h,
                   double* nrm2);
/* z = x - a*p - b*q          (a4; q_ref may equal p_ref with b = 0) */
int eigenex_axpy2(eigenex_basis_t b, int z_ref, int x_ref, double a, int p_ref, double bcoef, int q_ref);
/* dst = s * src              (a7) */
int eigenex_scale(eigenex_basis_t b, int dst_ref, int src_ref, double s);

/* ---- fused steps (what the solver classes call) -------------------------- */
/* Lanczos: start vector (setInitialVector) -> eigenex_vec_upload(b, EIGENEX_VEC_W, init).
 * Each *_enqueue(b, ncalls) enqueues `ncalls` calls of updateLanczosSteps()/updateArnoldiSteps()
 * WITHOUT host synchronisation; breakdown (beta <= threshold, zero start vector, residue <=
 * threshold) is detected on the device and turns the remaining calls into no-ops, exactly as
 * the reference would have stopped.  A batch of >= 4 calls on a device operator (no communicator, profiling off)
 * is recorded as a hipGraph the first time and replayed when the same batch is enqueued again from the same state
 * with the same settings (repeated solves of one size); EIGENEX_NO_GRAPHS=1 in the environment turns that off. */
int eigenex_lanczos_enqueue(eigenex_basis_t b, int ncalls);
int eigenex_arnoldi_enqueue(eigenex_basis_t b, int ncalls);
/* Thick restart of a Lanczos run (not in the reference, which has no restart: SURVEY F6; built on the same
 * device state).  Precondition: m+1 vectors u_0..u_m on the device.  S (column-major m x nkeep, leading
 * dimension lds, real) holds the kept eigenvectors of T_m.  Afterwards columns 0..nkeep-1 are the Ritz vectors
 * V_m S, column nkeep is u_m, v_ and alpha[nkeep] are those of u_m, beta[nkeep-1] = coupling_last
 * (= beta_{m-1} * S[m-1, nkeep-1]); the next eigenex_lanczos_enqueue continues from there (full
 * re-orthogonalisation supplies the remaining couplings).  Needs capacity >= (m+1) + nkeep. Synchronises. */
int eigenex_lanczos_restart(eigenex_basis_t b, int nkeep, const double* S, int lds, double coupling_last);
/* Krylov-Schur restart of an Arnoldi run (not in the reference, which has no restart: SURVEY F6).  Precondition: a complete
 * Arnoldi state of m = nvec vectors (nalpha == m, not stopped), i.e.  A V_m = V_m H_m + w e_m^T  with the unnormalised residual
 * in W and residue = |w|.
 * Q: m x nkeep, column-major, orthonormal columns spanning an invariant subspace of H_m, in the basis' scalar type (complex
 *    basis: (re, im) pairs; ldq in entries).
 * B: (nkeep+1) x nkeep, same scalar type: rows 0..nkeep-1 = Q^H H_m Q, row nkeep = residue * Q[m-1, :]; ldb in entries.
 * Afterwards columns 0..nkeep-1 hold V_m Q, nvec = nalpha = nkeep, the stored projected matrix is B, W / residue / scale
 * are untouched, and the next eigenex_arnoldi_enqueue continues from there.  Needs capacity >= m + nkeep.  Synchronises.
 * EIGENEX_ERR_STATE: incomplete or stopped state, capacity too small; EIGENEX_ERR_ARG: nkeep < 1, nkeep >= m, ldq < m,
 * ldb < nkeep + 1. */
int eigenex_arnoldi_restart(eigenex_basis_t b, int nkeep, const double* Q, int ldq, const double* B, int ldb);

typedef struct {
  int32_t nvec;        /* lanczosvectors_.size() / arnoldivectors_.size() */
  int32_t iterations;  /* iterations_ */
  int32_t nalpha;      /* alpha_.size()  (Arnoldi: h_.size()) */
  int32_t nbeta;       /* beta_.size() */
  int32_t stopped;     /* 1 = a step returned false on the device (breakdown / start vector failed) */
  int32_t calls_true;  /* number of enqueued calls that returned true since the last clear */
  double residue;      /* Arnoldi residue_ */
} eigenex_state_t;

/* synchronises and returns the coefficients: Lanczos alpha[nalpha], beta[nbeta] (real);
 * Arnoldi: hess column-major with leading dimension ldh (>= nalpha+1): hess[r + c*ldh] = h_[c][r]
 * (complex basis: (re, im) pairs, i.e. 2*ldh doubles per column).
 * Any output pointer may be NULL. */
int eigenex_lanczos_state(eigenex_basis_t b, eigenex_state_t* st, double* alpha, double* beta);
int eigenex_arnoldi_state(eigenex_basis_t b, eigenex_state_t* st, double* hess, int ldh);

/* X[:, e] = sum_m S[m + e*lds] * col(m), m < nvec, e < nev (S real: eigenvectors of the tridiagonal
 * matrix); then each column is normalised and divided by the phase z/|z| of its first non-zero entry
 * (lanczos.hpp:798-816).  X is returned to the host (rows owned by this context), leading dimension
 * ldx entries; it has the basis' scalar type (interleaved complex for a complex basis). */
int eigenex_ritz_vectors(eigenex_basis_t b, int nvec, int nev, const double* S, int lds, double* X, int64_t ldx);
/* complex coefficients (Arnoldi, arnoldi.hpp:841-865): S_re/S_im column-major nvec x nev (leading dimension lds);
 * X receives interleaved (re,im) pairs, i.e. std::complex<double>[ldx * nev]; each column is normalised and divided by
 * the phase z/|z| of its first non-zero entry. */
int eigenex_ritz_vectors_complex(eigenex_basis_t b, int nvec, int nev, const double* S_re, const double* S_im, int lds,
                                 double* X_interleaved, int64_t ldx);
/* X[:, e] = sum_m C[m + e*ldc] * col(m), m < nvec, e < ncols, returned as it is (no normalisation, no phase):
 * any vector of the Krylov space from its coefficients in one pass over the basis, e.g. f(A) v ~ V f(T) e_1 |v|
 * (reference: LanczosFunctionSolver / LanczosExponentialSolver::solveWithEigens, lanczos.hpp:953-1075, which go
 * through all Ritz vectors instead).  C_im == NULL: real coefficients, X has the basis' scalar type; otherwise
 * complex coefficients C_re + i C_im and X holds interleaved (re, im) pairs. */
int eigenex_krylov_combine(eigenex_basis_t b, int nvec, int ncols, const double* C_re, const double* C_im, int ldc,
                           double* X, int64_t ldx);
/* dst = sum_m C[m] * col(m), m < nvec, left on the device in a vector of the same state: the one-column case of
 * eigenex_krylov_combine (the same kernels, the same arithmetic, the same bytes) without the transfer to the host, e.g. a time
 * step psi <- V c.  dst_ref is EIGENEX_VEC_W, EIGENEX_VEC_V or a basis column at or above nvec; a column below nvec (it is
 * read), any other reference, nvec outside 1..capacity or complex coefficients on a real state: EIGENEX_ERR_ARG.  C_im == NULL:
 * real coefficients.  Any operator, real or complex state, one shard (more: EIGENEX_ERR_STATE).  A pending close of a one-sweep
 * batch is carried out first; synchronises once. */
int eigenex_krylov_combine_to(eigenex_basis_t b, int nvec, const double* C_re, const double* C_im_or_null, int dst_ref);

#ifdef __cplusplus
}
#endif
#endif /* EIGENEX_HIP_H */
