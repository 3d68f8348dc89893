/* libscilmm_hip C ABI -- the drop-in boundary of the MI355X-native sparse-Cholesky REML engine.
 *
 * The reference has no FFI: its boundary is the duck-typed Python protocol
 *     cholesky_func(V) -> factor ;  factor(b), factor.L(), factor.P(), factor.logdet()
 * implemented by sksparse.cholmod (reference scilmm/SparseCholesky.py:16-26, used at :30,:32,:40,:50,
 * :52,:93,:100; twin scilmm/Estimation/LMM.py:14-24).  Each entry point below names the reference call it
 * replaces.  The Python shim (scilmm_amd/_lib.py, scilmm_amd/factor.py) binds exactly these symbols through
 * ctypes; INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions: plain pointers and sizes only; every function returns an int status (0 = ok, <0 = error);
 * opaque handles; caller-allocated outputs; int64 offsets, int32 indices, float64 values; dense
 * right-hand sides are ROW-major n x r (NumPy C order, what the reference passes); one handle may be used
 * from one thread at a time; no global state.  Functions suffixed _dev take DEVICE pointers (HBM) and
 * enqueue on the handle's stream without synchronising.
 */
#ifndef SCILMM_HIP_H
#define SCILMM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  SCILMM_OK = 0,
  SCILMM_ERR_ARG = -1,        /* bad argument / handle */
  SCILMM_ERR_NOT_PD = -2,     /* V is not positive definite (sksparse: CholmodNotPositiveDefiniteError) */
  SCILMM_ERR_DEVICE = -3,     /* HIP runtime error (no device, launch failure, out of memory) */
  SCILMM_ERR_STATE = -4       /* call order violated (e.g. factorize before values_upload) */
};

typedef struct scilmm_symbolic scilmm_symbolic; /* pattern analysis + device-resident A_k values */
typedef struct scilmm_factor scilmm_factor;     /* numeric factor L of V[P][:,P]                  */

/* Ordering / supernode options; the counterpart of the reference's constructor kwargs
 * SparseCholesky(use_long=False, mode='supernodal', ordering_method='nesdis') (SparseCholesky.py:17-20).
 * Negative / zero fields mean "library default". */
typedef struct scilmm_options {
  int32_t ordering;     /* 0 = approximate minimum degree, 1 = natural, 2 = perm_in, 3 = nested dissection ('nesdis',
                           SparseCholesky.py:17), 4 = whichever of 0 / 3 gives fewer factor flops */
  int32_t relax_small;  /* relaxed amalgamation: always merge when merged width <= this */
  int32_t relax_w1, relax_w2;
  double relax_z1, relax_z2, relax_z3;
  double amd_dense;
  int32_t max_width;    /* split supernodes wider than this (0 = library default) */
  double nd_oksep;      /* nested dissection: accept a separator only below this share of its subgraph (0 = default 0.1;
                           1.0 = always dissect, CHOLMOD's nd_oksep default) */
  double dense_relax;   /* the top of the elimination tree is padded to a dense block-column matrix while padded / true
                           flops stay below this (0 = default: 1.10, and up to 1.25 once the tail is >= 32768 columns
                           wide, where the dense kernel takes it over; negative = never pad) */
} scilmm_options;

typedef struct scilmm_info {
  int32_t n, K, nsuper, nlevels;
  int64_t nnzL;         /* sum_j colcount_j : algorithmic nonzeros of L (BASELINE metric nnz(L)/s) */
  int64_t nnzL_stored;  /* doubles of supernodal panel storage */
  int64_t nnz_pattern;  /* entries of tril(union pattern of the A_k) */
  double flops;         /* sum_j colcount_j^2 (CHOLMOD "fl" convention) */
  int64_t n_rows_total; /* sum_s m_s */
  int64_t n_updates;    /* number of (target, descendant) update pairs */
  double update_flops;  /* algorithmic flops of the supernodal update kernels (lower-triangular count, true structure) */
  double solve_flops_per_rhs; /* 4 nnz(L_stored) : forward + backward sweep per right-hand side */
  double update_flops_executed; /* update_flops plus the explicit zeros of the padded dense tail */
  int32_t dense_first;  /* fronts [dense_first, nsuper) form the dense tail (nsuper: none) */
  double dense_flops;   /* algorithmic update flops among the fronts of the dense tail (true structure): k_dense's work */
} scilmm_info;

/* --- symbolic phase: replaces cholmod_analyze inside sk_cholesky (SparseCholesky.py:23-26), but once per
 * pattern instead of once per evaluation.  indptr[k]/indices[k] is the CSR pattern of mats[k]; VALUES are only ever
 * read from the entries with column <= row (the matrices are symmetric).  Inputs that store both halves with
 * strictly ascending rows (what SciPy hands over) are analysed without any scatter pass -- verified by a hash of the
 * mirrored entries; anything else (one half only, unsorted rows, an unsymmetric pattern, whose upper entries are
 * ignored) takes a slower path with the same result.  perm_in[new] = old or NULL; a given permutation is used exactly
 * as it is, otherwise the library's ordering may be followed by moving the dense tail's fronts to the end of the
 * order (same fill). */
int scilmm_symbolic_create(int32_t n, int32_t K, const int64_t* const* indptr, const int32_t* const* indices,
                           const int32_t* perm_in, const scilmm_options* opts, int32_t ngpus,
                           scilmm_symbolic** out);  /* ngpus: must be >= 1; the analysis itself does not depend on it (the
                                                       distribution is chosen by scilmm_dist_init) */
int scilmm_symbolic_info(const scilmm_symbolic* sym, scilmm_info* info);
/* Copy a named int32/int64 array of the analysis ("perm" replaces factor.P(), SparseCholesky.py:93).
 * Call with out == NULL to get the element count.  Names: perm, iperm, parent, colcount, sn_start, sn_parent,
 * sn_rowptr, sn_rows, sn_loff, sn_level, level_ptr, level_fronts, dense_first, tail_blk_ptr / tail_blk (block pattern
 * of the dense tail's true structure), asm_dst, diag_dst, pat_colptr, pat_row, val_slot:k / val_src:k (value-assembly
 * maps of input matrix k), upd_*, tile_*, combo_* (built on demand), level_tile_*, level_pair_*, inv_off, child_*;
 * deterministic mode (built on demand): pat_rowptr / pat_rowslot / pat_rowcol (int64, int64, int32: the strict lower triangle
 * of the pattern by ROW -- per entry its pattern slot and its column, columns ascending) and the pull schedule of the forward
 * sweep pull_seg_front / pull_seg_ptr (int64) / pull_seg_slot / pull_front_seg / pull_level_ptr (int64) / pull_level_segs /
 * pull_fold_ptr (int64) / pull_fold (csrc/symbolic.h describes them). */
int scilmm_symbolic_get(const scilmm_symbolic* sym, const char* what, void* out, int64_t* count);
const char* scilmm_symbolic_error(const scilmm_symbolic* sym);
void scilmm_symbolic_free(scilmm_symbolic* sym);
/* Image of an analysis on disk or in /dev/shm (the reference keeps its stage artefacts as files,
 * scilmm/IBDCompute.py:82-84): the 20 s analysis of the 1M config is done once per pattern and NODE instead of once per
 * process (8 ranks of a multi-GPU run, repeated fits).  `key` = the caller's 64-bit hash of everything the analysis
 * depends on (patterns, permutation, options); scilmm_symbolic_load returns SCILMM_ERR_STATE unless the file exists, was
 * written by this build and carries that key -- the caller then analyses afresh.  Host only. */
int scilmm_symbolic_save(const scilmm_symbolic* sym, const char* path, uint64_t key);
int scilmm_symbolic_load(const char* path, uint64_t key, scilmm_symbolic** out);

/* The ordering step of cholmod_analyze alone (SparseCholesky.py:17 ordering_method): fill-reducing permutation of a
 * symmetric CSR pattern (only entries with column < row are read).  method 0 = approximate minimum degree,
 * 1 = nested dissection (graph bisection, minimum degree on the leaves and wherever no separator below 10 % of the
 * subgraph exists), 2 = nested dissection that accepts every separator.  perm_out[new] = old. */
int scilmm_order(int32_t n, const int64_t* indptr, const int32_t* indices, int32_t method, int32_t* perm_out);
/* nnz(L), sum colcount^2 and the largest column count of the factor of pattern[perm][:,perm] (perm NULL = natural):
 * elimination tree + column counts only -- what the ordering study in profiles/ and bench.py's fill figures use. */
int scilmm_fill_count(int32_t n, const int64_t* indptr, const int32_t* indices, const int32_t* perm, int64_t* nnzL,
                      double* flops, int32_t* max_colcount);

/* Frees the host copies of the value-assembly maps (asm_dst, pat_row, val_slot / val_src: 13 GB at the 1M config) once the
 * values are in HBM and the device plan exists; afterwards scilmm_values_upload and the corresponding scilmm_symbolic_get
 * names are no longer available on this handle.  For processes that only evaluate (8 ranks of one node each hold a copy). */
int scilmm_symbolic_release_host_maps(scilmm_symbolic* sym);

/* --- values: one upload per A_k replaces the per-evaluation CSR arithmetic of matrices_weighted_sum
 * (SparseCholesky.py:55-59).  data_k is the CSR data array matching indptr[k]/indices[k]. */
int scilmm_values_upload(scilmm_symbolic* sym, int32_t k, const double* data_k);

/* --- numeric phase: V = sum_k sigma2[k] A_k assembled on the device, then L L^T = V[P][:,P].
 * Replaces matrices_weighted_sum + cholesky_func(V) (SparseCholesky.py:88,92).  A factor handle can be
 * re-used: scilmm_refactorize overwrites its values for new sigma2. On SCILMM_ERR_NOT_PD,
 * *bad_col receives the failing (permuted) column. */
int scilmm_factorize(scilmm_symbolic* sym, const double* sigma2, scilmm_factor** out, int32_t* bad_col);
int scilmm_refactorize(scilmm_factor* fac, const double* sigma2, int32_t* bad_col);
/* Queue the same work and return at once: the host can draw the next normal matrix (np.random.randn(n,100),
 * SparseCholesky.py:50) while the device factorizes.  scilmm_factor_wait -- or any call that uses the factor --
 * completes it and reports SCILMM_ERR_NOT_PD / *bad_col exactly like scilmm_refactorize. */
int scilmm_refactorize_async(scilmm_factor* fac, const double* sigma2);
int scilmm_factor_wait(scilmm_factor* fac, int32_t* bad_col);
void scilmm_factor_free(scilmm_factor* fac);

/* --- multi-GPU: one process per GPU, ONE cohort factored by all of them.  The fronts of the dense
 * tail at the top of the block elimination tree (the separator supernodes: > 99 % of the flops and of the storage of a
 * pedigree factor) are owned 1-D block-cyclically (tail front dense_first + j belongs to rank j % world); everything
 * below (the "prelude") is replicated.  FAN-OUT with rank-local storage: a rank keeps the prelude, its OWN tail panels
 * and a ring of a few panel slots through which the other ranks' panels pass -- a finished panel is broadcast by its
 * owner, applied by every rank to those of its own targets that need it (the sources of a whole group of panels at a
 * time, so the accumulators stay in registers over K = group x 128) and dropped.  Per rank nnz(L) / world + ring instead
 * of nnz(L): this is what lets BASELINE configs[4] (3M individuals, ~1.3 TB of factor) fit 8 x 288 GB.  The triangular
 * sweeps run with one small collective per tail block (forward: all-reduce of the block's accumulated contributions;
 * backward: broadcast of the block's solution); L*R is summed by one all-reduce.  DESIGN.md section 7 has the numbers.
 * The library links no communication library: it calls `fn` at ENQUEUE time, in the same order on every rank, and
 * the callback issues the collective on `comm_stream` (torch.distributed over RCCL in production, gloo in rehearsals):
 *   op 0 = broadcast from `root`, 1 = all-reduce (sum), 2 = all-reduce (min);
 *   buffer 0 = L, 1 = invD, 2 = logd (the arrays given to scilmm_factor_create_external), 3 = the sweeps' work
 *   buffer (scilmm_dist_set_work);  offset / count in doubles, offsets are RANK-LOCAL (the same panel lives at
 *   different offsets on its owner and in a receiver's ring).
 * The engine orders its own streams against `comm_stream` with events (before the call: comm_stream waits for the
 * producer's kernels; after it: an event recorded on comm_stream releases the consumers).  Must be called before the
 * first numeric call on the handle.  A non-positive pivot is reported by EVERY rank (the status word is all-reduced).
 * The reference has no counterpart (single-process CHOLMOD). */
typedef int (*scilmm_comm_fn)(void* ctx, int32_t op, int32_t buffer, int64_t offset, int64_t count, int32_t root);
int scilmm_dist_init(scilmm_symbolic* sym, int32_t rank, int32_t world, void* comm_stream, scilmm_comm_fn fn, void* ctx);
/* Factor storage owned by the caller (so that the communication layer can address it, e.g. as torch tensors):
 * sizes in doubles incl. the slack the kernels over-read -- of THIS rank's share once scilmm_dist_init has been called;
 * then create the handle and use scilmm_refactorize. */
int scilmm_factor_sizes(const scilmm_symbolic* sym, int64_t* L_doubles, int64_t* invD_doubles, int64_t* logd_doubles);
int scilmm_factor_create_external(scilmm_symbolic* sym, double* L, double* invD, double* logd, scilmm_factor** out);
/* Work buffer of the distributed sweeps (right-hand sides, solutions, the forward sweep's accumulator), caller-owned
 * for the same reason: scilmm_dist_work_size doubles; required before the first solve / L*R when world > 1. */
int scilmm_dist_work_size(const scilmm_symbolic* sym, int64_t* doubles);
int scilmm_dist_set_work(scilmm_symbolic* sym, double* work);
/* The distribution rule as data (tests cross-check the CPU rehearsal engine against it): owner[nsuper] (-1 = replicated),
 * loff[nsuper + 1] rank-local panel offsets for `rank` of `world` (last entry: doubles of local panel storage),
 * params = {first distributed front, group size, ring slots}.  Host only. */
int scilmm_dist_layout(const scilmm_symbolic* sym, int32_t rank, int32_t world, int32_t* owner, int64_t* loff, int32_t* params);

/* factor.logdet()  (SparseCholesky.py:40) */
int scilmm_logdet(scilmm_factor* fac, double* out);
/* factor(b): X = V^{-1} B, B and X row-major n x r  (SparseCholesky.py:30,32,52,100,149,153) */
int scilmm_solve(scilmm_factor* fac, const double* B, int32_t r, double* X);
/* (factor.L() @ R)[argsort(P)] : Z = P^T L R  (simulate_vector, SparseCholesky.py:50-51) */
int scilmm_lmul(scilmm_factor* fac, const double* R, int32_t r, double* Z);
/* factor.L() as CSC of the permuted factor (SparseCholesky.py:50); call with vals == NULL to get nnz.
 * On a DISTRIBUTED factor (scilmm_dist_init with world > 1) it returns SCILMM_ERR_STATE with an explanatory message and leaves
 * the factor untouched: a rank holds the prelude and its own tail panels only, and nothing on the hot path needs the gathered
 * factor (simulate_vector goes through scilmm_lmul, which IS collective). */
int scilmm_export_L(scilmm_factor* fac, int64_t* colptr, int32_t* rowidx, double* vals, int64_t* nnz);
/* out[j] = sum_i (A_k U)_ij U_ij  (compute_gradients, SparseCholesky.py:65-66,70); U row-major n x r */
int scilmm_quadforms(scilmm_symbolic* sym, int32_t k, const double* U, int32_t r, double* out);
/* Y = A_k X, row-major n x r (SparseCholesky.py:66,70,160,163) */
int scilmm_spmm(scilmm_symbolic* sym, int32_t k, const double* X, int32_t r, double* Y);
/* the same with DEVICE pointers, asynchronous on the engine's stream (the residual of a refinement sweep without a host round trip) */
int scilmm_spmm_dev(scilmm_symbolic* sym, int32_t k, const double* dX, int32_t r, double* dY);

/* The two halves of factor(b), without the permutation: L X = B (scilmm_solve_L) and L^T X = B (scilmm_solve_Lt), B and X
 * row-major n x r with rows in the factor's PERMUTED order (row p belongs to individual P[p]).  They replace
 * sksparse's factor.solve_L(b, use_LDLt_decomposition=False) and factor.solve_Lt(b, use_LDLt_decomposition=False)
 * (cholmod_solve2 with CHOLMOD_L / CHOLMOD_Lt); factor.apply_P / apply_Pt (CHOLMOD_P / CHOLMOD_Pt) are index operations
 * on the caller's side (scilmm_symbolic_get "perm").  X = apply_Pt(solve_Lt(solve_L(apply_P(B)))) is scilmm_solve's X: the
 * same launches in the same order, bit for bit in deterministic mode.  Any r >= 1 (blocks of 128 columns, like
 * scilmm_solve); r <= 0 or a null pointer: SCILMM_ERR_ARG.  Refused with SCILMM_ERR_STATE and a message, the handle left
 * as it was: a distributed factor (scilmm_dist_init with world > 1), a handle with scilmm_set_front_precision(32) (a
 * half-solve cannot be refined against the exact V the way factor(b) is), a factor consumed by scilmm_selected_inverse.
 * The reference never takes a half-solve; the marker scan below is what they are for. */
int scilmm_solve_L(scilmm_factor* fac, const double* B, int32_t r, double* X);
int scilmm_solve_Lt(scilmm_factor* fac, const double* B, int32_t r, double* X);

/* One block of a marker association scan with V held fixed (EMMAX / P3D form), on the device: with w(b) = L^-1 P b,
 * GLS of y on [C, g] under V is OLS of w(y) on [w(C), w(g)], so a marker costs the FORWARD half of a solve and a column
 * reduction -- in place of one scilmm_solve_dev (cholmod_solve2 with CHOLMOD_A) and an n x r device-to-host copy per block
 * of markers.
 *   d_geno : marker j of the block = d_geno + j * ld_geno, n int8 values, individuals in the ORIGINAL order (the row order
 *            of the matrices), 0 / 1 / 2 = allele count, any negative value = missing; ld_geno >= n.  Any alignment; the
 *            rows are read in aligned 16-byte pieces, so the buffer must lie in an allocation that starts and ends on
 *            16-byte boundaries (every hipMalloc allocation does).
 *   r      : markers in the block, 1 .. 128.
 *   d_Q    : n x q row-major, PERMUTED order: the caller's whitened [w(C) | w(y)] as scilmm_solve_L_dev writes it; 1 <= q <= 32.
 *   d_stats: (q + 4) x r row-major: n_obs | mean over the observed | centred sum of squares over the observed |
 *            |w(g~)|^2 | the q rows of Q^T w(g~), where g~ = genotype minus the marker's mean, missing = 0 (mean imputation).
 * Everything is enqueued on the handle's stream without synchronising; the n x r block never leaves the engine's work
 * buffers.  Every sum is taken in an order that depends on (n, r) alone and without floating-point atomics, so the call
 * adds to scilmm_timing.n_float_atomic_launches only what its forward sweep adds (nothing in deterministic mode).
 * Arguments out of range or null: SCILMM_ERR_ARG; refusals as for the half-solves.  No counterpart in the reference. */
int scilmm_scan_block_dev(scilmm_factor* fac, const int8_t* d_geno, int64_t ld_geno, int32_t r, const double* d_Q, int32_t q,
                          double* d_stats);

/* scilmm_scan_block_dev for markers as they lie in a PLINK 1 binary file (.bed, variant-major): the 2-bit genotypes are
 * decoded, and gathered through a sample map, inside the two kernels that build the sweep's right-hand side; the forward
 * sweep and the statistics are those of scilmm_scan_block_dev.
 *   d_bed    : marker j of the block = d_bed + j * ld_bed, ceil(n_samples / 4) bytes: sample s is bits 2 (s & 3) .. 2 (s & 3) + 1
 *              of byte s >> 2; 00 = two copies of allele A1, 01 = missing, 10 = one copy, 11 = none.  The bits past the
 *              last sample are ignored.  ld_bed >= ceil(n_samples / 4), so a slab of the file (after its 3 magic bytes) is
 *              taken as it is.  Any alignment, under the rule of d_geno: aligned 16-byte pieces, the buffer inside an
 *              allocation that starts and ends on 16-byte boundaries.
 *   n_samples: samples per row of the file (N), >= 1.
 *   d_sample : n int32, d_sample[i] = the file's sample of individual i (the row order of the matrices).  Any value outside
 *              0 .. n_samples - 1, every negative one included, = not genotyped: missing for every marker, and no byte is
 *              read for it.  Two individuals may share a sample.  NULL = identity; n_samples must then equal n.  With a
 *              map the rows are read byte by byte at row + (sample >> 2).
 *   flags    : bit 0 set = count allele A2 (g -> 2 - g for the observed); every other bit must be 0.
 *   r, d_Q, q, d_stats: as for scilmm_scan_block_dev; d_stats is (q + 4) x r with the same rows.
 * The moments are integer sums through the expressions of the int8 path and W holds the same doubles, so the statistics
 * are bit for bit those of scilmm_scan_block_dev on the unpacked, gathered markers; no atomics of any kind are added.
 * Everything is enqueued on the handle's stream without synchronising; scilmm_scan_timing reports decode + moments +
 * dequantise in ms[0] for these blocks.  SCILMM_ERR_ARG before anything is dereferenced: a null d_bed, d_Q or d_stats, r or q
 * out of range, n_samples < 1, ld_bed < ceil(n_samples / 4), an unknown flag bit, a null d_sample with n_samples != n;
 * refusals as for the half-solves (a distributed handle, fp32-product fronts, a factor consumed by the selected
 * inverse).  No counterpart in the reference: it reads no genotype files, and its only per-variable test is
 * compute_fixed_effects_p_value on the covariates of the fit (scilmm/Estimation/LMM.py:129-133). */
int scilmm_scan_block_bed_dev(scilmm_factor* fac, const uint8_t* d_bed, int64_t ld_bed, int32_t n_samples, const int32_t* d_sample,
                              int32_t flags, int32_t r, const double* d_Q, int32_t q, double* d_stats);

/* The two scan blocks above with one more output, for variant-SET tests (burden, SKAT / famSKAT): besides the per-marker
 * statistics the block hands back the Gram matrix of its whitened markers,
 *   d_gram : r x r row-major, leading dimension r: d_gram[i][j] = w(g~_i)' w(g~_j) = g~_i' V^-1 g~_j.
 * With X the forward solution and Z = R^-T w(C)' X (R'R = w(C)'w(C); w(C)'X are rows 4 .. of d_stats), X'X - Z'Z is
 * G~' P_V G~ (P_V = V^-1 - V^-1 C (C' V^-1 C)^-1 C' V^-1): the null covariance of the score vector G~' P_V y, whose entries
 * the scan's statistics already give.  The forward solution is read a second time where it lies, on the fp64 matrix pipe
 * (v_mfma_f64_16x16x4_f64; lower-triangle tiles in fixed row slices, folded in slice order, no floating-point atomics),
 * so every entry's bits depend on (n, r) alone in either mode of the handle, the matrix is symmetric bit for bit, and
 * exactly r * r doubles are written.  Its diagonal is row 3 of d_stats summed in another order (agreement to rounding, not
 * bit for bit).  d_stats holds the bits the plain entry point writes: the launches before the Gram are the same.
 * Everything else -- arguments, their checks, the refusals, the stream, scilmm_scan_timing (the Gram counts into ms[2]) --
 * is as for the plain entry points; a null d_gram: SCILMM_ERR_ARG.  The slice partials (12 MB per 100k individuals) are
 * allocated by the first such call on a handle, nothing per block afterwards.  scilmm_amd.VariantSetTest is the
 * interface.  No counterpart in the reference. */
int scilmm_scan_block_gram_dev(scilmm_factor* fac, const int8_t* d_geno, int64_t ld_geno, int32_t r, const double* d_Q, int32_t q,
                               double* d_stats, double* d_gram);
int scilmm_scan_block_bed_gram_dev(scilmm_factor* fac, const uint8_t* d_bed, int64_t ld_bed, int32_t n_samples, const int32_t* d_sample,
                                   int32_t flags, int32_t r, const double* d_Q, int32_t q, double* d_stats, double* d_gram);

/* The two scan blocks for IMPUTED DOSAGES: expected allele counts in [0, 2] (BGEN / pgen / VCF DS readers) instead of hard
 * calls, in one of two element types, with the sample map of scilmm_scan_block_bed_dev.  Only the two kernels that build
 * the sweep's right-hand side know the element type; the forward sweep, the statistics and the Gram matrix are those of
 * the int8 entry points.
 *   d_dos    : marker j of the block = d_dos + j * ld ELEMENTS, n_samples elements; aligned to the element size, otherwise
 *              any alignment under the rule of d_geno (aligned 16-byte pieces, the buffer inside an allocation that starts
 *              and ends on 16-byte boundaries).
 *   dtype    : SCILMM_DOSAGE_U16 -- uint16, PLINK 2's fixed point: 16384 = 1.0, 32768 = 2.0, any code above 32768 = missing
 *              (65535 is the canonical code).  The moments are 64-bit integer sums of the codes, scaled by powers of two
 *              and put through the expressions of the int8 path (mean = sum / cnt, css = sq - sum * mean), so a marker of
 *              hard calls coded g * 16384 gives the statistics of scilmm_scan_block_dev bit for bit, and a constant marker
 *              has a centred sum of squares of exactly 0.
 *              SCILMM_DOSAGE_F32 -- float: a non-finite value = missing, any finite value is taken at face value (the path
 *              also serves an arbitrary quantitative candidate covariate).  fp64 sums in a fixed order (one workgroup per
 *              marker, a fixed thread stride and a fixed tree; no atomics): a call repeats its bits.  The centred sum of
 *              squares is a second pass, sum of (g - mean)^2, and exactly 0 when the smallest observed value equals the
 *              largest.  The order of the sums depends on n_samples and on the row's offset inside its 16-byte piece (with
 *              a map: on n alone), so rows that start on 16-byte boundaries give the same bits wherever they lie.
 *   ld       : elements between rows, >= n_samples.
 *   n_samples, d_sample: as for scilmm_scan_block_bed_dev (a sample outside 0 .. n_samples - 1 = not genotyped, nothing is
 *              read for it; NULL = identity, n_samples must equal n).  With a map the rows are read element by element.
 *   r, d_Q, q, d_stats, d_gram: as for scilmm_scan_block_dev / scilmm_scan_block_gram_dev.
 * Everything is enqueued on the handle's stream without synchronising; scilmm_scan_timing reports moments + dequantise in
 * ms[0].  SCILMM_ERR_ARG before anything of the handle is read: a null d_dos (d_gram in the Gram form), d_Q or d_stats, an
 * unknown dtype, d_dos not aligned to its element size, n_samples < 1, ld < n_samples, r or q out of range, a null d_sample
 * with n_samples != n; refusals as for the half-solves.  scilmm_amd.AssociationScan.scan_dosages and
 * VariantSetTest.test_dosages are the interfaces.  No counterpart in the reference. */
enum { SCILMM_DOSAGE_U16 = 0, SCILMM_DOSAGE_F32 = 1 };
int scilmm_scan_block_dosage_dev(scilmm_factor* fac, const void* d_dos, int32_t dtype, int64_t ld, int32_t n_samples,
                                 const int32_t* d_sample, int32_t r, const double* d_Q, int32_t q, double* d_stats);
int scilmm_scan_block_dosage_gram_dev(scilmm_factor* fac, const void* d_dos, int32_t dtype, int64_t ld, int32_t n_samples,
                                      const int32_t* d_sample, int32_t r, const double* d_Q, int32_t q, double* d_stats,
                                      double* d_gram);

/* The three scan blocks for a marker x environment INTERACTION test (G x E): every marker of the block is tested with d = 1 + m
 * terms, its own column g~ and g~ o e_1 .. g~ o e_m (o = the entry-wise product with an environment column: sex, treatment,
 * herd, age, diet), so the interaction columns differ from marker to marker and cannot be covariates of the scan.  The
 * whitening identity of scilmm_scan_block_dev holds term by term: GLS of y on [C, g~, g~ o e_1 ..] under V is OLS on the
 * whitened columns, so a marker costs d columns of the forward sweep and one symmetric d x d system on the host.
 *   d_E    : n x m row-major, PERMUTED order (the order of d_Q: row p = individual perm[p]); 1 <= m <= 3.  The columns are
 *            expected among the covariates behind d_Q (the main effects in the null model): g~ o e_a is then g o e_a with mean
 *            imputation after projection, and nothing else needs centring.  The entry points do not check it.
 *   r      : markers in the block, 1 .. 128 / d rounded down (64, 42, 32).
 *   d_stats: (3 + (q + 1) d + d (d - 1) / 2) x r row-major:
 *            rows 0 .. 2           n_obs | mean | centred sum of squares, as scilmm_scan_block_dev writes them;
 *            row 3 + k d + a       quantity k of term a: k = 0 is |x_a|^2, k = 1 .. q is row k - 1 of Q^T x_a, where
 *                                  x_a = w(g~ o e_a), x_0 = w(g~);
 *            then                  x_a' x_b for the pairs (a, b), a < b, in lexicographic order.
 *   the form's own arguments, d_Q, q: as for the plain entry point of the form.
 * The block has d r columns, column a r + c = term a of marker c: the form's two kernels write columns 0 .. r - 1 as ever,
 * k_scan_expand multiplies them into columns r .. d r - 1 in place (one kernel for every form), the forward sweep and
 * the statistics are those of scilmm_scan_block_dev on d r columns -- its (q + 1) x (d r) output is rows 3 .. of d_stats
 * as they stand -- and k_scan_cross reads the forward solution a second time where it lies for the pairs: fixed row
 * slices, rows in ascending order, folded by the statistics' own tree; no floating-point atomics, so every number's bits
 * depend on (n, r, m) alone in either mode of the handle and the call adds to scilmm_timing.n_float_atomic_launches only
 * what its forward sweep adds.  The pairs' partial sums live in the statistics' buffer: nothing is allocated per block.
 * Everything is enqueued on the handle's stream without synchronising; scilmm_scan_timing counts the expansion into ms[0]
 * and the cross products into ms[2], scilmm_gxe_timing reports the two alone.  SCILMM_ERR_ARG before anything of the handle
 * is read: a null d_E, m outside 1 .. 3, r outside 1 .. 128 / d, and everything the plain entry point of the form rejects;
 * refusals as for the half-solves (a distributed handle, fp32-product fronts, a factor consumed by the selected inverse).
 * scilmm_amd.InteractionScan (AssociationScan.interaction) is the interface.  No counterpart in the reference. */
int scilmm_scan_block_gxe_dev(scilmm_factor* fac, const int8_t* d_geno, int64_t ld_geno, int32_t r, const double* d_E, int32_t m,
                              const double* d_Q, int32_t q, double* d_stats);
int scilmm_scan_block_bed_gxe_dev(scilmm_factor* fac, const uint8_t* d_bed, int64_t ld_bed, int32_t n_samples, const int32_t* d_sample,
                                  int32_t flags, int32_t r, const double* d_E, int32_t m, const double* d_Q, int32_t q,
                                  double* d_stats);
int scilmm_scan_block_dosage_gxe_dev(scilmm_factor* fac, const void* d_dos, int32_t dtype, int64_t ld, int32_t n_samples,
                                     const int32_t* d_sample, int32_t r, const double* d_E, int32_t m, const double* d_Q, int32_t q,
                                     double* d_stats);

/* HIP-event times of the last scilmm_scan_block_dev on the handle, in milliseconds, valid after the scilmm_sync that follows
 * it: ms[0] moments + dequantise (+ permute), ms[1] forward sweep, ms[2] statistics (tools/assoc_timing.py). */
int scilmm_scan_timing(const scilmm_symbolic* sym, double* ms);

/* The two kernels a gxe block adds, of the last scan block on the handle, in milliseconds, valid after the scilmm_sync that
 * follows it: ms[0] k_scan_expand (part of scilmm_scan_timing's ms[0]), ms[1] k_scan_cross and its fold (part of its ms[2]);
 * zeros after a block that was no gxe block (tools/gxe_timing.py). */
int scilmm_gxe_timing(const scilmm_symbolic* sym, double* ms);

/* Phenotype panels: X^T Y for the forward solution X that the LAST scan block on this handle left behind (any form: plain,
 * Gram or gxe -- for gxe, r is the block's d r columns) and a resident panel Y of t phenotype columns.  The whitened markers
 * do not depend on the phenotype, so one forward sweep serves any number of traits, or of simulated null phenotypes (a
 * parametric bootstrap of the genome-wide maximum): one more GEMM-shaped pass over X on the fp64 matrix pipe.
 *   r      : columns of the block left behind, 1 .. 128; it must be the r of that block.
 *   d_Y    : n x ld_y row-major, PERMUTED order (the order of d_Q), 16-byte aligned; t <= ld_y, ld_y % 16 == 0.  The values
 *            of the padding columns t .. ld_y - 1 reach no output (they may be anything, NaN included).
 *   t      : columns of the panel, 1 .. 4096.
 *   d_xty  : r x t, leading dimension ld_out >= t: xty[j][k] = x_j . y_k.  Exactly r t numbers are written.
 * Fixed row slices, folded in a fixed tree, no floating-point atomics: the bits of xty[j][k] depend on n and on the values of
 * x_j and y_k alone -- not on t, on where y_k sits in Y, on r, or on the mode of the handle -- and
 * scilmm_timing.n_float_atomic_launches is not touched.  The call is enqueued on the handle's stream without synchronising;
 * it writes nothing of the work buffers, so several panels may follow one block.  Its partial tiles are allocated on the
 * first call and grown for a wider panel only (the stream is synchronised before that).
 * SCILMM_ERR_ARG before anything is dereferenced: a null fac, d_Y or d_xty, r outside 1 .. 128, t outside 1 .. 4096,
 * ld_y < t or ld_y % 16 != 0, ld_out < t, d_Y not 16-byte aligned.  SCILMM_ERR_STATE with a message, the handle left usable:
 * no block left behind -- whatever may overwrite the work buffers (a solve, a half-solve, L*R, a product) forgets it, and so
 * do a refactorization and scilmm_inverse_traces -- or another r than that block's; refusals as for the half-solves (a
 * distributed handle, fp32-product fronts, a factor consumed by the selected inverse).  scilmm_scan_timing is unaffected;
 * scilmm_panel_timing reports the call's own two kernels.  scilmm_amd.TraitPanel (AssociationScan.traits, .null_panel) is
 * the interface.  No counterpart in the reference. */
int scilmm_scan_panel_dev(scilmm_factor* fac, int32_t r, const double* d_Y, int64_t ld_y, int32_t t, double* d_xty, int64_t ld_out);

/* HIP-event times of the last scilmm_scan_panel_dev on the handle, in milliseconds, valid after the scilmm_sync that
 * follows it: ms[0] k_scan_panel, ms[1] k_panel_fold (tools/panel_timing.py).  No counterpart in the reference. */
int scilmm_panel_timing(const scilmm_symbolic* sym, double* ms);

/* Variant sets wider than one block: keep the forward solution X that the LAST scan block on this handle left behind (any
 * form), so that the sub-blocks that follow can form their cross products X_b^T X_a against it with scilmm_scan_panel_dev.  X is
 * n x rp row-major in the PERMUTED row order, rp = r rounded up to 16, columns r .. rp - 1 zero; element (i, j) goes to
 * d_dst[i * ld_dst + col0 + j].
 *   r      : columns of the block left behind, 1 .. 128; it must be the r of that block.
 *   d_dst  : the store, n x ld_dst row-major, 16-byte aligned; ld_dst % 16 == 0 and ld_dst >= col0 + rp.
 *   col0   : first column of the store that is written, >= 0 and a multiple of 16.
 * Exactly n rp doubles are written, the zero padding included: the store can go to scilmm_scan_panel_dev as d_Y (ld_y = ld_dst,
 * t = the columns kept so far) without a memset; nothing outside columns col0 .. col0 + rp - 1 is touched.  One store-only
 * kernel (k_scan_keep: 16-byte loads, 16-byte stores, no LDS, no atomics) is enqueued on the handle's stream without
 * synchronising; scilmm_timing.n_float_atomic_launches is not touched.  It writes nothing of the work buffers and does not
 * forget the block: a Gram pass has come before it, and panels and further keeps may follow the same block.  Nothing is allocated.
 * SCILMM_ERR_ARG before anything is dereferenced: a null fac or d_dst, r outside 1 .. 128, col0 < 0 or col0 % 16 != 0,
 * ld_dst % 16 != 0 or ld_dst < col0 + rp, d_dst not 16-byte aligned.  SCILMM_ERR_STATE with a message, the handle left usable,
 * as for scilmm_scan_panel_dev: no block left behind, or another r than that block's; refusals as for the half-solves (a
 * distributed handle, fp32-product fronts, a factor consumed by the selected inverse).  scilmm_amd.VariantSetTest with
 * max_markers is the interface.  No counterpart in the reference. */
int scilmm_scan_block_keep_dev(scilmm_factor* fac, int32_t r, double* d_dst, int64_t ld_dst, int64_t col0);

/* Binary traits: the saddlepoint (SPA) p-value of the score test for the r markers of a plain scan block, queued BEHIND that
 * block (scilmm_scan_block_dev, _bed_dev or _dosage_dev with the same marker arguments and the same r) on the handle's stream.
 * With the working vector y~ of a logistic mixed model in the place of y (scilmm_amd.glmm), the block's statistics hold the
 * score b = g~' P y~ and its variance a = g~' P g~; the call reads them where the block wrote them and re-reads the marker rows.
 *   d_stats : the block's (q + 4) x r statistics, q = c + 1.
 *   d_R, d_u: c x c upper triangular R with R'R = w(C)'w(C), row-major, and u = R^-T w(C)'w(y~) (c numbers).
 *   d_mu    : n fitted probabilities in the ORIGINAL order of the individuals, each in (0, 1).
 *   d_C     : n x c covariates, row-major, original order.   c: 1 .. 31.
 *   d_Minv  : (C' W C)^-1, c x c, W = diag(mu (1 - mu)).
 *   cutoff  : >= 0; a marker with |b / sqrt(a)| <= cutoff is not saddlepointed (flag 0).
 *   d_spa   : 7 x r row-major, rows  log_p | a_w | s | zeta_hi | zeta_lo | iters | flag:
 *             g^ = g~ - C Minv C'W g~,  a_w = sum w_i g^_i^2,  s = b sqrt(a_w / a);  zeta_hi > 0 > zeta_lo are the roots of
 *             K'(zeta) = +-|s| for the cumulant generating function K of sum g^_i (y_i - mu_i) under independent Bernoulli(mu_i)
 *             draws (safeguarded Newton from 0, |step| <= 1e-13 max(1, |zeta|), at most 64 steps per root; iters = the larger
 *             count); log_p = log of the sum of the two Lugannani-Rice tails, taken in logarithms (finite far beyond where p
 *             underflows).  flag 1: both roots converged and both tail arguments are finite and positive.  flag 2: anything
 *             else (|s| outside the support of the statistic, the step limit, a non-positive argument): log_p is the normal
 *             value log(2 Phi(-|b| / sqrt(a))).  flag 0: not attempted (no observed value, no variation, a <= 0, or within the
 *             cutoff): the other six rows are NaN.
 * One workgroup per marker, fixed thread stride and fixed reduction trees, no atomics: a marker's seven numbers depend on its
 * inputs alone, in either mode of the handle, and the three input forms of the same hard calls give the same bits;
 * scilmm_timing.n_float_atomic_launches is not touched.  Nothing of the work buffers is written (a scilmm_scan_panel_dev may
 * still follow the block).  The call keeps g^ in a scratch of 128 x n doubles that the first call on a handle allocates (the
 * stream is synchronised before that) and no later call reallocates.  Enqueued without synchronising.
 * SCILMM_ERR_ARG before anything is dereferenced: a null pointer, r outside 1 .. 128, c outside 1 .. 31, cutoff negative or
 * NaN, and whatever the plain entry point of the form rejects in the marker arguments.  Refusals as for the half-solves
 * (SCILMM_ERR_STATE, the handle left usable): a distributed handle, fp32-product fronts, a factor consumed by the selected
 * inverse.  scilmm_amd.glmm.BinaryScan is the interface.  No counterpart in the reference. */
int scilmm_scan_spa_dev(scilmm_factor* fac, const int8_t* d_geno, int64_t ld_geno, int32_t r, const double* d_stats, const double* d_R,
                        const double* d_u, const double* d_mu, const double* d_C, int32_t c, const double* d_Minv, double cutoff,
                        double* d_spa);
int scilmm_scan_spa_bed_dev(scilmm_factor* fac, const uint8_t* d_bed, int64_t ld_bed, int32_t n_samples, const int32_t* d_sample,
                            int32_t flags, int32_t r, const double* d_stats, const double* d_R, const double* d_u, const double* d_mu,
                            const double* d_C, int32_t c, const double* d_Minv, double cutoff, double* d_spa);
int scilmm_scan_spa_dosage_dev(scilmm_factor* fac, const void* d_dos, int32_t dtype, int64_t ld, int32_t n_samples,
                               const int32_t* d_sample, int32_t r, const double* d_stats, const double* d_R, const double* d_u,
                               const double* d_mu, const double* d_C, int32_t c, const double* d_Minv, double cutoff, double* d_spa);

/* HIP-event time of the last scilmm_scan_spa*_dev on the handle, in milliseconds, valid after the scilmm_sync that follows it:
 * ms[0] k_scan_spa (tools/spa_timing.py).  No counterpart in the reference. */
int scilmm_spa_timing(const scilmm_symbolic* sym, double* ms);

/* Variant-set tests: everything AFTER a Gram block (scilmm_scan_block_gram_dev or a twin of it), for the sets the block holds --
 * burden, SKAT and SKAT-O (Lee, Wu, Lin 2012) -- on the device, queued behind the block on the handle's stream.  A pure function
 * of what the block left behind: nothing of the factor is read, no work buffer is written, nothing is allocated.
 *   r, q, d_stats, d_gram: the block's markers, its q = c + 1, its (q + 4) x r statistics and its r x r Gram matrix.
 *            Of d_gram the sets' diagonal blocks are read, both triangles: entry (i, j) is taken as the mean of [i][j] and [j][i]
 *            (the Gram entry points write a bitwise symmetric matrix, so nothing changes for them).
 *   d_R, d_u, c: as for scilmm_scan_spa_dev (R'R = w(C)'w(C) upper triangular row-major, u = R^-T w(C)'w(y)); c: 1 .. 31.
 *   n_sets, set_start: HOST, n_sets + 1 int32 offsets into the block's columns, rising from 0 to at most r: set i is columns
 *            set_start[i] .. set_start[i + 1] - 1 (sets are contiguous and disjoint, in the order scilmm_amd.sets.pack_sets lays
 *            them out); 1 <= n_sets <= r.  Read before the call returns, like the ids of scilmm_rel_block_dev.
 *   weight_mode: 0 = the Beta(1, 25) density at the minor allele frequency from the `mean` row, 25 (1 - maf)^24,
 *            maf = min(mean / 2, 1 - mean / 2); 1 = ones; 2 = d_weights, r doubles on the device, one per column of the block
 *            (d_weights is not read in the other modes and may be null).
 *   method : the mixtures' tail, 0 = saddlepoint (Lugannani-Rice, with the seam of the host form), 1 = modified Liu.
 *   rho, n_rho: HOST, the SKAT-O grid, 0 .. 16 values in [0, 1] (a value above 0.999 is computed as 0.999); n_rho = 0: no
 *            SKAT-O (rho may then be null).
 *   d_out  : n_sets rows of ld_out >= 10 + n_rho doubles; row i:  n_used | burden_beta | burden_se | burden_chi2 | skat_q |
 *            skat_p | skato_p | skato_pmin | skato_rho | flags | the n_rho per-rho p-values.  A marker without an observed value
 *            or without variation is dropped from its set; a set with nothing left: n_used = 0, flags = 0, the rest NaN.
 *            Without SKAT-O the three skato numbers are NaN.  flags: bit 0 the degenerate rule answered (one marker, 1'A1 = 0
 *            or A of rank one: skato_p = skato_pmin, skato_rho = the first grid value; or skato_pmin = 0), bit 1 the Jacobi
 *            iteration ran out of sweeps, bit 2 a root ran out of steps, bit 3 SKAT-O was computed.  Exactly 10 + n_rho doubles
 *            of every row are written.
 *   d_lam  : null, or r doubles: the columns of a set's kept markers receive the eigenvalues of A = diag(w) K diag(w) in
 *            descending order, the columns of its dropped markers NaN; columns outside every set are not written.
 * With s, K as in scilmm_scan_block_gram_dev's contract, t = w o s and A = diag(w) K diag(w): Q_rho = (1 - rho) t't +
 * rho (1't)^2 has the null law sum lambda_i chi2_1 with the eigenvalues of A R_rho, R_rho = (1 - rho) I + rho 11'; skato_pmin is
 * the smallest of their p-values, skato_rho the first grid value that attains it, and skato_p the integral of DESIGN.md
 * section 19 in survival form, bounded by n_rho skato_pmin.  One workgroup per set with the set in LDS (sized by the block's
 * largest set: the call raises the kernel's dynamic-LDS limit once per device): one Jacobi eigendecomposition A = U Lambda U',
 * the other spectra as roots of secular equations on (Lambda, U'1).  No atomics, fixed strides and fixed reduction trees: a
 * set's numbers depend on its own inputs alone -- not on its place in the block, its neighbours or the mode of the handle --
 * and scilmm_timing.n_float_atomic_launches is not touched.  burden_p is left to the caller (F(1, n - 1) of burden_chi2).
 * Enqueued without synchronising.  SCILMM_ERR_ARG before anything of the handle or of the device is read: a null fac, d_stats,
 * d_gram, d_R, d_u, set_start or d_out (rho with n_rho > 0, d_weights in mode 2), r outside 1 .. 128, c outside 1 .. 31,
 * q != c + 1, n_sets outside 1 .. r, n_rho outside 0 .. 16, a rho outside [0, 1] or NaN, offsets that do not start at 0, do not
 * rise strictly or end beyond r, ld_out < 10 + n_rho, an unknown weight mode or method.  Refusals as for the scan blocks
 * (SCILMM_ERR_STATE, the handle left usable): a distributed handle, fp32-product fronts, a factor consumed by the selected
 * inverse.  scilmm_amd.VariantSetTest with finish="device" is the interface.  No counterpart in the reference. */
int scilmm_sets_finish_dev(scilmm_factor* fac, int32_t r, int32_t q, const double* d_stats, const double* d_gram, const double* d_R,
                           const double* d_u, int32_t c, int32_t n_sets, const int32_t* set_start, int32_t weight_mode,
                           const double* d_weights, int32_t method, const double* rho, int32_t n_rho, double* d_out, int64_t ld_out,
                           double* d_lam);

/* HIP-event time of the last scilmm_sets_finish_dev on the handle, in milliseconds, valid after the scilmm_sync that follows
 * it: ms[0] k_sets_finish (tools/sets_timing.py --finish).  No counterpart in the reference. */
int scilmm_sets_finish_timing(const scilmm_symbolic* sym, double* ms);

/* Variant-set tests over a phenotype panel: scilmm_sets_finish_dev for the sets of a Gram block against t traits at once
 * (DESIGN.md section 24), queued on the handle's stream behind the block and the scilmm_scan_panel_dev that formed the traits'
 * scores.  Of the finish only the score depends on the trait: the projection K = G - z'z, A = diag(w) K diag(w), its Jacobi
 * eigendecomposition, the secular equations of every A R_rho and of the remainder term, the floors and the Liu moments are
 * computed ONCE per set (k_sets_spectra, one workgroup per set) and kept as a record in a scratch buffer of the handle; one
 * workgroup per (set, group of traits) then loads the record and runs the tails, T = min p_rho and the SKAT-O integral per trait
 * (k_sets_panel_tail) with the routines scilmm_sets_finish_dev runs.
 *   r, q, d_stats, d_gram, d_R, c, n_sets, set_start, weight_mode, d_weights, method, rho, n_rho: as for scilmm_sets_finish_dev.
 *            There is no u: the traits arrive projected off the whitened covariates, so a trait's score is its column of d_xty
 *            as it stands; the score row of d_stats is not used.
 *   d_xty, ld_xty, t: the r x t scores X'Y~ as scilmm_scan_panel_dev wrote them (row = the block's column, column = the trait),
 *            ld_xty >= t doubles between rows; 1 <= t <= 4 096.
 *   d_tscale: null (every scale 1), or t positive finite scales on the device: trait k is tested with t = w o s / sqrt(scale_k),
 *            which divides burden_chi2 and skat_q by scale_k (scale="profile" of scilmm_amd.panel).
 *   d_head : n_sets rows of 4 doubles:  n_used | w'Kw | the set's flag word (bit 1 the Jacobi iteration ran out of sweeps, bit 2
 *            a secular root ran out of steps) | 0.
 *   d_out  : n_sets t rows of 8 doubles, row = set t + trait:  1'(w o s), unscaled | burden_chi2 | skat_q | skat_p | skato_p |
 *            skato_pmin | skato_rho | flags (the set's, and the trait's as scilmm_sets_finish_dev sets them).  burden_beta =
 *            1'(w o s) / w'Kw and burden_se = (scale / w'Kw)^1/2 are the caller's, as is burden_p.  A set with nothing left:
 *            n_used = 0, w'Kw NaN, flags 0, every row of it NaN with flags 0.  Without SKAT-O (n_rho = 0) the three skato numbers
 *            are NaN.  Exactly 4 n_sets and 8 n_sets t doubles are written.
 * The traits of a tail workgroup (1 .. 32) are chosen by the engine so that sets x groups covers the device several times over;
 * the environment variable SCILMM_SETS_PANEL_GROUP=<1 .. 32>, read per call, takes its place.  No atomics, fixed strides and
 * fixed reduction trees: the numbers of a (set, trait) pair depend on that set's inputs and that trait's column alone -- not on
 * t, the group size, the set's place in the block or the mode of the handle -- and scilmm_timing.n_float_atomic_launches is not
 * touched.  They agree with scilmm_sets_finish_dev on the same score to rounding in the sums (1e-9) and to the accuracy of the
 * tails (1e-6), not bit for bit.  The records (n_sets (96 + (n_rho + 3) cap) doubles, cap the block's largest set) are the
 * handle's: grown behind a stream synchronise, never allocated again for the same or a smaller call.  Enqueued without
 * synchronising; nothing of the factor is read.  SCILMM_ERR_ARG before anything of the handle or of the device is read: what
 * scilmm_sets_finish_dev rejects of the arguments they share, a null d_xty, d_head or d_out, t outside 1 .. 4 096, ld_xty < t,
 * and a scale that is not finite and positive where d_tscale is memory the host can read (pinned or managed; scales in device
 * memory are the caller's to check).  Refusals as for scilmm_sets_finish_dev.  scilmm_amd.VariantSetTest.set_traits is the
 * interface.  No counterpart in the reference. */
int scilmm_sets_finish_panel_dev(scilmm_factor* fac, int32_t r, int32_t q, const double* d_stats, const double* d_gram, const double* d_R,
                                 int32_t c, int32_t n_sets, const int32_t* set_start, int32_t weight_mode, const double* d_weights,
                                 int32_t method, const double* rho, int32_t n_rho, const double* d_xty, int64_t ld_xty, int32_t t,
                                 const double* d_tscale /* t scales or NULL = 1 */, double* d_head, double* d_out);

/* HIP-event times of the last scilmm_sets_finish_panel_dev on the handle, in milliseconds, valid after the scilmm_sync that
 * follows it: ms[0] k_sets_spectra, ms[1] k_sets_panel_tail (tools/sets_panel_timing.py).  No counterpart in the reference. */
int scilmm_sets_finish_panel_timing(const scilmm_symbolic* sym, double* ms);

/* Variant-set tests under annotation masks and MAF cutoffs: scilmm_sets_finish_dev for every set of a
 * Gram block under n_ann masks crossed with n_cut cutoffs of the minor allele frequency, with ACAT-V (Liu et al. 2019, in
 * STAAR's form) next to burden, SKAT and SKAT-O, queued on the handle's stream behind the block.  Every cell of a set is a
 * principal submatrix of the set's K and a sub-vector of its score: the block is swept once, and one workgroup per
 * (set, annotation, cutoff) finishes its cell from the statistics and the Gram matrix where the block left them
 * (k_sets_finish_masks, the threads and the LDS of k_sets_finish).
 *   r, q, d_stats, d_gram, d_R, d_u, c, n_sets, set_start, weight_mode, d_weights, method, rho, n_rho: as for
 *            scilmm_sets_finish_dev.
 *   d_ann, n_ann: r uint32 words on the device, one per column of the block: bit a set = the column is in annotation a;
 *            1 <= n_ann <= 32 (bits from n_ann up are not looked at).
 *   maf_cut, n_cut: HOST, 1 .. 8 cutoffs in (0, 0.5], read before the call returns.
 *   acat_mac: >= 0 and finite: ACAT-V pools the markers whose minor allele count is at most this.
 *   d_out  : n_sets n_ann n_cut rows of ld_out >= 12 + n_rho doubles, row = (set n_ann + a) n_cut + f.  Cell (a, f) of a set
 *            holds the columns that scilmm_sets_finish_dev keeps AND that carry bit a AND whose maf <= maf_cut[f], with
 *            maf = min(0.5 mean, 1 - 0.5 mean) from the `mean` row (the expression of weight mode 0; scilmm_amd.set_masks.maf_of
 *            is the same expression on the host, so membership cannot differ between the two).  The first 10 + n_rho doubles
 *            are the row of scilmm_sets_finish_dev for a block that holds the cell's columns alone -- the same routines on the
 *            cell's index list, the same bits --, then  acatv_p | n_pooled.  An empty cell: n_used = 0, flags = 0,
 *            n_pooled = 0, the rest NaN.  Exactly 12 + n_rho doubles of every row are written.
 * ACAT-V of a cell, from s, w and K of its kept markers: mac_j = 2 n_obs_j maf_j; a marker with mac_j > acat_mac and K_jj > 0
 * is a term p_j = erfc(sqrt(s_j^2 / 2 K_jj)) of weight omega_j = w_j^2 maf_j (1 - maf_j); the markers with mac_j <= acat_mac
 * (n_pooled of them) are one term, p = erfc(sqrt((sum w_j s_j)^2 / 2 sum_ij w_i K_ij w_j)) over the pool, left out where the
 * quadratic form is not positive, of weight the mean of the pool's omega_j.  Terms of weight 0 are left out; without a term
 * acatv_p is NaN.  T = sum omega tan((0.5 - p) pi) / sum omega, with p capped at 1 - 1e-15 and 1 / (p pi) for the tangent
 * where p < 1e-15; acatv_p = 0.5 - atan(T) / pi, 1 / (T pi) where T > 1e15; a term with p = 0 gives 0.  (The two functions
 * are evaluated without their cancellations: the tangent as 1 / tan(p pi) below p = 0.5, the p-value as atan(1 / T) / pi above
 * T = 1, so a small p keeps its digits and the branches are continuous.  The kernel takes s_j^2 / K_jj as t_j^2 / A_jj from
 * t = w o s and A = diag(w) K diag(w) while A is in LDS: the same number wherever omega_j > 0, and no division by a weight.)
 * No atomics: every sum runs in ascending column order or by the fixed fold, a
 * cell's numbers depend on its own inputs alone, and scilmm_timing.n_float_atomic_launches is not touched.  Enqueued without
 * synchronising; nothing is allocated and nothing of the factor is read.  SCILMM_ERR_ARG before anything of the handle or of
 * the device is read: what scilmm_sets_finish_dev rejects, a null d_ann or maf_cut, n_ann outside 1 .. 32, n_cut outside
 * 1 .. 8, a cutoff outside (0, 0.5] or NaN, acat_mac negative or not finite, ld_out < 12 + n_rho.  Refusals as for
 * scilmm_sets_finish_dev.  scilmm_amd.VariantSetTest.masks is the interface.  No counterpart in the reference. */
int scilmm_sets_finish_masks_dev(scilmm_factor* fac, int32_t r, int32_t q, const double* d_stats, const double* d_gram, const double* d_R,
                                 const double* d_u, int32_t c, int32_t n_sets, const int32_t* set_start, int32_t weight_mode,
                                 const double* d_weights, int32_t method, const double* rho, int32_t n_rho, const uint32_t* d_ann,
                                 int32_t n_ann, const double* maf_cut, int32_t n_cut, double acat_mac, double* d_out, int64_t ld_out);

/* HIP-event time of the last scilmm_sets_finish_masks_dev on the handle, in milliseconds, valid after the scilmm_sync that
 * follows it: ms[0] k_sets_finish_masks (tools/sets_masks_timing.py).  No counterpart in the reference. */
int scilmm_sets_finish_masks_timing(const scilmm_symbolic* sym, double* ms);

/* The finish of ONE variant set of k markers, 1 <= k <= 4 096, that ran as B = ceil(k / block) sub-blocks (DESIGN.md section
 * 22), queued on the handle's stream behind the last of them; everything scilmm_sets_finish_dev computes for a set, for a set
 * wider than one block.  With bp = block rounded up to 16: (B - 1) bp <= 4 096.
 *   block  : 1 .. 128, the markers of every sub-block but the last; sub-block b holds r_b = min(block, k - b block).
 *   d_stats: B slices at a stride of (q + 4) block doubles; slice b is the (q + 4) x r_b array scilmm_scan_block_gram_dev (or a
 *            twin) wrote for sub-block b.   d_gram: B slices at a stride of block^2; slice b is r_b x r_b.
 *   d_cross: row i (the marker's index in the set) holds the b bp columns scilmm_scan_panel_dev wrote for it, b = i / block:
 *            column a bp + j is marker a block + j, the padding columns are not read; ld_cross >= (B - 1) bp doubles between
 *            rows.  Null exactly when B = 1.
 *   d_R, d_u, c, q = c + 1, weight_mode, method, rho, n_rho: as for scilmm_sets_finish_dev; d_weights: k doubles, one per marker
 *            of the set (mode 2).  rho is a HOST array, read before the call returns.
 *   d_out  : ONE row of 10 + n_rho doubles in the layout of scilmm_sets_finish_dev.  flags: bit 0 the degenerate rule, bit 1 a
 *            bisection ran out of steps, bit 2 a root of a tail ran out of steps, bit 3 SKAT-O was computed.
 *   d_lam  : null, or k doubles: the eigenvalues of A = diag(w) K diag(w) in descending order (one per kept marker), then NaN.
 * A is reduced once to a tridiagonal T whose first basis vector is 1 / sqrt(m) (a Householder pre-step, then m - 1 steps of two
 * launches each on the m x m matrix in HBM); the spectra of A, of every A R_rho and of the remainder B are eigenvalues of
 * rescaled T, found by bisection; the tails and the integral follow scilmm_sets_finish_dev's.  The work space (k^2 + 92 k doubles)
 * is the handle's: grown for a wider set behind a stream synchronise, never allocated again for the same or a narrower one.
 * No atomics, fixed reduction orders: the row depends on the set's inputs alone, and scilmm_timing.n_float_atomic_launches is
 * not touched.  Enqueued without synchronising; nothing of the factor is read.  SCILMM_ERR_ARG before anything of the handle or
 * the device is read: a null fac, d_stats, d_gram, d_R, d_u or d_out (rho with n_rho > 0, d_weights in mode 2), k outside
 * 1 .. 4 096, block outside 1 .. 128, (B - 1) bp > 4 096, d_cross null with B > 1 or not null with B = 1, ld_cross < (B - 1) bp,
 * c outside 1 .. 31, q != c + 1, n_rho outside 0 .. 16, a rho outside [0, 1] or NaN, an unknown weight mode or method.  Refusals as
 * for scilmm_sets_finish_dev.  scilmm_amd.VariantSetTest with finish="wide" is the interface.  No counterpart in the reference. */
int scilmm_sets_finish_wide_dev(scilmm_factor* fac, int32_t k, int32_t block, int32_t q, const double* d_stats, const double* d_gram,
                                const double* d_cross, int64_t ld_cross, const double* d_R, const double* d_u, int32_t c,
                                int32_t weight_mode, const double* d_weights, int32_t method, const double* rho, int32_t n_rho,
                                double* d_out, double* d_lam);

/* HIP-event times of the last scilmm_sets_finish_wide_dev on the handle, in milliseconds, valid after the scilmm_sync that
 * follows it: ms[0] prep + form, ms[1] the reduction, ms[2] the eigenvalues, ms[3] the tails (tools/sets_timing.py
 * --wide-finish).  No counterpart in the reference. */
int scilmm_sets_finish_wide_timing(const scilmm_symbolic* sym, double* ms);

/* scilmm_sets_finish_dev with a variance scale per column of the block: in A alone a column's weight is multiplied by its
 * scale, A = diag(w o scale) K diag(w o scale), while t = w o s keeps w; everything else -- arguments, checks, refusals, the
 * layout of a row -- is scilmm_sets_finish_dev's (burden_chi2 = (1't)^2 / 1'A1 is then a chi-square with ONE degree of freedom
 * under the rescaled covariance: burden_p = chi2_1's tail, the caller's).
 *   d_vscale: r doubles on the device, what scilmm_sets_spa*_dev wrote; null is SCILMM_ERR_ARG.
 * flags: bit 4 (16) is set where a kept column's scale is not 1.  With every scale 1.0 the rows are the bits of
 * scilmm_sets_finish_dev (w * 1.0 = w).  scilmm_sets_finish_timing reports either.  scilmm_amd.glmm.BinarySetTest with
 * finish="device" is the interface.  No counterpart in the reference. */
int scilmm_sets_finish_scaled_dev(scilmm_factor* fac, int32_t r, int32_t q, const double* d_stats, const double* d_gram,
                                  const double* d_R, const double* d_u, int32_t c, int32_t n_sets, const int32_t* set_start,
                                  int32_t weight_mode, const double* d_weights, int32_t method, const double* rho, int32_t n_rho,
                                  double* d_out, int64_t ld_out, double* d_lam, const double* d_vscale);

/* Binary traits, variant sets (SAIGE-GENE / SMMAT with the exact K): per set of a Gram block the
 * saddlepoint-implied variance scale of every marker and the saddlepoint p-value of the burden -- the collapsed genotype
 * g_B = sum_j w_j g~_j -- queued BEHIND the block's Gram entry point and the scilmm_scan_spa*_dev of the same markers, on the
 * handle's stream; scilmm_sets_finish_scaled_dev follows it.
 *   the form's marker arguments, r, d_stats, d_R, d_u, d_mu, d_C, c, d_Minv, cutoff: as for the scilmm_scan_spa*_dev twin.
 *   d_gram  : the block's r x r Gram matrix; entry (i, j) is the mean of [i][j] and [j][i], as the finish reads it.
 *   d_spa   : INPUT, the block's 7 x r rows of scilmm_scan_spa*_dev.
 *   n_sets, set_start, weight_mode, d_weights: as for scilmm_sets_finish_dev (set_start is a HOST array, read before the
 *             call returns).
 *   d_bspa  : n_sets rows of 13 doubles:  log_p_B | a_w | s_B | zeta_hi | zeta_lo | iters | flag | a_B | b_B | v~_B | V_Q | phi |
 *             n_adj.  Exactly 13 doubles per set are written.
 *   d_vscale: r doubles; the columns of a set receive rho_j sqrt(phi) (kept markers) or 1.0 (dropped ones); columns outside
 *             every set are not written.
 * With the kept markers, s, K = G - z'z and w as in scilmm_sets_finish_dev, a_j = K_jj and zs_j = s_j / sqrt(a_j):
 *   rho_j   : where the marker's saddlepoint row has flag 1 and log_p_j < 0, v_j >= 0 solves log erfc(v / sqrt 2) = log_p_j (in
 *             logarithms: finite far beyond where p underflows), x_j = v_j^2 and rho_j^2 = zs_j^2 / x_j; rho_j = 1 exactly where
 *             the flag is 0 or 2, log_p_j is NaN or >= 0, x_j is not finite and positive, or a_j is not > 0.
 *   a_B = w'Kw, b_B = w's, V_Q = (w o rho)'K(w o rho): fixed-order sums over the pairs (i, j).
 *   Where a_B > 0 and |b_B| / sqrt(a_B) > cutoff, g_B goes through the steps of scilmm_scan_spa_dev with (a, b) = (a_B, b_B):
 *             log_p_B, a_w, s_B, the roots, iters and flag (0 / 1 / 2) are that call's seven numbers for g_B.  flag 0: the six
 *             numbers before it are NaN.
 *   v~_B = b_B^2 / x_B with x_B from log_p_B as x_j from log_p_j, where flag is 1 and x_B is valid; NaN otherwise.
 *   phi = v~_B / V_Q where v~_B exists, v~_B > V_Q and V_Q > 0, else 1: the burden only ever inflates the covariance.
 *   n_adj   : the kept markers with rho_j != 1.
 * A set with nothing kept: flag 0, n_adj 0, the other eleven numbers NaN.  One workgroup per set, 256 threads, fixed strides and
 * fixed reduction trees, no atomics: a set's numbers depend on its own inputs alone -- not on its place in the block, its
 * neighbours or the mode of the handle -- the three input forms of the same hard calls give the same bits, and
 * scilmm_timing.n_float_atomic_launches is not touched.  g^_B is kept in row `set` of the scratch of scilmm_scan_spa_dev
 * (allocated by the first saddlepoint call of either kind on the handle, never again).  Enqueued without synchronising.
 * SCILMM_ERR_ARG before anything is dereferenced: what scilmm_scan_spa*_dev rejects, a null d_gram, d_bspa, d_vscale or
 * set_start, n_sets outside 1 .. r, offsets that do not start at 0, do not rise strictly or end beyond r, an unknown weight
 * mode, mode 2 without d_weights.  Refusals as for the scan blocks (SCILMM_ERR_STATE, the handle left usable).
 * scilmm_amd.glmm.BinarySetTest is the interface.  No counterpart in the reference. */
int scilmm_sets_spa_dev(scilmm_factor* fac, const int8_t* d_geno, int64_t ld_geno, int32_t r, const double* d_stats, const double* d_gram,
                        const double* d_R, const double* d_u, const double* d_mu, const double* d_C, int32_t c, const double* d_Minv,
                        double cutoff, const double* d_spa, int32_t n_sets, const int32_t* set_start, int32_t weight_mode,
                        const double* d_weights, double* d_bspa, double* d_vscale);
int scilmm_sets_spa_bed_dev(scilmm_factor* fac, const uint8_t* d_bed, int64_t ld_bed, int32_t n_samples, const int32_t* d_sample,
                            int32_t flags, int32_t r, const double* d_stats, const double* d_gram, const double* d_R, const double* d_u,
                            const double* d_mu, const double* d_C, int32_t c, const double* d_Minv, double cutoff, const double* d_spa,
                            int32_t n_sets, const int32_t* set_start, int32_t weight_mode, const double* d_weights, double* d_bspa,
                            double* d_vscale);
int scilmm_sets_spa_dosage_dev(scilmm_factor* fac, const void* d_dos, int32_t dtype, int64_t ld, int32_t n_samples,
                               const int32_t* d_sample, int32_t r, const double* d_stats, const double* d_gram, const double* d_R,
                               const double* d_u, const double* d_mu, const double* d_C, int32_t c, const double* d_Minv, double cutoff,
                               const double* d_spa, int32_t n_sets, const int32_t* set_start, int32_t weight_mode,
                               const double* d_weights, double* d_bspa, double* d_vscale);

/* HIP-event time of the last scilmm_sets_spa*_dev on the handle, in milliseconds, valid after the scilmm_sync that follows it:
 * ms[0] k_sets_spa (tools/sets_timing.py --binary).  No counterpart in the reference. */
int scilmm_sets_spa_timing(const scilmm_symbolic* sym, double* ms);

/* Binary traits, ONE variant set of k markers, 1 <= k <= 4 096, that runs as B = ceil(k / block) sub-blocks (DESIGN.md section
 * 23): what scilmm_sets_spa*_dev does for the sets of one block, cut where a sub-block ends.  Three pieces:
 *
 * (a) scilmm_sets_collapse*_dev, queued BEHIND the Gram entry point of a sub-block, on the handle's stream: the collapsed
 * genotype g_B = sum_j w_j g~_j of the set grows by the sub-block's kept markers.
 *   the form's marker arguments and r: as for the scilmm_scan_spa*_dev twin (the sub-block's rows).
 *   d_stats    : the sub-block's (q + 4) x r statistics; rows 0 .. 2 (n_obs, mean, css) are read.
 *   weight_mode, d_weights: as for scilmm_sets_finish_dev; d_weights holds the sub-block's r entries (mode 2).
 *   first      : 1 for the set's first sub-block (the row starts from 0), 0 otherwise (it starts from what d_gB holds).
 *   d_gB       : n doubles, the caller's, in the ORIGINAL order of the individuals.
 * For every individual i: acc = first ? 0 : d_gB[i]; for the sub-block's kept markers j (an observed value and variation, as
 * scilmm_sets_finish_dev keeps them) in ascending column order acc = fma(w_j, g~_ji, acc), g~ the centred, mean-imputed value the
 * saddlepoint kernels read; d_gB[i] = acc.  An individual's value is ONE fma chain over the set's kept markers in the order
 * given: the row carries the same bits however the set is cut into sub-blocks, and from int8, .bed and hard-call dosage rows
 * alike.  A sub-block with nothing kept leaves the row as it is (zero if first).  A thread per individual on a capped grid with a
 * fixed stride, the reads of a marker row along the lanes; no atomics, nothing allocated, nothing of the work buffers or of the
 * saddlepoint scratch written: scilmm_scan_panel_dev and scilmm_scan_block_keep_dev may still follow the block.
 * SCILMM_ERR_ARG before anything is dereferenced: what the form's scilmm_scan_spa*_dev rejects of its marker arguments and r, a
 * null fac, d_stats or d_gB, first outside 0 / 1, an unknown weight mode, mode 2 without d_weights.  Refusals as for the scan
 * blocks.
 *
 * (b) scilmm_sets_spa_wide_dev, queued behind the last sub-block (its Gram entry point, saddlepoint call, collapse and panel):
 * the set's variance scales and the saddlepoint p-value of its burden.  It reads no genotypes.
 *   k, block, q, d_stats, d_gram, d_cross, ld_cross: the slices of scilmm_sets_finish_wide_dev.
 *   d_R, d_u, d_mu, d_C, c, d_Minv, cutoff: as for scilmm_sets_spa_dev.
 *   d_spa      : B slices at a stride of 7 block doubles; slice b is the 7 x r_b rows scilmm_scan_spa*_dev wrote for sub-block b.
 *   weight_mode, d_weights: as above; d_weights holds k entries, one per marker of the set.
 *   d_gB       : n doubles: in, the collapsed row; where the burden is attempted it is overwritten with g^_B, as
 *                scilmm_sets_spa_dev overwrites its scratch row.
 *   d_bspa     : ONE row of 13 doubles in the layout of scilmm_sets_spa_dev.
 *   d_vscale   : k doubles: rho_j sqrt(phi) for a kept marker, 1.0 for a dropped one.
 * Every number is defined as for scilmm_sets_spa_dev.  The pair sums a_B and V_Q are taken row by row (each row in ascending
 * column order, folded by a fixed tree, two partials per row in HBM) and the rows folded in a fixed order: they agree with
 * scilmm_sets_spa_dev's to rounding, not bit for bit.  A set with nothing kept: flag 0, n_adj 0, the other eleven numbers NaN,
 * every scale 1.0.  No atomics; scilmm_timing.n_float_atomic_launches is not touched.  The work space is the wide finish's, by
 * its growth rule: grown for a wider set behind a stream synchronise, and the finish that follows for the same k allocates
 * nothing.  SCILMM_ERR_ARG before anything is dereferenced: a null fac, d_stats, d_gram, d_R, d_u, d_mu, d_C, d_Minv, d_spa, d_gB,
 * d_bspa or d_vscale, what scilmm_sets_finish_wide_dev rejects of k, block, d_cross and ld_cross, c outside 1 .. 31, q != c + 1, a
 * negative or NaN cutoff, an unknown weight mode, mode 2 without d_weights.  Refusals as for the scan blocks.
 *
 * (c) scilmm_sets_finish_wide_scaled_dev: scilmm_sets_finish_wide_dev with a variance scale per marker of the set, in A alone:
 * A = diag(w o scale) K diag(w o scale), while t = w o s keeps w.
 *   d_vscale   : k doubles on the device, what scilmm_sets_spa_wide_dev wrote; null is SCILMM_ERR_ARG.
 * flags: bit 4 (16) is set where a kept marker's scale is not 1.  With every scale 1.0 the row is the bits of
 * scilmm_sets_finish_wide_dev (w * 1.0 = w), which passes none.  scilmm_sets_finish_wide_timing reports either.
 *
 * scilmm_amd.glmm.BinaryWideSetTest (NullModel.sets(max_markers=...)) is the interface.  No counterpart in the reference. */
int scilmm_sets_collapse_dev(scilmm_factor* fac, const int8_t* d_geno, int64_t ld_geno, int32_t r, const double* d_stats,
                             int32_t weight_mode, const double* d_weights, int32_t first, double* d_gB);
int scilmm_sets_collapse_bed_dev(scilmm_factor* fac, const uint8_t* d_bed, int64_t ld_bed, int32_t n_samples, const int32_t* d_sample,
                                 int32_t flags, int32_t r, const double* d_stats, int32_t weight_mode, const double* d_weights,
                                 int32_t first, double* d_gB);
int scilmm_sets_collapse_dosage_dev(scilmm_factor* fac, const void* d_dos, int32_t dtype, int64_t ld, int32_t n_samples,
                                    const int32_t* d_sample, int32_t r, const double* d_stats, int32_t weight_mode,
                                    const double* d_weights, int32_t first, double* d_gB);
int scilmm_sets_spa_wide_dev(scilmm_factor* fac, int32_t k, int32_t block, int32_t q, const double* d_stats, const double* d_gram,
                             const double* d_cross, int64_t ld_cross, const double* d_R, const double* d_u, const double* d_mu,
                             const double* d_C, int32_t c, const double* d_Minv, double cutoff, const double* d_spa, int32_t weight_mode,
                             const double* d_weights, double* d_gB, double* d_bspa, double* d_vscale);
int scilmm_sets_finish_wide_scaled_dev(scilmm_factor* fac, int32_t k, int32_t block, int32_t q, const double* d_stats, const double* d_gram,
                                       const double* d_cross, int64_t ld_cross, const double* d_R, const double* d_u, int32_t c,
                                       int32_t weight_mode, const double* d_weights, int32_t method, const double* rho, int32_t n_rho,
                                       double* d_out, double* d_lam, const double* d_vscale);

/* HIP-event times on the handle, in milliseconds, valid after the scilmm_sync that follows the call: ms[0] k_sets_collapse of the
 * last scilmm_sets_collapse*_dev; of the last scilmm_sets_spa_wide_dev ms[1] markers + pairs and ms[2] the burden kernel
 * (tools/sets_timing.py --binary-wide).  No counterpart in the reference. */
int scilmm_sets_spa_wide_timing(const scilmm_symbolic* sym, double* ms);

/* One block of BLUP predictions on the device: with the scan's w(b) = L^-1 P b and Q = [w(C) | w(y)], the right-hand-side
 * block is r columns g of a relationship matrix instead of r markers, and what comes back gives g' P_V g and g' P_V y
 * (P_V = V^-1 - V^-1 C (C' V^-1 C)^-1 C' V^-1) per column by the scan's algebra: predicted value, prediction error variance
 * and reliability of an individual for one forward-sweep column, with no matrix on the host.
 * scilmm_rel_block_dev takes the columns from the RESIDENT values: column c = (sum_k weights[k] A_k)[:, ids[c]].
 *   weights: HOST, one per matrix of the analysis (a zero weight leaves the matrix unread).
 *   ids    : HOST, r individuals in the ORIGINAL order (the row order of the matrices), distinct, each in 0 .. n-1.
 * scilmm_rows_block_dev takes them from the caller: column c = row c of an r-row CSR matrix, all DEVICE pointers,
 *   d_indptr int64[r + 1], d_indices int32 in the ORIGINAL order of the individuals, d_data double.  An index outside
 *   0 .. n-1 is skipped, never stored; the indices of a row must be distinct, and d_indptr must be ascending inside the
 *   two arrays (it is not read on the host).
 *   r      : columns in the block, 1 .. 128.
 *   d_Q    : as for scilmm_scan_block_dev, 1 <= q <= 32.
 *   d_stats: (q + 2) x r row-major: the column's own diagonal entry G[i, i] (0 from the rows form) | |w(g)|^2 | the q rows
 *            of Q^T w(g).
 * The block is cleared and then only stored into (every entry has one writer, no atomics in either mode of the handle);
 * the forward sweep and the statistics are those of scilmm_scan_block_dev, so scilmm_scan_timing reports block building |
 * forward sweep | statistics for these blocks too.  Everything is enqueued on the handle's stream without synchronising.
 * Null pointers, r or q out of range, an id outside 0 .. n-1 or repeated: SCILMM_ERR_ARG before anything is dereferenced;
 * refusals as for the half-solves.  No counterpart in the reference (it stops at the variance components and the
 * covariates' coefficients). */
int scilmm_rel_block_dev(scilmm_factor* fac, const double* weights, const int32_t* ids, int32_t r, const double* d_Q, int32_t q,
                         double* d_stats);
int scilmm_rows_block_dev(scilmm_factor* fac, const int64_t* d_indptr, const int32_t* d_indices, const double* d_data, int32_t r,
                          const double* d_Q, int32_t q, double* d_stats);

/* SURVEY section 8f rank 4 -- the exact tr(V^-1 A_k) of the gradient instead of the reference's Monte-Carlo estimate
 * (scilmm/SparseCholesky.py:49-52, :65).  scilmm_selected_inverse replaces, IN PLACE, every stored entry of the factor by
 * the entry of Z = (V[P][:,P])^-1 at the same position (Takahashi recursion over the supernodes from the last level
 * down: Z_RC = -Z_RR (L21 L11^-1), Z_CC = L11^-T L11^-1 - (L21 L11^-1)^T Z_RC; twice the factorization's flops, no
 * second copy of the factor).  The handle is consumed: refactorize before the next solve.  scilmm_inverse_traces then
 * returns out[k] = tr(V^-1 A_k) = sum over A_k's pattern of Z_ij A_k,ij for every matrix k (one streaming pass each);
 * scilmm_export_L on an inverted handle returns the entries of Z on L's pattern.  No counterpart in the reference. */
/* Single-GPU handles only: on a distributed factor both return SCILMM_ERR_STATE with an explanatory message before touching
 * anything -- the factor stays valid and usable (the Takahashi recursion reads, for every front, the inverse entries of ALL
 * later fronts: with rank-local storage that is a second fan-out in the opposite direction, not built).  The default
 * Monte-Carlo trace of the reference needs neither. */
int scilmm_selected_inverse(scilmm_factor* fac);
int scilmm_inverse_traces(scilmm_factor* fac, double* out);

/* Entries of the inverse on V's OWN pattern, read off an inverted handle: with Z = V^-1 the call writes the entries of
 *     M = alpha * diag(s) Z diag(s) + beta * T T'
 * that lie on the pattern of V (a subset of L's pattern: the value-assembly maps give their positions in the panels).
 *   d_diag : n doubles, d_diag[i] = M_ii, i in the ORIGINAL order of the matrices' rows.
 *   d_off  : nnz_pattern doubles, d_off[e] = M_ij for pattern slot e in the slot order of scilmm_symbolic_get "pat_colptr" /
 *            "pat_row" (the order of the resident values; the diagonal slot comes first in each column), i and j the slot's
 *            two individuals.  A diagonal slot holds the bits of d_diag.
 *   d_s    : n doubles in the original order, NULL = all ones.
 *   d_T    : n x c row-major in the original order, 0 <= c <= 32; NULL or c = 0: no low-rank term.  Rows are read 16 bytes
 *            at a time when c is even and d_T 16-byte aligned, else 8; the bits are the same.
 * Either output may be NULL to skip it.  Everything is a device pointer; two streaming kernels (one over the n diagonals,
 * one over the slots) are enqueued on the handle's stream without synchronising.  One thread owns one output element and
 * stores it once: no floating-point atomics, no scratch reductions, the dot product over c in ascending order, so the bits
 * depend on the inputs alone in either mode of the handle and scilmm_timing.n_float_atomic_launches is not touched.  The
 * handle stays inverted and no work buffer is written: the call may be repeated with other s, T, alpha, beta.
 * SCILMM_ERR_ARG before anything is dereferenced: a null fac, c outside 0 .. 32, both outputs NULL.  SCILMM_ERR_STATE with a
 * message: a handle that scilmm_selected_inverse has not inverted (so never a distributed one).  With alpha = -1, s = the
 * diagonal residual variances and T = C R^-1 - E H this is the prediction error (co)variance of every total genetic value
 * up to the diagonal's + e_i (scilmm_amd.BLUP.reliability_all, .prediction_error_covariance,
 * .leave_one_out are the interfaces).  No counterpart in the reference. */
int scilmm_inverse_pattern_dev(scilmm_factor* fac, double alpha, const double* d_s, double beta, const double* d_T, int32_t c,
                               double* d_diag, double* d_off);

/* BASELINE configs[4] ("fp64 factor with fp32 MFMA fronts"): bits = 32 runs the products of the dense-tail update on
 * the fp32 matrix pipe: the finished tail panels get an fp32 shadow (one rounding per entry; + 50 % tail storage -- of a rank's own
 * panels and ring slots when the tail is distributed --, dropped when the device has no room for it: the operands are then
 * rounded while they are staged), products are
 * summed in fp32 over 256 (staged form: 16) of them and those sums in fp64;
 * everything else -- the subtraction from the panel, potrf, trsm, the solves -- stays fp64.  The factor then has a
 * relative backward error of ~1e-7: callers refine their solves against the exact V (scilmm_spmm), as
 * scilmm_amd.factor.Factor does.  bits = 64 (default) restores the all-fp64 path.  No counterpart in the reference. */
int scilmm_set_front_precision(scilmm_symbolic* sym, int32_t bits);

/* Deterministic mode: every floating-point sum of an evaluation on this handle is taken in an order that depends on the
 * analysis only, so the same inputs give the same BITS -- in one process, in two processes, under a profiler.  on != 0 selects
 *   - the factorization's fixed-order schedule (the prelude's contributions to the dense tail stay on the target-coordinate
 *     path instead of k_outside's fp64 atomics),
 *   - the forward sweep and L*R (scilmm_solve / scilmm_lmul) in PULL form: the owner of a front's rows sums the contributions
 *     of its update pairs in list order (k_fwd_pull; long lists in fixed segments folded in slot order) instead of k_fwd's
 *     atomic pushes,
 *   - Y = A_k X (scilmm_spmm / _dev, and with it the refinement of solves on fp32 fronts) with row ownership through a
 *     transposed index of the pattern (k_spmm_row; 12 bytes per strictly lower pattern entry of device memory, allocated
 *     only in this mode: scilmm_symbolic_get "pat_rowptr" / "pat_rowslot" / "pat_rowcol" give the counts),
 *   - the selected inverse (scilmm_selected_inverse, and with it scilmm_inverse_traces) in store-and-sum form: the items of
 *     the dense-tail kernel store their accumulator tiles into slots that a second kernel adds in K-range order
 *     (k_sinv_tail<true> + k_sinv_tail_fold), the diagonal blocks are summed over fixed segments of consecutive row tiles
 *     (k_sinv_cc_ordered + k_sinv_cc_fold); every entry of Z is written with plain stores.  The slots are allocated with
 *     the handle's first inversion: at most about 2048 + (rows / 256) tiles of 256 x 128 doubles (0.54 GB) for the tail,
 *     one 128 x 128 tile per two row tiles of the largest level for the diagonal blocks (SCILMM_VERBOSE prints both).
 * The backward sweep, the chain sweeps, quadratic forms, the log-determinant and the Haseman-Elston moments are order-fixed in
 * either mode.  NOT covered: distributed handles -- the summation order of an all-reduce belongs to the communication library, so on a handle with
 * scilmm_dist_init(world > 1) the mode is refused with SCILMM_ERR_STATE (in either call order: scilmm_dist_init refuses a
 * deterministic handle as well).  Results in this mode differ from the default mode's in the last bits; the default
 * schedule is unchanged.  The initial value of a handle is SCILMM_DETERMINISTIC=1 in the environment at creation.  Must be
 * called before the first numeric call on the handle (the device plan depends on it); afterwards SCILMM_ERR_STATE.
 * scilmm_timing.n_float_atomic_launches lets a caller check the claim.  No counterpart in the reference (CHOLMOD on one
 * host thread is deterministic as it is). */
int scilmm_set_deterministic(scilmm_symbolic* sym, int32_t on);
int scilmm_get_deterministic(const scilmm_symbolic* sym, int32_t* on);

/* Haseman-Elston moments on the device (reference HE, SparseCholesky.py:192-246, REML's starting
 * point at :121): *frob = sum_ij (A_k1 o A_k2)_ij over the full symmetric matrices, *diag_dot = diag(A_k1) . diag(A_k2),
 * from the value arrays already resident in HBM (one streaming pass).  y'A_k y comes from scilmm_quadforms. */
int scilmm_he_moments(scilmm_symbolic* sym, int32_t k1, int32_t k2, double* frob, double* diag_dot);

/* Dominance relationship matrix on the pattern of the IBD matrix, built on the device (replaces
 * reference scilmm/Matrices/Dominance.py:12-43 `dominance(rel, ibd)`):
 *   out[t] = 1/4 (A[f_i,f_j] A[m_i,m_j] + A[f_i,m_j] A[m_i,f_j])  for the stored entry t = (i, j), i != j;  1 on the diagonal.
 * A: CSR with both halves stored, rows strictly ascending (canonical), explicit zeros removed (the reference calls
 * eliminate_zeros first); parents: n x 2 int32, -1 = unknown (contributes 0).  out has A's layout (same indptr /
 * indices).  Values equal the reference's NumPy arithmetic bit for bit (no fma contraction).
 * scilmm_dominance takes host buffers (upload, one kernel, download); scilmm_dominance_dev device buffers and a HIP
 * stream (0 = default) and only enqueues.  scilmm_dominance_error(): text of the calling thread's last failure. */
int scilmm_dominance(int32_t n, const int64_t* indptr, const int32_t* indices, const double* data, const int32_t* parents,
                     double* out);
int scilmm_dominance_dev(int32_t n, const int64_t* d_indptr, const int32_t* d_indices, const double* d_data,
                         const int32_t* d_parents, double* d_out, void* stream);
const char* scilmm_dominance_error(void);

/* Y = A X for a CSR matrix (both halves stored; any square sparse matrix) and a row-major n x r block, all DEVICE pointers,
 * enqueued on `stream` (0 = default): needs NO symbolic analysis.  The n x 100 products of the Haseman-Elston standard error
 * (reference SparseCholesky.py:259-278 `mat_j.dot(sim_y)`, `H.dot(t)`: four per matrix pair on the host) -- HE is what the
 * reference's authors run above 250k individuals (README.md:63) and it never factorizes.  X and Y must not alias.
 * scilmm_csr_spmm_error(): text of the calling thread's last failure. */
int scilmm_csr_spmm_dev(int32_t n, const int64_t* d_indptr, const int32_t* d_indices, const double* d_data, const double* d_X,
                        int32_t r, double* d_Y, void* stream);
const char* scilmm_csr_spmm_error(void);

/* --- device-pointer variants used by bench.py and by callers that keep data resident in HBM */
int scilmm_solve_dev(scilmm_factor* fac, const double* dB, int32_t r, double* dX);
int scilmm_lmul_dev(scilmm_factor* fac, const double* dR, int32_t r, double* dZ);
int scilmm_solve_L_dev(scilmm_factor* fac, const double* dB, int32_t r, double* dX);
int scilmm_solve_Lt_dev(scilmm_factor* fac, const double* dB, int32_t r, double* dX);
int scilmm_quadforms_dev(scilmm_symbolic* sym, int32_t k, const double* dU, int32_t r, double* d_out);
int scilmm_sync(scilmm_symbolic* sym);

/* --- measurement hooks (bench.py): HIP-event time of the last factorize / solve on the handle's
 * stream, in milliseconds, split by phase. */
typedef struct scilmm_timing {
  double assemble_ms, factor_ms, solve_fwd_ms, solve_bwd_ms, lmul_ms, quad_ms;
  int64_t n_launches;
  /* filled when profiling is on: HIP-event time summed per kernel class over the last factorize */
  double update_ms, potrf_ms, trsm_ms;
  int64_t n_update_launches;
  double reduce_cells_ms;
  /* wall time during which at least one update launch was running (early launches of consecutive levels
   * overlap on the two side streams, so update_ms -- the SUM of launch durations -- counts that time twice) */
  double update_union_ms;
  /* the dense-tail kernel alone (k_dense_b / k_dense_h / k_dense32): summed launch durations and launch count of the last factorize */
  double dense_ms;
  int64_t n_dense_launches;
  /* multi-GPU: own tail targets of the last factorize whose late update was issued in two parts -- the sources that had
   * already arrived first, the newest source panel's items after the wait for its broadcast (look-ahead on the chain's
   * critical path); 0 on one GPU */
  int64_t n_late_split;
  /* kernel launches on this handle SINCE IT WAS CREATED whose results are summed with floating-point atomics (k_outside,
   * the atomic forms of k_fwd, k_spmm_w, k_sinv_tail / k_sinv_cc): 0 in deterministic mode */
  int64_t n_float_atomic_launches;
} scilmm_timing;
int scilmm_last_timing(const scilmm_symbolic* sym, scilmm_timing* out);
/* Bracket every kernel class of the factorization with HIP events on the handle's stream (bench.py's
 * live roofline figure).  Off by default.  on = 2 additionally queues every look-ahead ("early") update launch on ONE
 * side stream instead of alternating between two, so that the durations of consecutive launches of the dominant kernel
 * do not overlap each other (the clean per-launch figure; slower as a whole -- a measurement mode, same results). */
int scilmm_set_profiling(scilmm_symbolic* sym, int32_t on);

/* --- SURVEY section 8(f) rank 1 ("next"): pedigree -> IBD matrix, the producer of the hot path's input.
 * Replaces Numerator.LD + create_numerator (scilmm/Matrices/Numerator.py:5-38) and, with count_only != 0,
 * Relationship.count_IBD_nonzero (scilmm/Matrices/Relationship.py:38-61).  parents: n x 2 int32, -1 = unknown,
 * individuals in topological order (parents first).  Host C++/OpenMP; no device needed. */
typedef struct scilmm_ibd scilmm_ibd;
/* count_only: 0 = pattern + values, 1 = the number of structural nonzeros only, 2 = the PATTERN only (no values: what the
 * symbolic analysis needs when the values are then computed on the device, scilmm_ibd_values_device) */
int scilmm_ibd_build(int32_t n, const int32_t* parents, int32_t count_only, scilmm_ibd** out, int64_t* nnz);
int scilmm_ibd_sizes(const scilmm_ibd* h, int64_t* nnz_A, int64_t* nnz_L);
/* A: symmetric CSR (both triangles, sorted); L: ancestor-weight rows; D, F: length n.  NULL pointers are skipped. */
int scilmm_ibd_export(const scilmm_ibd* h, int64_t* a_indptr, int32_t* a_indices, double* a_data, int64_t* l_indptr,
                      int32_t* l_indices, double* l_data, double* D, double* F);
void scilmm_ibd_free(scilmm_ibd* h);
/* The VALUES of the IBD matrix computed on the device, straight into the HBM-resident value slots of matrix k of `sym` --
 * they never exist on the host and never cross PCIe (replaces create_numerator's L D L^T, Numerator.py:37-38, and the
 * 8 bytes per entry of scilmm_values_upload: 7.3 GB at the 1M config).  Tabular recursion on the analysed pattern,
 * A[i,j] = 1/2 (A[f_i,j] + A[m_i,j]) for i > j, A[i,i] = 1 + 1/2 A[f_i,m_i], one launch per generation sum (every entry
 * depends on entries with a smaller gen(a) + gen(b) only).  parents: n x 2, -1 = unknown, individuals in pedigree order
 * (the row order of the matrices given to scilmm_symbolic_create); the analysed pattern must contain every pair with a
 * common ancestor (scilmm_ibd_build's pattern does).  Exact: the values are dyadic rationals. */
int scilmm_ibd_values_device(scilmm_symbolic* sym, int32_t k, int32_t n, const int32_t* parents);
/* The VALUES of the dominance relationship matrix computed on the device from the IBD values of matrix k_src already
 * resident in HBM, straight into the value slots of matrix k_dst (replaces reference scilmm/Matrices/Dominance.py:12-43
 * `dominance(rel, ibd)` and the upload of its result; scilmm_dominance / scilmm_dominance_dev are the CSR-layout forms):
 *   D[a,b] = 1/4 (A[f_a,f_b] A[m_a,m_b] + A[f_a,m_b] A[m_a,f_b]) for a != b, 1 on the diagonal, on every slot of the
 * analysed pattern (matrix k_dst is given to scilmm_symbolic_create with matrix k_src's pattern, as the reference builds
 * it).  Bit-identical to the reference's NumPy arithmetic.  With scilmm_ibd_values_device, BASELINE configs[4]'s two
 * variance components are built where they are used: only the pattern and the parent table reach a rank. */
int scilmm_dominance_values_device(scilmm_symbolic* sym, int32_t k_dst, int32_t k_src, int32_t n, const int32_t* parents);
/* Matrix k's device-resident values in PATTERN-SLOT order (scilmm_symbolic_get "pat_colptr" / "pat_row": permuted CSC of
 * the lower triangle, diagonal first; n values for a diagonal-only matrix) -- for tests and diagnostics. */
int scilmm_values_download(scilmm_symbolic* sym, int32_t k, double* slots_out);

/* --- the on-disk format in front of the path.  Replaces scipy.io.mmread(path).tocsr()
 * (scilmm/SparseCholesky.py:399) by a memory-mapped, all-cores parse of the MatrixMarket coordinate file (real /
 * integer / pattern; general / symmetric / skew-symmetric; duplicates summed, symmetric storage expanded): CSR with
 * sorted indices.  Host C++/OpenMP; no device needed. */
typedef struct scilmm_mm scilmm_mm;
int scilmm_mm_read(const char* path, scilmm_mm** out, int32_t* nrows, int32_t* ncols, int64_t* nnz);
int scilmm_mm_export(const scilmm_mm* m, int64_t* indptr, int32_t* indices, double* data);
const char* scilmm_mm_error(const scilmm_mm* m);
void scilmm_mm_free(scilmm_mm* m);

const char* scilmm_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SCILMM_HIP_H */
