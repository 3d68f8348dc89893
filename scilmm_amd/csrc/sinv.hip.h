// The selected inverse (included by engine.hip only, behind values.hip.h): the Takahashi recursion over the levels from
// the top down, in place on the factor's panels (the launchers sinv_y / sinv_tail / sinv_w / sinv_cc of launch.hip.h; on a
// deterministic handle the ordered branch of sinv_tail, and sinv_cc_ordered), and tr(V^-1 A_k) for every matrix from one
// pass over its pattern.
#pragma once

namespace {

int selected_inverse(scilmm_factor* fac) {
  scilmm_symbolic* sym = fac->sym;
  TRY(settle(fac, "scilmm_selected_inverse"));
  Dev* D = (Dev*)sym->device;
  const Symbolic& S = *sym->S;
  if (D->world > 1) {
    sym->err = "scilmm_selected_inverse: not available on a distributed factor";
    return SCILMM_ERR_STATE;
  }
  hipStream_t st = D->stream;
  const bool new_sinv_plan = !D->d_col_front;
  TRY(ensure_sinv_plan(sym, D));
  if (new_sinv_plan) {  // (the attribute belongs to an instance)
    HIPCHK(hipFuncSetAttribute((const void*)k_sinv_tail<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
    HIPCHK(hipFuncSetAttribute((const void*)k_sinv_tail<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
  }
  HIPCHK(hipEventRecord(D->ev[6], st));
  // SCILMM_SINV_GENERIC=1: the gather kernel for the dense tail as well (the round's first form)
  const Tuning tune = read_tuning();
  const bool tail_kernel = D->use_mfma && !tune.sinv_generic;
  // deterministic mode: every entry of Z from a sum whose order the plan fixes (k_sinv_tail<true> / k_sinv_cc_ordered and
  // their folds; plain stores).  SCILMM_SINV_REVERSE=1 turns the dispatch order of the two round: the bits must not move.
  const bool reverse = D->det && tune.sinv_reverse;
  for (int32_t l = S.nlevels - 1; l >= 0; --l) {
    const int64_t t0 = D->lv_tile_ptr[l], nt = D->lv_tile_ptr[l + 1] - t0;
    const int32_t f0 = D->lv_ptr[l], f1 = D->lv_ptr[l + 1];
    if (f1 == f0) continue;
    const int32_t* tiles = D->d_level_tiles + t0;
    const int32_t tf = tail_kernel ? D->sinv_tail_front[(size_t)l] : -1;
    const int32_t ydf = tail_kernel ? S.dense_first : S.nsuper;  // fronts from here on keep Y transposed
    sinv_y(D, fac, st, tiles, nt, ydf);
    hipLaunchKernelGGL(k_sinv_cc0, dim3((unsigned)(f1 - f0)), dim3(256), 0, st, D->v, D->d_level_fronts + f0, fac->L,
                       (const double*)fac->invD);
    if (tf >= 0) {
      sinv_tail(D, fac, st, tf - S.dense_first, reverse);
      // the gather kernel takes the non-tail fronts' tiles only
      sinv_w(D, fac, st, D->d_sinv_pre_tiles + D->sinv_pre_ptr[(size_t)l], D->sinv_pre_ptr[(size_t)l + 1] - D->sinv_pre_ptr[(size_t)l]);
    } else {
      sinv_w(D, fac, st, tiles, nt);  // ... or all of the level's
    }
    if (D->det) sinv_cc_ordered(D, fac, st, l, ydf, reverse);
    else sinv_cc(D, fac, st, tiles, nt, ydf);
  }
  HIPCHK(hipEventRecord(D->ev[7], st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, D->ev[6], D->ev[7]));
  D->timing.quad_ms = ms;  // (reported through the quad_ms slot: the selected inverse replaces the trace estimator's sweeps)
  fac->valid = false;
  fac->inverted = true;
  return SCILMM_OK;
}

int inverse_traces(scilmm_factor* fac, double* out) {
  scilmm_symbolic* sym = fac->sym;
  Dev* D = (Dev*)sym->device;
  const Symbolic& S = *sym->S;
  constexpr int NBLK = 1024;
  D->clear_block();  // (the factor a block in X was swept with is gone)
  TRY(ensure_io(sym, D, 2 * NBLK));
  hipStream_t s0 = D->stream;
  double* part = D->IO;
  for (int32_t k = 0; k < S.K; ++k) {
    if (!D->have_vals[k]) return SCILMM_ERR_STATE;
    HIPCHK(hipMemsetAsync(part, 0, sizeof(double) * 2 * NBLK, s0));
    const bool dg = S.is_diag[k];
    if (!dg && S.nnz_pattern > 0)
      hipLaunchKernelGGL(k_sinv_trace, dim3(NBLK), dim3(256), 0, s0, S.nnz_pattern, D->v.asm_dst, (const double*)D->vals[k],
                         (const double*)fac->L, part);
    if (S.n > 0)
      hipLaunchKernelGGL(k_sinv_trace_diag, dim3(NBLK), dim3(256), 0, s0, S.n, D->v.pat_colptr, D->v.diag_dst, (const double*)D->vals[k],
                         dg ? 1 : 0, (const double*)fac->L, part + NBLK);
    long double sum[2];  // all slots | diagonal
    TRY(fold_blocks(sym, D, part, 2, NBLK, sum));
    out[k] = dg ? (double)sum[1] : (double)(2.0L * sum[0] - sum[1]);  // every off-diagonal pair counts twice (V^-1 and A_k are symmetric)
  }
  HIPCHK(hipGetLastError());
  return SCILMM_OK;
}

// M = alpha diag(s) Z diag(s) + beta T T' on V's pattern from the inverted panels: two streaming kernels on the handle's stream,
// nothing waited for, no work buffer touched (the panels, the plan's maps and the caller's arrays are all they read).
int inverse_pattern(scilmm_factor* fac, double alpha, const double* d_s, double beta, const double* d_T, int32_t c, double* d_diag,
                    double* d_off) {
  scilmm_symbolic* sym = fac->sym;
  Dev* D = (Dev*)sym->device;
  const Symbolic& S = *sym->S;
  hipStream_t st = D->stream;
  if (!d_T) c = 0;
  const double* Z = (const double*)fac->L;
  const bool vec = c > 0 && c % 2 == 0 && ((uintptr_t)d_T & 15) == 0;  // rows of T as double2
  if (d_diag && S.n > 0) {
    const dim3 grid((unsigned)((S.n + 255) / 256));
    if (vec) hipLaunchKernelGGL(k_invpat_diag<true>, grid, dim3(256), 0, st, S.n, D->v.perm, D->v.diag_dst, Z, alpha, d_s, beta, d_T, c, d_diag);
    else hipLaunchKernelGGL(k_invpat_diag<false>, grid, dim3(256), 0, st, S.n, D->v.perm, D->v.diag_dst, Z, alpha, d_s, beta, d_T, c, d_diag);
  }
  if (d_off && S.nnz_pattern > 0) {
    const dim3 grid((unsigned)((S.nnz_pattern + 255) / 256));
    if (vec) hipLaunchKernelGGL(k_invpat_slots<true>, grid, dim3(256), 0, st, D->v, S.nnz_pattern, Z, alpha, d_s, beta, d_T, c, d_off);
    else hipLaunchKernelGGL(k_invpat_slots<false>, grid, dim3(256), 0, st, D->v, S.nnz_pattern, Z, alpha, d_s, beta, d_T, c, d_off);
  }
  HIPCHK(hipGetLastError());
  return SCILMM_OK;
}

}  // namespace
