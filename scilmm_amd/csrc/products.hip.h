// Products with the resident A_k values (included by engine.hip only, behind sweep.hip.h): quadratic forms, SpMM and the
// Hutchinson / HE moments.  run_quad and run_spmm are the device-pointer bodies; quad_host and spmm_host stage a host block
// through Dev::IO around them.  fold_blocks is the host end of every sum that is written as block partials.
#pragma once

namespace {

// Downloads `rows` rows of `nblk` block partial sums and adds each row up in block order, in long double: the same bits
// on every call.
int fold_blocks(scilmm_symbolic* sym, Dev* D, const double* d_part, int rows, size_t nblk, long double* sums) {
  std::vector<double> h((size_t)rows * nblk);
  HIPCHK(hipMemcpyAsync(h.data(), d_part, sizeof(double) * h.size(), hipMemcpyDeviceToHost, D->stream));
  HIPCHK(hipStreamSynchronize(D->stream));
  for (int q = 0; q < rows; ++q) {
    long double s = 0.0L;
    for (size_t b = 0; b < nblk; ++b) s += h[(size_t)q * nblk + b];
    sums[q] = s;
  }
  return SCILMM_OK;
}

// matrix k is one of the handle's and its values are resident (what the products, the traces and the download ask first)
inline bool resident(const scilmm_symbolic* sym, const Dev* D, int32_t k) { return k >= 0 && k < sym->S->K && D->have_vals[k]; }

// out[c] = u_c^T A_k u_c for the r columns of dU (device, row-major n x r); asynchronous, timed by events 6 and 7
int run_quad(scilmm_symbolic* sym, Dev* D, int32_t k, const double* dU, int32_t r, double* d_out) {
  const Symbolic& S = *sym->S;
  if (!resident(sym, D, k)) {
    sym->err = "quadforms: matrix index invalid or values not uploaded";
    return SCILMM_ERR_STATE;
  }
  TRY(ensure_work(sym, D));
  hipStream_t st = D->stream;
  const int64_t SPW = 512;
  const int64_t nw_gen = ((S.nnz_pattern + SPW - 1) / SPW + 3) / 4 * 4;
  const int64_t nw_dia = 1024;
  const int64_t nw = std::max(nw_gen, nw_dia);
  TRY(grow(sym, &D->partial, &D->partial_cap, (size_t)nw * RPMAX));
  HIPCHK(hipEventRecord(D->ev[6], st));
  for (int32_t cbeg = 0; cbeg < r; cbeg += RPMAX) {
    const int rc = std::min<int>(RPMAX, r - cbeg);
    const int rp = rp_of(rc);
    const int64_t tot = (int64_t)S.n * rp;
    hipLaunchKernelGGL(k_perm_in, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, S.n, r, rp, cbeg, D->v.perm, dU, D->W);
    int64_t nwaves;
    if (S.is_diag[k]) {
      nwaves = nw_dia;
      hipLaunchKernelGGL(k_quad_diag, dim3((unsigned)(nwaves / 4)), dim3(256), 0, st, S.n, (const double*)D->vals[k],
                         (const double*)D->W, rp, D->partial);
    } else {
      nwaves = nw_gen;
      hipLaunchKernelGGL(k_quad, dim3((unsigned)(nwaves / 4)), dim3(256), 0, st, D->v, S.nnz_pattern, SPW,
                         (const double*)D->vals[k], (const double*)D->W, rp, D->partial);
    }
    hipLaunchKernelGGL(k_quad_reduce, dim3(1), dim3(RPMAX), 0, st, nwaves, (const double*)D->partial, rp, D->d_out, 1.0, 0);
    HIPCHK(hipMemcpyAsync(d_out + cbeg, D->d_out, sizeof(double) * rc, hipMemcpyDeviceToDevice, st));
  }
  HIPCHK(hipEventRecord(D->ev[7], st));
  HIPCHK(hipGetLastError());
  return SCILMM_OK;
}

int quad_host(scilmm_symbolic* sym, Dev* D, int32_t k, const double* U, int32_t r, double* out) {
  const size_t cnt = (size_t)sym->S->n * (size_t)r;
  TRY(ensure_io(sym, D, cnt + (size_t)r));
  HIPCHK(hipMemcpyAsync(D->IO, U, cnt * sizeof(double), hipMemcpyHostToDevice, D->stream));
  TRY(run_quad(sym, D, k, D->IO, r, D->IO + cnt));
  HIPCHK(hipMemcpyAsync(out, D->IO + cnt, sizeof(double) * r, hipMemcpyDeviceToHost, D->stream));
  HIPCHK(hipStreamSynchronize(D->stream));
  float q = 0;
  HIPCHK(hipEventElapsedTime(&q, D->ev[6], D->ev[7]));
  D->timing.quad_ms = q;
  return SCILMM_OK;
}

// dY = A_k dX (device, row-major n x r, original row order); asynchronous on the handle's stream
int run_spmm(scilmm_symbolic* sym, Dev* D, int32_t k, const double* dX, int32_t r, double* dY) {
  const Symbolic& S = *sym->S;
  TRY(ensure_work(sym, D));
  hipStream_t s = D->stream;
  for (int32_t cbeg = 0; cbeg < r; cbeg += RPMAX) {
    const int rc = std::min<int>(RPMAX, r - cbeg);
    const int rp = rp_of(rc);
    const int64_t tot = (int64_t)S.n * rp;
    const unsigned pb = (unsigned)((tot + 255) / 256);
    hipLaunchKernelGGL(k_perm_in, dim3(pb), dim3(256), 0, s, S.n, r, rp, cbeg, D->v.perm, dX, D->W);
    HIPCHK(hipMemsetAsync(D->X, 0, sizeof(double) * (size_t)tot, s));
    if (S.is_diag[k]) {
      hipLaunchKernelGGL(k_spmm_diag, dim3(pb), dim3(256), 0, s, S.n, (const double*)D->vals[k], (const double*)D->W, rp, D->X);
    } else if (D->det) {
      // (deterministic mode: a workgroup per row of the product, fixed summation order, plain stores)
      hipLaunchKernelGGL(k_spmm_row, dim3((unsigned)S.n), dim3(256), 0, s, D->v, D->d_pat_rowptr, D->d_pat_rowcol, D->d_pat_rowslot,
                         (const double*)D->vals[k], (const double*)D->W, rp, D->X);
    } else {
      // (a wave per 256 pattern slots; lanes = right-hand-side columns)
      const int64_t spw = 256, nwav = (S.nnz_pattern + spw - 1) / spw;
      D->n_float_atomic++;
      hipLaunchKernelGGL(k_spmm_w, dim3((unsigned)((nwav + 3) / 4)), dim3(256), 0, s, D->v, S.nnz_pattern, spw,
                         (const double*)D->vals[k], (const double*)D->W, rp, D->X);
    }
    hipLaunchKernelGGL(k_perm_out, dim3(pb), dim3(256), 0, s, S.n, r, rp, cbeg, D->v.perm, (const double*)D->X, dY);
  }
  HIPCHK(hipGetLastError());
  return SCILMM_OK;
}

int spmm_host(scilmm_symbolic* sym, Dev* D, int32_t k, const double* X, int32_t r, double* Y) {
  const size_t cnt = (size_t)sym->S->n * (size_t)r;
  TRY(ensure_work(sym, D));  // (before anything is staged: a handle without work buffers is refused untouched)
  TRY(ensure_io(sym, D, 2 * cnt));
  HIPCHK(hipMemcpyAsync(D->IO, X, cnt * sizeof(double), hipMemcpyHostToDevice, D->stream));
  TRY(run_spmm(sym, D, k, D->IO, r, D->IO + cnt));
  HIPCHK(hipMemcpyAsync(Y, D->IO + cnt, cnt * sizeof(double), hipMemcpyDeviceToHost, D->stream));
  HIPCHK(hipStreamSynchronize(D->stream));
  return SCILMM_OK;
}

// sum(A_k1 o A_k2) over the full symmetric matrices and diag(A_k1) . diag(A_k2), from block partials in Dev::IO
int he_moments(scilmm_symbolic* sym, Dev* D, int32_t k1, int32_t k2, double* frob, double* diag_dot) {
  const Symbolic& S = *sym->S;
  constexpr int NBLK = 1024;
  TRY(ensure_io(sym, D, 2 * NBLK));
  hipStream_t s0 = D->stream;
  double* part = D->IO;
  HIPCHK(hipMemsetAsync(part, 0, sizeof(double) * 2 * NBLK, s0));
  const bool d1 = S.is_diag[k1], d2 = S.is_diag[k2];
  // sum over the FULL symmetric matrices = 2 * (sum over the stored lower-triangle slots) - (diagonal part); a
  // diagonal-only matrix meets any other matrix on the diagonal only
  if (!d1 && !d2 && S.nnz_pattern > 0)
    hipLaunchKernelGGL(k_dot_slots, dim3(NBLK), dim3(256), 0, s0, S.nnz_pattern, (const double*)D->vals[k1], (const double*)D->vals[k2], part);
  if (S.n > 0)
    hipLaunchKernelGGL(k_dot_diag, dim3(NBLK), dim3(256), 0, s0, S.n, D->v.pat_colptr, (const double*)D->vals[k1], (const double*)D->vals[k2],
                       d1 ? 1 : 0, d2 ? 1 : 0, part + NBLK);
  long double sum[2];  // all slots | diagonal
  TRY(fold_blocks(sym, D, part, 2, NBLK, sum));
  HIPCHK(hipGetLastError());
  *diag_dot = (double)sum[1];
  *frob = (d1 || d2) ? (double)sum[1] : (double)(2.0L * sum[0] - sum[1]);
  return SCILMM_OK;
}

}  // namespace
