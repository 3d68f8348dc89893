// Kernels of the BLUP blocks (scilmm_rel_block_dev / scilmm_rows_block_dev, engine.hip): the right-hand-side block of the
// forward sweep is built from columns of G = sum_k w_k A_k, or from the caller's sparse rows, instead of from markers; the
// forward sweep and the statistics are the marker scan's (scan.hip.h).  Both kernels only STORE into the cleared block:
//   k_rel_gather   : W[p][c] = G[p, p_c] for r requested individuals          reads  4 B per pattern slot (+ the hits' values)
//   k_rows_scatter : W[iperm[idx]][c] = data for r CSR rows                   reads  20 B per stored entry
// Nothing is summed across threads and there are no atomics: every entry of the block has one writer, so the block is the
// same bits in every run and in either mode of the handle.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "plan_types.h"

namespace scilmm {

constexpr int REL_GRID = 2048;  // workgroups of the streaming pass at most (grid-stride beyond)

// The requested individuals of one block, passed by value: permuted index, ascending, and the block column it fills.
struct RelReq {
  int32_t p[RPMAX];
  int32_t col[RPMAX];
};

__device__ __forceinline__ double rel_value(const ValPtrs& vp, int64_t e) {
  double v = 0.0;
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if (k < vp.count) v += vp.s2[k] * vp.v[k][e];
  return v;
}

// The values live as the lower triangle in permuted CSC (pat_colptr / pat_row, diagonal first), so column p_c of the
// symmetric G has two parts.
//   Workgroups 0 .. r-1, the STORED column of request t = blockIdx.x: slots pat_colptr[p] .. pat_colptr[p+1] go to
//     W[pat_row[e]][c].  Thread 0 owns the diagonal entry W[p][c]: the general matrices' first slot plus the diagonal-only
//     matrices' dvals[p]; it also goes to diag[c] (row 0 of the statistics).
//   Workgroups r .., the ROW part (entries (p_c, j < p_c)): one streaming pass over all pattern slots, 64 consecutive slots
//     per wave (coalesced pat_row reads).  A lane bisects its row label in the sorted request list (LDS); on the rare hit
//     it finds its column j by bisecting pat_colptr, as k_spmm does, and stores to W[j][c].
// W must be zero on entry (n x rp; the padding columns r <= c < rp stay zero).  Requests are distinct, so no two threads
// store to the same entry.
__global__ __launch_bounds__(256) void k_rel_gather(DevSym S, int64_t nnz, ValPtrs gen, ValPtrs dia, RelReq req, int32_t r,
                                                    int32_t rp, double* __restrict__ W, double* __restrict__ diag) {
  __shared__ int32_t ps[RPMAX];
  __shared__ int32_t cs[RPMAX];
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < r) {
    const int32_t p = req.p[blockIdx.x], c = req.col[blockIdx.x];
    const int64_t e0 = S.pat_colptr[p], e1 = S.pat_colptr[p + 1];
    const bool stored_diag = e0 < e1 && S.pat_row[e0] == p;
    if (tid == 0) {
      double d = stored_diag ? rel_value(gen, e0) : 0.0;
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (k < dia.count) d += dia.s2[k] * dia.v[k][p];
      W[(int64_t)p * rp + c] = d;
      diag[c] = d;
    }
    if (gen.count > 0)
      for (int64_t e = e0 + (stored_diag ? 1 : 0) + tid; e < e1; e += 256) W[(int64_t)S.pat_row[e] * rp + c] = rel_value(gen, e);
    return;
  }
  if (gen.count == 0) return;
  if (tid < RPMAX) {
    ps[tid] = tid < r ? req.p[tid] : 0x7fffffff;
    cs[tid] = tid < r ? req.col[tid] : 0;
  }
  __syncthreads();
  const int32_t pmin = ps[0], pmax = ps[r - 1];
  const int64_t stride = (int64_t)(gridDim.x - r) * 256;
  for (int64_t e = (int64_t)(blockIdx.x - r) * 256 + tid; e < nnz; e += stride) {
    const int32_t i = S.pat_row[e];
    if (i < pmin || i > pmax) continue;
    int lo = 0, hi = r;  // first request with p >= i
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (ps[mid] < i) lo = mid + 1; else hi = mid;
    }
    if (lo >= r || ps[lo] != i) continue;
    int32_t jl = 0, jh = S.n;  // the column that holds slot e
    while (jl < jh) {
      const int32_t mid = (jl + jh) >> 1;
      if (S.pat_colptr[mid + 1] <= e) jl = mid + 1; else jh = mid;
    }
    if (jl == i) continue;  // (the diagonal belongs to the stored column)
    W[(int64_t)jl * rp + cs[lo]] = rel_value(gen, e);
  }
}

// r caller rows in CSR (indices in the ORIGINAL order of the individuals): W[iperm[idx]][c] = data, one wave per row; an
// index outside 0 .. n-1 is skipped.  W must be zero on entry; a row's indices must be distinct (two entries of one index
// would race for one store).  diag[c] = 0: the rows form knows no diagonal entry.
__global__ __launch_bounds__(256) void k_rows_scatter(int32_t n, int32_t r, int32_t rp, const int64_t* __restrict__ indptr,
                                                      const int32_t* __restrict__ indices, const double* __restrict__ data,
                                                      const int32_t* __restrict__ iperm, double* __restrict__ W,
                                                      double* __restrict__ diag) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= r) return;
  if (lane == 0) diag[c] = 0.0;
  const int64_t e1 = indptr[c + 1];
  for (int64_t e = indptr[c] + lane; e < e1; e += 64) {
    const int32_t idx = indices[e];
    if (idx < 0 || idx >= n) continue;
    W[(int64_t)iperm[idx] * rp + c] = data[e];
  }
}

}  // namespace scilmm
