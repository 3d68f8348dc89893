// Dominance relationship matrix on the pattern of the IBD matrix, on the device (the
// "gather over A's pattern" half of the construction step before the hot path).  Replaces the reference's
// scilmm/Matrices/Dominance.py:12-43 -- fancy-indexed lookups of a root-padded scipy matrix, four per stored entry:
//   D_ij = 1/4 (A[f_i, f_j] A[m_i, m_j] + A[f_i, m_j] A[m_i, f_j])  for every stored (i, j), i != j;   D_ii = 1,
// f, m = the two recorded parents of an individual, an unknown parent contributing 0 (the reference's all-zero "root"
// row), A entries outside the stored pattern 0.
// HBM-bound integer / gather work: one wavefront per row i, lanes over its stored entries; the index lists of rows f_i
// and m_i are searched by every lane of the wave and stay in cache, the lists of rows f_j / m_j are not needed at all
// (A is symmetric: A[f_i, f_j] is looked up in row f_i).  Products and the sum are rounded one by one (no fma
// contraction), in the reference's order, so the values equal NumPy's bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "dev.h"

namespace {

__device__ __forceinline__ double look(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                       const double* __restrict__ data, int32_t r, int32_t c) {
  if (r < 0 || c < 0) return 0.0;
  int64_t lo = indptr[r], hi = indptr[r + 1];
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (indices[mid] < c) lo = mid + 1;
    else hi = mid;
  }
  return (lo < indptr[r + 1] && indices[lo] == c) ? data[lo] : 0.0;
}

__global__ __launch_bounds__(256) void k_dominance(int32_t n, const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                   const double* __restrict__ data, const int32_t* __restrict__ parents,
                                                   double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t i = wave; i < n; i += nwaves) {
    const int32_t fi = parents[2 * i], mi = parents[2 * i + 1];
    const int64_t b = indptr[i], e = indptr[i + 1];
    for (int64_t t = b + lane; t < e; t += 64) {
      const int32_t j = indices[t];
      double v = 1.0;
      if (j != (int32_t)i) {
        const int32_t fj = parents[2 * (int64_t)j], mj = parents[2 * (int64_t)j + 1];
        const double p1 = __dmul_rn(look(indptr, indices, data, fi, fj), look(indptr, indices, data, mi, mj));
        const double p2 = __dmul_rn(look(indptr, indices, data, fi, mj), look(indptr, indices, data, mi, fj));
        v = __dmul_rn(0.25, __dadd_rn(p1, p2));
      }
      out[t] = v;
    }
  }
}

thread_local std::string g_dom_err;

}  // namespace

extern "C" {

const char* scilmm_dominance_error(void) { return g_dom_err.c_str(); }

int scilmm_dominance_dev(int32_t n, const int64_t* d_indptr, const int32_t* d_indices, const double* d_data, const int32_t* d_parents,
                         double* d_out, void* stream) {
  if (n < 0 || !d_indptr || !d_indices || !d_data || !d_parents || !d_out) return SCILMM_ERR_ARG;
  if (n == 0) return SCILMM_OK;
  const unsigned blocks = (unsigned)std::min<int64_t>(((int64_t)n + 3) / 4, 256 * 32);
  hipLaunchKernelGGL(k_dominance, dim3(blocks), dim3(256), 0, (hipStream_t)stream, n, d_indptr, d_indices, d_data, d_parents, d_out);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    g_dom_err = std::string("k_dominance launch: ") + hipGetErrorString(e);
    return SCILMM_ERR_DEVICE;
  }
  return SCILMM_OK;
}

int scilmm_dominance(int32_t n, const int64_t* indptr, const int32_t* indices, const double* data, const int32_t* parents, double* out) {
  if (n < 0 || !indptr || (n > 0 && (!parents || !out))) return SCILMM_ERR_ARG;
  if (n == 0) return SCILMM_OK;
  const int64_t nz = indptr[n];
  if (nz > 0 && (!indices || !data)) return SCILMM_ERR_ARG;
  // rows must be strictly ascending (canonical CSR) and the parents valid: checked here, the kernel trusts them
  for (int32_t i = 0; i < n; ++i) {
    if (indptr[i + 1] < indptr[i]) { g_dom_err = "indptr is not monotone"; return SCILMM_ERR_ARG; }
    for (int64_t t = indptr[i]; t < indptr[i + 1]; ++t)
      if (indices[t] < 0 || indices[t] >= n || (t > indptr[i] && indices[t - 1] >= indices[t])) {
        g_dom_err = "row indices must be strictly ascending and inside [0, n)";
        return SCILMM_ERR_ARG;
      }
    for (int q = 0; q < 2; ++q)
      if (parents[2 * (int64_t)i + q] < -1 || parents[2 * (int64_t)i + q] >= n) { g_dom_err = "parent index out of range"; return SCILMM_ERR_ARG; }
  }
  // (the temporaries are freed on every return path)
  scilmm::DevScratch tmp(&g_dom_err);
  int64_t* dp = nullptr;
  int32_t *di = nullptr, *dpar = nullptr;
  double *dd = nullptr, *dout = nullptr;
  TRY(tmp.upload(indptr, (size_t)n + 1, &dp));
  TRY(tmp.upload(indices, (size_t)nz, &di));
  TRY(tmp.upload(data, (size_t)nz, &dd));
  TRY(tmp.upload(parents, 2 * (size_t)n, &dpar));
  TRY(tmp.alloc((size_t)nz, &dout));
  TRY(scilmm_dominance_dev(n, dp, di, dd, dpar, dout, nullptr));
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout, sizeof(double) * (size_t)nz, hipMemcpyDeviceToHost);
  return e == hipSuccess ? SCILMM_OK : tmp.fail("scilmm_dominance: synchronise and copy back", e);
}

}  // extern "C"
