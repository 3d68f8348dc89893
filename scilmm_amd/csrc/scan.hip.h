// Kernels of the marker association scan (scilmm_scan_block_dev, engine.hip): one block of up to RPMAX int8 markers is
// turned into the right-hand-side block of the forward sweep, and the forward solution is reduced to a few numbers per
// marker.  All three are streaming kernels (HBM-bound, no matrix-core work):
//   k_scan_moments : per marker n_obs, mean, centred sum of squares           reads  r * n bytes
//   k_scan_dequant : W = P (g - mean), missing = 0, columns padded to rp      reads  r * n bytes, writes n * rp * 8
//   k_scan_stats   : slice partial sums of |x_c|^2 and Q^T x_c from X         reads  n * (rp + q) * 8
//   k_scan_fold    : ... folded in slice order                                reads  slices * (q + 1) * RPMAX * 8
// The first two have two siblings per input form, which write the same rows of the statistics and the same W:
//   k_bed_moments / k_bed_dequant (bed.hip.h)           PLINK 1 2-bit rows       reads  r * ceil(N/4) bytes each
//   k_dos_moments<T> / k_dos_dequant<T> (dosage.hip.h)  uint16 / float dosages   reads  r * N * sizeof(T) each (float moments twice)
// A marker x environment block (scilmm_scan_block_gxe_dev; d = 1 + m columns per marker) adds two, for every input form:
//   k_scan_expand  : W[:, a r + c] = W[:, c] E[:, a - 1] in place               reads  n * (r + m) * 8, writes n * m * r * 8
//   k_scan_cross   : slice partial sums of x_a' x_b, a < b, per marker, from X   reads  n * d * r * 8; folded by k_scan_fold
// No floating-point atomics: a marker's statistics are the same bits in every run and in either mode of the handle.
//
// Genotype layout: marker j = geno + j * ld, n int8 values in the ORIGINAL order of the individuals, negative = missing.
// Rows are read in ALIGNED 16-byte pieces whatever ld and the base address are: a piece is fetched only when it holds at
// least one byte of the row, so it lies inside the caller's allocation (allocations start and end on 16-byte boundaries),
// and the bytes of a piece that belong to a neighbouring row are masked by their index.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "plan_types.h"

namespace scilmm {

constexpr int SCAN_QMAX = 32;    // columns of the whitened covariate block Q = [w(C) | w(y)]
constexpr int SCAN_SLICE = 256;  // rows of X per workgroup of k_scan_stats: the slices depend on n only
constexpr int SCAN_TILE = 64;    // individuals per workgroup of k_scan_dequant
constexpr int SCAN_LDG = 21;     // dwords per marker of its LDS image: 5 pieces of 16 B (64 + 15 bytes) and one of padding --
                                 // an odd stride, so the byte reads of 32 consecutive markers fall on 32 different banks
constexpr int SCAN_FOLD = 8;     // contiguous runs of slices summed side by side, then added up in run order

__device__ __forceinline__ int scan_byte(const int4& v, int j) {
  const int w = j >> 2 == 0 ? v.x : j >> 2 == 1 ? v.y : j >> 2 == 2 ? v.z : v.w;
  return (int)(int8_t)(w >> (8 * (j & 3)));
}

// stats[0][c] = observed individuals, stats[1][c] = their mean allele count (0 when there is none), stats[2][c] = their
// centred sum of squares.  One workgroup per marker; the three sums are INTEGERS, so their order is immaterial.
__global__ __launch_bounds__(256) void k_scan_moments(int32_t n, const int8_t* __restrict__ geno, int64_t ld, int32_t r,
                                                      double* __restrict__ stats) {
  __shared__ long long red[4][3];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int c = blockIdx.x;
  const int8_t* row = geno + (int64_t)c * ld;
  const int head = (int)((uintptr_t)row & 15);  // bytes of the first piece that precede the row
  const int4* base = (const int4*)(row - head);
  const int64_t npiece = ((int64_t)head + n + 15) >> 4;
  long long cnt = 0, sum = 0, sq = 0;
  for (int64_t k = tid; k < npiece; k += 256) {
    const int4 v = base[k];
    const int64_t i0 = 16 * k - head;  // individual of the piece's first byte
    const bool inside = i0 >= 0 && i0 + 16 <= n;
    int lc = 0, ls = 0, lq = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int g = scan_byte(v, j);
      const bool ok = g >= 0 && (inside || (i0 + j >= 0 && i0 + j < n));
      lc += ok ? 1 : 0;
      ls += ok ? g : 0;
      lq += ok ? g * g : 0;
    }
    cnt += lc;
    sum += ls;
    sq += lq;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cnt += __shfl_down(cnt, o);
    sum += __shfl_down(sum, o);
    sq += __shfl_down(sq, o);
  }
  if (lane == 0) {
    red[wv][0] = cnt;
    red[wv][1] = sum;
    red[wv][2] = sq;
  }
  __syncthreads();
  if (tid == 0) {
    cnt = red[0][0] + red[1][0] + red[2][0] + red[3][0];
    sum = red[0][1] + red[1][1] + red[2][1] + red[3][1];
    sq = red[0][2] + red[1][2] + red[2][2] + red[3][2];
    const double mean = cnt > 0 ? (double)sum / (double)cnt : 0.0;
    stats[c] = (double)cnt;
    stats[(int64_t)r + c] = mean;
    // (exactly 0 for a monomorphic marker: its mean is the integer every observed value equals)
    stats[2 * (int64_t)r + c] = cnt > 0 ? (double)sq - (double)sum * mean : 0.0;
  }
}

// The sweeps' right-hand-side block from the markers: out[iperm[i]][c] = g_c[i] - mean_c (0 where g_c[i] is missing, 0 in
// the padding columns r <= c < rp) -- the permutation is fused: individual i goes straight to its row of W.  A workgroup
// takes SCAN_TILE individuals of every marker: 16-byte reads along n into an LDS image [marker][individual], then every
// wave writes whole rows of the block, 512 contiguous bytes per store.  (Writing the original order into a staging buffer
// and permuting with k_perm_in was measured slower)
__global__ __launch_bounds__(256) void k_scan_dequant(int32_t n, int32_t r, int32_t rp, const int8_t* __restrict__ geno,
                                                      int64_t ld, const int32_t* __restrict__ iperm,
                                                      const double* __restrict__ mean, double* __restrict__ out) {
  __shared__ int32_t gs[RPMAX * SCAN_LDG];
  __shared__ double ms[RPMAX];
  __shared__ int32_t dst[SCAN_TILE];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t i0 = (int64_t)blockIdx.x * SCAN_TILE;
  const int ni = (int)min((int64_t)SCAN_TILE, (int64_t)n - i0);
  if (tid < RPMAX) ms[tid] = tid < r ? mean[tid] : 0.0;
  if (tid < SCAN_TILE) dst[tid] = tid < ni ? iperm[i0 + tid] : 0;
  for (int t = tid; t < 5 * r; t += 256) {
    const int c = t / 5, k = t - 5 * c;
    const int8_t* p = geno + (int64_t)c * ld + i0;
    const int head = (int)((uintptr_t)p & 15);
    // piece k holds the tile's individuals 16 k - head .. 16 k - head + 15: fetched when one of them exists
    if (16 * k - head < ni) {
      const int4 v = *(const int4*)(p - head + 16 * k);
      int32_t* g4 = gs + c * SCAN_LDG + 4 * k;
      g4[0] = v.x;
      g4[1] = v.y;
      g4[2] = v.z;
      g4[3] = v.w;
    }
  }
  __syncthreads();
  const int8_t* gb = (const int8_t*)gs;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int c = lane + 64 * h;
    if (c >= rp) continue;
    const bool live = c < r;
    const int off = live ? c * (4 * SCAN_LDG) + (int)((uintptr_t)(geno + (int64_t)c * ld + i0) & 15) : 0;
    const double m = ms[c];
    for (int i = wv; i < ni; i += 4) {
      const int g = live ? (int)gb[off + i] : -1;
      out[(int64_t)dst[i] * rp + c] = g >= 0 ? (double)g - m : 0.0;
    }
  }
}

// partial[slice][0][c] = sum over the slice's rows of X[p][c]^2, partial[slice][1 + k][c] = sum of Q[p][k] X[p][c]: X is
// read once.  A slice is SCAN_SLICE consecutive rows; threads 0..127 take its even rows and threads 128..255 its odd rows
// of column tid & 127, each in ascending order, and the two halves are added even + odd: the order of every sum depends
// on n alone.  The row of Q is the same for a whole wave (scalar loads, 2 QC registers per row in flight): QC = the bound
// on q the instance is compiled for, U = rows a thread keeps in flight -- neither changes the order of a sum.
template <int QC, int U>
__global__ __launch_bounds__(256) void k_scan_stats(int32_t n, int32_t rp, const double* __restrict__ X,
                                                    const double* __restrict__ Q, int32_t q, double* __restrict__ partial) {
  __shared__ double red[(QC + 1) * RPMAX];
  const int tid = threadIdx.x, c = tid & (RPMAX - 1);
  const int g = __builtin_amdgcn_readfirstlane(tid >> 7);
  const int64_t p0 = (int64_t)blockIdx.x * SCAN_SLICE;
  const int64_t p1 = min(p0 + SCAN_SLICE, (int64_t)n);
  const bool on = c < rp;
  double acc[QC + 1];
#pragma unroll
  for (int k = 0; k <= QC; ++k) acc[k] = 0.0;
  for (int64_t p = p0 + g; p < p1; p += 2 * U) {
    double x[U];
#pragma unroll
    for (int u = 0; u < U; ++u) x[u] = (on && p + 2 * u < p1) ? X[(p + 2 * u) * rp + c] : 0.0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (p + 2 * u >= p1) break;
      const double* qr = Q + (p + 2 * u) * q;
      acc[0] += x[u] * x[u];
#pragma unroll
      for (int k = 0; k < QC; ++k)
        if (k < q) acc[1 + k] += qr[k] * x[u];
    }
  }
  if (g == 1) {
#pragma unroll
    for (int k = 0; k <= QC; ++k)
      if (k <= q) red[k * RPMAX + c] = acc[k];
  }
  __syncthreads();
  if (g == 0) {
    double* o = partial + (int64_t)blockIdx.x * (q + 1) * RPMAX + c;
#pragma unroll
    for (int k = 0; k <= QC; ++k)
      if (k <= q) o[(int64_t)k * RPMAX] = acc[k] + red[k * RPMAX + c];
  }
}

// out[k][c] = sum over the slices of partial[slice][k][c], k = blockIdx.x: SCAN_FOLD contiguous runs of slices are summed
// side by side, each in slice order, and the runs are added up in run order -- a fixed tree whose shape depends on n alone.
__global__ __launch_bounds__(SCAN_FOLD * RPMAX) void k_scan_fold(int64_t nslice, const double* __restrict__ partial, int32_t q,
                                                                 int32_t r, double* __restrict__ out) {
  __shared__ double red[SCAN_FOLD * RPMAX];
  const int tid = threadIdx.x, c = tid & (RPMAX - 1), run = tid >> 7;
  const int k = blockIdx.x;
  const int64_t per = (nslice + SCAN_FOLD - 1) / SCAN_FOLD;
  const int64_t s0 = run * per, s1 = min(nslice, s0 + per);
  double s = 0.0;
  if (c < r)
    for (int64_t sl = s0; sl < s1; ++sl) s += partial[(sl * (q + 1) + k) * RPMAX + c];
  red[tid] = s;
  __syncthreads();
  if (run == 0 && c < r) {
    double t = red[c];
#pragma unroll
    for (int u = 1; u < SCAN_FOLD; ++u) t += red[u * RPMAX + c];
    out[(int64_t)k * r + c] = t;
  }
}

// ---- marker x environment blocks (scilmm_scan_block_gxe_dev): d = 1 + m terms per marker, column a r + c = term a of marker c.

constexpr int GXE_MMAX = 3;    // environment columns at most: d <= 4 terms, r <= RPMAX / d markers
constexpr int GXE_ROWS = 64;   // rows of W per workgroup of k_scan_expand
constexpr int GXE_PAIRS = (GXE_MMAX + 1) * GXE_MMAX / 2;

// W[p][a r + c] = W[p][c] E[p][a - 1], a = 1..m, c < r: the interaction columns from the centred marker columns a form's
// dequantise kernel has written (columns r..rp-1 hold its zeros: those past d r stay).  In place: columns < r are read,
// columns >= r written, every entry by the lane that read its source.  Lanes run along the markers (r <= 64: one lane each),
// a wave takes every fourth row of the workgroup's GXE_ROWS, U rows in flight; the row of E is the same for a whole wave
// (scalar loads).  E is n x m row-major in the PERMUTED order, like W.
template <int U>
__global__ __launch_bounds__(256) void k_scan_expand(int32_t n, int32_t r, int32_t m, int32_t rp, const double* __restrict__ E,
                                                     double* W) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t p0 = (int64_t)blockIdx.x * GXE_ROWS;
  const int64_t p1 = min(p0 + GXE_ROWS, (int64_t)n);
  if (lane >= r) return;
  for (int64_t p = p0 + wv; p < p1; p += 4 * U) {
    double x[U];
#pragma unroll
    for (int u = 0; u < U; ++u) x[u] = p + 4 * u < p1 ? W[(p + 4 * u) * rp + lane] : 0.0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (p + 4 * u >= p1) break;
      const double* e = E + (p + 4 * u) * m;
      double* row = W + (p + 4 * u) * rp + lane;
#pragma unroll
      for (int a = 1; a <= GXE_MMAX; ++a)
        if (a <= m) row[a * r] = x[u] * e[a - 1];
    }
  }
}

// partial[slice][k][c] = sum over the slice's rows of X[p][a r + c] X[p][b r + c], k = the index of the pair (a, b), a < b < D,
// in lexicographic order: the cross products between the D columns of one marker, from a second pass over X where it lies.
// The layout is k_scan_stats' with D (D - 1) / 2 rows in place of q + 1, so k_scan_fold folds it.  A slice is SCAN_SLICE
// consecutive rows; the workgroup is 256 / CWX row groups of CWX markers (CWX = 32 when r <= 32: no idle half-waves), group g
// takes rows g, g + G, .. of the slice in ascending order, and the groups are added in group order: the order of every sum
// depends on (n, r, D) alone.  No atomics.
template <int D, int CWX>
__global__ __launch_bounds__(256) void k_scan_cross(int32_t n, int32_t r, int32_t rp, const double* __restrict__ X,
                                                    double* __restrict__ partial) {
  constexpr int NP = D * (D - 1) / 2, G = 256 / CWX;
  __shared__ double red[G * NP * CWX];
  const int tid = threadIdx.x, c = tid & (CWX - 1), g = tid / CWX;
  const int64_t p0 = (int64_t)blockIdx.x * SCAN_SLICE;
  const int64_t p1 = min(p0 + SCAN_SLICE, (int64_t)n);
  const bool on = c < r;
  double acc[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) acc[k] = 0.0;
#pragma unroll 4
  for (int64_t p = p0 + g; p < p1; p += G) {
    double x[D];
#pragma unroll
    for (int a = 0; a < D; ++a) x[a] = on ? X[p * rp + a * r + c] : 0.0;
    int k = 0;
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int b = a + 1; b < D; ++b) acc[k++] += x[a] * x[b];
  }
#pragma unroll
  for (int k = 0; k < NP; ++k) red[(g * NP + k) * CWX + c] = acc[k];
  __syncthreads();
  for (int i = tid; i < NP * CWX; i += 256) {
    const int k = i / CWX, cc = i & (CWX - 1);
    double s = red[k * CWX + cc];
#pragma unroll
    for (int u = 1; u < G; ++u) s += red[(u * NP + k) * CWX + cc];
    if (cc < r) partial[((int64_t)blockIdx.x * NP + k) * RPMAX + cc] = s;
  }
}

}  // namespace scilmm
