// Kernels of the variant-set tests (scilmm_scan_block_gram_dev, engine.hip): the r x r Gram matrix X^T X of the forward
// solution X a scan block leaves behind -- one more pass over X, GEMM-shaped, on the fp64 matrix pipe.
//   k_scan_gram : slice partial tiles of X^T X (lower triangle of 16 x 16 tiles)   reads  n * rp * 8
//   k_gram_fold : ... folded in slice order and mirrored into the r x r result     reads  slices * tiles * 2 KB
//   k_scan_keep : X copied into a pitched store, for sets wider than a block       reads and writes  n * rp * 8
// No floating-point atomics: every entry's summation order is fixed by (n, rp) alone, in either mode of the handle.
//
// X is row-major n x rp, rp = r rounded up to 16, columns r .. rp zero (k_scan_dequant / k_bed_dequant write them so).
// With the operand convention of kernels.hip.h, for D = X^T X both operands of tile (I, J) at k-step k0 are the SAME
// expression of the column tile: lane l supplies X[k0 + (l >> 4)][16 T + (l & 15)], T = I for A and T = J for B.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "kernels.hip.h"
#include "plan_types.h"

#ifndef SCILMM_GRAM_SLICE
#define SCILMM_GRAM_SLICE 512
#endif
#ifndef SCILMM_GRAM_LDS
#define SCILMM_GRAM_LDS 1
#endif

namespace scilmm {

constexpr int GRAM_SLICE = SCILMM_GRAM_SLICE;  // rows of X per workgroup of k_scan_gram: the slices depend on n only
constexpr bool GRAM_LDS = SCILMM_GRAM_LDS;     // fragments from an LDS image of GRAM_ROWS rows (1) or straight from global memory (0)
constexpr int GRAM_ROWS = 16;                  // rows of X per LDS image: four k-steps between two barriers
constexpr int GRAM_LD = RPMAX + 16;            // its leading dimension: (ld * 8 B) == 128 mod 256 -> conflict-free b64 reads
constexpr int GRAM_TILES = (RPMAX / 16) * (RPMAX / 16 + 1) / 2;   // 16 x 16 tiles with J <= I at rp = RPMAX: 36
constexpr int GRAM_PER_WAVE = (GRAM_TILES + 3) / 4;               // ... dealt to four waves: 9 tiles = 36 accumulator doubles per lane
constexpr int GRAM_FOLD = 4;                   // contiguous runs of slices summed side by side, then added up in run order

// partial[slice][t][256]: tile t = I (I + 1) / 2 + J (J <= I < rp / 16) of the slice's rows, entry (row, col) of the tile at
// 16 * row + col.  One workgroup of four waves per slice; wave w takes tiles w, w + 4, ...  The rows of the last slice past
// n are zero fragments: nothing is read at or past X + n * rp.  A tile's sum runs over the slice's k-steps in ascending
// order, four rows per MFMA: the order depends on n alone.
template <int SLICE, bool LDS>
__global__ __launch_bounds__(256) void k_scan_gram(int32_t n, int32_t rp, const double* __restrict__ X, double* __restrict__ partial) {
  static_assert(SLICE % GRAM_ROWS == 0 && GRAM_ROWS % 4 == 0, "a slice is whole LDS images, an image whole k-steps");
  __shared__ double xs[LDS ? GRAM_ROWS * GRAM_LD : 1];
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nt = rp >> 4, ntile = nt * (nt + 1) / 2;
  const int64_t p0 = (int64_t)blockIdx.x * SLICE;
  const int64_t p1 = min(p0 + SLICE, (int64_t)n);
  // the wave's tiles: column offsets of the A and the B fragment (wave-uniform)
  int ca[GRAM_PER_WAVE], cb[GRAM_PER_WAVE];
#pragma unroll
  for (int s = 0; s < GRAM_PER_WAVE; ++s) {
    const int t = wv + 4 * s;
    int I = 0;
    while ((I + 1) * (I + 2) / 2 <= t) ++I;
    ca[s] = 16 * I;
    cb[s] = 16 * (t - I * (I + 1) / 2);
  }
  d4 acc[GRAM_PER_WAVE];
#pragma unroll
  for (int s = 0; s < GRAM_PER_WAVE; ++s) acc[s] = d4{0.0, 0.0, 0.0, 0.0};

  if constexpr (LDS) {
    // an image is GRAM_ROWS whole rows = GRAM_ROWS * rp contiguous doubles of X, fetched 16 bytes per lane (rp is even and X
    // starts on a 16-byte boundary); the next image travels in registers while the MFMAs of this one run
    const int half = rp >> 1;             // double2 per row
    const int per = GRAM_ROWS * half;     // ... per image: at most 4 per thread
    double2 st[4];
    auto fetch = [&](int64_t q0) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = tid + 256 * u;
        const int row = e / half;
        st[u] = (e < per && q0 + row < p1) ? *(const double2*)(X + (q0 + row) * rp + 2 * (e - row * half)) : double2{0.0, 0.0};
      }
    };
    fetch(p0);
    for (int64_t q0 = p0; q0 < p1; q0 += GRAM_ROWS) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = tid + 256 * u;
        const int row = e / half;
        if (e < per) *(double2*)(xs + row * GRAM_LD + 2 * (e - row * half)) = st[u];
      }
      __syncthreads();
      if (q0 + GRAM_ROWS < p1) fetch(q0 + GRAM_ROWS);
#pragma unroll
      for (int kk = 0; kk < GRAM_ROWS / 4; ++kk) {
        const double* xr = xs + (4 * kk + lk) * GRAM_LD + li;
#pragma unroll
        for (int s = 0; s < GRAM_PER_WAVE; ++s)
          if (wv + 4 * s < ntile) acc[s] = mfma_f64(xr[ca[s]], xr[cb[s]], acc[s]);
      }
      __syncthreads();
    }
  } else {
    for (int64_t q0 = p0; q0 < p1; q0 += 4) {
      const bool ok = q0 + lk < p1;
      const double* xr = X + (q0 + lk) * rp + li;
#pragma unroll
      for (int s = 0; s < GRAM_PER_WAVE; ++s)
        if (wv + 4 * s < ntile) acc[s] = mfma_f64(ok ? xr[ca[s]] : 0.0, ok ? xr[cb[s]] : 0.0, acc[s]);
    }
  }
  // lane l holds entries (lk + 4 reg, li) of its tiles: 16 (lk + 4 reg) + li = 64 reg + l
#pragma unroll
  for (int s = 0; s < GRAM_PER_WAVE; ++s) {
    const int t = wv + 4 * s;
    if (t < ntile) {
      double* o = partial + ((int64_t)blockIdx.x * ntile + t) * 256 + lane;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) o[64 * reg] = acc[s][reg];
    }
  }
}

// The slicing a Gram block runs with: GRAM_SLICE and GRAM_LDS.  Builds with -DSCILMM_DIAG (the timing ablations: another
// slicing gives other last bits) also take SCILMM_GRAM_SHAPE=<slice>:<lds>, slice in 256 / 512 / 1024 / 2048, read per call
// (tools/sets_timing.py times them side by side in one run).
struct GramShape {
  int slice;
  bool lds;
};
using GramKernel = void (*)(int32_t, int32_t, const double*, double*);
#ifdef SCILMM_DIAG
constexpr int GRAM_SLICE_MIN = 256;
#else
constexpr int GRAM_SLICE_MIN = GRAM_SLICE;
#endif

inline GramShape gram_shape() {
  GramShape g{GRAM_SLICE, GRAM_LDS};
#ifdef SCILMM_DIAG
  if (const char* e = getenv("SCILMM_GRAM_SHAPE")) {
    const int s = atoi(e);
    const char* c = strchr(e, ':');
    if (s == 256 || s == 512 || s == 1024 || s == 2048) g.slice = s;
    if (c) g.lds = c[1] != '0';
  }
#endif
  return g;
}

inline GramKernel gram_kernel(GramShape g) {
#ifdef SCILMM_DIAG
  switch (g.slice) {
    case 256: return g.lds ? k_scan_gram<256, true> : k_scan_gram<256, false>;
    case 512: return g.lds ? k_scan_gram<512, true> : k_scan_gram<512, false>;
    case 1024: return g.lds ? k_scan_gram<1024, true> : k_scan_gram<1024, false>;
    case 2048: return g.lds ? k_scan_gram<2048, true> : k_scan_gram<2048, false>;
  }
#endif
  return k_scan_gram<GRAM_SLICE, GRAM_LDS>;
}

// gram[i][j] (r x r, leading dimension r) = sum over the slices of the partial tiles, one workgroup per tile t =
// blockIdx.x: GRAM_FOLD contiguous runs of slices are summed side by side, each in slice order, and the runs are added up in
// run order -- the fixed tree of k_scan_fold.  Of a diagonal tile only the entries with col <= row are taken; every entry
// off the diagonal is written twice, as (i, j) and as (j, i), from ONE sum: the result is symmetric bit for bit.  Exactly
// r * r values are written (the padding rows and columns r .. rp are skipped).
__global__ __launch_bounds__(GRAM_FOLD * 256) void k_gram_fold(int64_t nslice, int32_t ntile, const double* __restrict__ partial,
                                                               int32_t r, double* __restrict__ gram) {
  __shared__ double red[GRAM_FOLD * 256];
  const int tid = threadIdx.x, e = tid & 255, run = tid >> 8;
  const int t = blockIdx.x;
  const int64_t per = (nslice + GRAM_FOLD - 1) / GRAM_FOLD;
  const int64_t s0 = run * per, s1 = min(nslice, s0 + per);
  double s = 0.0;
  for (int64_t sl = s0; sl < s1; ++sl) s += partial[(sl * ntile + t) * 256 + e];
  red[tid] = s;
  __syncthreads();
  if (run == 0) {
    int I = 0;
    while ((I + 1) * (I + 2) / 2 <= t) ++I;
    const int J = t - I * (I + 1) / 2;
    const int i = 16 * I + (e >> 4), j = 16 * J + (e & 15);
    if (i < r && j <= i) {
      double v = red[e];
#pragma unroll
      for (int u = 1; u < GRAM_FOLD; ++u) v += red[u * 256 + e];
      gram[(int64_t)i * r + j] = v;
      if (j < i) gram[(int64_t)j * r + i] = v;
    }
  }
}

// A set wider than one block (scilmm_scan_block_keep_dev): the block's forward solution X (n x rp, contiguous) copied to
// columns col0 .. col0 + rp - 1 of a pitched store (n x ld_dst), where scilmm_scan_panel_dev reads it as Y for the cross
// products with the sub-blocks that follow.  Store-only: 16 bytes per lane in, 16 bytes per lane out, no LDS, no atomics.  A
// workgroup takes KEEP_ROWS rows at a time, the workgroups stride over the chunks; rp, ld_dst and col0 are multiples of 16 and
// both bases are 16-byte aligned, so every access is an aligned one.  Nothing is read at or past X + n * rp, nothing is written
// outside the rp columns of a row below n (ld_dst >= col0 + rp); the zero padding r .. rp - 1 travels with the rest.
constexpr int KEEP_ROWS = 32;      // rows per chunk: 32 * rp / 2 = 256 .. 2048 double2, one to eight per thread
constexpr int KEEP_GRID = 2048;    // workgroups at most: eight per CU, the rest is strided

__global__ __launch_bounds__(256) void k_scan_keep(int32_t n, int32_t rp, const double* __restrict__ X, double* __restrict__ dst, int64_t ld_dst,
                                                   int64_t col0) {
  const int hx = rp >> 1;                                       // double2 per row
  const int64_t nchunk = ((int64_t)n + KEEP_ROWS - 1) / KEEP_ROWS;
  for (int64_t ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
    const int64_t p0 = ch * KEEP_ROWS;
    const int per = (int)min((int64_t)KEEP_ROWS, (int64_t)n - p0) * hx;
    const double* src = X + p0 * rp;
    double* out = dst + p0 * ld_dst + col0;
    for (int e = threadIdx.x; e < per; e += 256) {
      const int row = e / hx;
      const double2 v = *(const double2*)(src + 2 * e);
      *(double2*)(out + row * ld_dst + 2 * (e - row * hx)) = v;
    }
  }
}

}  // namespace scilmm
