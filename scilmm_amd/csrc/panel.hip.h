// Kernels of the phenotype panels (scilmm_scan_panel_dev, engine.hip): X^T Y for the forward solution X a scan block leaves
// behind (n x rp) and a resident phenotype panel Y (n x t, t up to PANEL_TMAX) -- one more pass over X, a tall-skinny GEMM on
// the fp64 matrix pipe; k_scan_gram (gram.hip.h) is its square symmetric special case.
//   k_scan_panel : slice partial tiles of X^T Y, 128 columns of Y per workgroup   reads  (n * rp + n * 128) * 8 per column panel
//   k_panel_fold : ... folded in slice order into the r x t result                reads  slices * tiles * 2 KB
// No floating-point atomics: the summation order of entry (j, k) is fixed by n alone -- the bits depend on n and on the values
// of X column j and Y column k, not on t, on where column k sits in Y, on r, or on the mode of the handle.
//
// X is row-major n x rp, rp = r rounded up to 16, columns r .. rp zero.  Y is row-major n x ld_y in the factor's PERMUTED row
// order, t <= ld_y, ld_y % 16 == 0, 16-byte aligned; columns t .. ld_y are padding whose VALUES are never used: a column of
// the product takes nothing from another column of Y, and the fold writes columns 0 .. t - 1 only.  With the operand
// convention of kernels.hip.h, for D = X^T Y lane l supplies X[k0 + (l >> 4)][16 I + (l & 15)] as A and
// Y[k0 + (l >> 4)][16 J + (l & 15)] as B; entry (row = (l >> 4) + 4 reg, col = l & 15) of tile (I, J) is
// x_{16 I + row} . y_{16 J + col}.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "kernels.hip.h"
#include "plan_types.h"

#ifndef SCILMM_PANEL_SLICE
#define SCILMM_PANEL_SLICE 2048
#endif

namespace scilmm {

constexpr int PANEL_SLICE = SCILMM_PANEL_SLICE;  // rows of X and Y per workgroup of k_scan_panel: the slices depend on n only
constexpr int PANEL_TMAX = 4096;                 // columns of Y at most
constexpr int PANEL_COLS = 128;                  // columns of Y per workgroup: a column panel of PANEL_NJ tiles
constexpr int PANEL_NJ = PANEL_COLS / 16;
constexpr int PANEL_NI = RPMAX / 16;             // column tiles of X at rp = RPMAX: two per wave
constexpr int PANEL_ROWS = 16;                   // rows per LDS image: four k-steps between two barriers
constexpr int PANEL_LD = RPMAX + 16;             // leading dimension of both images: the conflict-free pitch of GRAM_LD
constexpr int PANEL_FOLD = 4;                    // contiguous runs of slices summed side by side, then added up in run order
static_assert(PANEL_COLS == RPMAX, "both images share one pitch and one fetch pattern");

// partial[slice][panel][tile][256], tile = PANEL_NJ * I + J (I < rp / 16; J < 8, of which the panel's tiles that hold a column
// below t are written), entry (row, col) of the tile at 16 * row + col.  One workgroup of four waves per (slice = blockIdx.x,
// column panel = blockIdx.y); wave w owns X column tiles 2 w and 2 w + 1 against the panel's tiles of Y: 16 accumulators = 64
// doubles per lane, two A and eight B fragments per k-step for 16 MFMAs.  The fragments come from an LDS image of PANEL_ROWS
// rows of X and of the Y panel; the next image travels in registers while the MFMAs of this one run.  The rows of the last
// slice past n are zero fragments: nothing is read at or past X + n * rp or Y + n * ld_y, and of a row of Y only the columns
// below t rounded up to 16 (<= ld_y).  A tile's sum runs over the slice's k-steps in ascending order, four rows per MFMA.
template <int SLICE>
__global__ __launch_bounds__(256) void k_scan_panel(int32_t n, int32_t rp, const double* __restrict__ X, const double* __restrict__ Y,
                                                    int64_t ld_y, int32_t t, double* __restrict__ partial) {
  static_assert(SLICE % PANEL_ROWS == 0 && PANEL_ROWS % 4 == 0, "a slice is whole LDS images, an image whole k-steps");
  __shared__ double xs[PANEL_ROWS * PANEL_LD];
  __shared__ double ys[PANEL_ROWS * PANEL_LD];
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ni = rp >> 4;                                                 // column tiles of X
  const int c0 = PANEL_COLS * (int)blockIdx.y;                            // first column of the panel (< t)
  const int nj = (min(PANEL_COLS, t - c0) + 15) >> 4;                     // its tiles that hold a column below t: 1 .. 8
  const int64_t p0 = (int64_t)blockIdx.x * SLICE;
  const int64_t p1 = min(p0 + SLICE, (int64_t)n);
  const double* Yp = Y + c0;
  d4 acc[2][PANEL_NJ];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int j = 0; j < PANEL_NJ; ++j) acc[a][j] = d4{0.0, 0.0, 0.0, 0.0};

  // an image of X is PANEL_ROWS whole rows = PANEL_ROWS * rp contiguous doubles, an image of Y PANEL_ROWS pieces of 16 nj
  // doubles, ld_y apart; both are fetched 16 bytes per lane (rp, 16 nj, ld_y and c0 are even, X and Y start on 16-byte boundaries)
  const int hx = rp >> 1, hy = 8 * nj;              // double2 per row
  const int perx = PANEL_ROWS * hx, pery = PANEL_ROWS * hy;   // ... per image: at most 4 per thread
  double2 sx[4], sy[4];
  auto fetch = [&](int64_t q0) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = tid + 256 * u;
      const int rx = e / hx, ry = e / hy;
      sx[u] = (e < perx && q0 + rx < p1) ? *(const double2*)(X + (q0 + rx) * rp + 2 * (e - rx * hx)) : double2{0.0, 0.0};
      sy[u] = (e < pery && q0 + ry < p1) ? *(const double2*)(Yp + (q0 + ry) * ld_y + 2 * (e - ry * hy)) : double2{0.0, 0.0};
    }
  };
  const bool i0 = 2 * wv < ni, i1 = 2 * wv + 1 < ni;   // (wave-uniform)
  fetch(p0);
  for (int64_t q0 = p0; q0 < p1; q0 += PANEL_ROWS) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = tid + 256 * u;
      const int rx = e / hx, ry = e / hy;
      if (e < perx) *(double2*)(xs + rx * PANEL_LD + 2 * (e - rx * hx)) = sx[u];
      if (e < pery) *(double2*)(ys + ry * PANEL_LD + 2 * (e - ry * hy)) = sy[u];
    }
    __syncthreads();
    if (q0 + PANEL_ROWS < p1) fetch(q0 + PANEL_ROWS);
    if (i0) {
#pragma unroll
      for (int kk = 0; kk < PANEL_ROWS / 4; ++kk) {
        const double* xr = xs + (4 * kk + lk) * PANEL_LD + 32 * wv + li;
        const double* yr = ys + (4 * kk + lk) * PANEL_LD + li;
        const double a0 = xr[0], a1 = i1 ? xr[16] : 0.0;
#pragma unroll
        for (int j = 0; j < PANEL_NJ; ++j)
          if (j < nj) {
            const double b = yr[16 * j];
            acc[0][j] = mfma_f64(a0, b, acc[0][j]);
            if (i1) acc[1][j] = mfma_f64(a1, b, acc[1][j]);
          }
      }
    }
    __syncthreads();
  }
  // lane l holds entries (lk + 4 reg, li) of its tiles: 16 (lk + 4 reg) + li = 64 reg + l
  const int64_t cell = ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * (ni * PANEL_NJ);
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int I = 2 * wv + a;
    if (I < ni) {
#pragma unroll
      for (int j = 0; j < PANEL_NJ; ++j)
        if (j < nj) {
          double* o = partial + (cell + I * PANEL_NJ + j) * 256 + lane;
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) o[64 * reg] = acc[a][j][reg];
        }
    }
  }
}

// The slicing a panel call runs with: PANEL_SLICE.  Builds with -DSCILMM_DIAG (the timing ablations: another slicing gives
// other last bits) also take SCILMM_PANEL_SHAPE=<slice>, 512 / 1024 / 2048, read per call (tools/panel_timing.py times them
// side by side in one run).
using PanelKernel = void (*)(int32_t, int32_t, const double*, const double*, int64_t, int32_t, double*);
#ifdef SCILMM_DIAG
constexpr int PANEL_SLICE_MIN = 512;
#else
constexpr int PANEL_SLICE_MIN = PANEL_SLICE;
#endif

inline int panel_slice() {
#ifdef SCILMM_DIAG
  if (const char* e = getenv("SCILMM_PANEL_SHAPE")) {
    const int s = atoi(e);
    if (s == 512 || s == 1024 || s == 2048) return s;
  }
#endif
  return PANEL_SLICE;
}

inline PanelKernel panel_kernel(int slice) {
#ifdef SCILMM_DIAG
  switch (slice) {
    case 512: return k_scan_panel<512>;
    case 1024: return k_scan_panel<1024>;
    case 2048: return k_scan_panel<2048>;
  }
#endif
  return k_scan_panel<PANEL_SLICE>;
}

// xty[i][k] (r x t, leading dimension ld_out) = sum over the slices of the partial tiles, one workgroup per tile: blockIdx.x
// = (column panel) * ntile + tile, ntile = (rp / 16) * PANEL_NJ.  PANEL_FOLD contiguous runs of slices are summed side by side,
// each in slice order, and the runs are added up in run order -- the fixed tree of k_gram_fold / k_scan_fold; it depends on the
// number of slices alone.  A tile without a column below t was not written and is not read.  Exactly r * t values are written
// (the padding rows r .. rp and the columns t .. are skipped).
__global__ __launch_bounds__(PANEL_FOLD * 256) void k_panel_fold(int64_t nslice, int32_t npanel, int32_t ntile, const double* __restrict__ partial,
                                                                 int32_t r, int32_t t, double* __restrict__ xty, int64_t ld_out) {
  __shared__ double red[PANEL_FOLD * 256];
  const int tid = threadIdx.x, e = tid & 255, run = tid >> 8;
  const int cp = blockIdx.x / ntile, tile = blockIdx.x - cp * ntile;
  const int I = tile / PANEL_NJ, J = tile - I * PANEL_NJ;
  if (PANEL_COLS * cp + 16 * J >= t) return;   // (the whole workgroup)
  const int64_t per = (nslice + PANEL_FOLD - 1) / PANEL_FOLD;
  const int64_t s0 = run * per, s1 = min(nslice, s0 + per);
  double s = 0.0;
  for (int64_t sl = s0; sl < s1; ++sl) s += partial[((sl * npanel + cp) * ntile + tile) * 256 + e];
  red[tid] = s;
  __syncthreads();
  if (run == 0) {
    const int i = 16 * I + (e >> 4), k = PANEL_COLS * cp + 16 * J + (e & 15);
    if (i < r && k < t) {
      double v = red[e];
#pragma unroll
      for (int u = 1; u < PANEL_FOLD; ++u) v += red[u * 256 + e];
      xty[(int64_t)i * ld_out + k] = v;
    }
  }
}

}  // namespace scilmm
