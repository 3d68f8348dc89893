// Kernels of the variant-set tests for binary traits for ONE set of up to 4 096 markers that ran as sub-blocks
// (scilmm_sets_collapse*_dev, scilmm_sets_spa_wide_dev, engine.hip): what k_sets_spa (setspa.hip.h) does for
// a set held in one block, cut where a sub-block ends.
//   k_sets_collapse<Reader> : behind every sub-block; a thread per individual, a capped grid with a fixed stride over n; the
//                             collapsed genotype g_B = sum_j w_j g~_j grows by the sub-block's kept markers.  Reads the
//                             sub-block's r rows once, along the lanes; reads and writes n doubles.
//   k_swide_keep            : behind the last sub-block, one workgroup; the kept markers (in order, by a prefix sum, as k_wide_prep
//                             lists them);
//   k_swide_markers         : a thread per kept marker: z, s, w, a_j = G_jj - z_j'z_j and rho_j from its saddlepoint row; with
//                             k_swide_keep the scale of every marker of the set before the burden floor (1 for a dropped one).
//   k_swide_pairs           : a workgroup per kept row a; sum_b w_a K_ab w_b and the sum with w o rho, K_ab from where the
//                             sub-blocks left X'X (WideIn::xtx, which k_wide_form reads as well); two partials per row to HBM.
//   k_swide_burden          : one workgroup of 256 threads; a_B, V_Q and b_B from the rows' partials, the decision, spa_roots on
//                             the collapsed row, then step 4 of k_sets_spa: the set's 13 numbers and its k scales.
// No atomics; every sum is taken in a fixed order and folded by a fixed tree.  An individual's collapsed value is ONE fma chain
// over the set's kept markers in the order given, so the row carries the same bits however the set is cut into sub-blocks, and
// from the three input forms of the same hard calls (the readers of spa.hip.h).  The pair sums are folded row by row: they agree
// with k_sets_spa's (dealt at a stride of 256 over the pairs) to rounding, not bit for bit.
#pragma once
#include "setspa.hip.h"
#include "setwide.hip.h"

namespace scilmm {

constexpr int COLLAPSE_GRID = 2048;              // workgroups of k_sets_collapse at most

// The handle's wide work space (WideWs's allocation: wide_doubles(k) holds it) cut for the set saddlepoint of k markers.
struct SwideWs {
  double *Z, *s, *w, *rho, *scale, *pa, *pv;     // z (FIN_CMAX x k) | s | w | rho of the kept markers; the scale of every marker; the rows' partials
  int32_t *idx, *ic;
};
__host__ __device__ constexpr size_t swide_doubles(size_t k) { return (FIN_CMAX + 6) * k + (k + WI_N + 1) / 2 + 1; }
static_assert(swide_doubles(1) <= wide_doubles(1) && swide_doubles(WIDE_KMAX) <= wide_doubles(WIDE_KMAX), "the wide work space holds it");
inline SwideWs swide_cut(double* base, size_t k) {
  SwideWs w;
  w.Z = base;
  w.s = w.Z + FIN_CMAX * k;
  w.w = w.s + k;
  w.rho = w.w + k;
  w.scale = w.rho + k;
  w.pa = w.scale + k;
  w.pv = w.pa + k;
  w.idx = (int32_t*)(w.pv + k);
  w.ic = w.idx + k;
  return w;
}

// Where the sub-blocks' saddlepoint calls left a marker's row: slice b at a stride of SPA_ROWS block, SPA_ROWS x r_b
__device__ __forceinline__ double swide_spa(const WideIn& in, const double* __restrict__ spa, int row, int i) {
  const int b = i / in.block, j = i - b * in.block, rb = min(in.block, in.k - b * in.block);
  return spa[(int64_t)b * SPA_ROWS * in.block + (int64_t)row * rb + j];
}

// stats: the sub-block's (q + 4) x r statistics (rows 0 .. 2 are read); weights: its r entries (mode 2); gB: n doubles.
// The kept list, the means and the weights are staged in LDS once per workgroup; the loop over the individuals writes no LDS and
// meets no barrier: a marker's column, mean and weight are the same address for every lane (a broadcast read).
template <class Reader>
__global__ __launch_bounds__(256) void k_sets_collapse(int32_t n, int32_t r, Reader rd, const double* __restrict__ stats, int32_t wmode,
                                                       const double* __restrict__ weights, int32_t first, double* __restrict__ gB) {
  __shared__ double wv_[RPMAX], mv[RPMAX];
  __shared__ int32_t idx[RPMAX], ic[1];
  const int tid = threadIdx.x;
  if (tid == 0) {
    int k = 0;
    for (int j = 0; j < r; ++j)
      if (fin_kept(stats[j], stats[2 * (int64_t)r + j])) idx[k++] = j;
    ic[0] = k;
  }
  __syncthreads();
  const int k = ic[0];
  if (tid < k) {
    const int col = idx[tid];
    const double mean = stats[(int64_t)r + col];
    mv[tid] = mean;
    wv_[tid] = fin_weight(wmode, mean, weights, col);
  }
  __syncthreads();
  if (k == 0 && !first) return;  // (the whole workgroup: the row stays as it is)
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < n; i += stride) {
    double acc = first ? 0.0 : gB[i];
    for (int j = 0; j < k; ++j) acc = fma(wv_[j], rd(idx[j], i, mv[j]), acc);
    gB[i] = acc;
  }
}

// Step 0 of k_sets_spa for k <= 4 096: one workgroup of WIDE_PREP_NT threads, a run of consecutive markers each; the kept markers
// in order (as k_wide_prep lists them), their number, and the scale 1 of every dropped marker.
__global__ __launch_bounds__(WIDE_PREP_NT) void k_swide_keep(WideIn in, SwideWs ws) {
  __shared__ int32_t cnt[WIDE_PREP_NT];
  const int tid = threadIdx.x, k = in.k;
  const int per = (k + WIDE_PREP_NT - 1) / WIDE_PREP_NT, i0 = min(k, tid * per), i1 = min(k, i0 + per);
  int mine = 0;
  for (int i = i0; i < i1; ++i) mine += fin_kept(in.stat(0, i), in.stat(2, i)) ? 1 : 0;
  cnt[tid] = mine;
  __syncthreads();
  for (int o = 1; o < WIDE_PREP_NT; o <<= 1) {                // (inclusive prefix sum)
    const int v = tid >= o ? cnt[tid - o] : 0;
    __syncthreads();
    cnt[tid] += v;
    __syncthreads();
  }
  int at = cnt[tid] - mine;
  for (int i = i0; i < i1; ++i) {
    if (fin_kept(in.stat(0, i), in.stat(2, i))) ws.idx[at++] = i;
    else ws.scale[i] = 1.0;
  }
  if (tid == 0) ws.ic[WI_M] = cnt[WIDE_PREP_NT - 1];
}

// Step 1 of k_sets_spa: a thread per kept marker (64 to a workgroup; a workgroup with nothing to do returns)
__global__ __launch_bounds__(64) void k_swide_markers(WideIn in, int32_t c, const double* __restrict__ R, const double* __restrict__ u,
                                                      const double* __restrict__ spa, int32_t wmode, const double* __restrict__ weights,
                                                      SwideWs ws) {
  const int a = blockIdx.x * 64 + threadIdx.x, k = in.k;
  if (a >= ws.ic[WI_M]) return;
  const int col = ws.idx[a];
  const double uz = fin_forward(c, R, u, [&](int r) { return in.stat(4 + r, col); }, ws.Z, (int64_t)k, a);
  double zz = 0.0;
  for (int l = 0; l < c; ++l) zz = fma(ws.Z[(int64_t)l * k + a], ws.Z[(int64_t)l * k + a], zz);
  const double s = in.stat(4 + c, col) - uz;
  const double aj = in.xtx(col, col) - zz;                    // K_jj, as the pairs' kernel forms it
  const double x = sspa_chi2(swide_spa(in, spa, SPA_ROWS - 1, col), swide_spa(in, spa, 0, col));
  const double rho = x == x && aj > 0.0 ? sqrt(s * s / aj / x) : 1.0;   // rho^2 = zs^2 / x, zs^2 = s^2 / a
  ws.s[a] = s;
  ws.w[a] = fin_weight(wmode, in.stat(1, col), weights, col);
  ws.rho[a] = rho;
  ws.scale[col] = rho;
}

// Step 2, row a: sum_b w_a K_ab w_b and sum_b (w_a rho_a) K_ab (w_b rho_b), each thread in ascending b, folded by a fixed tree
__global__ __launch_bounds__(256) void k_swide_pairs(WideIn in, int32_t c, SwideWs ws) {
  __shared__ double red[256];
  const int tid = threadIdx.x, a = blockIdx.x, k = in.k;
  const int m = ws.ic[WI_M];
  if (a >= m) return;  // (the whole workgroup)
  const int i = ws.idx[a];
  const double wa = ws.w[a], ra = ws.rho[a];
  double pa = 0.0, pv = 0.0;
  for (int b = tid; b < m; b += 256) {
    const int j = ws.idx[b];
    double zz = 0.0;
    for (int l = 0; l < c; ++l) zz = fma(ws.Z[(int64_t)l * k + a], ws.Z[(int64_t)l * k + b], zz);
    const double kab = in.xtx(i, j) - zz, wb = ws.w[b];
    pa += wa * kab * wb;
    pv += (wa * ra) * kab * (wb * ws.rho[b]);
  }
  pa = fin_fold(pa, red, FinAdd{});
  pv = fin_fold(pv, red, FinAdd{});
  if (tid == 0) {
    ws.pa[a] = pa;
    ws.pv[a] = pv;
  }
}

// Steps 2 (the fold of the rows), 3 and 4.  mu, Cv, Minv, cutoff: as k_scan_spa takes them; gB: the collapsed row, overwritten
// with g^_B where the burden is attempted; bspa: SSPA_ROWLEN doubles; vscale: k.
__global__ __launch_bounds__(256) void k_swide_burden(WideIn in, int32_t n, int32_t c, const double* __restrict__ mu,
                                                      const double* __restrict__ Cv, const double* __restrict__ Minv, double cutoff,
                                                      SwideWs ws, double* gB, double* __restrict__ row, double* __restrict__ vscale) {
  __shared__ double red[4 * 3];
  __shared__ double tred[256];
  __shared__ double tt[SPA_CMAX + 1], gam[SPA_CMAX + 1], head[1];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, k = in.k;
  const SpaFold fold{red, lane, wv};
  const double nan = fin_nan();
  const int m = ws.ic[WI_M];
  if (m == 0) {
    for (int i = tid; i < k; i += 256) vscale[i] = 1.0;
    if (tid == 0) {
      for (int i = 0; i < SSPA_ROWLEN; ++i) row[i] = nan;
      row[6] = 0.0;
      row[12] = 0.0;
    }
    return;  // (the whole workgroup)
  }

  // 2. the rows' partials, a thread in ascending a, and b_B = w's the same way; the adjusted markers counted beside them
  double aB = 0.0, vq = 0.0, bB = 0.0, nadj = 0.0, z0 = 0.0, z1 = 0.0;
  for (int a = tid; a < m; a += 256) {
    aB += ws.pa[a];
    vq += ws.pv[a];
    bB += ws.w[a] * ws.s[a];
    nadj += ws.rho[a] != 1.0 ? 1.0 : 0.0;                     // (a sum of small integers: exact in any order)
  }
  fold(aB, vq, bB);
  fold(nadj, z0, z1);
  const double zsB = bB / sqrt(aB);
  const bool attempt = aB > 0.0 && fabs(zsB) > cutoff;

  // 3. the saddlepoint steps on the collapsed row, in place (a thread reads its own entry back before it writes it)
  SpaRoots o{nan, nan, nan, nan, nan, nan, 0, false};
  if (attempt) o = spa_roots(n, c, [&](int64_t i) { return gB[i]; }, aB, bB, mu, Cv, Minv, gB, tred, tt, gam, fold);

  // 4. the burden floor, the scales and the set's row
  if (tid == 0) {
    const double lp = attempt ? spa_log_p(o, zsB) : nan;
    const double flag = attempt ? (o.good ? 1.0 : 2.0) : 0.0;
    const double xB = sspa_chi2(flag, lp);
    const double vB = xB == xB ? bB * bB / xB : nan;
    const double phi = vB > vq && vq > 0.0 ? vB / vq : 1.0;  // (a NaN fails the comparison: never below 1)
    head[0] = sqrt(phi);
    row[0] = lp;
    row[1] = o.aw;
    row[2] = o.s;
    row[3] = o.zeta_hi;
    row[4] = o.zeta_lo;
    row[5] = attempt ? (double)o.iters : nan;
    row[6] = flag;
    row[7] = aB;
    row[8] = bB;
    row[9] = vB;
    row[10] = vq;
    row[11] = phi;
    row[12] = nadj;
  }
  __syncthreads();
  for (int i = tid; i < k; i += 256) vscale[i] = fin_kept(in.stat(0, i), in.stat(2, i)) ? ws.scale[i] * head[0] : 1.0;
}

}  // namespace scilmm
