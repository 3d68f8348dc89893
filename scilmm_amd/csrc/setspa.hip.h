// Kernel of the variant-set tests for binary traits (scilmm_sets_spa_dev and its two siblings, engine.hip): behind a Gram block
// and the saddlepoint call of its markers, every set of the block gets the variance scales of its markers and the saddlepoint
// p-value of its burden, the collapsed (weighted-sum) genotype (SAIGE-GENE / SMMAT).
//   k_sets_spa<Reader> : one workgroup per set, 256 threads            reads  the set's columns of the statistics and of the
//                        marker SPA rows, its k x k sub-block of the Gram matrix, its k marker rows once; then what
//                        k_scan_spa reads for one row (spa.hip.h)
// The steps, each between barriers that every thread reaches (every branch around a barrier is on a value all threads read from
// LDS or hold as the same folded bits):
//   0. the markers with an observed value and with variation are kept (k of the set's m), as k_sets_finish keeps them;
//   1. a thread per kept marker: z = R^-T w(C)'x, s_j, the weight w_j (the three modes of k_sets_finish), a_j = K_jj, and the
//      variance scale rho_j from the marker's SPA row: rho_j^2 = zs_j^2 / x_j, x_j the squared two-sided normal deviate of log p_j;
//   2. a_B = w'Kw, V_Q = (w o rho)'K(w o rho) and b_B = w's: the pairs (i, j) dealt to the threads at a fixed stride, each
//      K_ij = (G_ij + G_ji) / 2 - z_i'z_j formed as the finish forms it; no k x k image is stored;
//   3. where a_B > 0 and |b_B| / sqrt(a_B) > cutoff: the collapsed genotype sum_j w_j g~_j into the set's scratch row, then steps
//      1 - 3 of k_scan_spa on it (spa_roots) with (a, b) = (a_B, b_B);
//   4. x_B from log p_B, v~_B = b_B^2 / x_B, the burden floor phi = max(1, v~_B / V_Q), the scales rho_j sqrt(phi) of the set's
//      columns (1 for a dropped one) and the set's row.
// No atomics; every sum is taken in a fixed order and folded by a fixed tree: a set's numbers depend on its own inputs alone, not
// on its place in the block, its neighbours or the mode of the handle, and the three input forms of the same hard calls give the
// same bits (the readers of spa.hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "plan_types.h"
#include "setmath.hip.h"
#include "spa.hip.h"

namespace scilmm {

// a set's row: log_p_B | a_w | s_B | zeta_hi | zeta_lo | iters | flag | a_B | b_B | v~_B (NaN: none) | V_Q | phi | n_adj
constexpr int SSPA_ROWLEN = 13;
constexpr int SSPA_ITMAX = 100;     // steps of the deviate's root at most

struct SpaSets {
  int32_t start[RPMAX + 1];     // offsets of the sets into the block's columns
};

// log erfc(v / sqrt 2) for v >= 0: the logarithm of the two-sided normal tail, finite far beyond where the tail underflows
__device__ __forceinline__ double sspa_log_erfc(double v) {
  const double y = v * 0.70710678118654752440;
  return y < 0.5 ? log1p(-erf(y)) : log(erfcx(y)) - 0.5 * v * v;
}

// v >= 0 with log erfc(v / sqrt 2) = lp, for lp < 0: Newton inside a bracket from its upper end sqrt(-2 lp) (erfc(y) <= exp(-y^2));
// the function is decreasing and concave, so the steps come down to the root from above.  Infinite for lp = -inf.
__device__ double sspa_deviate(double lp) {
  if (!(lp > -INFINITY)) return INFINITY;
  double lo = 0.0, hi = sqrt(-2.0 * lp), v = hi;
  for (int it = 0; it < SSPA_ITMAX; ++it) {
    const double f = sspa_log_erfc(v) - lp;
    if (f > 0.0) lo = v; else hi = v;
    // d/dv log erfc(v / sqrt 2) = -sqrt(2 / pi) / erfcx(v / sqrt 2)
    double vn = v + f * erfcx(v * 0.70710678118654752440) * 1.25331413731550025121;
    if (!(vn > lo && vn < hi)) vn = 0.5 * (lo + hi);
    const double dv = fabs(vn - v);
    v = vn;
    if (dv <= 1e-15 * v) break;
  }
  return v;
}

// x = v^2 of a saddlepoint row (flag, log p), or NaN where the row gives none: the flag is not 1, log p is NaN or >= 0, or x is
// not finite and positive
__device__ __forceinline__ double sspa_chi2(double flag, double lp) {
  const double nan = fin_nan();
  if (!(flag == 1.0) || !(lp < 0.0)) return nan;
  const double v = sspa_deviate(lp), x = v * v;
  return x > 0.0 && x < INFINITY ? x : nan;
}

// stats, gram, R, u, wmode, weights: as k_sets_finish takes them; spa: the block's SPA_ROWS x r rows of k_scan_spa; mu, Cv, Minv,
// cutoff, gs: as k_scan_spa takes them (row `set` of gs is this set's).  bspa: n_sets rows of SSPA_ROWLEN doubles; vscale: r.
template <class Reader>
__global__ __launch_bounds__(256) void k_sets_spa(int32_t n, int32_t r, int32_t c, Reader rd, const double* __restrict__ stats,
                                                  const double* __restrict__ gram, const double* __restrict__ R,
                                                  const double* __restrict__ u, const double* __restrict__ mu,
                                                  const double* __restrict__ Cv, const double* __restrict__ Minv, double cutoff,
                                                  const double* __restrict__ spa, SpaSets sets, int32_t wmode,
                                                  const double* __restrict__ weights, double* gs, double* __restrict__ bspa,
                                                  double* __restrict__ vscale) {
  __shared__ double Z[SPA_CMAX * RPMAX];        // z of the kept markers, c x RPMAX
  __shared__ double sv[RPMAX], wv_[RPMAX], rv[RPMAX], mv[RPMAX];   // s | w | rho | mean
  __shared__ int32_t idx[RPMAX], slot[RPMAX];   // the kept markers' columns; a set column's place among them, or -1
  __shared__ double red[4 * 3];
  __shared__ double tred[256];
  __shared__ double tt[SPA_CMAX + 1], gam[SPA_CMAX + 1], head[4];
  __shared__ int32_t ic[2];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int set = blockIdx.x;
  const int c0 = sets.start[set], m = sets.start[set + 1] - c0;
  const SpaFold fold{red, lane, wv};
  const double nan = fin_nan();
  double* row = bspa + (int64_t)set * SSPA_ROWLEN;

  // 0. the kept markers
  if (tid == 0) {
    int k = 0;
    for (int j = 0; j < m; ++j) {
      const bool keep = fin_kept(stats[c0 + j], stats[2 * (int64_t)r + c0 + j]);
      slot[j] = keep ? k : -1;
      if (keep) idx[k++] = c0 + j;
    }
    ic[0] = k;
  }
  __syncthreads();
  const int k = ic[0];
  if (k == 0) {
    if (tid < m) vscale[c0 + tid] = 1.0;
    if (tid == 0) {
      for (int i = 0; i < SSPA_ROWLEN; ++i) row[i] = nan;
      row[6] = 0.0;
      row[12] = 0.0;
    }
    return;  // (the whole workgroup)
  }

  // 1. z, s, w, a and rho: a thread per kept marker
  if (tid < k) {
    const int col = idx[tid];
    const double uz = fin_forward(c, R, u, [&](int a) { return stats[(int64_t)(4 + a) * r + col]; }, Z, RPMAX, tid);
    double zz = 0.0;
    for (int l = 0; l < c; ++l) zz = fma(Z[l * RPMAX + tid], Z[l * RPMAX + tid], zz);
    const double s = stats[(int64_t)(4 + c) * r + col] - uz;
    const double mean = stats[(int64_t)r + col];
    const double a = gram[(int64_t)col * r + col] - zz;      // K_jj, as the pairs' loop forms it
    const double x = sspa_chi2(spa[(int64_t)(SPA_ROWS - 1) * r + col], spa[col]);
    sv[tid] = s;
    wv_[tid] = fin_weight(wmode, mean, weights, col);
    mv[tid] = mean;
    rv[tid] = x == x && a > 0.0 ? sqrt(s * s / a / x) : 1.0;  // rho^2 = zs^2 / x, zs^2 = s^2 / a
  }
  __syncthreads();

  // 2. a_B = w'Kw, V_Q = (w o rho)'K(w o rho), b_B = w's
  double aB = 0.0, vq = 0.0, bB = tid < k ? wv_[tid] * sv[tid] : 0.0;
  for (int at = tid; at < k * k; at += 256) {
    const int i = at / k, j = at - i * k;
    double zz = 0.0;
    for (int l = 0; l < c; ++l) zz = fma(Z[l * RPMAX + i], Z[l * RPMAX + j], zz);
    const double kij = fin_kernel_entry(gram[(int64_t)idx[i] * r + idx[j]], gram[(int64_t)idx[j] * r + idx[i]], zz);
    aB += wv_[i] * kij * wv_[j];
    vq += (wv_[i] * rv[i]) * kij * (wv_[j] * rv[j]);
  }
  fold(aB, vq, bB);
  const double zsB = bB / sqrt(aB);
  const bool attempt = aB > 0.0 && fabs(zsB) > cutoff;

  // 3. the collapsed genotype into the set's scratch row (a thread's own entries), then the saddlepoint steps on that row
  SpaRoots o{nan, nan, nan, nan, nan, nan, 0, false};
  if (attempt) {
    double* g = gs + (int64_t)set * n;
    for (int64_t i = tid; i < n; i += 256) {
      double acc = 0.0;
      for (int j = 0; j < k; ++j) acc = fma(wv_[j], rd(idx[j], i, mv[j]), acc);
      g[i] = acc;
    }
    __syncthreads();   // (step 1 of spa_roots reads the row across the threads)
    o = spa_roots(n, c, [&](int64_t i) { return g[i]; }, aB, bB, mu, Cv, Minv, g, tred, tt, gam, fold);
  }

  // 4. the burden floor, the scales and the set's row
  if (tid == 0) {
    const double lp = attempt ? spa_log_p(o, zsB) : nan;
    const double flag = attempt ? (o.good ? 1.0 : 2.0) : 0.0;
    const double xB = sspa_chi2(flag, lp);
    const double vB = xB == xB ? bB * bB / xB : nan;
    const double phi = vB > vq && vq > 0.0 ? vB / vq : 1.0;  // (a NaN fails the comparison: never below 1)
    int nadj = 0;
    for (int j = 0; j < k; ++j) nadj += rv[j] != 1.0 ? 1 : 0;
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
    row[12] = (double)nadj;
  }
  __syncthreads();
  if (tid < m) vscale[c0 + tid] = slot[tid] >= 0 ? rv[slot[tid]] * head[0] : 1.0;
}

}  // namespace scilmm
