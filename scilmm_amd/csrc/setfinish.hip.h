// Kernel of the variant-set finish (scilmm_sets_finish_dev, engine.hip): everything after a Gram block -- the projection of the
// covariates, the weights, the burden numbers, SKAT and SKAT-O -- for the sets of one block, from the block's statistics and its
// Gram matrix where the block left them.
//   k_sets_finish : one workgroup per set, 256 threads (512 where the block's largest set has more than 64 markers), everything
//                   of the set in LDS (dynamic, sized by the block's largest set: 146 KiB at 128 markers, 13 KiB at 16)
// The steps, each between barriers that every thread reaches (every branch around a barrier is on a value all threads read from LDS):
//   0. the markers with an observed value and with variation are kept (k of the set's m);
//   1. z = R^-T w(C)'x by forward substitution (a thread per marker), s = w(y)'x - u'z, the weights, t = w o s;
//   2. A = diag(w) (G_SS - z'z) diag(w) (every thread forms its entries in registers, then the image of z is overwritten); with
//      variance scales (scilmm_sets_finish_scaled_dev) diag(w o scale) takes the place of diag(w), in A alone;
//   3. the burden numbers and Q = t't;
//   4. A = U Lambda U' by the two-sided Jacobi iteration, disjoint pairs in round-robin order, with c = U'1 carried through the
//      rotations; Lambda sorted in descending order;
//   5. per grid value rho: the eigenvalues of A R_rho are those of (1 - rho) Lambda + rho v v', v = Lambda^1/2 c; the eigenvalues
//      of B = A - a a' / s11 those of Lambda - (Lambda c)(Lambda c)' / (c' Lambda c): diagonal plus rank one, roots of the secular
//      equation 1 + sum_l w_l / (d_l - mu) = 0 between the poles, after equal poles are merged and zero weights taken out
//      (a thread per task for that, then a thread per root: bracketed Newton in the distance from the lower pole);
//   6. the tails (a lane per task, the tasks dealt to the waves in turn): saddlepoint with its seam or modified Liu, the chi-square
//      quantiles by Newton from a Wilson-Hilferty start, all on one regularised incomplete gamma function;
//   7. the SKAT-O integral: break points sorted in LDS, a piece per 32 lanes with a Gauss-Legendre node each, the tail in closed form.
// No atomics; every sum is taken in a fixed order and folded by a fixed tree: a set's numbers depend on its own inputs alone, not
// on its place in the block, its neighbours or the mode of the handle.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "plan_types.h"

namespace scilmm {

constexpr int FIN_HEAD = 10;        // doubles of a set's row before its per-rho p-values
constexpr int FIN_RHO_MAX = 16;     // grid values at most
constexpr int FIN_CMAX = 31;        // covariates at most (SCAN_QMAX - 1)
constexpr int FIN_NT_MAX = 512;     // threads of a workgroup at most
constexpr int FIN_GL = 32;          // Gauss-Legendre nodes per piece of the integral
constexpr int FIN_SWEEPS = 40;      // Jacobi sweeps at most
constexpr int FIN_ITMAX = 200;      // steps of a root at most
constexpr int FIN_ENTRIES = 32;     // entries of A a thread forms at most (128 * 128 / 512, 64 * 64 / 256)
constexpr double FIN_FLOOR = 1e-10;    // eigenvalues below this fraction of the largest are dropped from a mixture
constexpr double FIN_SEAM = 0.05;      // the saddlepoint seam, in standard deviations
constexpr double FIN_RHO_CAP = 0.999;  // a grid value above it is computed as it
constexpr double FIN_Z_END = 40.0;     // the integral stops here
enum { FIN_BETA = 0, FIN_ONES = 1, FIN_GIVEN = 2 };         // weight modes
enum { FIN_SADDLE = 0, FIN_LIU = 1 };                       // tail methods
// the flag word: bit 0 the degenerate rule answered (p = T); bit 1 the Jacobi iteration ran out of sweeps; bit 2 a root
// (secular equation, saddlepoint, quantile) ran out of steps; bit 3 SKAT-O was asked for and computed; bit 4 a kept column's
// variance scale is not 1 (scilmm_sets_finish_scaled_dev)
enum { FIN_F_DEGENERATE = 1, FIN_F_SWEEPS = 2, FIN_F_ROOT = 4, FIN_F_SKATO = 8, FIN_F_SCALED = 16 };

struct FinSets {
  int32_t start[RPMAX + 1];     // offsets of the sets into the block's columns
  double rho[FIN_RHO_MAX];
};

__device__ const double FIN_GL_X[FIN_GL / 2] = {
    4.83076656877383104e-02, 1.44471961582796488e-01, 2.39287362252137065e-01, 3.31868602282127667e-01,
    4.21351276130635333e-01, 5.06899908932229359e-01, 5.87715757240762304e-01, 6.63044266930215231e-01,
    7.32182118740289711e-01, 7.94483795967942386e-01, 8.49367613732569970e-01, 8.96321155766052202e-01,
    9.34906075937739667e-01, 9.64762255587506390e-01, 9.85611511545268382e-01, 9.97263861849481570e-01};
__device__ const double FIN_GL_W[FIN_GL / 2] = {
    9.65400885147278121e-02, 9.56387200792748332e-02, 9.38443990808045664e-02, 9.11738786957638631e-02,
    8.76520930044039082e-02, 8.33119242269468457e-02, 7.81938957870703111e-02, 7.23457941088484491e-02,
    6.58222227763617523e-02, 5.86840934785357038e-02, 5.09980592623762441e-02, 4.28358980222264263e-02,
    3.42738629130216257e-02, 2.53920653092624266e-02, 1.62743947309059653e-02, 7.01861000946929839e-03};

// ---- special functions (a thread each) ----

// the regularised upper incomplete gamma function Q(a, x), a > 0: the series of P below a + 1, the continued fraction of Q
// (modified Lentz) above; relative accuracy in the upper tail
__device__ double fin_gamma_q(double a, double x) {
  if (!(x > 0.0)) return 1.0;
  const double pre = exp(a * log(x) - x - lgamma(a));    // x^a e^-x / Gamma(a)
  if (x < a + 1.0) {
    double ap = a, del = 1.0 / a, sum = del;
    for (int n = 0; n < 10000; ++n) {
      ap += 1.0;
      del *= x / ap;
      sum += del;
      if (fabs(del) <= fabs(sum) * 1e-17) break;
    }
    return 1.0 - sum * pre;
  }
  const double tiny = 1e-300;
  double b = x + 1.0 - a, c = 1.0 / tiny, d = 1.0 / b, h = d;
  for (int i = 1; i < 10000; ++i) {
    const double an = -(double)i * ((double)i - a);
    b += 2.0;
    d = an * d + b;
    if (fabs(d) < tiny) d = tiny;
    c = b + an / c;
    if (fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    const double del = d * c;
    h *= del;
    if (fabs(del - 1.0) <= 1e-16) break;
  }
  return pre * h;
}

__device__ __forceinline__ double fin_chi2_sf(double x, double df) { return x > 0.0 ? fin_gamma_q(0.5 * df, 0.5 * x) : 1.0; }
__device__ __forceinline__ double fin_norm_sf(double x) { return 0.5 * erfc(x * 0.70710678118654752440); }

// x with chi2_df's upper tail at x equal to p (0 < p < 1): Newton on the logarithm of the tail from a Wilson-Hilferty start,
// inside a bracket that every step tightens
__device__ double fin_chi2_isf(double p, double df, bool& ok) {
  ok = true;
  if (p >= 1.0) return 0.0;                                  // (a Liu tail is exactly 1 for a small Q)
  const double a = 0.5 * df, lg = lgamma(a), lp = log(p);
  const double z = -normcdfinv(p), v = 2.0 / (9.0 * df);
  double w = 1.0 - v + z * sqrt(v);
  double x = df * w * w * w;
  if (!(x > 0.0) || w <= 0.0) x = 0.01 * df;                 // (far in the lower tail: the bracket takes over)
  double lo = 0.0, hi = INFINITY;
  ok = false;
  for (int it = 0; it < FIN_ITMAX; ++it) {
    const double q = fin_gamma_q(a, 0.5 * x);
    const double f = log(q) - lp;                           // decreasing in x
    if (f > 0.0) lo = x; else hi = x;
    const double dens = 0.5 * exp((a - 1.0) * log(0.5 * x) - 0.5 * x - lg);
    double xn = x + f * q / dens;
    if (!(xn > lo && xn < hi)) xn = hi < INFINITY ? 0.5 * (lo + hi) : 2.0 * x;
    const double dx = fabs(xn - x);
    x = xn;
    if (dx <= 1e-14 * x) {
      ok = true;
      break;
    }
  }
  return x;
}

// the modified Liu matching of sum lam_i chi2_1 (mean c1, variance 2 c2; scale a, degrees of freedom l).  Every spectrum here is
// positive, so c3^2 <= c2 c4 (Cauchy-Schwarz) and the host form's branch that matches the skewness as well, with a non-central
// chi-square, is never taken: the kurtosis is matched, l = c2^2 / c4, and the tail is a central chi-square's.
struct FinLiu {
  double c1, c2, a, l;
};

__device__ FinLiu fin_liu_params(const double* lam, int n) {
  double c1 = 0.0, c2 = 0.0, c4 = 0.0;
  for (int i = 0; i < n; ++i) {
    const double v = lam[i], v2 = v * v;
    c1 += v;
    c2 += v2;
    c4 += v2 * v2;
  }
  FinLiu p{c1, c2, 0.0, c2 * c2 / c4};
  p.a = sqrt(p.l);
  return p;
}

__device__ double fin_liu_sf(double q, const FinLiu& p) {
  const double x = (q - p.c1) / sqrt(2.0 * p.c2) * (1.41421356237309504880 * p.a) + p.l;
  return fin_chi2_sf(x, p.l);
}

// Lugannani-Rice for q > 0 away from the mean: K'(t) = sum lam / (1 - 2 lam t) = q by Newton from 0 inside the bracket of the
// host form (scilmm_amd.sets._lugannani_rice), a step that leaves it replaced by its midpoint
__device__ double fin_lugannani_rice(double q, const double* lam, int n, double mu, double lmax, bool& ok) {
  const double pole = 0.5 / lmax;
  auto k1 = [&](double t, double& k2) {
    double f = 0.0;
    k2 = 0.0;
    for (int i = 0; i < n; ++i) {
      const double r = lam[i] / (1.0 - 2.0 * lam[i] * t);
      f += r;
      k2 += r * r;
    }
    k2 *= 2.0;
    return f - q;
  };
  double lo, hi, k2;
  if (q > mu) {
    lo = 0.0;
    hi = pole * (1.0 - fmin(0.5, lmax / (2.0 * q)));
  } else {
    lo = -pole;
    hi = 0.0;
    for (int g = 0; g < 1100 && k1(lo, k2) > 0.0; ++g) lo *= 2.0;
  }
  double t = 0.0;
  ok = false;
  for (int it = 0; it < FIN_ITMAX; ++it) {
    const double f = k1(t, k2);
    if (f < 0.0) lo = t; else hi = t;
    double tn = t - f / k2;
    if (!(tn > lo && tn < hi)) tn = 0.5 * (lo + hi);
    const double dt = fabs(tn - t);
    t = tn;
    if (dt <= 1e-15 * pole + 4e-16 * fabs(t)) {
      ok = true;
      break;
    }
  }
  double K0 = 0.0;
  k2 = 0.0;
  for (int i = 0; i < n; ++i) {
    const double den = 1.0 - 2.0 * lam[i] * t, r = lam[i] / den;
    K0 += log1p(-2.0 * lam[i] * t);
    k2 += r * r;
  }
  K0 *= -0.5;
  k2 *= 2.0;
  const double w = copysign(sqrt(2.0 * (t * q - K0)), t), v = t * sqrt(k2);
  return fin_norm_sf(w + log(v / w) / w);
}

// P(sum lam_i chi2_1 > q) for the n positive lam (the floor applied), by `method`; the seam as on the host
__device__ double fin_mixture_sf(double q, const double* lam, int n, const FinLiu& liu, int method, bool& ok) {
  ok = true;
  if (method == FIN_LIU) return fin_liu_sf(q, liu);
  if (q <= 0.0) return 1.0;
  double lmax = 0.0;
  for (int i = 0; i < n; ++i) lmax = fmax(lmax, lam[i]);
  const double mu = liu.c1, sd = sqrt(2.0 * liu.c2);
  if (fabs(q - mu) >= FIN_SEAM * sd) return fin_lugannani_rice(q, lam, n, mu, lmax, ok);
  const double lo = mu - FIN_SEAM * sd, hi = mu + FIN_SEAM * sd;
  bool ok1, ok2;
  const double c_lo = fin_lugannani_rice(lo, lam, n, mu, lmax, ok1) / fin_liu_sf(lo, liu);
  const double c_hi = fin_lugannani_rice(hi, lam, n, mu, lmax, ok2) / fin_liu_sf(hi, liu);
  ok = ok1 && ok2;
  return fin_liu_sf(q, liu) * (c_lo + (c_hi - c_lo) * (q - lo) / (hi - lo));
}

// root number i of 1 + sum_l w_l / (d_l - mu) = 0 for the poles d_0 > d_1 > ... > d_{m-1} and weights w_l > 0: it lies in
// (d_i, d_{i-1}), root 0 in (d_0, d_0 + sum w].  Solved in eta = mu - d_i (no cancellation next to the lower pole).
__device__ double fin_secular_root(const double* d, const double* w, int m, int i, double wsum, double scale, bool& ok) {
  ok = true;
  if (m == 1) return d[0] + w[0];
  const double org = d[i];
  double lo = 0.0, hi = i == 0 ? wsum : d[i - 1] - org;
  double eta = 0.5 * (lo + hi);
  ok = false;
  for (int it = 0; it < FIN_ITMAX; ++it) {
    double f = 1.0, fp = 0.0;
    for (int l = 0; l < m; ++l) {
      const double inv = 1.0 / ((d[l] - org) - eta), qv = w[l] * inv;
      f += qv;
      fp = fma(qv, inv, fp);
    }
    if (f > 0.0) hi = eta; else lo = eta;                   // (f increases with eta)
    double en = eta - f / fp;
    if (!(en > lo && en < hi)) en = 0.5 * (lo + hi);
    const double de = fabs(en - eta);
    eta = en;
    if (de <= 1e-15 * eta + 1e-20 * scale || hi - lo <= 1e-20 * scale) {
      ok = true;
      break;
    }
  }
  return org + eta;
}

// the workgroup's values folded by a fixed tree; every thread gets the result (red: blockDim.x doubles, reusable at once)
__device__ __forceinline__ double fin_fold(double v, double* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int s = blockDim.x >> 1; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  const double out = red[0];
  __syncthreads();
  return out;
}

// a marker's weight by the mode: the Beta(1, 25) density at its minor allele frequency (half its mean), 1, or the caller's
__device__ __forceinline__ double fin_weight(int32_t wmode, double mean, const double* __restrict__ weights, int col) {
  if (wmode == FIN_BETA) {
    const double maf = fmin(0.5 * mean, 1.0 - 0.5 * mean), x = 1.0 - maf;
    const double x2 = x * x, x4 = x2 * x2, x8 = x4 * x4;
    return 25.0 * (x8 * x8 * x8);                            // 25 (1 - maf)^24
  }
  return wmode == FIN_GIVEN ? weights[col] : 1.0;
}

// doubles of dynamic LDS for a block whose largest set has `cap` markers (cap even, >= 2): the matrix image (or the image of z, or
// the secular work space: three rows of cap per task), nine vectors, the fold, the pairs' rotations, the per-rho numbers and the
// break points, the kept markers' columns and the pairs' indices (int32, two to a double)
__host__ __device__ constexpr int fin_image(int cap) {
  const int a = cap * (cap + 1), z = FIN_CMAX * cap, s = 3 * (FIN_RHO_MAX + 1) * cap;
  return a > z ? (a > s ? a : s) : (z > s ? z : s);
}
__host__ __device__ constexpr int fin_lds_doubles(int cap, int nt) {
  return fin_image(cap) + 9 * cap + nt + cap + 8 * FIN_RHO_MAX + 64 + 2 * 128 + (cap + cap + 64) / 2 + 8;
}

// stats: the block's (q + 4) x r statistics, q = c + 1; gram: r x r; R: c x c upper; u: c; sets: the offsets and the grid, by
// value; out: n_sets rows of ld_out >= FIN_HEAD + n_rho doubles; lam_out: r doubles or null; vscale: r variance scales of the
// columns or null (all 1).  cap: the largest set, rounded up to an even number.
__global__ __launch_bounds__(FIN_NT_MAX) void k_sets_finish(int32_t r, int32_t c, const double* __restrict__ stats,
                                                            const double* __restrict__ gram, const double* __restrict__ R,
                                                            const double* __restrict__ u, FinSets sets, int32_t wmode,
                                                            const double* __restrict__ weights, int32_t method, int32_t n_rho,
                                                            int32_t cap, double* __restrict__ out, int64_t ld_out,
                                                            double* __restrict__ lam_out, const double* __restrict__ vscale) {
  extern __shared__ double fin_lds[];
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wv = tid >> 6, nw = nt >> 6;
  const int set = blockIdx.x;
  const int c0 = sets.start[set], m = sets.start[set + 1] - c0;
  const int ld = cap + 1;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);

  double* M = fin_lds;                         // the matrix, ld = cap + 1 (odd: a column is read without bank conflicts)
  double* sv = M + fin_image(cap);             // s | w | t | lambda (sorted) | c = U'1 (sorted) | c (unsorted) | lambda above the floor | w o scale | 1 spare
  double *wv_ = sv + cap, *tv = wv_ + cap, *lam = tv + cap, *cs = lam + cap, *cu = cs + cap, *lamf = cu + cap, *wa = lamf + cap;
  double* red = sv + 9 * cap;                  // nt
  double* rot = red + nt;                      // cos | sin of the pairs of a step (cap / 2 each)
  double* prho = rot + cap;                    // p_rho | Q_rho | c1 | sd | l | alpha | beta | spare (FIN_RHO_MAX each)
  double *qrho = prho + FIN_RHO_MAX, *lc1 = qrho + FIN_RHO_MAX, *lsd = lc1 + FIN_RHO_MAX, *ll = lsd + FIN_RHO_MAX;
  double *al = ll + FIN_RHO_MAX, *be = al + FIN_RHO_MAX;
  double* sc = prho + 8 * FIN_RHO_MAX;         // 64 scalars
  double* fm = sc + 40;                        // a root that ran out of steps: SKAT's tail | the grid values' (marks, 0 or 1)
  double* pts = sc + 64;                       // break points, unsorted | sorted (128 each)
  double* spts = pts + 128;
  int32_t* idx = (int32_t*)(spts + 128);       // the kept markers' columns of the block (cap)
  int32_t* pp = idx + cap;                     // the pairs' indices (cap / 2 each)
  int32_t* pq = pp + cap / 2;
  int32_t* ic = pq + cap / 2;                  // 64 integers: counts per task, flags
  enum { S_WS = 0, S_TT, S_S11, S_TR, S_SKATP, S_T, S_MU, S_SD, S_DF, S_Z0, S_END, S_LEVEL, S_AA, S_S11E, S_ABA };
  enum { I_K = 0, I_ROT, I_FLAG, I_J0, I_DEG, I_ROOT, I_NSKAT, I_NB, I_CNT = 8, I_M = 8 + FIN_RHO_MAX + 1, I_NDEF = 8 + 2 * (FIN_RHO_MAX + 1) };

  double* row = out + (int64_t)set * ld_out;

  // 0. the kept markers
  if (tid == 0) {
    int k = 0, scaled = 0;
    for (int j = 0; j < m; ++j) {
      const double n_obs = stats[c0 + j], css = stats[2 * (int64_t)r + c0 + j];
      if (!(n_obs == 0.0 || css == 0.0)) {
        idx[k++] = c0 + j;
        if (vscale && vscale[c0 + j] != 1.0) scaled = FIN_F_SCALED;
      }
    }
    ic[I_K] = k;
    ic[I_FLAG] = scaled;
    ic[I_ROOT] = 0;
    for (int j = 0; j < FIN_RHO_MAX + 2; ++j) fm[j] = 0.0;
  }
  __syncthreads();
  const int k = ic[I_K];
  if (lam_out && tid < m) lam_out[c0 + tid] = nan;          // (the kept markers' slots are written again in step 4)
  if (k == 0) {
    if (tid == 0) {
      row[0] = 0.0;
      for (int i = 1; i < FIN_HEAD - 1; ++i) row[i] = nan;
      row[FIN_HEAD - 1] = 0.0;
      for (int j = 0; j < n_rho; ++j) row[FIN_HEAD + j] = nan;
    }
    return;  // (the whole workgroup)
  }

  // 1. z, s, w, t: a thread per kept marker; the image of z is c x cap in M
  if (tid < k) {
    const int col = idx[tid];
    double uz = 0.0;
    for (int a = 0; a < c; ++a) {
      double v = stats[(int64_t)(4 + a) * r + col];
      for (int l = 0; l < a; ++l) v -= R[l * c + a] * M[l * cap + tid];
      v /= R[a * c + a];
      M[a * cap + tid] = v;
      uz += u[a] * v;
    }
    const double s = stats[(int64_t)(4 + c) * r + col] - uz;
    const double w = fin_weight(wmode, stats[(int64_t)r + col], weights, col);
    sv[tid] = s;
    wv_[tid] = w;
    wa[tid] = vscale ? w * vscale[col] : w;                   // (the weight in A alone: t keeps w)
    tv[tid] = w * s;
    cu[tid] = 1.0;
  }
  __syncthreads();

  // 2. A = diag(w) (G - z'z) diag(w): the entries in registers, then over the image of z
  double acc[FIN_ENTRIES];
#pragma unroll
  for (int e = 0; e < FIN_ENTRIES; ++e) {
    const int at = tid + e * nt;
    acc[e] = 0.0;
    if (at < k * k) {
      const int i = at / k, j = at - i * k;
      double zz = 0.0;
      for (int l = 0; l < c; ++l) zz = fma(M[l * cap + i], M[l * cap + j], zz);
      const double kij = 0.5 * (gram[(int64_t)idx[i] * r + idx[j]] + gram[(int64_t)idx[j] * r + idx[i]]) - zz;   // (the host's 0.5 (K + K'))
      acc[e] = wa[i] * kij * wa[j];
    }
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < FIN_ENTRIES; ++e) {
    const int at = tid + e * nt;
    if (at < k * k) {
      const int i = at / k, j = at - i * k;
      M[i * ld + j] = acc[e];
    }
  }
  __syncthreads();

  // 3. the burden numbers and Q
  {
    double rs = 0.0;
    if (tid < k)
      for (int j = 0; j < k; ++j) rs += M[tid * ld + j];
    const double s11 = fin_fold(rs, red);                     // w'Kw = 1'A1
    const double ws = fin_fold(tid < k ? tv[tid] : 0.0, red);
    const double tt = fin_fold(tid < k ? tv[tid] * tv[tid] : 0.0, red);
    const double tr = fin_fold(tid < k ? M[tid * ld + tid] : 0.0, red);
    if (tid == 0) {
      sc[S_WS] = ws;
      sc[S_TT] = tt;
      sc[S_S11] = s11;
      sc[S_TR] = tr;
      row[0] = (double)k;
      row[1] = ws / s11;
      row[2] = 1.0 / sqrt(s11);
      row[3] = ws * ws / s11;
      row[4] = tt;
    }
  }
  __syncthreads();
  const double ws = sc[S_WS], tt = sc[S_TT], tr = sc[S_TR];

  // 4. two-sided Jacobi: me - 1 steps of me / 2 disjoint pairs per sweep (round robin; me = k rounded up to even, a pair with
  // the index k is idle), until a sweep rotates nothing.  A rotation is skipped where |a_pq| <= 1e-18 trace.
  if (k > 1) {
    const int me = (k + 1) & ~1, half = me / 2;
    const double tol = 1e-18 * tr;
    bool done = false;
    for (int sweep = 0; sweep < FIN_SWEEPS && !done; ++sweep) {
      if (tid == 0) ic[I_ROT] = 0;
      __syncthreads();
      for (int step = 0; step < me - 1; ++step) {
        if (tid < half) {
          int p, q;
          if (tid == 0) {
            p = me - 1;
            q = step;
          } else {
            p = (step + tid) % (me - 1);
            q = (step + me - 1 - tid) % (me - 1);
          }
          if (p > q) {
            const int t = p;
            p = q;
            q = t;
          }
          double cv = 1.0, sn = 0.0;
          if (q < k) {
            const double apq = M[p * ld + q];
            if (fabs(apq) > tol) {
              const double th = (M[q * ld + q] - M[p * ld + p]) / (2.0 * apq);
              const double t = copysign(1.0, th) / (fabs(th) + sqrt(1.0 + th * th));
              cv = 1.0 / sqrt(1.0 + t * t);
              sn = t * cv;
              ic[I_ROT] = 1;                                  // (every writer stores the same value)
            }
          }
          rot[tid] = cv;
          rot[half + tid] = sn;
          pp[tid] = p;
          pq[tid] = q;
        }
        __syncthreads();
        // columns: (a_ip, a_iq) <- (c a_ip - s a_iq, s a_ip + c a_iq), the row index along the lanes; c = U'1 goes with them
        for (int at = tid; at < half * k; at += nt) {
          const int pr = at / k, i = at - pr * k;
          const double sn = rot[half + pr];
          if (sn != 0.0) {
            const double cv = rot[pr];
            const int p = pp[pr], q = pq[pr];
            const double x = M[i * ld + p], y = M[i * ld + q];
            M[i * ld + p] = cv * x - sn * y;
            M[i * ld + q] = sn * x + cv * y;
            if (i == 0) {
              const double a = cu[p], b = cu[q];
              cu[p] = cv * a - sn * b;
              cu[q] = sn * a + cv * b;
            }
          }
        }
        __syncthreads();
        // rows, the column index along the lanes; the rotated pair's own off-diagonal entries are set to zero
        for (int at = tid; at < half * k; at += nt) {
          const int pr = at / k, j = at - pr * k;
          const double sn = rot[half + pr];
          if (sn != 0.0) {
            const double cv = rot[pr];
            const int p = pp[pr], q = pq[pr];
            const double x = M[p * ld + j], y = M[q * ld + j];
            M[p * ld + j] = j == q ? 0.0 : cv * x - sn * y;
            M[q * ld + j] = j == p ? 0.0 : sn * x + cv * y;
          }
        }
        __syncthreads();
      }
      done = ic[I_ROT] == 0;
      __syncthreads();
    }
    if (!done && tid == 0) ic[I_FLAG] |= FIN_F_SWEEPS;
  }
  // the eigenvalues in descending order (ties in index order), c with them
  if (tid < k) {
    const double v = M[tid * ld + tid];
    int rank = 0;
    for (int j = 0; j < k; ++j) {
      const double o = M[j * ld + j];
      rank += (o > v || (o == v && j < tid)) ? 1 : 0;
    }
    lam[rank] = v;
    cs[rank] = cu[tid];
  }
  __syncthreads();
  if (lam_out && tid < k) lam_out[idx[tid]] = lam[tid];
  // the positive part (what the rank-one problems are built on), and the mixture of SKAT: the eigenvalues above the floor
  if (tid == 0) {
    int nf = 0;
    for (int i = 0; i < k; ++i)
      if (lam[i] > FIN_FLOOR * lam[0]) lamf[nf++] = lam[i];
    ic[I_NSKAT] = lam[0] > 0.0 ? nf : 0;
    double s11e = 0.0, aa = 0.0, a3 = 0.0;
    for (int i = 0; i < k; ++i) {
      const double l = fmax(lam[i], 0.0), lc2 = l * cs[i] * cs[i];
      s11e += lc2;
      aa += l * lc2;
      a3 += l * l * lc2;
    }
    sc[S_S11E] = s11e;                                        // 1'A1 in the eigenbasis
    sc[S_AA] = aa;                                            // a'a, a = A1
    sc[S_ABA] = fmax(a3 - aa * aa / s11e, 0.0);               // a'Ba
  }
  __syncthreads();
  const int nskat = ic[I_NSKAT];
  const double s11e = sc[S_S11E];
  const bool skato = n_rho > 0 && nskat > 0;
  // the remainder term exists where there is more than one marker and a'1 is not rounding
  const bool want_b = skato && k > 1 && s11e > FIN_FLOOR * tr;
  const int ntask = skato && k > 1 ? n_rho + (want_b ? 1 : 0) : 0;

  // 5a. per task (grid value j < n_rho; the remainder term j = n_rho) the reduced rank-one problem: poles in descending order
  // with positive weights, equal poles merged (one of them stays an eigenvalue), zero weights taken out.  Rows of the work
  // space over M: poles | weights | eigenvalues.
  double* work = M;
  if (tid < ntask) {
    const int j = tid;
    double *dd = work + (3 * j) * cap, *ww = dd + cap, *ev = ww + cap;
    const bool isb = j == n_rho;
    const double rho = isb ? 0.0 : fmin(sets.rho[j], FIN_RHO_CAP);
    auto pole = [&](int i) { return isb ? -fmax(lam[k - 1 - i], 0.0) : (1.0 - rho) * fmax(lam[i], 0.0); };
    auto wgt = [&](int i) {
      if (isb) {
        const double lc = fmax(lam[k - 1 - i], 0.0) * cs[k - 1 - i];
        return lc * lc / s11e;
      }
      return rho * fmax(lam[i], 0.0) * cs[i] * cs[i];
    };
    double wsum = 0.0;
    for (int i = 0; i < k; ++i) wsum += wgt(i);
    const double scale = fmax(fabs(pole(0)), fabs(pole(k - 1))) + wsum;
    const double tolw = 1e-17 * scale, told = 1e-15 * scale;
    int mr = 0, nd = 0;
    double wred = 0.0;
    for (int i = 0; i < k; ++i) {
      const double di = pole(i), wi = wgt(i);
      if (!(wi > tolw)) {
        ev[nd++] = di;
      } else if (mr > 0 && dd[mr - 1] - di <= told) {
        ww[mr - 1] += wi;
        wred += wi;
        ev[nd++] = di;
      } else {
        dd[mr] = di;
        ww[mr] = wi;
        wred += wi;
        ++mr;
      }
    }
    ic[I_M + j] = mr;
    ic[I_NDEF + j] = nd;
    // (the sum of the reduced weights and the scale, for the roots' threads: behind the eigenvalues' row is no room, so in
    // the per-rho block: alpha and beta are not yet in use)
    if (isb) {
      sc[32] = wred;
      sc[33] = scale;
    } else {
      al[j] = wred;
      be[j] = scale;
    }
  }
  __syncthreads();
  // 5b. a thread per root
  for (int at = tid; at < ntask * cap; at += nt) {
    const int j = at / cap, i = at - j * cap;
    const int mr = ic[I_M + j];
    if (i < mr) {
      const double *dd = work + (3 * j) * cap, *ww = dd + cap;
      double* ev = work + (3 * j + 2) * cap;
      const bool isb = j == n_rho;
      bool ok;
      ev[ic[I_NDEF + j] + i] = fin_secular_root(dd, ww, mr, i, isb ? sc[32] : al[j], isb ? sc[33] : be[j], ok);
      if (!ok) ic[I_ROOT] = 1;                                // (every writer stores the same value)
    }
  }
  __syncthreads();

  // 6. the tails: a lane per task, the tasks dealt to the waves in turn.  Task n_rho + 1 is SKAT's own p-value.
  for (int j = wv; j < FIN_RHO_MAX + 2; j += nw) {
    if (lane != 0) continue;
    if (j == FIN_RHO_MAX + 1) {
      double p = nan;
      if (nskat > 0) {
        const FinLiu liu = fin_liu_params(lamf, nskat);
        bool ok;
        p = fin_mixture_sf(tt, lamf, nskat, liu, method, ok);
        if (!ok) fm[0] = 1.0;
      }
      sc[S_SKATP] = p;
    } else if (j < ntask && j < n_rho) {
      double* ev = work + (3 * j + 2) * cap;
      double top = 0.0;
      for (int i = 0; i < k; ++i) top = fmax(top, ev[i]);
      int nf = 0;
      for (int i = 0; i < k; ++i) {
        const double v = ev[i];
        if (v > FIN_FLOOR * top) ev[nf++] = v;
      }
      const double rho = fmin(sets.rho[j], FIN_RHO_CAP);
      const double q = (1.0 - rho) * tt + rho * ws * ws;
      double p = nan;
      if (nf > 0) {
        const FinLiu liu = fin_liu_params(ev, nf);
        bool ok;
        p = fin_mixture_sf(q, ev, nf, liu, method, ok);
        if (!ok) fm[1 + j] = 1.0;
        lc1[j] = liu.c1;
        lsd[j] = sqrt(2.0 * liu.c2);
        ll[j] = liu.l;
      }
      prho[j] = p;
      qrho[j] = q;
    } else if (j < ntask && j == n_rho) {
      // the remainder term: the eigenvalues of B are minus the roots; those above the floor (none where the largest is rounding)
      double* ev = work + (3 * j + 2) * cap;
      double top = 0.0;
      for (int i = 0; i < k; ++i) {
        ev[i] = -ev[i];
        top = fmax(top, ev[i]);
      }
      double mu = 0.0, l2 = 0.0, l4 = 0.0;
      int nf = 0;
      if (top > FIN_FLOOR * tr)
        for (int i = 0; i < k; ++i) {
          const double v = ev[i];
          if (v > FIN_FLOOR * top) {
            ++nf;
            mu += v;
            l2 += v * v;
            l4 += (v * v) * (v * v);
          }
        }
      ic[I_NB] = nf;
      sc[S_MU] = mu;
      sc[S_SD] = sqrt(2.0 * l2 + 4.0 * sc[S_ABA] / s11e);
      sc[S_DF] = l2 * l2 / l4;
    }
  }
  __syncthreads();
  // T, its first minimiser, the degenerate rule
  if (tid == 0) {
    const double ps = sc[S_SKATP];
    row[5] = ps;
    int flag = ic[I_FLAG] | (ic[I_ROOT] ? FIN_F_ROOT : 0);
    for (int j = 0; j < 1 + FIN_RHO_MAX; ++j)
      if (fm[j] != 0.0) flag |= FIN_F_ROOT;
    int deg = 1;
    double T = nan;
    int j0 = 0;
    if (skato) {
      flag |= FIN_F_SKATO;
      if (k == 1) {
        for (int j = 0; j < n_rho; ++j) prho[j] = ps;          // one marker: every Q_rho is t^2
        T = ps;
      } else {
        bool any_nan = false;
        T = prho[0];
        for (int j = 0; j < n_rho; ++j) {
          any_nan = any_nan || !(prho[j] == prho[j]);
          if (prho[j] < T) {
            T = prho[j];
            j0 = j;
          }
        }
        if (any_nan) T = nan;
        deg = any_nan || !want_b || ic[I_NB] == 0 || !(T > 0.0);
      }
      if (deg) {
        // one marker, a'1 = 0 or B = 0: every p_rho is the same up to rounding, p = T and the first grid value stands for the
        // minimiser; T = 0 (underflow): so is p
        const bool same = k == 1 || !want_b || ic[I_NB] == 0;
        row[6] = T;
        row[7] = T;
        row[8] = T == T ? sets.rho[same ? 0 : j0] : nan;
        flag |= FIN_F_DEGENERATE;
      }
      for (int j = 0; j < n_rho; ++j) row[FIN_HEAD + j] = prho[j];
    } else {
      row[6] = row[7] = row[8] = nan;
      for (int j = 0; j < n_rho; ++j) row[FIN_HEAD + j] = nan;
    }
    sc[S_T] = T;
    ic[I_J0] = j0;
    ic[I_DEG] = skato ? deg : 1;
    ic[I_FLAG] = flag;
  }
  __syncthreads();
  if (ic[I_DEG]) {
    if (tid == 0) row[9] = (double)ic[I_FLAG];
    return;  // (the whole workgroup)
  }

  // 7. the quantiles q_min(rho) and the lines (alpha - beta x): a lane per grid value
  const double T = sc[S_T];
  for (int j = wv; j < n_rho; j += nw) {
    if (lane != 0) continue;
    bool ok;
    const double l = ll[j], rho = fmin(sets.rho[j], FIN_RHO_CAP);
    const double qmin = (fin_chi2_isf(T, l, ok) - l) / sqrt(2.0 * l) * lsd[j] + lc1[j];
    const double tau = rho * s11e + (1.0 - rho) * sc[S_AA] / s11e;
    al[j] = qmin / (1.0 - rho);
    be[j] = tau / (1.0 - rho);
    fm[1 + j] = ok ? 0.0 : 1.0;
  }
  __syncthreads();
  const double mu = sc[S_MU], sd = sc[S_SD], df = sc[S_DF];
  if (tid == 0) {
    const double level = mu - sd * sqrt(0.5 * df);            // where the argument of S_df reaches 0
    double x0 = INFINITY;
    for (int j = 0; j < n_rho; ++j) x0 = fmin(x0, (al[j] - level) / be[j]);
    const double z0 = x0 > 0.0 ? sqrt(x0) : 0.0;
    sc[S_Z0] = z0;
    sc[S_END] = fmin(z0, FIN_Z_END);
    for (int j = 0; j < n_rho; ++j)
      if (fm[1 + j] != 0.0) ic[I_FLAG] |= FIN_F_ROOT;
  }
  __syncthreads();
  const double z0 = sc[S_Z0], end = sc[S_END];
  // the break points: 0, the end, and the pairwise intersections of the lines inside (an intersection outside counts as the end:
  // a piece of no length)
  const int npair = n_rho * (n_rho - 1) / 2, npts = npair + 2;
  for (int at = tid; at < npts; at += nt) {
    double z = end;
    if (at == 0) {
      z = 0.0;
    } else if (at >= 2) {
      int i = 0, rest = at - 2;
      while (rest >= n_rho - 1 - i) {
        rest -= n_rho - 1 - i;
        ++i;
      }
      const int j = i + 1 + rest;
      if (be[i] != be[j]) {
        const double x = (al[i] - al[j]) / (be[i] - be[j]);
        if (x > 0.0 && sqrt(x) < end) z = sqrt(x);
      }
    }
    pts[at] = z;
  }
  __syncthreads();
  for (int at = tid; at < npts; at += nt) {
    const double v = pts[at];
    int rank = 0;
    for (int j = 0; j < npts; ++j) rank += (pts[j] < v || (pts[j] == v && j < at)) ? 1 : 0;
    spts[rank] = v;
  }
  __syncthreads();
  // the integral: a piece per group of FIN_GL lanes, a node per lane; the group's terms are folded by a fixed tree and the
  // pieces' sums added in the order of the pieces, so the bits do not depend on the number of threads (which the block's
  // largest set decides)
  const double sq = sqrt(2.0 * df);
  const int node = tid & (FIN_GL - 1), grp = tid / FIN_GL, ngrp = nt / FIN_GL;
  const int hn = node < FIN_GL / 2 ? FIN_GL / 2 - 1 - node : node - FIN_GL / 2;
  const double xn = node < FIN_GL / 2 ? -FIN_GL_X[hn] : FIN_GL_X[hn];
  for (int base = 0; base < npts - 1; base += ngrp) {
    const int piece = base + grp;
    double term = 0.0;
    if (piece < npts - 1) {
      const double lo = spts[piece], hi = spts[piece + 1];
      if (hi > lo) {
        // z = hi - (hi - lo) v^2, v in (0, 1): the nodes crowd towards the piece's upper end, where S_df has a square-root
        // singularity at z0 for df = 1 (and close behind the end of the pieces before the last, whose kinks crowd towards z0)
        const double v = 0.5 + 0.5 * xn, z = hi - (hi - lo) * (v * v);
        double del = INFINITY;
        for (int j = 0; j < n_rho; ++j) del = fmin(del, al[j] - be[j] * (z * z));
        const double arg = (del - mu) / sd * sq + df;
        term = (hi - lo) * v * FIN_GL_W[hn] * fin_chi2_sf(arg, df) * (0.79788456080286535588 * exp(-0.5 * z * z));   // 2 phi(z)
      }
    }
#pragma unroll
    for (int o = FIN_GL / 2; o > 0; o >>= 1) term += __shfl_down(term, o, FIN_GL);
    if (node == 0 && piece < npts - 1) pts[piece] = term;    // (the unsorted break points are no longer needed)
  }
  __syncthreads();
  if (tid == 0) {
    double integral = 0.0;
    for (int piece = 0; piece < npts - 1; ++piece) integral += pts[piece];
    const double p = integral + erfc(z0 * 0.70710678118654752440);    // + 2 Phi(-z0)
    row[6] = fmin(p, (double)n_rho * T);
    row[7] = T;
    row[8] = sets.rho[ic[I_J0]];
    row[9] = (double)ic[I_FLAG];
  }
}

}  // namespace scilmm
