// Kernel of the saddlepoint score scan for binary traits (scilmm_scan_spa_dev and its two siblings, engine.hip): behind a plain
// scan block of the same markers, the score b = g~' P y~ and its variance a = g~' P g~ of that block (from its statistics) are
// turned into a two-sided saddlepoint p-value under independent Bernoulli(mu_i) draws (SAIGE / fastGWA-GLMM; DESIGN.md
// section 18).
//   k_scan_spa<Reader>     : one workgroup per marker, 256 threads with a fixed stride over n   reads  n (c + 2) * 8 + the
//                            marker's row twice; then 16 B per individual and one fp64 exp per Newton pass, from its scratch row
// Steps 1 - 3 (the covariate adjustment, a_w and s, the two roots) are the device function spa_roots, which k_sets_spa
// (setspa.hip.h) runs on a set's collapsed genotype as well.
// Every sum is taken thread by thread in ascending order of i and folded by a fixed tree (shuffles inside a wave, then the four
// waves in wave order; the covariate sums of step 1 in lane groups added in group order); no atomics, no sum across workgroups:
// a marker's bits depend on its inputs alone, in either mode of the handle.  The kernel is templated on a row READER, the only part that knows the input form: reader(c, i) = individual i's
// centred, mean-imputed g~_i = g_i - mean (0 where the value is missing or the individual not genotyped), by the decode
// expressions of k_scan_dequant / k_bed_dequant / k_dos_dequant<T>, so the three forms of the same hard calls give the same bits.
//
// mu, C are in the ORIGINAL order of the individuals (like the marker rows): nothing here is permuted.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "bed.hip.h"
#include "dosage.hip.h"
#include "plan_types.h"
#include "scan.hip.h"

namespace scilmm {

constexpr int SPA_ROWS = 7;      // rows of the result: log_p | a_w | s | zeta_hi | zeta_lo | iters | flag
constexpr int SPA_CMAX = 31;     // covariates at most (SCAN_QMAX - 1)
constexpr int SPA_ITMAX = 64;    // Newton / bisection steps per root at most
constexpr double SPA_TOL = 1e-13;  // |step| <= SPA_TOL max(1, |zeta|) ends a root

struct SpaInt8 {
  const int8_t* geno;
  int64_t ld;
  __device__ __forceinline__ double operator()(int c, int64_t i, double m) const {
    const int g = (int)geno[(int64_t)c * ld + i];
    return g >= 0 ? (double)g - m : 0.0;
  }
};

struct SpaBed {
  const uint8_t* bed;
  int64_t ld;
  int32_t N;
  const int32_t* sample;
  int32_t flags;
  __device__ __forceinline__ double operator()(int c, int64_t i, double m) const {
    const uint32_t s = sample ? (uint32_t)sample[i] : (uint32_t)i;
    if (s >= (uint32_t)N) return 0.0;
    const int code = (bed[(int64_t)c * ld + (s >> 2)] >> (2 * (s & 3))) & 3;
    const int hl = (code >> 1) + (code & 1);
    const int g = (flags & BED_A2) ? hl : 2 - hl;
    return code != 1 ? (double)g - m : 0.0;
  }
};

template <class T>
struct SpaDos {
  const T* dos;
  int64_t ld;
  int32_t N;
  const int32_t* sample;
  __device__ __forceinline__ double operator()(int c, int64_t i, double m) const {
    const uint32_t s = sample ? (uint32_t)sample[i] : (uint32_t)i;
    if (s >= (uint32_t)N) return 0.0;
    const T g = dos[(int64_t)c * ld + s];
    return dos_observed(g) ? dos_value(g) - m : 0.0;
  }
};

// log of the upper normal tail, finite far beyond where the tail underflows: log(erfcx(v / sqrt 2) / 2) - v^2 / 2
__device__ __forceinline__ double spa_log_tail(double v) { return log(0.5 * erfcx(v * 0.70710678118654752440)) - 0.5 * v * v; }

// One individual's terms of the cumulant generating function of T = sum g_i (y_i - mu_i) at x = g_i t, each with its own share
// of t m1 = sum mu_i x_i taken off (the same sums as K = sum log(1 - mu + mu e^x) - t m1 and its derivatives, without the
// cancellation between the two): pm = p - mu with p = mu e^x / (1 - mu + mu e^x), pq = p (1 - p).  Overflow-free: e^-|x| only.
__device__ __forceinline__ void spa_term(double x, double mu, double& pm, double& pq) {
  const double e = exp(-fabs(x));
  const double den = x > 0.0 ? fma(1.0 - mu, e, mu) : fma(mu, e, 1.0 - mu);
  const double p = (x > 0.0 ? mu : mu * e) / den;
  const double q = (x > 0.0 ? (1.0 - mu) * e : 1.0 - mu) / den;
  pm = x > 0.0 ? (1.0 - mu) - q : p - mu;   // (the smaller of p, 1 - p is the one that is formed: no rounding against 1)
  pq = p * q;
}
// log(1 - mu + mu e^x) - mu x: log1p(mu expm1(x)) for x <= 0, its mirrored form x + log1p((1 - mu) expm1(-x)) for x > 0
__device__ __forceinline__ double spa_logterm(double x, double mu) {
  return x > 0.0 ? fma(1.0 - mu, x, log1p((1.0 - mu) * expm1(-x))) : log1p(mu * expm1(x)) - mu * x;
}

struct SpaFold {
  double* red;  // 4 x 3 doubles
  int lane, wv;
  // the 256 threads' values folded by a fixed tree; every thread gets the result (two barriers: `red` is reusable at once)
  __device__ __forceinline__ void operator()(double& a, double& b, double& c) const {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      a += __shfl_down(a, o);
      b += __shfl_down(b, o);
      c += __shfl_down(c, o);
    }
    if (lane == 0) {
      red[3 * wv] = a;
      red[3 * wv + 1] = b;
      red[3 * wv + 2] = c;
    }
    __syncthreads();
    a = ((red[0] + red[3]) + red[6]) + red[9];
    b = ((red[1] + red[4]) + red[7]) + red[10];
    c = ((red[2] + red[5]) + red[8]) + red[11];
    __syncthreads();
  }
};

// What steps 1 - 3 leave behind: the numbers of a result row behind log_p (which `spa_log_p` makes of them on one thread).
struct SpaRoots {
  double aw, s, zeta_hi, zeta_lo, ltail_hi, ltail_lo;
  int iters;
  bool good;
};

// Steps 1 - 3 of the saddlepoint call for ONE centred row `row(i)` with score b and variance a (a marker's in k_scan_spa, a
// set's collapsed genotype in k_sets_spa: setspa.hip.h), by the 256 threads of a workgroup; every thread returns the same bits.
// mu: n fitted probabilities; Cv: n x c covariates, row-major; Minv: (C' W C)^-1, W = diag(mu (1 - mu)); g: a scratch row of n
// doubles, g^ = g~ - C (Minv C' W g~) when the call returns; tred: 256 doubles, tt and gam: SPA_CMAX + 1 doubles each, in LDS.
// Every branch on a sum is uniform over the workgroup (all threads hold the same folded bits), so the barriers inside the root
// loop are reached by all of them.
template <class Row>
__device__ __forceinline__ SpaRoots spa_roots(int32_t n, int32_t c, Row row, double a, double b, const double* __restrict__ mu,
                                              const double* __restrict__ Cv, const double* __restrict__ Minv, double* g,
                                              double* tred, double* tt, double* gam, const SpaFold& fold) {
  const int tid = threadIdx.x;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);

  // 1. t_k = sum_i w_i C_ik g~_i, gamma = Minv t.  Lanes run along the covariates (a row of C is read once, contiguously): groups
  // of LG = 8, 16 or 32 lanes (the least that holds c), group g takes individuals g, g + 256 / LG, ... in ascending order, and
  // the groups are added in group order: the order of every sum depends on (n, c) alone.
  {
    const int lg = c <= 8 ? 8 : c <= 16 ? 16 : 32, ng = 256 / lg;
    const int k = tid & (lg - 1), grp = tid / lg;
    double acc = 0.0;
    for (int64_t i = grp; i < n; i += ng) {
      const double m = mu[i];
      const double wg = (m * (1.0 - m)) * row(i);
      if (k < c) acc = fma(Cv[i * c + k], wg, acc);
    }
    tred[tid] = acc;
    __syncthreads();
    if (tid < c) {
      double v = tred[tid];
      for (int u = 1; u < ng; ++u) v += tred[u * lg + tid];
      tt[tid] = v;
    }
    __syncthreads();
    if (tid < c) {
      double v = 0.0;
      for (int l = 0; l < c; ++l) v = fma(Minv[tid * c + l], tt[l], v);
      gam[tid] = v;
    }
    __syncthreads();
  }

  // 2. g^_i = g~_i - C_i . gamma into the scratch row; a_w = sum w_i g^_i^2; s = b sqrt(a_w / a); the support of T
  double aw = 0.0, up = 0.0, dn = 0.0;   // up, -dn: the ends of T's support, K'(+inf) and K'(-inf)
  for (int64_t i = tid; i < n; i += 256) {
    const double m = mu[i];
    const double* crow = Cv + i * c;
    double d = 0.0;
    for (int k = 0; k < c; ++k) d = fma(crow[k], gam[k], d);
    const double gh = row(i) - d;
    g[i] = gh;
    aw = fma((m * (1.0 - m)) * gh, gh, aw);
    up += gh > 0.0 ? gh * (1.0 - m) : -gh * m;
    dn += gh > 0.0 ? gh * m : -gh * (1.0 - m);
  }
  fold(aw, up, dn);
  const double s = b * sqrt(aw / a), sa = fabs(s);

  // 3. the two roots K'(zeta) = +-|s| by safeguarded Newton from 0 (K' is increasing: a bracket is kept, and a step that
  // leaves it is replaced by its midpoint), then K, K', K'' at each root and the two tails.  A thread reads its own g^_i back.
  double zeta[2] = {nan, nan}, ltail[2] = {nan, nan};
  // |s| at or beyond an end of the support: there is no root on that side, the result is the normal value -- no pass is spent
  bool good = sa < up && sa < dn;
  int iters = 0;
#pragma unroll 1
  for (int side = 0; good && side < 2; ++side) {
    const double sg = side == 0 ? 1.0 : -1.0;
    // in the mirrored variable y = sg * zeta >= 0: f(y) = sg K'(sg y) - |s| is increasing, f(0) = -|s| < 0
    double lo = 0.0, hi = INFINITY, y = 0.0;
    bool conv = false, dead = false;
    int it = 0;
#pragma unroll 1
    for (; it < SPA_ITMAX; ++it) {
      const double t = sg * y;
      double k1 = 0.0, k2 = 0.0, z0 = 0.0;
      for (int64_t i = tid; i < n; i += 256) {
        const double gh = g[i];
        double pm, pq;
        spa_term(gh * t, mu[i], pm, pq);
        k1 = fma(gh, pm, k1);
        k2 = fma(gh * gh, pq, k2);
      }
      fold(k1, k2, z0);
      const double f = sg * k1 - sa;
      if (f < 0.0) lo = y; else hi = y;
      double yn = y - f / k2;
      if (!(yn > lo && yn < hi)) yn = 0.5 * (lo + hi);  // (a NaN step as well; lo + inf where no upper end is known yet)
      if (!(fabs(yn) < INFINITY)) {
        dead = true;  // K'' has underflowed below the target: |s| lies outside the support of T
        break;
      }
      const double dy = fabs(yn - y);
      y = yn;
      if (dy <= SPA_TOL * fmax(1.0, y)) {
        conv = true;
        ++it;
        break;
      }
    }
    iters = max(iters, it);
    zeta[side] = dead ? nan : sg * y;
    if (!conv) {
      good = false;
      break;
    }
    const double t = sg * y;
    double k0 = 0.0, k1 = 0.0, k2 = 0.0;
    for (int64_t i = tid; i < n; i += 256) {
      const double gh = g[i], m = mu[i], x = gh * t;
      double pm, pq;
      spa_term(x, m, pm, pq);
      k0 += spa_logterm(x, m);
      k1 = fma(gh, pm, k1);
      k2 = fma(gh * gh, pq, k2);
    }
    fold(k0, k1, k2);
    const double om = sqrt(2.0 * (t * k1 - k0)), nu = y * sqrt(k2);
    const double v = om + log(nu / om) / om;
    if (v > 0.0 && v < INFINITY) ltail[side] = spa_log_tail(v);
    else good = false;
  }
  return SpaRoots{aw, s, zeta[0], zeta[1], ltail[0], ltail[1], iters, good};
}

// log p of a call: the sum of the two tails, or the normal value log(2 upper tail(|zs|)) where the saddlepoint failed (a thread)
__device__ __forceinline__ double spa_log_p(const SpaRoots& o, double zs) {
  if (o.good) {
    const double hi = fmax(o.ltail_hi, o.ltail_lo), lw = fmin(o.ltail_hi, o.ltail_lo);
    return hi + log1p(exp(lw - hi));
  }
  return log(erfcx(fabs(zs) * 0.70710678118654752440)) - 0.5 * zs * zs;
}

// stats: the (q + 4) x r statistics of the plain block (q = c + 1): rows n_obs | mean | css | |x|^2 | w(C)'x (c rows) | w(y~)'x.
// R: c x c upper triangular, R'R = w(C)'w(C); u: R^-T w(C)'w(y~); mu, Cv, Minv: as spa_roots takes them; gs: the handle's
// scratch, row `marker` of n doubles holds g^.  out: SPA_ROWS x r.
template <class Reader>
__global__ __launch_bounds__(256) void k_scan_spa(int32_t n, int32_t r, int32_t c, Reader rd, const double* __restrict__ stats,
                                                  const double* __restrict__ R, const double* __restrict__ u,
                                                  const double* __restrict__ mu, const double* __restrict__ Cv,
                                                  const double* __restrict__ Minv, double cutoff, double* __restrict__ gs,
                                                  double* __restrict__ out) {
  __shared__ double red[4 * 3];
  __shared__ double tred[256];
  __shared__ double tt[SPA_CMAX + 1], gam[SPA_CMAX + 1], head[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int j = blockIdx.x;
  const SpaFold fold{red, lane, wv};
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  auto put = [&](int row, double v) { out[(int64_t)row * r + j] = v; };

  // 0. a, b, zs from the block's statistics: R' z = w(C)'x by forward substitution (thread 0; c <= 31)
  if (tid == 0) {
    const double* S = stats + j;
    double zz = 0.0, uz = 0.0;
    for (int k = 0; k < c; ++k) {
      double v = S[(int64_t)(4 + k) * r];
      for (int l = 0; l < k; ++l) v -= R[l * c + k] * tt[l];
      v /= R[k * c + k];
      tt[k] = v;
      zz += v * v;
      uz += u[k] * v;
    }
    const double a = S[3 * (int64_t)r] - zz, b = S[(int64_t)(4 + c) * r] - uz;
    head[0] = a;
    head[1] = b;
    head[2] = S[0];
    head[3] = S[2 * (int64_t)r];
  }
  __syncthreads();
  const double a = head[0], b = head[1];
  const double zs = b / sqrt(a);
  if (head[2] == 0.0 || head[3] == 0.0 || !(a > 0.0) || !(fabs(zs) > cutoff)) {
    if (tid == 0) {
#pragma unroll
      for (int row = 0; row < SPA_ROWS - 1; ++row) put(row, nan);
      put(SPA_ROWS - 1, 0.0);
    }
    return;  // (the whole workgroup)
  }
  const double mean = stats[(int64_t)r + j];
  const SpaRoots o = spa_roots(n, c, [&](int64_t i) { return rd(j, i, mean); }, a, b, mu, Cv, Minv, gs + (int64_t)j * n, tred, tt,
                               gam, fold);
  if (tid == 0) {
    put(0, spa_log_p(o, zs));
    put(1, o.aw);
    put(2, o.s);
    put(3, o.zeta_hi);
    put(4, o.zeta_lo);
    put(5, (double)o.iters);
    put(6, o.good ? 1.0 : 2.0);
  }
}

}  // namespace scilmm
