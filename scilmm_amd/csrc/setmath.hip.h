// What the kernels of the variant-set finish share (setfinish.hip.h, setwide.hip.h, setspa.hip.h; DESIGN.md sections 19, 20 and
// 22), every formula once:
//   the small pieces : the keep predicate, the forward substitution z = R^-T w(C)'x, an entry of the projected kernel, the weight
//                      modes, the row of a set with nothing left, the workgroup's fold;
//   special functions: the regularised incomplete gamma function, the chi-square and normal tails, the chi-square quantile;
//   the mixtures     : the modified Liu matching, Lugannani-Rice and the seam between them, and the moments of the remainder
//                      term, each over a walk policy that says who walks the spectrum -- FinSerial: one lane, in index order;
//                      FinWave: the 64 lanes of a wave, lane l the entries l, l + 64, ..., the lanes' sums added by a fixed
//                      butterfly that leaves the same bits in every lane, so all 64 lanes take every branch together;
//   the SKAT-O tail  : fin_skato_decide (T, its first minimiser, the degenerate rule) and fin_skato_integral (the quantiles, the
//                      lines, the break points and the piecewise quadrature), called by a whole workgroup on a FinTail of LDS.
// No atomics; every sum is taken in a fixed order and folded by a fixed tree.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "plan_types.h"

namespace scilmm {

constexpr int FIN_HEAD = 10;        // doubles of a set's row before its per-rho p-values
constexpr int FIN_RHO_MAX = 16;     // grid values at most
constexpr int FIN_CMAX = 31;        // covariates at most (SCAN_QMAX - 1)
constexpr int FIN_GL = 32;          // Gauss-Legendre nodes per piece of the integral
constexpr int FIN_ITMAX = 200;      // steps of a root at most
constexpr double FIN_FLOOR = 1e-10;    // eigenvalues below this fraction of the largest are dropped from a mixture
constexpr double FIN_SEAM = 0.05;      // the saddlepoint seam, in standard deviations
constexpr double FIN_RHO_CAP = 0.999;  // a grid value above it is computed as it
constexpr double FIN_Z_END = 40.0;     // the integral stops here
enum { FIN_BETA = 0, FIN_ONES = 1, FIN_GIVEN = 2 };         // weight modes
enum { FIN_SADDLE = 0, FIN_LIU = 1 };                       // tail methods
// the flag word: bit 0 the degenerate rule answered (p = T); bit 1 the Jacobi iteration ran out of sweeps (the bisection of a
// wide set out of steps); bit 2 a root (secular equation, saddlepoint, quantile) ran out of steps; bit 3 SKAT-O was asked for and
// computed; bit 4 a kept column's variance scale is not 1 (scilmm_sets_finish_scaled_dev)
enum { FIN_F_DEGENERATE = 1, FIN_F_SWEEPS = 2, FIN_F_ROOT = 4, FIN_F_SKATO = 8, FIN_F_SCALED = 16 };

// the grid of rho, a kernel argument by value
struct FinGrid {
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

// ---- the small pieces ----

__device__ __forceinline__ double fin_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// a marker is kept where it has an observed value and variation
__device__ __forceinline__ bool fin_kept(double n_obs, double css) { return !(n_obs == 0.0 || css == 0.0); }

// z = R^-T w(C)'x of one marker by forward substitution: load(r) is entry r of w(C)'x, the marker's z goes to Z[r * ld + a]
// (read back by this thread alone); returns u'z
template <class Load, class Ld>
__device__ __forceinline__ double fin_forward(int c, const double* __restrict__ R, const double* __restrict__ u, Load load, double* Z, Ld ld, int a) {
  double uz = 0.0;
  for (int r = 0; r < c; ++r) {
    double v = load(r);
    for (int l = 0; l < r; ++l) v -= R[l * c + r] * Z[l * ld + a];
    v /= R[r * c + r];
    Z[r * ld + a] = v;
    uz += u[r] * v;
  }
  return uz;
}

// entry (i, j) of the projected kernel from the two entries of X'X (the host's 0.5 (K + K')) and z_i'z_j
__device__ __forceinline__ double fin_kernel_entry(double g_ij, double g_ji, double zz) { return 0.5 * (g_ij + g_ji) - zz; }

// a marker's weight by the mode: the Beta(1, 25) density at its minor allele frequency (half its mean), 1, or the caller's
__device__ __forceinline__ double fin_weight(int32_t wmode, double mean, const double* __restrict__ weights, int col) {
  if (wmode == FIN_BETA) {
    const double maf = fmin(0.5 * mean, 1.0 - 0.5 * mean), x = 1.0 - maf;
    const double x2 = x * x, x4 = x2 * x2, x8 = x4 * x4;
    return 25.0 * (x8 * x8 * x8);                            // 25 (1 - maf)^24
  }
  return wmode == FIN_GIVEN ? weights[col] : 1.0;
}

// the row of a set with nothing left
__device__ __forceinline__ void fin_empty_row(double* row, int n_rho) {
  row[0] = 0.0;
  for (int i = 1; i < FIN_HEAD - 1; ++i) row[i] = fin_nan();
  row[FIN_HEAD - 1] = 0.0;
  for (int j = 0; j < n_rho; ++j) row[FIN_HEAD + j] = fin_nan();
}

// the workgroup's values folded by a fixed tree; every thread gets the result (red: blockDim.x values, reusable at once)
struct FinAdd {
  template <class T>
  __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct FinMax {   // (exact, whatever the order)
  __device__ __forceinline__ double operator()(double a, double b) const { return fmax(a, b); }
};
template <class T, class Op>
__device__ __forceinline__ T fin_fold(T v, T* red, Op op) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int s = blockDim.x >> 1; s > 0; s >>= 1) {
    if (tid < s) red[tid] = op(red[tid], red[tid + s]);
    __syncthreads();
  }
  const T out = red[0];
  __syncthreads();
  return out;
}

// ---- special functions (a thread each) ----

// the regularised upper incomplete gamma function Q(a, x), a > 0: the series of P below a + 1, the continued fraction of Q
// (modified Lentz) above; relative accuracy in the upper tail.  Out of line: every tail of a kernel calls this one copy.
__device__ __noinline__ double fin_gamma_q(double a, double x) {
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

// ---- the mixtures sum lam_i chi2_1, over a walk policy ----

struct FinSerial {   // one lane walks the list in index order
  static constexpr int stride = 1;
  static __device__ __forceinline__ int first() { return 0; }
  static __device__ __forceinline__ double total(double v) { return v; }
};
struct FinWave {     // the 64 lanes of a wave walk it together; every lane gets the same total
  static constexpr int stride = 64;
  static __device__ __forceinline__ int first() { return threadIdx.x & 63; }
  static __device__ __forceinline__ double total(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
  }
};

// the modified Liu matching of sum lam_i chi2_1 (mean c1, variance 2 c2; scale a, degrees of freedom l).  Every spectrum here is
// positive, so c3^2 <= c2 c4 (Cauchy-Schwarz) and the host form's branch that matches the skewness as well, with a non-central
// chi-square, is never taken: the kurtosis is matched, l = c2^2 / c4, and the tail is a central chi-square's.
struct FinLiu {
  double c1, c2, a, l;
};

template <class Walk>
__device__ FinLiu fin_liu_params(const double* lam, int n) {
  double c1 = 0.0, c2 = 0.0, c4 = 0.0;
  for (int i = Walk::first(); i < n; i += Walk::stride) {
    const double v = lam[i], v2 = v * v;
    c1 += v;
    c2 += v2;
    c4 += v2 * v2;
  }
  c1 = Walk::total(c1);
  c2 = Walk::total(c2);
  c4 = Walk::total(c4);
  FinLiu p{c1, c2, 0.0, c2 * c2 / c4};
  p.a = sqrt(p.l);
  return p;
}

__device__ double fin_liu_sf(double q, const FinLiu& p) {
  const double x = (q - p.c1) / sqrt(2.0 * p.c2) * (1.41421356237309504880 * p.a) + p.l;
  return fin_chi2_sf(x, p.l);
}

// the first, second and fourth power sums of the remainder term's eigenvalues (the list holds those above the floor)
struct FinMoments {
  double mu, l2, l4;
};

template <class Walk>
__device__ __forceinline__ FinMoments fin_b_moments(const double* ev, int n) {
  double mu = 0.0, l2 = 0.0, l4 = 0.0;
  for (int i = Walk::first(); i < n; i += Walk::stride) {
    const double v = ev[i];
    mu += v;
    l2 += v * v;
    l4 += (v * v) * (v * v);
  }
  return FinMoments{Walk::total(mu), Walk::total(l2), Walk::total(l4)};
}

// Lugannani-Rice for q > 0 away from the mean: K'(t) = sum lam / (1 - 2 lam t) = q by Newton from 0 inside the bracket of the
// host form (scilmm_amd.sets._lugannani_rice), a step that leaves it replaced by its midpoint; lmax: the largest of lam
template <class Walk>
__device__ double fin_lugannani_rice(double q, const double* lam, int n, double mu, double lmax, bool& ok) {
  const double pole = 0.5 / lmax;
  auto k1 = [&](double t, double& k2) {
    double f = 0.0, g = 0.0;
    for (int i = Walk::first(); i < n; i += Walk::stride) {
      const double r = lam[i] / (1.0 - 2.0 * lam[i] * t);
      f += r;
      g += r * r;
    }
    k2 = 2.0 * Walk::total(g);
    return Walk::total(f) - q;
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
  for (int i = Walk::first(); i < n; i += Walk::stride) {
    const double den = 1.0 - 2.0 * lam[i] * t, r = lam[i] / den;
    K0 += log1p(-2.0 * lam[i] * t);
    k2 += r * r;
  }
  K0 = -0.5 * Walk::total(K0);
  k2 = 2.0 * Walk::total(k2);
  const double w = copysign(sqrt(2.0 * (t * q - K0)), t), v = t * sqrt(k2);
  return fin_norm_sf(w + log(v / w) / w);
}

// P(sum lam_i chi2_1 > q) for the n positive lam (the floor applied) with the largest lmax, by `method`; the seam as on the host
template <class Walk>
__device__ double fin_mixture_sf(double q, const double* lam, int n, double lmax, const FinLiu& liu, int method, bool& ok) {
  ok = true;
  if (method == FIN_LIU) return fin_liu_sf(q, liu);
  if (q <= 0.0) return 1.0;
  const double mu = liu.c1, sd = sqrt(2.0 * liu.c2);
  if (fabs(q - mu) >= FIN_SEAM * sd) return fin_lugannani_rice<Walk>(q, lam, n, mu, lmax, ok);
  const double lo = mu - FIN_SEAM * sd, hi = mu + FIN_SEAM * sd;
  bool ok1, ok2;
  const double c_lo = fin_lugannani_rice<Walk>(lo, lam, n, mu, lmax, ok1) / fin_liu_sf(lo, liu);
  const double c_hi = fin_lugannani_rice<Walk>(hi, lam, n, mu, lmax, ok2) / fin_liu_sf(hi, liu);
  ok = ok1 && ok2;
  return fin_liu_sf(q, liu) * (c_lo + (c_hi - c_lo) * (q - lo) / (hi - lo));
}

// ---- the SKAT-O tail, by a whole workgroup ----

enum { FS_SKATP = 0, FS_T, FS_MU, FS_SD, FS_DF, FS_Z0, FS_END, FS_AA, FS_N };   // scalars of the tail
enum { FI_FLAG = 0, FI_J0, FI_DEG, FI_NB, FI_N };                        // integers of the tail

// The LDS of the tail.  Before fin_skato_decide the caller's tasks have left: p_rho, Q_rho and the Liu numbers c1, sd, l of every
// grid value; sc[FS_SKATP]; the remainder term's sc[FS_MU], sc[FS_SD], sc[FS_DF] and ic[FI_NB]; sc[FS_AA] = a'a, a = A1; the flags
// so far in ic[FI_FLAG]; fm[0] and fm[1 + j] marked where the tail of SKAT or of grid value j ran out of steps.
struct FinTail {
  double* prho;          // p_rho | Q_rho | c1 | sd | l | alpha | beta (FIN_RHO_MAX each)
  double* sc;            // FS_N scalars
  double* fm;            // FIN_RHO_MAX + 2 marks, 0 or 1
  double *pts, *spts;    // break points, unsorted | sorted (128 each)
  int32_t* ic;           // FI_N integers
  __device__ __forceinline__ double* qrho() const { return prho + FIN_RHO_MAX; }
  __device__ __forceinline__ double* lc1() const { return prho + 2 * FIN_RHO_MAX; }
  __device__ __forceinline__ double* lsd() const { return prho + 3 * FIN_RHO_MAX; }
  __device__ __forceinline__ double* ll() const { return prho + 4 * FIN_RHO_MAX; }
  __device__ __forceinline__ double* al() const { return prho + 5 * FIN_RHO_MAX; }
  __device__ __forceinline__ double* be() const { return prho + 6 * FIN_RHO_MAX; }
};

// T = min p_rho, its first minimiser and the degenerate rule; row[5 .. 8] where they are final, the per-rho p-values and the flag
// word `ic[FI_FLAG] | flags`.  Behind a barrier of the caller; true where the row is finished (every thread gets the same answer).
__device__ __forceinline__ bool fin_skato_decide(const FinTail& t, int kept, int nskat, bool want_b, int n_rho, int flags,
                                                 const FinGrid& grid, double* row) {
  const bool skato = n_rho > 0 && nskat > 0;
  if (threadIdx.x == 0) {
    const double nan = fin_nan();
    double* prho = t.prho;
    const double ps = t.sc[FS_SKATP];
    row[5] = ps;
    int flag = t.ic[FI_FLAG] | flags;
    for (int j = 0; j < 1 + FIN_RHO_MAX; ++j)
      if (t.fm[j] != 0.0) flag |= FIN_F_ROOT;
    int deg = 1;
    double T = nan;
    int j0 = 0;
    if (skato) {
      flag |= FIN_F_SKATO;
      if (kept == 1) {
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
        deg = any_nan || !want_b || t.ic[FI_NB] == 0 || !(T > 0.0);
      }
      if (deg) {
        // one marker, a'1 = 0 or B = 0: every p_rho is the same up to rounding, p = T and the first grid value stands for the
        // minimiser; T = 0 (underflow): so is p
        const bool same = kept == 1 || !want_b || t.ic[FI_NB] == 0;
        row[6] = T;
        row[7] = T;
        row[8] = T == T ? grid.rho[same ? 0 : j0] : nan;
        flag |= FIN_F_DEGENERATE;
      }
      for (int j = 0; j < n_rho; ++j) row[FIN_HEAD + j] = prho[j];
    } else {
      row[6] = row[7] = row[8] = nan;
      for (int j = 0; j < n_rho; ++j) row[FIN_HEAD + j] = nan;
    }
    t.sc[FS_T] = T;
    t.ic[FI_J0] = j0;
    t.ic[FI_DEG] = skato ? deg : 1;
    t.ic[FI_FLAG] = flag;
  }
  __syncthreads();
  if (!t.ic[FI_DEG]) return false;
  if (threadIdx.x == 0) row[9] = (double)t.ic[FI_FLAG];
  return true;
}

// The SKAT-O integral behind fin_skato_decide, with s11e = 1'A1: the quantiles q_min(rho) and the lines (alpha - beta x), the
// break points sorted in LDS, a piece per FIN_GL lanes with a Gauss-Legendre node each, the tail in closed form; row[6 .. 9].
// (a'a is read from LDS by the few lanes that need it: as an argument it would stay in registers across the quantiles' calls.)
__device__ __forceinline__ void fin_skato_integral(const FinTail& t, int n_rho, double s11e, const FinGrid& grid, double* row) {
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wv = tid >> 6, nw = nt >> 6;
  double *al = t.al(), *be = t.be(), *pts = t.pts, *spts = t.spts;
  // the quantiles and the lines: a lane per grid value
  const double T = t.sc[FS_T];
  for (int j = wv; j < n_rho; j += nw) {
    if (lane != 0) continue;
    bool ok;
    const double l = t.ll()[j], rho = fmin(grid.rho[j], FIN_RHO_CAP);
    const double qmin = (fin_chi2_isf(T, l, ok) - l) / sqrt(2.0 * l) * t.lsd()[j] + t.lc1()[j];
    const double tau = rho * s11e + (1.0 - rho) * t.sc[FS_AA] / s11e;
    al[j] = qmin / (1.0 - rho);
    be[j] = tau / (1.0 - rho);
    t.fm[1 + j] = ok ? 0.0 : 1.0;
  }
  __syncthreads();
  const double mu = t.sc[FS_MU], sd = t.sc[FS_SD], df = t.sc[FS_DF];
  if (tid == 0) {
    const double level = mu - sd * sqrt(0.5 * df);            // where the argument of S_df reaches 0
    double x0 = INFINITY;
    for (int j = 0; j < n_rho; ++j) x0 = fmin(x0, (al[j] - level) / be[j]);
    const double z0 = x0 > 0.0 ? sqrt(x0) : 0.0;
    t.sc[FS_Z0] = z0;
    t.sc[FS_END] = fmin(z0, FIN_Z_END);
    for (int j = 0; j < n_rho; ++j)
      if (t.fm[1 + j] != 0.0) t.ic[FI_FLAG] |= FIN_F_ROOT;
  }
  __syncthreads();
  const double z0 = t.sc[FS_Z0], end = t.sc[FS_END];
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
  // pieces' sums added in the order of the pieces, so the bits do not depend on the number of threads
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
    row[8] = grid.rho[t.ic[FI_J0]];
    row[9] = (double)t.ic[FI_FLAG];
  }
}

}  // namespace scilmm
