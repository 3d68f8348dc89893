// Kernels of the variant-set finish for ONE set of up to 4 096 markers (scilmm_sets_finish_wide_dev, engine.hip; DESIGN.md
// section 22): the set's sub-blocks left their statistics, their diagonal blocks of X'X and their rows of cross products in HBM;
// the finish needs no eigenvector.  One orthogonal reduction of A = diag(w) K diag(w) to a tridiagonal T whose first basis vector
// is 1 / sqrt(m) gives every spectrum of SKAT-O as the eigenvalues of a tridiagonal matrix:
//   k_wide_prep   : one workgroup; the kept markers (in order, by a prefix sum), z = R^-T w(C)'x, the weights, t = w o s; with
//                   the markers' variance scales (scilmm_sets_finish_wide_scaled_dev) the weight in A is w o scale, t keeps w;
//   k_wide_form   : a workgroup per kept row; A, compacted (m x m, ld = m, symmetric bit for bit), its row sums and diagonal;
//   k_wide_burden : one workgroup; 1'A1, 1't, t't, trace, the burden numbers and Q into the output row;
//   k_wide_symv, k_wide_rank2 : the reduction, two launches per step.  Step -1 is the Householder reflector that maps 1 to
//                   -sqrt(m) e_1, over the whole matrix; step j >= 0 that of column j below the diagonal, over the trailing matrix
//                   of order m - 1 - j.  Every workgroup forms the step's reflector itself from row j (= column j) with the same
//                   fixed-order norm, so all hold the same bits; symv leaves p = tau A v, rank2 re-forms w = p - tau/2 (p'v) v
//                   and applies A -= v w' + w v' to its rows.  The kernel boundary is the only synchronisation.
//   k_wide_scale  : a workgroup per task (SKAT, the grid values, the remainder B): the task's scaled d and e^2, its Gershgorin
//                   interval, pivmin;
//   k_wide_eig    : a thread per (task, index): bisection on the Sturm count, the spectra in descending order;
//   k_wide_tails  : one workgroup; the tails of the mixtures on the spectra in HBM, a wave per task with the task's spectrum
//                   dealt across its lanes (FinWave), then the SKAT-O tail of setmath.hip.h, the one k_sets_finish runs.
// The full symmetric matrix is kept (not one triangle): row j is then the step's column, read along the lanes, and symv and rank2
// share one decomposition (WIDE_ROWS rows per workgroup, a wave per two rows, the columns along the lanes).  No atomics; every
// sum is taken in a fixed order and folded by a fixed tree.  The number m of kept markers is known to the device alone: the grids
// are sized by k and a workgroup with nothing to do returns.
#pragma once
#include "setmath.hip.h"

namespace scilmm {

constexpr int WIDE_KMAX = 4096;                  // markers of a set at most
constexpr int WIDE_TASKS = FIN_RHO_MAX + 2;      // SKAT | the grid values | the remainder term
constexpr int WIDE_ROWS = 8;                     // rows of a workgroup of symv / rank2 (256 threads: two per wave)
constexpr int WIDE_PREP_NT = 1024;
constexpr int WIDE_BISECT = 100;                 // bisection steps at most (54 halve a Gershgorin interval to eps |T|)
constexpr int WIDE_TSC = 8;                      // doubles of a task's record: order | lower end | upper end | pivmin | atol
enum { WS_TAU = 0, WS_SCALE, WS_WS, WS_TT, WS_S11, WS_TR, WS_N = 16 };   // scalars of the work space
enum { WI_M = 0, WI_FLAG, WI_SCALED, WI_N = 16 };                        // integers of the work space (WI_SCALED: FIN_F_SCALED or 0)

// The handle's work space of one call, cut for a set of k markers and c covariates.
struct WideWs {
  double *A, *Z, *wa, *t, *rs, *dg, *p, *d, *e, *td, *te2, *ev, *tsc, *sc;
  int32_t *idx, *ic;
};
__host__ __device__ constexpr size_t wide_doubles(size_t k) {
  return k * k + (FIN_CMAX + 7 + 3 * WIDE_TASKS) * k + WIDE_TASKS * WIDE_TSC + WS_N + (k + WI_N + 1) / 2 + 1;
}
inline WideWs wide_cut(double* base, size_t k) {
  WideWs w;
  w.A = base;
  w.Z = w.A + k * k;
  w.wa = w.Z + FIN_CMAX * k;
  w.t = w.wa + k;
  w.rs = w.t + k;
  w.dg = w.rs + k;
  w.p = w.dg + k;
  w.d = w.p + k;
  w.e = w.d + k;
  w.td = w.e + k;
  w.te2 = w.td + WIDE_TASKS * k;
  w.ev = w.te2 + WIDE_TASKS * k;
  w.tsc = w.ev + WIDE_TASKS * k;
  w.sc = w.tsc + WIDE_TASKS * WIDE_TSC;
  w.idx = (int32_t*)(w.sc + WS_N);
  w.ic = w.idx + k;
  return w;
}

// Where the sub-blocks left the set's numbers: marker i of the set is column i % block of sub-block i / block.
struct WideIn {
  int32_t k, block, bp, q;
  const double *stats, *gram, *cross;
  int64_t ld_cross;
  __device__ __forceinline__ double stat(int row, int i) const {
    const int b = i / block, j = i - b * block, rb = min(block, k - b * block);
    return stats[(int64_t)b * (q + 4) * block + (int64_t)row * rb + j];
  }
  // entry (i, j) of X'X as the host puts it together (sets.assemble_wide, then set_kernel's 0.5 (K + K')): inside a sub-block the
  // mean of [i][j] and [j][i]; between two, the later marker's row of cross products -- a padding column is never addressed
  __device__ __forceinline__ double xtx(int i, int j) const {
    const int bi = i / block, bj = j / block, ji = i - bi * block, jj = j - bj * block;
    if (bi == bj) {
      const int rb = min(block, k - bi * block);
      const double* g = gram + (int64_t)bi * block * block;
      return fin_kernel_entry(g[ji * rb + jj], g[jj * rb + ji], 0.0);
    }
    return bi > bj ? cross[(int64_t)i * ld_cross + bj * bp + jj] : cross[(int64_t)j * ld_cross + bi * bp + ji];
  }
};

// Steps 0 and 1 of k_sets_finish for k <= 4 096: one workgroup of WIDE_PREP_NT threads, a run of consecutive markers each.
// vscale: k variance scales, one per marker of the set, or null (all 1).
__global__ __launch_bounds__(WIDE_PREP_NT) void k_wide_prep(WideIn in, int32_t c, const double* __restrict__ R, const double* __restrict__ u,
                                                            int32_t wmode, const double* __restrict__ weights, WideWs ws, int32_t n_rho,
                                                            double* __restrict__ row, double* __restrict__ lam_out,
                                                            const double* __restrict__ vscale) {
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
  const int m = cnt[WIDE_PREP_NT - 1];
  int at = cnt[tid] - mine;
  for (int i = i0; i < i1; ++i)
    if (fin_kept(in.stat(0, i), in.stat(2, i))) ws.idx[at++] = i;
  if (tid == 0) {
    ws.ic[WI_M] = m;
    ws.ic[WI_FLAG] = 0;
    ws.ic[WI_SCALED] = 0;
    if (m == 0) fin_empty_row(row, n_rho);
  }
  if (lam_out)
    for (int i = tid; i < k; i += WIDE_PREP_NT) lam_out[i] = fin_nan();
  __syncthreads();                                            // (the list of kept markers is visible to the workgroup)
  for (int a = tid; a < m; a += WIDE_PREP_NT) {
    const int col = ws.idx[a];
    const double uz = fin_forward(c, R, u, [&](int r) { return in.stat(4 + r, col); }, ws.Z, (int64_t)k, a);
    const double s = in.stat(4 + c, col) - uz;
    const double w = fin_weight(wmode, in.stat(1, col), weights, col);
    ws.wa[a] = vscale ? w * vscale[col] : w;                  // (the weight in A alone: t keeps w)
    ws.t[a] = w * s;
    if (vscale && vscale[col] != 1.0) ws.ic[WI_SCALED] = FIN_F_SCALED;   // (every writer stores the same value)
  }
}

// Step 2: row a of A = diag(w) (0.5 (G + G') - z'z) diag(w) for the kept markers.  Entry (a, b) and entry (b, a) are the same
// bits: the products below commute and nothing is contracted across them.
__global__ __launch_bounds__(256) void k_wide_form(WideIn in, int32_t c, WideWs ws) {
#pragma clang fp contract(off)
  __shared__ double red[256];
  const int tid = threadIdx.x, a = blockIdx.x, k = in.k;
  const int m = ws.ic[WI_M];
  if (a >= m) return;  // (the whole workgroup)
  const int i = ws.idx[a];
  const double wi = ws.wa[a];
  double rs = 0.0;
  for (int b = tid; b < m; b += 256) {
    const int j = ws.idx[b];
    double zz = 0.0;
    for (int l = 0; l < c; ++l) zz = fma(ws.Z[(int64_t)l * k + a], ws.Z[(int64_t)l * k + b], zz);
    const double kij = in.xtx(i, j) - zz;
    const double v = kij * (wi * ws.wa[b]);
    ws.A[(int64_t)a * m + b] = v;
    if (b == a) ws.dg[a] = v;
    rs += v;
  }
  rs = fin_fold(rs, red, FinAdd{});
  if (tid == 0) ws.rs[a] = rs;
}

// Step 3: the burden numbers and Q = t't.
__global__ __launch_bounds__(256) void k_wide_burden(WideWs ws, double* __restrict__ row) {
  __shared__ double red[256];
  const int tid = threadIdx.x, m = ws.ic[WI_M];
  if (m == 0) return;
  double a = 0.0, b = 0.0, c = 0.0, d = 0.0;
  for (int i = tid; i < m; i += 256) {
    const double t = ws.t[i];
    a += ws.rs[i];
    b += t;
    c += t * t;
    d += ws.dg[i];
  }
  const double s11 = fin_fold(a, red, FinAdd{}), sum = fin_fold(b, red, FinAdd{}), tt = fin_fold(c, red, FinAdd{}), tr = fin_fold(d, red, FinAdd{});
  if (tid == 0) {
    ws.sc[WS_S11] = s11;
    ws.sc[WS_WS] = sum;
    ws.sc[WS_TT] = tt;
    ws.sc[WS_TR] = tr;
    row[0] = (double)m;
    row[1] = sum / s11;
    row[2] = 1.0 / sqrt(s11);
    row[3] = sum * sum / s11;
    row[4] = tt;
  }
}

// The reflector of a step, the same bits in every workgroup of symv and of rank2: v_0 = 1, v_b = x_b scale.
struct WideRefl {
  const double* x;     // row j of A from column j + 1 on, or null: the pre-step, v_b = scale
  double scale;
  __device__ __forceinline__ double v(int b) const {
#pragma clang fp contract(off)
    return b == 0 ? 1.0 : (x ? x[b] * scale : scale);
  }
};

// p = tau A v over the trailing matrix of a step (step = -1: the pre-step), tau, the scale, d_j and e_j
__global__ __launch_bounds__(256) void k_wide_symv(int32_t step, WideWs ws) {
  __shared__ double red[256];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int m = ws.ic[WI_M], j = step, s = j + 1, n = m - s;
  if (j >= m) return;  // (the whole workgroup, here and below)
  const bool first = blockIdx.x == 0 && tid == 0;
  if (j >= 0 && first) ws.d[j] = ws.A[(int64_t)j * m + j];
  if (n < 1) return;
  double tau;
  WideRefl h;
  if (j < 0) {
    const double sq = sqrt((double)m);                        // x = 1: alpha = 1, beta = -sqrt(m)
    tau = 1.0 + 1.0 / sq;
    h.x = nullptr;
    h.scale = 1.0 / (1.0 + sq);
  } else {
    h.x = ws.A + (int64_t)j * m + s;
    double ss = 0.0;
    for (int b = 1 + tid; b < n; b += 256) ss = fma(h.x[b], h.x[b], ss);
    ss = fin_fold(ss, red, FinAdd{});
    const double alpha = h.x[0];
    double beta = alpha;
    tau = 0.0;
    h.scale = 0.0;
    if (ss != 0.0) {                                          // dlarfg without its rescaling loop
      beta = -copysign(sqrt(alpha * alpha + ss), alpha);
      tau = (beta - alpha) / beta;
      h.scale = 1.0 / (alpha - beta);
    }
    if (first) ws.e[j] = beta;
  }
  if (first) {
    ws.sc[WS_TAU] = tau;
    ws.sc[WS_SCALE] = h.scale;
  }
  if (tau == 0.0) return;
  const int r0 = blockIdx.x * WIDE_ROWS + 2 * wv, r1 = r0 + 1;
  if (r0 >= n) return;  // (the wave: no barrier follows)
  const double* a0 = ws.A + (int64_t)(s + r0) * m + s;
  const double* a1 = ws.A + (int64_t)(s + min(r1, n - 1)) * m + s;
  double acc0 = 0.0, acc1 = 0.0;
  for (int b = lane; b < n; b += 64) {
    const double vb = h.v(b);
    acc0 = fma(a0[b], vb, acc0);
    acc1 = fma(a1[b], vb, acc1);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    acc0 += __shfl_xor(acc0, o, 64);
    acc1 += __shfl_xor(acc1, o, 64);
  }
  if (lane == 0) {
    ws.p[s + r0] = tau * acc0;
    if (r1 < n) ws.p[s + r1] = tau * acc1;
  }
}

// A -= v w' + w v' over the trailing matrix of a step, w = p - tau/2 (p'v) v; entries (a, b) and (b, a) get the same bits
__global__ __launch_bounds__(256) void k_wide_rank2(int32_t step, WideWs ws) {
#pragma clang fp contract(off)
  __shared__ double red[256];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int m = ws.ic[WI_M], j = step, s = j + 1, n = m - s;
  if (j >= m || n < 1) return;  // (the whole workgroup)
  const double tau = ws.sc[WS_TAU];
  if (tau == 0.0) return;
  WideRefl h{j < 0 ? nullptr : ws.A + (int64_t)j * m + s, ws.sc[WS_SCALE]};
  const double* p = ws.p + s;
  double dot = 0.0;
  for (int b = tid; b < n; b += 256) dot = fma(p[b], h.v(b), dot);
  dot = fin_fold(dot, red, FinAdd{});
  const double half = 0.5 * tau * dot;
  auto w = [&](int b) { return fma(-half, h.v(b), p[b]); };
  const int r0 = blockIdx.x * WIDE_ROWS + 2 * wv, r1 = r0 + 1;
  if (r0 >= n) return;  // (the wave)
  const bool two = r1 < n;
  double* a0 = ws.A + (int64_t)(s + r0) * m + s;
  double* a1 = ws.A + (int64_t)(s + (two ? r1 : r0)) * m + s;
  const double v0 = h.v(r0), w0 = w(r0), v1 = h.v(two ? r1 : r0), w1 = w(two ? r1 : r0);
  for (int b = lane; b < n; b += 64) {
    const double vb = h.v(b), wb = w(b);
    // (two rounded products and their sum: the same bits with the row and the column exchanged)
    a0[b] = a0[b] - (v0 * wb + w0 * vb);
    if (two) a1[b] = a1[b] - (v1 * wb + w1 * vb);
  }
}

// The tasks' tridiagonal matrices from T = (d, e): task 0 SKAT (T itself), task 1 + j the grid value rho_j (D^1/2 T D^1/2), task
// n_rho + 1 the remainder B (the Schur complement of d_0, order m - 1); with them the Gershgorin interval widened as dstebz widens
// it, pivmin and the absolute tolerance eps |T| (dstebz's default).  A task that is not wanted has order 0.
__global__ __launch_bounds__(256) void k_wide_scale(int32_t k, int32_t n_rho, FinGrid grid, WideWs ws) {
  __shared__ double red[256];
  const int tid = threadIdx.x, task = blockIdx.x, m = ws.ic[WI_M];
  if (m == 0) return;
  const bool isb = task == n_rho + 1;
  const double d0 = ws.d[0], e0 = m > 1 ? ws.e[0] : 0.0, tr = ws.sc[WS_TR];
  int n = m;
  if (task > 0) n = m > 1 ? m : 0;                            // (one marker: every Q_rho is t^2)
  if (isb) n = n_rho > 0 && m > 1 && (double)m * d0 > FIN_FLOOR * tr ? m - 1 : 0;
  double c1 = 1.0, c0 = 1.0;
  if (task > 0 && !isb) {
    const double rho = fmin(grid.rho[task - 1], FIN_RHO_CAP);
    c0 = 1.0 - rho;
    c1 = 1.0 - rho + rho * (double)m;
  }
  auto dd = [&](int i) {
    if (isb) return i == 0 ? ws.d[1] - e0 * e0 / d0 : ws.d[i + 1];
    return i == 0 ? d0 * c1 : ws.d[i] * c0;
  };
  auto ee2 = [&](int i) {                                     // (between i and i + 1)
    if (isb) return ws.e[i + 1] * ws.e[i + 1];
    return i == 0 ? e0 * e0 * (c1 * c0) : ws.e[i] * ws.e[i] * (c0 * c0);
  };
  double *td = ws.td + (int64_t)task * k, *te2 = ws.te2 + (int64_t)task * k;
  double hi = -INFINITY, nlo = -INFINITY, emax = 0.0;
  for (int i = tid; i < n; i += 256) {
    const double d = dd(i), below = i > 0 ? ee2(i - 1) : 0.0, above = i < n - 1 ? ee2(i) : 0.0;
    td[i] = d;
    te2[i] = above;
    const double rad = sqrt(below) + sqrt(above);
    hi = fmax(hi, d + rad);
    nlo = fmax(nlo, rad - d);
    emax = fmax(emax, above);
  }
  hi = fin_fold(hi, red, FinMax{});
  nlo = fin_fold(nlo, red, FinMax{});
  emax = fin_fold(emax, red, FinMax{});
  if (tid == 0) {
    double* rec = ws.tsc + task * WIDE_TSC;
    rec[0] = (double)n;
    if (n > 0) {
      const double eps = 2.220446049250313e-16, lo = -nlo;
      const double pivmin = 2.2250738585072014e-308 * fmax(1.0, emax), tnorm = fmax(fabs(lo), fabs(hi));
      rec[1] = lo - 2.1 * tnorm * eps * (double)n - 4.2 * pivmin;
      rec[2] = hi + 2.1 * tnorm * eps * (double)n + 2.1 * pivmin;
      rec[3] = pivmin;
      rec[4] = eps * tnorm;
    }
  }
}

// Eigenvalue number i of a task, counted from the largest: bisection on the number of eigenvalues <= x (the Sturm count with
// pivmin, as dlaebz counts), until the interval is 2 eps max(|lo|, |hi|) + 2 pivmin + eps |T| wide
__global__ __launch_bounds__(64) void k_wide_eig(int32_t k, WideWs ws, double* __restrict__ lam_out) {
  const int task = blockIdx.y, i = blockIdx.x * 64 + threadIdx.x;
  if (ws.ic[WI_M] == 0) return;
  const double* rec = ws.tsc + task * WIDE_TSC;
  const int n = (int)rec[0];
  if (i >= n) return;
  const double *d = ws.td + (int64_t)task * k, *e2 = ws.te2 + (int64_t)task * k;
  const double pivmin = rec[3], atol = rec[4], eps = 2.220446049250313e-16;
  const int want = n - i;                                     // the smallest x with count(x) >= want
  double lo = rec[1], hi = rec[2];
  bool ok = false;
  for (int it = 0; it < WIDE_BISECT; ++it) {
    if (hi - lo <= 2.0 * eps * fmax(fabs(lo), fabs(hi)) + 2.0 * pivmin + atol) {
      ok = true;
      break;
    }
    const double x = 0.5 * (lo + hi);
    double t = d[0] - x;
    if (fabs(t) < pivmin) t = -pivmin;
    int cnt = t <= 0.0 ? 1 : 0;
    for (int l = 1; l < n; ++l) {
      t = d[l] - e2[l - 1] / t - x;
      if (fabs(t) < pivmin) t = -pivmin;
      cnt += t <= 0.0 ? 1 : 0;
    }
    if (cnt >= want) hi = x; else lo = x;
  }
  const double v = 0.5 * (lo + hi);
  ws.ev[(int64_t)task * k + i] = v;
  if (task == 0 && lam_out) lam_out[i] = v;
  if (!ok) ws.ic[WI_FLAG] = FIN_F_SWEEPS;                     // (every writer stores the same value)
}

// The tails of the mixtures and the SKAT-O tail on the spectra in HBM (descending: what is above a floor is a prefix, the largest
// is the first).  Measured before the spectra were dealt across a wave: a lane per task walked 1 024 eigenvalues per Newton step
// and the tails took 11.4 ms beside a reduction of 16.4 ms.
__global__ __launch_bounds__(256) void k_wide_tails(int32_t k, int32_t n_rho, FinGrid grid, int32_t method, WideWs ws, double* __restrict__ row) {
  __shared__ double prho[8 * FIN_RHO_MAX], sc[64], fm[FIN_RHO_MAX + 2], pts[128], spts[128];
  __shared__ int32_t ic[16], nf[WIDE_TASKS], redi[256];
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wv = tid >> 6, nw = nt >> 6;
  const int m = ws.ic[WI_M];
  if (m == 0) return;  // (the whole workgroup; k_wide_prep wrote the row)
  const double nan = fin_nan();
  const FinTail tail{prho, sc, fm, pts, spts, ic};
  double *qrho = tail.qrho(), *lc1 = tail.lc1(), *lsd = tail.lsd(), *ll = tail.ll();
  const double ws_ = ws.sc[WS_WS], tt = ws.sc[WS_TT], tr = ws.sc[WS_TR];
  // the scalars of the route: s11 = m d0, a'a = m (d0^2 + e0^2), a'Ba = m e0^2 (d1 - e0^2 / d0)
  const double d0 = ws.d[0], e0 = m > 1 ? ws.e[0] : 0.0, d1 = m > 1 ? ws.d[1] : 0.0;
  const double s11e = (double)m * d0, aa = (double)m * (d0 * d0 + e0 * e0);
  const double aba = m > 1 ? fmax((double)m * e0 * e0 * (d1 - e0 * e0 / d0), 0.0) : 0.0;
  // the mixtures: per task the eigenvalues above the floor (B's: none where its largest is not above 1e-10 trace)
  for (int task = 0; task < n_rho + 2; ++task) {
    const int n = (int)ws.tsc[task * WIDE_TSC];
    const double* ev = ws.ev + (int64_t)task * k;
    const double top = n > 0 ? ev[0] : 0.0;
    const bool live = top > 0.0 && (task != n_rho + 1 || top > FIN_FLOOR * tr);
    int c = 0;
    if (live)
      for (int i = tid; i < n; i += nt) c += ev[i] > FIN_FLOOR * top ? 1 : 0;
    c = fin_fold(c, redi, FinAdd{});
    if (tid == 0) nf[task] = c;
  }
  if (tid == 0) {
    ic[FI_FLAG] = ws.ic[WI_FLAG] | ws.ic[WI_SCALED];
    sc[FS_AA] = aa;
    for (int j = 0; j < FIN_RHO_MAX + 2; ++j) fm[j] = 0.0;
  }
  __syncthreads();
  const int nskat = nf[0];
  const bool skato = n_rho > 0 && nskat > 0;
  const bool want_b = skato && m > 1 && (int)ws.tsc[(n_rho + 1) * WIDE_TSC] > 0;
  const int ntask = skato && m > 1 ? n_rho + (want_b ? 1 : 0) : 0;

  // the tails: a WAVE per task, the tasks dealt to the waves in turn, the task's spectrum dealt across the lanes (every lane
  // holds the same numbers; lane 0 stores them)
  for (int j = wv; j < FIN_RHO_MAX + 2; j += nw) {
    if (j == FIN_RHO_MAX + 1) {
      double p = nan;
      bool ok = true;
      if (nskat > 0) {
        const FinLiu liu = fin_liu_params<FinWave>(ws.ev, nskat);
        p = fin_mixture_sf<FinWave>(tt, ws.ev, nskat, ws.ev[0], liu, method, ok);
      }
      if (lane == 0) {
        if (!ok) fm[0] = 1.0;
        sc[FS_SKATP] = p;
      }
    } else if (j < ntask && j < n_rho) {
      const double* ev = ws.ev + (int64_t)(1 + j) * k;
      const int n = nf[1 + j];
      const double rho = fmin(grid.rho[j], FIN_RHO_CAP);
      const double q = (1.0 - rho) * tt + rho * ws_ * ws_;
      double p = nan;
      bool ok = true;
      FinLiu liu{0.0, 0.0, 0.0, 0.0};
      if (n > 0) {
        liu = fin_liu_params<FinWave>(ev, n);
        p = fin_mixture_sf<FinWave>(q, ev, n, ev[0], liu, method, ok);
      }
      if (lane == 0) {
        if (n > 0) {
          if (!ok) fm[1 + j] = 1.0;
          lc1[j] = liu.c1;
          lsd[j] = sqrt(2.0 * liu.c2);
          ll[j] = liu.l;
        }
        prho[j] = p;
        qrho[j] = q;
      }
    } else if (j < ntask && j == n_rho) {
      const double* ev = ws.ev + (int64_t)(n_rho + 1) * k;
      const int n = nf[n_rho + 1];
      const FinMoments b = fin_b_moments<FinWave>(ev, n);
      if (lane == 0) {
        ic[FI_NB] = n;
        sc[FS_MU] = b.mu;
        sc[FS_SD] = sqrt(2.0 * b.l2 + 4.0 * aba / s11e);
        sc[FS_DF] = b.l2 * b.l2 / b.l4;
      }
    }
  }
  __syncthreads();
  if (fin_skato_decide(tail, m, nskat, want_b, n_rho, 0, grid, row)) return;  // (the whole workgroup)
  fin_skato_integral(tail, n_rho, s11e, grid, row);
}

}  // namespace scilmm
