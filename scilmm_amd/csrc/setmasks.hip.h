// Kernel of the variant-set finish under annotation masks and MAF cutoffs (scilmm_sets_finish_masks_dev, engine.hip; DESIGN.md
// section 25): the sets of one Gram block, each under n_ann annotation masks crossed with n_cut cutoffs of the minor allele
// frequency.  Every cell of a set is a principal submatrix of the set's K and a sub-vector of its score, so the block's
// statistics and Gram matrix are read where they lie and nothing is swept again.
//   k_sets_finish_masks : one workgroup per (set, annotation, cutoff), the threads and the LDS of k_sets_finish (sized by the
//                         block's largest set).  Step 0 keeps the cell's markers: what fin_kept keeps AND bit a of the column's
//                         annotation word AND maf <= cut; steps 1 to 7 are those of k_sets_finish on that index list, by the same
//                         routines (fin_form, fin_sums, fin_jacobi, fin_plan, fin_secular, the tails, fin_skato_decide,
//                         fin_skato_integral), so the first 10 + n_rho numbers of a cell are the bits k_sets_finish gives for a
//                         block that holds the cell's markers alone.  Between steps 3 and 4, while A = diag(w) K diag(w) is still
//                         in LDS, ACAT-V (Liu et al. 2019, in STAAR's form) is taken from t = w o s, diag(A) and the pool's
//                         corner of A; its work space is `lamf` and the fold, both free until step 4.
// ACAT-V never divides by a weight: s_j^2 / K_jj = t_j^2 / A_jj wherever w_j != 0, a marker with w_j = 0 has omega_j = 0 and is
// left out, and the pool's numbers are sums of t and of A as they stand.
// No atomics; every sum runs in ascending column order or by the fixed fold: a cell's numbers depend on its own inputs alone.
#pragma once
#include "setfinish.hip.h"

namespace scilmm {

constexpr int MASK_ANN_MAX = 32;    // annotations at most (the bits of a column's word)
constexpr int MASK_CUT_MAX = 8;     // MAF cutoffs at most
constexpr int MASK_TAIL = 2;        // doubles of a cell's row behind the row of k_sets_finish: acatv_p | n_pooled
constexpr double ACAT_TINY = 1e-15; // below it tan((0.5 - p) pi) is 1 / (p pi); p is capped at 1 - ACAT_TINY
constexpr double ACAT_HUGE = 1e15;  // above it 0.5 - atan(T) / pi is 1 / (T pi)
constexpr double ACAT_PI = 3.14159265358979323846;

// the cutoffs, a kernel argument by value
struct FinCuts {
  double cut[MASK_CUT_MAX];
};

// the minor allele frequency from a column's mean: the expression of fin_weight's mode 0 and of scilmm_amd.set_masks.maf_of
__device__ __forceinline__ double fin_maf(double mean) { return fmin(0.5 * mean, 1.0 - 0.5 * mean); }

// 0. fin_keep for a cell: the kept markers of columns c0 .. c0 + m - 1 that carry `bit` in their annotation word and whose
// minor allele frequency is at most `cut`; their number (every thread gets it)
__device__ __forceinline__ int fin_keep(const FinLds& L, int32_t r, const double* __restrict__ stats, const uint32_t* __restrict__ ann,
                                        uint32_t bit, double cut, int c0, int m) {
  if (threadIdx.x == 0) {
    int k = 0;
    for (int j = 0; j < m; ++j) {
      const int col = c0 + j;
      if (fin_kept(stats[col], stats[2 * (int64_t)r + col]) && (ann[col] & bit) != 0u && fin_maf(stats[(int64_t)r + col]) <= cut)
        L.idx[k++] = col;
    }
    L.ic[I_K] = k;
    L.ic[FI_FLAG] = 0;
    L.ic[I_ROOT] = 0;
    for (int j = 0; j < FIN_RHO_MAX + 2; ++j) L.fm[j] = 0.0;
  }
  __syncthreads();
  return L.ic[I_K];
}

// a term of the Cauchy combination: tan((0.5 - p) pi), p capped at 1 - ACAT_TINY; 1 / (p pi) below ACAT_TINY (infinite at p = 0).
// Below 0.5 the tangent is taken as 1 / tan(p pi), the same function without the cancellation in 0.5 - p (which would cost a
// small p its leading digits, and the branch at ACAT_TINY its continuity); scilmm_amd.set_masks.cauchy_term is the host twin.
__device__ __forceinline__ double fin_cauchy_term(double p) {
  p = fmin(p, 1.0 - ACAT_TINY);
  if (p < ACAT_TINY) return 1.0 / (p * ACAT_PI);
  return p < 0.5 ? 1.0 / tan(p * ACAT_PI) : tan((0.5 - p) * ACAT_PI);
}

// ... and the p-value of the combined statistic: 0.5 - atan(T) / pi, 1 / (T pi) above ACAT_HUGE; above 1 it is taken as
// atan(1 / T) / pi, again the same function without the cancellation
__device__ __forceinline__ double fin_cauchy_sf(double T) {
  if (T > ACAT_HUGE) return 1.0 / (T * ACAT_PI);
  return T > 1.0 ? atan(1.0 / T) / ACAT_PI : 0.5 - atan(T) / ACAT_PI;
}

// ACAT-V of the cell, by the whole workgroup behind step 3 (A in M, t in tv, w in wv; lamf and the fold are free): a marker with
// minor allele count 2 n_obs maf > acat_mac is a term of its own, p = erfc(sqrt(t^2 / 2 A_jj)) with the weight omega = w^2 maf
// (1 - maf), where A_jj > 0; the others are pooled into one burden term, p = erfc(sqrt((1't)^2 / 2 1'A1)) over the pool with the
// mean of their omega, where 1'A1 > 0.  Terms of weight 0 are left out.  Thread 0 writes acatv_p | n_pooled; a barrier at the end
// (the last fold's).
__device__ __forceinline__ void fin_acatv(const FinLds& L, int k, int32_t r, const double* __restrict__ stats, double acat_mac,
                                          double* __restrict__ tail2) {
  const int tid = threadIdx.x, ld = L.ld;
  double om = 0.0, num = 0.0, den = 0.0;
  bool pooled = false;
  if (tid < k) {
    const int col = L.idx[tid];
    const double maf = fin_maf(stats[(int64_t)r + col]), mac = 2.0 * stats[col] * maf, w = L.wv[tid];
    om = w * w * maf * (1.0 - maf);
    pooled = mac <= acat_mac;
    L.lamf[tid] = pooled ? 1.0 : 0.0;
    const double a = L.M[tid * ld + tid], t = L.tv[tid];
    if (!pooled && a > 0.0 && om > 0.0) {
      num = om * fin_cauchy_term(erfc(sqrt(0.5 * (t * t) / a)));
      den = om;
    }
  }
  __syncthreads();
  double rs = 0.0;                                            // the pool's corner of A: a row each, in ascending column order
  if (pooled)
    for (int j = 0; j < k; ++j)
      if (L.lamf[j] != 0.0) rs += L.M[tid * ld + j];
  const double npool = fin_fold(pooled ? 1.0 : 0.0, L.red, FinAdd{});
  const double pws = fin_fold(pooled ? L.tv[tid] : 0.0, L.red, FinAdd{});
  const double pq = fin_fold(rs, L.red, FinAdd{});
  const double pom = fin_fold(pooled ? om : 0.0, L.red, FinAdd{});
  num = fin_fold(num, L.red, FinAdd{});
  den = fin_fold(den, L.red, FinAdd{});
  if (tid == 0) {
    if (npool > 0.0 && pq > 0.0) {
      const double omp = pom / npool;
      if (omp > 0.0) {
        num += omp * fin_cauchy_term(erfc(sqrt(0.5 * (pws * pws) / pq)));
        den += omp;
      }
    }
    tail2[0] = den > 0.0 ? fin_cauchy_sf(num / den) : fin_nan();
    tail2[1] = npool;
  }
}

// stats, gram, R, u, sets, wmode, weights, method, n_rho, cap: as k_sets_finish takes them; ann: r annotation words; cuts: the
// n_cut cutoffs by value; out: n_sets n_ann n_cut rows of ld_out >= FIN_HEAD + n_rho + MASK_TAIL doubles, row = blockIdx.x =
// (set n_ann + a) n_cut + f
__global__ __launch_bounds__(FIN_NT_MAX) void k_sets_finish_masks(int32_t r, int32_t c, const double* __restrict__ stats,
                                                                  const double* __restrict__ gram, const double* __restrict__ R,
                                                                  const double* __restrict__ u, FinSets sets, int32_t wmode,
                                                                  const double* __restrict__ weights, int32_t method, int32_t n_rho,
                                                                  int32_t cap, const uint32_t* __restrict__ ann, int32_t n_ann,
                                                                  FinCuts cuts, int32_t n_cut, double acat_mac,
                                                                  double* __restrict__ out, int64_t ld_out) {
  extern __shared__ double fin_lds[];
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wv = tid >> 6, nw = nt >> 6;
  const int ncell = n_ann * n_cut;
  const int set = blockIdx.x / ncell, cell = blockIdx.x - set * ncell, a = cell / n_cut, f = cell - a * n_cut;
  const int c0 = sets.start[set], m = sets.start[set + 1] - c0;
  const double nan = fin_nan();
  const FinLds L = fin_cut(fin_lds, cap, nt);
  double *lamf = L.lamf, *prho = L.prho, *sc = L.sc, *fm = L.fm;
  int32_t* ic = L.ic;
  const FinTail tail = L.tail();
  double *qrho = tail.qrho(), *lc1 = tail.lc1(), *lsd = tail.lsd(), *ll = tail.ll();

  double* row = out + (int64_t)blockIdx.x * ld_out;

  // 0. the cell's markers
  const int k = fin_keep(L, r, stats, ann, 1u << a, cuts.cut[f], c0, m);
  if (k == 0) {
    if (tid == 0) {
      fin_empty_row(row, n_rho);
      row[FIN_HEAD + n_rho] = nan;
      row[FIN_HEAD + n_rho + 1] = 0.0;
    }
    return;  // (the whole workgroup)
  }

  // 1. z, s, w, t; 2. A
  fin_form(L, k, r, c, stats, gram, R, u, wmode, weights, nullptr);

  // 3. the burden numbers and Q
  {
    const FinSums o = fin_sums(L, k);
    if (tid == 0) {
      sc[S_WS] = o.ws;
      sc[S_TT] = o.tt;
      sc[S_S11] = o.s11;
      sc[S_TR] = o.tr;
      row[0] = (double)k;
      row[1] = o.ws / o.s11;
      row[2] = 1.0 / sqrt(o.s11);
      row[3] = o.ws * o.ws / o.s11;
      row[4] = o.tt;
    }
  }
  __syncthreads();
  const double ws = sc[S_WS], tt = sc[S_TT], tr = sc[S_TR];

  // ACAT-V, before step 4 overwrites A
  fin_acatv(L, k, r, stats, acat_mac, row + FIN_HEAD + n_rho);

  // 4. the eigendecomposition; 5. the spectra of the grid values and of the remainder term
  fin_jacobi(L, k, tr, nullptr);
  const FinPlan plan = fin_plan(L, k, n_rho, tr);
  const int nskat = plan.nskat, ntask = plan.ntask;
  const double s11e = plan.s11e;
  fin_secular(L, k, n_rho, plan, sets.grid);

  // 6. the tails, task by task as k_sets_finish deals them (its loop, statement by statement: the bits are its bits)
  for (int j = wv; j < FIN_RHO_MAX + 2; j += nw) {
    if (lane != 0) continue;
    if (j == FIN_RHO_MAX + 1) {
      double p = nan;
      if (nskat > 0) {
        const FinLiu liu = fin_liu_params<FinSerial>(lamf, nskat);
        bool ok;
        p = fin_mixture_sf<FinSerial>(tt, lamf, nskat, lamf[0], liu, method, ok);
        if (!ok) fm[0] = 1.0;
      }
      sc[FS_SKATP] = p;
    } else if (j < ntask && j < n_rho) {
      double* ev = L.eigs(j);
      double top;
      const int nf = fin_floor_grid(ev, k, top);
      const double rho = fmin(sets.grid.rho[j], FIN_RHO_CAP);
      const double q = (1.0 - rho) * tt + rho * ws * ws;
      double p = nan;
      if (nf > 0) {
        const FinLiu liu = fin_liu_params<FinSerial>(ev, nf);
        bool ok;
        p = fin_mixture_sf<FinSerial>(q, ev, nf, top, liu, method, ok);   // (the list is not sorted)
        if (!ok) fm[1 + j] = 1.0;
        lc1[j] = liu.c1;
        lsd[j] = sqrt(2.0 * liu.c2);
        ll[j] = liu.l;
      }
      prho[j] = p;
      qrho[j] = q;
    } else if (j < ntask && j == n_rho) {
      fin_b_task(L, L.eigs(j), k, tr, s11e);
    }
  }
  __syncthreads();
  // T, its first minimiser, the degenerate rule; then 7. the SKAT-O integral
  if (fin_skato_decide(tail, k, nskat, plan.want_b, n_rho, ic[I_ROOT] ? FIN_F_ROOT : 0, sets.grid, row)) return;  // (the whole workgroup)
  fin_skato_integral(tail, n_rho, s11e, sets.grid, row);
}

}  // namespace scilmm
