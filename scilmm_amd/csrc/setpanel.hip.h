// Kernels of the variant-set finish for a phenotype panel (scilmm_sets_finish_panel_dev, engine.hip): the
// sets of one Gram block against the t traits whose scores X'Y~ scilmm_scan_panel_dev left behind the block.  Everything of the
// finish but the score is the same for every trait, so it is computed once per set and kept as a record in HBM:
//   k_sets_spectra    : one workgroup per set, the LDS and the threads of k_sets_finish.  Steps 0 to 5 of k_sets_finish by the
//                       routines of setfinish.hip.h (there is no u: the traits arrive projected off the whitened covariates;
//                       z is still needed for K), then what step 6 does before it looks at Q: the floor of every spectrum, the
//                       Liu numbers of SKAT's and of every grid value's, the moments of the remainder term.  The record is
//                       written with plain stores; the set's head row (n_used, w'Kw, the flags so far) goes to the caller.
//   k_sets_panel_tail : grid (set, trait group), PT_NT threads.  The set's record is loaded into LDS once (at most
//                       (n_rho + 2) cap doubles, the head and the tail's state); then for the traits of the group
//                         a. a wave per trait: t = w o s / sqrt(scale_t) from the kept rows of the trait's column of X'Y~, and
//                            the sums 1'(w o s), 1't, t't, lane l the entries l, l + 64, ..., folded by FinWave's butterfly;
//                         b. a lane per (trait, tail): SKAT's own and the grid values', fin_mixture_sf as k_sets_finish calls it;
//                         c. trait by trait, the whole workgroup: fin_skato_decide and fin_skato_integral of setmath.hip.h on a
//                            row in LDS, of which thread 0 copies the trait's eight numbers out.
// No atomics.  The numbers of a (set, trait) pair depend on the set's inputs and the trait's column alone: every sum has a fixed
// order that neither t, nor the group size, nor the set's place in the block enters.
#pragma once
#include "setfinish.hip.h"

namespace scilmm {

constexpr int PT_NT = 256;          // threads of k_sets_panel_tail
constexpr int PT_GROUP_MAX = 32;    // traits of a group at most
constexpr int PT_TMAX = 4096;       // traits of a call at most (PANEL_TMAX)
constexpr int PT_HEAD = 4;          // doubles of a set's head row: n_used | w'Kw | flags | 0
constexpr int PT_OUT = 8;           // doubles of a (set, trait) row: 1'(w o s) | burden_chi2 | skat_q | skat_p | skato_p | skato_pmin | skato_rho | flags

// A set's record: PR_HEAD scalars, then four sections of cap doubles (the grid's n_rho times): the kept columns | w | SKAT's
// spectrum above the floor | the grid values' spectra above the floor, cap apart
enum {
  PR_K = 0, PR_NSKAT, PR_WANT_B, PR_FLAGS, PR_S11, PR_S11E, PR_AA, PR_NGRID,   // kept | ... | w'Kw | 1'A1 in the eigenbasis | a'a | grid values with a spectrum (n_rho or 0)
  PR_MU, PR_SD, PR_DF, PR_NB,                                                   // the remainder term
  PR_C1, PR_C2, PR_L,                                                           // the Liu numbers of SKAT's spectrum
  PR_GRID = 16                                                                  // per grid value PR_PER doubles: n above the floor | the largest | c1 | c2 | l
};
constexpr int PR_PER = 5;
constexpr int PR_HEAD = PR_GRID + PR_PER * FIN_RHO_MAX;
__host__ __device__ constexpr int64_t rec_doubles(int cap, int n_rho) { return PR_HEAD + (int64_t)(3 + n_rho) * cap; }

// per trait of a group, in LDS: the three sums, SKAT's tail, then p | Q | a mark where the tail's root ran out of steps per grid value
enum { PG_WSU = 0, PG_WS, PG_TT, PG_SKATP, PG_SKATM, PG_P = 6, PG_Q = PG_P + FIN_RHO_MAX, PG_M = PG_Q + FIN_RHO_MAX, PG_N = PG_M + FIN_RHO_MAX };
constexpr int PT_ROW = FIN_HEAD + FIN_RHO_MAX;    // the row fin_skato_decide and fin_skato_integral write
__host__ __device__ constexpr int ptail_lds_doubles(int cap, int n_rho, int group) {
  return PR_HEAD + (2 + n_rho) * cap + 8 * FIN_RHO_MAX + 64 + 2 * 128 + PT_ROW + FIN_RHO_MAX + group * PG_N + (cap + 16) / 2 + 8;
}

// stats, gram, R, sets, wmode, weights, cap: as k_sets_finish takes them (the score row of stats is not read); rec: n_sets records,
// ld_rec >= rec_doubles(cap, n_rho) apart; head: n_sets rows of PT_HEAD doubles
__global__ __launch_bounds__(FIN_NT_MAX) void k_sets_spectra(int32_t r, int32_t c, const double* __restrict__ stats,
                                                             const double* __restrict__ gram, const double* __restrict__ R, FinSets sets,
                                                             int32_t wmode, const double* __restrict__ weights, int32_t n_rho,
                                                             int32_t cap, double* __restrict__ rec_all, int64_t ld_rec,
                                                             double* __restrict__ head_all) {
  extern __shared__ double fin_lds[];
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wv = tid >> 6, nw = nt >> 6;
  const int set = blockIdx.x;
  const int c0 = sets.start[set], m = sets.start[set + 1] - c0;
  const FinLds L = fin_cut(fin_lds, cap, nt);
  double* rec = rec_all + (int64_t)set * ld_rec;
  double* head = head_all + (int64_t)set * PT_HEAD;
  double* grid_rec = rec + PR_GRID;

  // u = 0: c zeros where step 1 reads u (the fold of step 3 is the first to write there)
  if (tid < FIN_CMAX) L.red[tid] = 0.0;
  const int k = fin_keep(L, r, stats, nullptr, c0, m);
  if (k == 0) {
    if (tid == 0) {
      rec[PR_K] = 0.0;
      head[0] = 0.0;
      head[1] = fin_nan();
      head[2] = 0.0;
      head[3] = 0.0;
    }
    return;  // (the whole workgroup)
  }
  // (the score row of the statistics is not read: with u = 0, s is the row's own entry, and it is not a trait of the panel)
  fin_form(L, k, r, c, stats, gram, R, L.red, wmode, weights, nullptr);
  {
    const FinSums o = fin_sums(L, k);
    if (tid == 0) {
      L.sc[S_S11] = o.s11;
      L.sc[S_TR] = o.tr;
    }
  }
  __syncthreads();
  const double tr = L.sc[S_TR];
  fin_jacobi(L, k, tr, nullptr);
  const FinPlan plan = fin_plan(L, k, n_rho, tr);
  fin_secular(L, k, n_rho, plan, sets.grid);
  const int ngrid = plan.ntask > 0 ? n_rho : 0;

  // 6, before the score comes in: a lane per task, dealt to the waves as k_sets_finish deals them
  for (int j = wv; j < FIN_RHO_MAX + 2; j += nw) {
    if (lane != 0) continue;
    if (j == FIN_RHO_MAX + 1) {
      if (plan.nskat > 0) {
        const FinLiu liu = fin_liu_params<FinSerial>(L.lamf, plan.nskat);
        rec[PR_C1] = liu.c1;
        rec[PR_C2] = liu.c2;
        rec[PR_L] = liu.l;
      }
    } else if (j < ngrid) {
      double* ev = L.eigs(j);
      double top;
      const int nf = fin_floor_grid(ev, k, top);
      double* g = grid_rec + PR_PER * j;
      g[0] = (double)nf;
      g[1] = top;
      if (nf > 0) {
        const FinLiu liu = fin_liu_params<FinSerial>(ev, nf);
        g[2] = liu.c1;
        g[3] = liu.c2;
        g[4] = liu.l;
      }
      L.ic[I_M + j] = nf;                                     // (the count of step 5 is no longer needed)
    } else if (j < plan.ntask && j == n_rho) {
      fin_b_task(L, L.eigs(j), k, tr, plan.s11e);
    }
  }
  __syncthreads();
  if (tid == 0) {
    const int flags = L.ic[FI_FLAG] | (L.ic[I_ROOT] ? FIN_F_ROOT : 0);
    rec[PR_K] = (double)k;
    rec[PR_NSKAT] = (double)plan.nskat;
    rec[PR_WANT_B] = plan.want_b ? 1.0 : 0.0;
    rec[PR_FLAGS] = (double)flags;
    rec[PR_S11] = L.sc[S_S11];
    rec[PR_S11E] = plan.s11e;
    rec[PR_AA] = L.sc[FS_AA];
    rec[PR_NGRID] = (double)ngrid;
    const bool b = plan.want_b;
    rec[PR_MU] = b ? L.sc[FS_MU] : 0.0;
    rec[PR_SD] = b ? L.sc[FS_SD] : 0.0;
    rec[PR_DF] = b ? L.sc[FS_DF] : 0.0;
    rec[PR_NB] = b ? (double)L.ic[FI_NB] : 0.0;
    head[0] = (double)k;
    head[1] = L.sc[S_S11];
    head[2] = (double)flags;
    head[3] = 0.0;
  }
  double *cols = rec + PR_HEAD, *w = cols + cap, *lamf = w + cap, *spec = lamf + cap;
  if (tid < k) {
    cols[tid] = (double)L.idx[tid];
    w[tid] = L.wv[tid];
    if (tid < plan.nskat) lamf[tid] = L.lamf[tid];
  }
  for (int at = tid; at < ngrid * cap; at += nt) {
    const int j = at / cap, i = at - j * cap;
    if (i < L.ic[I_M + j]) spec[at] = L.eigs(j)[i];
  }
}

// T, the degenerate rule and the integral of one trait, by the whole workgroup behind a barrier.  Out of line: inside the loop
// over a group's traits the inlined pair costs the kernel its registers (256 and 1.5 KB of scratch, against 169 and none).
__device__ __noinline__ void ptail_skato(FinTail tail, int k, int nskat, bool want_b, int n_rho, double s11e, const FinGrid& grid, double* row) {
  if (!fin_skato_decide(tail, k, nskat, want_b, n_rho, 0, grid, row)) fin_skato_integral(tail, n_rho, s11e, grid, row);
}

// rec: the records k_sets_spectra wrote; xty: r x t scores, ld_xty apart (row = the block's column, column = the trait);
// tscale: t scales or null (all 1); group: traits per workgroup, 1 .. PT_GROUP_MAX; out: n_sets t rows of PT_OUT doubles, row =
// set t + trait
__global__ __launch_bounds__(PT_NT, 2) void k_sets_panel_tail(int32_t cap, int32_t n_rho, FinGrid grid, int32_t method,
                                                           const double* __restrict__ rec_all, int64_t ld_rec,
                                                           const double* __restrict__ xty, int64_t ld_xty, int32_t t,
                                                           const double* __restrict__ tscale, int32_t group, double* __restrict__ out) {
  extern __shared__ double pt_lds[];
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wv = tid >> 6, nw = nt >> 6;
  const int set = blockIdx.x, g0 = blockIdx.y * group;
  const int ng = min(group, t - g0);
  const double* __restrict__ rec = rec_all + (int64_t)set * ld_rec;
  const double nan = fin_nan();
  double* orow = out + ((int64_t)set * t + g0) * PT_OUT;

  const int k = (int)rec[PR_K];
  if (k == 0) {
    // a set with nothing left: the convention of fin_empty_row
    for (int at = tid; at < ng * PT_OUT; at += nt) orow[at] = (at % PT_OUT) == PT_OUT - 1 ? 0.0 : nan;
    return;  // (the whole workgroup)
  }

  double* hd = pt_lds;                          // the record's head
  double* w = hd + PR_HEAD;                     // cap
  double* lamf = w + cap;                       // cap
  double* spec = lamf + cap;                    // n_rho x cap
  double* prho = spec + n_rho * cap;            // the tail's state, as k_sets_finish lays it out
  double* sc = prho + 8 * FIN_RHO_MAX;
  double* fm = sc + 40;
  double* pts = sc + 64;
  double* spts = pts + 128;
  double* row = spts + 128;                     // PT_ROW
  double* rhol = row + PT_ROW;                  // the grid (FIN_RHO_MAX)
  double* pg = rhol + FIN_RHO_MAX;              // group x PG_N
  int32_t* cols = (int32_t*)(pg + group * PG_N);   // cap
  int32_t* ic = cols + cap;                     // 16
  const FinTail tail{prho, sc, fm, pts, spts, ic};

  for (int i = tid; i < PR_HEAD; i += nt) hd[i] = rec[i];
  if (tid < FIN_RHO_MAX) rhol[tid] = tid < n_rho ? grid.rho[tid] : 0.0;   // (the grid in LDS: part c reads it there as a FinGrid)
  const int nskat = (int)rec[PR_NSKAT], ngrid = (int)rec[PR_NGRID];
  {
    const double *rc = rec + PR_HEAD, *rw = rc + cap, *rl = rw + cap, *rs = rl + cap;
    for (int i = tid; i < k; i += nt) {
      cols[i] = (int32_t)rc[i];
      w[i] = rw[i];
      if (i < nskat) lamf[i] = rl[i];
    }
    for (int at = tid; at < ngrid * cap; at += nt) {
      const int j = at / cap, i = at - j * cap;
      if (i < (int)rec[PR_GRID + PR_PER * j]) spec[at] = rs[at];
    }
  }
  __syncthreads();
  const bool want_b = hd[PR_WANT_B] != 0.0;
  const double s11 = hd[PR_S11], s11e = hd[PR_S11E];

  // a. the sums of a trait: a wave each
  for (int g = wv; g < ng; g += nw) {
    const int col = g0 + g;
    const double sq = tscale ? sqrt(tscale[col]) : 1.0;
    double a = 0.0, b = 0.0, q = 0.0;
    for (int i = FinWave::first(); i < k; i += FinWave::stride) {
      const double wsi = w[i] * xty[(int64_t)cols[i] * ld_xty + col], ti = wsi / sq;
      a += wsi;
      b += ti;
      q += ti * ti;
    }
    a = FinWave::total(a);
    b = FinWave::total(b);
    q = FinWave::total(q);
    if (lane == 0) {
      double* p = pg + g * PG_N;
      p[PG_WSU] = a;
      p[PG_WS] = b;
      p[PG_TT] = q;
    }
  }
  __syncthreads();

  // b. the tails: a lane per (trait, tail); tail ngrid is SKAT's own
  const int ntail = ngrid + 1;
  for (int at = tid; at < ng * ntail; at += nt) {
    const int g = at / ntail, j = at - g * ntail;
    double* p = pg + g * PG_N;
    const double ws = p[PG_WS], tt = p[PG_TT];
    bool ok = true;
    double pv = nan;
    if (j == ngrid) {
      if (nskat > 0) {
        const FinLiu liu{hd[PR_C1], hd[PR_C2], sqrt(hd[PR_L]), hd[PR_L]};
        pv = fin_mixture_sf<FinSerial>(tt, lamf, nskat, lamf[0], liu, method, ok);
      }
      p[PG_SKATP] = pv;
      p[PG_SKATM] = ok ? 0.0 : 1.0;
    } else {
      const double* g5 = hd + PR_GRID + PR_PER * j;
      const int nf = (int)g5[0];
      const double rho = fmin(rhol[j], FIN_RHO_CAP);             // (j differs from lane to lane: from LDS, not from the argument)
      const double q = (1.0 - rho) * tt + rho * ws * ws;
      if (nf > 0) {
        const FinLiu liu{g5[2], g5[3], sqrt(g5[4]), g5[4]};
        pv = fin_mixture_sf<FinSerial>(q, spec + j * cap, nf, g5[1], liu, method, ok);   // (the list is not sorted)
      }
      p[PG_P + j] = pv;
      p[PG_Q + j] = q;
      p[PG_M + j] = ok ? 0.0 : 1.0;
    }
  }
  __syncthreads();

  // c. trait by trait: the state fin_skato_decide expects, T and the degenerate rule, the integral, the trait's row
  for (int g = 0; g < ng; ++g) {
    const double* p = pg + g * PG_N;
    if (tid < FIN_RHO_MAX + 2) fm[tid] = 0.0;
    __syncthreads();
    if (tid < ngrid) {
      const double* g5 = hd + PR_GRID + PR_PER * tid;
      prho[tid] = p[PG_P + tid];
      tail.qrho()[tid] = p[PG_Q + tid];
      fm[1 + tid] = p[PG_M + tid];
      if ((int)g5[0] > 0) {
        tail.lc1()[tid] = g5[2];
        tail.lsd()[tid] = sqrt(2.0 * g5[3]);
        tail.ll()[tid] = g5[4];
      }
    }
    if (tid == 0) {
      fm[0] = p[PG_SKATM];
      sc[FS_SKATP] = p[PG_SKATP];
      sc[FS_MU] = hd[PR_MU];
      sc[FS_SD] = hd[PR_SD];
      sc[FS_DF] = hd[PR_DF];
      sc[FS_AA] = hd[PR_AA];
      ic[FI_NB] = (int)hd[PR_NB];
      ic[FI_FLAG] = (int)hd[PR_FLAGS];
    }
    __syncthreads();
    ptail_skato(tail, k, nskat, want_b, n_rho, s11e, *(const FinGrid*)rhol, row);
    if (tid == 0) {                             // (the thread that wrote the row)
      double* o = orow + g * PT_OUT;
      const double ws = p[PG_WS];
      o[0] = p[PG_WSU];
      o[1] = ws * ws / s11;
      o[2] = p[PG_TT];
      o[3] = row[5];
      o[4] = row[6];
      o[5] = row[7];
      o[6] = row[8];
      o[7] = row[9];
    }
    __syncthreads();
  }
}

}  // namespace scilmm
