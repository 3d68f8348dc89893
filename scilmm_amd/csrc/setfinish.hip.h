// Kernel of the variant-set finish (scilmm_sets_finish_dev, engine.hip): everything after a Gram block -- the projection of the
// covariates, the weights, the burden numbers, SKAT and SKAT-O -- for the sets of one block, from the block's statistics and its
// Gram matrix where the block left them.  The formulas it shares with the finish of a wide set and with the
// binary-trait kernel -- the small pieces of steps 0 to 3, the special functions, the mixtures' tails, the SKAT-O tail behind step
// 6 -- are in setmath.hip.h; here are the kernel, the secular solver and the LDS sizing.
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
// Steps 0 to 5 and the parts of step 6 that do not look at the score are routines of a whole workgroup on a FinLds (fin_keep,
// fin_form, fin_sums, fin_jacobi, fin_plan, fin_secular, fin_floor_grid, fin_b_task): k_sets_spectra (setpanel.hip.h) runs the
// same ones for a phenotype panel and stops where the trait comes in.
#pragma once
#include "setmath.hip.h"

namespace scilmm {

constexpr int FIN_NT_MAX = 512;     // threads of a workgroup at most
constexpr int FIN_SWEEPS = 40;      // Jacobi sweeps at most
constexpr int FIN_ENTRIES = 32;     // entries of A a thread forms at most (128 * 128 / 512, 64 * 64 / 256)

struct FinSets {
  int32_t start[RPMAX + 1];     // offsets of the sets into the block's columns
  FinGrid grid;
};

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

// The LDS of a set, cut from fin_lds_doubles(cap, nt) doubles.
struct FinLds {
  int cap, ld;                  // the largest set of the block (even), and the matrix's leading dimension cap + 1 (odd: a column is read without bank conflicts)
  double* M;                    // the matrix | the image of z (c x cap) | the secular work space
  double *sv, *wv, *tv, *lam, *cs, *cu, *lamf, *wa;   // s | w | t | lambda (sorted) | c = U'1 (sorted) | c (unsorted) | lambda above the floor | w o scale (cap each, and one spare)
  double* red;                  // nt
  double* rot;                  // cos | sin of the pairs of a step (cap / 2 each)
  double* prho;                 // p_rho | Q_rho | c1 | sd | l | alpha | beta | spare (FIN_RHO_MAX each)
  double* sc;                   // 64 scalars: the tail's (FS_*), then the finish's (S_*)
  double* fm;                   // a root that ran out of steps: SKAT's tail | the grid values' (marks, 0 or 1)
  double *pts, *spts;           // break points, unsorted | sorted (128 each)
  int32_t* idx;                 // the kept markers' columns of the block (cap)
  int32_t *pp, *pq;             // the pairs' indices (cap / 2 each)
  int32_t* ic;                  // 64 integers: the tail's (FI_*), then the finish's (I_*); counts per task
  __device__ __forceinline__ FinTail tail() const { return FinTail{prho, sc, fm, pts, spts, ic}; }
  // task j's rows of the work space over M: poles | weights | eigenvalues
  __device__ __forceinline__ double* poles(int j) const { return M + (3 * j) * cap; }
  __device__ __forceinline__ double* eigs(int j) const { return M + (3 * j + 2) * cap; }
};
enum { S_WS = FS_N, S_TT, S_S11, S_TR, S_S11E, S_ABA };
enum { I_K = FI_N, I_ROT, I_ROOT, I_NSKAT, I_M = 8 + FIN_RHO_MAX + 1, I_NDEF = 8 + 2 * (FIN_RHO_MAX + 1) };

__device__ __forceinline__ FinLds fin_cut(double* lds, int cap, int nt) {
  FinLds L;
  L.cap = cap;
  L.ld = cap + 1;
  L.M = lds;
  L.sv = L.M + fin_image(cap);
  L.wv = L.sv + cap;
  L.tv = L.wv + cap;
  L.lam = L.tv + cap;
  L.cs = L.lam + cap;
  L.cu = L.cs + cap;
  L.lamf = L.cu + cap;
  L.wa = L.lamf + cap;
  L.red = L.sv + 9 * cap;
  L.rot = L.red + nt;
  L.prho = L.rot + cap;
  L.sc = L.prho + 8 * FIN_RHO_MAX;
  L.fm = L.sc + 40;
  L.pts = L.sc + 64;
  L.spts = L.pts + 128;
  L.idx = (int32_t*)(L.spts + 128);
  L.pp = L.idx + cap;
  L.pq = L.pp + cap / 2;
  L.ic = L.pq + cap / 2;
  return L;
}

// 0. the kept markers of the set of columns c0 .. c0 + m - 1: their number (every thread gets it)
__device__ __forceinline__ int fin_keep(const FinLds& L, int32_t r, const double* __restrict__ stats, const double* __restrict__ vscale,
                                        int c0, int m) {
  if (threadIdx.x == 0) {
    int k = 0, scaled = 0;
    for (int j = 0; j < m; ++j) {
      if (fin_kept(stats[c0 + j], stats[2 * (int64_t)r + c0 + j])) {
        L.idx[k++] = c0 + j;
        if (vscale && vscale[c0 + j] != 1.0) scaled = FIN_F_SCALED;
      }
    }
    L.ic[I_K] = k;
    L.ic[FI_FLAG] = scaled;
    L.ic[I_ROOT] = 0;
    for (int j = 0; j < FIN_RHO_MAX + 2; ++j) L.fm[j] = 0.0;
  }
  __syncthreads();
  return L.ic[I_K];
}

// 1. z, s, w, t: a thread per kept marker; the image of z is c x cap in M.  2. A = diag(w) (G - z'z) diag(w): the entries in
// registers, then over the image of z
__device__ __forceinline__ void fin_form(const FinLds& L, int k, int32_t r, int32_t c, const double* __restrict__ stats,
                                         const double* __restrict__ gram, const double* __restrict__ R, const double* __restrict__ u,
                                         int32_t wmode, const double* __restrict__ weights, const double* __restrict__ vscale) {
  const int tid = threadIdx.x, nt = blockDim.x, cap = L.cap, ld = L.ld;
  double* M = L.M;
  const int32_t* idx = L.idx;
  if (tid < k) {
    const int col = idx[tid];
    const double uz = fin_forward(c, R, u, [&](int a) { return stats[(int64_t)(4 + a) * r + col]; }, M, cap, tid);
    const double s = stats[(int64_t)(4 + c) * r + col] - uz;
    const double w = fin_weight(wmode, stats[(int64_t)r + col], weights, col);
    L.sv[tid] = s;
    L.wv[tid] = w;
    L.wa[tid] = vscale ? w * vscale[col] : w;                 // (the weight in A alone: t keeps w)
    L.tv[tid] = w * s;
    L.cu[tid] = 1.0;
  }
  __syncthreads();
  double acc[FIN_ENTRIES];
#pragma unroll
  for (int e = 0; e < FIN_ENTRIES; ++e) {
    const int at = tid + e * nt;
    acc[e] = 0.0;
    if (at < k * k) {
      const int i = at / k, j = at - i * k;
      double zz = 0.0;
      for (int l = 0; l < c; ++l) zz = fma(M[l * cap + i], M[l * cap + j], zz);
      const double kij = fin_kernel_entry(gram[(int64_t)idx[i] * r + idx[j]], gram[(int64_t)idx[j] * r + idx[i]], zz);
      acc[e] = L.wa[i] * kij * L.wa[j];
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
}

// 3. the sums of the burden numbers and Q, to every thread
struct FinSums {
  double s11, ws, tt, tr;       // w'Kw = 1'A1 | 1't | t't | the trace of A
};
__device__ __forceinline__ FinSums fin_sums(const FinLds& L, int k) {
  const int tid = threadIdx.x, ld = L.ld;
  double rs = 0.0;
  if (tid < k)
    for (int j = 0; j < k; ++j) rs += L.M[tid * ld + j];
  FinSums o;
  o.s11 = fin_fold(rs, L.red, FinAdd{});
  o.ws = fin_fold(tid < k ? L.tv[tid] : 0.0, L.red, FinAdd{});
  o.tt = fin_fold(tid < k ? L.tv[tid] * L.tv[tid] : 0.0, L.red, FinAdd{});
  o.tr = fin_fold(tid < k ? L.M[tid * ld + tid] : 0.0, L.red, FinAdd{});
  return o;
}

// 4. two-sided Jacobi: me - 1 steps of me / 2 disjoint pairs per sweep (round robin; me = k rounded up to even, a pair with
// the index k is idle), until a sweep rotates nothing.  A rotation is skipped where |a_pq| <= 1e-18 trace.  Then the eigenvalues
// in descending order with c = U'1 (lam_out: null, or the block's row of them), the positive part and the numbers built on it
// (ic[I_NSKAT], sc[S_S11E], sc[FS_AA], sc[S_ABA]); a barrier at the end.
__device__ __forceinline__ void fin_jacobi(const FinLds& L, int k, double tr, double* __restrict__ lam_out) {
  const int tid = threadIdx.x, nt = blockDim.x, ld = L.ld;
  double *M = L.M, *rot = L.rot, *cu = L.cu, *lam = L.lam, *cs = L.cs, *lamf = L.lamf, *sc = L.sc;
  int32_t *pp = L.pp, *pq = L.pq, *ic = L.ic;
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
    if (!done && tid == 0) ic[FI_FLAG] |= FIN_F_SWEEPS;
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
  if (lam_out && tid < k) lam_out[L.idx[tid]] = lam[tid];
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
    sc[FS_AA] = aa;                                           // a'a, a = A1
    sc[S_ABA] = fmax(a3 - aa * aa / s11e, 0.0);               // a'Ba
  }
  __syncthreads();
}

// What step 4 decides for the steps behind it (every thread reads the same from LDS): the remainder term exists where there is
// more than one marker and a'1 is not rounding; the tasks of step 5 are the grid values and, behind them, the remainder term
struct FinPlan {
  int nskat;
  double s11e;
  bool skato, want_b;
  int ntask;
};
__device__ __forceinline__ FinPlan fin_plan(const FinLds& L, int k, int n_rho, double tr) {
  FinPlan p;
  p.nskat = L.ic[I_NSKAT];
  p.s11e = L.sc[S_S11E];
  p.skato = n_rho > 0 && p.nskat > 0;
  p.want_b = p.skato && k > 1 && p.s11e > FIN_FLOOR * tr;
  p.ntask = p.skato && k > 1 ? n_rho + (p.want_b ? 1 : 0) : 0;
  return p;
}

// 5a. per task (grid value j < n_rho; the remainder term j = n_rho) the reduced rank-one problem: poles in descending order
// with positive weights, equal poles merged (one of them stays an eigenvalue), zero weights taken out.  Rows of the work
// space over M: poles | weights | eigenvalues.  5b. a thread per root; ic[I_ROOT] where one ran out of steps.  A barrier at the end.
__device__ __forceinline__ void fin_secular(const FinLds& L, int k, int n_rho, const FinPlan& plan, const FinGrid& grid) {
  const int tid = threadIdx.x, nt = blockDim.x, cap = L.cap, ntask = plan.ntask;
  const double s11e = plan.s11e;
  double *lam = L.lam, *cs = L.cs, *sc = L.sc;
  int32_t* ic = L.ic;
  const FinTail tail = L.tail();
  double *al = tail.al(), *be = tail.be();
  if (tid < ntask) {
    const int j = tid;
    double *dd = L.poles(j), *ww = dd + cap, *ev = ww + cap;
    const bool isb = j == n_rho;
    const double rho = isb ? 0.0 : fmin(grid.rho[j], FIN_RHO_CAP);
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
  for (int at = tid; at < ntask * cap; at += nt) {
    const int j = at / cap, i = at - j * cap;
    const int mr = ic[I_M + j];
    if (i < mr) {
      const double *dd = L.poles(j), *ww = dd + cap;
      double* ev = L.eigs(j);
      const bool isb = j == n_rho;
      bool ok;
      ev[ic[I_NDEF + j] + i] = fin_secular_root(dd, ww, mr, i, isb ? sc[32] : al[j], isb ? sc[33] : be[j], ok);
      if (!ok) ic[I_ROOT] = 1;                                // (every writer stores the same value)
    }
  }
  __syncthreads();
}

// 6, before the score comes in (a lane each).  A grid value's spectrum: the eigenvalues above the floor moved to the front of
// ev (the list is not sorted); their number, and the largest in `top`
__device__ __forceinline__ int fin_floor_grid(double* ev, int k, double& top) {
  top = 0.0;
  for (int i = 0; i < k; ++i) top = fmax(top, ev[i]);
  int nf = 0;
  for (int i = 0; i < k; ++i) {
    const double v = ev[i];
    if (v > FIN_FLOOR * top) ev[nf++] = v;
  }
  return nf;
}

// ... the remainder term: the eigenvalues of B are minus the roots; those above the floor (none where the largest is rounding)
// and their moments: ic[FI_NB], sc[FS_MU], sc[FS_SD], sc[FS_DF]
__device__ __forceinline__ void fin_b_task(const FinLds& L, double* ev, int k, double tr, double s11e) {
  double top = 0.0;
  for (int i = 0; i < k; ++i) {
    ev[i] = -ev[i];
    top = fmax(top, ev[i]);
  }
  int nf = 0;
  if (top > FIN_FLOOR * tr)
    for (int i = 0; i < k; ++i) {
      const double v = ev[i];
      if (v > FIN_FLOOR * top) ev[nf++] = v;
    }
  const FinMoments b = fin_b_moments<FinSerial>(ev, nf);
  L.ic[FI_NB] = nf;
  L.sc[FS_MU] = b.mu;
  L.sc[FS_SD] = sqrt(2.0 * b.l2 + 4.0 * L.sc[S_ABA] / s11e);
  L.sc[FS_DF] = b.l2 * b.l2 / b.l4;
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
  const double nan = fin_nan();
  const FinLds L = fin_cut(fin_lds, cap, nt);
  double *lamf = L.lamf, *prho = L.prho, *sc = L.sc, *fm = L.fm;
  int32_t* ic = L.ic;
  const FinTail tail = L.tail();
  double *qrho = tail.qrho(), *lc1 = tail.lc1(), *lsd = tail.lsd(), *ll = tail.ll();

  double* row = out + (int64_t)set * ld_out;

  // 0. the kept markers
  const int k = fin_keep(L, r, stats, vscale, c0, m);
  if (lam_out && tid < m) lam_out[c0 + tid] = nan;          // (the kept markers' slots are written again in step 4)
  if (k == 0) {
    if (tid == 0) fin_empty_row(row, n_rho);
    return;  // (the whole workgroup)
  }

  // 1. z, s, w, t; 2. A
  fin_form(L, k, r, c, stats, gram, R, u, wmode, weights, vscale);

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

  // 4. the eigendecomposition; 5. the spectra of the grid values and of the remainder term
  fin_jacobi(L, k, tr, lam_out);
  const FinPlan plan = fin_plan(L, k, n_rho, tr);
  const int nskat = plan.nskat, ntask = plan.ntask;
  const double s11e = plan.s11e;
  fin_secular(L, k, n_rho, plan, sets.grid);

  // 6. the tails: a lane per task, the tasks dealt to the waves in turn.  Task n_rho + 1 is SKAT's own p-value.
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
