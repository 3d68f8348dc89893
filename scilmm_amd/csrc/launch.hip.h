// Typed launchers of the numeric phase (included by engine.hip only, behind struct scilmm_factor).
//
// One function per kernel family: it picks the template instantiation (matrix-core or scalar, atomic or plain, ...) ONCE,
// takes only what differs between its call sites, cuts its grid at max_groups() and -- where the variant it launches sums
// with floating-point atomics -- counts the launch in Dev::n_float_atomic (scilmm_timing.n_float_atomic_launches: what the
// deterministic-mode tests read).  An empty list launches nothing.  Kernels with one call site and one variant (k_potrf,
// k_assemble, k_shadow, ...) are launched where they are used.
#pragma once

namespace {

// the kernels that take more dynamic LDS than a launch gets by default: once per handle
int set_attrs(scilmm_symbolic* sym, Dev* D) {
  if (D->attrs_set) return SCILMM_OK;
  const int big = 150 * 1024;
  HIPCHK(hipFuncSetAttribute((const void*)k_potrf, hipFuncAttributeMaxDynamicSharedMemorySize, big));
  HIPCHK(hipFuncSetAttribute((const void*)k_fwd<true, 0, true>, hipFuncAttributeMaxDynamicSharedMemorySize, big));
  HIPCHK(hipFuncSetAttribute((const void*)k_fwd<true, 0, false>, hipFuncAttributeMaxDynamicSharedMemorySize, big));
  HIPCHK(hipFuncSetAttribute((const void*)k_fwd<true, 1, true>, hipFuncAttributeMaxDynamicSharedMemorySize, big));
  HIPCHK(hipFuncSetAttribute((const void*)k_fwd<false, 0, true>, hipFuncAttributeMaxDynamicSharedMemorySize, big));
  HIPCHK(hipFuncSetAttribute((const void*)k_fwd<false, 0, false>, hipFuncAttributeMaxDynamicSharedMemorySize, big));
  HIPCHK(hipFuncSetAttribute((const void*)k_fwd<false, 1, true>, hipFuncAttributeMaxDynamicSharedMemorySize, big));
  HIPCHK(hipFuncSetAttribute((const void*)k_dense32, hipFuncAttributeMaxDynamicSharedMemorySize, big));
  HIPCHK(hipFuncSetAttribute((const void*)k_dense_h, hipFuncAttributeMaxDynamicSharedMemorySize, big));
  HIPCHK(hipFuncSetAttribute((const void*)k_dense_b<2>, hipFuncAttributeMaxDynamicSharedMemorySize, big));
  HIPCHK(hipFuncSetAttribute((const void*)k_dense_b<0>, hipFuncAttributeMaxDynamicSharedMemorySize, big));
  HIPCHK(hipFuncSetAttribute((const void*)k_update2<true>, hipFuncAttributeMaxDynamicSharedMemorySize, big));
  HIPCHK(hipFuncSetAttribute((const void*)k_update2<false>, hipFuncAttributeMaxDynamicSharedMemorySize, big));
  D->attrs_set = true;
  return SCILMM_OK;
}

// A dispatch counts WORK-ITEMS in 32 bits: cnt workgroups of `threads` threads must stay below 2^32 of them.
// Every launcher below cuts its grid at max_groups(threads) workgroups (k_outside was the only
// chunked launch; the 1M plan has single launches of several million workgroups).
inline int64_t max_groups(unsigned threads) { return (int64_t)(((uint64_t)1 << 32) / threads) - 1; }

// ---- the factorization's kernels.  The stream is an argument: main, side, batch and k_outside streams all launch them.
struct FactorLaunch {
  Dev* const D;
  scilmm_factor* const fac;
  int64_t launches = 0;  // scilmm_timing.n_launches
  const bool dense_feed = read_dense_feed();  // read per factorization, like SCILMM_SHADOW

  void update(hipStream_t stream, const UpdWork* work, int64_t cnt, double* scratch_half) {
#ifdef SCILMM_DIAG
    if (D->ablate == 4) return;  // timing ablation: no explicit MFMA update items at all (WRONG numbers)
#endif
    const size_t sm_upd = sizeof(double) * (size_t)(2 * KC * LDA + 2 * KC * LDB) + sizeof(int32_t) * TM;
    const auto k = D->use_mfma ? k_update2<true> : k_update2<false>;
    for (int64_t o = 0; o < cnt; o += max_groups(UPD_THREADS)) {
      const unsigned c = (unsigned)std::min<int64_t>(cnt - o, max_groups(UPD_THREADS));
      hipLaunchKernelGGL(k, dim3(c), dim3(UPD_THREADS), sm_upd, stream, D->v, work + o, D->d_combos, fac->L, scratch_half);
      launches++;
    }
  }

  void dense(hipStream_t stream, const DenseWork* dw, int64_t cnt, double* scratch_half) {
    const int32_t dense_first = fac->sym->S->dense_first;
    for (int64_t o = 0; o < cnt; o += max_groups(1024)) {
      const unsigned c = (unsigned)std::min<int64_t>(cnt - o, max_groups(1024));  // (k_dense_h launches 2 c workgroups of 512)
      if (D->front_bits == 32 && fac->L32)
        // (two workgroups per work item: one per 128-row tile)
        hipLaunchKernelGGL(k_dense_h, dim3(2 * c), dim3(512), dense_h_lds, stream, D->v, dense_first, dw + o, fac->L, (const float*)fac->L32,
                           fac->base32, scratch_half, (const float*)D->d_zeros);
      else if (D->front_bits == 32)
        hipLaunchKernelGGL(k_dense32, dim3(c), dim3(512), sizeof(float) * (size_t)(2 * KC * LDA2F + 2 * KC * LDBF), stream, D->v,
                           dense_first, dw + o, fac->L, scratch_half);
      else
        hipLaunchKernelGGL(dense_feed ? k_dense_b<2> : k_dense_b<0>, dim3(c), dim3(512),
                           sizeof(double) * (size_t)(2 * KBA * LDB), stream, D->v, dense_first, dw + o, fac->L, scratch_half,
                           (const double*)D->d_zeros);
      launches++;
    }
  }

  void reduce(hipStream_t stream, const int32_t* tiles, int64_t cnt, const int32_t* pslot, const int32_t* pnseg, const double* slabs) {
    const int64_t per = max_groups(128) / (NB / 4);  // tiles per dispatch
    for (int64_t o = 0; o < cnt; o += per) {
      const int64_t c = std::min(cnt - o, per);
      hipLaunchKernelGGL(k_reduce, dim3((unsigned)((NB / 4) * c)), dim3(128), 0, stream, D->v, tiles + o, pslot, pnseg, slabs, fac->L);
      launches++;
    }
  }

  // cell-wise updates of level l: set 0 = early, 1 = late
  int cells(hipStream_t stream, int which, int32_t l) {
    const Dev::CellSet& CS = D->cellset[which];
    const int64_t u0 = CS.level_ptr[l], u1 = CS.level_ptr[l + 1];
    if (u1 <= u0) return SCILMM_OK;
#ifdef SCILMM_DIAG
    if (D->ablate == 5) return SCILMM_OK;  // timing ablation: no cell-path updates (WRONG numbers)
#endif
    const int64_t nshort = CS.level_short[l], nlong = (u1 - u0) - nshort;
    const int64_t nblk = (nshort + 255) / 256 + (nlong + 3) / 4;
    if (nblk > max_groups(256)) {  // 2^24 workgroups = 4e9 cells of one level: beyond any plan the cell limit admits
      fac->sym->err = "cell plan: one level has more target cells than a dispatch can hold";
      return SCILMM_ERR_ARG;
    }
    hipLaunchKernelGGL(k_sparse_cells, dim3((unsigned)nblk), dim3(256), 0, stream, u0, nshort, u1 - u0, (const int64_t*)CS.dst,
                       (const int64_t*)CS.grp, (const int64_t*)CS.srct, (const int64_t*)CS.srcq, (const int32_t*)CS.md,
                       (const int32_t*)CS.wd, fac->L);
    launches++;
    return SCILMM_OK;
  }

  // panel solve of `cnt` tiles; late partial slabs (`slabs`) are folded on load
  void trsm(hipStream_t stream, const int32_t* tiles, int64_t cnt, const double* slabs) {
    // (k_trsm_lite: four workgroups of 32 rows per tile, register-light and LDS-free: starts beside the resident update kernel)
    const bool lite = D->use_mfma && D->trsm_lite;
    const auto k = lite ? k_trsm_lite : D->use_mfma ? k_trsm<true> : k_trsm<false>;
    const int64_t per = lite ? max_groups(256) / 4 : max_groups(256);  // tiles per dispatch
    for (int64_t o = 0; o < cnt; o += per) {
      const int64_t c = std::min(cnt - o, per);
      hipLaunchKernelGGL(k, dim3((unsigned)(lite ? 4 * c : c)), dim3(256), 0, stream, D->v, tiles + o, fac->L, fac->invD, D->d_tile_pslot,
                         D->d_tile_pnseg, slabs);
      launches++;
    }
  }

  // prelude -> tail contributions, atomic subtraction: one launch per max_groups(256) items
  void outside(hipStream_t stream, const OutsideWork* work, int64_t cnt) {
    auto k = D->use_mfma ? k_outside<true> : k_outside<false>;
#ifdef SCILMM_DIAG
    if (D->ablate == 6) k = k_outside<true, 1>;  // timing ablations: no scatter / plain stores (WRONG numbers)
    if (D->ablate == 7) k = k_outside<true, 2>;
#endif
    for (int64_t o = 0; o < cnt; o += max_groups(256)) {
      const unsigned c = (unsigned)std::min<int64_t>(max_groups(256), cnt - o);
      hipLaunchKernelGGL(k, dim3(c), dim3(256), 0, stream, D->v, fac->sym->S->dense_first, work + o, D->d_tail_front, D->d_keep_front,
                         D->d_grp_next, D->d_grp_t0, fac->L);
      launches++;
      D->n_float_atomic++;
    }
  }
};

// ---- the sweeps' kernels (solve, L*R): one stream, one block of rp right-hand-side columns (gy windows of CW)
struct SweepLaunch {
  Dev* const D;
  const scilmm_factor* const fac;
  const hipStream_t st;
  int rp = 0;
  unsigned gy = 1;

  // out[front] = invL_front * in[front] (trans: invL^T)
  void diag_solve(bool trans, const int32_t* fronts, int64_t cnt, const double* in, double* out) const {
    if (cnt <= 0) return;
    const auto k = D->use_mfma ? (trans ? k_diag_solve<true, true> : k_diag_solve<true, false>)
                               : (trans ? k_diag_solve<false, true> : k_diag_solve<false, false>);
    hipLaunchKernelGGL(k, dim3((unsigned)cnt, gy), dim3(256), 0, st, D->v, fronts, fac->invD, in, out, rp);
  }

  // tiles below the diagonal blocks.  mode 0: out -= L_tile * in (atomic where targets may share rows); mode 1: out += (L*R,
  // always atomic)
  void fwd(int mode, bool atomic, const int32_t* tiles, int64_t cnt, const double* in, double* out) const {
    if (cnt <= 0) return;
    const size_t sm_fwd = sizeof(double) * (size_t)(NB * LDW + KCS * LDA);
    atomic = atomic || mode == 1;
    const auto k = D->use_mfma ? (mode == 1 ? k_fwd<true, 1, true> : atomic ? k_fwd<true, 0, true> : k_fwd<true, 0, false>)
                               : (mode == 1 ? k_fwd<false, 1, true> : atomic ? k_fwd<false, 0, true> : k_fwd<false, 0, false>);
    if (atomic) D->n_float_atomic++;
    hipLaunchKernelGGL(k, dim3((unsigned)cnt, gy), dim3(256), sm_fwd, st, D->v, tiles, fac->L, in, out, rp);
  }

  // backward pushes into X.  ptr / slot / partial: the grouped form of the chain's descendants (null: one pair per workgroup)
  void bwd_push(const int32_t* pairs, int64_t cnt, const int64_t* ptr = nullptr, const int32_t* slot = nullptr,
                double* partial = nullptr) const {
    if (cnt <= 0) return;
    const auto k = D->use_mfma ? k_bwd_push<true> : k_bwd_push<false>;
    hipLaunchKernelGGL(k, dim3((unsigned)cnt, gy), dim3(256), 0, st, D->v, pairs, ptr, fac->L, D->X, rp, slot, partial);
  }

  // deterministic mode: `cnt` pull segments (targets collect their update pairs; lmul: rows of L*R), in -> out
  void fwd_pull(bool lmul, const int32_t* segs, int64_t cnt, const uint8_t* skip, const double* in, double* out) const {
    const auto k = D->use_mfma ? (lmul ? k_fwd_pull<true, 1> : k_fwd_pull<true, 0>) : (lmul ? k_fwd_pull<false, 1> : k_fwd_pull<false, 0>);
    for (int64_t a = 0; a < cnt; a += max_groups(256)) {
      const unsigned c = (unsigned)std::min<int64_t>(max_groups(256), cnt - a);
      hipLaunchKernelGGL(k, dim3(c, gy), dim3(256), 0, st, D->v, D->pull, segs + a, skip, fac->L, in, out, D->d_pull_partial, rp);
    }
  }

  // ... and the partial sums of `cnt` long pair lists (triples in `fold`), added up in slot order
  void pull_fold(bool lmul, const int32_t* fold, int64_t cnt, double* out) const {
    if (cnt <= 0) return;
    const auto k = lmul ? k_pull_fold<1> : k_pull_fold<0>;
    hipLaunchKernelGGL(k, dim3((unsigned)cnt, gy), dim3(256), 0, st, D->v, fold, D->d_pull_partial, out, rp);
  }
};

// ---- the selected inverse's per-level kernels (ydf: fronts from here on keep Y transposed)
inline void sinv_y(Dev* D, const scilmm_factor* fac, hipStream_t st, const int32_t* tiles, int64_t cnt, int32_t ydf) {
  if (cnt <= 0) return;
  const auto k = D->use_mfma ? k_sinv_y<true> : k_sinv_y<false>;
  hipLaunchKernelGGL(k, dim3((unsigned)cnt), dim3(256), 0, st, D->v, tiles, fac->L, fac->invD, D->d_ybuf, D->d_yoff, ydf);
}

inline void sinv_w(Dev* D, const scilmm_factor* fac, hipStream_t st, const int32_t* tiles, int64_t cnt) {
  if (cnt <= 0) return;
  const auto k = D->use_mfma ? k_sinv_w<true> : k_sinv_w<false>;  // (a tile runs its whole reduction and stores: no atomics)
  hipLaunchKernelGGL(k, dim3((unsigned)cnt), dim3(256), 0, st, D->v, tiles, fac->L, D->d_ybuf, D->d_yoff, D->d_col_front,
                     fac->sym->S->dense_first);
}

inline void sinv_cc(Dev* D, const scilmm_factor* fac, hipStream_t st, const int32_t* tiles, int64_t cnt, int32_t ydf) {
  if (cnt <= 0) return;
  const auto k = D->use_mfma ? k_sinv_cc<true> : k_sinv_cc<false>;
  D->n_float_atomic++;
  hipLaunchKernelGGL(k, dim3((unsigned)cnt), dim3(256), 0, st, D->v, tiles, fac->L, D->d_ybuf, D->d_yoff, ydf);
}

// Z_RC of tail front dense_first + jj: the atomic form behind k_sinv_zero, or (deterministic mode) the ordered form, which
// writes every row of R x C exactly once -- straight from the items where the front has one K range, else from
// k_sinv_tail_fold
inline void sinv_tail(Dev* D, const scilmm_factor* fac, hipStream_t st, int32_t jj, bool reverse) {
  const Symbolic& S = *fac->sym->S;
  const int64_t i0 = D->sinv_work_ptr[(size_t)jj], i1 = D->sinv_work_ptr[(size_t)jj + 1];
  if (i1 <= i0) return;
  const int32_t tf = S.dense_first + jj;
  const size_t lds = sizeof(double) * (size_t)(2 * KBA * LDB);
  if (!D->det) {
    const int32_t wtf = S.sn_start[tf + 1] - S.sn_start[tf];
    hipLaunchKernelGGL(k_sinv_zero, dim3(1, (unsigned)wtf), dim3(256), 0, st, D->v, (const int32_t*)(D->d_sinv_tail_fronts + jj), fac->L);
    D->n_float_atomic++;
    hipLaunchKernelGGL(k_sinv_tail<false>, dim3((unsigned)(i1 - i0)), dim3(512), lds, st, D->v, S.dense_first,
                       (const SinvWork*)(D->d_sinv_work + i0), fac->L, (const double*)D->d_ybuf, (const int64_t*)D->d_yoff,
                       (const int32_t*)D->d_col_front, (const double*)D->d_zeros, SinvTailOrd{nullptr, 1, 0});
    return;
  }
  const int32_t nseg = D->sinv_tail_nseg[(size_t)jj];
  hipLaunchKernelGGL(k_sinv_tail<true>, dim3((unsigned)(i1 - i0)), dim3(512), lds, st, D->v, S.dense_first,
                     (const SinvWork*)(D->d_sinv_work + i0), fac->L, (const double*)D->d_ybuf, (const int64_t*)D->d_yoff,
                     (const int32_t*)D->d_col_front, (const double*)D->d_zeros, SinvTailOrd{D->d_sinv_tail_partial, nseg, reverse ? 1 : 0});
  if (nseg > 1)
    hipLaunchKernelGGL(k_sinv_tail_fold, dim3((unsigned)((i1 - i0) / nseg), (unsigned)((S.sn_start[tf + 1] - S.sn_start[tf] + 15) / 16)),
                       dim3(512), 0, st, D->v, tf, nseg, (const double*)D->d_sinv_tail_partial, fac->L);
}

// deterministic mode: the diagonal blocks of level l, segment by segment, and the fronts with several segments folded
inline void sinv_cc_ordered(Dev* D, const scilmm_factor* fac, hipStream_t st, int32_t l, int32_t ydf, bool reverse) {
  const int64_t s0 = D->sinv_cc_seg_ptr[(size_t)l], ns = D->sinv_cc_seg_ptr[(size_t)l + 1] - s0;
  const int64_t f0 = D->sinv_cc_fold_ptr[(size_t)l], nf = D->sinv_cc_fold_ptr[(size_t)l + 1] - f0;
  if (ns <= 0) return;
  const auto k = D->use_mfma ? k_sinv_cc_ordered<true> : k_sinv_cc_ordered<false>;
  hipLaunchKernelGGL(k, dim3((unsigned)ns), dim3(256), 0, st, D->v, (const SinvSeg*)(D->d_sinv_cc_segs + s0), fac->L,
                     (const double*)D->d_ybuf, (const int64_t*)D->d_yoff, ydf, D->d_sinv_cc_partial, reverse ? 1 : 0);
  if (nf > 0)
    hipLaunchKernelGGL(k_sinv_cc_fold, dim3((unsigned)nf, NJB), dim3(256), 0, st, D->v, (const SinvFold*)(D->d_sinv_cc_folds + f0),
                       (const double*)D->d_sinv_cc_partial, fac->L);
}

}  // namespace
