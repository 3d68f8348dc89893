// The sweeps over a resident factor (included by engine.hip only, behind factorize.hip.h).
//
// Sweep is one solve / L*R call: a struct that lives for one call, with one method per sequence of a block of up to RPMAX
// right-hand-side columns -- solve_single (= forward_single, mark_mid, backward_single: the half-solves run one of the two),
// solve_dist, lmul_single, lmul_dist -- built from pull / pull_groups (deterministic mode), chain, handoff (distributed) and
// mark_mid; the kernels go through SweepLaunch.  begin_rhs is what every sweep call does first, run_rhs the device-pointer
// body of the solves and L*R, host_rhs its host form (staged through Dev::IO), finish_rhs_timing what scilmm_sync reads.
// The block calls (marker scan, BLUP) run forward_single between their own producer and reduction: blocks.hip.h.
#pragma once

namespace {

int ensure_work(scilmm_symbolic* sym, Dev* D) {
  const Symbolic& S = *sym->S;
  D->clear_block();  // (whoever asks for the work buffers is about to write them: X no longer holds a scan block, scilmm_scan_panel_dev)
  size_t bytes = (size_t)std::max(S.n, 1) * RPMAX * sizeof(double);
  if (D->world > 1 && !D->work_external) {
    sym->err = "multi-GPU: scilmm_dist_set_work has not been called (the sweeps' buffers must be addressable by the communication layer)";
    return SCILMM_ERR_STATE;
  }
  if (!D->W) HIPCHK(hipMalloc((void**)&D->W, bytes));
  if (!D->X) HIPCHK(hipMalloc((void**)&D->X, bytes));
  return set_attrs(sym, D);
}

inline int rp_of(int rc) { return (rc + 15) & ~15; }

// One solve / L*R call: the sequences of a block of up to RPMAX right-hand-side columns, which sit permuted in W
// (solve) or unpermuted (L*R) and leave through X.
struct Sweep : SweepLaunch {
  scilmm_symbolic* const sym;
  const Symbolic& S;
  int64_t tot = 0;  // doubles of the block: n * rp
  int chain_wide_T = 0, chain_full_T = 0, chain_stagger = 0;
  bool chain_pipe = true;
  bool mid_recorded = false;

  Sweep(scilmm_factor* f, Dev* d) : SweepLaunch{d, f, d->stream}, sym(f->sym), S(*f->sym->S) {}

  void set_block(int rc) {
    rp = rp_of(rc);
    gy = (unsigned)((rp + CW - 1) / CW);
    tot = (int64_t)S.n * rp;
    // the chain sweeps pick their own window width: 64 columns for long chains (every window streams the whole dense
    // tail once), 32 for short ones (twice the workgroups on the latency-bound chain)
    // (read per call: the parity tests force each width on small chains)
    const Tuning tune = read_tuning();
    chain_wide_T = tune.chain_wide_t;
    chain_full_T = tune.chain_full_t;
    chain_pipe = tune.chain_pipe;
    chain_stagger = tune.chain_stagger;
  }

  // the event between the forward and the backward half (of the call's first block)
  int mark_mid() {
    if (!mid_recorded) HIPCHK(hipEventRecord(D->ev[4], st));
    mid_recorded = true;
    return SCILMM_OK;
  }

  int chain(bool bwd) {
    const bool mf = D->use_mfma;
    const bool wide = D->chain_T >= chain_wide_T;
    const bool full = D->chain_T >= chain_full_T && rp > 64;  // every column in one 112-wide window
    const int32_t cwc = full ? 112 : wide ? 64 : 32;
    const int32_t gyc = (int32_t)((rp + cwc - 1) / cwc);
    const unsigned grid = (unsigned)D->chain_T * (unsigned)gyc;
    const int32_t ep = ++D->chain_epoch;
    HIPCHK(hipMemsetAsync(D->d_chain_err + 2, 0, sizeof(int32_t), st));
    const int32_t* cptr = bwd ? (const int32_t*)D->d_cb_ptr : (const int32_t*)D->d_cf_ptr;
    const ChainPair* cpairs = bwd ? (const ChainPair*)D->d_cb : (const ChainPair*)D->d_cf;
    const ChainDesc* cdesc = bwd ? (const ChainDesc*)D->d_cbd : (const ChainDesc*)D->d_cfd;
#define SCILMM_CHAIN_LAUNCH(MF, BW, NC, PP)                                                                                                  \
  hipLaunchKernelGGL((k_chain<MF, BW, NC, PP>), dim3(grid), dim3(512), 0, st, D->v, D->chain_T, (const int32_t*)D->d_chain, cptr, cpairs,   \
                     cdesc, (const int32_t*)D->d_colmap, (const double*)fac->L, (const double*)fac->invD, (const double*)D->W, D->X, rp, gyc, \
                     D->d_chain_flags, ep, D->d_chain_err, D->d_chain_err + 2, (int32_t)chain_stagger)
    // (the pipelined pair loop exists in the 64-column form only: two fragment sets and the x window fit its 256 registers,
    //  not those of the 112-column accumulators; the 32-column chains are bound by the hop)
    const bool pipe = chain_pipe && wide && !full;
    if (mf) {
      if (bwd) {
        if (full) SCILMM_CHAIN_LAUNCH(true, true, 7, false);
        else if (pipe) SCILMM_CHAIN_LAUNCH(true, true, 4, true);
        else if (wide) SCILMM_CHAIN_LAUNCH(true, true, 4, false);
        else SCILMM_CHAIN_LAUNCH(true, true, 2, false);
      } else {
        if (full) SCILMM_CHAIN_LAUNCH(true, false, 7, false);
        else if (pipe) SCILMM_CHAIN_LAUNCH(true, false, 4, true);
        else if (wide) SCILMM_CHAIN_LAUNCH(true, false, 4, false);
        else SCILMM_CHAIN_LAUNCH(true, false, 2, false);
      }
    } else {
      if (bwd) SCILMM_CHAIN_LAUNCH(false, true, 2, false); else SCILMM_CHAIN_LAUNCH(false, false, 2, false);
    }
#undef SCILMM_CHAIN_LAUNCH
    return SCILMM_OK;
  }

  // deterministic mode: the targets of levels [la, lb) pull their update pairs, long pair lists are folded in slot order
  // (one launch: the caller keeps the levels inside one slot group when they are more than one)
  void pull(int32_t la, int32_t lb, bool lmul, const uint8_t* skip) {
    const int64_t g0 = S.pull_level_ptr[(size_t)la], g1 = S.pull_level_ptr[(size_t)lb];
    const int64_t h0 = S.pull_fold_ptr[(size_t)la], h1 = S.pull_fold_ptr[(size_t)lb];
    double* out = lmul ? D->X : D->W;
    fwd_pull(lmul, D->d_pull_level_segs + g0, g1 - g0, skip, lmul ? D->W : D->X, out);
    pull_fold(lmul, D->d_pull_fold + 3 * h0, h1 - h0, out);
  }
  // levels from `lo` on, a launch per slot group: for targets that do not depend on each other
  void pull_groups(int32_t lo, bool lmul, const uint8_t* skip) {
    for (size_t q = 0; q + 1 < S.pull_group_ptr.size(); ++q) {
      const int32_t la = std::max(lo, S.pull_group_ptr[q]), lb = S.pull_group_ptr[q + 1];
      if (la < lb) pull(la, lb, lmul, skip);
    }
  }

  // the levels below the chain are swept level by level, the chain levels by k_chain
  int32_t level_end() const { return D->chain_T > 0 ? D->chain_l0 : S.nlevels; }

  // forward half, X = L^-1 W (W permuted; it is consumed): level sweep, then the chain
  int forward_single() {
    const int32_t lend = level_end();
    for (int32_t l = 0; l < lend; ++l) {
      const int64_t t0 = S.level_tile_ptr[l], t1 = S.level_tile_ptr[l + 1];
      const int32_t f0 = S.level_ptr[l], f1 = S.level_ptr[l + 1];
      if (f1 == f0) continue;
      // deterministic mode: every front of the level first collects the contributions of its (final) descendants
      if (D->det && l > 0) pull(l, l + 1, false, nullptr);
      // x_s = invL_s * W[c0:c1] -> X rows c0..c1 (final), then push to the rows below (atomic where fronts may share them)
      diag_solve(false, D->d_level_fronts + f0, f1 - f0, D->W, D->X);
      if (!D->det) fwd(0, (f1 - f0) > 1, D->d_level_tiles + t0, t1 - t0, D->X, D->W);
    }
    if (D->chain_T > 0) {
      // (deterministic mode: what the fronts below the chain contribute to the chain blocks arrives through the pull form too)
      if (D->det) pull_groups(lend, false, D->d_chain_mask);
      TRY(chain(false));
    }
    return SCILMM_OK;
  }

  // backward half, X = L^-T X in place: the chain, then the levels below it from the top down
  int backward_single() {
    const int32_t lend = level_end();
    if (D->chain_T > 0) {
      TRY(chain(true));
      // descendants below the chain: all their chain targets are final now, one read-modify-write each
      bwd_push(D->d_cg_pairs, D->chain_groups, D->d_cg_ptr, D->d_cg_slot, D->d_push_partial);
      if (D->chain_groups > 0 && D->n_fold > 0)
        hipLaunchKernelGGL(k_push_fold, dim3((unsigned)D->n_fold, gy), dim3(256), 0, st, D->v, (const int32_t*)D->d_fold,
                           (const double*)D->d_push_partial, D->X, rp);
    }
    for (int32_t l = lend - 1; l >= 0; --l) {
      diag_solve(true, D->d_level_fronts + S.level_ptr[l], S.level_ptr[l + 1] - S.level_ptr[l], D->X, D->X);
      bwd_push(D->d_level_pairs + S.level_pair_ptr[l], S.level_pair_ptr[l + 1] - S.level_pair_ptr[l]);
    }
    return SCILMM_OK;
  }

  // X = V^-1 W on one device: forward, then backward
  int solve_single() {
    TRY(forward_single());
    TRY(mark_mid());
    return backward_single();
  }

  // X = L W on one device
  int lmul_single() {
    HIPCHK(hipMemsetAsync(D->X, 0, sizeof(double) * (size_t)tot, st));
    // deterministic mode: every front owns its rows of Z: no dependencies between fronts (the level groups only bound the partial slots)
    if (D->det) pull_groups(0, true, nullptr);
    else fwd(1, true, D->d_level_tiles, (int64_t)S.level_tiles.size(), D->W, D->X);
    return SCILMM_OK;
  }

  // ---- distributed factor.  The prelude is replicated: every rank sweeps it alike.  A tail panel lives on its owner:
  //   forward : the owner pushes x_f through its panel into ACC (its private sum of tail contributions); when block f
  //             is due, the ranks ALL-REDUCE the 128 rows of ACC that belong to it, add them to W (which carries the
  //             right-hand side and the prelude's contributions, identical everywhere) and every rank solves the block
  //             with the replicated inverse diagonal block: x_f is known everywhere without a broadcast;
  //   backward: the owner of panel f has received every push into X[f] (a push (target t, descendant f) needs the
  //             panel of f): it solves the block and BROADCASTS x_f; then every rank pushes x_f into the descendants
  //             it holds (the prelude: all ranks; tail panels: their owners).
  //   L * R   : every panel is multiplied where it lives (the prelude on rank 0), one all-reduce of the product.
  // One collective per tail block and direction, issued on the communication stream between two event hand-offs.
  // (buffer 3 = the caller's work buffer, scilmm_dist_set_work: W | X | ACC, nW doubles each)
  int64_t nW() const { return (int64_t)S.n * RPMAX; }
  int handoff(int32_t op, int64_t off, int64_t cnt, int32_t root) {
    HIPCHK(hipEventRecord(D->ev_x0, st));
    HIPCHK(hipStreamWaitEvent(D->comm, D->ev_x0, 0));
    if (sym->comm_fn(sym->comm_ctx, op, 3, off, cnt, root) != 0) {
      sym->err = "multi-GPU: the communication callback failed";
      return SCILMM_ERR_DEVICE;
    }
    HIPCHK(hipEventRecord(D->ev_x1, D->comm));
    HIPCHK(hipStreamWaitEvent(st, D->ev_x1, 0));
    return SCILMM_OK;
  }

  int solve_dist() {
    HIPCHK(hipMemsetAsync(D->ACC, 0, sizeof(double) * (size_t)tot, st));
    for (int32_t l = 0; l < S.nlevels; ++l) {
      const int32_t tf = D->tail_of_level[l];
      const int64_t t0 = D->lv_tile_ptr[l], tm = D->lv_tile_mid[l], t1 = D->lv_tile_ptr[l + 1];
      const int32_t f0 = S.level_ptr[l], f1 = S.level_ptr[l + 1];  // ALL fronts of the level (replicated diagonal solves)
      if (f1 == f0) continue;
      if (tf >= 0) {
        const int64_t c0 = S.sn_start[tf], wf = S.sn_start[tf + 1] - c0;
        TRY(handoff(1, 2 * nW() + c0 * rp, wf * rp, 0));
        hipLaunchKernelGGL(k_add_rows, dim3((unsigned)((wf * rp + 255) / 256)), dim3(256), 0, st, wf * rp, (const double*)(D->ACC + c0 * rp),
                           D->W + c0 * rp);
      }
      diag_solve(false, D->d_all_fronts + f0, f1 - f0, D->W, D->X);
      // pushes of the prelude fronts of the level go to W (atomic: they may share rows), of an own tail panel to ACC
      fwd(0, true, D->d_level_tiles + t0, tm - t0, D->X, D->W);
      fwd(0, false, D->d_level_tiles + tm, t1 - tm, D->X, D->ACC);
    }
    TRY(mark_mid());
    for (int32_t l = S.nlevels - 1; l >= 0; --l) {
      const int32_t tf = D->tail_of_level[l];
      // (the fronts this rank holds)
      diag_solve(true, D->d_level_fronts + D->lv_ptr[l], D->lv_ptr[l + 1] - D->lv_ptr[l], D->X, D->X);
      if (tf >= 0) {
        const int64_t c0 = S.sn_start[tf], wf = S.sn_start[tf + 1] - c0;
        TRY(handoff(0, nW() + c0 * rp, wf * rp, (tf - D->dist_first) % D->world));
      }
      bwd_push(D->d_level_pairs + D->lv_pair_ptr[l], D->lv_pair_ptr[l + 1] - D->lv_pair_ptr[l]);
    }
    return SCILMM_OK;
  }

  int lmul_dist() {
    HIPCHK(hipMemsetAsync(D->X, 0, sizeof(double) * (size_t)tot, st));
    fwd(1, true, D->d_lmul_tiles, D->n_lmul_tiles, D->W, D->X);
    return handoff(1, nW(), tot, 0);
  }
};

// A chain sweep that timed out: the flag and its pinned mirror are cleared, the call fails.
int report_chain_timeout(scilmm_symbolic* sym, Dev* D, const char* where) {
  HIPCHK(hipMemset(D->d_chain_err, 0, sizeof(int32_t)));
  if (D->h_chain_err) *D->h_chain_err = 0;
  sym->err = std::string("chain sweep: a workgroup timed out waiting for its predecessor") + where;
  return SCILMM_ERR_DEVICE;
}

// What every sweep call does first: settle the factor, make sure the work buffers exist, and report a chain sweep of an
// earlier call that timed out.
int begin_rhs(scilmm_factor* fac, const char* who) {
  scilmm_symbolic* sym = fac->sym;
  Dev* D = (Dev*)sym->device;
  TRY(settle(fac, who));
  TRY(ensure_work(sym, D));
  if (D->h_chain_err && *D->h_chain_err != 0) {
    // an earlier (already completed) chain sweep timed out: report it before queueing more work on top of it
    HIPCHK(hipStreamSynchronize(D->stream));
    return report_chain_timeout(sym, D, " (previous solve)");
  }
  return SCILMM_OK;
}

// The half-solves and the scan stand on the factor alone: refused (handle untouched) where L is not the whole story.
int check_half(scilmm_factor* fac, const char* who) {
  scilmm_symbolic* sym = fac->sym;
  Dev* D = (Dev*)sym->device;
  if (!D) {
    sym->err = std::string(who) + ": the handle has no device state";
    return SCILMM_ERR_STATE;
  }
  if (D->world > 1) {
    sym->err = std::string(who) + ": not available on a distributed factor";
    return SCILMM_ERR_STATE;
  }
  if (D->front_bits == 32) {
    sym->err = std::string(who) + ": not available with fp32 fronts (a half-solve cannot be refined against the exact V)";
    return SCILMM_ERR_STATE;
  }
  return SCILMM_OK;
}

enum RhsMode { RHS_SOLVE = 0, RHS_LMUL = 1, RHS_SOLVE_L = 2, RHS_SOLVE_LT = 3 };

// dB/dX: device, row-major n x r.  RHS_SOLVE: X = V^-1 B.  RHS_LMUL: X = P^T L B.  Both in the ORIGINAL row order.
// RHS_SOLVE_L: X = L^-1 B.  RHS_SOLVE_LT: X = L^-T B.  Both in the factor's PERMUTED row order (single device only).
int run_rhs(scilmm_factor* fac, const double* dB, int32_t r, double* dX, int mode) {
  scilmm_symbolic* sym = fac->sym;
  Dev* D = (Dev*)sym->device;
  const Symbolic& S = *sym->S;
  static const char* const who[] = {"solve", "L*R", "L half-solve", "L^T half-solve"};
  TRY(begin_rhs(fac, who[mode]));
  hipStream_t st = D->stream;
  HIPCHK(hipEventRecord(D->ev[3], st));
  Sweep sw(fac, D);
  const int32_t* perm_in = mode == RHS_SOLVE ? D->v.perm : (const int32_t*)nullptr;
  const int32_t* perm_out = mode == RHS_SOLVE || mode == RHS_LMUL ? D->v.perm : (const int32_t*)nullptr;
  for (int32_t cbeg = 0; cbeg < r; cbeg += RPMAX) {
    sw.set_block(std::min<int>(RPMAX, r - cbeg));
    const unsigned pb = (unsigned)((sw.tot + 255) / 256);
    // Z = P^T (L R): R is NOT permuted on the way in (SparseCholesky.py:50-51); the backward half works in place on X
    hipLaunchKernelGGL(k_perm_in, dim3(pb), dim3(256), 0, st, S.n, r, sw.rp, cbeg, perm_in, dB, mode == RHS_SOLVE_LT ? D->X : D->W);
    if (D->world > 1) TRY(mode == RHS_LMUL ? sw.lmul_dist() : sw.solve_dist());
    else if (mode == RHS_SOLVE_L) TRY(sw.forward_single());
    else if (mode == RHS_SOLVE_LT) { TRY(sw.mark_mid()); TRY(sw.backward_single()); }
    else TRY(mode == RHS_LMUL ? sw.lmul_single() : sw.solve_single());
    hipLaunchKernelGGL(k_perm_out, dim3(pb), dim3(256), 0, st, S.n, r, sw.rp, cbeg, perm_out, D->X, dX);
  }
  TRY(sw.mark_mid());
  if (D->h_chain_err && mode != RHS_LMUL) HIPCHK(hipMemcpyAsync(D->h_chain_err, D->d_chain_err, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipEventRecord(D->ev[5], st));
  HIPCHK(hipGetLastError());
  D->rhs_pending = mode;
  return SCILMM_OK;
}

int finish_rhs_timing(scilmm_symbolic* sym, Dev* D, int mode) {
  D->rhs_pending = -1;
  if (D->chain_T > 0 && mode != RHS_LMUL) {
    int32_t cerr = 0;
    HIPCHK(hipMemcpy(&cerr, D->d_chain_err, sizeof(int32_t), hipMemcpyDeviceToHost));
    if (cerr != 0) return report_chain_timeout(sym, D, "");
  }
  float a = 0, b = 0;
  HIPCHK(hipEventElapsedTime(&a, D->ev[3], D->ev[4]));
  HIPCHK(hipEventElapsedTime(&b, D->ev[4], D->ev[5]));
  if (mode != RHS_LMUL) {  // (a half-solve: the other half's time is that of nothing)
    D->timing.solve_fwd_ms = a;
    D->timing.solve_bwd_ms = b;
  } else {
    D->timing.lmul_ms = a + b;
  }
  return SCILMM_OK;
}

// Host form of run_rhs: B and X are staged through Dev::IO; synchronous.
int host_rhs(scilmm_factor* fac, const double* B, int32_t r, double* X, int mode) {
  scilmm_symbolic* sym = fac->sym;
  Dev* D = (Dev*)sym->device;
  const size_t cnt = (size_t)sym->S->n * (size_t)r;
  TRY(ensure_io(sym, D, 2 * cnt));
  double* dB = D->IO;
  double* dX = D->IO + cnt;
  HIPCHK(hipMemcpyAsync(dB, B, cnt * sizeof(double), hipMemcpyHostToDevice, D->stream));
  TRY(run_rhs(fac, dB, r, dX, mode));
  HIPCHK(hipMemcpyAsync(X, dX, cnt * sizeof(double), hipMemcpyDeviceToHost, D->stream));
  HIPCHK(hipStreamSynchronize(D->stream));
  return finish_rhs_timing(sym, D, mode);
}

}  // namespace
