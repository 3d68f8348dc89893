// The factorization (included by engine.hip only, behind launch.hip.h).
//
// Factorization is one factorization being queued: a struct that lives for one call, with one method per step, in the order
// run_factorize calls them (prepare_shadow, assemble, prepare_profiling, early(l), late_updates(l), factor_panel(l),
// broadcast_tail(l), batch(grp), outside_and_deferred_early(l), exchange_status); the kernels go through FactorLaunch.
// finish_factorize waits for the queued work and reads the status word; ProfRead turns the profiling events (enum ProfEvent)
// into scilmm_timing.  settle is what every consumer of a factor calls first.  factor_create allocates a factor's storage.
#pragma once

namespace {

// Profiling events of one level: Dev::pev[PEV_PER_LEVEL * l + slot].  The late brackets are recorded on the main stream, the
// early ones on the level's side stream; consecutive main-stream slots bracket the reduce / cells, k_potrf and k_trsm parts.
enum ProfEvent {
  PEV_LATE_BEGIN,     // before the late update items ...
  PEV_LATE_END,       // ... behind the late dense items
  PEV_CELLS_END,      // behind the late cells (= before k_potrf)
  PEV_POTRF_END,      // (= before k_trsm)
  PEV_LEVEL_END,      // behind k_trsm and the level's shadow
  PEV_EARLY_BEGIN,    // side stream: before the early update items ...
  PEV_EARLY_END,      // ... behind the early dense items (before their reduce and cells)
  PEV_DENSE_E_BEGIN,  // side stream: the early dense items alone
  PEV_DENSE_E_END,
  PEV_DENSE_L_BEGIN,  // the late dense items (of a split level: the older sources' only)
  PEV_DENSE_L_END,
  PEV_DENSE_N_BEGIN,  // split level: the newest source's items, behind the wait for its arrival
  PEV_DENSE_N_END,
  PEV_PER_LEVEL
};

int finish_factorize(scilmm_factor* fac, int32_t* bad_col);

// one more matrix (its resident values, its coefficient) in the list a kernel takes by value: at most 8 of a kind
int push_val(scilmm_symbolic* sym, ValPtrs& t, const double* v, double s2) {
  if (t.count >= 8) {
    sym->err = "more than 8 matrices of one kind";
    return SCILMM_ERR_ARG;
  }
  t.v[t.count] = v;
  t.s2[t.count++] = s2;
  return SCILMM_OK;
}

// One factorization being queued: the steps of run_factorize, in the order it calls them.
struct Factorization : FactorLaunch {
  scilmm_symbolic* const sym;
  const Symbolic& S;
  const hipStream_t st;  // the main stream
  const bool prof;
  const bool dist;       // the dense tail is distributed
  const size_t half;     // doubles of one scratch half (three for the side streams, the fourth for the main stream)
  int32_t last_tail_level = -1;

  Factorization(scilmm_factor* f, Dev* d)
      : FactorLaunch{d, f}, sym(f->sym), S(*f->sym->S), st(d->stream), prof(d->profiling),
        dist(d->world > 1 && d->dist_first < S.nsuper), half((size_t)d->max_slots * TM * NB) {}

  double* late_scratch() const { return D->scratch + (size_t)3 * half; }
  int32_t tail_front(int32_t l) const { return dist ? D->tail_of_level[l] : -1; }  // the distributed front of level l
  bool has_early(int32_t l) const {
    return D->early_ptr[l + 1] > D->early_ptr[l] || D->cellset[0].level_ptr[l + 1] > D->cellset[0].level_ptr[l] ||
           D->dwork_e_ptr[l + 1] > D->dwork_e_ptr[l];
  }
  // (early launches of tail levels are deferred until the k_outside launch has been queued: outside_and_deferred_early)
  bool deferred(int32_t le) const { return D->outside_on && le >= D->tail_level; }
  int mark(int32_t l, ProfEvent e, hipStream_t stream) {
    if (prof) HIPCHK(hipEventRecord(D->pev[(size_t)PEV_PER_LEVEL * l + e], stream));
    return SCILMM_OK;
  }

  int prepare_shadow() {
    // front precision 32: the dense-tail kernel reads an fp32 shadow of the finished tail panels (k_dense_h) -- of the rank's own
    // panels and of its ring slots when the tail is distributed (same rank-local offsets as L, minus the prelude).  It is
    // allocated with the first such factorization and kept (zeroed once: the kernel may read a few entries past a panel, into
    // the next panel's or the slack's, which must be finite); a device without room for it keeps k_dense32 (fp64 operands
    // rounded while they are staged).  SCILMM_TUNING=1 SCILMM_SHADOW=0: k_dense32.
    const bool want = D->front_bits == 32 && D->dense_on && read_tuning().shadow;
    if (want && !fac->L32) {
      fac->base32 = S.sn_loff[S.dense_first];  // (= the prelude's size: the prelude is replicated and stored first on every rank)
      const size_t cnt32 = (size_t)(D->nL_local - fac->base32) + 16384;
      if (hipMalloc((void**)&fac->L32, sizeof(float) * cnt32) != hipSuccess) {
        (void)hipGetLastError();
        fac->L32 = nullptr;
      } else {
        HIPCHK(hipMemsetAsync(fac->L32, 0, sizeof(float) * cnt32, st));
      }
    } else if (!want && fac->L32) {
      HIPCHK(hipStreamSynchronize(st));
      (void)hipFree(fac->L32);
      fac->L32 = nullptr;
    }
    if (verbose() && D->front_bits == 32 && D->dense_on)
      fprintf(stderr, "[scilmm plan] fp32 fronts: %s\n", fac->L32 ? "k_dense_h (fp32 shadow)" : "k_dense32 (fp64 operands rounded while staged)");
    return SCILMM_OK;
  }

  // L = sum_k sigma2[k] A_k on the stored pattern, the status word, and every other stream behind it
  int assemble(const double* sigma2) {
    HIPCHK(hipEventRecord(D->ev[0], st));
    HIPCHK(hipMemsetAsync(fac->L, 0, sizeof(double) * (size_t)std::max<int64_t>(D->nL_local, 1), st));
    int32_t big = 0x7fffffff;
    HIPCHK(hipMemcpyAsync(fac->status, &big, sizeof(int32_t), hipMemcpyHostToDevice, st));
    ValPtrs gen{}, dia{};
    for (int k = 0; k < S.K; ++k) TRY(push_val(sym, S.is_diag[k] ? dia : gen, D->vals[k], sigma2[k]));
    if (S.nnz_pattern > 0) {
      int blocks = (int)std::min<int64_t>((S.nnz_pattern + 255) / 256, 256 * 16);
      hipLaunchKernelGGL(k_assemble, dim3(blocks), dim3(256), 0, st, S.nnz_pattern, D->v.asm_dst, gen, fac->L);
      launches++;
    }
    if (dia.count > 0 && S.n > 0) {
      hipLaunchKernelGGL(k_add_diag, dim3((S.n + 255) / 256), dim3(256), 0, st, S.n, D->v.diag_dst, dia, fac->L);
      launches++;
    }
    HIPCHK(hipEventRecord(D->ev[1], st));
    HIPCHK(hipEventRecord(D->ev_asm, st));
    HIPCHK(hipStreamWaitEvent(D->side, D->ev_asm, 0));
    HIPCHK(hipStreamWaitEvent(D->side2, D->ev_asm, 0));
    if (D->side3) HIPCHK(hipStreamWaitEvent(D->side3, D->ev_asm, 0));
    if (D->outside_st) HIPCHK(hipStreamWaitEvent(D->outside_st, D->ev_asm, 0));
    if (dist) {
      // nothing may land in the ring (or be read-modify-written by a batch) before the storage is cleared and assembled
      HIPCHK(hipStreamWaitEvent(D->bstream, D->ev_asm, 0));
      HIPCHK(hipStreamWaitEvent(D->comm, D->ev_asm, 0));
    }
    return SCILMM_OK;
  }

  int prepare_profiling() {
    D->n_late_split = 0;
    if (prof && D->pev.size() < (size_t)PEV_PER_LEVEL * S.nlevels) {
      size_t old = D->pev.size();
      D->pev.resize((size_t)PEV_PER_LEVEL * S.nlevels, nullptr);
      for (size_t i = old; i < D->pev.size(); ++i) HIPCHK(hipEventCreate(&D->pev[i]));
    }
    if (prof && dist && D->bpev.size() < 2 * D->batch_ev.size()) {
      size_t old = D->bpev.size();
      D->bpev.resize(2 * D->batch_ev.size(), nullptr);
      for (size_t i = old; i < D->bpev.size(); ++i) HIPCHK(hipEventCreate(&D->bpev[i]));
    }
    return SCILMM_OK;
  }

  // Look-ahead: the EARLY part of level l (descendants finished at levels <= l - look_depth - 1) runs on a side stream
  // while the main stream works through an earlier level's latency-bound tail (late update, cells, potrf, trsm).
  int early(int32_t l) {
    const int64_t e0 = D->early_ptr[l], e1 = D->early_ptr[l + 1];
    if (!has_early(l)) return SCILMM_OK;
    const int sidx = D->serial_early ? 0 : l % D->nside;
    hipStream_t sd = sidx == 0 ? D->side : (sidx == 1 ? D->side2 : D->side3);
    double* scratch = D->scratch + (size_t)sidx * half;
    // its youngest descendants sit look_depth + 1 levels below
    if (l >= D->look_depth + 1) HIPCHK(hipStreamWaitEvent(sd, D->lev_ev[2 * (l - D->look_depth - 1)], 0));
    // tail targets: the atomic contributions of the prelude (k_outside) must have landed before anything else
    // reads-modifies-writes a tail panel (the event has been recorded: these launches are deferred until it is)
    if (D->outside_on && l >= D->tail_level && D->out_wait_chunk[(size_t)l] >= 0)
      HIPCHK(hipStreamWaitEvent(sd, D->out_evs[(size_t)D->out_wait_chunk[(size_t)l]], 0));
    TRY(mark(l, PEV_EARLY_BEGIN, sd));
    update(sd, D->d_work_early + e0, e1 - e0, scratch);
    TRY(mark(l, PEV_DENSE_E_BEGIN, sd));
    dense(sd, D->d_dwork_e + D->dwork_e_ptr[l], D->dwork_e_ptr[l + 1] - D->dwork_e_ptr[l], scratch);
    TRY(mark(l, PEV_DENSE_E_END, sd));
    TRY(mark(l, PEV_EARLY_END, sd));
    // fold the early partial slabs on the side stream as well: the main stream keeps only its own (rare) ones
    reduce(sd, D->d_red_tiles_e + D->red_ptr_e[l], D->red_ptr_e[l + 1] - D->red_ptr_e[l], D->d_tile_pslot_e, D->d_tile_pnseg_e, scratch);
    TRY(cells(sd, 0, l));  // early cells: same stream, after the early MFMA update of the same panels
    HIPCHK(hipEventRecord(D->lev_ev[2 * l + 1], sd));
    return SCILMM_OK;
  }

  // the main stream's waits of level l, then its late update and dense items
  int late_updates(int32_t l) {
    double* sh = late_scratch();
    // (progressive k_outside: this level's tail panel needs the chunks that reach it, not the whole launch sequence)
    if (D->outside_on && l >= D->tail_level && D->out_wait_chunk[(size_t)l] >= 0 &&
        (l == D->tail_level || D->out_wait_chunk[(size_t)l] != D->out_wait_chunk[(size_t)l - 1]))
      HIPCHK(hipStreamWaitEvent(st, D->out_evs[(size_t)D->out_wait_chunk[(size_t)l]], 0));
    const int32_t tf = tail_front(l), Wg = D->dist_Wg;
    const int32_t jj = tf >= 0 ? tf - D->dist_first : -1, grp = tf >= 0 ? jj / Wg : -1;
    const bool own_tail = tf >= 0 && D->keep_front[tf];
    // look-ahead split of an own tail panel's late dense items: the older sources' first, the newest source's behind its arrival
    const bool split_late = own_tail && D->dwork_l_mid[(size_t)l] < D->dwork_l_ptr[l + 1];
    if (has_early(l)) HIPCHK(hipStreamWaitEvent(st, D->lev_ev[2 * l + 1], 0));
    if (own_tail) {
      // own tail panel: every batch up to group grp - 2 has been applied to it; its late sources -- the panels of the
      // group before and of its own group so far -- have arrived (own ones: their level event)
      if (grp >= 2) HIPCHK(hipStreamWaitEvent(st, D->batch_ev[grp - 2], 0));
      // (look-ahead split: the wait for the NEWEST source, panel jj - 1, comes after the launch of the older sources' items)
      const int32_t q_end = split_late ? jj - 1 : jj;
      for (int32_t q = std::max(0, (grp - 1) * Wg); q < q_end; ++q) HIPCHK(hipStreamWaitEvent(st, D->lev_ev[2 * S.sn_level[D->dist_first + q]], 0));
    }
    TRY(mark(l, PEV_LATE_BEGIN, st));
    update(st, D->d_work + D->work_ptr[l], D->work_ptr[l + 1] - D->work_ptr[l], sh);
    TRY(mark(l, PEV_DENSE_L_BEGIN, st));
    dense(st, D->d_dwork_l + D->dwork_l_ptr[l], (split_late ? D->dwork_l_mid[(size_t)l] : D->dwork_l_ptr[l + 1]) - D->dwork_l_ptr[l], sh);
    TRY(mark(l, PEV_DENSE_L_END, st));
    if (split_late) {
      // the older sources' items are queued (they run while panel jj - 1 is still on its way); now its arrival, then its items
      HIPCHK(hipStreamWaitEvent(st, D->lev_ev[2 * S.sn_level[D->dist_first + jj - 1]], 0));
      TRY(mark(l, PEV_DENSE_N_BEGIN, st));
      dense(st, D->d_dwork_l + D->dwork_l_mid[(size_t)l], D->dwork_l_ptr[l + 1] - D->dwork_l_mid[(size_t)l], sh);
      TRY(mark(l, PEV_DENSE_N_END, st));
      D->n_late_split++;
    }
    return mark(l, PEV_LATE_END, st);
  }

  // late cells, k_potrf, k_trsm and the fp32 shadow of the level's fronts
  int factor_panel(int32_t l) {
    const int64_t t0 = D->lv_tile_ptr[l], t1 = D->lv_tile_ptr[l + 1];
    const int32_t f0 = D->lv_ptr[l], f1 = D->lv_ptr[l + 1];
    const double* sh = late_scratch();
    // (the late slabs are folded by k_potrf / k_trsm on load: no k_reduce launch on the main stream's chain)
    TRY(cells(st, 1, l));
    TRY(mark(l, PEV_CELLS_END, st));
    if (f1 > f0) {
      const size_t sm_potrf = sizeof(double) * (size_t)((NB / 2) * (NB + 1) + NJB * 16 * 17 + 32);
      hipLaunchKernelGGL(k_potrf, dim3((unsigned)(f1 - f0)), dim3(256), sm_potrf, st, D->v, D->d_level_fronts + f0, fac->L,
                         fac->invD, fac->logd, fac->status, (const int32_t*)D->d_tile_pslot, (const int32_t*)D->d_tile_pnseg, sh);
      launches++;
    }
    TRY(mark(l, PEV_POTRF_END, st));
    trsm(st, D->d_level_tiles + t0, t1 - t0, sh);
    if (fac->L32) {
      // front precision 32: the level's finished tail panel -> its fp32 shadow, before the level's event (the look-ahead
      // launches of later targets read the shadow only)
      for (int32_t q = f0; q < f1; ++q) {
        const int32_t fr = D->lv_fronts[(size_t)q];  // (the level's fronts THIS rank holds: another rank's panel is shadowed when it arrives: broadcast_tail)
        if (fr < S.dense_first || !D->keep_front[fr]) continue;
        shadow(st, fr, S.sn_loff[fr + 1] - S.sn_loff[fr]);
      }
    }
    return mark(l, PEV_LEVEL_END, st);
  }

  void shadow(hipStream_t stream, int32_t fr, int64_t cnt) {
    hipLaunchKernelGGL(k_shadow, dim3((unsigned)std::min<int64_t>((cnt + 255) / 256, 8192)), dim3(256), 0, stream,
                       (const double*)(fac->L + D->loff[fr]), fac->L32 + (D->loff[fr] - fac->base32), cnt);
    launches++;
  }

  // Level with a distributed tail panel: the owner's panel (+ inverse diagonal block + log-sum) goes to every rank -- into
  // the receiver's ring slot.  The level is complete (lev_ev) when the panel has arrived AND this rank's own kernels of
  // the level (its prelude fronts) have finished.
  int broadcast_tail(int32_t l) {
    const int32_t tf = tail_front(l), jj = tf - D->dist_first;
    const int32_t root = jj % D->world;
    HIPCHK(hipEventRecord(D->done_ev[l], st));
    HIPCHK(hipStreamWaitEvent(D->comm, D->done_ev[l], 0));
    if (!D->keep_front[tf]) {
      // ring re-use: the slot's previous occupant (panel jj - G, group gd) must have been consumed -- by its batch and by
      // the late updates of this rank's targets of groups gd and gd + 1
      const int32_t gd = (jj - D->dist_G) / D->dist_Wg;
      if (jj >= D->dist_G) {
        HIPCHK(hipStreamWaitEvent(D->comm, D->batch_ev[gd], 0));
        for (int32_t q = std::min<int32_t>(gd + 1, (int32_t)D->last_own_level.size() - 1); q >= 0; --q)
          if (D->last_own_level[q] >= 0) {
            HIPCHK(hipStreamWaitEvent(D->comm, D->done_ev[D->last_own_level[q]], 0));
            break;
          }
      }
    }
    const int64_t pm = S.sn_rowptr[tf + 1] - S.sn_rowptr[tf], pw = S.sn_start[tf + 1] - S.sn_start[tf];
    int rcm = sym->comm_fn(sym->comm_ctx, 0, 0, D->loff[tf], pm * pw, root);
    if (rcm == 0) rcm = sym->comm_fn(sym->comm_ctx, 0, 1, S.inv_off[tf], pw * pw, root);
    if (rcm == 0) rcm = sym->comm_fn(sym->comm_ctx, 0, 2, tf, 1, root);
    if (rcm != 0) {
      sym->err = "multi-GPU: the communication callback failed";
      return SCILMM_ERR_DEVICE;
    }
    // front precision 32: the arrived panel's fp32 shadow, on the communication stream behind the broadcast
    if (fac->L32 && !D->keep_front[tf]) shadow(D->comm, tf, pm * pw);
    HIPCHK(hipEventRecord(D->lev_ev[2 * l], D->comm));
    last_tail_level = l;
    return SCILMM_OK;
  }

  // source group grp is complete on this rank: its batch (every own target at least two groups ahead), on the batches' stream
  int batch(int32_t grp) {
    hipStream_t bs = D->bstream;
    const int32_t q_end = std::min((grp + 1) * D->dist_Wg, S.nsuper - D->dist_first);
    for (int32_t q = grp * D->dist_Wg; q < q_end; ++q) HIPCHK(hipStreamWaitEvent(bs, D->lev_ev[2 * S.sn_level[D->dist_first + q]], 0));
    if (D->outside_on) HIPCHK(hipStreamWaitEvent(bs, D->out_evs.back(), 0));  // (a batch writes targets up to the last panel)
    if (prof) HIPCHK(hipEventRecord(D->bpev[2 * (size_t)grp], bs));
    dense(bs, D->d_dwork_b + D->dbatch_ptr[grp], D->dbatch_ptr[grp + 1] - D->dbatch_ptr[grp], nullptr);
    if (prof) HIPCHK(hipEventRecord(D->bpev[2 * (size_t)grp + 1], bs));
    HIPCHK(hipEventRecord(D->batch_ev[grp], bs));
    return SCILMM_OK;
  }

  // Every prelude front below the tail's first level is final (l = tail_level - 1): its contribution to the tail, in ITS
  // coordinates, with atomic subtraction (k_outside), a chunk of items and an event at a time; nothing else touches a tail
  // panel meanwhile.  Then the early launches of the tail levels that were held back for it.
  int outside_and_deferred_early(int32_t l) {
    HIPCHK(hipStreamWaitEvent(D->outside_st, D->lev_ev[2 * l], 0));
    for (size_t og = 0; og + 1 < D->ochunk_ptr.size(); ++og) {
      outside(D->outside_st, (const OutsideWork*)D->d_owork + D->ochunk_ptr[og], D->ochunk_ptr[og + 1] - D->ochunk_ptr[og]);
      HIPCHK(hipGetLastError());
      HIPCHK(hipEventRecord(D->out_evs[og], D->outside_st));
    }
    for (int32_t le = std::max(D->tail_level, 1); le <= l + D->look_depth && le < S.nlevels; ++le) TRY(early(le));
    return SCILMM_OK;
  }

  // Distributed tail: the main stream joins the communication and batch streams.  The status word (first non-positive pivot,
  // or "none") is written by the owner of the failing panel only: every rank takes the minimum, so that all of them report
  // SCILMM_ERR_NOT_PD together
  int exchange_status() {
    if (last_tail_level >= 0) HIPCHK(hipStreamWaitEvent(st, D->lev_ev[2 * last_tail_level], 0));
    if (!D->batch_ev.empty()) HIPCHK(hipStreamWaitEvent(st, D->batch_ev.back(), 0));
    hipLaunchKernelGGL(k_status_pack, dim3(1), dim3(1), 0, st, (const int32_t*)fac->status, fac->logd + S.nsuper);
    HIPCHK(hipEventRecord(D->ev_x0, st));
    HIPCHK(hipStreamWaitEvent(D->comm, D->ev_x0, 0));
    if (sym->comm_fn(sym->comm_ctx, 2, 2, S.nsuper, 1, 0) != 0) {
      sym->err = "multi-GPU: the communication callback failed";
      return SCILMM_ERR_DEVICE;
    }
    HIPCHK(hipEventRecord(D->ev_x1, D->comm));
    HIPCHK(hipStreamWaitEvent(st, D->ev_x1, 0));
    hipLaunchKernelGGL(k_status_unpack, dim3(1), dim3(1), 0, st, (const double*)(fac->logd + S.nsuper), fac->status);
    return SCILMM_OK;
  }
};

int run_factorize(scilmm_factor* fac, const double* sigma2, int32_t* bad_col, bool wait = true) {
  scilmm_symbolic* sym = fac->sym;
  if (fac->pending) {
    int stp = finish_factorize(fac, nullptr);
    if (stp != SCILMM_OK && stp != SCILMM_ERR_NOT_PD) return stp;
  }
  Dev* D = (Dev*)sym->device;
  const Symbolic& S = *sym->S;
  for (int k = 0; k < S.K; ++k)
    if (!D->have_vals[k]) {
      sym->err = "scilmm_values_upload has not been called for every matrix";
      return SCILMM_ERR_STATE;
    }
  D->clear_block();  // (a block left in X belongs to the factor that is replaced here)
  fac->valid = false;
  fac->inverted = false;
  if (D->world > 1 && (!sym->comm_fn || !D->comm)) {
    sym->err = "multi-GPU: scilmm_dist_init was called without a communication callback / stream";
    return SCILMM_ERR_STATE;
  }
  if (D->world > 1 && !fac->external) {
    sym->err = "multi-GPU: the factor must live in caller-owned storage (scilmm_factor_create_external)";
    return SCILMM_ERR_STATE;
  }
  TRY(set_attrs(sym, D));
  Factorization F(fac, D);
  TRY(F.prepare_shadow());
  TRY(F.assemble(sigma2));
  TRY(F.prepare_profiling());
  for (int32_t l = 1; l <= D->look_depth && l < S.nlevels; ++l)
    if (!F.deferred(l)) TRY(F.early(l));
  for (int32_t l = 0; l < S.nlevels; ++l) {
    // early(l + depth) may start as soon as level l-1 is finished: issue it before this level's own kernels
    const int32_t le = l + D->look_depth;
    if (l >= 1 && le < S.nlevels && !(l < D->tail_level && F.deferred(le))) TRY(F.early(le));
    TRY(F.late_updates(l));
    TRY(F.factor_panel(l));
    const int32_t tf = F.tail_front(l);
    if (tf < 0) {
      HIPCHK(hipEventRecord(D->lev_ev[2 * l], F.st));
    } else {
      TRY(F.broadcast_tail(l));
      const int32_t jj = tf - D->dist_first;
      if ((jj + 1) % D->dist_Wg == 0 || jj == S.nsuper - D->dist_first - 1) TRY(F.batch(jj / D->dist_Wg));
    }
    if (D->outside_on && l == D->tail_level - 1) TRY(F.outside_and_deferred_early(l));
  }
  if (F.dist) TRY(F.exchange_status());
  HIPCHK(hipEventRecord(D->ev[2], F.st));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(fac->h_status, fac->status, sizeof(int32_t), hipMemcpyDeviceToHost, F.st));
  D->timing.n_launches = F.launches;
  fac->pending = true;
  if (!wait) return SCILMM_OK;
  return finish_factorize(fac, bad_col);
}

// Reads the profiling events of a finished factorization into scilmm_timing.  hipEventElapsedTime errors are kept (the
// first one) and reported by finish_factorize.
struct ProfRead {
  Dev* const D;
  const Symbolic& S;
  hipError_t err = hipSuccess;

  float elapsed_ms(hipEvent_t a, hipEvent_t b) {
    float x = 0;
    const hipError_t e = hipEventElapsedTime(&x, a, b);
    if (e != hipSuccess && err == hipSuccess) err = e;
    return x;
  }
  hipEvent_t pev(int32_t l, ProfEvent e) const { return D->pev[(size_t)PEV_PER_LEVEL * l + e]; }
  float span(int32_t l, ProfEvent a, ProfEvent b) { return elapsed_ms(pev(l, a), pev(l, b)); }
  float since_assembly(int32_t l, ProfEvent e) { return elapsed_ms(D->ev[1], pev(l, e)); }
  // which of a level's launches exist (an empty bracket is not read)
  bool upd_l(int32_t l) const { return D->work_ptr[l + 1] > D->work_ptr[l]; }
  bool upd_e(int32_t l) const { return D->early_ptr[l + 1] > D->early_ptr[l]; }
  bool dense_l(int32_t l) const { return D->dwork_l_ptr[l + 1] > D->dwork_l_ptr[l]; }
  bool dense_e(int32_t l) const { return D->dwork_e_ptr[l + 1] > D->dwork_e_ptr[l]; }

  // sums of the launch durations per kernel class
  void level_sums() {
    double tu = 0, tp = 0, tt = 0, tmid = 0, td = 0;
    int64_t nu = 0, nd = 0;
    for (int32_t l = 0; l < S.nlevels; ++l) {
      if (upd_l(l) || dense_l(l)) {
        tu += span(l, PEV_LATE_BEGIN, PEV_LATE_END);
        nu += upd_l(l) + dense_l(l);
      }
      if (upd_e(l) || dense_e(l)) {
        tu += span(l, PEV_EARLY_BEGIN, PEV_EARLY_END);
        nu += upd_e(l) + dense_e(l);
      }
      if (dense_e(l)) {
        td += span(l, PEV_DENSE_E_BEGIN, PEV_DENSE_E_END);
        nd++;
      }
      if (dense_l(l)) {
        const bool split = D->world > 1 && D->dwork_l_mid[(size_t)l] < D->dwork_l_ptr[l + 1] && D->tail_of_level[l] >= 0 &&
                           D->keep_front[D->tail_of_level[l]];
        if (!split || D->dwork_l_mid[(size_t)l] > D->dwork_l_ptr[l]) {
          td += span(l, PEV_DENSE_L_BEGIN, PEV_DENSE_L_END);
          nd++;
        }
        if (split) {  // (the newest source's items: their own bracket, so that the wait for its broadcast is not counted as kernel time)
          td += span(l, PEV_DENSE_N_BEGIN, PEV_DENSE_N_END);
          nd++;
        }
      }
      tmid += span(l, PEV_LATE_END, PEV_CELLS_END);
      tp += span(l, PEV_CELLS_END, PEV_POTRF_END);
      tt += span(l, PEV_POTRF_END, PEV_LEVEL_END);
    }
    if (D->world > 1 && D->dist_first < S.nsuper && D->bpev.size() >= 2 * D->batch_ev.size()) {
      // distributed tail: the batches (one launch sequence per complete source group, on their own stream) carry the bulk of
      // this rank's dense-tail flops; the per-level "late" launches above the rest
      for (size_t g = 0; g < D->batch_ev.size(); ++g) {
        if (D->dbatch_ptr[g + 1] <= D->dbatch_ptr[g]) continue;
        const float x = elapsed_ms(D->bpev[2 * g], D->bpev[2 * g + 1]);
        td += x;
        tu += x;
        nd++;
        nu++;
      }
    }
    D->timing.update_ms = tu;       // sum of k_update launch durations (early + late; they overlap other kernels)
    D->timing.potrf_ms = tp;
    D->timing.trsm_ms = tt;
    D->timing.reduce_cells_ms = tmid;
    D->timing.n_update_launches = nu;
    D->timing.dense_ms = td;          // k_dense launches alone (early + late; they overlap each other on the two side streams)
    D->timing.n_dense_launches = nd;
  }

  // union of the update launches' [start, end] intervals, measured from the end of the assembly
  void update_union() {
    std::vector<std::pair<float, float>> iv;
    for (int32_t l = 0; l < S.nlevels; ++l) {
      if (upd_l(l) || dense_l(l)) {
        const float a0 = since_assembly(l, PEV_LATE_BEGIN);
        iv.push_back({a0, since_assembly(l, PEV_LATE_END)});
      }
      if (upd_e(l) || dense_e(l)) {
        const float a0 = since_assembly(l, PEV_EARLY_BEGIN);
        iv.push_back({a0, since_assembly(l, PEV_EARLY_END)});
      }
    }
    std::sort(iv.begin(), iv.end());
    double uni = 0.0;
    float cur0 = 0, cur1 = -1;
    for (auto& q : iv) {
      if (cur1 < cur0 || q.first > cur1) {
        if (cur1 >= cur0) uni += cur1 - cur0;
        cur0 = q.first;
        cur1 = q.second;
      } else {
        cur1 = std::max(cur1, q.second);
      }
    }
    if (cur1 >= cur0) uni += cur1 - cur0;
    D->timing.update_union_ms = uni;
  }

  // SCILMM_LEVEL_DUMP diagnostic: one line per level (durations in ms; cost = combos + K-chunks of the level's dense work)
  void level_dump(const char* path) {
    FILE* fp = fopen(path, "w");
    if (!fp) return;
    fprintf(fp, "level,fronts,tiles,items_early,items_late,cost_early,cost_late,early_ms,late_ms,mid_ms,potrf_ms,trsm_ms,t_potrf_ms,t_early0_ms,t_early1_ms,dense_early_ms,dense_late_ms\n");
    for (int32_t l = 0; l < S.nlevels; ++l) {
      const float xl = upd_l(l) ? span(l, PEV_LATE_BEGIN, PEV_LATE_END) : 0;
      const float xe = upd_e(l) ? span(l, PEV_EARLY_BEGIN, PEV_EARLY_END) : 0;
      const float xm = span(l, PEV_LATE_END, PEV_CELLS_END);
      const float xp = span(l, PEV_CELLS_END, PEV_POTRF_END);
      const float xt = span(l, PEV_POTRF_END, PEV_LEVEL_END);
      // absolute times since the end of the assembly: this level's potrf, its early dense launch (begin, end)
      const float tp = since_assembly(l, PEV_CELLS_END);
      const float te0 = dense_e(l) ? since_assembly(l, PEV_DENSE_E_BEGIN) : 0;
      const float te1 = dense_e(l) ? since_assembly(l, PEV_DENSE_E_END) : 0;
      const float dl = dense_l(l) ? span(l, PEV_DENSE_L_BEGIN, PEV_DENSE_L_END) : 0;
      fprintf(fp, "%d,%d,%lld,%lld,%lld,%lld,%lld,%.4f,%.4f,%.4f,%.4f,%.4f,%.3f,%.3f,%.3f,%.4f,%.4f\n", l, S.level_ptr[l + 1] - S.level_ptr[l],
              (long long)(S.level_tile_ptr[l + 1] - S.level_tile_ptr[l]), (long long)(D->early_ptr[l + 1] - D->early_ptr[l]),
              (long long)(D->work_ptr[l + 1] - D->work_ptr[l]), (long long)D->lev_cost_e[l], (long long)D->lev_cost_l[l], xe, xl,
              xm, xp, xt, tp, te0, te1, te1 - te0, dl);
    }
    fclose(fp);
  }
};

// second half of a factorization: wait for the queued work, read the event timings and the status word
int finish_factorize(scilmm_factor* fac, int32_t* bad_col) {
  scilmm_symbolic* sym = fac->sym;
  Dev* D = (Dev*)sym->device;
  fac->pending = false;
  HIPCHK(hipStreamSynchronize(D->stream));
  HIPCHK(hipStreamSynchronize(D->side));
  HIPCHK(hipStreamSynchronize(D->side2));
  if (D->side3) HIPCHK(hipStreamSynchronize(D->side3));
  if (D->bstream) HIPCHK(hipStreamSynchronize(D->bstream));
  if (D->world > 1 && D->comm) HIPCHK(hipStreamSynchronize(D->comm));
  if (D->outside_st) HIPCHK(hipStreamSynchronize(D->outside_st));
  ProfRead T{D, *sym->S};
  D->timing.assemble_ms = T.elapsed_ms(D->ev[0], D->ev[1]);
  D->timing.factor_ms = T.elapsed_ms(D->ev[1], D->ev[2]);
  const int32_t status = *fac->h_status;
  if (D->profiling && T.err == hipSuccess) {
    T.level_sums();
    T.update_union();
    if (const char* dump = getenv("SCILMM_LEVEL_DUMP")) T.level_dump(dump);
  }
  if (T.err != hipSuccess) {
    sym->err = std::string("hipEventElapsedTime: ") + hipGetErrorString(T.err);
    return SCILMM_ERR_DEVICE;
  }
  if (status != 0x7fffffff) {
    if (bad_col) *bad_col = status;
    return SCILMM_ERR_NOT_PD;
  }
  fac->valid = true;
  return SCILMM_OK;
}

// What every consumer of a factor does first: complete a queued factorization, refuse a factor that is not valid
// (inverted_ok: ... unless it holds the selected inverse).
int settle(scilmm_factor* fac, const char* who, bool inverted_ok = false) {
  if (fac->pending) TRY(finish_factorize(fac, nullptr));
  if (!fac->valid && !(inverted_ok && fac->inverted)) {
    fac->sym->err = std::string(who) + ": the factor is not valid";
    return SCILMM_ERR_STATE;
  }
  return SCILMM_OK;
}

// slack behind L and invD: the chain sweeps read whole 4-deep k-steps of a panel / an inverse block and discard the
// lanes past its last column (at most 3 columns of the tallest panel resp. of an NB-wide block)
void factor_sizes(const scilmm_symbolic* sym, size_t* nL, size_t* padL, size_t* nI, size_t* padI) {
  const Symbolic& S = *sym->S;
  int64_t max_m = 0;
  for (int32_t q = 0; q < S.nsuper; ++q) max_m = std::max<int64_t>(max_m, S.sn_rowptr[q + 1] - S.sn_rowptr[q]);
  *padL = (size_t)(4 * max_m + 4 * NB);
  *padI = (size_t)(5 * NB);
  *nL = (size_t)std::max<int64_t>(S.nnzL_stored, 1);
  if (sym->world > 1) {  // rank-local storage: prelude + own tail panels + ring (DistLayout)
    DistLayout lay;
    dist_layout(S, sym->rank, sym->world, read_tuning(), &lay);
    *nL = (size_t)std::max<int64_t>(lay.nL, 1);
  }
  *nI = (size_t)std::max<int64_t>(S.inv_off[S.nsuper], 1);
}

void factor_free(scilmm_factor* fac) {
  if (fac->pending) (void)finish_factorize(fac, nullptr);
  if (fac->h_status) (void)hipHostFree(fac->h_status);
  if (!fac->external) {
    if (fac->L) (void)hipFree(fac->L);
    if (fac->invD) (void)hipFree(fac->invD);
    if (fac->logd) (void)hipFree(fac->logd);
  }
  if (fac->status) (void)hipFree(fac->status);
  if (fac->L32) (void)hipFree(fac->L32);
  delete fac;
}

// the storage of f: its own, or the caller's (L_ext / invD_ext / logd_ext)
int factor_alloc(scilmm_factor* f, double* L_ext, double* invD_ext, double* logd_ext) {
  scilmm_symbolic* sym = f->sym;
  size_t nL, padL, nI, padI;
  factor_sizes(sym, &nL, &padL, &nI, &padI);
  if (L_ext) {
    f->external = true;
    f->L = L_ext;
    f->invD = invD_ext;
    f->logd = logd_ext;
  } else {
    HIPCHK(hipMalloc((void**)&f->L, sizeof(double) * (nL + padL)));
    HIPCHK(hipMalloc((void**)&f->invD, sizeof(double) * (nI + padI)));
    HIPCHK(hipMalloc((void**)&f->logd, sizeof(double) * ((size_t)sym->S->nsuper + 1)));
  }
  HIPCHK(hipMemset(f->L + nL, 0, sizeof(double) * padL));
  // (all of invD: k_potrf only ever writes the lower triangles, the upper ones must read as zero)
  HIPCHK(hipMemset(f->invD, 0, sizeof(double) * (nI + padI)));
  HIPCHK(hipMalloc((void**)&f->status, sizeof(int32_t)));
  HIPCHK(hipHostMalloc((void**)&f->h_status, sizeof(int32_t), hipHostMallocDefault));
  return SCILMM_OK;
}

// A new factor of the handle, nothing factorized yet.  On failure whatever was allocated is freed and *out stays null.
int factor_create(scilmm_symbolic* sym, double* L_ext, double* invD_ext, double* logd_ext, scilmm_factor** out) {
  *out = nullptr;
  Dev* D;
  TRY(ensure_device(sym, &D));
  scilmm_factor* f = new (std::nothrow) scilmm_factor();
  if (!f) {
    sym->err = "scilmm_factor: out of host memory";
    return SCILMM_ERR_DEVICE;
  }
  f->sym = sym;
  f->device = D->device;
  const int st = factor_alloc(f, L_ext, invD_ext, logd_ext);
  if (st != SCILMM_OK) {
    factor_free(f);
    return st;
  }
  *out = f;
  return SCILMM_OK;
}

}  // namespace
