// Host side of the numeric phase: the A_k values on the device, the level-scheduled launch sequences
// (factorize / solve / L*R / quadratic forms) and the numeric C-ABI entry points of include/scilmm_hip.h.
// The device state they run on (struct Dev, dev.h) is built once per handle by plan.hip.  Everything runs on one
// HIP stream per symbolic handle; host entry points synchronise only where they hand data back to the caller.
//
// A launch sequence is a struct that lives for one call, with one method per step (the kernels go through the typed
// launchers of launch.hip.h):
//   Factorization (run_factorize): prepare_shadow, assemble, prepare_profiling, early(l), late_updates(l), factor_panel(l),
//     broadcast_tail(l), batch(grp), outside_and_deferred_early(l), exchange_status;
//     finish_factorize waits for it, ProfRead turns the profiling events (enum ProfEvent) into scilmm_timing;
//   Sweep (run_rhs): solve_single (= forward_single, mark_mid, backward_single: the half-solves run one of the two),
//     solve_dist, lmul_single, lmul_dist per block of RPMAX columns, built from pull / pull_groups (deterministic mode),
//     chain, handoff (distributed) and mark_mid;
//   Scan block (scilmm_scan_block_dev): the kernels of scan.hip.h around Sweep::forward_single;
//   BLUP blocks (scilmm_rel_block_dev, scilmm_rows_block_dev): the kernels of blup.hip.h in front of the same sweep and statistics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <functional>
#include <thread>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/scilmm_hip.h"
#include <hipcub/hipcub.hpp>

#include "kernels.hip.h"
#include "scan.hip.h"
#include "blup.hip.h"
#include "dev.h"
#include "host_threads.h"

using namespace scilmm;

namespace {

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
  HIPCHK(hipFuncSetAttribute((const void*)k_dense_b, hipFuncAttributeMaxDynamicSharedMemorySize, big));
  HIPCHK(hipFuncSetAttribute((const void*)k_update2<true>, hipFuncAttributeMaxDynamicSharedMemorySize, big));
  HIPCHK(hipFuncSetAttribute((const void*)k_update2<false>, hipFuncAttributeMaxDynamicSharedMemorySize, big));
  D->attrs_set = true;
  return SCILMM_OK;
}

int ensure_work(scilmm_symbolic* sym, Dev* D) {
  const Symbolic& S = *sym->S;
  size_t bytes = (size_t)std::max(S.n, 1) * RPMAX * sizeof(double);
  if (D->world > 1 && !D->work_external) {
    sym->err = "multi-GPU: scilmm_dist_set_work has not been called (the sweeps' buffers must be addressable by the communication layer)";
    return SCILMM_ERR_STATE;
  }
  if (!D->W) HIPCHK(hipMalloc((void**)&D->W, bytes));
  if (!D->X) HIPCHK(hipMalloc((void**)&D->X, bytes));
  return set_attrs(sym, D);
}

int ensure_io(scilmm_symbolic* sym, Dev* D, size_t doubles) {
  if (D->io_cap >= doubles) return SCILMM_OK;
  if (D->IO) (void)hipFree(D->IO);
  D->IO = nullptr;
  D->io_cap = 0;
  HIPCHK(hipMalloc((void**)&D->IO, std::max<size_t>(doubles, 1) * sizeof(double)));
  D->io_cap = doubles;
  return SCILMM_OK;
}

inline int rp_of(int rc) { return (rc + 15) & ~15; }
inline int ldy_of(int rp) { return (rp % 32 == 16) ? rp : rp + 16; }

}  // namespace

struct scilmm_factor {
  scilmm_symbolic* sym = nullptr;
  double* L = nullptr;
  double* invD = nullptr;
  double* logd = nullptr;
  int32_t* status = nullptr;
  bool valid = false;
  int device = -1;            // device of the owning handle (kept here: the factor may outlive its symbolic handle's Dev)
  bool external = false;      // L / invD / logd belong to the caller (scilmm_factor_create_external)
  bool pending = false;       // a factorization has been queued (scilmm_refactorize_async) and not yet waited for
  bool inverted = false;      // L has been replaced by the selected inverse (scilmm_selected_inverse): no solves until refactorized
  float* L32 = nullptr;       // front precision 32: fp32 shadow of the dense-tail panels (k_shadow / k_dense_h), else null
  int64_t base32 = 0;         // index in L of the shadow's first entry (= sn_loff[dense_first])
  int32_t* h_status = nullptr;  // pinned host copy of *status, filled by the queued copy
};

#include "launch.hip.h"

namespace {

#define TRY(call)                      \
  do {                                 \
    int _rc = (call);                  \
    if (_rc != SCILMM_OK) return _rc;  \
  } while (0)

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
    return SCILMM_OK;
  }

  // L = sum_k sigma2[k] A_k on the stored pattern, the status word, and every other stream behind it
  int assemble(const double* sigma2) {
    HIPCHK(hipEventRecord(D->ev[0], st));
    HIPCHK(hipMemsetAsync(fac->L, 0, sizeof(double) * (size_t)std::max<int64_t>(D->nL_local, 1), st));
    int32_t big = 0x7fffffff;
    HIPCHK(hipMemcpyAsync(fac->status, &big, sizeof(int32_t), hipMemcpyHostToDevice, st));
    ValPtrs gen{}, dia{};
    for (int k = 0; k < S.K; ++k) {
      ValPtrs& t = S.is_diag[k] ? dia : gen;
      if (t.count >= 8) {
        sym->err = "more than 8 matrices of one kind";
        return SCILMM_ERR_ARG;
      }
      t.v[t.count] = D->vals[k];
      t.s2[t.count] = sigma2[k];
      t.count++;
    }
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

// One solve / L*R call: the sequences of a block of up to RPMAX right-hand-side columns, which sit permuted in W
// (solve) or unpermuted (L*R) and leave through X.
struct Sweep : SweepLaunch {
  scilmm_symbolic* const sym;
  const Symbolic& S;
  int64_t tot = 0;  // doubles of the block: n * rp
  int chain_wide_T = 0, chain_full_T = 0;
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
#define SCILMM_CHAIN_LAUNCH(MF, BW, NC)                                                                                                  \
  hipLaunchKernelGGL((k_chain<MF, BW, NC>), dim3(grid), dim3(512), 0, st, D->v, D->chain_T, (const int32_t*)D->d_chain, cptr, cpairs, \
                     (const int32_t*)D->d_colmap, (const double*)fac->L, (const double*)fac->invD, (const double*)D->W, D->X, rp, gyc,  \
                     D->d_chain_flags, ep, D->d_chain_err, D->d_chain_err + 2)
    if (mf) {
      if (bwd) { if (full) SCILMM_CHAIN_LAUNCH(true, true, 7); else if (wide) SCILMM_CHAIN_LAUNCH(true, true, 4); else SCILMM_CHAIN_LAUNCH(true, true, 2); }
      else { if (full) SCILMM_CHAIN_LAUNCH(true, false, 7); else if (wide) SCILMM_CHAIN_LAUNCH(true, false, 4); else SCILMM_CHAIN_LAUNCH(true, false, 2); }
    } else {
      if (bwd) SCILMM_CHAIN_LAUNCH(false, true, 2); else SCILMM_CHAIN_LAUNCH(false, false, 2);
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

// What every sweep call does first: complete a queued factorization, refuse a factor that is not valid, make sure the work
// buffers exist, and report a chain sweep of an earlier call that timed out.
int begin_rhs(scilmm_factor* fac) {
  scilmm_symbolic* sym = fac->sym;
  Dev* D = (Dev*)sym->device;
  if (fac->pending) {
    int stp = finish_factorize(fac, nullptr);
    if (stp != SCILMM_OK) return stp;
  }
  if (!fac->valid) {
    sym->err = "factor is not valid";
    return SCILMM_ERR_STATE;
  }
  int stc = ensure_work(sym, D);
  if (stc != SCILMM_OK) return stc;
  if (D->h_chain_err && *D->h_chain_err != 0) {
    // an earlier (already completed) chain sweep timed out: report it before queueing more work on top of it
    HIPCHK(hipStreamSynchronize(D->stream));
    HIPCHK(hipMemset(D->d_chain_err, 0, sizeof(int32_t)));
    *D->h_chain_err = 0;
    sym->err = "chain sweep: a workgroup timed out waiting for its predecessor (previous solve)";
    return SCILMM_ERR_DEVICE;
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
  TRY(begin_rhs(fac));
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
    if (cerr != 0) {
      HIPCHK(hipMemset(D->d_chain_err, 0, sizeof(int32_t)));
      if (D->h_chain_err) *D->h_chain_err = 0;
      sym->err = "chain sweep: a workgroup timed out waiting for its predecessor";
      return SCILMM_ERR_DEVICE;
    }
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

int run_quad(scilmm_symbolic* sym, Dev* D, int32_t k, const double* dU, int32_t r, double* d_out) {
  const Symbolic& S = *sym->S;
  if (k < 0 || k >= S.K || !D->have_vals[k]) {
    sym->err = "quadforms: matrix index invalid or values not uploaded";
    return SCILMM_ERR_STATE;
  }
  int stc = ensure_work(sym, D);
  if (stc != SCILMM_OK) return stc;
  hipStream_t st = D->stream;
  const int64_t SPW = 512;
  const int64_t nw_gen = ((S.nnz_pattern + SPW - 1) / SPW + 3) / 4 * 4;
  const int64_t nw_dia = 1024;
  const int64_t nw = std::max(nw_gen, nw_dia);
  if (D->nwaves_quad < nw) {
    if (D->partial) (void)hipFree(D->partial);
    D->partial = nullptr;
    HIPCHK(hipMalloc((void**)&D->partial, sizeof(double) * (size_t)nw * RPMAX));
    D->nwaves_quad = nw;
  }
  HIPCHK(hipEventRecord(D->ev[6], st));
  for (int32_t cbeg = 0; cbeg < r; cbeg += RPMAX) {
    const int rc = std::min<int>(RPMAX, r - cbeg);
    const int rp = rp_of(rc);
    const int64_t tot = (int64_t)S.n * rp;
    hipLaunchKernelGGL(k_perm_in, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, S.n, r, rp, cbeg, D->v.perm, dU, D->W);
    int64_t nwaves;
    if (S.is_diag[k]) {
      nwaves = nw_dia;
      hipLaunchKernelGGL(k_quad_diag, dim3((unsigned)(nwaves / 4)), dim3(256), 0, st, S.n, (const double*)D->vals[k],
                         (const double*)D->W, rp, D->partial);
    } else {
      nwaves = nw_gen;
      hipLaunchKernelGGL(k_quad, dim3((unsigned)(nwaves / 4)), dim3(256), 0, st, D->v, S.nnz_pattern, SPW,
                         (const double*)D->vals[k], (const double*)D->W, rp, D->partial);
    }
    hipLaunchKernelGGL(k_quad_reduce, dim3(1), dim3(RPMAX), 0, st, nwaves, (const double*)D->partial, rp, D->d_out, 1.0, 0);
    HIPCHK(hipMemcpyAsync(d_out + cbeg, D->d_out, sizeof(double) * rc, hipMemcpyDeviceToDevice, st));
  }
  HIPCHK(hipEventRecord(D->ev[7], st));
  HIPCHK(hipGetLastError());
  return SCILMM_OK;
}

}  // namespace

extern "C" {

int scilmm_values_upload(scilmm_symbolic* sym, int32_t k, const double* data_k) {
  if (!sym || !sym->S || !data_k) return SCILMM_ERR_ARG;
  DevGuard guard(sym);
  const Symbolic& S = *sym->S;
  if (k < 0 || k >= S.K) return SCILMM_ERR_ARG;
  if (sym->maps_released) {
    sym->err = "scilmm_values_upload: the value-assembly maps of this handle were released";
    return SCILMM_ERR_STATE;
  }
  Dev* D;
  int st = ensure_device(sym, &D);
  if (st != SCILMM_OK) return st;
  // general matrix: values permuted into pattern-slot order; diagonal-only matrix: one value per
  // permuted row.  Either way h[val_slot] = data[val_src].
  std::vector<double> h(S.is_diag[k] ? (size_t)S.n : (size_t)S.nnz_pattern, 0.0);
  {
    const auto& slot = S.val_slot[k];
    const auto& src = S.val_src[k];
    // every pattern slot is written by exactly one entry: the permutation is split over a few host threads
    const size_t cnt = slot.size();
    const unsigned nth = (unsigned)std::max<size_t>(1, std::min<size_t>((size_t)std::min(16, scilmm::host_threads()), cnt / (1 << 20) + 1));
    auto part = [&](unsigned q) {
      const size_t a = cnt * q / nth, b = cnt * (q + 1) / nth;
      for (size_t t = a; t < b; ++t) h[slot[t]] = data_k[src[t]];
    };
    std::vector<std::thread> pool;
    for (unsigned q = 1; q < nth; ++q) pool.emplace_back(part, q);
    part(0);
    for (auto& th : pool) th.join();
  }
  if (!D->vals[k]) HIPCHK(hipMalloc((void**)&D->vals[k], std::max<size_t>(h.size(), 1) * sizeof(double)));
  if (!h.empty()) HIPCHK(hipMemcpy(D->vals[k], h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
  D->have_vals[k] = 1;
  return SCILMM_OK;
}

// slack behind L and invD: the chain sweeps read whole 4-deep k-steps of a panel / an inverse block and discard the
// lanes past its last column (at most 3 columns of the tallest panel resp. of an NB-wide block)
static void factor_sizes(const scilmm_symbolic* sym, size_t* nL, size_t* padL, size_t* nI, size_t* padI) {
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

int scilmm_factor_sizes(const scilmm_symbolic* sym, int64_t* L_doubles, int64_t* invD_doubles, int64_t* logd_doubles) {
  if (!sym || !sym->S) return SCILMM_ERR_ARG;
  size_t nL, padL, nI, padI;
  factor_sizes(sym, &nL, &padL, &nI, &padI);
  if (L_doubles) *L_doubles = (int64_t)(nL + padL);
  if (invD_doubles) *invD_doubles = (int64_t)(nI + padI);
  if (logd_doubles) *logd_doubles = (int64_t)sym->S->nsuper + 1;  // + one slot for the status word's trip through the comm layer
  return SCILMM_OK;
}

int scilmm_dist_layout(const scilmm_symbolic* sym, int32_t rank, int32_t world, int32_t* owner, int64_t* loff, int32_t* params) {
  if (!sym || !sym->S || world < 1 || rank < 0 || rank >= world) return SCILMM_ERR_ARG;
  const Symbolic& S = *sym->S;
  DistLayout lay;
  dist_layout(S, rank, world, read_tuning(), &lay);
  if (owner)
    for (int32_t f = 0; f < S.nsuper; ++f) owner[f] = (world > 1 && f >= lay.first) ? (f - lay.first) % world : -1;
  if (loff) {
    std::memcpy(loff, lay.loff.data(), sizeof(int64_t) * (size_t)S.nsuper);
    loff[S.nsuper] = lay.nL;
  }
  if (params) {
    params[0] = lay.first;
    params[1] = lay.Wg;
    params[2] = lay.G;
  }
  return SCILMM_OK;
}

int scilmm_dist_work_size(const scilmm_symbolic* sym, int64_t* doubles) {
  if (!sym || !sym->S || !doubles) return SCILMM_ERR_ARG;
  *doubles = (int64_t)3 * std::max(sym->S->n, 1) * RPMAX;
  return SCILMM_OK;
}

int scilmm_dist_set_work(scilmm_symbolic* sym, double* work) {
  if (!sym || !sym->S || !work) return SCILMM_ERR_ARG;
  DevGuard guard(sym);
  Dev* D;
  int st = ensure_device(sym, &D);
  if (st != SCILMM_OK) return st;
  if ((D->W || D->X) && !D->work_external) {
    sym->err = "scilmm_dist_set_work must precede the first solve on this handle";
    return SCILMM_ERR_STATE;
  }
  const size_t nW = (size_t)std::max(sym->S->n, 1) * RPMAX;
  D->W = work;
  D->X = work + nW;
  D->ACC = work + 2 * nW;
  D->work_external = true;
  return SCILMM_OK;
}

static int factor_create(scilmm_symbolic* sym, double* L_ext, double* invD_ext, double* logd_ext, scilmm_factor** out) {
  Dev* D;
  int st = ensure_device(sym, &D);
  if (st != SCILMM_OK) return st;
  const Symbolic& S = *sym->S;
  scilmm_factor* f = new scilmm_factor();
  f->sym = sym;
  f->device = D->device;
  *out = f;
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
    HIPCHK(hipMalloc((void**)&f->logd, sizeof(double) * ((size_t)S.nsuper + 1)));
  }
  HIPCHK(hipMemset(f->L + nL, 0, sizeof(double) * padL));
  // (all of invD: k_potrf only ever writes the lower triangles, the upper ones must read as zero)
  HIPCHK(hipMemset(f->invD, 0, sizeof(double) * (nI + padI)));
  HIPCHK(hipMalloc((void**)&f->status, sizeof(int32_t)));
  HIPCHK(hipHostMalloc((void**)&f->h_status, sizeof(int32_t), hipHostMallocDefault));
  return SCILMM_OK;
}

int scilmm_factorize(scilmm_symbolic* sym, const double* sigma2, scilmm_factor** out, int32_t* bad_col) {
  if (!sym || !sym->S || !sigma2 || !out) return SCILMM_ERR_ARG;
  DevGuard guard(sym);
  int st = factor_create(sym, nullptr, nullptr, nullptr, out);
  if (st != SCILMM_OK) return st;
  return run_factorize(*out, sigma2, bad_col);
}

int scilmm_factor_create_external(scilmm_symbolic* sym, double* L, double* invD, double* logd, scilmm_factor** out) {
  if (!sym || !sym->S || !L || !invD || !logd || !out) return SCILMM_ERR_ARG;
  DevGuard guard(sym);
  return factor_create(sym, L, invD, logd, out);
}

int scilmm_dist_init(scilmm_symbolic* sym, int32_t rank, int32_t world, void* comm_stream, scilmm_comm_fn fn, void* ctx) {
  if (!sym || !sym->S || world < 1 || rank < 0 || rank >= world) return SCILMM_ERR_ARG;
  if (sym->device) {
    sym->err = "scilmm_dist_init must precede the first numeric call on this handle (the device plan depends on it)";
    return SCILMM_ERR_STATE;
  }
  if (world > 1 && (!fn || !comm_stream)) return SCILMM_ERR_ARG;
  if (world > 1 && sym->deterministic) {
    sym->err = "scilmm_dist_init: deterministic mode is not available on a distributed handle (the summation order of an "
               "all-reduce belongs to the communication library); call scilmm_set_deterministic(sym, 0) first";
    return SCILMM_ERR_STATE;
  }
  sym->rank = rank;
  sym->world = world;
  sym->comm_stream = comm_stream;
  sym->comm_fn = fn;
  sym->comm_ctx = ctx;
  return SCILMM_OK;
}

int scilmm_refactorize(scilmm_factor* fac, const double* sigma2, int32_t* bad_col) {
  if (!fac || !fac->sym || !sigma2) return SCILMM_ERR_ARG;
  DevGuard guard(fac->sym);
  return run_factorize(fac, sigma2, bad_col);
}

int scilmm_refactorize_async(scilmm_factor* fac, const double* sigma2) {
  if (!fac || !fac->sym || !sigma2) return SCILMM_ERR_ARG;
  DevGuard guard(fac->sym);
  return run_factorize(fac, sigma2, nullptr, false);
}

int scilmm_factor_wait(scilmm_factor* fac, int32_t* bad_col) {
  if (!fac || !fac->sym) return SCILMM_ERR_ARG;
  DevGuard guard(fac->sym);
  if (!fac->pending) return fac->valid ? SCILMM_OK : SCILMM_ERR_STATE;
  return finish_factorize(fac, bad_col);
}

void scilmm_factor_free(scilmm_factor* fac) {
  if (!fac) return;
  DevGuard guard(fac->device);
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

int scilmm_logdet(scilmm_factor* fac, double* out) {
  if (!fac || !fac->sym || !out) return SCILMM_ERR_ARG;
  DevGuard guard(fac->sym);
  scilmm_symbolic* sym = fac->sym;
  if (fac->pending) {
    int stp = finish_factorize(fac, nullptr);
    if (stp != SCILMM_OK) return stp;
  }
  if (!fac->valid) return SCILMM_ERR_STATE;
  Dev* D = (Dev*)sym->device;
  const Symbolic& S = *sym->S;
  std::vector<double> h(S.nsuper);
  HIPCHK(hipMemcpyAsync(h.data(), fac->logd, sizeof(double) * S.nsuper, hipMemcpyDeviceToHost, D->stream));
  HIPCHK(hipStreamSynchronize(D->stream));
  // fixed-order pairwise-free summation: deterministic
  long double s = 0.0L;
  for (double v : h) s += v;
  *out = (double)(2.0L * s);
  return SCILMM_OK;
}

static int host_rhs(scilmm_factor* fac, const double* B, int32_t r, double* X, int mode) {
  if (!fac || !fac->sym || !B || !X || r <= 0) return SCILMM_ERR_ARG;
  DevGuard guard(fac->sym);
  scilmm_symbolic* sym = fac->sym;
  Dev* D = (Dev*)sym->device;
  const Symbolic& S = *sym->S;
  const size_t cnt = (size_t)S.n * (size_t)r;
  int st = ensure_io(sym, D, 2 * cnt);
  if (st != SCILMM_OK) return st;
  double* dB = D->IO;
  double* dX = D->IO + cnt;
  HIPCHK(hipMemcpyAsync(dB, B, cnt * sizeof(double), hipMemcpyHostToDevice, D->stream));
  st = run_rhs(fac, dB, r, dX, mode);
  if (st != SCILMM_OK) return st;
  HIPCHK(hipMemcpyAsync(X, dX, cnt * sizeof(double), hipMemcpyDeviceToHost, D->stream));
  HIPCHK(hipStreamSynchronize(D->stream));
  return finish_rhs_timing(sym, D, mode);
}

int scilmm_solve(scilmm_factor* fac, const double* B, int32_t r, double* X) { return host_rhs(fac, B, r, X, 0); }
int scilmm_lmul(scilmm_factor* fac, const double* R, int32_t r, double* Z) { return host_rhs(fac, R, r, Z, 1); }

int scilmm_solve_dev(scilmm_factor* fac, const double* dB, int32_t r, double* dX) {
  if (!fac || !fac->sym || !dB || !dX || r <= 0) return SCILMM_ERR_ARG;
  DevGuard guard(fac->sym);
  return run_rhs(fac, dB, r, dX, 0);
}
int scilmm_lmul_dev(scilmm_factor* fac, const double* dR, int32_t r, double* dZ) {
  if (!fac || !fac->sym || !dR || !dZ || r <= 0) return SCILMM_ERR_ARG;
  DevGuard guard(fac->sym);
  return run_rhs(fac, dR, r, dZ, 1);
}

// The half-solves: argument checks before anything is dereferenced, then the refusals, then the sweep.
static int half_rhs(scilmm_factor* fac, const double* B, int32_t r, double* X, int mode, bool host, const char* who) {
  if (!fac || !B || !X || r <= 0) return SCILMM_ERR_ARG;
  if (!fac->sym) return SCILMM_ERR_ARG;
  DevGuard guard(fac->sym);
  int st = check_half(fac, who);
  if (st != SCILMM_OK) return st;
  return host ? host_rhs(fac, B, r, X, mode) : run_rhs(fac, B, r, X, mode);
}

int scilmm_solve_L(scilmm_factor* fac, const double* B, int32_t r, double* X) {
  return half_rhs(fac, B, r, X, RHS_SOLVE_L, true, "scilmm_solve_L");
}
int scilmm_solve_Lt(scilmm_factor* fac, const double* B, int32_t r, double* X) {
  return half_rhs(fac, B, r, X, RHS_SOLVE_LT, true, "scilmm_solve_Lt");
}
int scilmm_solve_L_dev(scilmm_factor* fac, const double* dB, int32_t r, double* dX) {
  return half_rhs(fac, dB, r, dX, RHS_SOLVE_L, false, "scilmm_solve_L_dev");
}
int scilmm_solve_Lt_dev(scilmm_factor* fac, const double* dB, int32_t r, double* dX) {
  return half_rhs(fac, dB, r, dX, RHS_SOLVE_LT, false, "scilmm_solve_Lt_dev");
}

// What the three block entry points (marker scan, relationship columns, caller rows) share around their own producer of
// the right-hand-side block.  block_begin: the refusals, the one allocation of the slice partial sums (first call on a
// handle, or a wider q; nothing is allocated per block afterwards), the events and the inverse permutation.
static int block_begin(scilmm_factor* fac, int32_t q, const char* who) {
  scilmm_symbolic* sym = fac->sym;
  int st = check_half(fac, who);
  if (st != SCILMM_OK) return st;
  st = begin_rhs(fac);
  if (st != SCILMM_OK) return st;
  Dev* D = (Dev*)sym->device;
  const Symbolic& S = *sym->S;
  const int64_t nslice = ((int64_t)S.n + SCAN_SLICE - 1) / SCAN_SLICE;
  const size_t need = (size_t)nslice * (size_t)(q + 1) * RPMAX;
  if (D->scan_partial_cap < need) {
    HIPCHK(hipStreamSynchronize(D->stream));
    if (D->scan_partial) (void)hipFree(D->scan_partial);
    D->scan_partial = nullptr;
    D->scan_partial_cap = 0;
    HIPCHK(hipMalloc((void**)&D->scan_partial, need * sizeof(double)));
    D->scan_partial_cap = need;
  }
  if (!D->scan_ev[0])
    for (auto& e : D->scan_ev) HIPCHK(hipEventCreate(&e));
  if (!D->d_iperm) {
    st = upload(sym, D, S.iperm, &D->d_iperm);
    if (st != SCILMM_OK) return st;
  }
  return SCILMM_OK;
}

// block_finish: W holds the block (event 1 is recorded here): the forward sweep, then |x_c|^2 and Q^T x_c from one pass over
// X, in fixed row slices folded in slice order, to d_out ((q + 1) x r).
static int block_finish(Sweep& sw, int32_t r, const double* d_Q, int32_t q, double* d_out) {
  Dev* D = sw.D;
  scilmm_symbolic* sym = sw.sym;
  const int32_t n = sw.S.n;
  hipStream_t s0 = D->stream;
  const int64_t nslice = ((int64_t)n + SCAN_SLICE - 1) / SCAN_SLICE;
  HIPCHK(hipEventRecord(D->scan_ev[1], s0));
  int st = sw.forward_single();
  if (st != SCILMM_OK) return st;
  HIPCHK(hipEventRecord(D->scan_ev[2], s0));
  const auto k_stats = q <= 8 ? k_scan_stats<8, 4> : q <= 16 ? k_scan_stats<16, 2> : k_scan_stats<SCAN_QMAX, 1>;
  hipLaunchKernelGGL(k_stats, dim3((unsigned)nslice), dim3(256), 0, s0, n, sw.rp, (const double*)D->X, d_Q, q, D->scan_partial);
  hipLaunchKernelGGL(k_scan_fold, dim3((unsigned)(q + 1)), dim3(SCAN_FOLD * RPMAX), 0, s0, nslice, (const double*)D->scan_partial, q, r, d_out);
  HIPCHK(hipEventRecord(D->scan_ev[3], s0));
  D->scan_pending = true;
  if (D->h_chain_err) HIPCHK(hipMemcpyAsync(D->h_chain_err, D->d_chain_err, sizeof(int32_t), hipMemcpyDeviceToHost, s0));
  HIPCHK(hipGetLastError());
  return SCILMM_OK;
}

int scilmm_scan_block_dev(scilmm_factor* fac, const int8_t* d_geno, int64_t ld_geno, int32_t r, const double* d_Q, int32_t q,
                          double* d_stats) {
  if (!fac || !d_geno || !d_Q || !d_stats || r < 1 || r > RPMAX || q < 1 || q > SCAN_QMAX) return SCILMM_ERR_ARG;
  if (!fac->sym || !fac->sym->S || ld_geno < fac->sym->S->n) return SCILMM_ERR_ARG;
  DevGuard guard(fac->sym);
  scilmm_symbolic* sym = fac->sym;
  int st = block_begin(fac, q, "scilmm_scan_block_dev");
  if (st != SCILMM_OK) return st;
  Dev* D = (Dev*)sym->device;
  const int32_t n = sym->S->n;
  hipStream_t s0 = D->stream;
  Sweep sw(fac, D);
  sw.set_block(r);
  const int32_t rp = sw.rp;
  HIPCHK(hipEventRecord(D->scan_ev[0], s0));
  // rows 0..2 of the statistics: n_obs, mean, centred sum of squares (exact integer sums: no order to fix)
  hipLaunchKernelGGL(k_scan_moments, dim3((unsigned)r), dim3(256), 0, s0, n, d_geno, ld_geno, r, d_stats);
  // W = P (g - mean), missing = 0, columns padded to rp: each tile of individuals is written straight to its permuted rows
  const unsigned tiles = (unsigned)(((int64_t)n + SCAN_TILE - 1) / SCAN_TILE);
  hipLaunchKernelGGL(k_scan_dequant, dim3(tiles), dim3(256), 0, s0, n, r, rp, d_geno, ld_geno, (const int32_t*)D->d_iperm,
                     (const double*)(d_stats + r), D->W);
  // rows 3..: |w(g)|^2 and Q^T w(g)
  return block_finish(sw, r, d_Q, q, d_stats + 3 * (int64_t)r);
}

int scilmm_rel_block_dev(scilmm_factor* fac, const double* weights, const int32_t* ids, int32_t r, const double* d_Q, int32_t q,
                         double* d_stats) {
  if (!fac || !weights || !ids || !d_Q || !d_stats || r < 1 || r > RPMAX || q < 1 || q > SCAN_QMAX) return SCILMM_ERR_ARG;
  if (!fac->sym || !fac->sym->S) return SCILMM_ERR_ARG;
  DevGuard guard(fac->sym);
  scilmm_symbolic* sym = fac->sym;
  const Symbolic& S = *sym->S;
  const int32_t n = S.n;
  // the requests sorted by permuted index: the kernel bisects this list; a repeated individual shows as a repeated index
  std::pair<int32_t, int32_t> order[RPMAX];
  for (int32_t c = 0; c < r; ++c) {
    if (ids[c] < 0 || ids[c] >= n) {
      sym->err = "scilmm_rel_block_dev: an individual outside 0 .. n-1";
      return SCILMM_ERR_ARG;
    }
    order[c] = {S.iperm[(size_t)ids[c]], c};
  }
  std::sort(order, order + r);
  for (int32_t c = 1; c < r; ++c)
    if (order[c].first == order[c - 1].first) {
      sym->err = "scilmm_rel_block_dev: an individual is requested twice in one block";
      return SCILMM_ERR_ARG;
    }
  int st = block_begin(fac, q, "scilmm_rel_block_dev");
  if (st != SCILMM_OK) return st;
  Dev* D = (Dev*)sym->device;
  ValPtrs gen{}, dia{};
  for (int k = 0; k < S.K; ++k) {
    if (weights[k] == 0.0) continue;
    if (!D->have_vals[k]) {
      sym->err = "scilmm_rel_block_dev: the values of a matrix with a nonzero weight are not resident";
      return SCILMM_ERR_STATE;
    }
    ValPtrs& t = S.is_diag[k] ? dia : gen;
    if (t.count >= 8) {
      sym->err = "more than 8 matrices of one kind";
      return SCILMM_ERR_ARG;
    }
    t.v[t.count] = D->vals[k];
    t.s2[t.count] = weights[k];
    t.count++;
  }
  RelReq req{};
  for (int32_t c = 0; c < r; ++c) {
    req.p[c] = order[c].first;
    req.col[c] = order[c].second;
  }
  hipStream_t s0 = D->stream;
  Sweep sw(fac, D);
  sw.set_block(r);
  HIPCHK(hipEventRecord(D->scan_ev[0], s0));
  HIPCHK(hipMemsetAsync(D->W, 0, sizeof(double) * (size_t)sw.tot, s0));
  // W = P G[:, ids]: the stored columns (r workgroups), then one streaming pass over the pattern for the row parts; row 0 of
  // the statistics = G[i, i]
  const unsigned pass = gen.count > 0 ? (unsigned)std::min<int64_t>((S.nnz_pattern + 255) / 256, REL_GRID) : 0u;
  hipLaunchKernelGGL(k_rel_gather, dim3((unsigned)r + pass), dim3(256), 0, s0, D->v, S.nnz_pattern, gen, dia, req, r, sw.rp, D->W,
                     d_stats);
  return block_finish(sw, r, d_Q, q, d_stats + (int64_t)r);
}

int scilmm_rows_block_dev(scilmm_factor* fac, const int64_t* d_indptr, const int32_t* d_indices, const double* d_data, int32_t r,
                          const double* d_Q, int32_t q, double* d_stats) {
  if (!fac || !d_indptr || !d_indices || !d_data || !d_Q || !d_stats || r < 1 || r > RPMAX || q < 1 || q > SCAN_QMAX)
    return SCILMM_ERR_ARG;
  if (!fac->sym || !fac->sym->S) return SCILMM_ERR_ARG;
  DevGuard guard(fac->sym);
  scilmm_symbolic* sym = fac->sym;
  int st = block_begin(fac, q, "scilmm_rows_block_dev");
  if (st != SCILMM_OK) return st;
  Dev* D = (Dev*)sym->device;
  hipStream_t s0 = D->stream;
  Sweep sw(fac, D);
  sw.set_block(r);
  HIPCHK(hipEventRecord(D->scan_ev[0], s0));
  HIPCHK(hipMemsetAsync(D->W, 0, sizeof(double) * (size_t)sw.tot, s0));
  // W[iperm[idx]][c] = data: a wave per row; row 0 of the statistics = 0
  hipLaunchKernelGGL(k_rows_scatter, dim3((unsigned)((r + 3) / 4)), dim3(256), 0, s0, sym->S->n, r, sw.rp, d_indptr, d_indices, d_data,
                     (const int32_t*)D->d_iperm, D->W, d_stats);
  return block_finish(sw, r, d_Q, q, d_stats + (int64_t)r);
}

int scilmm_quadforms_dev(scilmm_symbolic* sym, int32_t k, const double* dU, int32_t r, double* d_out) {
  if (!sym || !sym->S || !dU || !d_out || r <= 0) return SCILMM_ERR_ARG;
  DevGuard guard(sym);
  Dev* D;
  int st = ensure_device(sym, &D);
  if (st != SCILMM_OK) return st;
  st = run_quad(sym, D, k, dU, r, d_out);
  D->quad_pending = st == SCILMM_OK;  // (asynchronous: scilmm_last_timing reads the events once they have happened)
  return st;
}

int scilmm_quadforms(scilmm_symbolic* sym, int32_t k, const double* U, int32_t r, double* out) {
  if (!sym || !sym->S || !U || !out || r <= 0) return SCILMM_ERR_ARG;
  DevGuard guard(sym);
  Dev* D;
  int st = ensure_device(sym, &D);
  if (st != SCILMM_OK) return st;
  const Symbolic& S = *sym->S;
  const size_t cnt = (size_t)S.n * (size_t)r;
  st = ensure_io(sym, D, cnt + (size_t)r);
  if (st != SCILMM_OK) return st;
  HIPCHK(hipMemcpyAsync(D->IO, U, cnt * sizeof(double), hipMemcpyHostToDevice, D->stream));
  st = run_quad(sym, D, k, D->IO, r, D->IO + cnt);
  if (st != SCILMM_OK) return st;
  HIPCHK(hipMemcpyAsync(out, D->IO + cnt, sizeof(double) * r, hipMemcpyDeviceToHost, D->stream));
  HIPCHK(hipStreamSynchronize(D->stream));
  float q = 0;
  HIPCHK(hipEventElapsedTime(&q, D->ev[6], D->ev[7]));
  D->timing.quad_ms = q;
  return SCILMM_OK;
}

int scilmm_he_moments(scilmm_symbolic* sym, int32_t k1, int32_t k2, double* frob, double* diag_dot) {
  if (!sym || !sym->S || !frob || !diag_dot) return SCILMM_ERR_ARG;
  DevGuard guard(sym);
  Dev* D;
  int st = ensure_device(sym, &D);
  if (st != SCILMM_OK) return st;
  const Symbolic& S = *sym->S;
  if (k1 < 0 || k1 >= S.K || k2 < 0 || k2 >= S.K || !D->have_vals[k1] || !D->have_vals[k2]) return SCILMM_ERR_STATE;
  constexpr int NBLK = 1024;
  st = ensure_io(sym, D, 2 * NBLK);
  if (st != SCILMM_OK) return st;
  hipStream_t s0 = D->stream;
  double* part = D->IO;
  HIPCHK(hipMemsetAsync(part, 0, sizeof(double) * 2 * NBLK, s0));
  const bool d1 = S.is_diag[k1], d2 = S.is_diag[k2];
  // sum over the FULL symmetric matrices = 2 * (sum over the stored lower-triangle slots) - (diagonal part); a
  // diagonal-only matrix meets any other matrix on the diagonal only
  if (!d1 && !d2 && S.nnz_pattern > 0)
    hipLaunchKernelGGL(k_dot_slots, dim3(NBLK), dim3(256), 0, s0, S.nnz_pattern, (const double*)D->vals[k1], (const double*)D->vals[k2], part);
  if (S.n > 0)
    hipLaunchKernelGGL(k_dot_diag, dim3(NBLK), dim3(256), 0, s0, S.n, D->v.pat_colptr, (const double*)D->vals[k1], (const double*)D->vals[k2],
                       d1 ? 1 : 0, d2 ? 1 : 0, part + NBLK);
  std::vector<double> h(2 * NBLK);
  HIPCHK(hipMemcpyAsync(h.data(), part, sizeof(double) * 2 * NBLK, hipMemcpyDeviceToHost, s0));
  HIPCHK(hipStreamSynchronize(s0));
  HIPCHK(hipGetLastError());
  long double all = 0.0L, dg = 0.0L;
  for (int b = 0; b < NBLK; ++b) { all += h[b]; dg += h[NBLK + b]; }
  *diag_dot = (double)dg;
  *frob = (d1 || d2) ? (double)dg : (double)(2.0L * all - dg);
  return SCILMM_OK;
}

int scilmm_spmm(scilmm_symbolic* sym, int32_t k, const double* X, int32_t r, double* Y) {
  if (!sym || !sym->S || !X || !Y || r <= 0) return SCILMM_ERR_ARG;
  DevGuard guard(sym);
  Dev* D;
  int st = ensure_device(sym, &D);
  if (st != SCILMM_OK) return st;
  const Symbolic& S = *sym->S;
  if (k < 0 || k >= S.K || !D->have_vals[k]) return SCILMM_ERR_STATE;
  st = ensure_work(sym, D);
  if (st != SCILMM_OK) return st;
  const size_t cnt = (size_t)S.n * (size_t)r;
  st = ensure_io(sym, D, 2 * cnt);
  if (st != SCILMM_OK) return st;
  hipStream_t s = D->stream;
  HIPCHK(hipMemcpyAsync(D->IO, X, cnt * sizeof(double), hipMemcpyHostToDevice, s));
  for (int32_t cbeg = 0; cbeg < r; cbeg += RPMAX) {
    const int rc = std::min<int>(RPMAX, r - cbeg);
    const int rp = rp_of(rc);
    const int64_t tot = (int64_t)S.n * rp;
    const unsigned pb = (unsigned)((tot + 255) / 256);
    hipLaunchKernelGGL(k_perm_in, dim3(pb), dim3(256), 0, s, S.n, r, rp, cbeg, D->v.perm, (const double*)D->IO, D->W);
    HIPCHK(hipMemsetAsync(D->X, 0, sizeof(double) * (size_t)tot, s));
    if (S.is_diag[k])
      hipLaunchKernelGGL(k_spmm_diag, dim3(pb), dim3(256), 0, s, S.n, (const double*)D->vals[k], (const double*)D->W, rp, D->X);
    else
    if (D->det)
      // (deterministic mode: a workgroup per row of the product, fixed summation order, plain stores)
      hipLaunchKernelGGL(k_spmm_row, dim3((unsigned)S.n), dim3(256), 0, s, D->v, D->d_pat_rowptr, D->d_pat_rowcol, D->d_pat_rowslot,
                         (const double*)D->vals[k], (const double*)D->W, rp, D->X);
    else
    {
      // (a wave per 256 pattern slots; lanes = right-hand-side columns)
      const int64_t spw = 256, nwav = (S.nnz_pattern + spw - 1) / spw;
      D->n_float_atomic++;
      hipLaunchKernelGGL(k_spmm_w, dim3((unsigned)((nwav + 3) / 4)), dim3(256), 0, s, D->v, S.nnz_pattern, spw,
                         (const double*)D->vals[k], (const double*)D->W, rp, D->X);
    }
    hipLaunchKernelGGL(k_perm_out, dim3(pb), dim3(256), 0, s, S.n, r, rp, cbeg, D->v.perm, (const double*)D->X, D->IO + cnt);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(Y, D->IO + cnt, cnt * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return SCILMM_OK;
}

int scilmm_spmm_dev(scilmm_symbolic* sym, int32_t k, const double* dX, int32_t r, double* dY) {
  // device-pointer form of scilmm_spmm (same [n][r] layout): asynchronous on the engine's stream, like the other _dev calls
  if (!sym || !sym->S || !dX || !dY || r <= 0) return SCILMM_ERR_ARG;
  DevGuard guard(sym);
  Dev* D;
  int st = ensure_device(sym, &D);
  if (st != SCILMM_OK) return st;
  const Symbolic& S = *sym->S;
  if (k < 0 || k >= S.K || !D->have_vals[k]) return SCILMM_ERR_STATE;
  st = ensure_work(sym, D);
  if (st != SCILMM_OK) return st;
  hipStream_t s = D->stream;
  for (int32_t cbeg = 0; cbeg < r; cbeg += RPMAX) {
    const int rc = std::min<int>(RPMAX, r - cbeg);
    const int rp = rp_of(rc);
    const int64_t tot = (int64_t)S.n * rp;
    const unsigned pb = (unsigned)((tot + 255) / 256);
    hipLaunchKernelGGL(k_perm_in, dim3(pb), dim3(256), 0, s, S.n, r, rp, cbeg, D->v.perm, dX, D->W);
    HIPCHK(hipMemsetAsync(D->X, 0, sizeof(double) * (size_t)tot, s));
    if (S.is_diag[k])
      hipLaunchKernelGGL(k_spmm_diag, dim3(pb), dim3(256), 0, s, S.n, (const double*)D->vals[k], (const double*)D->W, rp, D->X);
    else
    if (D->det)
      // (deterministic mode: a workgroup per row of the product, fixed summation order, plain stores)
      hipLaunchKernelGGL(k_spmm_row, dim3((unsigned)S.n), dim3(256), 0, s, D->v, D->d_pat_rowptr, D->d_pat_rowcol, D->d_pat_rowslot,
                         (const double*)D->vals[k], (const double*)D->W, rp, D->X);
    else
    {
      // (a wave per 256 pattern slots; lanes = right-hand-side columns)
      const int64_t spw = 256, nwav = (S.nnz_pattern + spw - 1) / spw;
      D->n_float_atomic++;
      hipLaunchKernelGGL(k_spmm_w, dim3((unsigned)((nwav + 3) / 4)), dim3(256), 0, s, D->v, S.nnz_pattern, spw,
                         (const double*)D->vals[k], (const double*)D->W, rp, D->X);
    }
    hipLaunchKernelGGL(k_perm_out, dim3(pb), dim3(256), 0, s, S.n, r, rp, cbeg, D->v.perm, (const double*)D->X, dY);
  }
  HIPCHK(hipGetLastError());
  return SCILMM_OK;
}

int scilmm_export_L(scilmm_factor* fac, int64_t* colptr, int32_t* rowidx, double* vals, int64_t* nnz) {
  if (!fac || !fac->sym || !nnz) return SCILMM_ERR_ARG;
  DevGuard guard(fac->sym);
  scilmm_symbolic* sym = fac->sym;
  const Symbolic& S = *sym->S;
  int64_t total = 0;
  for (int32_t s = 0; s < S.nsuper; ++s) {
    int64_t m = S.sn_rowptr[s + 1] - S.sn_rowptr[s];
    int64_t w = S.sn_start[s + 1] - S.sn_start[s];
    total += m * w - w * (w - 1) / 2;
  }
  *nnz = total;
  if (!vals) return SCILMM_OK;
  if (!colptr || !rowidx) return SCILMM_ERR_ARG;
  if (fac->pending) {
    int stp = finish_factorize(fac, nullptr);
    if (stp != SCILMM_OK) return stp;
  }
  if (!fac->valid && !fac->inverted) return SCILMM_ERR_STATE;  // (after scilmm_selected_inverse: the entries of Z on L's pattern)
  Dev* D = (Dev*)sym->device;
  if (D->world > 1) {
    sym->err = "Factor.L(): a distributed factor is not gathered (every rank holds its own tail panels only)";
    return SCILMM_ERR_STATE;
  }
  std::vector<double> h((size_t)std::max<int64_t>(S.nnzL_stored, 1));
  HIPCHK(hipMemcpyAsync(h.data(), fac->L, sizeof(double) * (size_t)S.nnzL_stored, hipMemcpyDeviceToHost, D->stream));
  HIPCHK(hipStreamSynchronize(D->stream));
  int64_t p = 0;
  for (int32_t s = 0; s < S.nsuper; ++s) {
    const int32_t* rs = S.sn_rows.data() + S.sn_rowptr[s];
    int64_t m = S.sn_rowptr[s + 1] - S.sn_rowptr[s];
    int32_t c0 = S.sn_start[s], w = S.sn_start[s + 1] - c0;
    const double* P = h.data() + S.sn_loff[s];
    for (int32_t j = 0; j < w; ++j) {
      colptr[c0 + j] = p;
      for (int64_t t = j; t < m; ++t) {
        rowidx[p] = rs[t];
        vals[p] = P[(int64_t)j * m + t];
        ++p;
      }
    }
  }
  colptr[S.n] = p;
  return SCILMM_OK;
}

int scilmm_ibd_values_device(scilmm_symbolic* sym, int32_t k, int32_t n, const int32_t* parents) {
  if (!sym || !sym->S || !parents) return SCILMM_ERR_ARG;
  DevGuard guard(sym);
  const Symbolic& S = *sym->S;
  if (k < 0 || k >= S.K || n != S.n || S.is_diag[k]) return SCILMM_ERR_ARG;
  if (S.nnz_pattern >= ((int64_t)1 << 32)) {
    sym->err = "scilmm_ibd_values_device: more than 2^32 pattern slots";
    return SCILMM_ERR_ARG;
  }
  // generation (longest path from a founder) of every individual; individuals must be in pedigree order
  std::vector<int32_t> gen((size_t)n, 0);
  int32_t maxgen = 0;
  for (int32_t i = 0; i < n; ++i) {
    int32_t g = 0;
    for (int q = 0; q < 2; ++q) {
      const int32_t p = parents[2 * i + q];
      if (p >= i) {
        sym->err = "scilmm_ibd_values_device: individuals are not in pedigree order (a parent follows its child)";
        return SCILMM_ERR_ARG;
      }
      if (p >= 0) g = std::max(g, gen[p] + 1);
    }
    gen[i] = g;
    maxgen = std::max(maxgen, g);
  }
  if (2 * maxgen > 254) {
    sym->err = "scilmm_ibd_values_device: pedigree deeper than 127 generations";
    return SCILMM_ERR_ARG;
  }
  Dev* D;
  int st = ensure_device(sym, &D);
  if (st != SCILMM_OK) return st;
  hipStream_t s0 = D->stream;
  const int64_t nnz = S.nnz_pattern;
  std::vector<void*> tmp;
  struct Cleanup {
    std::vector<void*>& v;
    ~Cleanup() { for (void* p : v) (void)hipFree(p); }
  } cleanup{tmp};
  auto tmalloc = [&](void** p, size_t bytes) -> int {
    HIPCHK(hipMalloc(p, std::max<size_t>(bytes, 8)));
    tmp.push_back(*p);
    return SCILMM_OK;
  };
  int32_t *d_gen = nullptr, *d_par = nullptr, *d_iperm = nullptr;
  uint8_t *key = nullptr, *skey = nullptr;
  uint32_t *slot = nullptr, *sslot = nullptr;
  int64_t* d_pass = nullptr;
  if ((st = tmalloc((void**)&d_gen, sizeof(int32_t) * (size_t)n)) != SCILMM_OK) return st;
  if ((st = tmalloc((void**)&d_par, sizeof(int32_t) * 2 * (size_t)n)) != SCILMM_OK) return st;
  if ((st = tmalloc((void**)&d_iperm, sizeof(int32_t) * (size_t)n)) != SCILMM_OK) return st;
  if ((st = tmalloc((void**)&key, (size_t)nnz)) != SCILMM_OK) return st;
  if ((st = tmalloc((void**)&skey, (size_t)nnz)) != SCILMM_OK) return st;
  if ((st = tmalloc((void**)&slot, sizeof(uint32_t) * (size_t)nnz)) != SCILMM_OK) return st;
  if ((st = tmalloc((void**)&sslot, sizeof(uint32_t) * (size_t)nnz)) != SCILMM_OK) return st;
  if ((st = tmalloc((void**)&d_pass, sizeof(int64_t) * 256)) != SCILMM_OK) return st;
  if (n > 0) {
    HIPCHK(hipMemcpyAsync(d_gen, gen.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s0));
    HIPCHK(hipMemcpyAsync(d_par, parents, sizeof(int32_t) * 2 * (size_t)n, hipMemcpyHostToDevice, s0));
    HIPCHK(hipMemcpyAsync(d_iperm, S.iperm.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s0));
  }
  if (!D->vals[k]) HIPCHK(hipMalloc((void**)&D->vals[k], std::max<size_t>((size_t)nnz, 1) * sizeof(double)));
  if (nnz > 0) {
    hipLaunchKernelGGL(k_ibd_keys, dim3(4096), dim3(256), 0, s0, n, D->v.pat_colptr, D->v.pat_row, D->v.perm, (const int32_t*)d_gen, key, slot);
    size_t need = 0;
    void* cub = nullptr;
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, need, key, skey, slot, sslot, nnz, 0, 8, s0));
    if ((st = tmalloc(&cub, need)) != SCILMM_OK) return st;
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(cub, need, key, skey, slot, sslot, nnz, 0, 8, s0));
    HIPCHK(hipMemsetAsync(d_pass, 0xff, sizeof(int64_t) * 256, s0));  // -1 = key absent
    hipLaunchKernelGGL(k_ibd_bounds, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, s0, nnz, (const uint8_t*)skey, d_pass);
    std::vector<int64_t> pass(257, -1);
    HIPCHK(hipMemcpyAsync(pass.data(), d_pass, sizeof(int64_t) * 256, hipMemcpyDeviceToHost, s0));
    HIPCHK(hipStreamSynchronize(s0));
    pass[256] = nnz;
    for (int q = 255; q >= 0; --q)
      if (pass[q] < 0) pass[q] = pass[q + 1];
    for (int q = 0; q <= 2 * maxgen; ++q) {
      const int64_t cnt = pass[q + 1] - pass[q];
      if (cnt <= 0) continue;
      hipLaunchKernelGGL(k_ibd_pass, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s0, cnt, (const uint32_t*)(sslot + pass[q]), n,
                         D->v.pat_colptr, D->v.pat_row, D->v.perm, (const int32_t*)d_iperm, (const int32_t*)d_par, D->vals[k]);
    }
  }
  HIPCHK(hipStreamSynchronize(s0));
  HIPCHK(hipGetLastError());
  D->have_vals[k] = 1;
  return SCILMM_OK;
}

int scilmm_dominance_values_device(scilmm_symbolic* sym, int32_t k_dst, int32_t k_src, int32_t n, const int32_t* parents) {
  if (!sym || !sym->S || !parents) return SCILMM_ERR_ARG;
  DevGuard guard(sym);
  const Symbolic& S = *sym->S;
  if (k_dst < 0 || k_dst >= S.K || k_src < 0 || k_src >= S.K || k_dst == k_src || n != S.n || S.is_diag[k_dst] || S.is_diag[k_src])
    return SCILMM_ERR_ARG;
  for (int64_t t = 0; t < 2 * (int64_t)n; ++t)
    if (parents[t] >= n) {
      sym->err = "scilmm_dominance_values_device: parent index out of range";
      return SCILMM_ERR_ARG;
    }
  Dev* D;
  int st = ensure_device(sym, &D);
  if (st != SCILMM_OK) return st;
  if (!D->have_vals[k_src]) {
    sym->err = "scilmm_dominance_values_device: the values of the source matrix are not resident";
    return SCILMM_ERR_STATE;
  }
  hipStream_t s0 = D->stream;
  int32_t *d_par = nullptr, *d_iperm = nullptr;
  struct Cleanup {
    int32_t*& a;
    int32_t*& b;
    ~Cleanup() { if (a) (void)hipFree(a); if (b) (void)hipFree(b); }
  } cleanup{d_par, d_iperm};
  HIPCHK(hipMalloc((void**)&d_par, sizeof(int32_t) * 2 * (size_t)std::max(n, 1)));
  HIPCHK(hipMalloc((void**)&d_iperm, sizeof(int32_t) * (size_t)std::max(n, 1)));
  if (n > 0) {
    HIPCHK(hipMemcpyAsync(d_par, parents, sizeof(int32_t) * 2 * (size_t)n, hipMemcpyHostToDevice, s0));
    HIPCHK(hipMemcpyAsync(d_iperm, S.iperm.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s0));
  }
  if (!D->vals[k_dst]) HIPCHK(hipMalloc((void**)&D->vals[k_dst], std::max<size_t>((size_t)S.nnz_pattern, 1) * sizeof(double)));
  if (S.nnz_pattern > 0)
    hipLaunchKernelGGL(k_dom_slots, dim3(4096), dim3(256), 0, s0, n, D->v.pat_colptr, D->v.pat_row, D->v.perm, (const int32_t*)d_iperm,
                       (const int32_t*)d_par, (const double*)D->vals[k_src], D->vals[k_dst]);
  HIPCHK(hipStreamSynchronize(s0));
  HIPCHK(hipGetLastError());
  D->have_vals[k_dst] = 1;
  return SCILMM_OK;
}

int scilmm_values_download(scilmm_symbolic* sym, int32_t k, double* slots_out) {
  if (!sym || !sym->S || !sym->device || !slots_out) return SCILMM_ERR_ARG;
  DevGuard guard(sym);
  Dev* D = (Dev*)sym->device;
  const Symbolic& S = *sym->S;
  if (k < 0 || k >= S.K || !D->have_vals[k]) return SCILMM_ERR_STATE;
  const size_t cnt = S.is_diag[k] ? (size_t)S.n : (size_t)S.nnz_pattern;
  HIPCHK(hipMemcpy(slots_out, D->vals[k], cnt * sizeof(double), hipMemcpyDeviceToHost));
  return SCILMM_OK;
}

int scilmm_selected_inverse(scilmm_factor* fac) {
  if (!fac || !fac->sym) return SCILMM_ERR_ARG;
  DevGuard guard(fac->sym);
  scilmm_symbolic* sym = fac->sym;
  if (fac->pending) {
    int stp = finish_factorize(fac, nullptr);
    if (stp != SCILMM_OK) return stp;
  }
  if (!fac->valid) {
    sym->err = "scilmm_selected_inverse needs a valid factor";
    return SCILMM_ERR_STATE;
  }
  Dev* D = (Dev*)sym->device;
  const Symbolic& S = *sym->S;
  if (D->world > 1) {
    sym->err = "scilmm_selected_inverse: not available on a distributed factor";
    return SCILMM_ERR_STATE;
  }
  hipStream_t st = D->stream;
  const bool new_sinv_plan = !D->d_col_front;
  {
    int stq = ensure_sinv_plan(sym, D);
    if (stq != SCILMM_OK) return stq;
  }
  if (new_sinv_plan)
    HIPCHK(hipFuncSetAttribute((const void*)k_sinv_tail, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
  HIPCHK(hipEventRecord(D->ev[6], st));
  // SCILMM_SINV_GENERIC=1: the gather kernel for the dense tail as well (the round's first form)
  const bool tail_kernel = D->use_mfma && !read_tuning().sinv_generic;
  for (int32_t l = S.nlevels - 1; l >= 0; --l) {
    const int64_t t0 = D->lv_tile_ptr[l], nt = D->lv_tile_ptr[l + 1] - t0;
    const int32_t f0 = D->lv_ptr[l], f1 = D->lv_ptr[l + 1];
    if (f1 == f0) continue;
    const int32_t* tiles = D->d_level_tiles + t0;
    const int32_t tf = tail_kernel ? D->sinv_tail_front[(size_t)l] : -1;
    const int32_t ydf = tail_kernel ? S.dense_first : S.nsuper;  // fronts from here on keep Y transposed
    sinv_y(D, fac, st, tiles, nt, ydf);
    hipLaunchKernelGGL(k_sinv_cc0, dim3((unsigned)(f1 - f0)), dim3(256), 0, st, D->v, D->d_level_fronts + f0, fac->L,
                       (const double*)fac->invD);
    if (tf >= 0) {
      const int32_t jj = tf - S.dense_first;
      const int64_t i0 = D->sinv_work_ptr[(size_t)jj], i1 = D->sinv_work_ptr[(size_t)jj + 1];
      if (i1 > i0) {
        const int32_t wtf = S.sn_start[tf + 1] - S.sn_start[tf];
        hipLaunchKernelGGL(k_sinv_zero, dim3(1, (unsigned)wtf), dim3(256), 0, st, D->v, (const int32_t*)(D->d_sinv_tail_fronts + jj), fac->L);
        D->n_float_atomic++;
        hipLaunchKernelGGL(k_sinv_tail, dim3((unsigned)(i1 - i0)), dim3(512), sizeof(double) * (size_t)(2 * KBA * LDB), st, D->v,
                           S.dense_first, (const SinvWork*)(D->d_sinv_work + i0), fac->L, (const double*)D->d_ybuf,
                           (const int64_t*)D->d_yoff, (const int32_t*)D->d_col_front, (const double*)D->d_zeros);
      }
      // the gather kernel takes the non-tail fronts' tiles only
      sinv_w(D, fac, st, D->d_sinv_pre_tiles + D->sinv_pre_ptr[(size_t)l], D->sinv_pre_ptr[(size_t)l + 1] - D->sinv_pre_ptr[(size_t)l]);
    } else {
      sinv_w(D, fac, st, tiles, nt);  // ... or all of the level's
    }
    sinv_cc(D, fac, st, tiles, nt, ydf);
  }
  HIPCHK(hipEventRecord(D->ev[7], st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, D->ev[6], D->ev[7]));
  D->timing.quad_ms = ms;  // (reported through the quad_ms slot: the selected inverse replaces the trace estimator's sweeps)
  fac->valid = false;
  fac->inverted = true;
  return SCILMM_OK;
}

int scilmm_inverse_traces(scilmm_factor* fac, double* out) {
  if (!fac || !fac->sym || !out) return SCILMM_ERR_ARG;
  DevGuard guard(fac->sym);
  scilmm_symbolic* sym = fac->sym;
  if (!fac->inverted) {
    sym->err = "scilmm_inverse_traces: call scilmm_selected_inverse first";
    return SCILMM_ERR_STATE;
  }
  Dev* D = (Dev*)sym->device;
  const Symbolic& S = *sym->S;
  constexpr int NBLK = 1024;
  int st = ensure_io(sym, D, 2 * NBLK);
  if (st != SCILMM_OK) return st;
  hipStream_t s0 = D->stream;
  double* part = D->IO;
  std::vector<double> h(2 * NBLK);
  for (int32_t k = 0; k < S.K; ++k) {
    if (!D->have_vals[k]) return SCILMM_ERR_STATE;
    HIPCHK(hipMemsetAsync(part, 0, sizeof(double) * 2 * NBLK, s0));
    const bool dg = S.is_diag[k];
    if (!dg && S.nnz_pattern > 0)
      hipLaunchKernelGGL(k_sinv_trace, dim3(NBLK), dim3(256), 0, s0, S.nnz_pattern, D->v.asm_dst, (const double*)D->vals[k],
                         (const double*)fac->L, part);
    if (S.n > 0)
      hipLaunchKernelGGL(k_sinv_trace_diag, dim3(NBLK), dim3(256), 0, s0, S.n, D->v.pat_colptr, D->v.diag_dst, (const double*)D->vals[k],
                         dg ? 1 : 0, (const double*)fac->L, part + NBLK);
    HIPCHK(hipMemcpyAsync(h.data(), part, sizeof(double) * 2 * NBLK, hipMemcpyDeviceToHost, s0));
    HIPCHK(hipStreamSynchronize(s0));
    long double all = 0.0L, d1 = 0.0L;
    for (int b = 0; b < NBLK; ++b) { all += h[b]; d1 += h[NBLK + b]; }
    out[k] = dg ? (double)d1 : (double)(2.0L * all - d1);  // every off-diagonal pair counts twice (V^-1 and A_k are symmetric)
  }
  HIPCHK(hipGetLastError());
  return SCILMM_OK;
}

int scilmm_sync(scilmm_symbolic* sym) {
  if (!sym || !sym->device) return SCILMM_ERR_ARG;
  DevGuard guard(sym);
  Dev* D = (Dev*)sym->device;
  HIPCHK(hipStreamSynchronize(D->stream));
  if (D->scan_pending) {
    D->scan_pending = false;
    float a = 0, b = 0, c = 0;
    HIPCHK(hipEventElapsedTime(&a, D->scan_ev[0], D->scan_ev[1]));
    HIPCHK(hipEventElapsedTime(&b, D->scan_ev[1], D->scan_ev[2]));
    HIPCHK(hipEventElapsedTime(&c, D->scan_ev[2], D->scan_ev[3]));
    D->scan_ms[0] = a;
    D->scan_ms[1] = b;
    D->scan_ms[2] = c;
    if (D->h_chain_err && *D->h_chain_err != 0) {  // (the queued copy behind the block's sweep has arrived)
      HIPCHK(hipMemset(D->d_chain_err, 0, sizeof(int32_t)));
      *D->h_chain_err = 0;
      sym->err = "chain sweep: a workgroup timed out waiting for its predecessor (scan block)";
      return SCILMM_ERR_DEVICE;
    }
  }
  if (D->rhs_pending >= 0) return finish_rhs_timing(sym, D, D->rhs_pending);
  return SCILMM_OK;
}

int scilmm_last_timing(const scilmm_symbolic* sym, scilmm_timing* out) {
  if (!sym || !sym->device || !out) return SCILMM_ERR_ARG;
  Dev* D = (Dev*)sym->device;
  if (D->quad_pending) {
    // the device-pointer form of the quadratic forms returns without waiting: its timer (the LAST call's) is read here
    DevGuard guard(const_cast<scilmm_symbolic*>(sym));
    float q = 0;
    if (hipEventSynchronize(D->ev[7]) == hipSuccess && hipEventElapsedTime(&q, D->ev[6], D->ev[7]) == hipSuccess) D->timing.quad_ms = q;
    D->quad_pending = false;
  }
  D->timing.n_late_split = D->n_late_split;
  D->timing.n_float_atomic_launches = D->n_float_atomic;
  *out = D->timing;
  return SCILMM_OK;
}

int scilmm_scan_timing(const scilmm_symbolic* sym, double* ms) {
  if (!sym || !sym->device || !ms) return SCILMM_ERR_ARG;
  const Dev* D = (const Dev*)sym->device;
  for (int i = 0; i < 3; ++i) ms[i] = D->scan_ms[i];
  return SCILMM_OK;
}

int scilmm_set_front_precision(scilmm_symbolic* sym, int32_t bits) {
  if (!sym || !sym->S || (bits != 32 && bits != 64)) return SCILMM_ERR_ARG;
  DevGuard guard(sym);
  Dev* D;
  int st = ensure_device(sym, &D);
  if (st != SCILMM_OK) return st;
  if (bits == 32 && !D->dense_on) {
    // (the handle keeps the precision it had: a refused request must not leave a half-set mode behind)
    sym->err = "fp32 fronts need the dense-tail path (tail narrower than 8192 columns: set SCILMM_TUNING=1 SCILMM_DENSE=1)";
    return SCILMM_ERR_STATE;
  }
  D->front_bits = bits;
  return SCILMM_OK;
}

int scilmm_set_profiling(scilmm_symbolic* sym, int32_t on) {
  if (!sym || !sym->S) return SCILMM_ERR_ARG;
  DevGuard guard(sym);
  Dev* D;
  int st = ensure_device(sym, &D);
  if (st != SCILMM_OK) return st;
  D->profiling = on != 0;
  D->serial_early = on == 2;
  return SCILMM_OK;
}

const char* scilmm_version(void) { return "scilmm_hip 0.1 (gfx950)"; }

}  // extern "C"

#ifdef SCILMM_POTRF_PROF
extern "C" int scilmm_debug_potrf_prof(unsigned long long* out16, int reset) {
  if (out16 && hipMemcpyFromSymbol(out16, HIP_SYMBOL(scilmm::g_potrf_prof), sizeof(unsigned long long) * 16) != hipSuccess) return -3;
  if (reset) {
    unsigned long long z[16] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(scilmm::g_potrf_prof), z, sizeof(z)) != hipSuccess) return -3;
  }
  return 0;
}
#endif

#ifdef SCILMM_CHAIN_PROF
extern "C" int scilmm_debug_chain_prof(unsigned long long* out, int n) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(scilmm::g_chain_prof), sizeof(unsigned long long) * 8 * (size_t)n) != hipSuccess) return -3;
  return 0;
}
#endif
