// Construction of a symbolic handle's device state: streams and events, multi-GPU ownership, the symbolic arrays on the
// device and the plans the kernels of kernels.hip.h consume (update work items, cell lists, dense-tail items, k_outside
// chunks, the chain sweep, the selected inverse).  Runs once per handle (ensure_device), as a sequence of stages; the
// only kernels launched from here are the cell-plan builders of cellplan.hip.h.
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

#include "dev.h"
#include "cellplan.hip.h"
#include "host_threads.h"

namespace scilmm {

void dev_free(void* p) {
  Dev* D = (Dev*)p;
  if (!D) return;
  for (void* a : D->allocs) (void)hipFree(a);
  for (double* v : D->vals)
    if (v) (void)hipFree(v);
  if (D->W && !D->work_external) (void)hipFree(D->W);
  if (D->X && !D->work_external) (void)hipFree(D->X);
  if (D->IO) (void)hipFree(D->IO);
  if (D->partial) (void)hipFree(D->partial);
  if (D->scan_partial) (void)hipFree(D->scan_partial);
  if (D->gram_partial) (void)hipFree(D->gram_partial);
  if (D->panel_partial) (void)hipFree(D->panel_partial);
  if (D->spa_scratch) (void)hipFree(D->spa_scratch);
  if (D->wide_ws) (void)hipFree(D->wide_ws);
  for (auto t : Dev::TIMERS) (D->*t).destroy();
  if (D->pfin_rec) (void)hipFree(D->pfin_rec);
  if (D->d_out) (void)hipFree(D->d_out);
  for (auto& e : D->ev)
    if (e) (void)hipEventDestroy(e);
  for (auto& e : D->pev)
    if (e) (void)hipEventDestroy(e);
  for (auto& e : D->lev_ev)
    if (e) (void)hipEventDestroy(e);
  if (D->ev_asm) (void)hipEventDestroy(D->ev_asm);
  if (D->ev_x0) (void)hipEventDestroy(D->ev_x0);
  if (D->ev_x1) (void)hipEventDestroy(D->ev_x1);
  if (D->side) (void)hipStreamDestroy(D->side);
  if (D->side2) (void)hipStreamDestroy(D->side2);
  if (D->side3) (void)hipStreamDestroy(D->side3);
  if (D->outside_st) (void)hipStreamDestroy(D->outside_st);
  for (auto& e : D->out_evs)
    if (e) (void)hipEventDestroy(e);
  if (D->h_chain_err) (void)hipHostFree(D->h_chain_err);
  if (D->stream) (void)hipStreamDestroy(D->stream);
  for (auto& e : D->done_ev)
    if (e) (void)hipEventDestroy(e);
  for (auto& e : D->batch_ev)
    if (e) (void)hipEventDestroy(e);
  for (auto& e : D->bpev)
    if (e) (void)hipEventDestroy(e);
  if (D->bstream) (void)hipStreamDestroy(D->bstream);
  delete D;
}

void dist_layout(const Symbolic& S, int32_t rank, int32_t world, const Tuning& tune, DistLayout* o) {
  o->loff.assign(S.sn_loff.begin(), S.sn_loff.end());
  o->nL = std::max<int64_t>(S.nnzL_stored, 1);
  o->first = S.nsuper;
  if (world <= 1 || S.dense_first >= S.nsuper) return;
  o->first = S.dense_first;
  int32_t wg = world;
  while (wg < 8) wg += world;
  if (tune.dist_group) wg = std::max(world, *tune.dist_group / world * world);
  o->Wg = wg;
  o->G = 4 * wg;
  const int32_t nT = S.nsuper - o->first;
  int64_t at = S.sn_loff[o->first];
  for (int32_t jj = 0; jj < nT; ++jj) {
    const int32_t f = o->first + jj;
    const int64_t sz = S.sn_loff[f + 1] - S.sn_loff[f];
    o->slot = std::max(o->slot, (sz + 1) & ~(int64_t)1);
    if (jj % world == rank) {
      o->loff[f] = at;
      at += (sz + 1) & ~(int64_t)1;
    }
  }
  o->ring_base = at;
  const int32_t nslots = std::min(o->G, nT);
  for (int32_t jj = 0; jj < nT; ++jj)
    if (jj % world != rank) o->loff[o->first + jj] = o->ring_base + (int64_t)(jj % o->G) * o->slot;
  o->nL = o->ring_base + (int64_t)nslots * o->slot;
  o->loff[S.nsuper] = o->nL;
}

namespace {

// Expand the small combos to the cell lists of k_sparse_cells on the device (see cellplan.hip.h).
// (ccparts: the small combos as the classification threads produced them, in tile order; they are uploaded part by
// part -- concatenating 17 GB of them on the host first cost seconds of every first evaluation at the 1M config)
int build_cells_device(scilmm_symbolic* sym, Dev* D, const std::vector<const std::vector<CellCombo>*>& ccparts, int32_t NL,
                       int64_t* ngroups_total, int64_t* n_early) {
  const Symbolic& S = *sym->S;
  int64_t ncc = 0;
  for (auto* pv : ccparts) ncc += (int64_t)pv->size();
  std::vector<int64_t> off((size_t)ncc + 1, 0);
  {
    int64_t c = 0;
    for (auto* pv : ccparts)
      for (const CellCombo& q : *pv) {
        off[(size_t)c + 1] = off[(size_t)c] + (int64_t)q.nt * q.nq;
        ++c;
      }
  }
  const int64_t total = off[(size_t)ncc];
  auto dmalloc = [&](void** p, size_t bytes) -> int {
    HIPCHK(hipMalloc(p, std::max<size_t>(bytes, 8)));
    return SCILMM_OK;
  };
  int st;
  DevScratch tmp(&sym->err);  // freed on exit
  for (int c = 0; c < 3; ++c) {
    D->cellset[c].level_ptr.assign(S.nlevels + 1, 0);
    D->cellset[c].level_short.assign(std::max<int32_t>(NL, 1), 0);
  }
  *ngroups_total = 0;
  *n_early = 0;
  D->n_cells = 0;
  if (total == 0) {
    void* d8 = nullptr;
    if ((st = dmalloc(&d8, 64)) != SCILMM_OK) return st;
    D->allocs.push_back(d8);
    HIPCHK(hipMemset(d8, 0, 64));
    for (int c = 0; c < 3; ++c) {
      Dev::CellSet& CS = D->cellset[c];
      CS.dst = CS.grp = CS.srct = CS.srcq = (int64_t*)d8;
      CS.md = CS.wd = (int32_t*)d8;
    }
    return SCILMM_OK;
  }
  CellCombo* d_cc = nullptr; int64_t* d_off = nullptr;
  unsigned long long *key = nullptr, *skey = nullptr, *d_ninv = nullptr;
  uint32_t *idx = nullptr, *sidx = nullptr;
  int64_t *cst = nullptr, *csq = nullptr; int32_t *cmd = nullptr, *cwd = nullptr;
  TRY(tmp.alloc((size_t)ncc, &d_cc));
  TRY(tmp.alloc((size_t)(ncc + 1), &d_off));
  {
    size_t at = 0;
    for (auto* pv : ccparts) {
      if (!pv->empty()) HIPCHK(hipMemcpy(d_cc + at, pv->data(), sizeof(CellCombo) * pv->size(), hipMemcpyHostToDevice));
      at += pv->size();
    }
  }
  HIPCHK(hipMemcpy(d_off, off.data(), sizeof(int64_t) * (size_t)(ncc + 1), hipMemcpyHostToDevice));
  TRY(tmp.alloc((size_t)total, &key));
  TRY(tmp.alloc((size_t)total, &skey));
  TRY(tmp.alloc((size_t)total, &idx));
  TRY(tmp.alloc((size_t)total, &sidx));
  TRY(tmp.alloc((size_t)total, &cst));
  TRY(tmp.alloc((size_t)total, &csq));
  TRY(tmp.alloc((size_t)total, &cmd));
  TRY(tmp.alloc((size_t)total, &cwd));
  TRY(tmp.alloc(1, &d_ninv));
  HIPCHK(hipMemset(d_ninv, 0, 8));
  hipStream_t s0 = D->stream;
  hipLaunchKernelGGL(k_emit_cells, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 1 << 20)), dim3(256), 0, s0, total, ncc,
                     (const CellCombo*)d_cc, (const int64_t*)d_off, D->v.sn_rows, key, idx, cst, csq, cmd, cwd, d_ninv);
  uint8_t* cubtmp = nullptr;
  size_t cubbytes = 0, need = 0;
  auto ensure_tmp = [&](size_t bytes) -> int {
    if (bytes <= cubbytes) return SCILMM_OK;
    TRY(tmp.alloc(bytes, &cubtmp));  // the smaller one is freed at exit as well
    cubbytes = bytes;
    return SCILMM_OK;
  };
  HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, need, key, skey, idx, sidx, total, 0, 62, s0));
  if ((st = ensure_tmp(need)) != SCILMM_OK) return st;
  need = cubbytes;
  HIPCHK(hipcub::DeviceRadixSort::SortPairs(cubtmp, need, key, skey, idx, sidx, total, 0, 62, s0));
  unsigned long long ninv = 0;
  HIPCHK(hipMemcpyAsync(&ninv, d_ninv, 8, hipMemcpyDeviceToHost, s0));
  HIPCHK(hipStreamSynchronize(s0));
  const int64_t nvalid = total - (int64_t)ninv;
  D->n_cells = nvalid;
  // groups of equal key (= equal class, level, target address)
  unsigned long long* ukey = nullptr; int64_t* ucnt = nullptr; int64_t* ustart = nullptr; int64_t* d_ng = nullptr;
  TRY(tmp.alloc((size_t)std::max<int64_t>(nvalid, 1), &ukey));
  TRY(tmp.alloc((size_t)std::max<int64_t>(nvalid, 1), &ucnt));
  TRY(tmp.alloc(1, &d_ng));
  HIPCHK(hipMemset(d_ng, 0, 8));
  int64_t ng = 0;
  if (nvalid > 0) {
    need = 0;
    HIPCHK(hipcub::DeviceRunLengthEncode::Encode(nullptr, need, skey, ukey, ucnt, d_ng, (int)nvalid, s0));
    if ((st = ensure_tmp(need)) != SCILMM_OK) return st;
    need = cubbytes;
    HIPCHK(hipcub::DeviceRunLengthEncode::Encode(cubtmp, need, skey, ukey, ucnt, d_ng, (int)nvalid, s0));
    HIPCHK(hipMemcpyAsync(&ng, d_ng, 8, hipMemcpyDeviceToHost, s0));
    HIPCHK(hipStreamSynchronize(s0));
  }
  *ngroups_total = ng;
  // final arrays (kept): group targets, entry offsets, entries
  int64_t *udst = nullptr, *grp2 = nullptr, *ost = nullptr, *osq = nullptr; int32_t *omd = nullptr, *owd = nullptr;
  if ((st = dmalloc((void**)&udst, 8 * (size_t)std::max<int64_t>(ng, 1))) != SCILMM_OK) return st; D->allocs.push_back(udst);
  if ((st = dmalloc((void**)&grp2, 8 * (size_t)(ng + 1))) != SCILMM_OK) return st; D->allocs.push_back(grp2);
  if ((st = dmalloc((void**)&ost, 8 * (size_t)std::max<int64_t>(nvalid, 1))) != SCILMM_OK) return st; D->allocs.push_back(ost);
  if ((st = dmalloc((void**)&osq, 8 * (size_t)std::max<int64_t>(nvalid, 1))) != SCILMM_OK) return st; D->allocs.push_back(osq);
  if ((st = dmalloc((void**)&omd, 4 * (size_t)std::max<int64_t>(nvalid, 1))) != SCILMM_OK) return st; D->allocs.push_back(omd);
  if ((st = dmalloc((void**)&owd, 4 * (size_t)std::max<int64_t>(nvalid, 1))) != SCILMM_OK) return st; D->allocs.push_back(owd);
  std::vector<unsigned int> counters((size_t)3 * NL * 2, 0u);
  if (ng > 0) {
    TRY(tmp.alloc((size_t)ng, &ustart));
    need = 0;
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, need, ucnt, ustart, (int)ng, s0));
    if ((st = ensure_tmp(need)) != SCILMM_OK) return st;
    need = cubbytes;
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(cubtmp, need, ucnt, ustart, (int)ng, s0));
    unsigned long long *gkey = nullptr, *gkey_s = nullptr; uint32_t *gidx = nullptr, *order = nullptr; int64_t* cnt2 = nullptr;
    unsigned int* d_counters = nullptr;
    TRY(tmp.alloc((size_t)ng, &gkey));
    TRY(tmp.alloc((size_t)ng, &gkey_s));
    TRY(tmp.alloc((size_t)ng, &gidx));
    TRY(tmp.alloc((size_t)ng, &order));
    TRY(tmp.alloc((size_t)ng, &cnt2));
    TRY(tmp.alloc(counters.size(), &d_counters));
    HIPCHK(hipMemsetAsync(d_counters, 0, 4 * counters.size(), s0));
    const unsigned gb = (unsigned)((ng + 255) / 256);
    hipLaunchKernelGGL(k_group_keys, dim3(gb), dim3(256), 0, s0, ng, (const unsigned long long*)ukey, (const int64_t*)ucnt,
                       (int64_t)16, gkey, gidx);
    need = 0;
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, need, gkey, gkey_s, gidx, order, ng, 0, 62, s0));
    if ((st = ensure_tmp(need)) != SCILMM_OK) return st;
    need = cubbytes;
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(cubtmp, need, gkey, gkey_s, gidx, order, ng, 0, 62, s0));
    hipLaunchKernelGGL(k_gather_counts, dim3(gb), dim3(256), 0, s0, ng, (const uint32_t*)order, (const int64_t*)ucnt, cnt2);
    need = 0;
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, need, cnt2, grp2, (int)ng, s0));
    if ((st = ensure_tmp(need)) != SCILMM_OK) return st;
    need = cubbytes;
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(cubtmp, need, cnt2, grp2, (int)ng, s0));
    HIPCHK(hipMemcpy(grp2 + ng, &nvalid, 8, hipMemcpyHostToDevice));  // one element past what the scan writes
    hipLaunchKernelGGL(k_finish_groups, dim3(gb), dim3(256), 0, s0, ng, (const unsigned long long*)gkey_s, udst);
    hipLaunchKernelGGL(k_bucket_counts, dim3((unsigned)((counters.size() + 255) / 256)), dim3(256), 0, s0, (int32_t)counters.size(), NL,
                       ng, (const unsigned long long*)gkey_s, d_counters);
    hipLaunchKernelGGL(k_gather_entries, dim3((unsigned)std::min<int64_t>((nvalid + 255) / 256, 1 << 20)), dim3(256), 0, s0, nvalid, ng,
                       (const int64_t*)grp2, (const uint32_t*)order, (const int64_t*)ustart, (const uint32_t*)sidx,
                       (const int64_t*)cst, (const int64_t*)csq, (const int32_t*)cmd, (const int32_t*)cwd, ost, osq, omd, owd);
    HIPCHK(hipMemcpyAsync(counters.data(), d_counters, 4 * counters.size(), hipMemcpyDeviceToHost, s0));
    HIPCHK(hipStreamSynchronize(s0));
  } else {
    const int64_t zero = 0;
    HIPCHK(hipMemcpy(grp2, &zero, 8, hipMemcpyHostToDevice));
  }
  HIPCHK(hipGetLastError());
  int64_t gbase = 0, ebase_unused = 0;
  (void)ebase_unused;
  for (int c = 0; c < 3; ++c) {
    Dev::CellSet& CS = D->cellset[c];
    CS.dst = udst + gbase;
    CS.grp = grp2 + gbase;
    CS.srct = ost;
    CS.srcq = osq;
    CS.md = omd;
    CS.wd = owd;
    int64_t run = 0;
    for (int32_t l = 0; l < NL; ++l) {
      const int64_t ns = counters[((size_t)c * NL + l) * 2], nl = counters[((size_t)c * NL + l) * 2 + 1];
      if (l < S.nlevels) {
        CS.level_short[l] = ns;
        run += ns + nl;
        CS.level_ptr[l + 1] = run;
      }
    }
    if (c == 0) *n_early = run;  // groups of the early class (diagnostic)
    gbase += run;
  }
  return SCILMM_OK;
}

// Between the stages of ensure_device: what a stage leaves for a later one and is not device state.  It lives for the
// duration of one ensure_device call.
struct Cell { int64_t dst, st, sq; int32_t md, wd, level, late; };  // late: 0 early (side streams), 1 late (main stream)
struct PlanBuild {
  bool verbose = false;                               // SCILMM_VERBOSE: the [scilmm plan] lines
  std::chrono::steady_clock::time_point lap_start = std::chrono::steady_clock::now();
  void lap(const char* what) {
    auto now = std::chrono::steady_clock::now();
    if (verbose) fprintf(stderr, "[scilmm plan] %-30s %8.3f s\n", what, std::chrono::duration<double>(now - lap_start).count());
    lap_start = now;
  }
  // classify_combos -> build_cells, cut_work_items
  std::vector<int64_t> dptr, dmid;                    // per tile: its dense combos in d_combos, their early|late split
  std::vector<uint8_t> cd_cost;                       // per dense-path combo: 1 + K chunks (what the work-item cuts need)
  bool gpu_cells = true;
  std::vector<Cell> cells;                            // host cell path: the cells, in tile order
  std::vector<std::vector<CellCombo>> cellparts;      // device cell path: the small combos, one vector per classification thread (tile order)
};

inline bool distributed_tail(const Dev* D, const Symbolic& S) { return D->world > 1 && D->dist_first < S.nsuper; }
// columns of the dense tail (0: none)
inline int32_t tail_width(const Symbolic& S) { return S.dense_first < S.nsuper ? S.n - S.sn_start[S.dense_first] : 0; }

int create_streams_and_events(scilmm_symbolic* sym, Dev* D) {
  const Symbolic& S = *sym->S;
  {
    // the main stream carries the latency-bound per-level chain: give it dispatch priority over the side
    // stream that streams the look-ahead updates
    int& lo = D->prio_lo;
    int& hi = D->prio_hi;
    HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
    HIPCHK(hipStreamCreateWithPriority(&D->stream, hipStreamNonBlocking, hi));
    // SCILMM_RESERVE_CUS = r > 0: the look-ahead side streams are created with a CU mask that leaves r CUs per
    // XCD-group free, so the main stream's single-workgroup kernels never queue behind resident update items.
    const int reserve = D->tune.reserve_cus;
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, D->device));
    const int ncu = prop.multiProcessorCount;
    if (reserve > 0 && reserve < ncu) {
      std::vector<uint32_t> mask((size_t)(ncu + 31) / 32, 0u);
      // keep every (ncu / reserve)-th CU out of the mask so the reserved CUs are spread over the XCDs
      const int stride = std::max(1, ncu / reserve);
      int kept_out = 0;
      for (int c = 0; c < ncu; ++c) {
        const bool out = (c % stride == stride - 1) && kept_out < reserve;
        if (out) { kept_out++; continue; }
        mask[c / 32] |= (1u << (c % 32));
      }
      HIPCHK(hipExtStreamCreateWithCUMask(&D->side, (uint32_t)mask.size(), mask.data()));
      HIPCHK(hipExtStreamCreateWithCUMask(&D->side2, (uint32_t)mask.size(), mask.data()));
    } else {
      HIPCHK(hipStreamCreateWithPriority(&D->side, hipStreamNonBlocking, lo));
      HIPCHK(hipStreamCreateWithPriority(&D->side2, hipStreamNonBlocking, lo));
      if (D->tune.side_streams == 3) {
        HIPCHK(hipStreamCreateWithPriority(&D->side3, hipStreamNonBlocking, lo));
        D->nside = 3;
      } else if (D->tune.side_streams == 1) {
        D->nside = 1;  // early updates strictly one after the other (their launch durations then do not overlap)
      }
    }
  }
  HIPCHK(hipEventCreateWithFlags(&D->ev_asm, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&D->ev_x0, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&D->ev_x1, hipEventDisableTiming));
  D->lev_ev.assign((size_t)2 * std::max(S.nlevels, 1), nullptr);
  for (auto& e : D->lev_ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  for (auto& e : D->ev) HIPCHK(hipEventCreate(&e));
  return SCILMM_OK;
}

// The distributed tail's events and the batches' stream (plan_ownership: they follow the tail fronts' levels and groups)
int create_dist_streams_and_events(scilmm_symbolic* sym, Dev* D, int32_t ngroups) {
  const Symbolic& S = *sym->S;
  D->done_ev.assign((size_t)std::max(S.nlevels, 1), nullptr);
  for (int32_t l = 0; l < S.nlevels; ++l)
    if (D->tail_of_level[l] >= 0) HIPCHK(hipEventCreateWithFlags(&D->done_ev[l], hipEventDisableTiming));
  D->batch_ev.assign((size_t)ngroups, nullptr);
  for (auto& e : D->batch_ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  HIPCHK(hipStreamCreateWithPriority(&D->bstream, hipStreamNonBlocking, D->prio_lo));
  return SCILMM_OK;
}

int check_block_widths(scilmm_symbolic* sym) {
  const Symbolic& S = *sym->S;
  for (int32_t b = 0; b < S.nsuper; ++b)
    if (S.sn_start[b + 1] - S.sn_start[b] > NB) {
      sym->err = "symbolic analysis has supernode blocks wider than the kernels' block width (max_width > NB)";
      return SCILMM_ERR_ARG;
    }
  return SCILMM_OK;
}

// ---- multi-GPU ownership and rank-local storage; the level lists of this rank
int plan_ownership(scilmm_symbolic* sym, Dev* D, PlanBuild& pb) {
  const Symbolic& S = *sym->S;
  D->rank = sym->rank;
  D->world = std::max<int32_t>(1, sym->world);
  D->comm = (hipStream_t)sym->comm_stream;
  D->keep_front.assign((size_t)std::max(S.nsuper, 1), 1);
  D->tail_of_level.assign((size_t)std::max(S.nlevels, 1), -1);
  {
    DistLayout lay;
    dist_layout(S, D->rank, D->world, D->tune, &lay);
    D->dist_first = lay.first;
    D->dist_Wg = lay.Wg;
    D->dist_G = lay.G;
    D->loff.swap(lay.loff);
    D->nL_local = lay.nL;
  }
  if (D->world > 1 && D->dist_first < S.nsuper) {
    const int32_t nT = S.nsuper - D->dist_first, ngroups = (nT + D->dist_Wg - 1) / D->dist_Wg;
    for (int32_t f = D->dist_first; f < S.nsuper; ++f) {
      D->keep_front[f] = ((f - D->dist_first) % D->world) == D->rank ? 1 : 0;
      if (D->tail_of_level[S.sn_level[f]] >= 0) {
        sym->err = "multi-GPU: two fronts of the dense tail share a level (the tail is expected to be a chain)";
        return SCILMM_ERR_ARG;
      }
      D->tail_of_level[S.sn_level[f]] = f;
    }
    int st = create_dist_streams_and_events(sym, D, ngroups);
    if (st != SCILMM_OK) return st;
    D->last_own_level.assign((size_t)ngroups, -1);
    for (int32_t f = D->dist_first; f < S.nsuper; ++f)
      if (D->keep_front[f]) D->last_own_level[(size_t)((f - D->dist_first) / D->dist_Wg)] = S.sn_level[f];
    if (pb.verbose)
      fprintf(stderr, "[scilmm plan] rank %d of %d: %d tail panels distributed (every %d-th one mine), groups of %d, ring of %d slots; "
              "local panel storage %.2f GB of %.2f GB\n", D->rank, D->world, nT, D->world, D->dist_Wg, D->dist_G,
              8e-9 * (double)D->nL_local, 8e-9 * (double)S.nnzL_stored);
  }
  // level lists of this rank: everything except the tail fronts of other ranks
  {
    D->lv_ptr.assign(1, 0);
    D->lv_tile_ptr.assign(1, 0);
    D->lv_pair_ptr.assign(1, 0);
    for (int32_t l = 0; l < S.nlevels; ++l) {
      for (int32_t q = S.level_ptr[l]; q < S.level_ptr[l + 1]; ++q)
        if (D->keep_front[S.level_fronts[q]]) D->lv_fronts.push_back(S.level_fronts[q]);
      // (tiles of an own distributed panel last: the forward sweep pushes them into a different accumulator)
      for (int64_t q = S.level_tile_ptr[l]; q < S.level_tile_ptr[l + 1]; ++q)
        if (S.tile_front[S.level_tiles[q]] < D->dist_first) D->lv_tiles.push_back(S.level_tiles[q]);
      D->lv_tile_mid.push_back((int64_t)D->lv_tiles.size());
      for (int64_t q = S.level_tile_ptr[l]; q < S.level_tile_ptr[l + 1]; ++q)
        if (S.tile_front[S.level_tiles[q]] >= D->dist_first && D->keep_front[S.tile_front[S.level_tiles[q]]]) D->lv_tiles.push_back(S.level_tiles[q]);
      // backward pushes (target in level l -> descendant d): this rank needs the panel of d
      for (int64_t q = S.level_pair_ptr[l]; q < S.level_pair_ptr[l + 1]; ++q)
        if (D->keep_front[S.upd_src[S.level_pairs[q]]]) D->lv_pairs.push_back(S.level_pairs[q]);
      D->lv_ptr.push_back((int32_t)D->lv_fronts.size());
      D->lv_tile_ptr.push_back((int64_t)D->lv_tiles.size());
      D->lv_pair_ptr.push_back((int64_t)D->lv_pairs.size());
    }
  }
  return SCILMM_OK;
}

// dense_on / outside_on: which of the two dense-tail paths this handle takes
int choose_tail_paths(scilmm_symbolic* sym, Dev* D) {
  const Symbolic& S = *sym->S;
  const int32_t tail_w = tail_width(S);
  {
    // The dense-tail path (k_dense_b + k_outside) serves every tail of 8192+ columns.  Round 2 kept the 100k config (15.7k
    // columns, 123 panels) on the explicit path (its one-workgroup-per-CU items balanced worse: 66 -> 72 ms); with k_dense_b,
    // k_outside and SHORT launches of ~128 items fitted to whole rounds of workgroups it is the faster one there too:
    // 65.3 -> 58.6 ms (items 64 / 96 / 128 / 192 / 256 / 512: 60.0 / 59.2 / 58.6 / 60.6 / 60.9 / 60.4; without k_outside 66.3;
    // without the fitting 62.7).  SCILMM_DENSE=1 / 0 forces it.
    // (k_dense_b has no scalar form: with SCILMM_NO_MFMA=1 the tail goes through the explicit items of k_update2<false>)
    D->dense_on = S.dense_first < S.nsuper && D->use_mfma && D->tune.dense.value_or(tail_w >= 8192);
    // a distributed tail is always updated by the implicit items (the batches have no explicit-combo form)
    if (distributed_tail(D, S)) D->dense_on = true;
    if (D->dense_on && !D->d_zeros) {
      HIPCHK(hipMalloc((void**)&D->d_zeros, 2048));
      HIPCHK(hipMemset(D->d_zeros, 0, 2048));
    }
  }
  {
    // k_outside takes over the update pairs (tail target, prelude descendant below the tail's first level) unless the
    // caller asks for the bitwise-reproducible schedule (scilmm_set_deterministic / SCILMM_DETERMINISTIC=1) or the combos
    // were already built
    D->outside_desc.assign((size_t)std::max(S.nsuper, 1), 0);
    // (switched on with the dense-tail path, by the width of the tail -- SCILMM_OUTSIDE=1 / 0 forces it)
    D->outside_on = S.dense_first < S.nsuper && !D->det && !sym->S->combos_built && D->tune.outside.value_or(tail_w >= 8192);
  }
  return SCILMM_OK;
}

// The k_outside plan: items, groups of descendants with identical tail rows, progressive chunks (outside_on only)
int plan_outside(scilmm_symbolic* sym, Dev* D, PlanBuild& pb) {
  const Symbolic& S = *sym->S;
  int st = SCILMM_OK;
  D->tail_level = S.sn_level[S.dense_first];
  const int32_t c0_tail = S.sn_start[S.dense_first];
  std::vector<OutsideWork> ow;
  // descendants with IDENTICAL tail rows (the 128-column blocks of one wide supernode) form a group: one set of items for
  // the group's leader, the kernel sums the members' products in its registers before the one atomic scatter
  std::vector<int32_t> grp_next((size_t)std::max(S.nsuper, 1), -1), grp_t0((size_t)std::max(S.nsuper, 1), 0);
  std::vector<int32_t> grp_width((size_t)std::max(S.nsuper, 1), 0);  // leader -> columns of the whole group
  {
    const bool merge = D->tune.outside_merge;
    std::vector<std::pair<uint64_t, int32_t>> keyed;  // (hash of the tail rows, descendant)
    for (int32_t d = 0; d < S.dense_first; ++d) {
      if (S.sn_level[d] >= D->tail_level) continue;  // finished too late for the launches before the tail
      const int32_t* rd = S.sn_rows.data() + S.sn_rowptr[d];
      const int32_t md = (int32_t)(S.sn_rowptr[d + 1] - S.sn_rowptr[d]);
      const int32_t t0 = (int32_t)(std::lower_bound(rd, rd + md, c0_tail) - rd);
      if (t0 >= md) continue;
      D->outside_desc[d] = 1;
      grp_t0[(size_t)d] = t0;
      uint64_t h = 1469598103934665603ull ^ (uint64_t)(md - t0);
      for (int32_t t = t0; t < md; ++t) h = (h ^ (uint64_t)(uint32_t)rd[t]) * 1099511628211ull;
      keyed.push_back({merge ? h : (uint64_t)d, d});
    }
    std::stable_sort(keyed.begin(), keyed.end(), [](const std::pair<uint64_t, int32_t>& a, const std::pair<uint64_t, int32_t>& b) { return a.first < b.first; });
    auto same_rows = [&](int32_t a, int32_t b) -> bool {
      const int64_t na = S.sn_rowptr[a + 1] - S.sn_rowptr[a] - grp_t0[(size_t)a], nb = S.sn_rowptr[b + 1] - S.sn_rowptr[b] - grp_t0[(size_t)b];
      return na == nb && std::memcmp(S.sn_rows.data() + S.sn_rowptr[a] + grp_t0[(size_t)a], S.sn_rows.data() + S.sn_rowptr[b] + grp_t0[(size_t)b],
                                     sizeof(int32_t) * (size_t)na) == 0;
    };
    std::vector<int32_t> leaders;
    for (size_t i = 0; i < keyed.size();) {
      // members of one hash bucket, split into runs of truly identical row lists (a collision must not merge anything)
      size_t j = i;
      while (j < keyed.size() && keyed[j].first == keyed[i].first) ++j;
      std::vector<uint8_t> used(j - i, 0);
      for (size_t a = i; a < j; ++a) {
        if (used[a - i]) continue;
        const int32_t lead = keyed[a].second;
        leaders.push_back(lead);
        int32_t last = lead;
        grp_width[(size_t)lead] = S.sn_start[lead + 1] - S.sn_start[lead];
        for (size_t b = a + 1; b < j; ++b) {
          if (used[b - i] || !merge || !same_rows(lead, keyed[b].second)) continue;
          used[b - i] = 1;
          grp_next[(size_t)last] = keyed[b].second;
          last = keyed[b].second;
          grp_width[(size_t)lead] += S.sn_start[last + 1] - S.sn_start[last];
        }
      }
      i = j;
    }
    std::sort(leaders.begin(), leaders.end());
    // multi-GPU: a block pair adds into the panels of the columns of its block bj only; a rank keeps the pairs that reach
    // a panel it owns (a 128-row block of a tall front spans a few panels: at 8 ranks most pairs are somebody else's --
    // until round 4 every rank multiplied all of them and threw 7/8 of the products away in the epilogue)
    const bool own_only = distributed_tail(D, S);
    int64_t pairs_all = 0;
    for (int32_t d : leaders) {
      const int32_t md = (int32_t)(S.sn_rowptr[d + 1] - S.sn_rowptr[d]), t0 = grp_t0[(size_t)d];
      const int32_t* rd = S.sn_rows.data() + S.sn_rowptr[d];
      const int32_t nb = (md - t0 + TM - 1) / TM;
      std::vector<uint8_t> col_mine((size_t)nb, 1);
      if (own_only)
        for (int32_t bj = 0; bj < nb; ++bj) {
          // panels of the block's first and last column label (sorted rows: everything in between lies between them)
          const int32_t r_lo = rd[t0 + NB * bj], r_hi = rd[std::min(md, t0 + NB * (bj + 1)) - 1];
          int32_t f_lo = (int32_t)(std::upper_bound(S.sn_start.begin() + S.dense_first, S.sn_start.begin() + S.nsuper + 1, r_lo) - S.sn_start.begin()) - 1;
          int32_t f_hi = (int32_t)(std::upper_bound(S.sn_start.begin() + S.dense_first, S.sn_start.begin() + S.nsuper + 1, r_hi) - S.sn_start.begin()) - 1;
          uint8_t mine = 0;
          for (int32_t f = f_lo; f <= f_hi && !mine; ++f) mine = D->keep_front[(size_t)f];
          col_mine[(size_t)bj] = mine;
        }
      for (int32_t bi = 0; bi < nb; ++bi)
        for (int32_t bj = 0; bj <= bi; ++bj) {
          ++pairs_all;
          if (col_mine[(size_t)bj]) ow.push_back(OutsideWork{d, t0, bi, bj});
        }
    }
    if (pb.verbose)
      fprintf(stderr, "[scilmm plan] k_outside: %zu descendants in %zu groups of identical tail rows; %lld of %lld block pairs reach a panel of this rank\n",
              keyed.size(), leaders.size(), (long long)ow.size(), (long long)pairs_all);
  }
  D->n_owork = (int64_t)ow.size();
  if (D->n_owork == 0 || D->tail_level == 0) {
    D->outside_on = false;
    std::fill(D->outside_desc.begin(), D->outside_desc.end(), 0);
  } else {
    std::vector<int32_t> tf((size_t)(S.n - c0_tail));
    for (int32_t f = S.dense_first; f < S.nsuper; ++f)
      for (int32_t c = S.sn_start[f]; c < S.sn_start[f + 1]; ++c) tf[(size_t)(c - c0_tail)] = f;
    // first tail panel an item touches = the panel of its smallest column label (first row of block bj)
    auto first_front = [&](const OutsideWork& w) -> int32_t {
      return tf[(size_t)(S.sn_rows[S.sn_rowptr[w.d] + w.t0 + NB * w.bj] - c0_tail)];
    };
    // (100k / 300k factorization, ms: 1 chunk 57.8 / 1357; 4 / 8 / 16 chunks on a low-priority stream 55.5 / 1344, - / 1339, 56.1 / 1335)
    // ... and the count follows the size: one chunk per ~16k block pairs, 4 .. 32 (1M: 2 / 8 / 32 chunks 26.64 / 26.63 / 26.51 s)
    const int32_t want_chunks = std::max(1, D->tune.outside_chunks.value_or((int32_t)std::min<int64_t>(32, std::max<int64_t>(4, (int64_t)ow.size() / 16384))));
    std::vector<int32_t> ffront(ow.size());
    for (size_t i = 0; i < ow.size(); ++i) ffront[i] = first_front(ow[i]);
    std::vector<size_t> ord(ow.size());
    for (size_t i = 0; i < ord.size(); ++i) ord[i] = i;
    std::stable_sort(ord.begin(), ord.end(), [&](size_t a, size_t b) { return ffront[a] < ffront[b]; });
    // chunk boundaries where the first panel changes, about equal item counts
    D->ochunk_ptr.assign(1, 0);
    std::vector<int32_t> chunk_lo;  // first panel of the chunk's first item
    {
      const size_t N = ord.size();
      size_t panels = N ? 1 : 0;  // distinct first panels
      for (size_t k = 1; k < N; ++k) panels += ffront[ord[k]] != ffront[ord[k - 1]];
      // (as many chunks as there are first panels, or more, were asked for: one chunk per panel, however few items it holds)
      const size_t per = (size_t)want_chunks >= panels ? 1 : std::max<size_t>(1, (N + want_chunks - 1) / want_chunks);
      size_t i = 0;
      while (i < N) {
        chunk_lo.push_back(ffront[ord[i]]);
        size_t e = std::min(N, i + per);
        while (e < N && ffront[ord[e]] == ffront[ord[e - 1]]) ++e;
        D->ochunk_ptr.push_back((int64_t)e);
        i = e;
      }
    }
    const int32_t nch = (int32_t)chunk_lo.size();
    // inside a chunk: widest descendants first (all items are 128 x 128 x w_d: the long ones start early)
    {
      std::vector<OutsideWork> sorted(ow.size());
      for (int32_t g = 0; g < nch; ++g) {
        std::stable_sort(ord.begin() + D->ochunk_ptr[g], ord.begin() + D->ochunk_ptr[g + 1], [&](size_t a, size_t b) {
          return grp_width[(size_t)ow[a].d] > grp_width[(size_t)ow[b].d];
        });
      }
      for (size_t i = 0; i < ord.size(); ++i) sorted[i] = ow[ord[i]];
      ow.swap(sorted);
    }
    // per level: the chunk its tail front waits for = the last chunk whose first item starts at that panel or before it
    D->out_wait_chunk.assign((size_t)std::max(S.nlevels, 1), -1);
    for (int32_t f = S.dense_first; f < S.nsuper; ++f) {
      const int32_t g = (int32_t)(std::upper_bound(chunk_lo.begin(), chunk_lo.end(), f) - chunk_lo.begin()) - 1;
      int32_t& w = D->out_wait_chunk[(size_t)S.sn_level[f]];
      w = std::max(w, g);
    }
    // (a level at or above the tail's first one without a tail front of its own waits like the level before it)
    for (int32_t l = D->tail_level + 1; l < S.nlevels; ++l)
      D->out_wait_chunk[(size_t)l] = std::max(D->out_wait_chunk[(size_t)l], D->out_wait_chunk[(size_t)l - 1]);
    D->out_evs.assign((size_t)nch, nullptr);
    for (auto& e : D->out_evs) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    if ((st = upload(sym, D, ow, &D->d_owork)) != SCILMM_OK) return st;
    {
      if ((st = upload(sym, D, grp_next, &D->d_grp_next)) != SCILMM_OK) return st;
      if ((st = upload(sym, D, grp_t0, &D->d_grp_t0)) != SCILMM_OK) return st;
    }
    if ((st = upload(sym, D, tf, &D->d_tail_front)) != SCILMM_OK) return st;
    if ((st = upload(sym, D, D->keep_front, &D->d_keep_front)) != SCILMM_OK) return st;
    {
      // SCILMM_OUTSIDE_PRIO = 1: the chain's priority, 0: the look-ahead streams'
      // (low: the chunks that later panels wait for fill the gaps of the chain-bound first tail levels instead of taking
      //  the chain's CU slots -- with the chain's priority the overlap gains nothing)
      HIPCHK(hipStreamCreateWithPriority(&D->outside_st, hipStreamNonBlocking, D->tune.outside_prio ? D->prio_hi : D->prio_lo));
    }
    if (pb.verbose) {
      fprintf(stderr, "[scilmm plan] k_outside: %lld block-pair items of prelude fronts below level %d (tail starts at column %d), %d chunks by first panel:",
              (long long)D->n_owork, D->tail_level, c0_tail, nch);
      for (int32_t g = 0; g < nch; ++g) fprintf(stderr, " [%d..: %lld]", chunk_lo[g] - S.dense_first, (long long)(D->ochunk_ptr[g + 1] - D->ochunk_ptr[g]));
      fprintf(stderr, "\n");
      fprintf(stderr, "[scilmm plan] k_outside: on a stream of %s priority\n", D->tune.outside_prio ? "the chain's" : "the look-ahead streams'");
    }
  }
  return SCILMM_OK;
}

// The symbolic arrays, the value-assembly maps (rank-local offsets when distributed) and the level lists on the device
int upload_symbolic(scilmm_symbolic* sym, Dev* D) {
  const Symbolic& S = *sym->S;
  const std::vector<int64_t>& LOFF = D->loff;
  D->v.n = S.n;
  D->v.nsuper = S.nsuper;
  int st;
#define UP(field, vec)                                          \
  if ((st = upload(sym, D, S.vec, &D->v.field)) != SCILMM_OK) return st;
  UP(sn_start, sn_start)
  UP(sn_rowptr, sn_rowptr)
  UP(sn_rows, sn_rows)
  if ((st = upload(sym, D, D->loff, &D->v.sn_loff)) != SCILMM_OK) return st;
  UP(inv_off, inv_off)
  UP(upd_src, upd_src)
  UP(upd_p0, upd_p0)
  UP(upd_p1, upd_p1)
  UP(tile_front, tile_front)
  UP(tile_base, tile_base)
  // (the per-tile combo arrays stay on the host: the kernels read the flattened descriptors of classify_combos)
  if (distributed_tail(D, S)) {
    // value-assembly maps in rank-local offsets; entries of other ranks' tail panels are dropped (-1)
    std::vector<int64_t> ad(S.asm_dst.size()), dd(S.diag_dst.size());
    const int nth = std::max(1, std::min(16, scilmm::host_threads()));
    std::vector<std::thread> pool;
    auto part = [&](int q) {
      for (int32_t f = q; f < S.nsuper; f += nth) {
        const bool keep = D->keep_front[f] != 0;
        const int64_t delta = LOFF[f] - S.sn_loff[f];
        for (int32_t j = S.sn_start[f]; j < S.sn_start[f + 1]; ++j) {
          dd[(size_t)j] = keep ? S.diag_dst[(size_t)j] + delta : -1;
          for (int64_t e = S.pat_colptr[j]; e < S.pat_colptr[j + 1]; ++e) ad[(size_t)e] = keep ? S.asm_dst[(size_t)e] + delta : -1;
        }
      }
    };
    for (int q = 1; q < nth; ++q) pool.emplace_back(part, q);
    part(0);
    for (auto& th : pool) th.join();
    if ((st = upload(sym, D, ad, &D->v.asm_dst)) != SCILMM_OK) return st;
    if ((st = upload(sym, D, dd, &D->v.diag_dst)) != SCILMM_OK) return st;
  } else {
    UP(asm_dst, asm_dst)
    UP(diag_dst, diag_dst)
  }
  UP(pat_colptr, pat_colptr)
  UP(pat_row, pat_row)
  UP(perm, perm)
#undef UP
  if ((st = upload(sym, D, D->lv_tiles, &D->d_level_tiles)) != SCILMM_OK) return st;
  if ((st = upload(sym, D, D->lv_fronts, &D->d_level_fronts)) != SCILMM_OK) return st;
  if ((st = upload(sym, D, D->lv_pairs, &D->d_level_pairs)) != SCILMM_OK) return st;
  if (D->world > 1) {
    // L*R: every panel is multiplied by exactly one rank (own tail panels; the replicated prelude by rank 0), then summed
    std::vector<int32_t> lt;
    for (int32_t g : D->lv_tiles)
      if (S.tile_front[g] >= D->dist_first || D->rank == 0) lt.push_back(g);
    D->n_lmul_tiles = (int64_t)lt.size();
    if ((st = upload(sym, D, lt, &D->d_lmul_tiles)) != SCILMM_OK) return st;
    if ((st = upload(sym, D, S.level_fronts, &D->d_all_fronts)) != SCILMM_OK) return st;
  }
  D->vals.assign(S.K, nullptr);
  D->have_vals.assign(S.K, 0);
  HIPCHK(hipMalloc((void**)&D->d_out, sizeof(double) * RPMAX));
  return SCILMM_OK;
}

// ---- deterministic mode: pull schedule of the forward sweep and of L*R, row index of the pattern (k_spmm_row)
int upload_deterministic_plan(scilmm_symbolic* sym, Dev* D) {
  const Symbolic& S = *sym->S;
  int st;
  scilmm::build_pull_schedule(sym->S);
  if (!scilmm::build_row_index(sym->S)) {
    sym->err = "deterministic mode: the pattern maps of this handle are not available (released before the first numeric call)";
    return SCILMM_ERR_STATE;
  }
  if ((st = upload(sym, D, S.pull_seg_front, &D->pull.seg_front)) != SCILMM_OK) return st;
  if ((st = upload(sym, D, S.pull_seg_ptr, &D->pull.seg_ptr)) != SCILMM_OK) return st;
  if ((st = upload(sym, D, S.pull_seg_slot, &D->pull.seg_slot)) != SCILMM_OK) return st;
  if ((st = upload(sym, D, S.pull_front_seg, &D->pull.front_seg)) != SCILMM_OK) return st;
  if ((st = upload(sym, D, S.pull_level_segs, &D->d_pull_level_segs)) != SCILMM_OK) return st;
  if ((st = upload(sym, D, S.pull_fold, &D->d_pull_fold)) != SCILMM_OK) return st;
  if (S.pull_max_slots > 0) {
    void* pp = nullptr;
    HIPCHK(hipMalloc(&pp, sizeof(double) * (size_t)S.pull_max_slots * NB * RPMAX));
    D->allocs.push_back(pp);
    D->d_pull_partial = (double*)pp;
  }
  if ((st = upload(sym, D, S.pat_rowptr, &D->d_pat_rowptr)) != SCILMM_OK) return st;
  if ((st = upload(sym, D, S.pat_rowslot, &D->d_pat_rowslot)) != SCILMM_OK) return st;
  if ((st = upload(sym, D, S.pat_rowcol, &D->d_pat_rowcol)) != SCILMM_OK) return st;
  // (the device holds the index now: the host copy goes, like the maps scilmm_symbolic_release_host_maps frees)
  std::vector<int64_t>().swap(sym->S->pat_rowslot);
  std::vector<int32_t>().swap(sym->S->pat_rowcol);
  std::vector<int64_t>().swap(sym->S->pat_rowptr);
  sym->S->rowidx_built = false;
  return SCILMM_OK;
}

// ---- update-kernel plan
// pairs with cells*width up to the limit take the cell-wise path
double choose_cell_limit(const Symbolic& S, const Dev* D, const PlanBuild& pb) {
  const int64_t nc = (int64_t)S.combo_pair.size();
  double cell_limit = D->tune.cell_limit.value_or(4096.0);
  if (!D->tune.cell_limit) {
    // very large patterns: keep the expanded cell plan below ~1.5e9 cells (32-bit counts in the device sort;
    // 32 B per cell) by lowering the limit -- the 1 M-individual config ends at 64
    const double cand[5] = {4096.0, 1024.0, 256.0, 64.0, 16.0};
    double cells_at[5] = {0, 0, 0, 0, 0};
    for (int64_t c = 0; c < nc; ++c) {
      const int32_t e = S.combo_pair[c];
      const int32_t d = S.upd_src[e];
      const double cellsn = (double)(S.combo_tb[c] - S.combo_ta[c]) * (double)(S.upd_p1[e] - S.upd_p0[e]);
      const double vol = cellsn * (double)(S.sn_start[d + 1] - S.sn_start[d]);
      for (int k = 0; k < 5; ++k)
        if (vol <= cand[k]) cells_at[k] += cellsn;
    }
    int pick = 0;
    while (pick < 4 && cells_at[pick] > 1.5e9) ++pick;
    cell_limit = cand[pick];
    if (pb.verbose && pick > 0)
      fprintf(stderr, "[scilmm plan] cell limit lowered to %.0f (%.3e cells)\n", cell_limit, cells_at[pick]);
  }
  return cell_limit;
}

// "late" = on the main stream, right before the target's potrf: the descendant finished at most look_depth levels below
// the target.  A DISTRIBUTED tail target takes all its explicit items late: its panel is read-modify-written by the
// batches on their own stream until its late update starts, so nothing else may touch it ahead of time.
inline bool is_late(const Symbolic& S, const Dev* D, int32_t d, int32_t sfr) {
  return D->tune.no_lookahead || S.sn_level[d] + D->look_depth >= S.sn_level[sfr] || (D->world > 1 && sfr >= D->dist_first);
}

// What one classification thread makes of its tile range
struct ClassifiedPart {
  std::vector<ComboDesc> cd;          // dense combos only, grouped by tile
  std::vector<int64_t> dend, dmidv;  // per tile: end of its dense list, its early|late split
  std::vector<Cell> cells;
  std::vector<CellCombo> cellcombos;  // device-built cell plan: the small combos themselves
  int64_t n_sparse = 0;
};

void classify_tile_range(const Symbolic& S, const Dev* D, double cell_limit, bool gpu_cells, int64_t gbeg, int64_t gend,
                         ClassifiedPart& Pt) {
  const std::vector<int64_t>& LOFF = D->loff;
  std::vector<ComboDesc>& cd = Pt.cd;
  std::vector<Cell>& cells = Pt.cells;
  std::vector<ComboDesc> late_tmp;
  for (int64_t g = gbeg; g < gend; ++g) {
    const int32_t sfr = S.tile_front[g];
    const int32_t ti = (int32_t)(g - S.tile_base[sfr]);
    const int32_t c0s = S.sn_start[sfr];
    const int64_t ms = S.sn_rowptr[sfr + 1] - S.sn_rowptr[sfr];
    const int32_t* rs = S.sn_rows.data() + S.sn_rowptr[sfr];
    const int64_t R0 = (int64_t)ti * TM;
    const int64_t tile_end = std::min<int64_t>(R0 + TM, ms);
    for (int64_t c = S.combo_ptr[g]; c < S.combo_ptr[g + 1]; ++c) {
      const int32_t e = S.combo_pair[c];
      const int32_t d = S.upd_src[e];
      ComboDesc x;
      x.loff = LOFF[d];
      x.rowoff = S.sn_rowptr[d];
      x.md = (int32_t)(S.sn_rowptr[d + 1] - S.sn_rowptr[d]);
      x.wd = S.sn_start[d + 1] - S.sn_start[d];
      x.ta = S.combo_ta[c];
      x.nt = S.combo_tb[c] - S.combo_ta[c];
      x.p0 = S.upd_p0[e];
      x.nq = S.upd_p1[e] - S.upd_p0[e];
      x.ip0 = S.combo_ip0[c];
      x.jp0 = S.upd_jp0[e];
      const bool fake_contig = D->ablate == 3;  // diagnostic: pretend every combo is contiguous (wrong numbers, timing only)
      {
        // spans in target coordinates: rows and columns of a descendant are sorted, so first/last suffice
        const int32_t* rdx = S.sn_rows.data() + x.rowoff;
        const int32_t* lo0 = rs + R0;
        x.ilo = (int32_t)(std::lower_bound(lo0, rs + tile_end, rdx[x.ta]) - lo0);
        x.ihi = (int32_t)(std::lower_bound(lo0, rs + tile_end, rdx[x.ta + x.nt - 1]) - lo0);
        x.jlo = rdx[x.p0] - c0s;
        x.jhi = rdx[x.p0 + x.nq - 1] - c0s;
      }
      if (fake_contig) {
        if (x.ip0 < 0) x.ip0 = std::min<int32_t>(x.ilo, TM - x.nt);
        if (x.jp0 < 0) x.jp0 = std::min<int32_t>(x.jlo, NB - x.nq);
      }
      if ((double)x.nt * (double)x.nq * (double)x.wd > cell_limit) {
        // "late" = the descendant sits one level below the target (finished only just before this level)
        const bool late = is_late(S, D, d, sfr);
        if (late) late_tmp.push_back(x); else cd.push_back(x);
        continue;
      }
      Pt.n_sparse++;
      if (gpu_cells) {
        Pt.cellcombos.push_back(CellCombo{x.loff, x.rowoff, LOFF[sfr], S.sn_rowptr[sfr] + R0, x.md, x.wd, x.ta, x.nt, x.p0, x.nq,
                                          x.ip0, (int32_t)ms, (int32_t)R0, (int32_t)(tile_end - R0), c0s, S.sn_level[sfr],
                                          is_late(S, D, d, sfr) ? 1 : 0});
        continue;
      }
      const int32_t* rd = S.sn_rows.data() + x.rowoff;
      const int32_t* lo = rs + R0;
      for (int32_t t = x.ta; t < x.ta + x.nt; ++t) {
        const int64_t R = (x.ip0 >= 0) ? R0 + x.ip0 + (t - x.ta) : (std::lower_bound(lo, rs + tile_end, rd[t]) - rs);
        for (int32_t q = x.p0; q < x.p0 + x.nq; ++q) {
          const int64_t j = rd[q] - c0s;
          if (R < j) continue;  // strict upper part of the diagonal block is never referenced
          cells.push_back(Cell{LOFF[sfr] + j * ms + R, x.loff + t, x.loff + q, x.md, x.wd, S.sn_level[sfr],
                               is_late(S, D, d, sfr) ? 1 : 0});
        }
      }
    }
    Pt.dmidv.push_back((int64_t)cd.size());
    cd.insert(cd.end(), late_tmp.begin(), late_tmp.end());
    late_tmp.clear();
    Pt.dend.push_back((int64_t)cd.size());
  }
}

// Every update combo becomes a dense descriptor (d_combos; uploaded part by part) or goes to the cell-wise path
int classify_combos(scilmm_symbolic* sym, Dev* D, PlanBuild& pb) {
  const Symbolic& S = *sym->S;
  const int64_t nc = (int64_t)S.combo_pair.size();
  const int64_t ntiles0 = (int64_t)S.tile_front.size();
  const double cell_limit = choose_cell_limit(S, D, pb);
  std::vector<int64_t>& dptr = pb.dptr;
  std::vector<int64_t>& dmid = pb.dmid;
  dptr.assign((size_t)ntiles0 + 1, 0);
  dmid.assign((size_t)ntiles0 + 1, 0);
  D->look_depth = D->tune.look_depth;  // measured at 100k: depth 1 81.4 ms, 2 77.6 ms, 3 78.4 ms
  std::vector<Cell>& cells = pb.cells;
  // The tiles are classified by a few host threads over contiguous tile ranges of about equal combo counts; the
  // per-range outputs are concatenated in tile order, so the plan does not depend on the thread count.
  // The cell lists are built on the device from the small combos (cellplan.hip.h); SCILMM_HOST_CELLS=1 keeps the
  // host enumeration (same lists up to the order of the contributions inside a group).
  const bool gpu_cells = pb.gpu_cells = !D->tune.host_cells && S.nnzL_stored < ((int64_t)1 << 38);
  std::vector<std::vector<CellCombo>>& cellparts = pb.cellparts;
  std::vector<uint8_t>& cd_cost = pb.cd_cost;
  int64_t n_dense_total = 0;
  {
    const unsigned nth = (unsigned)std::max<int64_t>(
        1, std::min<int64_t>((nc > 50000000 ? 3 : 1) * scilmm::host_threads(), ntiles0));  // static shares: finer = better balanced
    std::vector<int64_t> cut(nth + 1, ntiles0);
    cut[0] = 0;
    for (unsigned k = 1; k < nth; ++k) {
      const int64_t want = nc * (int64_t)k / nth;  // first tile whose combos start at or after this share
      cut[k] = std::lower_bound(S.combo_ptr.begin(), S.combo_ptr.begin() + ntiles0, want) - S.combo_ptr.begin();
      cut[k] = std::max(cut[k], cut[k - 1]);
    }
    std::vector<ClassifiedPart> parts(nth);
    std::vector<std::thread> pool;
    for (unsigned k = 1; k < nth; ++k) pool.emplace_back([&, k]() { classify_tile_range(S, D, cell_limit, gpu_cells, cut[k], cut[k + 1], parts[k]); });
    classify_tile_range(S, D, cell_limit, gpu_cells, cut[0], cut[1], parts[0]);
    for (auto& th : pool) th.join();
    size_t ncd = 0, ncell = 0;
    for (auto& Pt : parts) { ncd += Pt.cd.size(); ncell += Pt.cells.size(); }
    cells.reserve(ncell);
    // The dense-path descriptors (18 GB at the 1M config) are NOT concatenated on the host: every part goes straight
    // to its place in the device array, and the host keeps one byte per combo (its cost) for the work-item cuts.
    {
      void* pdc = nullptr;
      HIPCHK(hipMalloc(&pdc, sizeof(ComboDesc) * (ncd + 1)));
      D->allocs.push_back(pdc);
      D->d_combos = (ComboDesc*)pdc;
    }
    cd_cost.resize(ncd);
    std::vector<int64_t> dbases(nth + 1, 0);
    for (unsigned k = 0; k < nth; ++k) dbases[k + 1] = dbases[k] + (int64_t)parts[k].cd.size();
    {
      std::vector<std::thread> pool2;
      auto fill_cost = [&](unsigned k) {
        const std::vector<ComboDesc>& v = parts[k].cd;
        uint8_t* dst = cd_cost.data() + dbases[k];
        for (size_t c = 0; c < v.size(); ++c) dst[c] = (uint8_t)(1 + (v[c].wd + KC - 1) / KC);
      };
      for (unsigned k = 1; k < nth; ++k) pool2.emplace_back(fill_cost, k);
      fill_cost(0);
      for (auto& th : pool2) th.join();
    }
    for (unsigned k = 0; k < nth; ++k) {
      ClassifiedPart& Pt = parts[k];
      const int64_t dbase = dbases[k];
      for (int64_t g = cut[k]; g < cut[k + 1]; ++g) {
        dmid[g] = dbase + Pt.dmidv[(size_t)(g - cut[k])];
        dptr[g + 1] = dbase + Pt.dend[(size_t)(g - cut[k])];
      }
      if (!Pt.cd.empty())
        HIPCHK(hipMemcpy(D->d_combos + dbase, Pt.cd.data(), sizeof(ComboDesc) * Pt.cd.size(), hipMemcpyHostToDevice));
      cells.insert(cells.end(), Pt.cells.begin(), Pt.cells.end());
      D->n_sparse_combos += Pt.n_sparse;
      std::vector<ComboDesc>().swap(Pt.cd);
      std::vector<Cell>().swap(Pt.cells);
    }
    n_dense_total = (int64_t)ncd;
    for (unsigned k = 0; k < nth; ++k) cellparts.push_back(std::move(parts[k].cellcombos));
  }
  D->n_dense_combos = n_dense_total;
  D->n_cells = (int64_t)cells.size();
  return SCILMM_OK;
}

// The cell lists built on the host (SCILMM_HOST_CELLS=1): consumes pb.cells
int build_cells_host(scilmm_symbolic* sym, Dev* D, PlanBuild& pb, size_t* n_early, int64_t* ngroups) {
  const Symbolic& S = *sym->S;
  std::vector<Cell>& cells = pb.cells;
  size_t& split = *n_early;
  int64_t& ngroups_total = *ngroups;
  int st;
  // Cells are ordered by (late class, level, dst, st, sq): counting sort on (class, level), then every bucket is
  // sorted, cut into groups of equal target address (short groups first) and written to the upload arrays
  // independently on a few host threads (one global std::sort of 27 M cells cost 7 s of every first evaluation).
  const size_t NL = (size_t)std::max(S.nlevels, 1), nbk = 3 * NL;
  std::vector<size_t> bptr(nbk + 1, 0);
  for (const Cell& c : cells) bptr[(size_t)c.late * NL + c.level + 1]++;
  for (size_t k = 0; k < nbk; ++k) bptr[k + 1] += bptr[k];
  split = bptr[NL];
  {
    std::vector<Cell> sorted(cells.size());
    std::vector<size_t> fill(bptr.begin(), bptr.end() - 1);
    for (const Cell& c : cells) sorted[fill[(size_t)c.late * NL + c.level]++] = c;
    cells.swap(sorted);
  }
  const unsigned nth = (unsigned)std::max(1, std::min(16, scilmm::host_threads()));
  auto parallel_buckets = [&](const std::function<void(size_t)>& fn) {
    std::atomic<size_t> next{0};
    auto worker = [&]() {
      for (;;) {
        const size_t k = next.fetch_add(1);
        if (k >= nbk) break;
        fn(k);
      }
    };
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < nth; ++t) pool.emplace_back(worker);
    worker();
    for (auto& th : pool) th.join();
  };
  const int64_t long_limit = 16;
  std::vector<int64_t> g_short(nbk, 0), g_long(nbk, 0), e_short(nbk, 0);
  parallel_buckets([&](size_t k) {
    std::sort(cells.begin() + bptr[k], cells.begin() + bptr[k + 1], [](const Cell& a, const Cell& b) {
      if (a.dst != b.dst) return a.dst < b.dst;
      if (a.st != b.st) return a.st < b.st;
      return a.sq < b.sq;
    });
    for (size_t i = bptr[k]; i < bptr[k + 1];) {
      size_t j = i + 1;
      while (j < bptr[k + 1] && cells[j].dst == cells[i].dst) ++j;
      if ((int64_t)(j - i) <= long_limit) { g_short[k]++; e_short[k] += (int64_t)(j - i); } else g_long[k]++;
      i = j;
    }
  });
  for (int which = 0; which < 3; ++which) {
    Dev::CellSet& CS = D->cellset[which];
    CS.level_ptr.assign(S.nlevels + 1, 0);
    CS.level_short.assign(NL, 0);
    std::vector<int64_t> gbase(NL + 1, 0), ebase(NL + 1, 0);
    for (size_t l = 0; l < NL; ++l) {
      const size_t k = (size_t)which * NL + l;
      gbase[l + 1] = gbase[l] + g_short[k] + g_long[k];
      ebase[l + 1] = ebase[l] + (int64_t)(bptr[k + 1] - bptr[k]);
      if ((int32_t)l < S.nlevels) {
        CS.level_ptr[l + 1] = gbase[l + 1];
        CS.level_short[l] = g_short[k];
      }
    }
    const int64_t ng = gbase[NL], ne = ebase[NL];
    std::vector<int64_t> udst((size_t)ng), grp((size_t)ng + 1), st_((size_t)ne), sq_((size_t)ne);
    std::vector<int32_t> md_((size_t)ne), wd_((size_t)ne);
    grp[(size_t)ng] = ne;
    parallel_buckets([&](size_t k) {
      if (k / NL != (size_t)which) return;
      const size_t l = k - (size_t)which * NL;
      // short groups first, then the long ones; both in address order
      int64_t gs = gbase[l], gl = gbase[l] + g_short[k];
      int64_t es = ebase[l], el = ebase[l] + e_short[k];
      for (size_t i = bptr[k]; i < bptr[k + 1];) {
        size_t j = i + 1;
        while (j < bptr[k + 1] && cells[j].dst == cells[i].dst) ++j;
        const bool shortg = (int64_t)(j - i) <= long_limit;
        int64_t& gi = shortg ? gs : gl;
        int64_t& ei = shortg ? es : el;
        udst[(size_t)gi] = cells[i].dst;
        grp[(size_t)gi] = ei;
        ++gi;
        for (size_t c = i; c < j; ++c, ++ei) {
          st_[(size_t)ei] = cells[c].st; sq_[(size_t)ei] = cells[c].sq; md_[(size_t)ei] = cells[c].md; wd_[(size_t)ei] = cells[c].wd;
        }
        i = j;
      }
    });
    ngroups_total += ng;
    if (udst.empty()) udst.push_back(0);
    if (st_.empty()) { st_.push_back(0); sq_.push_back(0); md_.push_back(0); wd_.push_back(0); }
    if ((st = upload(sym, D, udst, &CS.dst)) != SCILMM_OK) return st;
    if ((st = upload(sym, D, grp, &CS.grp)) != SCILMM_OK) return st;
    if ((st = upload(sym, D, st_, &CS.srct)) != SCILMM_OK) return st;
    if ((st = upload(sym, D, sq_, &CS.srcq)) != SCILMM_OK) return st;
    if ((st = upload(sym, D, md_, &CS.md)) != SCILMM_OK) return st;
    if ((st = upload(sym, D, wd_, &CS.wd)) != SCILMM_OK) return st;
  }
  return SCILMM_OK;
}

// The cell lists of k_sparse_cells (cellset[]), on the device from the small combos or on the host from the cells
int build_cells(scilmm_symbolic* sym, Dev* D, PlanBuild& pb) {
  const Symbolic& S = *sym->S;
  std::vector<Cell>& cells = pb.cells;
  std::vector<std::vector<CellCombo>>& cellparts = pb.cellparts;
  int st;
  size_t split = 0;
  int64_t ngroups_total = 0;
  if (pb.gpu_cells) {
    int64_t potential = 0;
    std::vector<const std::vector<CellCombo>*> ccparts;
    for (auto& pv : cellparts) {
      ccparts.push_back(&pv);
      for (const CellCombo& q : pv) potential += (int64_t)q.nt * q.nq;
    }
    if (potential >= ((int64_t)1 << 31)) {
      sym->err = "cell plan: more than 2^31 cells (raise SCILMM_CELL_LIMIT granularity or set SCILMM_HOST_CELLS=1)";
      return SCILMM_ERR_ARG;
    }
    int64_t n_early_groups = 0;
    if ((st = build_cells_device(sym, D, ccparts, std::max(S.nlevels, 1), &ngroups_total, &n_early_groups)) != SCILMM_OK) return st;
    split = (size_t)n_early_groups;
    std::vector<std::vector<CellCombo>>().swap(cellparts);
  } else {
    if ((st = build_cells_host(sym, D, pb, &split, &ngroups_total)) != SCILMM_OK) return st;
  }
  {
    if (pb.verbose)
      fprintf(stderr, "[scilmm plan] dense combos %lld, cell-path combos %lld, cells %lld (early %lld) in %lld target groups\n",
              (long long)D->n_dense_combos, (long long)D->n_sparse_combos, (long long)D->n_cells, (long long)split,
              (long long)ngroups_total);
    std::vector<Cell>().swap(cells);
  }
  return SCILMM_OK;
}

// cut_work_items: the lists under construction (uploaded at its end), the cut parameters and the block pattern of the
// dense tail.  The methods are the parts of the cut in the order cut_work_items calls them.
struct WorkCut {
  const Symbolic& S;
  Dev* const D;
  const PlanBuild& pb;
  const std::vector<int64_t>&dptr, &dmid;
  std::vector<int32_t> pslot, pnseg, pslot_e, pnseg_e, red_tiles, red_tiles_e;
  std::vector<UpdWork> work, work_early;
  std::vector<DenseWork> dwork_e, dwork_l;
  int64_t max_slots = 0;
  const bool lookahead = !D->tune.no_lookahead;
  const int32_t depth = D->look_depth;
  const bool allow_split = !D->tune.no_splitk;
  // ... but an item never exceeds max_item units (~0.5 ms): the main stream's kernels start in the slots that
  // retiring update items free, so long items starve the per-level chain (300k probe: 2.3 ms per trsm launch)
  const int64_t target_items = D->tune.target_items, min_item = D->tune.min_item, max_item = std::max<int64_t>(min_item, D->tune.max_item);
  const int64_t dense_fill = D->tune.dense_fill;  // workgroups per round the dense item counts are fitted to (0: no fitting)
  // k_dense_b items per launch (target): long tails want launches of several rounds of workgroups (300k: 384 / 512 / 768 /
  // 1024 / 2048 / 3072 = 1373 / 1369 / 1365 / 1357 / 1384 / 1407 ms, 1M: 1024 vs 2048 = 27.0 vs 27.35 s), the short chain of the
  // 100k config short ones (see dense_on in choose_tail_paths)
  const int32_t tail_w = tail_width(S);
  const int64_t dense_items = std::max<int64_t>(64, D->tune.dense_items.value_or(tail_w < 24576 ? 128 : tail_w < 32768 ? 512 : 1024));
  std::vector<std::vector<int32_t>> tail_src;
  std::vector<int32_t> tail_col_front;  // label - first tail column -> relative tail front
  const bool dist = distributed_tail(D, S);
  const int32_t Wg = D->dist_Wg;
  std::vector<std::vector<uint8_t>> own_pair_on;  // [own tail front (relative)] -> mask, dist mode only
  int64_t dense_pairs_all = 0, dense_pairs_kept = 0, dense_tiles_all = 0, dense_tiles_kept = 0;
  int64_t dense_prod_all = 0, dense_prod_kept = 0, dense_items_empty = 0;  // (tile pair, descendant) products of the items; items trimmed to nothing

  WorkCut(const Symbolic& S_, Dev* D_, const PlanBuild& pb_) : S(S_), D(D_), pb(pb_), dptr(pb_.dptr), dmid(pb_.dmid) {
    const int64_t ntiles = (int64_t)S.tile_front.size();
    pslot.assign((size_t)std::max<int64_t>(ntiles, 1), 0);
    pnseg.assign(pslot.size(), 0);
    pslot_e.assign(pslot.size(), 0);
    pnseg_e.assign(pslot.size(), 0);
    D->red_ptr_e.assign(S.nlevels + 1, 0);
    D->dwork_e_ptr.assign(S.nlevels + 1, 0);
    D->dwork_l_ptr.assign(S.nlevels + 1, 0);
    D->dwork_l_mid.assign((size_t)std::max(S.nlevels, 1), 0);
    D->work_ptr.assign(S.nlevels + 1, 0);
    D->early_ptr.assign(S.nlevels + 1, 0);
    D->red_ptr.assign(S.nlevels + 1, 0);
    // dense tail, block pattern: tail_src[j] = the tail fronts (relative index, ascending) whose TRUE row lists reach
    // the columns of tail front j -- the others hold only padding there and are left out of j's dense items
    if (D->dense_on && !S.tail_blk_ptr.empty()) {
      const int32_t nT = S.nsuper - S.dense_first;
      tail_src.resize((size_t)nT);
      for (int32_t d = 0; d < nT; ++d)
        for (int64_t e = S.tail_blk_ptr[d]; e < S.tail_blk_ptr[d + 1]; ++e) tail_src[(size_t)S.tail_blk[e]].push_back(d);
    }
    if (!tail_src.empty()) {
      const int32_t c0t = S.sn_start[S.dense_first];
      tail_col_front.resize((size_t)(S.n - c0t));
      for (int32_t f = S.dense_first; f < S.nsuper; ++f)
        for (int32_t c = S.sn_start[f]; c < S.sn_start[f + 1]; ++c) tail_col_front[(size_t)(c - c0t)] = f - S.dense_first;
    }
    // distributed tail: the far part of an own target's update arrives as one BATCH per source group (see the level
    // loop of run_factorize); the per-target tile-pair masks are kept for the batch items built after this loop
    if (dist) own_pair_on.resize((size_t)(S.nsuper - S.dense_first));
  }

  // Cost model: a combo costs one fixed unit plus one unit per K-chunk it streams.  Each launch (the early
  // and the late part of a level) is cut into about 4 work items per CU of equal cost, so that one launch
  // fills the chip once with balanced items (late levels of a dense chain: few tiles, long combo lists).
  int64_t combo_cost(int64_t c) const { return pb.cd_cost[(size_t)c]; }
  // cut [cb,ce) into segments; returns the number of items appended to `out` (slot = 0 placeholder)
  int64_t cut(int32_t g, int64_t cb, int64_t ce, int64_t per_item, std::vector<UpdWork>& out) const {
    if (ce <= cb) return 0;
    int64_t tcost = 0;
    for (int64_t c = cb; c < ce; ++c) tcost += combo_cost(c);
    const int64_t nseg = std::min<int64_t>(64, std::max<int64_t>(1, (tcost + per_item / 2) / per_item));
    const int64_t seg_cost = (tcost + nseg - 1) / nseg;
    const size_t first = out.size();
    int64_t a = cb, acc = 0;
    for (int64_t c = cb; c < ce; ++c) {
      acc += combo_cost(c);
      if (nseg > 1 && acc >= seg_cost && c + 1 < ce) {
        out.push_back(UpdWork{g, 0, a, c + 1});
        a = c + 1;
        acc = 0;
      }
    }
    out.push_back(UpdWork{g, 0, a, ce});
    return (int64_t)(out.size() - first);
  }
  // runs of ACTIVE descendants (those whose true structure reaches target jj) inside [lo, hi)
  int64_t active_runs(int32_t jj, int32_t lo, int32_t hi, std::vector<std::pair<int32_t, int32_t>>& runs) const {
    runs.clear();
    if (hi <= lo) return 0;
    if (tail_src.empty()) {
      runs.push_back({lo, hi});
    } else {
      const std::vector<int32_t>& src = tail_src[(size_t)jj];
      auto it = std::lower_bound(src.begin(), src.end(), lo);
      for (; it != src.end() && *it < hi; ++it) {
        if (!runs.empty() && runs.back().second == *it) runs.back().second = *it + 1;
        else runs.push_back({*it, *it + 1});
      }
      if (runs.size() > 16) runs = {{runs.front().first, runs.back().second}};  // too fragmented: take the hull
    }
    int64_t total = 0;
    for (auto& r : runs) total += r.second - r.first;
    return total;
  }

  // The dense-tail items of level l: K segments, active tile pairs, cost
  struct DenseLevel {
    int32_t dj = -1;          // the level's own tail front, or -1
    int32_t nseg_older = -1;  // look-ahead split: K segments of the level's late dense items that do NOT read the newest source
    std::vector<std::pair<int32_t, int32_t>> segs_e, segs_l;  // descendant ranges of the level's dense items
    std::vector<uint8_t> pair_on;                             // per tile pair of the dense target: does it get items
    int64_t cost_e = 0, cost_l = 0;
  };
  DenseLevel plan_dense_level(int32_t l) {
    // dense tail: the level's (single) front j = dense_first + jj receives every earlier tail front; the last
    // look_depth of them are "late", the others "early" -- implicit items, one per (pair of tiles, K segment).
    // Distributed tail: late = the sources of the target's own group and of the group before it (they arrive while
    // the chain advances); everything older is applied by the per-group batches.
    int64_t total_e = 0, total_l = 0;  // cost units of the level's dense items
    int32_t dj = -1, dcnt_e = 0, dcnt_l = 0;
    std::vector<std::pair<int32_t, int32_t>> segs_e, segs_l;  // descendant ranges of the level's dense items
    std::vector<uint8_t> pair_on;                             // per tile pair of the dense target: does it get items
    const int64_t dunit = 1 + (NB + KC - 1) / KC;  // cost units of one tail descendant on one tile
    int32_t nseg_older = -1;  // look-ahead split: K segments of the level's late dense items that do NOT read the newest source
    int32_t dfr = -1;  // the tail fronts lie on a chain: at most one of them per level
    if (D->dense_on)
      for (int32_t q = S.level_ptr[l]; q < S.level_ptr[l + 1]; ++q)
        if (S.level_fronts[q] >= S.dense_first) dfr = S.level_fronts[q];
    if (dfr >= 0) {
      const int32_t fr = dfr;
      if (D->keep_front[fr]) {
        dj = fr;
        const int32_t jj = fr - S.dense_first;
        if (dist) {
          const int32_t lo = std::max(0, (jj / Wg - 1) * Wg);
          dcnt_l = jj - lo;
          dcnt_e = 0;  // (the batches)
        } else {
          dcnt_l = lookahead ? std::min<int32_t>(depth, jj) : jj;
          dcnt_e = jj - dcnt_l;
        }
        const int64_t ntl = S.tile_base[fr + 1] - S.tile_base[fr];
        // K segments = contiguous ranges of ACTIVE descendants (the same for every tile of the front), about
        // dense_items items per launch: every item writes two 128 KB slabs that k_reduce reads back, so few long
        // items beat many short ones as long as the launch still fills the chip a few times over
        const int64_t npairs = (ntl + 1) / 2;
        // rows of the target that NO active descendant reaches receive nothing but padding: their tile pairs get no
        // items (below the dense region the fronts of one side branch do not reach the columns of the others, nor
        // the part of the region sorted to its start)
        pair_on.assign((size_t)npairs, 1);
        if (!tail_src.empty() && jj > 0) {
          const std::vector<int32_t>& src = tail_src[(size_t)jj];
          const auto a_end = std::lower_bound(src.begin(), src.end(), jj);
          const int32_t c0t = S.sn_start[S.dense_first], c0j = S.sn_start[fr];
          for (int64_t pq = 0; pq < npairs; ++pq) {
            const int64_t lo = (int64_t)c0j + 2 * TM * pq, hi = std::min<int64_t>(lo + 2 * TM, S.n);
            const int32_t f_lo = tail_col_front[(size_t)(lo - c0t)], f_hi = tail_col_front[(size_t)(hi - 1 - c0t)];
            bool need = f_lo <= jj;  // the target's own columns
            for (int32_t f = std::max(f_lo, jj + 1); f <= f_hi && !need; ++f) {
              const std::vector<int32_t>& sf = tail_src[(size_t)f];
              auto x = src.begin();
              auto y = sf.begin();
              while (x != a_end && y != sf.end()) {
                if (*x < *y) ++x;
                else if (*y < *x) ++y;
                else { need = true; break; }
              }
            }
            pair_on[(size_t)pq] = need ? 1 : 0;
          }
        }
        int64_t np_on = 0;
        for (uint8_t v : pair_on) np_on += v;
        // K segments: about dense_items items per launch, and -- when the plan may choose (dense_fill) -- a count that
        // fills the last round of workgroups: the items of a launch last about equally long, so I items on 256 CUs take
        // ceil(I / 256) rounds whatever I is (1M config: 1100 items = 4.3 rounds paid as 5)
        const int64_t want = std::max<int64_t>(1, (dense_items + std::max<int64_t>(1, np_on) / 2) / std::max<int64_t>(1, np_on));
        std::vector<std::pair<int32_t, int32_t>> runs;
        auto cut_runs = [&](int64_t total, int64_t nseg, std::vector<std::pair<int32_t, int32_t>>* out) -> int64_t {
          int64_t cnt = 0;
          for (auto& r : runs) {
            const int64_t len = r.second - r.first;
            const int64_t ns_r = std::max<int64_t>(1, std::min<int64_t>(len, (nseg * len + total / 2) / total));
            for (int64_t q = 0; q < ns_r; ++q) {
              const int32_t a = r.first + (int32_t)(len * q / ns_r), b = r.first + (int32_t)(len * (q + 1) / ns_r);
              if (b > a) {
                ++cnt;
                if (out) out->push_back({a, b});
              }
            }
          }
          return cnt;
        };
        bool taper = false;
        auto build = [&](int32_t lo, int32_t hi, std::vector<std::pair<int32_t, int32_t>>& out) -> int64_t {
          out.clear();
          const int64_t total = active_runs(jj, lo, hi, runs);
          if (total == 0) return 0;
          const int64_t cap = std::min<int64_t>(64, total);
          int64_t nseg = std::min(cap, want);
          if (dense_fill && np_on > 0) {
            double best = -1.0;
            for (int64_t ns = std::max<int64_t>(1, want * 2 / 3); ns <= std::min(cap, want * 3 / 2 + 1); ++ns) {
              const int64_t items = np_on * cut_runs(total, ns, nullptr);
              const int64_t rounds = (items + dense_fill - 1) / dense_fill;
              const double score = (double)items / (double)(rounds * dense_fill) - 0.02 * std::fabs((double)(ns - want)) / (double)want;
              if (score > best) { best = score; nseg = ns; }
            }
          }
          cut_runs(total, nseg, &out);
          // TAPER (long launches only): the items of a launch start in list order, K-segment major, and last about as long as
          // their segment is deep -- with equal segments the chip idles at the end of a launch while the last round of
          // workgroups finishes (measured ~8 % of a serialised 9.8 ms launch at 1M).  The second-to-last segment is therefore
          // cut in two and the last one in four: the launch ends on quarter-length items (a few more partial slabs per tile).
          if (taper && out.size() >= 3) {
            std::vector<std::pair<int32_t, int32_t>> tp(out.begin(), out.end() - 2);
            auto split = [&](std::pair<int32_t, int32_t> sgm, int parts) {
              const int32_t len = sgm.second - sgm.first;
              for (int q = 0; q < parts; ++q) {
                const int32_t a = sgm.first + (int32_t)((int64_t)len * q / parts), b = sgm.first + (int32_t)((int64_t)len * (q + 1) / parts);
                if (b > a) tp.push_back({a, b});
              }
            };
            split(out[out.size() - 2], 2);
            split(out[out.size() - 1], 4);
            out.swap(tp);
          }
          return total;
        };
        int64_t act_l;
        if (dist && dcnt_l >= 2 && !D->tune.dist_nosplit) {
          // look-ahead split (multi-GPU critical path): the NEWEST source, panel jj - 1, gets K segments of its own, listed
          // last -- the level loop launches the segments of the older sources before it waits for that panel's broadcast
          std::vector<std::pair<int32_t, int32_t>> newest;
          act_l = build(jj - dcnt_l, jj - 1, segs_l);
          nseg_older = (int32_t)segs_l.size();
          act_l += build(jj - 1, jj, newest);
          segs_l.insert(segs_l.end(), newest.begin(), newest.end());
          if (newest.empty()) nseg_older = -1;  // (the newest source does not reach this target: nothing to wait for separately)
        } else {
          act_l = build(jj - dcnt_l, jj, segs_l);
        }
        // (the early launch of a long tail: 1024-item launches, several rounds of workgroups)
        taper = D->tune.dense_taper.value_or(dense_items >= 1024);
        const int64_t act_e = dist ? 0 : build(0, dcnt_e, segs_e);
        taper = false;
        dense_pairs_all += dist ? dcnt_l : jj;
        dense_pairs_kept += act_e + act_l;
        for (uint8_t v : pair_on) { dense_tiles_all += 1; dense_tiles_kept += v; }
        if (dist) own_pair_on[(size_t)jj] = pair_on;
        total_e += ntl * dunit * act_e;
        total_l += ntl * dunit * act_l;
      }
    }
    return DenseLevel{dj, nseg_older, std::move(segs_e), std::move(segs_l), std::move(pair_on), total_e, total_l};
  }

  // Explicit items and partial slabs of level l (and the slabs of its dense items: dbase_e / dbase_l, per tile of front dj
  // the first dense slab, -1 = subtract directly); returns the slabs the level needs
  int64_t cut_explicit_items(int32_t l, const DenseLevel& dl, int64_t total_e, int64_t total_l, std::vector<int32_t>& dbase_e,
                             std::vector<int32_t>& dbase_l) {
    const int32_t dj = dl.dj;
    const std::vector<uint8_t>& pair_on = dl.pair_on;
    const std::vector<std::pair<int32_t, int32_t>>&segs_e = dl.segs_e, &segs_l = dl.segs_l;
    const int64_t big = (int64_t)1 << 60;
    // (at most ~8192 items per launch: the slabs of a level must stay a few GB on the largest patterns)
    const int64_t cap_e = std::max<int64_t>(max_item, total_e / 8192), cap_l = std::max<int64_t>(max_item, total_l / 8192);
    const int64_t per_e = allow_split ? std::min(cap_e, std::max<int64_t>(min_item, (total_e + target_items - 1) / target_items)) : big;
    const int64_t per_l = allow_split ? std::min(cap_l, std::max<int64_t>(min_item, (total_l + target_items - 1) / target_items)) : big;
    int64_t slots = 0;
    const int64_t nde = (int64_t)segs_e.size(), ndl = (int64_t)segs_l.size();
    if (dj >= 0) {
      dbase_e.assign((size_t)(S.tile_base[dj + 1] - S.tile_base[dj]), -1);
      dbase_l.assign(dbase_e.size(), -1);
    }
    std::vector<int32_t> order(S.level_tiles.begin() + S.level_tile_ptr[l], S.level_tiles.begin() + S.level_tile_ptr[l + 1]);
    // heaviest tiles (most combos) first: the long items of a launch start early
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
      return (S.combo_ptr[a + 1] - S.combo_ptr[a]) > (S.combo_ptr[b + 1] - S.combo_ptr[b]);
    });
    for (size_t oi = 0; oi < order.size(); ++oi) {
      const int32_t g = order[oi];
      const size_t fe = work_early.size(), fl = work.size();
      const int64_t ne = cut(g, dptr[g], dmid[g], per_e, work_early);
      const int64_t nl = cut(g, dmid[g], dptr[g + 1], per_l, work);
      // a single dense item of a launch subtracts straight into the panel (the early and the late launch of a
      // level never overlap in time); two or more go through partial slabs
      // (the implicit dense-tail items of the tile count like explicit ones: dte / dtl of them)
      const bool dtile = dj >= 0 && S.tile_front[g] == dj && pair_on[(size_t)((g - S.tile_base[dj]) / 2)];
      const int64_t dte = dtile ? nde : 0, dtl = dtile ? ndl : 0;
      const int64_t pe = (ne + dte) >= 2 ? ne : 0, pl = (nl + dtl) >= 2 ? nl : 0;
      const int64_t pde = (ne + dte) >= 2 ? dte : 0, pdl = (nl + dtl) >= 2 ? dtl : 0;
      if (ne == 1 && pe == 0) work_early[fe].slot = -1;
      if (nl == 1 && pl == 0) work[fl].slot = -1;
      if (pe + pde > 0) {
        pslot_e[g] = (int32_t)slots;
        pnseg_e[g] = (int32_t)(pe + pde);
        red_tiles_e.push_back(g);
        for (int64_t k = 0; k < pe; ++k) work_early[fe + k].slot = (int32_t)(slots + k);
        if (pde > 0) dbase_e[(size_t)(g - S.tile_base[dj])] = (int32_t)(slots + pe);
        slots += pe + pde;
      }
      if (pl + pdl > 0) {
        pslot[g] = (int32_t)slots;
        pnseg[g] = (int32_t)(pl + pdl);
        red_tiles.push_back(g);
        for (int64_t k = 0; k < pl; ++k) work[fl + k].slot = (int32_t)(slots + k);
        if (pdl > 0) dbase_l[(size_t)(g - S.tile_base[dj])] = (int32_t)(slots + pl);
        slots += pl + pdl;
      }
    }
    // Launch order = K-segment major, tile minor: the workgroups resident at any moment then work on the SAME few
    // descendant panels (their target-column rows -- the B operand -- are shared by every tile of the level), so that
    // operand comes out of the L2s / the infinity cache instead of HBM once per tile.  (Slots were assigned above:
    // the partial slabs of a tile stay contiguous whatever the launch order.)
    {
      auto seg_major = [&](std::vector<UpdWork>& v, size_t first) {
        if (v.size() - first < 2) return;
        std::vector<std::pair<int32_t, int32_t>> key(v.size() - first);  // (segment index within its tile, position)
        int32_t seg = 0;
        for (size_t k = first; k < v.size(); ++k) {
          seg = (k > first && v[k].tile == v[k - 1].tile) ? seg + 1 : 0;
          key[k - first] = {seg, (int32_t)(k - first)};
        }
        std::stable_sort(key.begin(), key.end(), [](const std::pair<int32_t, int32_t>& a, const std::pair<int32_t, int32_t>& b) { return a.first < b.first; });
        std::vector<UpdWork> tmp(v.begin() + first, v.end());
        for (size_t k = 0; k < key.size(); ++k) v[first + k] = tmp[(size_t)key[k].second];
      };
      seg_major(work_early, (size_t)D->early_ptr[l]);
      seg_major(work, (size_t)D->work_ptr[l]);
    }
    return slots;
  }

  void emit_dense_items(const DenseLevel& dl, const std::vector<int32_t>& dbase_e, const std::vector<int32_t>& dbase_l) {
    const int32_t dj = dl.dj;
    const std::vector<uint8_t>& pair_on = dl.pair_on;
    const std::vector<std::pair<int32_t, int32_t>>&segs_e = dl.segs_e, &segs_l = dl.segs_l;
    if (dj >= 0) {
      // K-segment major, tile-pair minor (same reason as above); a pair = two vertically adjacent tiles of the front
      const int32_t ntl = (int32_t)(S.tile_base[dj + 1] - S.tile_base[dj]);
      // PER-PAIR REACH: the K segments are the same for every tile pair of the target, but a descendant whose true rows do not
      // reach a pair's 256 rows holds only padding (zeros) there.  The pair's rows lie in the tail fronts f_lo..f_hi; descendant d
      // reaches the pair if f_lo <= jj (the target's own columns: every active descendant has rows there) or if its row blocks
      // (tail_blk) hold one of the fronts max(f_lo, jj + 1)..f_hi.  Every item's K range is trimmed to its first and last
      // reaching descendant (zero products dropped from both ends: the sums keep their values and their order); an item that
      // no descendant of its segment reaches is still emitted, with k0 == k1 -- slab numbering, the fitted item counts and the
      // taper stay as they are, and the kernels store zeros to such an item's slabs.
      const int32_t jj = dj - S.dense_first;
      const bool reach_known = !tail_src.empty() && jj > 0;
      const int32_t c0t = S.sn_start[S.dense_first], c0j = S.sn_start[dj];
      auto trim = [&](int32_t q, int32_t& k0, int32_t& k1) {
        if (!reach_known || k1 <= k0) return;
        const int64_t lo = (int64_t)c0j + (int64_t)TM * q, hi = std::min<int64_t>(lo + 2 * TM, S.n);
        const int32_t f_lo = tail_col_front[(size_t)(lo - c0t)], f_hi = tail_col_front[(size_t)(hi - 1 - c0t)];
        if (f_lo <= jj) return;
        int32_t first = k1, last = k0 - 1;
        for (int32_t f = f_lo; f <= f_hi; ++f) {
          const std::vector<int32_t>& sf = tail_src[(size_t)f];
          const auto a = std::lower_bound(sf.begin(), sf.end(), k0), b = std::lower_bound(sf.begin(), sf.end(), k1);
          if (a != b) {
            first = std::min(first, *a);
            last = std::max(last, *(b - 1));
          }
        }
        if (first > last) k1 = k0;
        else { k0 = first; k1 = last + 1; }
      };
      auto emit = [&](std::vector<DenseWork>& out, const std::vector<std::pair<int32_t, int32_t>>& segs, const std::vector<int32_t>& base) {
        for (size_t sg = 0; sg < segs.size(); ++sg) {
          for (int32_t q = 0; q < ntl; q += 2) {
            if (!pair_on[(size_t)(q / 2)]) continue;
            int32_t k0 = segs[sg].first, k1 = segs[sg].second;
            dense_prod_all += k1 - k0;
            trim(q, k0, k1);
            dense_prod_kept += k1 - k0;
            dense_items_empty += k1 <= k0 ? 1 : 0;
            const int32_t nt2 = std::min<int32_t>(2, ntl - q);
            DenseWork wk{dj, q, nt2, k0, k1, base[(size_t)q] < 0 ? -1 : base[(size_t)q] + (int32_t)sg,
                         (nt2 == 2 && base[(size_t)q + 1] >= 0) ? base[(size_t)q + 1] + (int32_t)sg : -1, 0};
            out.push_back(wk);
          }
        }
      };
      emit(dwork_e, segs_e, dbase_e);
      emit(dwork_l, segs_l, dbase_l);
    }
  }

  void cut_level(int32_t l) {
    int64_t total_e = 0, total_l = 0;
    for (int64_t i = S.level_tile_ptr[l]; i < S.level_tile_ptr[l + 1]; ++i) {
      const int32_t g = S.level_tiles[i];
      for (int64_t c = dptr[g]; c < dmid[g]; ++c) total_e += combo_cost(c);
      for (int64_t c = dmid[g]; c < dptr[g + 1]; ++c) total_l += combo_cost(c);
    }
    const DenseLevel dl = plan_dense_level(l);
    total_e += dl.cost_e;
    total_l += dl.cost_l;
    std::vector<int32_t> dbase_e, dbase_l;
    const int64_t slots = cut_explicit_items(l, dl, total_e, total_l, dbase_e, dbase_l);
    emit_dense_items(dl, dbase_e, dbase_l);
    const int32_t dj = dl.dj, nseg_older = dl.nseg_older;
    const std::vector<uint8_t>& pair_on = dl.pair_on;
    D->dwork_e_ptr[l + 1] = (int64_t)dwork_e.size();
    D->dwork_l_ptr[l + 1] = (int64_t)dwork_l.size();
    {
      // (items are K-segment major: the first nseg_older segments x the active tile pairs are the older sources' items)
      int64_t np_on_l = 0;
      if (dj >= 0 && nseg_older >= 0)
        for (uint8_t v : pair_on) np_on_l += v;
      D->dwork_l_mid[(size_t)l] = (dj >= 0 && nseg_older >= 0) ? D->dwork_l_ptr[l] + (int64_t)nseg_older * np_on_l : D->dwork_l_ptr[l + 1];
    }
    max_slots = std::max(max_slots, slots);
    D->lev_cost_e.push_back(total_e);
    D->lev_cost_l.push_back(total_l);
    D->work_ptr[l + 1] = (int64_t)work.size();
    D->early_ptr[l + 1] = (int64_t)work_early.size();
    D->red_ptr[l + 1] = (int64_t)red_tiles.size();
    D->red_ptr_e[l + 1] = (int64_t)red_tiles_e.size();
  }

  int plan_dist_batches(scilmm_symbolic* sym) {
    int st;
    // ---- batches of the distributed tail: batch g = the contribution of source group g (tail fronts
    //      [g Wg, (g+1) Wg)) to every own target that lies at least two groups later -- one item per (target, tile
    //      pair), K = the hull of the group's active sources, subtracted straight from the panel (batches run one
    //      after the other on one stream, and a target's late update waits for its last batch)
    const int32_t nT = S.nsuper - S.dense_first;
    const int32_t ngroups = (nT + Wg - 1) / Wg;
    std::vector<DenseWork> dwork_b;
    D->dbatch_ptr.assign((size_t)ngroups + 1, 0);
    std::vector<std::pair<int32_t, int32_t>> runs;
    for (int32_t g = 0; g < ngroups; ++g) {
      for (int32_t jj = (g + 2) * Wg; jj < nT; ++jj) {
        const int32_t fr = S.dense_first + jj;
        if (!D->keep_front[fr]) continue;
        if (active_runs(jj, g * Wg, std::min((g + 1) * Wg, nT), runs) == 0) continue;
        const int32_t k0 = runs.front().first, k1 = runs.back().second;
        const int32_t ntl = (int32_t)(S.tile_base[fr + 1] - S.tile_base[fr]);
        const std::vector<uint8_t>& pon = own_pair_on[(size_t)jj];
        for (int32_t q = 0; q < ntl; q += 2) {
          if (!pon.empty() && !pon[(size_t)(q / 2)]) continue;
          dwork_b.push_back(DenseWork{fr, q, std::min<int32_t>(2, ntl - q), k0, k1, -1, -1, 0});
        }
      }
      D->dbatch_ptr[(size_t)g + 1] = (int64_t)dwork_b.size();
    }
    if (dwork_b.empty()) dwork_b.push_back(DenseWork{});
    if ((st = upload(sym, D, dwork_b, &D->d_dwork_b)) != SCILMM_OK) return st;
    if (pb.verbose)
      fprintf(stderr, "[scilmm plan] rank %d: %lld batch items in %d source groups of %d tail panels\n", D->rank,
              (long long)D->dbatch_ptr[(size_t)ngroups], ngroups, Wg);
    return SCILMM_OK;
  }

  // one line per launch class: explicit items, and the partial slabs per tile that k_reduce (early) and k_potrf / k_trsm (late) fold
  void report_slabs(const char* cls, int64_t items, const std::vector<int32_t>& tiles, const std::vector<int32_t>& nseg) const {
    int64_t slabs = 0, odd = 0;
    int32_t lo = 0, hi = 0;
    for (int32_t g : tiles) {
      const int32_t c = nseg[(size_t)g];
      slabs += c;
      odd += c & 1;
      lo = lo == 0 ? c : std::min(lo, c);
      hi = std::max(hi, c);
    }
    fprintf(stderr, "[scilmm plan] %s: %lld explicit items, %lld partial slabs on %zu tiles, %d .. %d per tile, %lld tiles with an odd count, %lld with an even one\n",
            cls, (long long)items, (long long)slabs, tiles.size(), lo, hi, (long long)odd, (long long)((int64_t)tiles.size() - odd));
  }

  int upload_items(scilmm_symbolic* sym) {
    int st;
    if (pb.verbose) {
      report_slabs("early launches", (int64_t)work_early.size(), red_tiles_e, pnseg_e);
      report_slabs("late launches", (int64_t)work.size(), red_tiles, pnseg);
      fprintf(stderr, "[scilmm plan] split-K %s, panel solve %s, %d side streams\n", allow_split ? "on" : "off",
              !D->use_mfma ? "k_trsm<false>" : D->trsm_lite ? "k_trsm_lite" : "k_trsm<true>", D->nside);
    }
    {
      if (dwork_e.empty()) dwork_e.push_back(DenseWork{});
      if (dwork_l.empty()) dwork_l.push_back(DenseWork{});
      if ((st = upload(sym, D, dwork_e, &D->d_dwork_e)) != SCILMM_OK) return st;
      if ((st = upload(sym, D, dwork_l, &D->d_dwork_l)) != SCILMM_OK) return st;
      if (pb.verbose && dense_pairs_all > 0)
        fprintf(stderr, "[scilmm plan] dense tail: %lld of %lld (target, descendant) panel pairs carry true entries, %lld of %lld target tile pairs are reached by a descendant (the others are padding only and skipped)\n",
                (long long)dense_pairs_kept, (long long)dense_pairs_all, (long long)dense_tiles_kept, (long long)dense_tiles_all);
      if (pb.verbose && dense_prod_all > 0)
        fprintf(stderr, "[scilmm plan] dense tail: per-pair reach keeps %lld of %lld (tile pair, descendant) products, %lld empty items (zero slabs)\n",
                (long long)dense_prod_kept, (long long)dense_prod_all, (long long)dense_items_empty);
      if (pb.verbose)
        fprintf(stderr, "[scilmm plan] dense tail: fronts %d..%d (%d wide), %lld early + %lld late implicit items (k_dense_b)\n",
                S.dense_first, S.nsuper - 1, tail_w,
                (long long)D->dwork_e_ptr[S.nlevels], (long long)D->dwork_l_ptr[S.nlevels]);
    }
    if (work_early.empty()) work_early.push_back(UpdWork{0, -1, 0, 0});
    if ((st = upload(sym, D, work_early, &D->d_work_early)) != SCILMM_OK) return st;
    if (red_tiles_e.empty()) red_tiles_e.push_back(0);
    if ((st = upload(sym, D, red_tiles_e, &D->d_red_tiles_e)) != SCILMM_OK) return st;
    if ((st = upload(sym, D, pslot_e, &D->d_tile_pslot_e)) != SCILMM_OK) return st;
    if ((st = upload(sym, D, pnseg_e, &D->d_tile_pnseg_e)) != SCILMM_OK) return st;
    if (red_tiles.empty()) red_tiles.push_back(0);
    if ((st = upload(sym, D, red_tiles, &D->d_red_tiles)) != SCILMM_OK) return st;
    if (work.empty()) work.push_back(UpdWork{0, -1, 0, 0});
    if ((st = upload(sym, D, work, &D->d_work)) != SCILMM_OK) return st;
    if ((st = upload(sym, D, pslot, &D->d_tile_pslot)) != SCILMM_OK) return st;
    if ((st = upload(sym, D, pnseg, &D->d_tile_pnseg)) != SCILMM_OK) return st;
    void* sc = nullptr;
    // three regions: early slabs by level parity (two side streams), late slabs (main stream)
    HIPCHK(hipMalloc(&sc, sizeof(double) * (size_t)4 * (size_t)D->max_slots * TM * NB));
    D->allocs.push_back(sc);
    D->scratch = (double*)sc;
    return SCILMM_OK;
  }
};

// Work items, partial slabs, the dense-tail items and the distributed batches
int cut_work_items(scilmm_symbolic* sym, Dev* D, PlanBuild& pb) {
  WorkCut wc(*sym->S, D, pb);
  for (int32_t l = 0; l < sym->S->nlevels; ++l) wc.cut_level(l);
  D->max_slots = std::max<int64_t>(wc.max_slots, 1);
  int st;
  if (wc.dist && (st = wc.plan_dist_batches(sym)) != SCILMM_OK) return st;
  return wc.upload_items(sym);
}

// ---- dense-chain plan for the triangular sweeps, the push slices of the backward sweep
int plan_chain(scilmm_symbolic* sym, Dev* D, PlanBuild& pb) {
  const Symbolic& S = *sym->S;
  int st;
  const int32_t ns = S.nsuper;
  // the sweep set: all fronts of the top levels, as many levels as fit the cap (the dense chain and the few
  // wide fronts just below it; every dependency of a member is either a member or finished by the level kernels)
  // (a level joins while it has at most `wide` fronts: a pull step costs ~8 us whatever its size, so the many
  // small fronts of the lower levels stay with the level kernels -- measured optimum at the 100k pedigree)
  const int32_t cap = D->tune.chain_cap, wide = D->tune.chain_wide;
  int32_t l0 = S.nlevels;
  while (l0 > 0 && S.level_ptr[l0] - S.level_ptr[l0 - 1] <= wide && S.level_ptr[S.nlevels] - S.level_ptr[l0 - 1] <= cap) --l0;
  int32_t T = l0 < S.nlevels ? S.level_ptr[S.nlevels] - S.level_ptr[l0] : 0;
  if (S.nlevels - l0 < 4 || D->tune.no_chain) T = 0;
  if (D->world > 1) T = 0;  // a distributed factor is swept level by level with a collective per tail block (run_rhs)
  D->chain_T = T;
  D->chain_l0 = l0;
  if (T > 0 && D->det) {
    std::vector<uint8_t> mask((size_t)ns, 0);
    for (int32_t i = 0; i < T; ++i) mask[(size_t)S.level_fronts[S.level_ptr[l0] + i]] = 1;
    if ((st = upload(sym, D, mask, &D->d_chain_mask)) != SCILMM_OK) return st;
  }
  if (T > 0) {
    std::vector<int32_t> chain(T), pos(ns, -1);
    for (int32_t i = 0; i < T; ++i) {
      chain[i] = S.level_fronts[S.level_ptr[l0] + i];  // level order = a topological order of the update pairs
      pos[chain[i]] = i;
    }
    std::vector<std::vector<ChainPair>> fw(T), bw(T);
    std::vector<int32_t> colmap;  // forward, non-contiguous pairs: target column -> row of the pair (or -1)
    std::vector<std::pair<int32_t, int32_t>> outside;  // (descendant, pair id): chain target, descendant below the chain
    for (int32_t i = 0; i < T; ++i) {
      const int32_t t = chain[i];
      for (int64_t e = S.upd_ptr[t]; e < S.upd_ptr[t + 1]; ++e) {
        const int32_t d = S.upd_src[e];
        if (pos[d] >= 0) {
          int32_t moff = 0;
          if (S.upd_jp0[e] < 0) {
            moff = (int32_t)colmap.size();
            colmap.resize(colmap.size() + NB, -1);
            const int32_t* rd = S.sn_rows.data() + S.sn_rowptr[d];
            for (int32_t q = S.upd_p0[e]; q < S.upd_p1[e]; ++q) colmap[(size_t)moff + (rd[q] - S.sn_start[t])] = q - S.upd_p0[e];
          }
          fw[i].push_back(ChainPair{pos[d], S.upd_p0[e], S.upd_p1[e] - S.upd_p0[e], S.upd_jp0[e], moff});
          bw[pos[d]].push_back(ChainPair{i, S.upd_p0[e], S.upd_p1[e] - S.upd_p0[e], S.upd_jp0[e], 0});
        } else {
          outside.push_back({d, (int32_t)e});
        }
      }
    }
    std::vector<int32_t> fptr(T + 1, 0), bptr(T + 1, 0);
    std::vector<ChainPair> fl, bl;
    for (int32_t i = 0; i < T; ++i) {
      std::sort(fw[i].begin(), fw[i].end(), [](const ChainPair& a, const ChainPair& b) { return a.other < b.other; });
      std::sort(bw[i].begin(), bw[i].end(), [](const ChainPair& a, const ChainPair& b) { return a.other > b.other; });
      fl.insert(fl.end(), fw[i].begin(), fw[i].end());
      bl.insert(bl.end(), bw[i].begin(), bw[i].end());
      fptr[i + 1] = (int32_t)fl.size();
      bptr[i + 1] = (int32_t)bl.size();
    }
    // group by descendant, order by first row, merge adjacent row ranges (rows of consecutive chain blocks)
    std::sort(outside.begin(), outside.end(), [&](const std::pair<int32_t, int32_t>& a, const std::pair<int32_t, int32_t>& b) {
      if (a.first != b.first) return a.first < b.first;
      return S.upd_p0[a.second] < S.upd_p0[b.second];
    });
    std::vector<int64_t> gptr;
    std::vector<int32_t> gpairs;  // triples (descendant, p0, p1)
    for (size_t k = 0; k < outside.size(); ++k) {
      const int32_t d = outside[k].first, e = outside[k].second;
      const bool newgrp = k == 0 || d != outside[k - 1].first;
      if (newgrp) gptr.push_back((int64_t)gpairs.size() / 3);
      if (!newgrp && gpairs.back() == S.upd_p0[e]) {
        gpairs.back() = S.upd_p1[e];
      } else {
        gpairs.push_back(d);
        gpairs.push_back(S.upd_p0[e]);
        gpairs.push_back(S.upd_p1[e]);
      }
    }
    gptr.push_back((int64_t)gpairs.size() / 3);
    std::vector<int32_t> gslot, fold;
    {
      // one workgroup sweeps its rows 32 at a time (~3.5 us per step): a descendant with 10^4 rows in the chain
      // would take a millisecond alone, so long groups are cut into slices of <= slice_rows rows
      const int64_t slice_rows = std::max<int64_t>(256, D->tune.push_slice);
      std::vector<int64_t> gptr2;
      std::vector<int32_t> gp2;
      int32_t nslots = 0;
      for (size_t g = 0; g + 1 < gptr.size(); ++g) {
        int64_t rows = 0;
        for (int64_t q = gptr[g]; q < gptr[g + 1]; ++q) rows += gpairs[3 * q + 2] - gpairs[3 * q + 1];
        const int64_t nsl = (rows + slice_rows - 1) / slice_rows;
        if (nsl <= 1) {
          gptr2.push_back((int64_t)gp2.size() / 3);
          gp2.insert(gp2.end(), gpairs.begin() + 3 * gptr[g], gpairs.begin() + 3 * gptr[g + 1]);
          gslot.push_back(-1);
          continue;
        }
        const int64_t per = (rows + nsl - 1) / nsl;
        fold.push_back(gpairs[3 * gptr[g]]);
        fold.push_back(nslots);
        int32_t made = 0;
        int64_t acc = 0;
        gptr2.push_back((int64_t)gp2.size() / 3);
        gslot.push_back(nslots + made);
        ++made;
        for (int64_t q = gptr[g]; q < gptr[g + 1]; ++q) {
          int32_t a = gpairs[3 * q + 1];
          const int32_t b = gpairs[3 * q + 2];
          while (a < b) {
            if (acc == per) {  // start the next slice
              gptr2.push_back((int64_t)gp2.size() / 3);
              gslot.push_back(nslots + made);
              ++made;
              acc = 0;
            }
            const int32_t take = (int32_t)std::min<int64_t>(b - a, per - acc);
            gp2.push_back(gpairs[3 * q]);
            gp2.push_back(a);
            gp2.push_back(a + take);
            a += take;
            acc += take;
          }
        }
        fold.push_back(made);
        nslots += made;
      }
      gptr2.push_back((int64_t)gp2.size() / 3);
      gptr.swap(gptr2);
      gpairs.swap(gp2);
      D->n_fold = (int64_t)fold.size() / 3;
      if (nslots > 0) {
        void* pp = nullptr;
        HIPCHK(hipMalloc(&pp, sizeof(double) * (size_t)nslots * NB * RPMAX));
        D->allocs.push_back(pp);
        D->d_push_partial = (double*)pp;
      }
      if (fold.empty()) fold.assign(3, 0);
      if (gslot.empty()) gslot.push_back(-1);
    }
    D->chain_groups = (int64_t)gptr.size() - 1;
    // the flat descriptors of the pipelined pair loop, pair for pair beside fl / bl
    std::vector<ChainDesc> fd(fl.size()), bd(bl.size());
    for (int32_t i = 0; i < T; ++i) {
      const int32_t s = chain[i];
      const int32_t ms = (int32_t)(S.sn_rowptr[s + 1] - S.sn_rowptr[s]);
      for (int32_t e = fptr[i]; e < fptr[i + 1]; ++e) {
        const ChainPair& p = fl[(size_t)e];
        const int32_t so = chain[p.other];
        fd[(size_t)e] = ChainDesc{S.sn_loff[so] + p.p0, (int32_t)(S.sn_rowptr[so + 1] - S.sn_rowptr[so]), S.sn_start[so + 1] - S.sn_start[so],
                                  S.sn_start[so], p.other, p.map, (int16_t)p.jp0, (int16_t)p.nq};
      }
      for (int32_t e = bptr[i]; e < bptr[i + 1]; ++e) {
        const ChainPair& p = bl[(size_t)e];
        const int32_t so = chain[p.other];
        bd[(size_t)e] = ChainDesc{S.sn_loff[s] + p.p0, ms, p.nq, S.sn_start[so] + std::max(p.jp0, 0), p.other, p.p0, (int16_t)p.jp0, (int16_t)p.nq};
      }
    }
    D->chain_desc_bytes = (int64_t)(fd.size() + bd.size()) * (int64_t)sizeof(ChainDesc);
    if (fl.empty()) fl.push_back(ChainPair{0, 0, 0, 0, 0});
    if (bl.empty()) bl.push_back(ChainPair{0, 0, 0, 0, 0});
    if (fd.empty()) fd.push_back(ChainDesc{0, 0, 0, 0, 0, 0, 0, 0});
    if (bd.empty()) bd.push_back(ChainDesc{0, 0, 0, 0, 0, 0, 0, 0});
    const long long n_colmaps = (long long)(colmap.size() / NB);
    colmap.resize(std::max(colmap.size(), (size_t)NB), -1);  // (the pipelined loop reads colmap[map + column] of contiguous pairs too)
    if ((st = upload(sym, D, fd, &D->d_cfd)) != SCILMM_OK) return st;
    if ((st = upload(sym, D, bd, &D->d_cbd)) != SCILMM_OK) return st;
    if ((st = upload(sym, D, colmap, &D->d_colmap)) != SCILMM_OK) return st;
    if (gpairs.empty()) gpairs.assign(3, 0);
    const int64_t n_ranges = (int64_t)gpairs.size() / 3;
    if ((st = upload(sym, D, chain, &D->d_chain)) != SCILMM_OK) return st;
    if ((st = upload(sym, D, fptr, &D->d_cf_ptr)) != SCILMM_OK) return st;
    if ((st = upload(sym, D, bptr, &D->d_cb_ptr)) != SCILMM_OK) return st;
    if ((st = upload(sym, D, fl, &D->d_cf)) != SCILMM_OK) return st;
    if ((st = upload(sym, D, bl, &D->d_cb)) != SCILMM_OK) return st;
    if ((st = upload(sym, D, gptr, &D->d_cg_ptr)) != SCILMM_OK) return st;
    if ((st = upload(sym, D, gpairs, &D->d_cg_pairs)) != SCILMM_OK) return st;
    if ((st = upload(sym, D, gslot, &D->d_cg_slot)) != SCILMM_OK) return st;
    if ((st = upload(sym, D, fold, &D->d_fold)) != SCILMM_OK) return st;
    std::vector<int32_t> zeros((size_t)T * (RPMAX / CW) + 4, 0);
    if ((st = upload(sym, D, zeros, &D->d_chain_flags)) != SCILMM_OK) return st;
    D->d_chain_err = D->d_chain_flags + (size_t)T * (RPMAX / CW);
    HIPCHK(hipHostMalloc((void**)&D->h_chain_err, sizeof(int32_t), hipHostMallocDefault));
    *D->h_chain_err = 0;
    if (pb.verbose)
      fprintf(stderr, "[scilmm plan] chain sweep: %d fronts (levels %d..%d), %lld inner pairs (%lld column maps, %lld descriptor bytes), %lld outside pairs in %lld groups\n",
              T, l0, S.nlevels - 1, (long long)fl.size(), n_colmaps, (long long)D->chain_desc_bytes, (long long)outside.size(), (long long)D->chain_groups);
    (void)n_ranges;
  }
  return SCILMM_OK;
}

}  // namespace

int ensure_device(scilmm_symbolic* sym, Dev** out) {
  if (sym->device) {
    *out = (Dev*)sym->device;
    return SCILMM_OK;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    sym->err = "no HIP device available (the numeric phase has no CPU fallback)";
    return SCILMM_ERR_DEVICE;
  }
  PlanBuild pb;
  pb.verbose = verbose();
  {
    // a stale "last error" of this host thread (left by any earlier runtime call, ours or the caller's) would be
    // reported by the first library that polls hipGetLastError() -- hipCUB does, inside the plan construction
    const hipError_t stale = hipGetLastError();
    if (stale != hipSuccess && pb.verbose)
      fprintf(stderr, "[scilmm plan] cleared a stale HIP error of this thread: %s\n", hipGetErrorString(stale));
  }
  // (a stage that fails leaves sym->device set: device_free releases what was allocated so far)
  Dev* D = new Dev();
  sym->device = D;
  sym->device_free = dev_free;
  if (hipGetDevice(&D->device) != hipSuccess) D->device = 0;  // the handle binds to the caller's current device
  for (auto& e : D->ev) e = nullptr;
  D->tune = read_tuning();
  D->det = sym->deterministic;
  D->use_mfma = !D->tune.no_mfma;
  D->trsm_lite = D->tune.trsm_lite;
#ifdef SCILMM_DIAG
  const char* ab = getenv("SCILMM_ABLATE");  // timing ablations (WRONG numbers): diagnostic builds only
  D->ablate = ab ? atoi(ab) : 0;
#endif
  int st;
  if ((st = create_streams_and_events(sym, D)) != SCILMM_OK) return st;
  if ((st = check_block_widths(sym)) != SCILMM_OK) return st;
  if ((st = plan_ownership(sym, D, pb)) != SCILMM_OK) return st;
  if ((st = choose_tail_paths(sym, D)) != SCILMM_OK) return st;
  if (D->outside_on && (st = plan_outside(sym, D, pb)) != SCILMM_OK) return st;
  if (!sym->S->combos_built) {
    // (a handle analysed through scilmm_symbolic_get("combo_*") carries the full lists: then the dense path stays off)
    scilmm::build_tile_combos(sym->S, D->world > 1 ? D->keep_front.data() : nullptr, D->dense_on,
                              D->outside_on ? D->outside_desc.data() : nullptr);
    pb.lap("tile combos");
  } else {
    D->dense_on = false;
  }
  if ((st = upload_symbolic(sym, D)) != SCILMM_OK) return st;
  pb.lap("symbolic arrays -> device");
  if (D->det) {
    if ((st = upload_deterministic_plan(sym, D)) != SCILMM_OK) return st;
    pb.lap("deterministic mode: pull schedule, row index");
  }
  if ((st = classify_combos(sym, D, pb)) != SCILMM_OK) return st;
  pb.lap("classify combos, list cells");
  if ((st = build_cells(sym, D, pb)) != SCILMM_OK) return st;
  pb.lap("sort/group/upload cells");
  if ((st = cut_work_items(sym, D, pb)) != SCILMM_OK) return st;
  pb.lap("work items, slabs");
  if ((st = plan_chain(sym, D, pb)) != SCILMM_OK) return st;
  pb.lap("chain sweep plan");
  *out = D;
  return SCILMM_OK;
}

// The order-fixed selected inverse (deterministic mode): which sums go through slots, and where.  Everything is a function
// of the analysis and of T alone.
//  * tail: the items of a front are [K range][row tile] (ensure_sinv_plan), so item i of the front's launch is its own
//    slot i and row tile q sums slots q, ntile + q, ...; a front with one K range stores straight into its panel.
//  * diagonal blocks: the 128-row tiles of a front that hold rows of R are cut into segments of T consecutive tiles, in row
//    order; a front with one segment subtracts in place, the others take consecutive slots of their level.
struct SinvOrderedStats {
  int64_t tail_direct = 0, tail_folded = 0, tail_slots = 0;  // row tiles | row tiles | their slots
  int64_t cc_direct = 0, cc_folded = 0;                      // segments
  int64_t tail_bytes = 0, cc_bytes = 0;                      // the two slot buffers
  int T = 0;
};

static void plan_sinv_ordered(const Symbolic& S, Dev* D, int T, std::vector<SinvSeg>* segs, std::vector<SinvFold>* folds,
                              SinvOrderedStats* os) {
  os->T = T;
  const int32_t nT = S.nsuper - S.dense_first;
  D->sinv_tail_nseg.assign((size_t)std::max(nT, 1), 0);
  int64_t tail_slots_max = 0;  // doubles: slots of the front that needs most, each of its own width
  for (int32_t jj = 0; jj < nT; ++jj) {
    const int64_t items = D->sinv_work_ptr[(size_t)jj + 1] - D->sinv_work_ptr[(size_t)jj];
    if (items == 0) continue;
    const int32_t f = S.dense_first + jj;
    const int64_t u = (int64_t)S.n - S.sn_start[f + 1], ntile = (u + 255) / 256;
    const int64_t nseg = items / ntile;  // (every K range holds all ntile row tiles)
    D->sinv_tail_nseg[(size_t)jj] = (int32_t)nseg;
    if (nseg > 1) {
      os->tail_folded += ntile;
      os->tail_slots += items;
      tail_slots_max = std::max(tail_slots_max, items * sinv_tail_slot((int)((S.sn_start[f + 1] - S.sn_start[f] + 15) / 16)));
    } else {
      os->tail_direct += ntile;
    }
  }
  os->tail_bytes = tail_slots_max * (int64_t)sizeof(double);
  D->sinv_cc_seg_ptr.assign((size_t)S.nlevels + 1, 0);
  D->sinv_cc_fold_ptr.assign((size_t)S.nlevels + 1, 0);
  int64_t cc_slots_max = 0;
  for (int32_t l = 0; l < S.nlevels; ++l) {
    int32_t slot = 0;
    for (int32_t q = S.level_ptr[l]; q < S.level_ptr[l + 1]; ++q) {
      const int32_t f = S.level_fronts[q];
      const int64_t w = S.sn_start[f + 1] - S.sn_start[f], m = S.sn_rowptr[f + 1] - S.sn_rowptr[f];
      if (m <= w) continue;  // no R: the diagonal block is L11^-T L11^-1 already
      const int32_t t0 = (int32_t)(w / TM), t1 = (int32_t)((m + TM - 1) / TM);  // tiles [t0, t1) hold the rows w .. m
      const int32_t nseg = (t1 - t0 + T - 1) / T;
      if (nseg > 1) folds->push_back(SinvFold{f, slot, nseg});
      for (int32_t g = 0; g < nseg; ++g)
        segs->push_back(SinvSeg{f, t0 + g * T, std::min(T, t1 - (t0 + g * T)), nseg > 1 ? slot++ : -1});
      (nseg > 1 ? os->cc_folded : os->cc_direct) += nseg;
    }
    cc_slots_max = std::max<int64_t>(cc_slots_max, slot);
    D->sinv_cc_seg_ptr[(size_t)l + 1] = (int64_t)segs->size();
    D->sinv_cc_fold_ptr[(size_t)l + 1] = (int64_t)folds->size();
  }
  os->cc_bytes = cc_slots_max * SINV_CC_SLOT * (int64_t)sizeof(double);
}

// The selected inverse's plan, built with the first scilmm_selected_inverse of a handle: column -> front, where every
// front's Y = L21 L11^-1 lives inside the per-level scratch (dense-tail fronts keep it transposed, [u][128]), the
// non-tail tiles by level, and the items of the dense-tail kernel
int ensure_sinv_plan(scilmm_symbolic* sym, Dev* D) {
  if (D->d_col_front) return SCILMM_OK;
  const Symbolic& S = *sym->S;
  std::vector<int32_t> cf((size_t)std::max(S.n, 1), 0);
  for (int32_t f = 0; f < S.nsuper; ++f)
    for (int32_t c = S.sn_start[f]; c < S.sn_start[f + 1]; ++c) cf[(size_t)c] = f;
  std::vector<int64_t> yo((size_t)std::max(S.nsuper, 1), 0);
  int64_t ymax = 1;
  D->sinv_tail_front.assign((size_t)std::max(S.nlevels, 1), -1);
  D->sinv_pre_ptr.assign((size_t)S.nlevels + 1, 0);
  std::vector<int32_t> pre_tiles;
  for (int32_t l = 0; l < S.nlevels; ++l) {
    int64_t at = 0;
    for (int32_t q = S.level_ptr[l]; q < S.level_ptr[l + 1]; ++q) {
      const int32_t f = S.level_fronts[q];
      const int64_t w = S.sn_start[f + 1] - S.sn_start[f], u = (S.sn_rowptr[f + 1] - S.sn_rowptr[f]) - w;
      yo[(size_t)f] = at;
      at += ((f >= S.dense_first ? u * NB : u * w) + 1) & ~(int64_t)1;
      if (f >= S.dense_first) D->sinv_tail_front[(size_t)l] = f;
    }
    ymax = std::max(ymax, at);
    for (int64_t q = S.level_tile_ptr[l]; q < S.level_tile_ptr[l + 1]; ++q)
      if (S.tile_front[S.level_tiles[q]] < S.dense_first) pre_tiles.push_back(S.level_tiles[q]);
    D->sinv_pre_ptr[(size_t)l + 1] = (int64_t)pre_tiles.size();
  }
  // dense-tail items: (front s, 256 rows of R, a range of later fronts); about 1024 items per front
  std::vector<SinvWork> sw;
  std::vector<int32_t> tails;
  const int32_t nT = S.nsuper - S.dense_first;
  D->sinv_work_ptr.assign((size_t)nT + 1, 0);
  for (int32_t jj = 0; jj < nT; ++jj) {
    const int32_t f = S.dense_first + jj;
    tails.push_back(f);
    const int64_t w = S.sn_start[f + 1] - S.sn_start[f], u = (int64_t)S.n - S.sn_start[f] - w;
    const int32_t count = S.nsuper - 1 - f;  // later fronts
    if (u > 0 && count > 0) {
      const int64_t ntile = (u + 255) / 256;
      // about 1024 items per front, and a count that fills the last round of 256 workgroups: the fronts' launches follow
      // each other on one stream, so I items cost ceil(I / 256) rounds with nothing to fill the gap
      const int64_t base = std::max<int64_t>(1, std::min<int64_t>(count, 1024 / ntile));
      int32_t nseg = (int32_t)base;
      double best = -1.0;
      for (int64_t c = std::max<int64_t>(1, base / 2); c <= std::min<int64_t>(count, 2 * base + 1); ++c) {
        const int64_t items = ntile * c, rounds = (items + 255) / 256;
        const double score = (double)items / (double)(rounds * 256) - 0.02 * std::fabs((double)(c - base)) / (double)base;
        if (score > best) { best = score; nseg = (int32_t)c; }
      }
      for (int32_t sg = 0; sg < nseg; ++sg) {
        const int32_t ka = f + 1 + (int32_t)((int64_t)count * sg / nseg), kb = f + 1 + (int32_t)((int64_t)count * (sg + 1) / nseg);
        if (kb <= ka) continue;
        for (int64_t q = 0; q < ntile; ++q) sw.push_back(SinvWork{f, (int32_t)q, ka, kb});
      }
    }
    D->sinv_work_ptr[(size_t)jj + 1] = (int64_t)sw.size();
  }
  // deterministic mode: the same items, summed in an order the lists below fix (k_sinv_tail<true> + k_sinv_tail_fold,
  // k_sinv_cc_ordered + k_sinv_cc_fold)
  SinvOrderedStats os;
  std::vector<SinvSeg> cc_segs;
  std::vector<SinvFold> cc_folds;
  if (D->det) plan_sinv_ordered(S, D, read_tuning().sinv_cc_tiles, &cc_segs, &cc_folds, &os);
  if (verbose()) {
    int64_t multi = 0;
    for (const SinvWork& it : sw) multi += it.kb - it.ka > 1;
    fprintf(stderr, "[scilmm plan] selected inverse: %d tail fronts, %lld items, %lld of them over more than one front, pre-tail tiles %lld\n",
            (int)nT, (long long)sw.size(), (long long)multi, (long long)pre_tiles.size());
    if (D->det)
      fprintf(stderr, "[scilmm plan] selected inverse, order-fixed: tail row tiles %lld direct, %lld folded from %lld slots (%lld bytes); "
                      "cc segments of up to %d tiles: %lld direct, %lld folded (%lld bytes)\n",
              (long long)os.tail_direct, (long long)os.tail_folded, (long long)os.tail_slots, (long long)os.tail_bytes, os.T,
              (long long)os.cc_direct, (long long)os.cc_folded, (long long)os.cc_bytes);
  }
  if (sw.empty()) sw.push_back(SinvWork{0, 0, 0, 0});
  if (tails.empty()) tails.push_back(0);
  if (pre_tiles.empty()) pre_tiles.push_back(0);
  int stq;
  if (D->det) {  // (before d_col_front, which marks the plan as built: a handle that could not get its slots has no plan)
    if (cc_segs.empty()) cc_segs.push_back(SinvSeg{0, 0, 0, -1});
    if (cc_folds.empty()) cc_folds.push_back(SinvFold{0, 0, 0});
    if ((stq = upload(sym, D, cc_segs, &D->d_sinv_cc_segs)) != SCILMM_OK) return stq;
    if ((stq = upload(sym, D, cc_folds, &D->d_sinv_cc_folds)) != SCILMM_OK) return stq;
    void* pt = nullptr;
    HIPCHK(hipMalloc(&pt, (size_t)std::max<int64_t>(os.tail_bytes, 8)));
    D->allocs.push_back(pt);
    D->d_sinv_tail_partial = (double*)pt;
    void* pc = nullptr;
    HIPCHK(hipMalloc(&pc, (size_t)std::max<int64_t>(os.cc_bytes, 8)));
    D->allocs.push_back(pc);
    D->d_sinv_cc_partial = (double*)pc;
  }
  if ((stq = upload(sym, D, cf, &D->d_col_front)) != SCILMM_OK) return stq;
  if ((stq = upload(sym, D, yo, &D->d_yoff)) != SCILMM_OK) return stq;
  if ((stq = upload(sym, D, pre_tiles, &D->d_sinv_pre_tiles)) != SCILMM_OK) return stq;
  if ((stq = upload(sym, D, tails, &D->d_sinv_tail_fronts)) != SCILMM_OK) return stq;
  if ((stq = upload(sym, D, sw, &D->d_sinv_work)) != SCILMM_OK) return stq;
  void* yb = nullptr;
  HIPCHK(hipMalloc(&yb, sizeof(double) * (size_t)ymax));
  D->allocs.push_back(yb);
  D->d_ybuf = (double*)yb;
  if (!D->d_zeros) {
    HIPCHK(hipMalloc((void**)&D->d_zeros, 2048));
    HIPCHK(hipMemset(D->d_zeros, 0, 2048));
  }
  return SCILMM_OK;
}

}  // namespace scilmm
