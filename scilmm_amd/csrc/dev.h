// Device state of a symbolic handle (struct Dev), the schedule switches (struct Tuning) and the small helpers shared by
// the device translation units: HIPCHK / TRY, DevGuard, the owner of a call's temporary device memory (DevScratch) and
// the handle's grow-only buffers (grow, ensure_io, ensure_vals, ensure_iperm).  plan.hip builds the state once per handle,
// engine.hip and the headers it includes run the launch sequences on it.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <optional>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/scilmm_hip.h"
#include "plan_types.h"
#include "handles.h"

namespace scilmm {

// Schedule / tuning switches.  They are honoured only when SCILMM_TUNING=1 is set as well, so that a stray variable in a
// production environment cannot change the schedule.  Every value of every such switch gives the same factor to
// rounding (parity-tested); switches that would change RESULTS (the timing ablations) exist only in builds with
// -DSCILMM_DIAG.  A std::optional member is a switch whose default is decided from the matrix: unset -> decide.
// (INTEGRATION.md section 3 has the table; keep the two in step.)
// Parity-tested means: a case of tests/test_gpu_factor_schedules.py or of test_gpu_parity.py's schedule table sets the switch,
// factors with it and compares L, log-det, solves and L*R with the oracle -- the factor schedules there (dense tail, k_outside,
// item and slab counts, panel solve, side streams, fp32 fronts), the cell path, chain plan and look-ahead in test_gpu_parity;
// the chain sweeps' per-call switches in test_gpu_chain_pipeline.py, the selected inverse's in test_gpu_selected_inverse.py and
// test_gpu_sinv_deterministic.py, the distributed tail's in test_zz_gpu_dist.py.  tests/test_factor_shapes.py reads the names
// out of read_tuning() below and fails when one of them is set by no case and not exempted there with a reason.
struct Tuning {
  // -- read when the device plan of a handle is built (Dev::tune)
  int reserve_cus = 0;                 // SCILMM_RESERVE_CUS     CUs the look-ahead side streams leave free (CU mask); 0: none
  int side_streams = 2;                // SCILMM_SIDE_STREAMS    1 / 2 / 3 side streams for the early updates
  bool no_mfma = false;                // SCILMM_NO_MFMA=1       scalar kernels
  bool trsm_lite = true;               // SCILMM_TRSM_LITE=0     k_trsm<true> instead of k_trsm_lite
  std::optional<bool> dense;           // SCILMM_DENSE=1/0       dense-tail path (k_dense_b); unset: tails of 8192+ columns
  std::optional<bool> outside;         // SCILMM_OUTSIDE=1/0     k_outside; unset: tails of 8192+ columns
  bool outside_merge = true;           // SCILMM_OUTSIDE_MERGE=0 no groups of descendants with identical tail rows
  std::optional<int> outside_chunks;   // SCILMM_OUTSIDE_CHUNKS  launches of k_outside; unset: one per ~16k block pairs, 4 .. 32
  bool outside_prio = false;           // SCILMM_OUTSIDE_PRIO=1  k_outside on a stream of the chain's priority
  std::optional<double> cell_limit;    // SCILMM_CELL_LIMIT      pairs with cells*width up to this take the cell-wise path;
                                       //                        unset: 4096, lowered until the plan has < 1.5e9 cells
  bool no_lookahead = false;           // SCILMM_NO_LOOKAHEAD=1  every update on the main stream
  int look_depth = 2;                  // SCILMM_LOOK_DEPTH      "late" = descendants at most this many levels below (>= 1)
  bool host_cells = false;             // SCILMM_HOST_CELLS=1    cell lists enumerated on the host
  bool no_splitk = false;              // SCILMM_NO_SPLITK=1     one work item per tile and launch
  int64_t target_items = 1024;         // SCILMM_TARGET_ITEMS    explicit work items per launch (target)
  int64_t min_item = 24;               // SCILMM_MIN_ITEM        cost units of an item, lower bound
  int64_t max_item = 96;               // SCILMM_MAX_ITEM        ... and upper bound (>= min_item)
  std::optional<int64_t> dense_items;  // SCILMM_DENSE_ITEMS     k_dense_b items per launch (>= 64); unset: 128 / 512 / 1024
                                       //                        for tails below 24576 / below 32768 / wider
  int64_t dense_fill = 256;            // SCILMM_DENSE_FILL      workgroups per round the dense item counts are fitted to; 0: off
  std::optional<bool> dense_taper;     // SCILMM_DENSE_TAPER=1/0 shorter items at the end of an early dense launch;
                                       //                        unset: on for launches of 1024 items
  std::optional<int> dist_group;       // SCILMM_DIST_GROUP      source-group size of a distributed tail; unset: >= 8
  bool dist_nosplit = false;           // SCILMM_DIST_NOSPLIT=1  no look-ahead split of a distributed target's late update
  int chain_cap = 2048;                // SCILMM_CHAIN_CAP       fronts the chain sweep takes at most
  int chain_wide = 12;                 // SCILMM_CHAIN_WIDE      a level joins the chain while it has at most this many fronts
  bool no_chain = false;               // SCILMM_NO_CHAIN=1      level kernels only
  int64_t push_slice = 512;            // SCILMM_PUSH_SLICE      rows per slice of a long backward push group (>= 256)
  // -- read per call (the parity tests force each value on one handle)
  bool shadow = true;                  // SCILMM_SHADOW=0        run_factorize: k_dense32 instead of the fp32 shadow (k_dense_h)
  bool dense_feed = true;              // SCILMM_DENSE_FEED=0    run_factorize: k_dense_b's chunk loop before the hand-counted waits
                                       //                        (k_dense_b<0>; same bits: tests/test_gpu_dense_feed.py)
  int chain_wide_t = 160;              // SCILMM_CHAIN_WIDE_T    run_rhs: chains from this length on sweep 64-column windows (pipelined pair loop)
  int chain_full_t = 768;              // SCILMM_CHAIN_FULL_T    run_rhs: ... and from this length on one 112-column window
  bool chain_pipe = true;              // SCILMM_CHAIN_PIPE=0    run_rhs: k_chain's pair loop without the software pipeline
  int chain_stagger = 0;               // SCILMM_CHAIN_STAGGER   run_rhs: a chain workgroup with more pairs than this first waits for
                                       //                        its k-th-from-last pair (short chains reach the pipelined branch); 0: off
  bool sinv_generic = false;           // SCILMM_SINV_GENERIC=1  selected inverse: the gather kernel for the dense tail too
  bool sinv_reverse = false;           // SCILMM_SINV_REVERSE=1  selected inverse, deterministic mode: workgroup b of an ordered launch
                                       //                        takes item gridDim.x - 1 - b (the bits must not move)
  // -- read when the selected inverse's plan is built (the handle's first scilmm_selected_inverse)
  int sinv_cc_tiles = 2;               // SCILMM_SINV_CC_TILES   deterministic mode: 128-row tiles per segment of k_sinv_cc_ordered (>= 1)
};

// SCILMM_DENSE_FEED=0 (under SCILMM_TUNING=1, read per factorization) runs k_dense_b's chunk loop as it was before the
// hand-counted waits (k_dense_b<0>).  It changes no schedule, no item and no bit of the factor -- its cases are
// tests/test_gpu_dense_feed.py and test_gpu_dense_reach.py, which compare L bit for bit -- so it is read here and not among
// the schedule switches whose every value the parity tables of test_gpu_factor_schedules.py factor against the oracle.
inline bool read_dense_feed() {
  const char* gate = getenv("SCILMM_TUNING");
  const char* e = getenv("SCILMM_DENSE_FEED");
  return !(gate && gate[0] == '1' && e && e[0] == '0');
}

// The environment is read on every call: tests switch SCILMM_TUNING and a switch on and off inside one process.
inline Tuning read_tuning() {
  Tuning t;
  t.dense_feed = read_dense_feed();
  const char* gate = getenv("SCILMM_TUNING");
  if (!(gate && gate[0] == '1')) return t;
  auto env = [](const char* name) { return getenv(name); };
  auto is1 = [&](const char* name) { const char* e = env(name); return e && e[0] == '1'; };
  auto not0 = [&](const char* name) { const char* e = env(name); return !(e && e[0] == '0'); };
  const char* e;
  if ((e = env("SCILMM_RESERVE_CUS"))) t.reserve_cus = atoi(e);
  if ((e = env("SCILMM_SIDE_STREAMS"))) t.side_streams = atoi(e);
  t.no_mfma = is1("SCILMM_NO_MFMA");
  t.trsm_lite = not0("SCILMM_TRSM_LITE");
  if ((e = env("SCILMM_DENSE"))) t.dense = e[0] != '0';
  if ((e = env("SCILMM_OUTSIDE"))) t.outside = e[0] != '0';
  t.outside_merge = not0("SCILMM_OUTSIDE_MERGE");
  if ((e = env("SCILMM_OUTSIDE_CHUNKS"))) t.outside_chunks = atoi(e);
  t.outside_prio = is1("SCILMM_OUTSIDE_PRIO");
  if ((e = env("SCILMM_CELL_LIMIT"))) t.cell_limit = atof(e);
  t.no_lookahead = is1("SCILMM_NO_LOOKAHEAD");
  if ((e = env("SCILMM_LOOK_DEPTH"))) t.look_depth = std::max(1, atoi(e));
  t.host_cells = is1("SCILMM_HOST_CELLS");
  t.no_splitk = is1("SCILMM_NO_SPLITK");
  if ((e = env("SCILMM_TARGET_ITEMS"))) t.target_items = atoll(e);
  if ((e = env("SCILMM_MIN_ITEM"))) t.min_item = atoll(e);
  if ((e = env("SCILMM_MAX_ITEM"))) t.max_item = atoll(e);
  if ((e = env("SCILMM_DENSE_ITEMS"))) t.dense_items = atoll(e);
  if ((e = env("SCILMM_DENSE_FILL"))) t.dense_fill = atoll(e);
  if ((e = env("SCILMM_DENSE_TAPER"))) t.dense_taper = e[0] == '1';
  if ((e = env("SCILMM_DIST_GROUP"))) t.dist_group = atoi(e);
  t.dist_nosplit = is1("SCILMM_DIST_NOSPLIT");
  if ((e = env("SCILMM_CHAIN_CAP"))) t.chain_cap = atoi(e);
  if ((e = env("SCILMM_CHAIN_WIDE"))) t.chain_wide = atoi(e);
  t.no_chain = is1("SCILMM_NO_CHAIN");
  if ((e = env("SCILMM_PUSH_SLICE"))) t.push_slice = atoll(e);
  t.shadow = not0("SCILMM_SHADOW");
  if ((e = env("SCILMM_CHAIN_WIDE_T"))) t.chain_wide_t = atoi(e);
  if ((e = env("SCILMM_CHAIN_FULL_T"))) t.chain_full_t = atoi(e);
  t.chain_pipe = not0("SCILMM_CHAIN_PIPE");
  if ((e = env("SCILMM_CHAIN_STAGGER"))) t.chain_stagger = std::max(0, atoi(e));
  t.sinv_generic = is1("SCILMM_SINV_GENERIC");
  t.sinv_reverse = is1("SCILMM_SINV_REVERSE");
  if ((e = env("SCILMM_SINV_CC_TILES"))) t.sinv_cc_tiles = std::max(1, atoi(e));
  return t;
}

// SCILMM_VERBOSE only prints (the [scilmm plan] lines); it is not gated by SCILMM_TUNING.
inline bool verbose() { return getenv("SCILMM_VERBOSE") != nullptr; }

// The HIP-event timer of one call family behind a block (Dev holds one per family): n intervals between n + 1 events on the
// call's stream, plus `extra` marks that belong to no interval (the scan block's gxe marks).  A call does start, mark .., close;
// scilmm_sync reads whatever is pending, and ms keeps the last read call's figures until a later call of the family has been
// read.  The events are created by the family's first call on the handle.
struct StageTimer {
  static constexpr int MAX_EVENTS = 6;
  const int n, extra;
  hipEvent_t ev[MAX_EVENTS] = {};
  bool pending = false;                 // a call whose events have not been read yet
  double ms[MAX_EVENTS - 1] = {};
  explicit StageTimer(int intervals, int extra_marks = 0) : n(intervals), extra(extra_marks) {}
  hipError_t mark(hipStream_t s, int i) { return hipEventRecord(ev[i], s); }
  hipError_t start(hipStream_t s) {
    if (!ev[0])
      for (int i = 0; i <= n + extra; ++i)
        if (const hipError_t e = hipEventCreate(&ev[i]); e != hipSuccess) return e;
    return mark(s, 0);
  }
  hipError_t close(hipStream_t s) {
    const hipError_t e = mark(s, n);
    pending = pending || e == hipSuccess;
    return e;
  }
  // the time from mark a to mark b of a call that has finished
  hipError_t between(int a, int b, double* out) const {
    float t = 0;
    const hipError_t e = hipEventElapsedTime(&t, ev[a], ev[b]);
    if (e == hipSuccess) *out = t;
    return e;
  }
  hipError_t read() {
    if (!pending) return hipSuccess;
    pending = false;
    for (int i = 0; i < n; ++i)
      if (const hipError_t e = between(i, i + 1, &ms[i]); e != hipSuccess) return e;
    return hipSuccess;
  }
  void destroy() {
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

struct Dev {
  int device = 0;                  // HIP device the handle was created on; every entry point runs on it (DevGuard)
  hipStream_t stream = nullptr;
  Tuning tune;                     // the schedule switches as they were when this state was created
  int prio_lo = 0, prio_hi = 0;    // stream priority range of the device (hi: the main stream's)
  DevSym v{};
  std::vector<void*> allocs;
  int32_t* d_level_tiles = nullptr;
  int32_t* d_level_fronts = nullptr;
  int32_t* d_level_pairs = nullptr;
  int32_t* d_all_fronts = nullptr;  // multi-GPU: Symbolic::level_fronts unfiltered (the forward sweep solves every
                                    // tail block on every rank: the inverse diagonal blocks are replicated)
  std::vector<double*> vals;       // per matrix: pattern-order values or diagonal values
  std::vector<uint8_t> have_vals;
  double* W = nullptr;             // n x RPMAX workspaces (permuted right-hand sides)
  double* X = nullptr;
  double* IO = nullptr;            // staging for host<->device dense transfers
  size_t io_cap = 0;
  double* partial = nullptr;       // block partial sums of the quadratic forms
  size_t partial_cap = 0;          // doubles
  double* d_out = nullptr;         // RPMAX doubles
  bool use_mfma = true;
  bool trsm_lite = true;           // k_trsm_lite instead of k_trsm<true> (SCILMM_TUNING=1 SCILMM_TRSM_LITE=0: the round-1 kernel)
  hipEvent_t ev[8];
  scilmm_timing timing{};
  bool quad_pending = false;           // a scilmm_quadforms_dev call whose timer has not been read yet
  bool attrs_set = false;
  // update-kernel plan: flattened combo descriptors, per-level work items (split-K), partial slots
  ComboDesc* d_combos = nullptr;
  UpdWork* d_work = nullptr;
  std::vector<int64_t> work_ptr;   // [nlevels+1] LATE items (descendants one level below the target): main stream
  UpdWork* d_work_early = nullptr; // EARLY items (older descendants): side stream, overlaps the previous level
  std::vector<int64_t> early_ptr;  // [nlevels+1]
  int64_t max_slots = 0;           // partial slabs per scratch half (scratch is double-buffered by level parity)
  hipStream_t side = nullptr;
  hipStream_t side2 = nullptr;     // early updates alternate between two side streams (their tails overlap)
  hipStream_t side3 = nullptr;     // optional third one (SCILMM_SIDE_STREAMS=3)
  int nside = 2;
  bool serial_early = false;       // profiling mode 2: every early launch on ONE side stream (launch durations do not overlap)
  std::vector<hipEvent_t> lev_ev;  // 2 per level: [2l] = level l finished, [2l+1] = early update of level l finished
  hipEvent_t ev_asm = nullptr;
  hipEvent_t ev_x0 = nullptr, ev_x1 = nullptr;  // main <-> comm stream hand-offs (multi-GPU)
  int32_t* d_tile_pslot = nullptr;   // late partial slabs of a tile (main stream)
  int32_t* d_tile_pnseg = nullptr;
  int32_t* d_tile_pslot_e = nullptr; // early partial slabs of a tile (side stream)
  int32_t* d_tile_pnseg_e = nullptr;
  int32_t* d_red_tiles_e = nullptr;
  std::vector<int64_t> red_ptr_e;
  std::vector<int64_t> lev_cost_e, lev_cost_l;  // per-level dense update cost units (diagnostics)
  double* scratch = nullptr;       // max slots per level * TM*NB doubles
  int32_t* d_red_tiles = nullptr;  // tiles that carry partial slabs, grouped by level
  // cell-wise path for small update pairs: set 0 = early (side stream), set 1 = late (main stream)
  struct CellSet {
    int64_t* dst = nullptr;
    int64_t* grp = nullptr;
    int64_t* srct = nullptr;
    int64_t* srcq = nullptr;
    int32_t* md = nullptr;
    int32_t* wd = nullptr;
    std::vector<int64_t> level_ptr;    // [nlevels+1] over unique target cells
    std::vector<int64_t> level_short;  // [nlevels] short groups (listed first) per level
  } cellset[3];  // 0 = early (side streams), 1 = late (main stream); 2 unused (kept for the device cell plan's key layout)
  int64_t n_dense_combos = 0, n_sparse_combos = 0, n_cells = 0;
  std::vector<int64_t> red_ptr;    // [nlevels+1]
  bool profiling = false;
  int ablate = 0;
  // multi-GPU: the fronts of the dense tail (>= dist_first) are owned 1-D block-cyclically.  A rank STORES the prelude
  // (replicated), its own tail panels and a ring of dist_G slots through which the other ranks' panels pass (fan-out:
  // a received panel is applied to every own target that needs it and then dropped) -- see DistLayout.
  int32_t rank = 0, world = 1;
  int32_t dist_first = 0;               // first distributed front (nsuper: nothing is distributed)
  int32_t dist_Wg = 8, dist_G = 32;     // source-group size of the batched updates; ring slots
  std::vector<int64_t> loff;            // [nsuper+1] rank-local panel offsets (== Symbolic::sn_loff when world == 1)
  int64_t nL_local = 0;                 // doubles of rank-local panel storage (prelude + own tail + ring)
  std::vector<uint8_t> keep_front;      // [nsuper] this rank computes the panel of front s
  std::vector<int32_t> tail_of_level;   // [nlevels] the distributed front of level l, or -1
  // level lists without the tail fronts of other ranks (== the Symbolic's when world == 1)
  std::vector<int32_t> lv_ptr, lv_fronts, lv_tiles, lv_pairs;  // lv_ptr: [nlevels+1] into lv_fronts
  std::vector<int64_t> lv_tile_ptr, lv_tile_mid, lv_pair_ptr;  // lv_tile_mid[l]: first tile of the level's own distributed panel
  int32_t* d_lmul_tiles = nullptr;      // tiles this rank multiplies in L*R (own tail; the prelude on rank 0 only)
  int64_t n_lmul_tiles = 0;
  DenseWork* d_dwork_b = nullptr;       // batch items of the distributed tail
  std::vector<int64_t> dbatch_ptr;      // [ngroups+1]
  std::vector<hipEvent_t> batch_ev;     // [ngroups] batch g applied to all own targets
  std::vector<hipEvent_t> bpev;         // profiling: [2 ngroups] begin / end of batch g on the batches' stream
  std::vector<int32_t> last_own_level;  // [ngroups] level of this rank's last own tail front in group g, or -1
  hipStream_t bstream = nullptr;        // the batches' stream
  hipStream_t comm = nullptr;           // caller-owned stream the collectives are issued on
  std::vector<hipEvent_t> done_ev;      // per level with a distributed front: this rank's kernels of the level finished
  double* ACC = nullptr;                // forward sweep: contributions of this rank's own tail panels, n x RPMAX (dist)
  // selected inverse (scilmm_selected_inverse): column -> front, per-front offset of Y inside the per-level scratch
  int32_t* d_col_front = nullptr;
  int64_t* d_yoff = nullptr;
  double* d_ybuf = nullptr;
  int32_t* d_sinv_pre_tiles = nullptr;        // tiles of the non-tail fronts, by level (k_sinv_w)
  std::vector<int64_t> sinv_pre_ptr;          // [nlevels+1]
  std::vector<int32_t> sinv_tail_front;       // [nlevels] the dense-tail front of the level, or -1
  int32_t* d_sinv_tail_fronts = nullptr;      // the tail fronts, one per entry (k_sinv_zero takes a list)
  SinvWork* d_sinv_work = nullptr;            // items of k_sinv_tail, grouped by tail front
  std::vector<int64_t> sinv_work_ptr;         // [ntail+1]
  // ... in deterministic mode (the order-fixed forms): nothing below is built on a default handle
  std::vector<int32_t> sinv_tail_nseg;        // [ntail] K ranges per row tile of the front's items; > 1: slots + k_sinv_tail_fold
  double* d_sinv_tail_partial = nullptr;      // [items of the largest folded front][256 x NB]
  SinvSeg* d_sinv_cc_segs = nullptr;          // segments of k_sinv_cc_ordered, by level
  std::vector<int64_t> sinv_cc_seg_ptr;       // [nlevels+1]
  SinvFold* d_sinv_cc_folds = nullptr;        // fronts with several segments, by level (k_sinv_cc_fold)
  std::vector<int64_t> sinv_cc_fold_ptr;      // [nlevels+1]
  double* d_sinv_cc_partial = nullptr;        // [slots of the largest level][TM x NB]
  bool work_external = false;           // W / X / ACC belong to the caller (scilmm_dist_set_work)
  // dense tail (Symbolic::dense_first): implicit work items of k_dense, early (side streams) and late (main stream)
  // prelude -> tail contributions in descendant coordinates (k_outside; fp64 atomics): one launch between the last
  // prelude level and the first tail level
  bool outside_on = false;
  int32_t tail_level = 0;               // level of the first tail front
  std::vector<uint8_t> outside_desc;    // [nsuper] descendant handled by k_outside
  OutsideWork* d_owork = nullptr;
  int32_t* d_grp_next = nullptr;   // [nsuper] k_outside: next descendant with the same tail rows as this one, or -1
  int32_t* d_grp_t0 = nullptr;     // [nsuper] its first tail row
  int64_t n_owork = 0;
  int32_t* d_tail_front = nullptr;
  uint8_t* d_keep_front = nullptr;
  hipStream_t outside_st = nullptr;
  // PROGRESSIVE k_outside: the items are sorted by the FIRST tail panel they touch and cut into chunks; chunk g is one launch
  // and one event, and whatever touches tail panel f (its early / late updates, its potrf) waits only for the last chunk that
  // holds an item reaching f or an earlier panel -- left-looking updates write nothing but the level's own panel, so the rest
  // of the atomic contributions (to LATER panels only) overlaps with the first levels of the tail, which are chain-bound
  std::vector<int64_t> ochunk_ptr;       // [nchunks + 1] into d_owork
  std::vector<hipEvent_t> out_evs;       // [nchunks]
  std::vector<int32_t> out_wait_chunk;   // [nlevels] chunk the level's tail front waits for, -1: none
  bool dense_on = false;
  int front_bits = 64;                  // 32: dense-tail products on the fp32 matrix pipe (k_dense32), sums in fp64
  double* d_zeros = nullptr;            // 2 KiB of zeros: source of the B k-rows past a descendant's end (k_dense_b)
  DenseWork* d_dwork_e = nullptr;
  DenseWork* d_dwork_l = nullptr;
  std::vector<int64_t> dwork_e_ptr, dwork_l_ptr;  // [nlevels+1]
  // distributed tail, look-ahead split of an own target's late update: items [dwork_l_ptr[l], dwork_l_mid[l]) take the sources
  // that arrived EARLIER (they run while the newest source panel is still being factored / broadcast), items
  // [dwork_l_mid[l], dwork_l_ptr[l+1]) the newest source alone (== dwork_l_ptr[l+1] where nothing is split)
  std::vector<int64_t> dwork_l_mid;               // [nlevels]
  int64_t n_late_split = 0;                       // levels of the last factorization whose late launch was split
  int look_depth = 2;      // "late" = descendants at most this many levels below the target; older ones are "early"
  int rhs_pending = -1;            // mode of the last run_rhs whose events have not been read yet
  // dense-chain sweeps (k_chain): the last chain_T levels are single fronts whose mutual update pairs are contiguous
  int32_t chain_T = 0, chain_l0 = 0;
  int32_t* d_chain = nullptr;
  int32_t* d_colmap = nullptr;     // forward: column -> row maps of the non-contiguous chain pairs
  int32_t* d_cf_ptr = nullptr;     // forward: pairs of chain target i (descendants ascending)
  ChainPair* d_cf = nullptr;
  int32_t* d_cb_ptr = nullptr;     // backward: pairs of chain descendant i (targets descending)
  ChainPair* d_cb = nullptr;
  ChainDesc* d_cfd = nullptr;      // flat descriptors of the same pairs, in the same order (the pipelined pair loop)
  ChainDesc* d_cbd = nullptr;
  int64_t chain_desc_bytes = 0;    // ... and what they add to the plan
  int64_t* d_cg_ptr = nullptr;     // backward: pairs (chain target, non-chain descendant) grouped by descendant
  int32_t* d_cg_pairs = nullptr;
  int64_t chain_groups = 0;
  // long groups are cut into row slices that write partial sums; k_push_fold adds them up in fixed order
  int32_t* d_cg_slot = nullptr;      // per work item: partial slot or -1 (subtract straight from X)
  int32_t* d_fold = nullptr;         // triples (descendant, first slot, slices)
  int64_t n_fold = 0;
  double* d_push_partial = nullptr;  // [slots][NB][RPMAX]
  int32_t* d_chain_flags = nullptr;  // [chain_T * RPMAX/CW] epoch stamps
  int32_t* d_chain_err = nullptr;    // [0] error flag, [1] progress beacon, [2] ticket counter of the running sweep
  int32_t* h_chain_err = nullptr;    // pinned mirror of [0], refreshed by a queued copy after every solve
  int32_t chain_epoch = 0;
  std::vector<hipEvent_t> pev;     // profiling: PEV_PER_LEVEL events per level (enum ProfEvent, factorize.hip.h)
  // deterministic mode (scilmm_set_deterministic): pull schedule of the forward sweep / L*R, transposed pattern index
  bool det = false;
  PullPlan pull{};
  int32_t* d_pull_level_segs = nullptr;
  int32_t* d_pull_fold = nullptr;
  double* d_pull_partial = nullptr;     // [pull_max_slots][NB][RPMAX]
  uint8_t* d_chain_mask = nullptr;      // [nsuper] front is swept by k_chain
  const int64_t* d_pat_rowptr = nullptr;
  const int64_t* d_pat_rowslot = nullptr;
  const int32_t* d_pat_rowcol = nullptr;
  int64_t n_float_atomic = 0;           // launches since the handle was created that sum with floating-point atomics
  // marker scan and BLUP blocks: slice partial sums of the statistics; inverse permutation (ensure_iperm: the blocks, IBD and dominance values)
  double* scan_partial = nullptr;       // [slices][q + 1][RPMAX]; after its fold, a gxe block's [slices][pairs][RPMAX]
  size_t scan_partial_cap = 0;          // doubles
  double* gram_partial = nullptr;       // [slices of GRAM_SLICE rows][GRAM_TILES][256]: partial tiles of X^T X (the first Gram block allocates it)
  size_t gram_partial_cap = 0;          // doubles
  const int32_t* d_iperm = nullptr;
  StageTimer scan_t{3, 2};              // block begin | W ready | forward sweep done | statistics done: the last block's moments + dequantise |
                                        // forward sweep | statistics (scilmm_scan_timing); marks 4, 5: a gxe block's fill done | k_scan_fold done
  bool gxe_pending = false;             // the pending scan block is a gxe block
  double gxe_ms[2] = {0.0, 0.0};        // the last block's k_scan_expand (mark 4 to 1) | k_scan_cross + its fold (mark 5 to 3); 0 after a plain
                                        // block (scilmm_gxe_timing)
  // phenotype panels (scilmm_scan_panel_dev): X^T Y for the forward solution the last scan block left in X
  int32_t block_r = 0, block_rp = 0;    // X holds a block of block_r columns padded to block_rp (BlockCall::finish); 0: it does not --
                                        // whatever may overwrite the work buffers or replaces the factor clears the record (clear_block)
  double* panel_partial = nullptr;      // [slices of PANEL_SLICE rows][column panels][tiles][256]: partial tiles of X^T Y
  size_t panel_partial_cap = 0;         // doubles (grown for a wider panel only)
  StageTimer panel_t{2};                // the last call's k_scan_panel | k_panel_fold (scilmm_panel_timing)
  // saddlepoint score scan (scilmm_scan_spa*_dev): the covariate-adjusted marker rows of one block
  double* spa_scratch = nullptr;        // [RPMAX][n] (the first SPA call on the handle allocates it; never reallocated)
  size_t spa_scratch_cap = 0;           // doubles
  StageTimer spa_t{1};                  // the last call's k_scan_spa (scilmm_spa_timing)
  StageTimer fin_t{1};                  // the last call's k_sets_finish (scilmm_sets_finish_timing)
  // the finish of a block's sets against a phenotype panel (scilmm_sets_finish_panel_dev): a record per set (setpanel.hip.h)
  double* pfin_rec = nullptr;           // grown for more or wider sets behind a stream synchronise; nothing is allocated afterwards
  size_t pfin_rec_cap = 0;              // doubles
  int pfin_cu = 0;                      // compute units of the device (the first panel finish asks), for the tail's grid
  StageTimer pfin_t{2};                 // the last call's k_sets_spectra | k_sets_panel_tail (scilmm_sets_finish_panel_timing)
  StageTimer mfin_t{1};                 // the last call's k_sets_finish_masks (scilmm_sets_finish_masks_timing)
  StageTimer sspa_t{1};                 // the last call's k_sets_spa (scilmm_sets_spa_timing)
  // the finish of a wide set (scilmm_sets_finish_wide_dev): the m x m matrix, the vectors and the spectra (WideWs, setwide.hip.h)
  double* wide_ws = nullptr;            // grown for the widest set seen, behind a stream synchronise; nothing is allocated afterwards
  size_t wide_ws_cap = 0;               // doubles
  StageTimer wide_t{4};                 // the last call's prep + form | reduction | eigenvalues | tails (scilmm_sets_finish_wide_timing)
  // the set saddlepoint of a wide set (scilmm_sets_collapse*_dev, scilmm_sets_spa_wide_dev): it cuts wide_ws its own way (SwideWs)
  StageTimer coll_t{1};                 // the last k_sets_collapse: element 0 of scilmm_sets_spa_wide_timing
  StageTimer swide_t{2};                // the last call's markers + pairs | its burden kernel: elements 1 and 2
  void clear_block() { block_r = block_rp = 0; }
  // every stage timer, in the order scilmm_sync reads them (dev_free destroys them): a new call family adds its member here
  static constexpr int N_TIMERS = 10;
  static StageTimer Dev::*const TIMERS[N_TIMERS];
};
inline StageTimer Dev::*const Dev::TIMERS[Dev::N_TIMERS] = {&Dev::scan_t, &Dev::panel_t, &Dev::spa_t,  &Dev::fin_t,  &Dev::mfin_t,
                                                            &Dev::pfin_t, &Dev::wide_t,  &Dev::sspa_t, &Dev::coll_t, &Dev::swide_t};

#define HIPCHK(call)                                                                                   \
  do {                                                                                                 \
    hipError_t _e = (call);                                                                            \
    if (_e != hipSuccess) {                                                                            \
      sym->err = std::string(#call) + ": " + hipGetErrorString(_e);                                    \
      return SCILMM_ERR_DEVICE;                                                                        \
    }                                                                                                  \
  } while (0)

#define TRY(call)                      \
  do {                                 \
    int _rc = (call);                  \
    if (_rc != SCILMM_OK) return _rc;  \
  } while (0)

// Temporary device memory of one call: whatever alloc / upload handed out is freed when the owner goes out of scope, on
// every return path.  A failure is reported as HIPCHK does, to *err: a handle's sym->err, or a message that belongs to no
// handle (dominance.hip).
struct DevScratch {
  std::string* const err;
  std::vector<void*> held;

  explicit DevScratch(std::string* e) : err(e) {}
  DevScratch(const DevScratch&) = delete;
  DevScratch& operator=(const DevScratch&) = delete;
  ~DevScratch() {
    for (void* p : held) (void)hipFree(p);
  }

  int fail(const char* call, hipError_t e) const {
    *err = std::string(call) + ": " + hipGetErrorString(e);
    return SCILMM_ERR_DEVICE;
  }
  // count elements of T (at least 8 bytes, so that an empty array still has an address)
  template <typename T>
  int alloc(size_t count, T** out) {
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, std::max<size_t>(count * sizeof(T), 8));
    if (e != hipSuccess) return fail("hipMalloc", e);
    held.push_back(p);
    *out = (T*)p;
    return SCILMM_OK;
  }
  // ... filled from the host (pageable memory: the copy has left h when this returns)
  template <typename T>
  int upload(const T* h, size_t count, T** out, hipStream_t stream = nullptr) {
    TRY(alloc(count, out));
    const hipError_t e = count ? hipMemcpyAsync(*out, h, count * sizeof(T), hipMemcpyHostToDevice, stream) : hipSuccess;
    return e == hipSuccess ? SCILMM_OK : fail("hipMemcpyAsync", e);
  }
  template <typename T>
  int upload(const std::vector<T>& h, T** out, hipStream_t stream = nullptr) {
    return upload(h.data(), h.size(), out, stream);
  }
};

// Makes the handle's device current for the duration of an entry point and restores the caller's device afterwards
// (a handle may be used from a thread whose current device is a different one).
struct DevGuard {
  int prev = -1;
  bool switched = false;
  explicit DevGuard(const scilmm_symbolic* sym) {
    const Dev* D = sym ? (const Dev*)sym->device : nullptr;
    if (D) enter(D->device);
  }
  explicit DevGuard(int device) { enter(device); }
  void enter(int device) {
    if (device < 0) return;
    if (hipGetDevice(&prev) == hipSuccess && prev != device) switched = hipSetDevice(device) == hipSuccess;
    if (!switched) (void)hipGetLastError();  // never leave a failed hipSetDevice behind as the thread's "last error"
  }
  ~DevGuard() {
    if (switched) (void)hipSetDevice(prev);
  }
};

// (out: a T* or const T* of the device state)
template <typename T, typename P>
int upload(scilmm_symbolic* sym, Dev* D, const std::vector<T>& h, P** out) {
  static_assert(std::is_same<typename std::remove_const<P>::type, T>::value, "upload: pointer type != element type");
  void* p = nullptr;
  size_t bytes = std::max<size_t>(h.size(), 1) * sizeof(T);
  HIPCHK(hipMalloc(&p, bytes));
  D->allocs.push_back(p);
  if (!h.empty()) HIPCHK(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  *out = (P*)p;
  return SCILMM_OK;
}

// Grow-only device buffer of a handle: kept while it holds `need` elements, else replaced by one that does (the old
// contents are dropped).  The caller has made sure that nothing queued still uses the old one.
template <typename T>
int grow(scilmm_symbolic* sym, T** ptr, size_t* cap, size_t need) {
  if (*ptr && *cap >= need) return SCILMM_OK;
  if (*ptr) (void)hipFree(*ptr);
  *ptr = nullptr;
  *cap = 0;
  HIPCHK(hipMalloc((void**)ptr, std::max<size_t>(need, 1) * sizeof(T)));
  *cap = need;
  return SCILMM_OK;
}

// staging for host <-> device dense transfers
inline int ensure_io(scilmm_symbolic* sym, Dev* D, size_t doubles) { return grow(sym, &D->IO, &D->io_cap, doubles); }

// the value array of matrix k: pattern-slot order, or one value per row for a diagonal-only matrix
inline int ensure_vals(scilmm_symbolic* sym, Dev* D, int32_t k) {
  const Symbolic& S = *sym->S;
  if (D->vals[k]) return SCILMM_OK;
  HIPCHK(hipMalloc((void**)&D->vals[k], std::max<size_t>(S.is_diag[k] ? (size_t)S.n : (size_t)S.nnz_pattern, 1) * sizeof(double)));
  return SCILMM_OK;
}

// the inverse permutation (original -> permuted row) on the device: uploaded once per handle
inline int ensure_iperm(scilmm_symbolic* sym, Dev* D) {
  return D->d_iperm ? SCILMM_OK : upload(sym, D, sym->S->iperm, &D->d_iperm);
}

// Rank-local storage of a distributed factor (world > 1).  Tail front dense_first + jj belongs to rank jj % world.
//   [ prelude panels, as in the Symbolic | own tail panels, packed | ring: G slots of the largest tail panel ]
// A panel of another rank lives in slot jj % G from its broadcast until every own target has consumed it: the batch of
// its source group g = jj / Wg (applied when the group is complete) and the late updates of the own targets of groups
// g and g + 1 -- so a slot is free again well before panel jj + G arrives (G = 4 Wg; the level loop still orders the
// re-use with events).  Per rank: nnz(L_tail) / world + G panels instead of the whole factor.
struct DistLayout {
  int32_t first = 0, Wg = 8, G = 32;
  std::vector<int64_t> loff;
  int64_t nL = 0, ring_base = 0, slot = 0;
};

// plan.hip: what engine.hip calls across the boundary
void dev_free(void* p);
void dist_layout(const Symbolic& S, int32_t rank, int32_t world, const Tuning& tune, DistLayout* o);
int ensure_device(scilmm_symbolic* sym, Dev** out);
int ensure_sinv_plan(scilmm_symbolic* sym, Dev* D);

}  // namespace scilmm
