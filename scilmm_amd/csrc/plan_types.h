// Plain structs and constants shared by the kernels (kernels.hip.h) and the host code that builds their plans
// (plan.hip): what a kernel takes as an argument or reads from a device array.  No device code in here.
#pragma once
#include <stdint.h>
#ifndef SCILMM_KC
#define SCILMM_KC 16
#endif
#ifndef SCILMM_NB
#define SCILMM_NB 128
#endif
#ifndef SCILMM_CW
#define SCILMM_CW 32
#endif

namespace scilmm {

constexpr int NB = SCILMM_NB; // max supernode block width (symbolic max_width must be <= NB)
constexpr int TM = 128;       // target rows per tile
constexpr int KC = SCILMM_KC;  // k-chunk of the update kernel: 2 buffers x 16 x (144 + 144) doubles = 74 KB -> two workgroups per CU
constexpr int RPMAX = 128;    // max padded RHS columns per pass
constexpr int CW = SCILMM_CW;  // RHS columns per workgroup

struct DevSym {
  int32_t n, nsuper;
  const int32_t* sn_start;
  const int64_t* sn_rowptr;
  const int32_t* sn_rows;
  const int64_t* sn_loff;
  const int64_t* inv_off;
  const int32_t* upd_src;
  const int32_t* upd_p0;
  const int32_t* upd_p1;
  const int32_t* tile_front;
  const int64_t* tile_base;
  const int64_t* asm_dst;
  const int64_t* diag_dst;
  const int64_t* pat_colptr;
  const int32_t* pat_row;
  const int32_t* perm;
};

struct ValPtrs {
  const double* v[8];
  double s2[8];
  int32_t count;
};

// k_update2 (a work item is (tile, combo range [cb,ce), slot)): one descendant's contribution to one target tile
struct ComboDesc {
  int64_t loff;     // L offset of the descendant panel
  int64_t rowoff;   // offset of its row list in sn_rows
  int32_t md, wd;   // panel rows (leading dimension) and width (K extent)
  int32_t ta, nt;   // descendant rows [ta, ta+nt) land in this tile
  int32_t p0, nq;   // descendant rows [p0, p0+nq) are the target's columns
  int32_t ip0;      // >= 0: rows land at consecutive tile positions ip0..; -1: look each one up
  int32_t jp0;      // >= 0: columns land at consecutive target columns jp0..; -1: look each one up
  int32_t ilo, ihi; // first / last tile position touched (rows are sorted, so everything lies in between)
  int32_t jlo, jhi; // first / last target column touched
};

struct UpdWork {
  int32_t tile;
  int32_t slot;     // partial-slot index or -1
  int64_t cb, ce;   // combo range
};

// k_dense_b / k_dense32 / k_dense_h
struct DenseWork {
  int32_t front;       // target front j (>= dense_first)
  int32_t ti0;         // first of the (one or two) target tiles
  int32_t ntiles;      // 1 or 2
  int32_t k0, k1;      // descendants dense_first + k0 .. dense_first + k1 - 1
  int32_t slot0, slot1;  // partial slab of each tile, or -1: subtract straight from the panel
  int32_t pad;
};

// k_outside
struct OutsideWork {
  int32_t d;        // descendant front (below the dense tail)
  int32_t t0;       // first row of its panel that lies in the tail
  int32_t bi, bj;   // 128-row blocks of those rows: target rows / target columns
};

struct CellSrc { int64_t st, sq; int32_t md, wd; };

// k_fwd_pull (pull schedule of the forward sweep and of L*R)
struct PullPlan {
  const int32_t* seg_front;
  const int64_t* seg_ptr;
  const int32_t* seg_slot;
  const int32_t* front_seg;
};

// k_chain
struct ChainPair {
  int32_t other;  // chain position of the other block (descendant j forward, target t backward)
  int32_t p0, nq; // rows [p0, p0+nq) of the descendant panel ...
  int32_t jp0;    // ... are columns jp0.. of the target block when >= 0 (contiguous: every pair of a dense chain)
  int32_t map;    // jp0 < 0, forward: offset into the column -> row map (NB entries, -1 = no such row)
};

// k_chain, pipelined pair loop: everything about a pair that the kernel otherwise derives by chasing chain[] and the symbolic
// arrays, in one aligned record (two scalar loads), in the order of the ChainPair list beside it
struct alignas(32) ChainDesc {
  int64_t loff;   // element offset of the fragment's first entry: sn_loff[descendant] + p0
  int32_t ld;     // leading dimension of the descendant panel (rows)
  int32_t depth;  // depth of the product: width of the descendant (forward), nq (backward)
  int32_t xrow;   // first x row: first column of the descendant (forward), of the target + jp0 (backward, jp0 >= 0)
  int32_t other;  // as ChainPair::other
  int32_t map;    // jp0 < 0: forward, offset into the column -> row map; backward, p0 (the x rows are sn_rows[rowptr + p0 + k])
  int16_t jp0, nq;  // as ChainPair
};
static_assert(sizeof(ChainDesc) == 32, "ChainDesc: one 32-byte record per pair");

// selected inverse
struct SinvOwner {  // where the entries Z(., lo) with lo in one front live
  int64_t loff;       // panel offset
  const int32_t* rows;  // row list of the front (prelude fronts: searched)
  int32_t c0, m;      // first column, panel rows
  int32_t tail;       // rows = c0 .. n-1: position by arithmetic
};

// k_sinv_tail
struct SinvWork {
  int32_t front;   // tail front s
  int32_t q;       // rows [256 q, 256 q + 256) of R
  int32_t ka, kb;  // source fronts [ka, kb) (absolute front ids, all > s)
};

// deterministic mode: doubles per slot of k_sinv_tail<true> for a front of ncb = ceil(w / 16) column tiles, [wave 8][jb < ncb]
// [ib 2][reg 4][lane 64] (a launch is one front: its slots are of one size), and of k_sinv_cc_ordered, whose launches mix
// fronts of every width: [wave 4][jb NB / 16][ib 2][reg 4][lane 64]
constexpr int64_t sinv_tail_slot(int ncb) { return (int64_t)8 * ncb * 512; }
constexpr int64_t SINV_CC_SLOT = (int64_t)4 * (NB / 16) * 512;

// k_sinv_cc_ordered / k_sinv_cc_fold (deterministic mode)
struct SinvSeg {
  int32_t front;
  int32_t t0, nt;  // 128-row tiles [t0, t0 + nt) of the front's panel; the first one holds rows of R
  int32_t slot;    // partial slot of the level, or -1: the front's only segment
};
struct SinvFold {
  int32_t front;
  int32_t slot0, nseg;  // the front's slots [slot0, slot0 + nseg), in segment (= row) order
};

}  // namespace scilmm
