// The numeric C-ABI entry points of include/scilmm_hip.h.  This is the one translation unit of the numeric phase's kernels
// (kernels.hip.h, scan.hip.h, gram.hip.h, panel.hip.h, bed.hip.h, dosage.hip.h, spa.hip.h, setmath.hip.h, setfinish.hip.h, setpanel.hip.h, setmasks.hip.h, setwide.hip.h, setspa.hip.h, setspawide.hip.h, blup.hip.h); the host side behind the entry points is included by feature:
//   launch.hip.h     the typed launchers (FactorLaunch, SweepLaunch, the selected inverse's);
//   factorize.hip.h  Factorization / run_factorize, finish_factorize, ProfRead, settle, the factor's storage;
//   sweep.hip.h      Sweep / run_rhs (solve, L*R, half-solves), host_rhs, finish_rhs_timing;
//   blocks.hip.h     BlockCall, marker_block and the fills of its input forms (int8, .bed, dosage), rel_block, rows_block; PostCall, the
//                    frame of the calls behind a block (scan_panel, scan_keep, scan_spa, sets_finish, sets_finish_panel,
//                    sets_finish_masks, sets_finish_wide, sets_spa, sets_collapse, sets_spa_wide), grow_synced, set_layout;
//   products.hip.h   run_quad, run_spmm and their host forms, the HE moments, fold_blocks;
//   values.hip.h     the A_k values on the device: upload, download, IBD and dominance values;
//   sinv.hip.h       the selected inverse and its traces.
// The device state they run on (struct Dev, dev.h) is built once per handle by plan.hip.  Everything runs on one HIP stream
// per symbolic handle; host entry points synchronise only where they hand data back to the caller.  An entry point is its
// argument checks (before anything is dereferenced), a DevGuard (a block call's sits in its BlockCall or PostCall) and one
// call.  The three marker input forms (Int8Form, BedForm, DosageForm, below) state their checks, fill and reader once for the
// four call families that read markers.  Every call family behind a block times itself with a StageTimer of the device state
// (dev.h): scilmm_sync reads them in one loop, dev_free destroys them in one, and the timing getters are timing_out and a line each.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <functional>
#include <new>
#include <optional>
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
#include "gram.hip.h"
#include "panel.hip.h"
#include "bed.hip.h"
#include "dosage.hip.h"
#include "spa.hip.h"
#include "setfinish.hip.h"
#include "setpanel.hip.h"
#include "setmasks.hip.h"
#include "setwide.hip.h"
#include "setspa.hip.h"
#include "setspawide.hip.h"
#include "blup.hip.h"
#include "dev.h"
#include "host_threads.h"

using namespace scilmm;

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
#include "factorize.hip.h"
#include "sweep.hip.h"
#include "blocks.hip.h"
#include "products.hip.h"
#include "values.hip.h"
#include "sinv.hip.h"

namespace {

// The three input forms of a block of markers: int8 rows, packed PLINK rows, dosage rows of uint16 or float.  Each holds the
// form's arguments; ok(fac, rest) applies the form's checks around the caller's -- what needs no handle, then `rest` (the call
// family's args_ok, which looks at the handle last), then what needs n: with any argument wrong that needs no handle, nothing
// of the handle is read --; fill and reader hand the form's fill (blocks.hip.h) or its row reader (spa.hip.h) to `f`, the
// dosage form whichever of its two element types dtype names.
struct Int8Form {
  const int8_t* d_geno;
  int64_t ld;
  template <class Rest>
  bool ok(const scilmm_factor* fac, Rest rest) const { return d_geno && rest() && ld >= fac->sym->S->n; }
  template <class F>
  int fill(int32_t r, double* d_stats, F f) const { return f(fill_int8(d_geno, ld, r, d_stats)); }
  template <class F>
  int reader(F f) const { return f(SpaInt8{d_geno, ld}); }
};

struct BedForm {
  const uint8_t* d_bed;
  int64_t ld;
  int32_t n_samples;
  const int32_t* d_sample;
  int32_t flags;
  template <class Rest>
  bool ok(const scilmm_factor* fac, Rest rest) const {
    return d_bed && n_samples >= 1 && ld >= ((int64_t)n_samples + 3) / 4 && !(flags & ~BED_A2) && rest() &&
           (d_sample || n_samples == fac->sym->S->n);
  }
  template <class F>
  int fill(int32_t r, double* d_stats, F f) const { return f(fill_bed(d_bed, ld, n_samples, d_sample, flags, r, d_stats)); }
  template <class F>
  int reader(F f) const { return f(SpaBed{d_bed, ld, n_samples, d_sample, flags}); }
};

struct DosageForm {
  const void* d_dos;
  int32_t dtype;
  int64_t ld;
  int32_t n_samples;
  const int32_t* d_sample;
  bool u16() const { return dtype == SCILMM_DOSAGE_U16; }
  template <class Rest>
  bool ok(const scilmm_factor* fac, Rest rest) const {
    return d_dos && (u16() || dtype == SCILMM_DOSAGE_F32) && (uintptr_t)d_dos % (u16() ? sizeof(uint16_t) : sizeof(float)) == 0 &&
           n_samples >= 1 && ld >= n_samples && rest() && (d_sample || n_samples == fac->sym->S->n);
  }
  // (a step per element type: instantiated behind the int8 and .bed blocks, the kernels keep their order in the code object)
  template <class T, class F>
  int fill_as(int32_t r, double* d_stats, F f) const { return f(fill_dosage<T>(d_dos, ld, n_samples, d_sample, r, d_stats)); }
  template <class F>
  int fill(int32_t r, double* d_stats, F f) const { return u16() ? fill_as<uint16_t>(r, d_stats, f) : fill_as<float>(r, d_stats, f); }
  template <class F>
  int reader(F f) const {
    return u16() ? f(SpaDos<uint16_t>{(const uint16_t*)d_dos, ld, n_samples, d_sample}) : f(SpaDos<float>{(const float*)d_dos, ld, n_samples, d_sample});
  }
};

// The four call families that read markers, each for any form: the form's checks around the family's own, one call.  scan_block: `gram`: the entry point (`who`) hands X^T X back as well, to d_gram (null from the others);
// `d_E`, `m`: the gxe entry points' environment columns, which they have checked with r (null from the others).
template <class Form>
int scan_block(scilmm_factor* fac, const Form& g, int32_t r, const double* d_Q, int32_t q, double* d_stats, bool gram, double* d_gram,
               const char* who, const double* d_E = nullptr, int32_t m = 0) {
  if ((gram && !d_gram) || !g.ok(fac, [&] { return BlockCall::args_ok(fac, r, d_Q, q, d_stats); })) return SCILMM_ERR_ARG;
  return g.fill(r, d_stats, [&](auto fill) { return marker_block(fac, who, r, d_Q, q, d_stats, d_gram, fill, d_E, m); });
}

template <class Form>
int spa_call(scilmm_factor* fac, const Form& g, int32_t r, const SpaArgs& a, const char* who) {
  if (!g.ok(fac, [&] { return SpaArgs::args_ok(fac, r, a); })) return SCILMM_ERR_ARG;
  return g.reader([&](auto rd) { return scan_spa(fac, who, r, rd, a); });
}

template <class Form>
int sets_spa_call(scilmm_factor* fac, const Form& g, int32_t r, const SetSpaArgs& a, const char* who) {
  if (!g.ok(fac, [&] { return SetSpaArgs::args_ok(fac, r, a); })) return SCILMM_ERR_ARG;
  return g.reader([&](auto rd) { return sets_spa(fac, who, r, rd, a); });
}

template <class Form>
int collapse_call(scilmm_factor* fac, const Form& g, int32_t r, const CollapseArgs& a, const char* who) {
  if (!g.ok(fac, [&] { return CollapseArgs::args_ok(fac, r, a); })) return SCILMM_ERR_ARG;
  return g.reader([&](auto rd) { return sets_collapse(fac, who, r, rd, a); });
}

}  // namespace

extern "C" {

int scilmm_values_upload(scilmm_symbolic* sym, int32_t k, const double* data_k) {
  if (!sym || !sym->S || !data_k) return SCILMM_ERR_ARG;
  DevGuard guard(sym);
  if (k < 0 || k >= sym->S->K) return SCILMM_ERR_ARG;
  if (sym->maps_released) {
    sym->err = "scilmm_values_upload: the value-assembly maps of this handle were released";
    return SCILMM_ERR_STATE;
  }
  Dev* D;
  TRY(ensure_device(sym, &D));
  return values_upload(sym, D, k, data_k);
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
  TRY(ensure_device(sym, &D));
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

int scilmm_factorize(scilmm_symbolic* sym, const double* sigma2, scilmm_factor** out, int32_t* bad_col) {
  if (!sym || !sym->S || !sigma2 || !out) return SCILMM_ERR_ARG;
  DevGuard guard(sym);
  TRY(factor_create(sym, nullptr, nullptr, nullptr, out));
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
  factor_free(fac);
}

int scilmm_logdet(scilmm_factor* fac, double* out) {
  if (!fac || !fac->sym || !out) return SCILMM_ERR_ARG;
  DevGuard guard(fac->sym);
  TRY(settle(fac, "scilmm_logdet"));
  // the fronts' log-sums, added up in front order
  long double s = 0.0L;
  TRY(fold_blocks(fac->sym, (Dev*)fac->sym->device, fac->logd, 1, (size_t)fac->sym->S->nsuper, &s));
  *out = (double)(2.0L * s);
  return SCILMM_OK;
}

// The sweeps: argument checks before anything is dereferenced, the refusals of a half-solve (`half`: its name), the sweep
// in its host or its device-pointer form.
static int rhs_entry(scilmm_factor* fac, const double* B, int32_t r, double* X, int mode, bool host, const char* half = nullptr) {
  if (!fac || !B || !X || r <= 0 || !fac->sym) return SCILMM_ERR_ARG;
  DevGuard guard(fac->sym);
  if (half) TRY(check_half(fac, half));
  return host ? host_rhs(fac, B, r, X, mode) : run_rhs(fac, B, r, X, mode);
}

int scilmm_solve(scilmm_factor* fac, const double* B, int32_t r, double* X) { return rhs_entry(fac, B, r, X, RHS_SOLVE, true); }
int scilmm_lmul(scilmm_factor* fac, const double* R, int32_t r, double* Z) { return rhs_entry(fac, R, r, Z, RHS_LMUL, true); }
int scilmm_solve_dev(scilmm_factor* fac, const double* dB, int32_t r, double* dX) { return rhs_entry(fac, dB, r, dX, RHS_SOLVE, false); }
int scilmm_lmul_dev(scilmm_factor* fac, const double* dR, int32_t r, double* dZ) { return rhs_entry(fac, dR, r, dZ, RHS_LMUL, false); }
int scilmm_solve_L(scilmm_factor* fac, const double* B, int32_t r, double* X) {
  return rhs_entry(fac, B, r, X, RHS_SOLVE_L, true, "scilmm_solve_L");
}
int scilmm_solve_Lt(scilmm_factor* fac, const double* B, int32_t r, double* X) {
  return rhs_entry(fac, B, r, X, RHS_SOLVE_LT, true, "scilmm_solve_Lt");
}
int scilmm_solve_L_dev(scilmm_factor* fac, const double* dB, int32_t r, double* dX) {
  return rhs_entry(fac, dB, r, dX, RHS_SOLVE_L, false, "scilmm_solve_L_dev");
}
int scilmm_solve_Lt_dev(scilmm_factor* fac, const double* dB, int32_t r, double* dX) {
  return rhs_entry(fac, dB, r, dX, RHS_SOLVE_LT, false, "scilmm_solve_Lt_dev");
}

// The marker scan's blocks: a form of the markers (above the entry points), the family's call
int scilmm_scan_block_dev(scilmm_factor* fac, const int8_t* d_geno, int64_t ld_geno, int32_t r, const double* d_Q, int32_t q,
                          double* d_stats) {
  return scan_block(fac, Int8Form{d_geno, ld_geno}, r, d_Q, q, d_stats, false, nullptr, __func__);
}

int scilmm_scan_block_gram_dev(scilmm_factor* fac, const int8_t* d_geno, int64_t ld_geno, int32_t r, const double* d_Q, int32_t q,
                               double* d_stats, double* d_gram) {
  return scan_block(fac, Int8Form{d_geno, ld_geno}, r, d_Q, q, d_stats, true, d_gram, __func__);
}

int scilmm_scan_block_bed_dev(scilmm_factor* fac, const uint8_t* d_bed, int64_t ld_bed, int32_t n_samples, const int32_t* d_sample,
                              int32_t flags, int32_t r, const double* d_Q, int32_t q, double* d_stats) {
  return scan_block(fac, BedForm{d_bed, ld_bed, n_samples, d_sample, flags}, r, d_Q, q, d_stats, false, nullptr, __func__);
}

int scilmm_scan_block_bed_gram_dev(scilmm_factor* fac, const uint8_t* d_bed, int64_t ld_bed, int32_t n_samples, const int32_t* d_sample,
                                   int32_t flags, int32_t r, const double* d_Q, int32_t q, double* d_stats, double* d_gram) {
  return scan_block(fac, BedForm{d_bed, ld_bed, n_samples, d_sample, flags}, r, d_Q, q, d_stats, true, d_gram, __func__);
}

int scilmm_scan_block_dosage_dev(scilmm_factor* fac, const void* d_dos, int32_t dtype, int64_t ld, int32_t n_samples,
                                 const int32_t* d_sample, int32_t r, const double* d_Q, int32_t q, double* d_stats) {
  return scan_block(fac, DosageForm{d_dos, dtype, ld, n_samples, d_sample}, r, d_Q, q, d_stats, false, nullptr, __func__);
}

int scilmm_scan_block_dosage_gram_dev(scilmm_factor* fac, const void* d_dos, int32_t dtype, int64_t ld, int32_t n_samples,
                                      const int32_t* d_sample, int32_t r, const double* d_Q, int32_t q, double* d_stats, double* d_gram) {
  return scan_block(fac, DosageForm{d_dos, dtype, ld, n_samples, d_sample}, r, d_Q, q, d_stats, true, d_gram, __func__);
}

int scilmm_scan_block_gxe_dev(scilmm_factor* fac, const int8_t* d_geno, int64_t ld_geno, int32_t r, const double* d_E, int32_t m,
                              const double* d_Q, int32_t q, double* d_stats) {
  if (!Gxe::args_ok(d_E, m, r)) return SCILMM_ERR_ARG;
  return scan_block(fac, Int8Form{d_geno, ld_geno}, r, d_Q, q, d_stats, false, nullptr, __func__, d_E, m);
}

int scilmm_scan_block_bed_gxe_dev(scilmm_factor* fac, const uint8_t* d_bed, int64_t ld_bed, int32_t n_samples, const int32_t* d_sample,
                                  int32_t flags, int32_t r, const double* d_E, int32_t m, const double* d_Q, int32_t q, double* d_stats) {
  if (!Gxe::args_ok(d_E, m, r)) return SCILMM_ERR_ARG;
  return scan_block(fac, BedForm{d_bed, ld_bed, n_samples, d_sample, flags}, r, d_Q, q, d_stats, false, nullptr, __func__, d_E, m);
}

int scilmm_scan_block_dosage_gxe_dev(scilmm_factor* fac, const void* d_dos, int32_t dtype, int64_t ld, int32_t n_samples,
                                     const int32_t* d_sample, int32_t r, const double* d_E, int32_t m, const double* d_Q, int32_t q,
                                     double* d_stats) {
  if (!Gxe::args_ok(d_E, m, r)) return SCILMM_ERR_ARG;
  return scan_block(fac, DosageForm{d_dos, dtype, ld, n_samples, d_sample}, r, d_Q, q, d_stats, false, nullptr, __func__, d_E, m);
}

// X^T Y for the block the last scan block left behind and a resident phenotype panel: what needs no handle is checked first
int scilmm_scan_panel_dev(scilmm_factor* fac, int32_t r, const double* d_Y, int64_t ld_y, int32_t t, double* d_xty, int64_t ld_out) {
  if (!fac || !d_Y || !d_xty || r < 1 || r > RPMAX || t < 1 || t > PANEL_TMAX || ld_y < t || ld_y % 16 != 0 || ld_out < t ||
      (uintptr_t)d_Y % 16 != 0 || !fac->sym || !fac->sym->S)
    return SCILMM_ERR_ARG;
  return scan_panel(fac, r, d_Y, ld_y, t, d_xty, ld_out);
}

// The block the last scan block left behind, kept in a caller's store: what needs no handle is checked first
int scilmm_scan_block_keep_dev(scilmm_factor* fac, int32_t r, double* d_dst, int64_t ld_dst, int64_t col0) {
  if (!fac || !d_dst || r < 1 || r > RPMAX || col0 < 0 || col0 % 16 != 0 || ld_dst % 16 != 0) return SCILMM_ERR_ARG;
  const int64_t rp = (r + 15) / 16 * 16;
  if (ld_dst < rp || ld_dst - rp < col0 || (uintptr_t)d_dst % 16 != 0 || !fac->sym || !fac->sym->S) return SCILMM_ERR_ARG;
  return scan_keep(fac, r, d_dst, ld_dst, col0);
}

// The saddlepoint p-values behind a plain block: the form's marker arguments are checked as its plain entry point checks them
int scilmm_scan_spa_dev(scilmm_factor* fac, const int8_t* d_geno, int64_t ld_geno, int32_t r, const double* d_stats, const double* d_R,
                        const double* d_u, const double* d_mu, const double* d_C, int32_t c, const double* d_Minv, double cutoff,
                        double* d_spa) {
  const SpaArgs a{d_stats, d_R, d_u, d_mu, d_C, c, d_Minv, cutoff, d_spa};
  return spa_call(fac, Int8Form{d_geno, ld_geno}, r, a, __func__);
}

int scilmm_scan_spa_bed_dev(scilmm_factor* fac, const uint8_t* d_bed, int64_t ld_bed, int32_t n_samples, const int32_t* d_sample,
                            int32_t flags, int32_t r, const double* d_stats, const double* d_R, const double* d_u, const double* d_mu,
                            const double* d_C, int32_t c, const double* d_Minv, double cutoff, double* d_spa) {
  const SpaArgs a{d_stats, d_R, d_u, d_mu, d_C, c, d_Minv, cutoff, d_spa};
  return spa_call(fac, BedForm{d_bed, ld_bed, n_samples, d_sample, flags}, r, a, __func__);
}

int scilmm_scan_spa_dosage_dev(scilmm_factor* fac, const void* d_dos, int32_t dtype, int64_t ld, int32_t n_samples,
                               const int32_t* d_sample, int32_t r, const double* d_stats, const double* d_R, const double* d_u,
                               const double* d_mu, const double* d_C, int32_t c, const double* d_Minv, double cutoff, double* d_spa) {
  const SpaArgs a{d_stats, d_R, d_u, d_mu, d_C, c, d_Minv, cutoff, d_spa};
  return spa_call(fac, DosageForm{d_dos, dtype, ld, n_samples, d_sample}, r, a, __func__);
}

// The variant-set finish behind a Gram block: a pure function of what the block left behind
int scilmm_sets_finish_dev(scilmm_factor* fac, int32_t r, int32_t q, const double* d_stats, const double* d_gram, const double* d_R,
                           const double* d_u, int32_t c, int32_t n_sets, const int32_t* set_start, int32_t weight_mode,
                           const double* d_weights, int32_t method, const double* rho, int32_t n_rho, double* d_out, int64_t ld_out,
                           double* d_lam) {
  const FinishArgs a{r, q, d_stats, d_gram, d_R, d_u, c, n_sets, set_start, weight_mode, d_weights, method, rho, n_rho, d_out, ld_out, d_lam};
  if (!FinishArgs::args_ok(fac, a)) return SCILMM_ERR_ARG;
  return sets_finish(fac, a, __func__);
}

// ... with the variance scales of the block's columns (scilmm_sets_spa*_dev) in the weights of A
int scilmm_sets_finish_scaled_dev(scilmm_factor* fac, int32_t r, int32_t q, const double* d_stats, const double* d_gram,
                                  const double* d_R, const double* d_u, int32_t c, int32_t n_sets, const int32_t* set_start,
                                  int32_t weight_mode, const double* d_weights, int32_t method, const double* rho, int32_t n_rho,
                                  double* d_out, int64_t ld_out, double* d_lam, const double* d_vscale) {
  const FinishArgs a{r, q, d_stats, d_gram, d_R, d_u, c, n_sets, set_start, weight_mode, d_weights, method, rho, n_rho, d_out, ld_out, d_lam,
                     d_vscale};
  if (!d_vscale || !FinishArgs::args_ok(fac, a)) return SCILMM_ERR_ARG;
  return sets_finish(fac, a, __func__);
}

// The variant-set finish of a Gram block against the traits of a panel, behind the block and its scilmm_scan_panel_dev
int scilmm_sets_finish_panel_dev(scilmm_factor* fac, int32_t r, int32_t q, const double* d_stats, const double* d_gram, const double* d_R,
                                 int32_t c, int32_t n_sets, const int32_t* set_start, int32_t weight_mode, const double* d_weights,
                                 int32_t method, const double* rho, int32_t n_rho, const double* d_xty, int64_t ld_xty, int32_t t,
                                 const double* d_tscale, double* d_head, double* d_out) {
  // (there is no u and one fixed row layout: what FinishArgs checks of them is given what passes)
  const FinishArgs f{r, q, d_stats, d_gram, d_R, d_R, c, n_sets, set_start, weight_mode, d_weights, method, rho, n_rho, d_out,
                     FIN_HEAD + FIN_RHO_MAX, nullptr};
  const PanelFinishArgs a{f, d_xty, ld_xty, t, d_tscale, d_head, d_out};
  if (!PanelFinishArgs::args_ok(fac, a)) return SCILMM_ERR_ARG;
  return sets_finish_panel(fac, a, __func__);
}

// The variant-set finish of a Gram block under annotation masks and MAF cutoffs: a cell per (set, annotation, cutoff), with ACAT-V
int scilmm_sets_finish_masks_dev(scilmm_factor* fac, int32_t r, int32_t q, const double* d_stats, const double* d_gram, const double* d_R,
                                 const double* d_u, int32_t c, int32_t n_sets, const int32_t* set_start, int32_t weight_mode,
                                 const double* d_weights, int32_t method, const double* rho, int32_t n_rho, const uint32_t* d_ann,
                                 int32_t n_ann, const double* maf_cut, int32_t n_cut, double acat_mac, double* d_out, int64_t ld_out) {
  const FinishArgs f{r, q, d_stats, d_gram, d_R, d_u, c, n_sets, set_start, weight_mode, d_weights, method, rho, n_rho, d_out, ld_out, nullptr};
  const MasksFinishArgs a{f, d_ann, n_ann, maf_cut, n_cut, acat_mac};
  if (!MasksFinishArgs::args_ok(fac, a)) return SCILMM_ERR_ARG;
  return sets_finish_masks(fac, a, __func__);
}

// The finish of ONE set of up to 4 096 markers behind its sub-blocks: a pure function of what they left behind
int scilmm_sets_finish_wide_dev(scilmm_factor* fac, int32_t k, int32_t block, int32_t q, const double* d_stats, const double* d_gram,
                                const double* d_cross, int64_t ld_cross, const double* d_R, const double* d_u, int32_t c,
                                int32_t weight_mode, const double* d_weights, int32_t method, const double* rho, int32_t n_rho,
                                double* d_out, double* d_lam) {
  const WideArgs a{k, block, q, d_stats, d_gram, d_cross, ld_cross, d_R, d_u, c, weight_mode, d_weights, method, rho, n_rho, d_out, d_lam};
  if (!WideArgs::args_ok(fac, a)) return SCILMM_ERR_ARG;
  return sets_finish_wide(fac, a, __func__);
}

// ... with the variance scales of the set's markers (scilmm_sets_spa_wide_dev) in the weights of A
int scilmm_sets_finish_wide_scaled_dev(scilmm_factor* fac, int32_t k, int32_t block, int32_t q, const double* d_stats, const double* d_gram,
                                       const double* d_cross, int64_t ld_cross, const double* d_R, const double* d_u, int32_t c,
                                       int32_t weight_mode, const double* d_weights, int32_t method, const double* rho, int32_t n_rho,
                                       double* d_out, double* d_lam, const double* d_vscale) {
  const WideArgs a{k, block, q, d_stats, d_gram, d_cross, ld_cross, d_R, d_u, c, weight_mode, d_weights, method, rho, n_rho, d_out, d_lam,
                   d_vscale};
  if (!d_vscale || !WideArgs::args_ok(fac, a)) return SCILMM_ERR_ARG;
  return sets_finish_wide(fac, a, __func__);
}

// The collapsed genotype of a wide set behind a sub-block's Gram entry point: the form's marker arguments are checked as its
// scan_spa twin checks them
int scilmm_sets_collapse_dev(scilmm_factor* fac, const int8_t* d_geno, int64_t ld_geno, int32_t r, const double* d_stats,
                             int32_t weight_mode, const double* d_weights, int32_t first, double* d_gB) {
  const CollapseArgs a{d_stats, weight_mode, d_weights, first, d_gB};
  return collapse_call(fac, Int8Form{d_geno, ld_geno}, r, a, __func__);
}

int scilmm_sets_collapse_bed_dev(scilmm_factor* fac, const uint8_t* d_bed, int64_t ld_bed, int32_t n_samples, const int32_t* d_sample,
                                 int32_t flags, int32_t r, const double* d_stats, int32_t weight_mode, const double* d_weights,
                                 int32_t first, double* d_gB) {
  const CollapseArgs a{d_stats, weight_mode, d_weights, first, d_gB};
  return collapse_call(fac, BedForm{d_bed, ld_bed, n_samples, d_sample, flags}, r, a, __func__);
}

int scilmm_sets_collapse_dosage_dev(scilmm_factor* fac, const void* d_dos, int32_t dtype, int64_t ld, int32_t n_samples,
                                    const int32_t* d_sample, int32_t r, const double* d_stats, int32_t weight_mode,
                                    const double* d_weights, int32_t first, double* d_gB) {
  const CollapseArgs a{d_stats, weight_mode, d_weights, first, d_gB};
  return collapse_call(fac, DosageForm{d_dos, dtype, ld, n_samples, d_sample}, r, a, __func__);
}

// The variance scales and the burden saddlepoint of ONE wide set behind its last sub-block: it reads no genotypes, so there is one
int scilmm_sets_spa_wide_dev(scilmm_factor* fac, int32_t k, int32_t block, int32_t q, const double* d_stats, const double* d_gram,
                             const double* d_cross, int64_t ld_cross, const double* d_R, const double* d_u, const double* d_mu,
                             const double* d_C, int32_t c, const double* d_Minv, double cutoff, const double* d_spa, int32_t weight_mode,
                             const double* d_weights, double* d_gB, double* d_bspa, double* d_vscale) {
  const SpaWideArgs a{k, block, q, d_stats, d_gram, d_cross, ld_cross, d_R, d_u, d_mu, d_C, c, d_Minv, cutoff, d_spa, weight_mode, d_weights,
                      d_gB, d_bspa, d_vscale};
  if (!SpaWideArgs::args_ok(fac, a)) return SCILMM_ERR_ARG;
  return sets_spa_wide(fac, a, __func__);
}

// The sets' variance scales and burden saddlepoint p-values behind a Gram block and its markers' saddlepoint call: the form's
// marker arguments are checked as its scan_spa twin checks them
int scilmm_sets_spa_dev(scilmm_factor* fac, const int8_t* d_geno, int64_t ld_geno, int32_t r, const double* d_stats, const double* d_gram,
                        const double* d_R, const double* d_u, const double* d_mu, const double* d_C, int32_t c, const double* d_Minv,
                        double cutoff, const double* d_spa, int32_t n_sets, const int32_t* set_start, int32_t weight_mode,
                        const double* d_weights, double* d_bspa, double* d_vscale) {
  const SetSpaArgs a{{d_stats, d_R, d_u, d_mu, d_C, c, d_Minv, cutoff, const_cast<double*>(d_spa)}, d_gram, n_sets, set_start, weight_mode,
                     d_weights, d_bspa, d_vscale};
  return sets_spa_call(fac, Int8Form{d_geno, ld_geno}, r, a, __func__);
}

int scilmm_sets_spa_bed_dev(scilmm_factor* fac, const uint8_t* d_bed, int64_t ld_bed, int32_t n_samples, const int32_t* d_sample,
                            int32_t flags, int32_t r, const double* d_stats, const double* d_gram, const double* d_R, const double* d_u,
                            const double* d_mu, const double* d_C, int32_t c, const double* d_Minv, double cutoff, const double* d_spa,
                            int32_t n_sets, const int32_t* set_start, int32_t weight_mode, const double* d_weights, double* d_bspa,
                            double* d_vscale) {
  const SetSpaArgs a{{d_stats, d_R, d_u, d_mu, d_C, c, d_Minv, cutoff, const_cast<double*>(d_spa)}, d_gram, n_sets, set_start, weight_mode,
                     d_weights, d_bspa, d_vscale};
  return sets_spa_call(fac, BedForm{d_bed, ld_bed, n_samples, d_sample, flags}, r, a, __func__);
}

int scilmm_sets_spa_dosage_dev(scilmm_factor* fac, const void* d_dos, int32_t dtype, int64_t ld, int32_t n_samples,
                               const int32_t* d_sample, int32_t r, const double* d_stats, const double* d_gram, const double* d_R,
                               const double* d_u, const double* d_mu, const double* d_C, int32_t c, const double* d_Minv, double cutoff,
                               const double* d_spa, int32_t n_sets, const int32_t* set_start, int32_t weight_mode,
                               const double* d_weights, double* d_bspa, double* d_vscale) {
  const SetSpaArgs a{{d_stats, d_R, d_u, d_mu, d_C, c, d_Minv, cutoff, const_cast<double*>(d_spa)}, d_gram, n_sets, set_start, weight_mode,
                     d_weights, d_bspa, d_vscale};
  return sets_spa_call(fac, DosageForm{d_dos, dtype, ld, n_samples, d_sample}, r, a, __func__);
}

int scilmm_rel_block_dev(scilmm_factor* fac, const double* weights, const int32_t* ids, int32_t r, const double* d_Q, int32_t q,
                         double* d_stats) {
  if (!weights || !ids || !BlockCall::args_ok(fac, r, d_Q, q, d_stats)) return SCILMM_ERR_ARG;
  return rel_block(fac, weights, ids, r, d_Q, q, d_stats);
}

int scilmm_rows_block_dev(scilmm_factor* fac, const int64_t* d_indptr, const int32_t* d_indices, const double* d_data, int32_t r,
                          const double* d_Q, int32_t q, double* d_stats) {
  if (!d_indptr || !d_indices || !d_data || !BlockCall::args_ok(fac, r, d_Q, q, d_stats)) return SCILMM_ERR_ARG;
  return rows_block(fac, d_indptr, d_indices, d_data, r, d_Q, q, d_stats);
}

int scilmm_quadforms_dev(scilmm_symbolic* sym, int32_t k, const double* dU, int32_t r, double* d_out) {
  if (!sym || !sym->S || !dU || !d_out || r <= 0) return SCILMM_ERR_ARG;
  DevGuard guard(sym);
  Dev* D;
  TRY(ensure_device(sym, &D));
  const int st = run_quad(sym, D, k, dU, r, d_out);
  D->quad_pending = st == SCILMM_OK;  // (asynchronous: scilmm_last_timing reads the events once they have happened)
  return st;
}

int scilmm_quadforms(scilmm_symbolic* sym, int32_t k, const double* U, int32_t r, double* out) {
  if (!sym || !sym->S || !U || !out || r <= 0) return SCILMM_ERR_ARG;
  DevGuard guard(sym);
  Dev* D;
  TRY(ensure_device(sym, &D));
  return quad_host(sym, D, k, U, r, out);
}

int scilmm_he_moments(scilmm_symbolic* sym, int32_t k1, int32_t k2, double* frob, double* diag_dot) {
  if (!sym || !sym->S || !frob || !diag_dot) return SCILMM_ERR_ARG;
  DevGuard guard(sym);
  Dev* D;
  TRY(ensure_device(sym, &D));
  if (!resident(sym, D, k1) || !resident(sym, D, k2)) return SCILMM_ERR_STATE;
  return he_moments(sym, D, k1, k2, frob, diag_dot);
}

int scilmm_spmm(scilmm_symbolic* sym, int32_t k, const double* X, int32_t r, double* Y) {
  if (!sym || !sym->S || !X || !Y || r <= 0) return SCILMM_ERR_ARG;
  DevGuard guard(sym);
  Dev* D;
  TRY(ensure_device(sym, &D));
  if (!resident(sym, D, k)) return SCILMM_ERR_STATE;
  return spmm_host(sym, D, k, X, r, Y);
}

// device-pointer form of scilmm_spmm (same [n][r] layout): asynchronous on the engine's stream, like the other _dev calls
int scilmm_spmm_dev(scilmm_symbolic* sym, int32_t k, const double* dX, int32_t r, double* dY) {
  if (!sym || !sym->S || !dX || !dY || r <= 0) return SCILMM_ERR_ARG;
  DevGuard guard(sym);
  Dev* D;
  TRY(ensure_device(sym, &D));
  if (!resident(sym, D, k)) return SCILMM_ERR_STATE;
  return run_spmm(sym, D, k, dX, r, dY);
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
  TRY(settle(fac, "scilmm_export_L", true));  // (after scilmm_selected_inverse: the entries of Z on L's pattern)
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
  return ibd_values(sym, k, parents);
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
  TRY(ensure_device(sym, &D));
  if (!D->have_vals[k_src]) {
    sym->err = "scilmm_dominance_values_device: the values of the source matrix are not resident";
    return SCILMM_ERR_STATE;
  }
  return dominance_values(sym, D, k_dst, k_src, parents);
}

int scilmm_values_download(scilmm_symbolic* sym, int32_t k, double* slots_out) {
  if (!sym || !sym->S || !sym->device || !slots_out) return SCILMM_ERR_ARG;
  DevGuard guard(sym);
  Dev* D = (Dev*)sym->device;
  if (!resident(sym, D, k)) return SCILMM_ERR_STATE;
  return values_download(sym, D, k, slots_out);
}

int scilmm_selected_inverse(scilmm_factor* fac) {
  if (!fac || !fac->sym) return SCILMM_ERR_ARG;
  DevGuard guard(fac->sym);
  return selected_inverse(fac);
}

int scilmm_inverse_traces(scilmm_factor* fac, double* out) {
  if (!fac || !fac->sym || !out) return SCILMM_ERR_ARG;
  DevGuard guard(fac->sym);
  if (!fac->inverted) {
    fac->sym->err = "scilmm_inverse_traces: call scilmm_selected_inverse first";
    return SCILMM_ERR_STATE;
  }
  return inverse_traces(fac, out);
}

int scilmm_inverse_pattern_dev(scilmm_factor* fac, double alpha, const double* d_s, double beta, const double* d_T, int32_t c,
                               double* d_diag, double* d_off) {
  if (!fac || c < 0 || c > 32 || (!d_diag && !d_off)) return SCILMM_ERR_ARG;  // (before anything is dereferenced)
  if (!fac->sym || !fac->sym->S) return SCILMM_ERR_ARG;
  DevGuard guard(fac->sym);
  if (!fac->inverted || !fac->sym->device) {
    fac->sym->err = "scilmm_inverse_pattern_dev: call scilmm_selected_inverse first";
    return SCILMM_ERR_STATE;
  }
  return inverse_pattern(fac, alpha, d_s, beta, d_T, c, d_diag, d_off);
}

int scilmm_sync(scilmm_symbolic* sym) {
  if (!sym || !sym->device) return SCILMM_ERR_ARG;
  DevGuard guard(sym);
  Dev* D = (Dev*)sym->device;
  HIPCHK(hipStreamSynchronize(D->stream));
  for (auto t : Dev::TIMERS) {
    StageTimer& timer = D->*t;
    const bool block = timer.pending && t == &Dev::scan_t;
    HIPCHK(timer.read());
    if (!block) continue;
    // the one irregular reader: a gxe block's two intervals end at marks of the block itself
    D->gxe_ms[0] = D->gxe_ms[1] = 0.0;
    if (D->gxe_pending) {
      HIPCHK(timer.between(4, 1, &D->gxe_ms[0]));
      HIPCHK(timer.between(5, 3, &D->gxe_ms[1]));
    }
    // (the queued copy behind the block's sweep has arrived)
    if (D->h_chain_err && *D->h_chain_err != 0) return report_chain_timeout(sym, D, " (scan block)");
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

// The per-family timing getters: n figures from where `src` finds them in the device state
using TimingSrc = const double* (*)(const Dev&);
static int timing_out(const scilmm_symbolic* sym, double* ms, int n, TimingSrc src) {
  if (!sym || !sym->device || !ms) return SCILMM_ERR_ARG;
  const double* from = src(*(const Dev*)sym->device);
  for (int i = 0; i < n; ++i) ms[i] = from[i];
  return SCILMM_OK;
}

int scilmm_scan_timing(const scilmm_symbolic* sym, double* ms) {
  return timing_out(sym, ms, 3, [](const Dev& D) -> const double* { return D.scan_t.ms; });
}
int scilmm_gxe_timing(const scilmm_symbolic* sym, double* ms) {
  return timing_out(sym, ms, 2, [](const Dev& D) -> const double* { return D.gxe_ms; });
}
int scilmm_panel_timing(const scilmm_symbolic* sym, double* ms) {
  return timing_out(sym, ms, 2, [](const Dev& D) -> const double* { return D.panel_t.ms; });
}
int scilmm_spa_timing(const scilmm_symbolic* sym, double* ms) {
  return timing_out(sym, ms, 1, [](const Dev& D) -> const double* { return D.spa_t.ms; });
}
int scilmm_sets_finish_timing(const scilmm_symbolic* sym, double* ms) {
  return timing_out(sym, ms, 1, [](const Dev& D) -> const double* { return D.fin_t.ms; });
}
int scilmm_sets_finish_panel_timing(const scilmm_symbolic* sym, double* ms) {
  return timing_out(sym, ms, 2, [](const Dev& D) -> const double* { return D.pfin_t.ms; });
}
int scilmm_sets_finish_masks_timing(const scilmm_symbolic* sym, double* ms) {
  return timing_out(sym, ms, 1, [](const Dev& D) -> const double* { return D.mfin_t.ms; });
}
int scilmm_sets_finish_wide_timing(const scilmm_symbolic* sym, double* ms) {
  return timing_out(sym, ms, 4, [](const Dev& D) -> const double* { return D.wide_t.ms; });
}
int scilmm_sets_spa_timing(const scilmm_symbolic* sym, double* ms) {
  return timing_out(sym, ms, 1, [](const Dev& D) -> const double* { return D.sspa_t.ms; });
}
// the last collapse, then the two intervals of the last wide set saddlepoint
int scilmm_sets_spa_wide_timing(const scilmm_symbolic* sym, double* ms) {
  const int rc = timing_out(sym, ms, 1, [](const Dev& D) -> const double* { return D.coll_t.ms; });
  return rc != SCILMM_OK ? rc : timing_out(sym, ms + 1, 2, [](const Dev& D) -> const double* { return D.swide_t.ms; });
}

int scilmm_set_front_precision(scilmm_symbolic* sym, int32_t bits) {
  if (!sym || !sym->S || (bits != 32 && bits != 64)) return SCILMM_ERR_ARG;
  DevGuard guard(sym);
  Dev* D;
  TRY(ensure_device(sym, &D));
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
  TRY(ensure_device(sym, &D));
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
