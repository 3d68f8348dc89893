// The block calls on a resident factor (included by engine.hip only, behind sweep.hip.h; the entry points' argument checks
// stay there): BlockCall, marker_block for the marker scan's input forms and their fills (with environment columns: the gxe
// blocks), rel_block and rows_block for the BLUP; PostCall, the frame of every call that runs behind a block (the panel, the
// keep, the saddlepoints, the set finishes, the collapse), with grow_synced for the handle's buffers such a call grows and
// set_layout for what the finishes of a block's sets derive from the offsets.  Every call family times itself with its
// StageTimer of the device state (dev.h): start, mark .., close; scilmm_sync reads them.
#pragma once

namespace {

// A grow-only buffer of the handle that something queued may still read: the stream is synchronised first, and only where
// the buffer has to grow.
template <typename T>
int grow_synced(scilmm_symbolic* sym, Dev* D, T** ptr, size_t* cap, size_t need) {
  if (*cap < need) HIPCHK(hipStreamSynchronize(D->stream));
  return grow(sym, ptr, cap, need);
}

// What makes a marker block a marker x environment block: m environment columns d_E (n x m row-major, PERMUTED order), r markers
// of d = 1 + m terms each (column a r + c of the block = term a of marker c), the cross products' rows of the statistics.
struct Gxe {
  const double* d_E;
  int32_t m, r;
  double* d_cross;
  int32_t pairs() const { return (m + 1) * m / 2; }
  // before anything of the handle is read
  static bool args_ok(const double* d_E, int32_t m, int32_t r) { return d_E && m >= 1 && m <= GXE_MMAX && r >= 1 && r <= RPMAX / (1 + m); }
};

using CrossKernel = void (*)(int32_t, int32_t, int32_t, const double*, double*);
CrossKernel cross_kernel(int32_t d, int32_t r) {
  if (r <= 32) return d == 2 ? k_scan_cross<2, 32> : d == 3 ? k_scan_cross<3, 32> : k_scan_cross<4, 32>;
  return d == 2 ? k_scan_cross<2, 64> : k_scan_cross<3, 64>;  // (d = 4: r <= 32)
}

// One block of statistics (marker scan, relationship columns, caller rows).  The entry point checks its own arguments
// beside args_ok, then: begin (the refusals and the one-off allocations), its own checks that need the device state, open
// (the sweep's set-up, event 0, W zeroed where the producer only scatters), its producer kernel into W, finish.
struct BlockCall {
  scilmm_factor* const fac;
  scilmm_symbolic* const sym;
  const DevGuard guard;
  Dev* D = nullptr;
  std::optional<Sweep> sw;

  // before anything is dereferenced (fac->sym->S is what the constructor and the entry points read next)
  static bool args_ok(const scilmm_factor* fac, int32_t r, const double* d_Q, int32_t q, const double* d_stats) {
    return fac && d_Q && d_stats && r >= 1 && r <= RPMAX && q >= 1 && q <= SCAN_QMAX && fac->sym && fac->sym->S;
  }
  explicit BlockCall(scilmm_factor* f) : fac(f), sym(f->sym), guard(f->sym) {}

  // the refusals, the slice partial sums (allocated on the first call on a handle, or for a wider q; nothing is allocated
  // per block afterwards) and the inverse permutation; `gram`: the partial tiles of X^T X as well (allocated on the first
  // Gram block on a handle, for the widest block: never again); `pairs`: a gxe block's rows of cross products, which take the
  // statistics' partial sums over once those are folded
  int begin(int32_t q, const char* who, bool gram = false, int32_t pairs = 0) {
    TRY(check_half(fac, who));
    TRY(begin_rhs(fac, who));
    D = (Dev*)sym->device;
    const int64_t nslice = ((int64_t)sym->S->n + SCAN_SLICE - 1) / SCAN_SLICE;
    const size_t need = (size_t)nslice * (size_t)std::max(q + 1, pairs) * RPMAX;
    TRY(grow_synced(sym, D, &D->scan_partial, &D->scan_partial_cap, need));
    if (gram) TRY(grow_synced(sym, D, &D->gram_partial, &D->gram_partial_cap, (size_t)gram_slices(GRAM_SLICE_MIN) * GRAM_TILES * 256));
    return ensure_iperm(sym, D);
  }

  int open(int32_t r, bool zero_W) {
    sw.emplace(fac, D);
    sw->set_block(r);
    HIPCHK(D->scan_t.start(D->stream));
    if (zero_W) HIPCHK(hipMemsetAsync(D->W, 0, sizeof(double) * (size_t)sw->tot, D->stream));
    return SCILMM_OK;
  }

  int64_t gram_slices(int slice) const { return ((int64_t)sym->S->n + slice - 1) / slice; }

  // W holds the block (event 1 is recorded here): the forward sweep, then |x_c|^2 and Q^T x_c from one pass over X, in fixed
  // row slices folded in slice order, to d_out ((q + 1) x r).  With d_gram (begin was told so): X^T X (r x r) from a second
  // pass over X on the matrix pipe, inside the statistics interval; without it the launches are the same as ever.  With gxe
  // (begin was told its pairs; r = d * gxe->r columns): the cross products between the d columns of every marker, from a second
  // pass over X and the same fold, to gxe->d_cross (pairs x gxe->r), inside the statistics interval as well.
  int finish(int32_t r, const double* d_Q, int32_t q, double* d_out, double* d_gram = nullptr, const Gxe* gxe = nullptr) {
    const int32_t n = sym->S->n;
    hipStream_t s0 = D->stream;
    const int64_t nslice = ((int64_t)n + SCAN_SLICE - 1) / SCAN_SLICE;
    HIPCHK(D->scan_t.mark(s0, 1));
    TRY(sw->forward_single());
    HIPCHK(D->scan_t.mark(s0, 2));
    const auto k_stats = q <= 8 ? k_scan_stats<8, 4> : q <= 16 ? k_scan_stats<16, 2> : k_scan_stats<SCAN_QMAX, 1>;
    hipLaunchKernelGGL(k_stats, dim3((unsigned)nslice), dim3(256), 0, s0, n, sw->rp, (const double*)D->X, d_Q, q, D->scan_partial);
    hipLaunchKernelGGL(k_scan_fold, dim3((unsigned)(q + 1)), dim3(SCAN_FOLD * RPMAX), 0, s0, nslice, (const double*)D->scan_partial, q, r, d_out);
    if (d_gram) {
      const int32_t nt = sw->rp / 16, ntile = nt * (nt + 1) / 2;
      const GramShape g = gram_shape();
      const int64_t gs = gram_slices(g.slice);
      hipLaunchKernelGGL(gram_kernel(g), dim3((unsigned)gs), dim3(256), 0, s0, n, sw->rp, (const double*)D->X, D->gram_partial);
      hipLaunchKernelGGL(k_gram_fold, dim3((unsigned)ntile), dim3(GRAM_FOLD * 256), 0, s0, gs, ntile, (const double*)D->gram_partial, r, d_gram);
    }
    if (gxe) {
      const int32_t pairs = gxe->pairs();
      HIPCHK(D->scan_t.mark(s0, 5));
      hipLaunchKernelGGL(cross_kernel(gxe->m + 1, gxe->r), dim3((unsigned)nslice), dim3(256), 0, s0, n, gxe->r, sw->rp, (const double*)D->X,
                         D->scan_partial);
      hipLaunchKernelGGL(k_scan_fold, dim3((unsigned)pairs), dim3(SCAN_FOLD * RPMAX), 0, s0, nslice, (const double*)D->scan_partial, pairs - 1,
                         gxe->r, gxe->d_cross);
    }
    HIPCHK(D->scan_t.close(s0));
    D->gxe_pending = gxe != nullptr;
    D->block_r = r;  // X holds this block until the work buffers are asked for again (scan_panel)
    D->block_rp = sw->rp;
    if (D->h_chain_err) HIPCHK(hipMemcpyAsync(D->h_chain_err, D->d_chain_err, sizeof(int32_t), hipMemcpyDeviceToHost, s0));
    HIPCHK(hipGetLastError());
    return SCILMM_OK;
  }
};

// One block of markers, whatever their form.  `fill(D, n, rp)` launches the form's two kernels on D->stream: rows 0..2 of the
// statistics (n_obs, mean, centred sum of squares) by a workgroup per marker, then W = P (g - mean), missing = 0, columns padded
// to rp, each tile of individuals written straight to its permuted rows.  Rows 3..: |w(g)|^2 and Q^T w(g); with d_gram, X^T X.
// With d_E (m environment columns; the plain and the Gram calls pass none and keep their launches): the block is d = 1 + m times
// as wide, the fill writes its r columns and zeroes the rest, k_scan_expand multiplies them into the interaction columns, and
// the statistics are (q + 1) x (d r) -- read as ((q + 1) d) x r -- followed by the d (d - 1) / 2 rows of cross products.
template <class Fill>
int marker_block(scilmm_factor* fac, const char* who, int32_t r, const double* d_Q, int32_t q, double* d_stats, double* d_gram, Fill fill,
                 const double* d_E = nullptr, int32_t m = 0) {
  BlockCall b(fac);
  const int32_t d = 1 + m;
  const Gxe gxe{d_E, m, r, d_stats + (3 + (int64_t)(q + 1) * d) * r};
  TRY(b.begin(q, who, d_gram != nullptr, gxe.pairs()));
  TRY(b.open(d * r, false));
  scilmm_symbolic* sym = b.sym;
  const int32_t n = sym->S->n;
  fill(b.D, n, b.sw->rp);
  if (d_E) {
    HIPCHK(b.D->scan_t.mark(b.D->stream, 4));
    hipLaunchKernelGGL(k_scan_expand<4>, dim3((unsigned)(((int64_t)n + GXE_ROWS - 1) / GXE_ROWS)), dim3(256), 0, b.D->stream, n, r, m, b.sw->rp,
                       d_E, b.D->W);
  }
  return b.finish(d * r, d_Q, q, d_stats + 3 * (int64_t)r, d_gram, d_E ? &gxe : nullptr);
}

// The fills.  int8 rows: exact integer sums, no order to fix; packed PLINK rows: the same sums taken class by class; dosage rows
// of element type T: integer sums (uint16) or fixed-order fp64 sums in two passes (float).  W goes through the sample map if any.
unsigned scan_tiles(int32_t n) { return (unsigned)(((int64_t)n + SCAN_TILE - 1) / SCAN_TILE); }

auto fill_int8(const int8_t* d_geno, int64_t ld_geno, int32_t r, double* d_stats) {
  return [=](Dev* D, int32_t n, int32_t rp) {
    hipLaunchKernelGGL(k_scan_moments, dim3((unsigned)r), dim3(256), 0, D->stream, n, d_geno, ld_geno, r, d_stats);
    hipLaunchKernelGGL(k_scan_dequant, dim3(scan_tiles(n)), dim3(256), 0, D->stream, n, r, rp, d_geno, ld_geno, (const int32_t*)D->d_iperm,
                       (const double*)(d_stats + r), D->W);
  };
}

auto fill_bed(const uint8_t* d_bed, int64_t ld_bed, int32_t n_samples, const int32_t* d_sample, int32_t flags, int32_t r, double* d_stats) {
  return [=](Dev* D, int32_t n, int32_t rp) {
    hipLaunchKernelGGL(k_bed_moments, dim3((unsigned)r), dim3(256), 0, D->stream, n, n_samples, d_bed, ld_bed, d_sample, flags, r, d_stats);
    hipLaunchKernelGGL(k_bed_dequant, dim3(scan_tiles(n)), dim3(256), 0, D->stream, n, n_samples, r, rp, d_bed, ld_bed, d_sample, flags,
                       (const int32_t*)D->d_iperm, (const double*)(d_stats + r), D->W);
  };
}

template <class T>
auto fill_dosage(const void* d_dos, int64_t ld, int32_t n_samples, const int32_t* d_sample, int32_t r, double* d_stats) {
  return [=](Dev* D, int32_t n, int32_t rp) {
    hipLaunchKernelGGL(k_dos_moments<T>, dim3((unsigned)r), dim3(256), 0, D->stream, n, n_samples, (const T*)d_dos, ld, d_sample, r, d_stats);
    hipLaunchKernelGGL(k_dos_dequant<T>, dim3(scan_tiles(n)), dim3(256), 0, D->stream, n, n_samples, r, rp, (const T*)d_dos, ld, d_sample,
                       (const int32_t*)D->d_iperm, (const double*)(d_stats + r), D->W);
  };
}

// The frame of a call that runs behind a block and sweeps nothing itself: the handle's device made current, the refusals of
// the half-solves, the factor settled -- in that order --, then the device state, n and the stream.  Whatever the call asks
// next (block_left, its buffers) comes after begin.
struct PostCall {
  scilmm_factor* const fac;
  scilmm_symbolic* const sym;
  const DevGuard guard;
  Dev* D = nullptr;
  int32_t n = 0;
  hipStream_t s0 = nullptr;
  explicit PostCall(scilmm_factor* f) : fac(f), sym(f->sym), guard(f->sym) {}
  int begin(const char* who) {
    TRY(check_half(fac, who));
    TRY(settle(fac, who));
    D = (Dev*)sym->device;
    n = sym->S->n;
    s0 = D->stream;
    return SCILMM_OK;
  }
};

// What reads the block the last scan block on the handle left in X asks first: that it is still there, and that r is its.
int block_left(scilmm_symbolic* sym, const Dev* D, const char* who, int32_t r) {
  if (D->block_r == 0) {
    sym->err = std::string(who) + ": no scan block on this handle since the work buffers were last used (a solve, a product or a "
                                  "refactorization came in between): run the block first";
    return SCILMM_ERR_STATE;
  }
  if (D->block_r != r) {
    sym->err = std::string(who) + ": r = " + std::to_string(r) + ", the block left behind has " + std::to_string(D->block_r) + " columns";
    return SCILMM_ERR_STATE;
  }
  return SCILMM_OK;
}

// X^T Y for the block the last scan block on the handle left in X (scilmm_scan_panel_dev): the refusals of the half-solves, the
// record of that block, the partial tiles (grown for a wider panel only: the stream is synchronised first, and nothing is
// allocated afterwards for the same or a smaller t), k_scan_panel and k_panel_fold between the call's own events.  Nothing of
// the work buffers is written: the block stays where it is, and any number of panels may follow one block.
int scan_panel(scilmm_factor* fac, int32_t r, const double* d_Y, int64_t ld_y, int32_t t, double* d_xty, int64_t ld_out) {
  const char* who = "scilmm_scan_panel_dev";
  PostCall c(fac);
  TRY(c.begin(who));
  scilmm_symbolic* sym = c.sym;
  Dev* D = c.D;
  TRY(block_left(sym, D, who, r));
  const int32_t n = c.n, rp = D->block_rp, ntile = (rp / 16) * PANEL_NJ;
  const int32_t npanel = (t + PANEL_COLS - 1) / PANEL_COLS;
  const int slice = panel_slice();
  const int64_t nslice = ((int64_t)n + slice - 1) / slice;
  const size_t need = (size_t)(((int64_t)n + PANEL_SLICE_MIN - 1) / PANEL_SLICE_MIN) * (size_t)npanel * PANEL_NI * PANEL_NJ * 256;
  TRY(grow_synced(sym, D, &D->panel_partial, &D->panel_partial_cap, need));
  hipStream_t s0 = c.s0;
  HIPCHK(D->panel_t.start(s0));
  hipLaunchKernelGGL(panel_kernel(slice), dim3((unsigned)nslice, (unsigned)npanel), dim3(256), 0, s0, n, rp, (const double*)D->X, d_Y, ld_y, t,
                     D->panel_partial);
  HIPCHK(D->panel_t.mark(s0, 1));
  hipLaunchKernelGGL(k_panel_fold, dim3((unsigned)(npanel * ntile)), dim3(PANEL_FOLD * 256), 0, s0, nslice, npanel, ntile,
                     (const double*)D->panel_partial, r, t, d_xty, ld_out);
  HIPCHK(D->panel_t.close(s0));
  HIPCHK(hipGetLastError());
  return SCILMM_OK;
}

// The block the last scan block on the handle left in X, copied to columns col0 .. of a caller's store
// (scilmm_scan_block_keep_dev): the refusals and the record of scan_panel, then k_scan_keep.  Nothing is allocated, nothing of the
// work buffers is written and the record stays: a Gram pass, panels and further keeps may follow the same block.
int scan_keep(scilmm_factor* fac, int32_t r, double* d_dst, int64_t ld_dst, int64_t col0) {
  const char* who = "scilmm_scan_block_keep_dev";
  PostCall c(fac);
  TRY(c.begin(who));
  scilmm_symbolic* sym = c.sym;
  Dev* D = c.D;
  TRY(block_left(sym, D, who, r));
  const int64_t nchunk = ((int64_t)c.n + KEEP_ROWS - 1) / KEEP_ROWS;
  hipLaunchKernelGGL(k_scan_keep, dim3((unsigned)std::min<int64_t>(nchunk, KEEP_GRID)), dim3(256), 0, c.s0, c.n, D->block_rp,
                     (const double*)D->X, d_dst, ld_dst, col0);
  HIPCHK(hipGetLastError());
  return SCILMM_OK;
}

// What the three saddlepoint entry points share beside their form's marker arguments (scilmm_scan_spa*_dev).
struct SpaArgs {
  const double *d_stats, *d_R, *d_u, *d_mu, *d_C;
  int32_t c;
  const double* d_Minv;
  double cutoff;
  double* d_spa;
  // before anything of the handle is read (a NaN cutoff fails the comparison)
  static bool args_ok(const scilmm_factor* fac, int32_t r, const SpaArgs& a) {
    return fac && a.d_stats && a.d_R && a.d_u && a.d_mu && a.d_C && a.d_Minv && a.d_spa && r >= 1 && r <= RPMAX && a.c >= 1 &&
           a.c <= SPA_CMAX && a.cutoff >= 0.0 && fac->sym && fac->sym->S;
  }
};

// The scratch of g^ rows both saddlepoint kernels write (RPMAX x n doubles): allocated by the first call on the handle after a
// stream synchronise, never again.
int spa_scratch(scilmm_symbolic* sym, Dev* D) {
  return grow_synced(sym, D, &D->spa_scratch, &D->spa_scratch_cap, (size_t)RPMAX * (size_t)std::max(sym->S->n, 1));
}

// The saddlepoint p-values of the r markers of the plain block queued before this call (scilmm_scan_spa*_dev): the refusals of
// the half-solves, the scratch of g^ rows (spa_scratch), k_scan_spa between the call's own events.  Nothing of the work buffers
// is touched: the block stays available to scilmm_scan_panel_dev.
template <class Reader>
int scan_spa(scilmm_factor* fac, const char* who, int32_t r, Reader rd, const SpaArgs& a) {
  PostCall c(fac);
  TRY(c.begin(who));
  scilmm_symbolic* sym = c.sym;
  Dev* D = c.D;
  TRY(spa_scratch(sym, D));
  HIPCHK(D->spa_t.start(c.s0));
  hipLaunchKernelGGL(k_scan_spa<Reader>, dim3((unsigned)r), dim3(256), 0, c.s0, c.n, r, a.c, rd, a.d_stats, a.d_R, a.d_u, a.d_mu, a.d_C, a.d_Minv,
                     a.cutoff, D->spa_scratch, a.d_spa);
  HIPCHK(D->spa_t.close(c.s0));
  HIPCHK(hipGetLastError());
  return SCILMM_OK;
}

// What the finish of a block and of a wide set refuse alike: the pointers, c, q, the tail method, the weight mode and the grid (a
// HOST array, read here: a NaN fails its comparison).  Nothing of a handle is read.
inline bool fin_weights_ok(int32_t weight_mode, const double* d_weights) {
  return (weight_mode == FIN_BETA || weight_mode == FIN_ONES || weight_mode == FIN_GIVEN) && (weight_mode != FIN_GIVEN || d_weights);
}
template <class Args>
bool fin_args_ok(const Args& a) {
  if (!a.d_stats || !a.d_gram || !a.d_R || !a.d_u || !a.d_out || a.c < 1 || a.c > FIN_CMAX || a.q != a.c + 1 || a.n_rho < 0 ||
      a.n_rho > FIN_RHO_MAX || (a.n_rho > 0 && !a.rho) || (a.method != FIN_SADDLE && a.method != FIN_LIU) ||
      !fin_weights_ok(a.weight_mode, a.d_weights))
    return false;
  for (int32_t j = 0; j < a.n_rho; ++j)
    if (!(a.rho[j] >= 0.0 && a.rho[j] <= 1.0)) return false;
  return true;
}

// What scilmm_sets_finish_dev takes beside the factor.
struct FinishArgs {
  int32_t r, q;
  const double *d_stats, *d_gram, *d_R, *d_u;
  int32_t c, n_sets;
  const int32_t* set_start;
  int32_t weight_mode;
  const double* d_weights;
  int32_t method;
  const double* rho;
  int32_t n_rho;
  double* d_out;
  int64_t ld_out;
  double* d_lam;
  const double* d_vscale = nullptr;   // the columns' variance scales (scilmm_sets_finish_scaled_dev), or null: all 1
  // what the set SPA entry points check as well: the offsets (a HOST array, read here) and the weights
  static bool sets_ok(int32_t r, int32_t n_sets, const int32_t* set_start, int32_t weight_mode, const double* d_weights) {
    if (!set_start || n_sets < 1 || n_sets > r || !fin_weights_ok(weight_mode, d_weights)) return false;
    if (set_start[0] != 0 || set_start[n_sets] > r) return false;
    for (int32_t i = 0; i < n_sets; ++i)
      if (set_start[i + 1] <= set_start[i]) return false;
    return true;
  }
  // before anything of the handle is read; the offsets are a HOST array and are read here
  static bool args_ok(const scilmm_factor* fac, const FinishArgs& a) {
    if (!fac || !fin_args_ok(a) || a.r < 1 || a.r > RPMAX || a.ld_out < FIN_HEAD + a.n_rho ||
        !sets_ok(a.r, a.n_sets, a.set_start, a.weight_mode, a.d_weights))
      return false;
    return fac->sym && fac->sym->S;  // (what needs no handle has been checked: with it wrong, nothing of the handle is read)
  }
};

// What the three finishes of a block's sets derive from the offsets and the grid (HOST arrays, read here): the kernels' copy
// of both, the capacity the block's widest set asks for, the workgroup size and the dynamic LDS that go with it.  `kernel` is
// the one that takes the LDS: more than 64 KiB has to be asked for (for the widest block there can be; the call is cheap and
// idempotent).
struct SetLayout {
  FinSets sets{};
  int32_t cap = 0, nt = 0;
  size_t lds = 0;
};
int set_layout(scilmm_symbolic* sym, const FinishArgs& a, const void* kernel, SetLayout* l) {
  int32_t widest = 0;
  for (int32_t i = 0; i <= a.n_sets; ++i) l->sets.start[i] = a.set_start[i];
  for (int32_t i = 0; i < a.n_sets; ++i) widest = std::max(widest, a.set_start[i + 1] - a.set_start[i]);
  for (int32_t j = 0; j < a.n_rho; ++j) l->sets.grid.rho[j] = a.rho[j];
  l->cap = std::max(2, (widest + 1) & ~1);
  l->nt = l->cap > 64 ? FIN_NT_MAX : 256;
  l->lds = sizeof(double) * (size_t)fin_lds_doubles(l->cap, l->nt);
  HIPCHK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)(sizeof(double) * (size_t)fin_lds_doubles(RPMAX, FIN_NT_MAX))));
  return SCILMM_OK;
}

// Everything after a Gram block, for the sets of the block (scilmm_sets_finish_dev, scilmm_sets_finish_scaled_dev): the
// refusals of the scan blocks, then k_sets_finish between the call's own events, one workgroup per set, its LDS sized by the
// block's largest set.  Nothing of the factor is read and nothing of the work buffers is touched; nothing is allocated.
int sets_finish(scilmm_factor* fac, const FinishArgs& a, const char* who) {
  PostCall c(fac);
  TRY(c.begin(who));
  scilmm_symbolic* sym = c.sym;
  Dev* D = c.D;
  SetLayout l;
  TRY(set_layout(sym, a, (const void*)k_sets_finish, &l));
  HIPCHK(D->fin_t.start(c.s0));
  hipLaunchKernelGGL(k_sets_finish, dim3((unsigned)a.n_sets), dim3((unsigned)l.nt), l.lds, c.s0, a.r, a.c, a.d_stats, a.d_gram, a.d_R, a.d_u,
                     l.sets, a.weight_mode, a.d_weights, a.method, a.n_rho, l.cap, a.d_out, a.ld_out, a.d_lam, a.d_vscale);
  HIPCHK(D->fin_t.close(c.s0));
  HIPCHK(hipGetLastError());
  return SCILMM_OK;
}

// What scilmm_sets_finish_panel_dev takes beside the factor: the block and the sets of FinishArgs without u, the scores and the
// scales of the t traits, and the two outputs.
struct PanelFinishArgs {
  FinishArgs fin;               // d_u, d_out, ld_out, d_lam are not used
  const double* d_xty;
  int64_t ld_xty;
  int32_t t;
  const double* d_tscale;
  double *d_head, *d_out;
  // the scales where the host can read them (pinned or managed memory): finite and positive.  Device memory is the caller's to check.
  static bool scales_ok(const double* d_tscale, int32_t t) {
    if (!d_tscale) return true;
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, d_tscale) != hipSuccess) {
      (void)hipGetLastError();
      return true;
    }
    if (at.type != hipMemoryTypeHost && !at.isManaged) return true;
    for (int32_t i = 0; i < t; ++i)
      if (!(d_tscale[i] > 0.0 && std::isfinite(d_tscale[i]))) return false;
    return true;
  }
  // before anything of the handle is read
  static bool args_ok(const scilmm_factor* fac, const PanelFinishArgs& a) {
    if (!a.d_xty || !a.d_head || !a.d_out || a.t < 1 || a.t > PT_TMAX || a.ld_xty < a.t) return false;
    return FinishArgs::args_ok(fac, a.fin) && scales_ok(a.d_tscale, a.t);
  }
};

// Traits per workgroup of k_sets_panel_tail: enough groups that sets x groups covers the device PT_COVER times over, a group no
// larger than PT_GROUP_MAX; SCILMM_SETS_PANEL_GROUP=<1 .. 32>, read per call, takes its place (the numbers do not depend on it:
// tools/sets_panel_timing.py times the sizes side by side, the tests run a ragged last group with it).
constexpr int PT_COVER = 8;
inline int32_t panel_tail_group(int32_t n_sets, int32_t t, int32_t n_cu) {
  if (const char* e = getenv("SCILMM_SETS_PANEL_GROUP")) {
    const int g = atoi(e);
    if (g >= 1 && g <= PT_GROUP_MAX) return g;
  }
  const int64_t want = (int64_t)PT_COVER * std::max(n_cu, 1);
  const int64_t g = ((int64_t)n_sets * t + want - 1) / want;
  return (int32_t)std::min<int64_t>(std::max<int64_t>(g, 1), PT_GROUP_MAX);
}

// The finish of the sets of a Gram block against the t traits of a panel (scilmm_sets_finish_panel_dev; setpanel.hip.h, DESIGN.md
// section 24): the refusals of sets_finish, the records (grown for more sets, wider sets or a longer grid only: the stream is
// synchronised first, and nothing is allocated afterwards for the same or a smaller call), then k_sets_spectra, one workgroup per
// set, and k_sets_panel_tail, one per (set, trait group), between the call's own events.  Nothing of the factor is read and
// nothing of the work buffers is touched.
int sets_finish_panel(scilmm_factor* fac, const PanelFinishArgs& p, const char* who) {
  PostCall c(fac);
  TRY(c.begin(who));
  scilmm_symbolic* sym = c.sym;
  Dev* D = c.D;
  const FinishArgs& a = p.fin;
  SetLayout l;
  TRY(set_layout(sym, a, (const void*)k_sets_spectra, &l));
  const int64_t ld_rec = rec_doubles(l.cap, a.n_rho);
  TRY(grow_synced(sym, D, &D->pfin_rec, &D->pfin_rec_cap, (size_t)ld_rec * (size_t)a.n_sets));
  if (D->pfin_cu == 0) {
    int cu = 0;
    HIPCHK(hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, D->device));
    D->pfin_cu = std::max(cu, 1);
  }
  const int32_t group = panel_tail_group(a.n_sets, p.t, D->pfin_cu);
  const size_t lds_tail = sizeof(double) * (size_t)ptail_lds_doubles(l.cap, a.n_rho, group);
  hipStream_t s0 = c.s0;
  HIPCHK(D->pfin_t.start(s0));
  hipLaunchKernelGGL(k_sets_spectra, dim3((unsigned)a.n_sets), dim3((unsigned)l.nt), l.lds, s0, a.r, a.c, a.d_stats, a.d_gram, a.d_R, l.sets,
                     a.weight_mode, a.d_weights, a.n_rho, l.cap, D->pfin_rec, ld_rec, p.d_head);
  HIPCHK(D->pfin_t.mark(s0, 1));
  hipLaunchKernelGGL(k_sets_panel_tail, dim3((unsigned)a.n_sets, (unsigned)((p.t + group - 1) / group)), dim3(PT_NT), lds_tail, s0, l.cap,
                     a.n_rho, l.sets.grid, a.method, (const double*)D->pfin_rec, ld_rec, p.d_xty, p.ld_xty, p.t, p.d_tscale, group, p.d_out);
  HIPCHK(D->pfin_t.close(s0));
  HIPCHK(hipGetLastError());
  return SCILMM_OK;
}

// What scilmm_sets_finish_masks_dev takes beside the factor: the block and the sets of FinishArgs (d_lam is not used), the
// annotation words, the cutoffs (a HOST array, read here) and ACAT-V's pooling bound.
struct MasksFinishArgs {
  FinishArgs fin;
  const uint32_t* d_ann;
  int32_t n_ann;
  const double* maf_cut;
  int32_t n_cut;
  double acat_mac;
  // before anything of the handle is read (a NaN cutoff or bound fails its comparison)
  static bool args_ok(const scilmm_factor* fac, const MasksFinishArgs& a) {
    if (!a.d_ann || !a.maf_cut || a.n_ann < 1 || a.n_ann > MASK_ANN_MAX || a.n_cut < 1 || a.n_cut > MASK_CUT_MAX ||
        !(a.acat_mac >= 0.0 && std::isfinite(a.acat_mac)) || a.fin.n_rho < 0 || a.fin.ld_out < FIN_HEAD + MASK_TAIL + (int64_t)a.fin.n_rho)
      return false;
    for (int32_t i = 0; i < a.n_cut; ++i)
      if (!(a.maf_cut[i] > 0.0 && a.maf_cut[i] <= 0.5)) return false;
    return FinishArgs::args_ok(fac, a.fin);
  }
};

// The finish of the sets of a Gram block under n_ann annotation masks crossed with n_cut MAF cutoffs
// (scilmm_sets_finish_masks_dev; setmasks.hip.h): the refusals of sets_finish, then k_sets_finish_masks
// between the call's own events, one workgroup per (set, annotation, cutoff), its LDS sized by the block's largest set.  Nothing of
// the factor is read and nothing of the work buffers is touched; nothing is allocated.
int sets_finish_masks(scilmm_factor* fac, const MasksFinishArgs& p, const char* who) {
  PostCall c(fac);
  TRY(c.begin(who));
  scilmm_symbolic* sym = c.sym;
  Dev* D = c.D;
  const FinishArgs& a = p.fin;
  SetLayout l;
  TRY(set_layout(sym, a, (const void*)k_sets_finish_masks, &l));
  FinCuts cuts{};
  for (int32_t j = 0; j < p.n_cut; ++j) cuts.cut[j] = p.maf_cut[j];
  HIPCHK(D->mfin_t.start(c.s0));
  hipLaunchKernelGGL(k_sets_finish_masks, dim3((unsigned)(a.n_sets * p.n_ann * p.n_cut)), dim3((unsigned)l.nt), l.lds, c.s0, a.r, a.c, a.d_stats,
                     a.d_gram, a.d_R, a.d_u, l.sets, a.weight_mode, a.d_weights, a.method, a.n_rho, l.cap, p.d_ann, p.n_ann, cuts, p.n_cut,
                     p.acat_mac, a.d_out, a.ld_out);
  HIPCHK(D->mfin_t.close(c.s0));
  HIPCHK(hipGetLastError());
  return SCILMM_OK;
}

// What scilmm_sets_finish_wide_dev takes beside the factor.
struct WideArgs {
  int32_t k, block, q;
  const double *d_stats, *d_gram, *d_cross;
  int64_t ld_cross;
  const double *d_R, *d_u;
  int32_t c, weight_mode;
  const double* d_weights;
  int32_t method;
  const double* rho;
  int32_t n_rho;
  double *d_out, *d_lam;
  const double* d_vscale = nullptr;   // the markers' variance scales (scilmm_sets_finish_wide_scaled_dev), or null: all 1
  static int32_t bp(int32_t block) { return (block + 15) / 16 * 16; }   // a sub-block's columns in the cross store
  int32_t bp() const { return bp(block); }
  int32_t nsub() const { return (k + block - 1) / block; }
  // before anything of the handle is read
  // the shape of a wide set's pieces, which the set saddlepoint checks as well
  static bool shape_ok(int32_t k, int32_t block, const double* d_cross, int64_t ld_cross) {
    if (k < 1 || k > WIDE_KMAX || block < 1 || block > RPMAX) return false;
    const int32_t nsub = (k + block - 1) / block;
    const int64_t kept = (int64_t)(nsub - 1) * bp(block);    // the columns of the cross store
    return kept <= WIDE_KMAX && (nsub == 1) == (d_cross == nullptr) && (nsub == 1 || ld_cross >= kept);
  }
  static bool args_ok(const scilmm_factor* fac, const WideArgs& a) {
    if (!fac || !fin_args_ok(a) || !shape_ok(a.k, a.block, a.d_cross, a.ld_cross)) return false;
    return fac->sym && fac->sym->S;  // (what needs no handle has been checked: with it wrong, nothing of the handle is read)
  }
};

// Everything after the sub-blocks of ONE set of up to 4 096 markers (scilmm_sets_finish_wide_dev and, with the markers' variance
// scales, scilmm_sets_finish_wide_scaled_dev; setwide.hip.h): the refusals of sets_finish, the work space (grown for a wider set only: the stream is synchronised first, and nothing is
// allocated afterwards for the same or a narrower set), then plain launches between the call's own events -- prep, form, burden |
// the pre-step and k - 1 steps of the reduction, two launches each, sized by k (the number of kept markers is the device's) |
// scale, eig | tails.  Nothing of the factor is read and nothing of the work buffers is touched.
int sets_finish_wide(scilmm_factor* fac, const WideArgs& a, const char* who) {
  PostCall c(fac);
  TRY(c.begin(who));
  scilmm_symbolic* sym = c.sym;
  Dev* D = c.D;
  const int32_t k = a.k;
  TRY(grow_synced(sym, D, &D->wide_ws, &D->wide_ws_cap, wide_doubles((size_t)k)));
  const WideWs ws = wide_cut(D->wide_ws, (size_t)k);
  const WideIn in{k, a.block, a.bp(), a.q, a.d_stats, a.d_gram, a.d_cross, a.ld_cross};
  FinGrid grid{};
  for (int32_t j = 0; j < a.n_rho; ++j) grid.rho[j] = a.rho[j];
  hipStream_t s0 = c.s0;
  HIPCHK(D->wide_t.start(s0));
  hipLaunchKernelGGL(k_wide_prep, dim3(1), dim3(WIDE_PREP_NT), 0, s0, in, a.c, a.d_R, a.d_u, a.weight_mode, a.d_weights, ws, a.n_rho, a.d_out,
                     a.d_lam, a.d_vscale);
  hipLaunchKernelGGL(k_wide_form, dim3((unsigned)k), dim3(256), 0, s0, in, a.c, ws);
  hipLaunchKernelGGL(k_wide_burden, dim3(1), dim3(256), 0, s0, ws, a.d_out);
  HIPCHK(D->wide_t.mark(s0, 1));
  // step j works on the trailing matrix of order at most k - 1 - j; the last one (order 1) only stores d and e, as does "step"
  // k - 1, which has nothing behind it but the last diagonal entry
  for (int32_t j = -1; j < k; ++j) {
    const unsigned wgs = (unsigned)std::max(1, (k - 1 - j + WIDE_ROWS - 1) / WIDE_ROWS);
    hipLaunchKernelGGL(k_wide_symv, dim3(wgs), dim3(256), 0, s0, j, ws);
    if (k - 1 - j >= 2 || j < 0) hipLaunchKernelGGL(k_wide_rank2, dim3(wgs), dim3(256), 0, s0, j, ws);
  }
  HIPCHK(D->wide_t.mark(s0, 2));
  hipLaunchKernelGGL(k_wide_scale, dim3((unsigned)(a.n_rho + 2)), dim3(256), 0, s0, k, a.n_rho, grid, ws);
  hipLaunchKernelGGL(k_wide_eig, dim3((unsigned)((k + 63) / 64), (unsigned)(a.n_rho + 2)), dim3(64), 0, s0, k, ws, a.d_lam);
  HIPCHK(D->wide_t.mark(s0, 3));
  hipLaunchKernelGGL(k_wide_tails, dim3(1), dim3(256), 0, s0, k, a.n_rho, grid, a.method, ws, a.d_out);
  HIPCHK(D->wide_t.close(s0));
  HIPCHK(hipGetLastError());
  return SCILMM_OK;
}

// What the three set SPA entry points take beside their form's marker arguments and the common part of the marker calls
// (scilmm_sets_spa*_dev): the Gram matrix, the markers' saddlepoint rows, the sets and the two outputs.
struct SetSpaArgs {
  SpaArgs spa;                 // d_spa: the block's SPA_ROWS x r rows, an INPUT here
  const double* d_gram;
  int32_t n_sets;
  const int32_t* set_start;
  int32_t weight_mode;
  const double* d_weights;
  double *d_bspa, *d_vscale;
  // before anything of the handle is read
  static bool args_ok(const scilmm_factor* fac, int32_t r, const SetSpaArgs& a) {
    return a.d_gram && a.d_bspa && a.d_vscale && FinishArgs::sets_ok(r, a.n_sets, a.set_start, a.weight_mode, a.d_weights) &&
           SpaArgs::args_ok(fac, r, a.spa);   // (the handle is looked at last)
  }
};

// The variance scales and the burden's saddlepoint p-value of the sets of the Gram block queued before this call, behind the
// saddlepoint call of its markers (scilmm_sets_spa*_dev): the refusals of the scan blocks, the scratch of scan_spa (row `set` is
// the set's), k_sets_spa between the call's own events, one workgroup per set.  Nothing of the work buffers is touched.
template <class Reader>
int sets_spa(scilmm_factor* fac, const char* who, int32_t r, Reader rd, const SetSpaArgs& a) {
  PostCall c(fac);
  TRY(c.begin(who));
  scilmm_symbolic* sym = c.sym;
  Dev* D = c.D;
  TRY(spa_scratch(sym, D));
  SpaSets sets{};
  for (int32_t i = 0; i <= a.n_sets; ++i) sets.start[i] = a.set_start[i];
  HIPCHK(D->sspa_t.start(c.s0));
  hipLaunchKernelGGL(k_sets_spa<Reader>, dim3((unsigned)a.n_sets), dim3(256), 0, c.s0, c.n, r, a.spa.c, rd, a.spa.d_stats, a.d_gram, a.spa.d_R,
                     a.spa.d_u, a.spa.d_mu, a.spa.d_C, a.spa.d_Minv, a.spa.cutoff, (const double*)a.spa.d_spa, sets, a.weight_mode,
                     a.d_weights, D->spa_scratch, a.d_bspa, a.d_vscale);
  HIPCHK(D->sspa_t.close(c.s0));
  HIPCHK(hipGetLastError());
  return SCILMM_OK;
}

// The collapsed genotype of a wide set, grown by the kept markers of the sub-block queued before this call
// (scilmm_sets_collapse*_dev; setspawide.hip.h): the refusals of the scan blocks, k_sets_collapse between the
// call's own events, a capped grid over the individuals.  Nothing is allocated and nothing of the work buffers or of the
// saddlepoint scratch is touched: the panel and the keep may still follow the block.
struct CollapseArgs {
  const double* d_stats;
  int32_t weight_mode;
  const double* d_weights;
  int32_t first;
  double* d_gB;
  // before anything of the handle is read
  static bool args_ok(const scilmm_factor* fac, int32_t r, const CollapseArgs& a) {
    return fac && a.d_stats && a.d_gB && r >= 1 && r <= RPMAX && (a.first == 0 || a.first == 1) && fin_weights_ok(a.weight_mode, a.d_weights) &&
           fac->sym && fac->sym->S;
  }
};

template <class Reader>
int sets_collapse(scilmm_factor* fac, const char* who, int32_t r, Reader rd, const CollapseArgs& a) {
  PostCall c(fac);
  TRY(c.begin(who));
  scilmm_symbolic* sym = c.sym;
  Dev* D = c.D;
  const unsigned wgs = (unsigned)std::max<int64_t>(1, std::min<int64_t>(((int64_t)c.n + 255) / 256, COLLAPSE_GRID));
  HIPCHK(D->coll_t.start(c.s0));
  hipLaunchKernelGGL(k_sets_collapse<Reader>, dim3(wgs), dim3(256), 0, c.s0, c.n, r, rd, a.d_stats, a.weight_mode, a.d_weights, a.first, a.d_gB);
  HIPCHK(D->coll_t.close(c.s0));
  HIPCHK(hipGetLastError());
  return SCILMM_OK;
}

// What scilmm_sets_spa_wide_dev takes beside the factor.
struct SpaWideArgs {
  int32_t k, block, q;
  const double *d_stats, *d_gram, *d_cross;
  int64_t ld_cross;
  const double *d_R, *d_u, *d_mu, *d_C;
  int32_t c;
  const double* d_Minv;
  double cutoff;
  const double* d_spa;
  int32_t weight_mode;
  const double* d_weights;
  double *d_gB, *d_bspa, *d_vscale;
  // before anything of the handle is read (a NaN cutoff fails the comparison)
  static bool args_ok(const scilmm_factor* fac, const SpaWideArgs& a) {
    if (!fac || !a.d_stats || !a.d_gram || !a.d_R || !a.d_u || !a.d_mu || !a.d_C || !a.d_Minv || !a.d_spa || !a.d_gB || !a.d_bspa ||
        !a.d_vscale || a.c < 1 || a.c > SPA_CMAX || a.q != a.c + 1 || !(a.cutoff >= 0.0) || !fin_weights_ok(a.weight_mode, a.d_weights) ||
        !WideArgs::shape_ok(a.k, a.block, a.d_cross, a.ld_cross))
      return false;
    return fac->sym && fac->sym->S;
  }
};

// The variance scales and the burden's saddlepoint p-value of ONE set of up to 4 096 markers behind its last sub-block
// (scilmm_sets_spa_wide_dev; setspawide.hip.h): the refusals of the scan blocks, the wide finish's work
// space by the wide finish's growth rule (the finish that follows for the same k allocates nothing), then keep, markers, pairs | burden
// between the call's own events.  No genotype is read: the collapsed row is the caller's.
int sets_spa_wide(scilmm_factor* fac, const SpaWideArgs& a, const char* who) {
  PostCall c(fac);
  TRY(c.begin(who));
  scilmm_symbolic* sym = c.sym;
  Dev* D = c.D;
  const int32_t k = a.k;
  TRY(grow_synced(sym, D, &D->wide_ws, &D->wide_ws_cap, wide_doubles((size_t)k)));
  const SwideWs ws = swide_cut(D->wide_ws, (size_t)k);
  const WideIn in{k, a.block, WideArgs::bp(a.block), a.q, a.d_stats, a.d_gram, a.d_cross, a.ld_cross};
  hipStream_t s0 = c.s0;
  HIPCHK(D->swide_t.start(s0));
  hipLaunchKernelGGL(k_swide_keep, dim3(1), dim3(WIDE_PREP_NT), 0, s0, in, ws);
  hipLaunchKernelGGL(k_swide_markers, dim3((unsigned)((k + 63) / 64)), dim3(64), 0, s0, in, a.c, a.d_R, a.d_u, a.d_spa, a.weight_mode,
                     a.d_weights, ws);
  hipLaunchKernelGGL(k_swide_pairs, dim3((unsigned)k), dim3(256), 0, s0, in, a.c, ws);
  HIPCHK(D->swide_t.mark(s0, 1));
  hipLaunchKernelGGL(k_swide_burden, dim3(1), dim3(256), 0, s0, in, c.n, a.c, a.d_mu, a.d_C, a.d_Minv, a.cutoff, ws, a.d_gB, a.d_bspa, a.d_vscale);
  HIPCHK(D->swide_t.close(s0));
  HIPCHK(hipGetLastError());
  return SCILMM_OK;
}

// One block of columns `ids` of sum_k weights[k] A_k, built from the resident values (scilmm_rel_block_dev).
int rel_block(scilmm_factor* fac, const double* weights, const int32_t* ids, int32_t r, const double* d_Q, int32_t q, double* d_stats) {
  BlockCall b(fac);
  scilmm_symbolic* sym = fac->sym;
  const Symbolic& S = *sym->S;
  // the requests sorted by permuted index: the kernel bisects this list; a repeated individual shows as a repeated index
  std::pair<int32_t, int32_t> order[RPMAX];
  for (int32_t c = 0; c < r; ++c) {
    if (ids[c] < 0 || ids[c] >= S.n) {
      sym->err = "scilmm_rel_block_dev: an individual outside 0 .. n-1";
      return SCILMM_ERR_ARG;
    }
    order[c] = {S.iperm[(size_t)ids[c]], c};
  }
  std::sort(order, order + r);
  RelReq req{};
  for (int32_t c = 0; c < r; ++c) {
    if (c > 0 && order[c].first == order[c - 1].first) {
      sym->err = "scilmm_rel_block_dev: an individual is requested twice in one block";
      return SCILMM_ERR_ARG;
    }
    req.p[c] = order[c].first;
    req.col[c] = order[c].second;
  }
  TRY(b.begin(q, "scilmm_rel_block_dev"));
  Dev* D = b.D;
  ValPtrs gen{}, dia{};
  for (int k = 0; k < S.K; ++k) {
    if (weights[k] == 0.0) continue;
    if (!D->have_vals[k]) {
      sym->err = "scilmm_rel_block_dev: the values of a matrix with a nonzero weight are not resident";
      return SCILMM_ERR_STATE;
    }
    TRY(push_val(sym, S.is_diag[k] ? dia : gen, D->vals[k], weights[k]));
  }
  TRY(b.open(r, true));
  // W = P G[:, ids]: the stored columns (r workgroups), then one streaming pass over the pattern for the row parts; row 0 of
  // the statistics = G[i, i]
  const unsigned pass = gen.count > 0 ? (unsigned)std::min<int64_t>((S.nnz_pattern + 255) / 256, REL_GRID) : 0u;
  hipLaunchKernelGGL(k_rel_gather, dim3((unsigned)r + pass), dim3(256), 0, D->stream, D->v, S.nnz_pattern, gen, dia, req, r, b.sw->rp, D->W,
                     d_stats);
  return b.finish(r, d_Q, q, d_stats + (int64_t)r);
}

// The same for r caller rows in CSR on the device (scilmm_rows_block_dev).
int rows_block(scilmm_factor* fac, const int64_t* d_indptr, const int32_t* d_indices, const double* d_data, int32_t r, const double* d_Q,
               int32_t q, double* d_stats) {
  BlockCall b(fac);
  TRY(b.begin(q, "scilmm_rows_block_dev"));
  TRY(b.open(r, true));
  // W[iperm[idx]][c] = data: a wave per row; row 0 of the statistics = 0
  hipLaunchKernelGGL(k_rows_scatter, dim3((unsigned)((r + 3) / 4)), dim3(256), 0, b.D->stream, b.sym->S->n, r, b.sw->rp, d_indptr, d_indices,
                     d_data, (const int32_t*)b.D->d_iperm, b.D->W, d_stats);
  return b.finish(r, d_Q, q, d_stats + (int64_t)r);
}

}  // namespace
