// The A_k values on the device (included by engine.hip only, behind products.hip.h): upload from the host, download, and
// the two matrices that are computed where they live -- the IBD values from a pedigree and the dominance values from the
// IBD values.  Value arrays are allocated on first use (ensure_vals) and kept; temporaries belong to a DevScratch.
#pragma once

namespace {

int values_upload(scilmm_symbolic* sym, Dev* D, int32_t k, const double* data_k) {
  const Symbolic& S = *sym->S;
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
  TRY(ensure_vals(sym, D, k));
  if (!h.empty()) HIPCHK(hipMemcpy(D->vals[k], h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
  D->have_vals[k] = 1;
  return SCILMM_OK;
}

int values_download(scilmm_symbolic* sym, Dev* D, int32_t k, double* slots_out) {
  const Symbolic& S = *sym->S;
  const size_t cnt = S.is_diag[k] ? (size_t)S.n : (size_t)S.nnz_pattern;
  HIPCHK(hipMemcpy(slots_out, D->vals[k], cnt * sizeof(double), hipMemcpyDeviceToHost));
  return SCILMM_OK;
}

// (the host-side checks of the pedigree come first: nothing touches the device before they pass)
int ibd_values(scilmm_symbolic* sym, int32_t k, const int32_t* parents) {
  const Symbolic& S = *sym->S;
  const int32_t n = S.n;
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
  TRY(ensure_device(sym, &D));
  hipStream_t s0 = D->stream;
  const int64_t nnz = S.nnz_pattern;
  DevScratch tmp(&sym->err);
  int32_t *d_gen = nullptr, *d_par = nullptr;
  uint8_t *key = nullptr, *skey = nullptr;
  uint32_t *slot = nullptr, *sslot = nullptr;
  int64_t* d_pass = nullptr;
  TRY(tmp.upload(gen, &d_gen, s0));
  TRY(tmp.upload(parents, 2 * (size_t)n, &d_par, s0));
  TRY(ensure_iperm(sym, D));
  TRY(tmp.alloc((size_t)nnz, &key));
  TRY(tmp.alloc((size_t)nnz, &skey));
  TRY(tmp.alloc((size_t)nnz, &slot));
  TRY(tmp.alloc((size_t)nnz, &sslot));
  TRY(tmp.alloc(256, &d_pass));
  TRY(ensure_vals(sym, D, k));
  if (nnz > 0) {
    hipLaunchKernelGGL(k_ibd_keys, dim3(4096), dim3(256), 0, s0, n, D->v.pat_colptr, D->v.pat_row, D->v.perm, (const int32_t*)d_gen, key, slot);
    size_t need = 0;
    uint8_t* cub = nullptr;
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, need, key, skey, slot, sslot, nnz, 0, 8, s0));
    TRY(tmp.alloc(need, &cub));
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
                         D->v.pat_colptr, D->v.pat_row, D->v.perm, D->d_iperm, (const int32_t*)d_par, D->vals[k]);
    }
  }
  HIPCHK(hipStreamSynchronize(s0));
  HIPCHK(hipGetLastError());
  D->have_vals[k] = 1;
  return SCILMM_OK;
}

int dominance_values(scilmm_symbolic* sym, Dev* D, int32_t k_dst, int32_t k_src, const int32_t* parents) {
  const Symbolic& S = *sym->S;
  hipStream_t s0 = D->stream;
  DevScratch tmp(&sym->err);
  int32_t* d_par = nullptr;
  TRY(tmp.upload(parents, 2 * (size_t)S.n, &d_par, s0));
  TRY(ensure_iperm(sym, D));
  TRY(ensure_vals(sym, D, k_dst));
  if (S.nnz_pattern > 0)
    hipLaunchKernelGGL(k_dom_slots, dim3(4096), dim3(256), 0, s0, S.n, D->v.pat_colptr, D->v.pat_row, D->v.perm, D->d_iperm,
                       (const int32_t*)d_par, (const double*)D->vals[k_src], D->vals[k_dst]);
  HIPCHK(hipStreamSynchronize(s0));
  HIPCHK(hipGetLastError());
  D->have_vals[k_dst] = 1;
  return SCILMM_OK;
}

}  // namespace
