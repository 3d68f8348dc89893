// Microbenchmark, round 3: mfma_f32_feed's question for the fp64 dense-tail kernel.  A synthetic loop with k_dense_b's operand
// feeds -- 16 v_mfma_f64_16x16x4_f64 per k-step and wave, A fragments (two rows per lane) straight from global memory one
// sub-chunk ahead, B image (64 k-rows x 128 columns) by LDS-DMA with one barrier per 64 k, fragments prefetched one k-step
// ahead -- with the 256 workgroups either walking the operand matrix in LOCKSTEP (long contiguous runs per k-column) or each at
// ITS OWN column (2 KB pieces, as a real launch's drifting items produce).
// Variants of the chunk boundary (VAR), for profiles/dense_feed_micro.txt:
//   0  the loop as k_dense_b had it: `s_waitcnt vmcnt(0) lgkmcnt(0)` + barrier at every chunk boundary
//   1  counted wait: vmcnt(8) leaves load_A(next chunk, 0) in flight across the barrier
//   2  1 + a third set of A fragments, fetched two sub-chunks ahead (vmcnt(16) at the boundary)
//   3  the A loads as inline assembly with hand-counted waits: the compiler sees no vector-memory load in the loop, so it adds no
//      wait of its own -- with compiler-visible loads it drains vmcnt(0) at the first use of a loaded register after an LDS-DMA
//      copy was issued (a copy counts as a vector-memory AND an LDS operation: every later wait is a full one), i.e. right behind
//      the copies of the chunk after next, in variants 0 - 2 alike
//   hipcc -O3 --offload-arch=gfx950 mfma_f64_feed.hip -o mfma_f64_feed && ./mfma_f64_feed
#include <hip/hip_runtime.h>
#include <cstdio>
typedef double d4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* lds_vptr;
typedef const __attribute__((address_space(1))) void* gl_vptr;
constexpr int KR = 64, LDB = 144;

#define WAIT_A(a, N)                                                                                                       \
  asm volatile("s_waitcnt vmcnt(" #N ")"                                                                                   \
               : "+v"(a[0][0]), "+v"(a[0][1]), "+v"(a[1][0]), "+v"(a[1][1]), "+v"(a[2][0]), "+v"(a[2][1]), "+v"(a[3][0]), "+v"(a[3][1]))
template <bool DESYNC, int VAR>
__global__ __launch_bounds__(512, 1) void k_feed(double* out, const double* __restrict__ Ag, int md, int iters) {
  extern __shared__ double sm[];  // [2][KR][LDB]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int li = lane & 15, lk = lane >> 4;
  d4 c[8][2];
#pragma unroll
  for (int a = 0; a < 8; ++a) { c[a][0] = (d4){0, 0, 0, 0}; c[a][1] = (d4){0, 0, 0, 0}; }
  const double* A0 = Ag + (size_t)blockIdx.x * 256 + 32 * wv + li;  // this lane's rows: A0, A0 + 16
  const double* Bg = Ag;                                             // B rows: the matrix's first 128 rows (shared by all workgroups)
  constexpr int NS = VAR == 2 ? 3 : 2;  // sets of A fragments
  double rA[NS][4][2];
  auto load_A = [&](long k0, int sub, double (&a)[4][2]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double* p = A0 + (size_t)(k0 + 16 * sub + 4 * q + lk) * md;
      if (VAR == 3) {
        asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(a[q][0]) : "v"(p));
        asm volatile("global_load_dwordx2 %0, %1, off offset:128" : "=v"(a[q][1]) : "v"(p));
      } else {
        a[q][0] = p[0];
        a[q][1] = p[16];
      }
    }
  };
  auto issue_B = [&](long k0, int b) {
    double* Bs = sm + b * KR * LDB;
#pragma unroll
    for (int i = 0; i < KR / 8; ++i) {
      const int kr = wv + 8 * i;
      __builtin_amdgcn_global_load_lds((gl_vptr)(Bg + (size_t)(k0 + kr) * md + 2 * lane), (lds_vptr)(Bs + kr * LDB), 16, 0, 0);
    }
  };
  const long kwrap = 64L * iters;
  long kpos = DESYNC ? 64L * ((blockIdx.x * 37) % iters) : 0;
  load_A(kpos, 0, rA[0]);
  if (VAR == 2) load_A(kpos, 1, rA[1]);
  issue_B(kpos, 0);
  issue_B(kpos + 64, 1);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (VAR == 3) WAIT_A(rA[0], 0);
  __syncthreads();
  int buf = 0;
  double bf[2][8];
#pragma unroll
  for (int jb = 0; jb < 8; ++jb) bf[0][jb] = sm[lk * LDB + 16 * jb + li];
  constexpr int U = VAR == 2 ? 3 : 1;  // (three chunks per trip: the set of a sub-chunk is then known at compile time)
  for (int it0 = 0; it0 < iters; it0 += U)
#pragma unroll
  for (int it = 0; it < U; ++it) {
    const double* Bc = sm + buf * KR * LDB;
    const double* Bn = sm + (buf ^ 1) * KR * LDB;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int s = t >> 2, q = t & 3;
      // (sub-chunk g = 4 * chunk + s lives in set g % NS)
      if (q == 0 && VAR != 2) { if (s < 3) load_A(kpos, s + 1, rA[(s + 1) & 1]); else load_A(kpos + 64, 0, rA[0]); }
      if (q == 0 && VAR == 2) { if (s < 2) load_A(kpos, s + 2, rA[(4 * it + s + 2) % 3]); else load_A(kpos + 64, s - 2, rA[(4 * it + s + 2) % 3]); }
      // hand-counted waits of variant 3, in issue order [8 copies at the boundary] A(1) A(2) A(3) A(next, 0): the fragments of
      // sub-chunk s are used with the 8 loads of the next one (and, for s == 0, the 8 copies) behind them
      // (the waits name the fragment registers as in/out operands, as in k_dense_b: without that tie the scheduler moves MFMAs
      //  in front of their wait, the registers are reused -- for addresses -- while their loads are in flight, and the late
      //  data lands in an address: the first form of this variant ended in an illegal memory access)
      if (VAR == 3 && q == 0) { if (s == 0) WAIT_A(rA[0], 16); else WAIT_A(rA[s & 1], 8); }
      if (t < 15) {
#pragma unroll
        for (int jb = 0; jb < 8; ++jb) bf[(t + 1) & 1][jb] = Bc[(4 * (t + 1) + lk) * LDB + 16 * jb + li];
      } else {
        if (VAR == 0) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        else if (VAR == 2) asm volatile("s_waitcnt vmcnt(16) lgkmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
#pragma unroll
        for (int jb = 0; jb < 8; ++jb) bf[0][jb] = Bn[lk * LDB + 16 * jb + li];
        issue_B(kpos + 128, buf);
      }
#pragma unroll
      for (int jb = 0; jb < 8; ++jb) {
        const int set = VAR == 2 ? (4 * it + s) % 3 : s & 1;
        c[jb][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(bf[t & 1][jb], rA[set][q][0], c[jb][0], 0, 0, 0);
        c[jb][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(bf[t & 1][jb], rA[set][q][1], c[jb][1], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    kpos += 64;
    if (DESYNC && kpos >= kwrap) kpos -= kwrap;
    buf ^= 1;
  }
  double s = 0;
#pragma unroll
  for (int a = 0; a < 8; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) s += c[a][b][r];
  out[blockIdx.x * 512 + tid] = s;
}

template <bool DESYNC, int VAR>
void run(double* d, const double* A, int md, int iters, const char* what) {
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  const int grid = 256;
  const size_t lds = sizeof(double) * 2 * KR * LDB;
  (void)hipFuncSetAttribute((const void*)k_feed<DESYNC, VAR>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  for (int rep = 0; rep < 3; ++rep) {
    hipEventRecord(e0);
    hipLaunchKernelGGL((k_feed<DESYNC, VAR>), dim3(grid), dim3(512), lds, 0, d, A, md, iters);
    hipEventRecord(e1);
    hipEventSynchronize(e1);
    float ms;
    hipEventElapsedTime(&ms, e0, e1);
    const double flops = (double)grid * 8 * iters * 16 * 16 * 2048.0;
    if (rep == 2) printf("%-52s %.3f ms -> %.1f TFLOP/s (%s)\n", what, ms, flops / ms / 1e9, hipGetErrorString(hipGetLastError()));
  }
}

int main() {
  const int md = 256 * 256 + 64, iters = 399;
  const size_t K = 64 * (size_t)(iters + 4);
  double *d, *A;
  (void)hipMalloc(&d, sizeof(double) * 512 * 256);
  (void)hipMalloc(&A, sizeof(double) * (size_t)md * K);  // 13.6 GB
  (void)hipMemset(A, 0, sizeof(double) * (size_t)md * K);
  run<false, 0>(d, A, md, iters, "k_dense_b's feeds, workgroups in lockstep");
  run<true, 0>(d, A, md, iters, "k_dense_b's feeds, every workgroup at its own column");
  run<true, 1>(d, A, md, iters, "  own column, counted wait vmcnt(8)");
  run<true, 2>(d, A, md, iters, "  own column, counted wait + A two sub-chunks ahead");
  run<true, 3>(d, A, md, iters, "  own column, asm A loads + hand-counted waits");
  run<true, 0>(d, A, md, iters, "  own column, vmcnt(0) again (run-to-run spread)");
  run<false, 3>(d, A, md, iters, "  lockstep, asm A loads + hand-counted waits");
  return 0;
}
