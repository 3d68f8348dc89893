// Kernels of the marker scan from PLINK 1 .bed rows (scilmm_scan_block_bed_dev, engine.hip): the two streaming kernels of
// scan.hip.h with the 2-bit decode and the sample map fused in.  What follows them (forward sweep, k_scan_stats,
// k_scan_fold) is shared with the int8 path.
//   k_bed_moments : per marker n_obs, mean, centred sum of squares           reads  r * ceil(N/4) bytes (+ the map)
//   k_bed_dequant : W = P (g - mean), missing = 0, columns padded to rp      reads  r * ceil(N/4) bytes, writes n * rp * 8
// Every sum is an integer sum, every entry of W has one writer, no atomics: the doubles are the same bits as
// k_scan_moments / k_scan_dequant give for the unpacked marker.
//
// Packed layout (variant-major): marker j = bed + j * ld, ceil(N/4) bytes; sample s is bits 2 (s & 3) .. 2 (s & 3) + 1 of
// byte s >> 2.  Codes: 00 = two copies of A1, 01 = missing, 10 = one copy, 11 = none; the bits past sample N-1 are padding.
// With a code split into hi = code >> 1 and lo = code & 1: missing = lo & ~hi, count of A1 = 2 - hi - lo, of A2 = hi + lo.
// Sample map: sample[i] = the file's sample of individual i; a value outside 0 .. N-1 = not genotyped (missing for every
// marker, nothing is read for it); null = identity (N == n).
// Identity rows are read in ALIGNED 16-byte pieces whatever ld and the base address are, by the rule of scan.hip.h: a
// piece is fetched only when it holds at least one byte of the row, and the samples of foreign bytes are masked by their
// index.  The gathered form reads single bytes at row + (sample >> 2), for in-range samples only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "plan_types.h"
#include "scan.hip.h"

namespace scilmm {

constexpr int BED_A2 = 1;     // flags: the counted allele is A2 (g -> 2 - g for the observed)
constexpr int BED_LDG = 17;   // dwords per marker of its LDS image: 64 bytes (one gathered byte per individual of the tile; the
                              // identity form uses 2 pieces of 16 B) and one of padding -- an odd stride, as SCAN_LDG

// the genotype classes among the 16 samples of one packed word, `vm` = their low bits where the sample counts
__device__ __forceinline__ void bed_classes(uint32_t w, uint32_t vm, int& n00, int& n10, int& n11) {
  const uint32_t lo = w & vm, hi = (w >> 1) & vm;
  n00 += __popc(~hi & ~lo & vm);
  n10 += __popc(hi & ~lo);
  n11 += __popc(hi & lo);
}

// low bits of the samples of a packed word that exist: the word's first sample is s0 (may be negative), the row has N
__device__ __forceinline__ uint32_t bed_valid(int64_t s0, int64_t N) {
  uint32_t vm = 0x55555555u;
  if (s0 < 0) vm = s0 <= -16 ? 0u : vm & (~0u << (2 * (int)(-s0)));
  if (s0 + 16 > N) vm = s0 >= N ? 0u : vm & ((1u << (2 * (int)(N - s0))) - 1u);
  return vm;
}

// stats[0..2][c] as k_scan_moments writes them.  One workgroup per marker; a thread counts the three observed classes
// (integers), and the last thread standing forms sum and sum of squares from the counts: cnt = n00 + n10 + n11,
// sum = 2 n(two copies) + n10, sq = 4 n(two copies) + n10 -- the integers the int8 path adds up value by value.
__global__ __launch_bounds__(256) void k_bed_moments(int32_t n, int32_t N, const uint8_t* __restrict__ bed, int64_t ld,
                                                     const int32_t* __restrict__ sample, int32_t flags, int32_t r,
                                                     double* __restrict__ stats) {
  __shared__ long long red[4][3];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int c = blockIdx.x;
  const uint8_t* row = bed + (int64_t)c * ld;
  long long c00 = 0, c10 = 0, c11 = 0;
  if (sample) {
    // eight individuals in flight per thread (the byte read depends on the map's entry: two latencies per individual, and
    // a marker has one workgroup); 0x55 = missing stands in where nothing is read
    for (int64_t i = tid; i < n; i += 8 * 256) {
      uint32_t s[8], b[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) s[u] = i + 256 * u < n ? (uint32_t)sample[i + 256 * u] : ~0u;
#pragma unroll
      for (int u = 0; u < 8; ++u) b[u] = s[u] < (uint32_t)N ? row[s[u] >> 2] : 0x55u;
      int n00 = 0, n10 = 0, n11 = 0;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int code = (b[u] >> (2 * (s[u] & 3))) & 3;
        n00 += code == 0;
        n10 += code == 2;
        n11 += code == 3;
      }
      c00 += n00;
      c10 += n10;
      c11 += n11;
    }
  } else {
    const int head = (int)((uintptr_t)row & 15);  // bytes of the first piece that precede the row
    const int4* base = (const int4*)(row - head);
    const int64_t nb = ((int64_t)N + 3) >> 2;
    const int64_t npiece = ((int64_t)head + nb + 15) >> 4;
    for (int64_t k = tid; k < npiece; k += 256) {
      const int4 v = base[k];
      const int64_t s0 = 4 * (16 * k - head);  // sample of the piece's first bit pair
      int n00 = 0, n10 = 0, n11 = 0;
      bed_classes((uint32_t)v.x, bed_valid(s0, N), n00, n10, n11);
      bed_classes((uint32_t)v.y, bed_valid(s0 + 16, N), n00, n10, n11);
      bed_classes((uint32_t)v.z, bed_valid(s0 + 32, N), n00, n10, n11);
      bed_classes((uint32_t)v.w, bed_valid(s0 + 48, N), n00, n10, n11);
      c00 += n00;
      c10 += n10;
      c11 += n11;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    c00 += __shfl_down(c00, o);
    c10 += __shfl_down(c10, o);
    c11 += __shfl_down(c11, o);
  }
  if (lane == 0) {
    red[wv][0] = c00;
    red[wv][1] = c10;
    red[wv][2] = c11;
  }
  __syncthreads();
  if (tid == 0) {
    c00 = red[0][0] + red[1][0] + red[2][0] + red[3][0];
    c10 = red[0][1] + red[1][1] + red[2][1] + red[3][1];
    c11 = red[0][2] + red[1][2] + red[2][2] + red[3][2];
    const long long two = (flags & BED_A2) ? c11 : c00;  // observed with two copies of the counted allele
    const long long cnt = c00 + c10 + c11, sum = 2 * two + c10, sq = 4 * two + c10;
    const double mean = cnt > 0 ? (double)sum / (double)cnt : 0.0;
    stats[c] = (double)cnt;
    stats[(int64_t)r + c] = mean;
    stats[2 * (int64_t)r + c] = cnt > 0 ? (double)sq - (double)sum * mean : 0.0;
  }
}

// out[iperm[i]][c] as k_scan_dequant writes it, from packed rows.  A workgroup takes SCAN_TILE individuals of every marker
// into an LDS image [marker][byte]: in the identity form the tile's 16 packed bytes per marker (2 aligned pieces, the
// row's own misalignment kept as a byte offset), in the gathered form the byte of each individual's sample (0x55 = four
// missing codes for an individual that is not genotyped).  at[i] / sh[i] = byte of the image and shift of individual i's
// bit pair.  Then every wave writes whole rows of the block, 512 contiguous bytes per store, exactly as k_scan_dequant.
__global__ __launch_bounds__(256) void k_bed_dequant(int32_t n, int32_t N, int32_t r, int32_t rp, const uint8_t* __restrict__ bed,
                                                     int64_t ld, const int32_t* __restrict__ sample, int32_t flags,
                                                     const int32_t* __restrict__ iperm, const double* __restrict__ mean,
                                                     double* __restrict__ out) {
  __shared__ int32_t gs[RPMAX * BED_LDG];
  __shared__ double ms[RPMAX];
  __shared__ int32_t dst[SCAN_TILE];
  __shared__ int32_t src[SCAN_TILE];   // gathered form: the tile's samples, -1 = not genotyped
  __shared__ uint8_t at[SCAN_TILE], sh[SCAN_TILE];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t i0 = (int64_t)blockIdx.x * SCAN_TILE;
  const int ni = (int)min((int64_t)SCAN_TILE, (int64_t)n - i0);
  if (tid < RPMAX) ms[tid] = tid < r ? mean[tid] : 0.0;
  if (tid < SCAN_TILE) {
    dst[tid] = tid < ni ? iperm[i0 + tid] : 0;
    if (sample) {
      const uint32_t s = tid < ni ? (uint32_t)sample[i0 + tid] : ~0u;
      src[tid] = s < (uint32_t)N ? (int32_t)s : -1;
      at[tid] = (uint8_t)tid;
      sh[tid] = (uint8_t)(2 * (s & 3));
    } else {
      at[tid] = (uint8_t)(tid >> 2);
      sh[tid] = (uint8_t)(2 * (tid & 3));
    }
  }
  if (sample) {
    __syncthreads();
    uint8_t* gb = (uint8_t*)gs;
    // a wave per marker, a lane per individual: 64 byte reads inside one packed row
    const int32_t s = src[lane];
#pragma unroll 4
    for (int c = wv; c < r; c += 4)
      gb[c * (4 * BED_LDG) + lane] = s >= 0 ? bed[(int64_t)c * ld + (s >> 2)] : (uint8_t)0x55;
  } else {
    const int nbt = (ni + 3) >> 2;  // packed bytes of the tile
    for (int t = tid; t < 2 * r; t += 256) {
      const int c = t >> 1, k = t & 1;
      const uint8_t* p = bed + (int64_t)c * ld + (i0 >> 2);
      const int head = (int)((uintptr_t)p & 15);
      // piece k holds the tile's bytes 16 k - head .. 16 k - head + 15: fetched when one of them exists
      if (16 * k - head < nbt) {
        const int4 v = *(const int4*)(p - head + 16 * k);
        int32_t* g4 = gs + c * BED_LDG + 4 * k;
        g4[0] = v.x;
        g4[1] = v.y;
        g4[2] = v.z;
        g4[3] = v.w;
      }
    }
  }
  __syncthreads();
  const uint8_t* gb = (const uint8_t*)gs;
  const bool a2 = flags & BED_A2;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int c = lane + 64 * h;
    if (c >= rp) continue;
    const bool live = c < r;
    const int off = !live ? 0 : c * (4 * BED_LDG) + (sample ? 0 : (int)((uintptr_t)(bed + (int64_t)c * ld + (i0 >> 2)) & 15));
    const double m = ms[c];
    for (int i = wv; i < ni; i += 4) {
      const int code = live ? (gb[off + at[i]] >> sh[i]) & 3 : 1;
      const int hl = (code >> 1) + (code & 1);
      const int g = a2 ? hl : 2 - hl;
      out[(int64_t)dst[i] * rp + c] = code != 1 ? (double)g - m : 0.0;
    }
  }
}

}  // namespace scilmm
