// Kernels of the marker scan from imputed dosages (scilmm_scan_block_dosage_dev, engine.hip): the two streaming kernels of
// scan.hip.h for expected allele counts in [0, 2] instead of hard calls, in two element types, with the sample map of
// bed.hip.h.  What follows them (forward sweep, k_scan_stats, k_scan_fold, k_scan_gram) is shared with the int8 path.
//   k_dos_moments<T> : per marker n_obs, mean, centred sum of squares        reads  r * N * sizeof(T) (+ the map; f32 twice)
//   k_dos_dequant<T> : W = P (g - mean), missing = 0, columns padded to rp   reads  r * N * sizeof(T), writes n * rp * 8
// No atomics of any kind, one writer per entry of W.
//
// Layout (marker-major): marker j = dos + j * ld ELEMENTS, N samples.
//   uint16_t (SCILMM_DOSAGE_U16): PLINK 2's fixed point, 16384 = 1.0, 32768 = 2.0; any code above 32768 = missing (65535 is
//     the canonical one).  The moments are INTEGER sums of the codes (count, sum, sum of squares, 64-bit), so their order
//     is immaterial; mean, css and W come from them by power-of-two scalings (exact) and the two expressions of
//     k_scan_moments, mean = sum / cnt and css = sq - sum * mean: a marker of hard calls g * 16384 gives the doubles of the
//     int8 path, bit for bit.  A constant marker has css == 0 exactly: cnt * v / cnt is v, and sq and sum * mean round the
//     same real number -- as long as (double)sq is exact, cnt * v^2 < 2^53: any cohort below 2^23 observed individuals
//     (beyond it sq is rounded before the fused sq - sum * mean, and a constant marker may get a css of rounding size).
//     For fractional dosages this css is the one-pass form and loses about sq / css digits: row 2 of the uint16 statistics
//     is the zero test css == 0 and nothing more; the float form is the one that computes css to working accuracy.
//   float (SCILMM_DOSAGE_F32): a non-finite value = missing, any finite value is taken as it is.  The sums are fp64 in a
//     FIXED order: a thread adds its elements in ascending order, the 64 threads of a wave and then the 4 waves are folded
//     by a fixed tree, so a call repeats its bits (the order depends on N and on where the row starts within its 16-byte
//     piece; with a map on n alone).  mean = sum / cnt; css is a SECOND pass, sum of (g - mean)^2 (the one-pass form loses
//     sq / css digits where mean >> sd), forced to exactly 0 when the smallest observed value equals the largest (n v / n
//     need not round back to v): a constant marker is recognised as a monomorphic int8 marker is.
// Sample map: sample[i] = the file's sample of individual i; a value outside 0 .. N-1 = not genotyped (missing for every
// marker, nothing is read for it); null = identity (N == n).
// Identity rows are read in ALIGNED 16-byte pieces whatever ld and the (element-aligned) base address are, by the rule of
// scan.hip.h: a piece is fetched only when it holds at least one byte of the row, and foreign elements are masked by their
// index.  The gathered form reads single elements at row + sample, for in-range samples only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "plan_types.h"
#include "scan.hip.h"

namespace scilmm {

constexpr int DOS_FLIGHT = 8;             // gathered moments: individuals a thread keeps in flight, as k_bed_moments
constexpr int DOS_PIECES = 4;             // identity moments / dequant: 16-byte pieces a thread keeps in flight

template <class T>
struct Dos {
  static constexpr int PER = 16 / (int)sizeof(T);               // elements per 16-byte piece
  static constexpr int NP = SCAN_TILE / PER + 1;                // pieces of a tile of one marker: SCAN_TILE elements + 15 bytes
  // dwords per marker of its LDS image: NP pieces and one of padding -- an odd stride (37 / 69), as SCAN_LDG
  static constexpr int LDG = 4 * NP + 1;
  static constexpr int EL = LDG * 4 / (int)sizeof(T);           // the same stride in elements
  static_assert(LDG % 2 == 1, "odd dword stride");
};

__device__ __forceinline__ uint16_t dos_missing(uint16_t) { return 65535; }
__device__ __forceinline__ float dos_missing(float) { return __uint_as_float(0x7fc00000u); }
__device__ __forceinline__ bool dos_observed(uint16_t v) { return v <= 32768; }
__device__ __forceinline__ bool dos_observed(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ double dos_value(uint16_t v) { return ldexp((double)v, -14); }
__device__ __forceinline__ double dos_value(float v) { return (double)v; }

__device__ __forceinline__ uint32_t dos_word(const int4& v, int w) {
  return (uint32_t)(w == 0 ? v.x : w == 1 ? v.y : w == 2 ? v.z : v.w);
}
template <class T>
__device__ __forceinline__ T dos_elem(const int4& v, int j) {
  if constexpr (std::is_same<T, float>::value)
    return __uint_as_float(dos_word(v, j));
  else
    return (uint16_t)(dos_word(v, j >> 1) >> (16 * (j & 1)));
}

// f(v) for the elements of one marker that thread `tid` of 256 owns, in a fixed order.  Identity (sample == null): the
// pieces tid, tid + 256, ... of the row, each element by element, DOS_PIECES loads in flight; gathered: the individuals
// tid, tid + 256, ..., DOS_FLIGHT in flight, the missing value where nothing is read.
template <class T, class F>
__device__ __forceinline__ void dos_visit(const T* __restrict__ row, int32_t n, int32_t N, const int32_t* __restrict__ sample,
                                          int tid, F f) {
  constexpr int PER = Dos<T>::PER;
  if (sample) {
    for (int64_t i = tid; i < n; i += DOS_FLIGHT * 256) {
      uint32_t s[DOS_FLIGHT];
      T v[DOS_FLIGHT];
#pragma unroll
      for (int u = 0; u < DOS_FLIGHT; ++u) s[u] = i + 256 * u < n ? (uint32_t)sample[i + 256 * u] : ~0u;
#pragma unroll
      for (int u = 0; u < DOS_FLIGHT; ++u) v[u] = s[u] < (uint32_t)N ? row[s[u]] : dos_missing(T());
#pragma unroll
      for (int u = 0; u < DOS_FLIGHT; ++u) f(v[u]);
    }
  } else {
    const int head = (int)((uintptr_t)row & 15);  // bytes of the first piece that precede the row
    const int4* base = (const int4*)((const char*)row - head);
    const int64_t e0 = head / (int)sizeof(T);     // ... and elements
    const int64_t npiece = (e0 + N + PER - 1) / PER;
    for (int64_t k = tid; k < npiece; k += DOS_PIECES * 256) {
      int4 v[DOS_PIECES];
#pragma unroll
      for (int u = 0; u < DOS_PIECES; ++u) v[u] = k + 256 * u < npiece ? base[k + 256 * u] : make_int4(0, 0, 0, 0);
#pragma unroll
      for (int u = 0; u < DOS_PIECES; ++u) {
        if (k + 256 * u >= npiece) break;
        const int64_t i0 = PER * (k + 256 * u) - e0;  // sample of the piece's first element
#pragma unroll
        for (int j = 0; j < PER; ++j)
          if (i0 + j >= 0 && i0 + j < N) f(dos_elem<T>(v[u], j));
      }
    }
  }
}

// the 256 threads' values folded by a fixed tree: shuffles inside a wave, then the four waves in wave order; every thread
// gets the result.  `red` is one slot per wave; the two barriers make it reusable by the next call.
template <class V, class Op>
__device__ __forceinline__ V dos_fold(V x, V* red, int lane, int wv, Op op) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = op(x, __shfl_down(x, o));
  if (lane == 0) red[wv] = x;
  __syncthreads();
  x = op(op(op(red[0], red[1]), red[2]), red[3]);
  __syncthreads();
  return x;
}

// stats[0..2][c] as k_scan_moments writes them.  One workgroup per marker.
template <class T>
__global__ __launch_bounds__(256) void k_dos_moments(int32_t n, int32_t N, const T* __restrict__ dos, int64_t ld,
                                                     const int32_t* __restrict__ sample, int32_t r, double* __restrict__ stats) {
  __shared__ long long redi[4];
  __shared__ double redd[4];
  __shared__ float redf[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int c = blockIdx.x;
  const T* row = dos + (int64_t)c * ld;
  const auto addi = [](long long a, long long b) { return a + b; };
  const auto addd = [](double a, double b) { return a + b; };
  long long cnt = 0;
  if constexpr (std::is_same<T, uint16_t>::value) {
    long long sum = 0, sq = 0;
    dos_visit<T>(row, n, N, sample, tid, [&](uint16_t v) {
      const bool ok = dos_observed(v);
      cnt += ok ? 1 : 0;
      sum += ok ? (long long)v : 0;
      sq += ok ? (long long)v * v : 0;
    });
    cnt = dos_fold(cnt, redi, lane, wv, addi);
    sum = dos_fold(sum, redi, lane, wv, addi);
    sq = dos_fold(sq, redi, lane, wv, addi);
    if (tid == 0) {
      // the sums in allele counts: power-of-two scalings, exact (ldexp, not a product that could fuse with what follows)
      const double dsum = ldexp((double)sum, -14), dsq = ldexp((double)sq, -28);
      const double mean = cnt > 0 ? dsum / (double)cnt : 0.0;
      stats[c] = (double)cnt;
      stats[(int64_t)r + c] = mean;
      stats[2 * (int64_t)r + c] = cnt > 0 ? dsq - dsum * mean : 0.0;
    }
  } else {
    double sum = 0.0;
    float lo = __uint_as_float(0x7f800000u), hi = __uint_as_float(0xff800000u);
    dos_visit<T>(row, n, N, sample, tid, [&](float v) {
      if (dos_observed(v)) {
        cnt += 1;
        sum += (double)v;
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
      }
    });
    cnt = dos_fold(cnt, redi, lane, wv, addi);
    sum = dos_fold(sum, redd, lane, wv, addd);
    lo = dos_fold(lo, redf, lane, wv, [](float a, float b) { return fminf(a, b); });
    hi = dos_fold(hi, redf, lane, wv, [](float a, float b) { return fmaxf(a, b); });
    const double mean = cnt > 0 ? sum / (double)cnt : 0.0;
    // second pass over the row just read: the centred squares, in the same fixed order
    double css = 0.0;
    dos_visit<T>(row, n, N, sample, tid, [&](float v) {
      if (dos_observed(v)) {
        const double d = (double)v - mean;
        css += d * d;
      }
    });
    css = dos_fold(css, redd, lane, wv, addd);
    if (tid == 0) {
      stats[c] = (double)cnt;
      stats[(int64_t)r + c] = mean;
      stats[2 * (int64_t)r + c] = (cnt > 0 && lo != hi) ? css : 0.0;
    }
  }
}

// out[iperm[i]][c] as k_scan_dequant writes it, from dosage rows.  A workgroup takes SCAN_TILE individuals of every marker
// into an LDS image [marker][element] of stride Dos<T>::LDG dwords: in the identity form the tile's aligned pieces (the
// row's own misalignment kept as an element offset), in the gathered form the element of each individual's sample (the
// missing value for an individual that is not genotyped).  Then every wave writes whole rows of the block, 512 contiguous
// bytes per store, exactly as k_scan_dequant: lane = marker, so the 32 lanes of a half read 32 different banks.
template <class T>
__global__ __launch_bounds__(256) void k_dos_dequant(int32_t n, int32_t N, int32_t r, int32_t rp, const T* __restrict__ dos,
                                                     int64_t ld, const int32_t* __restrict__ sample,
                                                     const int32_t* __restrict__ iperm, const double* __restrict__ mean,
                                                     double* __restrict__ out) {
  constexpr int NP = Dos<T>::NP, LDG = Dos<T>::LDG, EL = Dos<T>::EL;
  __shared__ int32_t gs[RPMAX * LDG];
  __shared__ double ms[RPMAX];
  __shared__ int32_t dst[SCAN_TILE];
  __shared__ int32_t src[SCAN_TILE];   // gathered form: the tile's samples, -1 = not genotyped
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t i0 = (int64_t)blockIdx.x * SCAN_TILE;
  const int ni = (int)min((int64_t)SCAN_TILE, (int64_t)n - i0);
  if (tid < RPMAX) ms[tid] = tid < r ? mean[tid] : 0.0;
  if (tid < SCAN_TILE) {
    dst[tid] = tid < ni ? iperm[i0 + tid] : 0;
    if (sample) {
      const uint32_t s = tid < ni ? (uint32_t)sample[i0 + tid] : ~0u;
      src[tid] = s < (uint32_t)N ? (int32_t)s : -1;
    }
  }
  T* ge = (T*)gs;
  if (sample) {
    __syncthreads();
    // a wave per marker, a lane per individual: 64 element reads inside one row
    const int32_t s = src[lane];
#pragma unroll 4
    for (int c = wv; c < r; c += 4) ge[c * EL + lane] = s >= 0 ? dos[(int64_t)c * ld + s] : dos_missing(T());
  } else {
    const int nbt = ni * (int)sizeof(T);  // bytes of the tile in a row
    for (int t0 = tid; t0 < NP * r; t0 += DOS_PIECES * 256) {
      int4 v[DOS_PIECES];
#pragma unroll
      for (int u = 0; u < DOS_PIECES; ++u) {
        const int t = t0 + 256 * u, c = t / NP, k = t - NP * c;
        const char* p = (const char*)(dos + (int64_t)c * ld + i0);
        const int head = (int)((uintptr_t)p & 15);
        // piece k holds the tile's bytes 16 k - head .. 16 k - head + 15: fetched when one of them exists
        v[u] = (t < NP * r && 16 * k - head < nbt) ? *(const int4*)(p - head + 16 * k) : make_int4(0, 0, 0, 0);
      }
#pragma unroll
      for (int u = 0; u < DOS_PIECES; ++u) {
        const int t = t0 + 256 * u, c = t / NP, k = t - NP * c;
        if (t >= NP * r) break;
        int32_t* g4 = gs + c * LDG + 4 * k;
        g4[0] = v[u].x;
        g4[1] = v[u].y;
        g4[2] = v[u].z;
        g4[3] = v[u].w;
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int c = lane + 64 * h;
    if (c >= rp) continue;
    const bool live = c < r;
    const int off = !live ? 0 : c * EL + (sample ? 0 : (int)((uintptr_t)(dos + (int64_t)c * ld + i0) & 15) / (int)sizeof(T));
    const double m = ms[c];
    for (int i = wv; i < ni; i += 4) {
      const T g = live ? ge[off + i] : dos_missing(T());
      out[(int64_t)dst[i] * rp + c] = dos_observed(g) ? dos_value(g) - m : 0.0;
    }
  }
}

}  // namespace scilmm
