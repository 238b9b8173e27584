// Device code shared by sample.hip (the fused token sampler) and beam.hip (the beam selector): a row of logits held in
// registers as monotone u32 keys, and the radix threshold search over them.
//
// Chunk layout: thread t of 1024 holds the 16-byte chunks t + 1024*j (8 elements each, slab j = 8192 consecutive
// elements), so element e of chunk j of thread t is index 8 * (t + 1024 * j) + e of the row. A key is the monotone u32
// image of an f32 (larger value <=> larger key; 0 = no element). select_key is four 8-bit radix passes from the top
// digit over the keys that share the prefix found so far, each adding the element's weight (1, or its integer mass)
// into a 256-bin LDS histogram with integer atomics; a bin has 16 copies (32 for counts) selected by the lane, so that
// a popular bin does not serialise a wave.
#pragma once
#include "dropout_mask.h"
#include "routes.h"

namespace {

constexpr int SM_THREADS = 1024;
constexpr int SM_WAVES = SM_THREADS / 64;
constexpr int SM_COPIES = 16;       // histogram copies per bin
constexpr int SM_MAX_N = 65536;
constexpr int SM_MAX_CPT = 8;       // chunks per thread at n = 65536
constexpr float SM_LOG2E = 1.44269504088896340736f;

struct SampleLds {
  unsigned long long hist[256 * SM_COPIES];
  unsigned long long binsum[256];
  unsigned long long wsum[SM_MAX_CPT][SM_WAVES];
  unsigned long long red[SM_WAVES];
  unsigned long long ctl[4];
  uint2 tab[256];                   // {TAB[i], TAB[i] - TAB[i+1]}
  uint32_t bitmap[SM_MAX_N / 32];   // token ids already in the row's history
};

__device__ __forceinline__ uint32_t key_of(float z) {
  if (!(z == z)) z = -INFINITY;  // NaN counts as -inf
  if (z == 0.f) z = 0.f;         // -0 and +0 are one value
  const uint32_t u = __float_as_uint(z);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float z_of(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// Chunk c (elements 8c .. 8c + 7) of row b of logits [B, ld] (bf16, or f32 when F32) as f32; elements at or past n
// read as 0 and are never loaded.
template <bool F32>
__device__ __forceinline__ void load_chunk(const void* logits, int b, long ld, int n, int c, float (&z)[8]) {
  const int i0 = 8 * c;
  if (i0 + 8 <= n) {
    if (F32) {
      const float* src = (const float*)logits + (long)b * ld + i0;
      const float4 v0 = *reinterpret_cast<const float4*>(src);
      const float4 v1 = *reinterpret_cast<const float4*>(src + 4);
      z[0] = v0.x; z[1] = v0.y; z[2] = v0.z; z[3] = v0.w;
      z[4] = v1.x; z[5] = v1.y; z[6] = v1.z; z[7] = v1.w;
    } else {
      load8((const bf16_t*)logits + (long)b * ld + i0, z);
    }
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      z[e] = 0.f;
      if (i0 + e < n)
        z[e] = F32 ? ((const float*)logits)[(long)b * ld + i0 + e] : bf2f(((const bf16_t*)logits)[(long)b * ld + i0 + e]);
    }
  }
}

// Integer mass of an element: floor-interpolated 2^31 * 2^-t, t = (m - z) * log2(e); 0 outside [0, 40) (and for key 0,
// whose z reads as NaN). The key goes through an empty asm so that every pass computes its masses anew: otherwise the
// optimiser keeps each element's decoded logit and mass intermediates alive from one pass to the next, and a dozen live
// values per chunk beside the keys overflow the register file into scratch.
__device__ __forceinline__ uint32_t mass_of(uint32_t k, float m, const uint2* tab) {
  asm volatile("" : "+v"(k));
  const float t = (m - z_of(k)) * SM_LOG2E;
  if (!(t >= 0.f && t < 40.f)) return 0u;
  const uint32_t F = (uint32_t)floorf(t * 65536.f);
  const uint32_t e = F >> 16, idx = (F >> 8) & 255u, rem = F & 255u;
  const uint2 p = tab[idx];
  const uint32_t v = p.x - ((p.y * rem) >> 8);
  return e >= 32u ? 0u : (v >> e);
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned long long block_sum_u64(unsigned long long v, unsigned long long* red) {
  v = wave_sum_u64(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned long long t = 0;
#pragma unroll
  for (int i = 0; i < SM_WAVES; ++i) t += red[i];
  return t;
}
// max (MAX) or min of a u32 over the block
template <bool MAX>
__device__ __forceinline__ uint32_t block_ext_u32(uint32_t v, unsigned long long* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t w = __shfl_xor(v, o, 64);
    v = MAX ? (w > v ? w : v) : (w < v ? w : v);
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t t = (uint32_t)red[0];
#pragma unroll
  for (int i = 1; i < SM_WAVES; ++i) {
    const uint32_t w = (uint32_t)red[i];
    t = MAX ? (w > t ? w : t) : (w < t ? w : t);
  }
  return t;
}

// The largest key v with sum{weight_i : key_i >= v} >= need, over the elements with key >= floor_key; weight is 1
// (MASS = false) or the element's mass. need >= 1 and at most the total weight. Block-uniform result.
template <int CPT, bool MASS>
__device__ __forceinline__ uint32_t select_key(const uint32_t (&key)[CPT][8], unsigned long long need,
                                               uint32_t floor_key, float m, SampleLds& s) {
  const int tid = threadIdx.x, lane = tid & 63;
  uint32_t* hist32 = reinterpret_cast<uint32_t*>(s.hist);
  uint32_t prefix = 0;
  for (int p = 3; p >= 0; --p) {
    const int sh = 8 * p;
    const uint32_t hi_mask = p == 3 ? 0u : (0xffffffffu << (sh + 8));
    for (int i = tid; i < 256 * SM_COPIES; i += SM_THREADS) s.hist[i] = 0;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const uint32_t k = key[j][e];
        if (((k ^ prefix) & hi_mask) == 0u && k >= floor_key) {
          if (MASS) {
            const unsigned long long w = mass_of(k, m, s.tab);
            if (w) atomicAdd(&s.hist[((k >> sh) & 255u) * SM_COPIES + (lane & (SM_COPIES - 1))], w);
          } else {  // counts fit 32 bits: twice the copies in the same bytes
            atomicAdd(&hist32[((k >> sh) & 255u) * (2 * SM_COPIES) + (lane & (2 * SM_COPIES - 1))], 1u);
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();
    {  // 4 threads per bin, 4 copies each
      const int bin = tid >> 2, part = tid & 3;
      unsigned long long t = 0;
      if (MASS) {
#pragma unroll
        for (int c = 0; c < SM_COPIES / 4; ++c) t += s.hist[bin * SM_COPIES + part * (SM_COPIES / 4) + c];
      } else {
#pragma unroll
        for (int c = 0; c < SM_COPIES / 2; ++c) t += hist32[bin * (2 * SM_COPIES) + part * (SM_COPIES / 2) + c];
      }
      t += __shfl_xor(t, 1, 64);
      t += __shfl_xor(t, 2, 64);
      if (part == 0) s.binsum[bin] = t;
    }
    __syncthreads();
    if (tid < 64) {  // bins from the top: lane l owns bins 255 - 4l .. 252 - 4l
      unsigned long long loc[4], tot = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        loc[i] = s.binsum[255 - 4 * lane - i];
        tot += loc[i];
      }
      unsigned long long inc = tot;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long y = __shfl_up(inc, o, 64);
        if (lane >= o) inc += y;
      }
      unsigned long long run = inc - tot, above = 0;
      int bsel = -1;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (bsel < 0 && run + loc[i] >= need) {
          bsel = 255 - 4 * lane - i;
          above = run;
        }
        run += loc[i];
      }
      const unsigned long long found = __ballot(bsel >= 0);
      if (found == 0ull) {  // not reachable while need <= total weight: keep the lowest digit
        if (lane == 0) {
          s.ctl[0] = prefix;
          s.ctl[1] = need;
        }
      } else if (lane == __ffsll((long long)found) - 1) {
        s.ctl[0] = prefix | ((uint32_t)bsel << sh);
        s.ctl[1] = need - above;
      }
    }
    __syncthreads();
    prefix = (uint32_t)s.ctl[0];
    need = s.ctl[1];
  }
  return prefix;
}

}  // namespace
