// Token sampler of GPT2.generate: repetition penalty, temperature, top-k, top-p and the draw in one launch, one block
// per row of logits (ops/sample.py states the rule and holds its host replica; the two agree bit for bit).
//
// The row is read once into registers: thread t of 1024 holds the 16-byte chunks t + 1024*j (8 elements each, slab j =
// 8192 consecutive elements), as the monotone u32 image of the scaled logit (larger logit <=> larger key; 0 = no
// element). Every later pass runs from those registers with compile-time indices. Both threshold searches (k-th largest
// by count, nucleus by mass) are one routine: four 8-bit radix passes from the top digit over the keys that share the
// prefix found so far, each adding the element's weight (1, or its integer mass) into a 256-bin LDS histogram with
// integer atomics; a bin has 16 copies (32 for counts) selected by the lane, so that a popular bin does not serialise
// a wave. Masses are integers (a 2^-t table in LDS, linear interpolation in integer arithmetic), so no sum depends on
// its order; the only floating-point operations are single f32 multiplies and subtractions. The draw walks the index
// order exactly: slab totals, then the waves of the slab, then a lane scan, then the 8 elements of one chunk.
#include "dropout_mask.h"
#include "routes.h"

namespace {

constexpr int SM_THREADS = 1024;
constexpr int SM_WAVES = SM_THREADS / 64;
constexpr int SM_COPIES = 16;       // histogram copies per bin
constexpr int SM_MAX_N = 65536;
constexpr int SM_MAX_CPT = 8;       // chunks per thread at n = 65536
constexpr float SM_LOG2E = 1.44269504088896340736f;

struct SampleArgs {
  const void* logits;
  long ld;
  int n;
  float inv_t;
  int greedy;
  int top_k;   // 0: off
  int P;       // round(p * 65536), < 0: off
  float r, inv_r;
  int penalty;
  unsigned long long seed;
  const long* uniform;  // [B] values in [0, 2^32) replacing the hash draw, or null
  const long* tab;      // [257] round(2^31 * 2^(-j/256))
  long* out;
  long width;
  long* pos;
  unsigned char* done;
  long eos, pad;
  long* tok_out;
};

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

template <int CPT, bool F32>
__global__ void __launch_bounds__(SM_THREADS) sample_kernel(SampleArgs a) {
  __shared__ SampleLds s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const int n = a.n;

  // ---- history of the row -> bitmap; mass table -> LDS
  long p0 = a.pos[b];
  if (tid < 256) {
    const uint32_t t0 = (uint32_t)a.tab[tid], t1 = (uint32_t)a.tab[tid + 1];
    s.tab[tid] = make_uint2(t0, t0 - t1);
  }
  if (a.penalty) {
    for (int i = tid; i < SM_MAX_N / 32; i += SM_THREADS) s.bitmap[i] = 0u;
    __syncthreads();
    long hist_n = p0 < 0 ? 0 : (p0 > a.width ? a.width : p0);
    const long* row = a.out + (long)b * a.width;
    for (long i = tid; i < hist_n; i += SM_THREADS) {
      const long id = row[i];
      if (id >= 0 && id < n) atomicOr(&s.bitmap[id >> 5], 1u << (id & 31));
    }
  }
  __syncthreads();

  // ---- the row, once
  uint32_t key[CPT][8];
#pragma unroll
  for (int j = 0; j < CPT; ++j) {
    const int c = tid + SM_THREADS * j;
    const int i0 = 8 * c;
    float z[8];
    if (i0 + 8 <= n) {
      if (F32) {
        const float* src = (const float*)a.logits + (long)b * a.ld + i0;
        const float4 v0 = *reinterpret_cast<const float4*>(src);
        const float4 v1 = *reinterpret_cast<const float4*>(src + 4);
        z[0] = v0.x; z[1] = v0.y; z[2] = v0.z; z[3] = v0.w;
        z[4] = v1.x; z[5] = v1.y; z[6] = v1.z; z[7] = v1.w;
      } else {
        load8((const bf16_t*)a.logits + (long)b * a.ld + i0, z);
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        z[e] = 0.f;
        if (i0 + e < n)
          z[e] = F32 ? ((const float*)a.logits)[(long)b * a.ld + i0 + e]
                     : bf2f(((const bf16_t*)a.logits)[(long)b * a.ld + i0 + e]);
      }
    }
    uint32_t bits = 0u;
    if (a.penalty && i0 < n) bits = (s.bitmap[c >> 2] >> (8 * (c & 3))) & 255u;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float v = z[e];
      if ((bits >> e) & 1u) v = v > 0.f ? v * a.inv_r : v * a.r;
      if (!a.greedy) v = v * a.inv_t;
      key[j][e] = i0 + e < n ? key_of(v) : 0u;
    }
  }

  // ---- the maximum (always kept)
  uint32_t kmax = 0u;
#pragma unroll
  for (int j = 0; j < CPT; ++j)
#pragma unroll
    for (int e = 0; e < 8; ++e) kmax = key[j][e] > kmax ? key[j][e] : kmax;
  kmax = block_ext_u32<true>(kmax, s.red);

  uint32_t tok = 0u;
  if (a.greedy) {
    uint32_t first = 0xffffffffu;
#pragma unroll
    for (int j = CPT - 1; j >= 0; --j)
#pragma unroll
      for (int e = 7; e >= 0; --e)
        if (key[j][e] == kmax) first = (uint32_t)(8 * (tid + SM_THREADS * j) + e);
    tok = block_ext_u32<false>(first, s.red);
  } else {
    const float m = z_of(kmax);
    uint32_t thr = 1u;  // every element
    if (a.top_k > 0) thr = select_key<CPT, false>(key, (unsigned long long)a.top_k, 1u, m, s);
    if (a.P >= 0) {
      unsigned long long w = 0;
#pragma unroll
      for (int j = 0; j < CPT; ++j) {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (key[j][e] >= thr) w += mass_of(key[j][e], m, s.tab);
        __builtin_amdgcn_sched_barrier(0);
      }
      const unsigned long long W = block_sum_u64(w, s.red);
      if (W) {
        unsigned long long need = ((unsigned long long)a.P * W + 65535ull) >> 16;
        if (need < 1ull) need = 1ull;  // the maximum is always kept
        thr = select_key<CPT, true>(key, need, thr, m, s);
      }
    }
    // ---- the draw, in index order: slabs, waves of the slab, lanes of the wave, elements of the chunk
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
      unsigned long long w = 0;
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (key[j][e] >= thr) w += mass_of(key[j][e], m, s.tab);
      const unsigned long long t = wave_sum_u64(w);
      if (lane == 0) s.wsum[j][wave] = t;
      __builtin_amdgcn_sched_barrier(0);  // one chunk's temporaries at a time: the keys fill the register file
    }
    __syncthreads();
    if (tid == 0) {
      unsigned long long U;
      if (a.uniform) {
        U = (unsigned long long)a.uniform[b] & 0xffffffffull;
      } else {
        const unsigned long long G = 0x9E3779B97F4A7C15ull;
        U = mix64(mix64(a.seed + G * (unsigned long long)(b + 1)) + G * (unsigned long long)(p0 + 1)) >> 32;
      }
      unsigned long long Wk = 0;
      for (int j = 0; j < CPT; ++j)
        for (int w = 0; w < SM_WAVES; ++w) Wk += s.wsum[j][w];
      const unsigned long long target = __umul64hi(U << 32, Wk);
      unsigned long long run = 0;
      int J = -1, wv = 0;
      for (int j = 0; j < CPT && J < 0; ++j)
        for (int w = 0; w < SM_WAVES; ++w) {
          const unsigned long long x = s.wsum[j][w];
          if (run + x > target) {
            J = j;
            wv = w;
            break;
          }
          run += x;
        }
      s.ctl[0] = Wk ? (unsigned long long)J : ~0ull;  // J < 0 only when Wk == 0
      s.ctl[1] = (unsigned long long)wv;
      s.ctl[2] = target - run;                         // what remains inside wave wv of slab J
      s.ctl[3] = 0ull;                                 // the token (0 when nothing has mass)
    }
    __syncthreads();
    const int J = (int)(long long)s.ctl[0];
    if (J >= 0 && wave == (int)s.ctl[1]) {
      const unsigned long long rem = s.ctl[2];
      uint32_t kj[8], q[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) kj[e] = 0u;
#pragma unroll
      for (int j = 0; j < CPT; ++j)
#pragma unroll
        for (int e = 0; e < 8; ++e) kj[e] = j == J ? key[j][e] : kj[e];
      unsigned long long mine = 0;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        q[e] = kj[e] >= thr ? mass_of(kj[e], m, s.tab) : 0u;
        mine += q[e];
      }
      unsigned long long inc = mine;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long y = __shfl_up(inc, o, 64);
        if (lane >= o) inc += y;
      }
      if (inc - mine <= rem && rem < inc) {  // exactly one lane
        unsigned long long run = inc - mine;
        uint32_t got = 0xffffffffu;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          run += q[e];
          if (got == 0xffffffffu && run > rem) got = (uint32_t)(8 * (tid + SM_THREADS * J) + e);
        }
        s.ctl[3] = got;
      }
    }
    __syncthreads();
    tok = (uint32_t)s.ctl[3];
  }

  // ---- bookkeeping of the row: this block is the only reader and writer of pos[b], done[b] and out[b, :]
  if (tid == 0) {
    long t = (long)tok;
    unsigned char d = a.done[b];
    if (d) t = a.pad;
    if (a.eos >= 0 && t == a.eos) d = 1;
    a.done[b] = d;
    if (p0 >= 0 && p0 < a.width) a.out[(long)b * a.width + p0] = t;
    a.pos[b] = p0 + 1;
    a.tok_out[b] = t;
  }
}

}  // namespace

// One token per row of logits [B, ld] (bf16, or f32 when f32 != 0; the first n entries of a row count), by the rule of
// ops/sample.py. top_k 0 and P < 0 switch the two filters off; greedy ignores both and the temperature. out [B, width],
// pos [B], tok_out [B] int64; done [B] bytes.
DTF_API int dtf_sample_logits(const void* logits, int f32, long ld, int B, int n, float inv_t, int greedy, int top_k,
                              int P, float r, float inv_r, unsigned long long seed, const long* uniform,
                              const long* tab, long* out, long width, long* pos, unsigned char* done, long eos,
                              long pad, long* tok_out, void* stream) {
  if (!logits || !tab || !out || !pos || !done || !tok_out) return -1;
  if (B < 1 || n < 1 || n > SM_MAX_N || ld < n || (ld & 7) || width < 0 || !aligned16(logits)) return -1;
  if (top_k < 0 || P > 65535 || !(r > 0.f)) return -1;
  SampleArgs a;
  a.logits = logits;
  a.ld = ld;
  a.n = n;
  a.inv_t = inv_t;
  a.greedy = greedy ? 1 : 0;
  a.top_k = top_k >= n ? 0 : top_k;
  a.P = P;
  a.r = r;
  a.inv_r = inv_r;
  a.penalty = r != 1.f;
  a.seed = seed;
  a.uniform = uniform;
  a.tab = tab;
  a.out = out;
  a.width = width;
  a.pos = pos;
  a.done = done;
  a.eos = eos;
  a.pad = pad;
  a.tok_out = tok_out;
  hipStream_t st = (hipStream_t)stream;
  const int chunks = cdiv(n, 8 * SM_THREADS);
#define SAMPLE(C)                                                                                        \
  do {                                                                                                   \
    if (f32)                                                                                             \
      hipLaunchKernelGGL((sample_kernel<C, true>), dim3(B), dim3(SM_THREADS), 0, st, a);                 \
    else                                                                                                 \
      hipLaunchKernelGGL((sample_kernel<C, false>), dim3(B), dim3(SM_THREADS), 0, st, a);                \
  } while (0)
  if (chunks <= 1) SAMPLE(1);
  else if (chunks <= 2) SAMPLE(2);
  else if (chunks <= 4) SAMPLE(4);
  else if (chunks <= 7) SAMPLE(7);
  else SAMPLE(8);
#undef SAMPLE
  count_launch(LC_SAMPLE);
  return (int)hipGetLastError();
}
