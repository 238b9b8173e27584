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
// The keys, the chunk layout and the threshold search live in sample_core.h (beam.hip selects with them too).
#include "sample_core.h"

namespace {

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
    load_chunk<F32>(a.logits, b, a.ld, n, c, z);
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
