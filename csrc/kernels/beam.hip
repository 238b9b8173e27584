// Beam search of GPT2.generate(num_beams=G): the selection of the G best continuations of a group of G beams
// (dtf_beam_select) and the bookkeeping that lets a beam continue another beam's history without moving any K/V
// (dtf_beam_reorder). ops/beam.py states the rule and holds the torch reference.
//
// Candidates of group g: for a live beam j every token v < n with value scores[j] + (logits[j, v] - lse_j), lse_j the
// log-sum-exp of the row's n entries; for a done beam the single pair (j, pad) with value scores[j]. All f32. The G
// largest values win, ties to the smaller j * n + v, written in descending order. Two launches, no floating-point
// atomics, every reduction in a fixed order: the same inputs give the same bits.
//
// Stage 1, one block of 1024 threads per row: the row is read once into registers in the sampler's chunk layout
// (sample_core.h), first as f32 bits for the maximum and the sum of exponentials (thread, then wave butterfly, then
// the 16 waves in order), then in place as the monotone u32 keys of the values. A row contributes at most G winners:
// the G-th largest key is found by the sampler's radix threshold search, the fewer than G keys above it are collected
// through an LDS counter, and the remaining places go to the smallest indices that hold the threshold key, one block
// minimum each. The G (key, token) pairs are ranked among themselves and written to scratch in descending order. A
// done row writes its one candidate (token bit 31 marks it) and G - 1 empty pairs (key 0 = no candidate: below the
// key of -inf, which is a legal value). Up to 4 chunks a thread (n <= 32768) everything stays in registers; the 7- and
// 8-chunk instances (the GPT-2 vocabulary is the 7-chunk one) hit the 128-VGPR limit of a 1024-thread block inside the
// threshold search and spill 60 to 150 bytes of scratch per thread, which the sampler's instances of the same search
// do not.
//
// Stage 2, one wave per group: the G * G <= 256 pairs, four per lane, as u64 (key, ~index) in LDS; a candidate's place
// is the number of candidates larger than it (all-pairs count, no order of evaluation to depend on), and the places
// 0 .. G-1 write score, parent, token and done. Stage 2 reads nothing but the scratch, so scores and done are updated
// in place.
//
// dtf_beam_reorder, one thread per (group, column p): a column of the slot table [B0*G, capacity] (uint8: which
// physical row of the group holds row b's key at position p) and of the token history [B0*G, width] is gathered by
// parent; the thread loads the column's G entries before it stores any, so the update is in place. The column that
// the previous step closed (p = L - 1, L the group's length; each row stored that position in its own physical row)
// becomes parent[j]; columns from L on are not touched (the history's column L receives the new tokens).
#include "sample_core.h"

namespace {

constexpr int BM_MAX_G = 16;
constexpr uint32_t BM_DONE = 0x80000000u;  // token field of a candidate: the beam it comes from is done

struct BeamArgs {
  const void* logits;
  long ld;
  int n, G;
  const float* scores;
  const unsigned char* done;
  uint32_t pad;
  uint2* cand;  // [B0*G][G] (key of the value, token)
};

template <int CPT, bool F32>
__global__ void __launch_bounds__(SM_THREADS) beam_row_kernel(BeamArgs a) {
  __shared__ SampleLds s;
  __shared__ float fsum[SM_WAVES];
  __shared__ uint2 win[BM_MAX_G];
  __shared__ int nwin;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const int n = a.n, G = a.G;
  uint2* cand = a.cand + (long)b * G;
  const float score = a.scores[b];
  if (a.done[b]) {  // (block-uniform)
    if (tid < G) cand[tid] = tid == 0 ? make_uint2(key_of(score), a.pad | BM_DONE) : make_uint2(0u, 0u);
    return;
  }

  // ---- the row, once: f32 bits, entries past n and NaN as -inf
  uint32_t key[CPT][8];
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < CPT; ++j) {
    int c = tid + SM_THREADS * j;
    asm volatile("" : "+v"(c));  // addresses are formed chunk by chunk, not all of them ahead of the first load
    float z[8];
    load_chunk<F32>(a.logits, b, a.ld, n, c, z);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float v = (8 * c + e < n && z[e] == z[e]) ? z[e] : -INFINITY;
      key[j][e] = __float_as_uint(v);
      m = fmaxf(m, v);
    }
    __builtin_amdgcn_sched_barrier(0);  // one chunk's temporaries at a time: the keys fill the register file
  }
  m = z_of(block_ext_u32<true>(key_of(m), s.red));

  // ---- log-sum-exp: the thread's elements in index order, the wave's butterfly, the waves in order
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < CPT; ++j) {
#pragma unroll
    for (int e = 0; e < 8; ++e) sum += __expf(__uint_as_float(key[j][e]) - m);
    __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if (lane == 0) fsum[wave] = sum;
  if (tid == 0) nwin = 0;
  __syncthreads();
  float tot = 0.f;
#pragma unroll
  for (int i = 0; i < SM_WAVES; ++i) tot += fsum[i];
  const float lse = m + logf(tot);  // (a row of -inf only: NaN, and every value below reads as -inf)

  // ---- values -> keys, in place
#pragma unroll
  for (int j = 0; j < CPT; ++j) {
    int c = tid + SM_THREADS * j;
    asm volatile("" : "+v"(c));  // (the 8 CPT in-range masks of the loads are computed again, not kept)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float v = score + (__uint_as_float(key[j][e]) - lse);
      key[j][e] = 8 * c + e < n ? key_of(v) : 0u;
    }
    __builtin_amdgcn_sched_barrier(0);
  }

  // ---- the row's G best: everything above the G-th largest key, then the threshold's holders by index
  const uint32_t thr = select_key<CPT, false>(key, (unsigned long long)G, 1u, 0.f, s);
#pragma unroll
  for (int j = 0; j < CPT; ++j) {
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (key[j][e] > thr) {  // fewer than G of them in the block
        const int at = atomicAdd(&nwin, 1);
        if (at < BM_MAX_G) win[at] = make_uint2(key[j][e], (uint32_t)(8 * (tid + SM_THREADS * j) + e));
      }
    __builtin_amdgcn_sched_barrier(0);
  }
  __syncthreads();
  int have = nwin < G ? nwin : G;
  uint32_t from = 0u;
  for (; have < G; ++have) {  // (block-uniform) at least G - nwin elements hold thr
    uint32_t first = 0xffffffffu;
#pragma unroll
    for (int j = CPT - 1; j >= 0; --j)
#pragma unroll
      for (int e = 7; e >= 0; --e) {
        const uint32_t idx = (uint32_t)(8 * (tid + SM_THREADS * j) + e);
        if (key[j][e] == thr && idx >= from) first = idx;
      }
    first = block_ext_u32<false>(first, s.red);
    if (tid == 0) win[have] = first < (uint32_t)n ? make_uint2(thr, first) : make_uint2(0u, 0u);
    from = first + 1u;
  }
  __syncthreads();
  if (tid < G) {  // descending: place = how many of the G are better
    const uint2 me = win[tid];
    int place = 0;
    for (int i = 0; i < G; ++i) {
      const uint2 o = win[i];
      place += o.x > me.x || (o.x == me.x && (o.y < me.y || (o.y == me.y && i < tid)));
    }
    cand[place] = me;
  }
}

__global__ void __launch_bounds__(64) beam_merge_kernel(const uint2* __restrict__ cand, float* __restrict__ scores,
                                                        unsigned char* __restrict__ done, int* __restrict__ parent,
                                                        long* __restrict__ token, int n, int G, long eos) {
  __shared__ unsigned long long ck[BM_MAX_G * BM_MAX_G];
  const int g = blockIdx.x, lane = threadIdx.x;
  const int total = G * G;
  unsigned long long mine[4];
  uint32_t tok[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int c = 4 * lane + q;
    mine[q] = 0ull;
    tok[q] = 0u;
    if (c < total) {
      const uint2 x = cand[(long)g * total + c];
      const uint32_t idx = (uint32_t)(c / G) * (uint32_t)n + (x.y & ~BM_DONE);  // < 16 * 65536 + 65536
      if (x.x) mine[q] = ((unsigned long long)x.x << 32) | (0xffffffffu - idx);
      tok[q] = x.y;
    }
    ck[c] = mine[q];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (mine[q] == 0ull) continue;
    int place = 0;
    for (int i = 0; i < total; ++i) place += ck[i] > mine[q];  // valid candidates are pairwise different
    if (place < G) {
      const int row = g * G + place;
      const long t = (long)(tok[q] & ~BM_DONE);
      scores[row] = z_of((uint32_t)(mine[q] >> 32));
      parent[row] = (4 * lane + q) / G;
      token[row] = t;
      done[row] = (tok[q] & BM_DONE) || (eos >= 0 && t == eos) ? 1 : 0;
    }
  }
}

__global__ void __launch_bounds__(256) beam_reorder_kernel(unsigned char* __restrict__ slots, long* __restrict__ hist,
                                                           const int* __restrict__ parent,
                                                           const long* __restrict__ lens,
                                                           const long* __restrict__ token, int G, int cap, long width) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  const int r0 = blockIdx.y * G;
  const long L = lens[r0];  // the rows of a group share their length
  int par[BM_MAX_G];
#pragma unroll
  for (int j = 0; j < BM_MAX_G; ++j) {
    const int v = j < G ? parent[r0 + j] : 0;
    par[j] = v < 0 ? 0 : (v < G ? v : G - 1);
  }
  if (slots && p < cap && p < L) {
    unsigned char v[BM_MAX_G];
#pragma unroll
    for (int j = 0; j < BM_MAX_G; ++j)
      v[j] = p == L - 1 ? (unsigned char)par[j] : (j < G ? slots[(long)(r0 + par[j]) * cap + p] : 0);
#pragma unroll
    for (int j = 0; j < BM_MAX_G; ++j)
      if (j < G) slots[(long)(r0 + j) * cap + p] = v[j];
  }
  if (hist && p < width) {
    long v[BM_MAX_G];
#pragma unroll
    for (int j = 0; j < BM_MAX_G; ++j) {
      v[j] = 0;
      if (j < G) v[j] = token && p == L ? token[r0 + j] : hist[(long)(r0 + par[j]) * width + p];
    }
#pragma unroll
    for (int j = 0; j < BM_MAX_G; ++j)
      if (j < G) hist[(long)(r0 + j) * width + p] = v[j];
  }
}

}  // namespace

// The G best continuations of every group of G rows of logits [B0*G, ld] (bf16, or f32 when f32 != 0; the first n
// entries of a row count, G <= n <= 65536) by the rule above. scores [B0*G] f32 and done [B0*G] bytes are read and
// then overwritten with the winners' (descending within a group); parent [B0*G] int32 (0 .. G-1), token [B0*G] int64.
// eos < 0: none; 0 <= pad < 65536. scratch: B0*G*G*2 uint32.
DTF_API int dtf_beam_select(const void* logits, int f32, long ld, int B0, int G, int n, float* scores,
                            unsigned char* done, long eos, long pad, int* parent, long* token, void* scratch,
                            void* stream) {
  if (!logits || !scores || !done || !parent || !token || !scratch) return -1;
  if (B0 < 1 || G < 2 || G > BM_MAX_G || n < G || n > SM_MAX_N || ld < n || (ld & 7) || !aligned16(logits)) return -1;
  if (pad < 0 || pad >= SM_MAX_N) return -1;
  BeamArgs a;
  a.logits = logits;
  a.ld = ld;
  a.n = n;
  a.G = G;
  a.scores = scores;
  a.done = done;
  a.pad = (uint32_t)pad;
  a.cand = (uint2*)scratch;
  hipStream_t st = (hipStream_t)stream;
  const int chunks = cdiv(n, 8 * SM_THREADS);
#define BEAM_ROW(C)                                                                                      \
  do {                                                                                                   \
    if (f32)                                                                                             \
      hipLaunchKernelGGL((beam_row_kernel<C, true>), dim3(B0 * G), dim3(SM_THREADS), 0, st, a);          \
    else                                                                                                 \
      hipLaunchKernelGGL((beam_row_kernel<C, false>), dim3(B0 * G), dim3(SM_THREADS), 0, st, a);         \
  } while (0)
  if (chunks <= 1) BEAM_ROW(1);
  else if (chunks <= 2) BEAM_ROW(2);
  else if (chunks <= 4) BEAM_ROW(4);
  else if (chunks <= 7) BEAM_ROW(7);
  else BEAM_ROW(8);
#undef BEAM_ROW
  hipLaunchKernelGGL(beam_merge_kernel, dim3(B0), dim3(64), 0, st, (const uint2*)scratch, scores, done, parent, token,
                     n, G, eos);
  const int rc = (int)hipGetLastError();
  if (rc == 0) count_launch(LC_BEAM_SELECT);
  return rc;
}

// Row j of every group continues row parent[j]: slots [B0*G, cap] uint8 (or null) and hist [B0*G, width] int64 (or
// null) are gathered by parent in place, column by column; column lens - 1 of slots becomes parent itself, columns
// from lens on stay, and column lens of hist receives token [B0*G] (when given). lens [B0*G], equal within a group.
DTF_API int dtf_beam_reorder(unsigned char* slots, long* hist, const int* parent, const long* lens, const long* token,
                             int B0, int G, int cap, long width, void* stream) {
  if (!parent || !lens || (!slots && !hist)) return -1;
  if (B0 < 1 || B0 > 65535 || G < 2 || G > BM_MAX_G || cap < 0 || width < 0) return -1;
  const long cols = (slots ? (long)cap : 0) > (hist ? width : 0) ? (long)cap : width;
  if (cols < 1) return 0;
  hipLaunchKernelGGL(beam_reorder_kernel, dim3((unsigned)cdiv(cols, 256L), B0), dim3(256), 0, (hipStream_t)stream,
                     slots, hist, parent, lens, token, G, cap, width);
  return (int)hipGetLastError();
}
