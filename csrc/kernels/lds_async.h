// Primitives of the kernels that keep LDS-DMA in flight across their main loop (pwconv.hip, pwwgrad.hip, pwbwd.hip,
// stemwgrad.hip, c3wgrad.hip, gemm_w4*.hip): a ring of LDS images filled by `buffer_load ... lds`, counted vmcnt waits,
// and every LDS access beside the ring written as inline asm.
//
// The discipline, once:
//  * hipcc cannot tell an LDS access from the ring: LDS-DMA writes carry no alias information, so before a plain LDS
//    load or store, a builtin ds_read_tr, or __syncthreads() (whose fence counts the in-flight DMA as pending LDS
//    writes) it waits for EVERY outstanding vector-memory op — draining the tiles in flight once per tile. So inside
//    such a loop the LDS reads, the LDS writes and the barrier are the asm forms below, and the DMA is ordered by
//    explicit vm_wait<N>() with N = the ops this thread issued after the tile it needs. N must be the same on every
//    iteration: issue every DMA / load / store unconditionally (past the end with OOB_OFF: the range check makes it a
//    zero fill / a dropped store), or hipcc assumes the path without them and drains.
//  * hipcc neither sees nor waits for the asm accesses: an asm read's result exists only after lds_wait(), and every
//    register it filled is tied to that wait (tie) so no use moves above it; asm writes are published by lds_barrier().
//  * lds_barrier() is ONE asm statement (this thread's LDS ops done, then s_barrier) and a compiler memory barrier.
//    It does not pin register-only MFMAs (gemm_w4.h's sched_barrier-pinned w4_barrier / w4_lgkm0 do).
//  * per-kernel register operands loaded before the loop (filter slices, coefficients) are consumed before the first
//    DMA (asm volatile("" ::"v"(x))): otherwise their vmcnt waits land inside the loop and hold up the ring.
//  * fragments are assembled by whole-vector casts: per-element short -> __bf16 extraction miscompiles (ROCm 7.2).
#pragma once
#include "gemm_core.h"

namespace dtf {
namespace {

// ---- buffer descriptors, out-of-range offsets, the DMA itself
constexpr uint32_t OOB_OFF = 0x80000000u;  // past any descriptor's range (operands < 2 GiB): loads give 0, stores drop
// raw buffer over `bytes` bytes at p (32-bit data format word of gfx950; bytes 0: every access out of range)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* p, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, bytes, 0x00020000);
}
// 16 B per lane from the buffer (per-lane byte offset voff, wave-uniform soff) to LDS at lds + 16 * lane (lds is
// wave-uniform: a wave instruction fills 1 KiB lane-linearly)
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t r, char* lds, uint32_t voff, int soff = 0) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, LDS_PTR(void, lds), 16, voff, soff, 0, 0);
}
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t r, uint32_t lds, uint32_t voff, int soff = 0) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, LDS_PTR(void, (uintptr_t)lds), 16, voff, soff, 0, 0);
}

// ---- waits
__device__ __forceinline__ void lds_wait() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
template <int N>
__device__ __forceinline__ void vm_wait() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// after lds_wait(): the registers asm reads filled
template <class T>
__device__ __forceinline__ void tie(T& f) {
  asm volatile("" : "+v"(f));
}
template <class T, int N>
__device__ __forceinline__ void tie(T (&f)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) tie(f[i]);
}
template <class A, class B, class... R>
__device__ __forceinline__ void tie(A& a, B& b, R&... r) {
  tie(a);
  tie(b, r...);
}

// ---- inline-asm LDS accesses
__device__ __forceinline__ uint32_t lds_addr(const char* p) { return (uint32_t)(uintptr_t)LDS_PTR(const char, p); }
__device__ __forceinline__ void lds_store8(char* p, uint2 v) {
  asm volatile("ds_write_b64 %0, %1" ::"v"(lds_addr(p)), "v"(v) : "memory");
}
__device__ __forceinline__ void lds_store16(char* p, v4i v) {
  asm volatile("ds_write_b128 %0, %1" ::"v"(lds_addr(p)), "v"(v) : "memory");
}
// 16 B, result valid after lds_wait() + tie
__device__ __forceinline__ v4i lds_load16_async(const char* p) {
  v4i r;
  asm volatile("ds_read_b128 %0, %1" : "=v"(r) : "v"(lds_addr(p)));
  return r;
}
// 16 B, waited for
__device__ __forceinline__ uint4 lds_load16(const char* p) {
  v4i r;
  asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(r) : "v"(lds_addr(p)) : "memory");
  return __builtin_bit_cast(uint4, r);
}
// N x 16 B at base + off[i]: one wait for all N reads, each result tied to it
template <int N>
__device__ __forceinline__ void lds_load16(uint4 (&v)[N], const char* base, const int (&off)[N]) {
  v4i r[N];
#pragma unroll
  for (int i = 0; i < N; ++i) r[i] = lds_load16_async(base + off[i]);
  lds_wait();
#pragma unroll
  for (int i = 0; i < N; ++i) {
    tie(r[i]);
    v[i] = __builtin_bit_cast(uint4, r[i]);
  }
}
// the two ds_read_b64_tr_b16 of one 16x32 MFMA fragment (LDS byte addresses), valid after lds_wait() + tie
__device__ __forceinline__ v8bf tr_pair(uint32_t a0, uint32_t a1) {
  v4s r0, r1;
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(r0) : "v"(a0));
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(r1) : "v"(a1));
  v8s both = __builtin_shufflevector(r0, r1, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(v8bf, both);
}

// ---- K-outer image: [rows k][R cols] bf16, 8-B granules XOR-swizzled by kouter_swz<R>(k) (gemm_core.h)
// Transposed fragment, frag_kouter<R>'s addressing (gemm_core.h: the builtin form, for kernels with no DMA in
// flight): columns cb..cb+15, k rows 32 kk + shift + (the lane's slot). shift moves the read along k: a filter tap of
// an image whose k index is a pixel position. ADDR2: both addresses are formed before the first read is issued — the
// same reads, but hipcc allocates registers differently around the two forms; stemwgrad.hip / c3wgrad.hip use this one.
template <int R, bool ADDR2 = false>
__device__ __forceinline__ v8bf frag_kouter_async(const char* lds, int cb, int kk, int lane, int shift = 0) {
  const int G = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
  uint32_t ad[2];
  v4s r[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int k = 32 * kk + 8 * G + 4 * h + q + shift;
    const int g = ((cb >> 2) + p) ^ (kouter_swz<R>(k) << 2);
    ad[h] = lds_addr(lds + k * (R * 2) + g * 8);
    if constexpr (!ADDR2) asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(r[h]) : "v"(ad[h]));
  }
  if constexpr (ADDR2) return tr_pair(ad[0], ad[1]);
  v8s both = __builtin_shufflevector(r[0], r[1], 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(v8bf, both);
}
// row fragment of the same image: k row pr + (lane & 15), columns 32 s + 8 (lane >> 4) .. +7
template <int R>
__device__ __forceinline__ v8bf row_frag(const char* lds, int pr, int s, int lane) {
  const int row = pr + (lane & 15);
  const int pc = (4 * s + (lane >> 4)) ^ (kouter_swz<R>(row) << 1);
  return __builtin_bit_cast(v8bf, lds_load16_async(lds + row * (R * 2) + pc * 16));
}
// LDS-DMA of the [64][R] slice (columns col0 .. col0+R of rows with stride ld elements) of a [rows][ld] operand into
// the image: 256 threads x 16 B per instruction set, each lane fetching the logical chunk that the swizzle puts at its
// physical slot (GldsKOuter's mapping); rows past P read zeros through the range check
template <int R>
struct KOuterDma {
  static constexpr int L = R / 32;  // DMA instructions per thread per tile
  __amdgpu_buffer_rsrc_t rsrc;
  int kr[L], coff[L], rowb;

  __device__ __forceinline__ void init(const bf16_t* p, long rows, int ld, int col0) {
    const int t = threadIdx.x;
    rsrc = buf_rsrc(p, (int)(rows * ld * 2));
    rowb = ld * 2;
#pragma unroll
    for (int i = 0; i < L; ++i) {
      const int pb = i * 4096 + t * 16;
      kr[i] = pb / (R * 2);
      const int c = ((pb % (R * 2)) >> 4) ^ (kouter_swz<R>(kr[i]) << 1);
      coff[i] = (col0 + c * 8) * 2;
    }
  }
  __device__ __forceinline__ void issue(int p0, int P, char* lds) {
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < L; ++i) {
      const int p = p0 + kr[i];
      const uint32_t off = p < P ? (uint32_t)(p * rowb + coff[i]) : OOB_OFF;
      dma16(rsrc, lds + i * 4096 + wave * 1024, off);
    }
  }
};

}  // namespace
}  // namespace dtf
