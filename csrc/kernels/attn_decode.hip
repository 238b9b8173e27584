// Single-token (decode) attention over a persistent KV cache, and the M <= 16 "skinny" dense layer of a decode step.
//
// Both are memory-bound streams read once: a key / value row of the cache (128 contiguous bytes) or a weight row goes
// straight from global memory to VGPRs in 16-byte loads, every load of a wave's step issued before the first use; no
// LDS staging of the streamed operand (LDS only carries the small cross-wave reductions, in a fixed order).
//
// Cache layout: per layer K and V are [B, H, Smax, 64] bf16; lens[B] (int64, device) holds the number of valid
// positions of each batch row and is shared by all layers. Call order of a decode step: dtf_kv_store (append the
// token's K/V at position lens[b]), then dtf_attn_decode (attend over 0 .. min(lens[b], Smax-1)); the caller advances
// lens once per token. Nothing here reads a device value on the host, allocates or synchronises: grids are sized by
// the cache capacity, so a launch is identical eagerly and under hipGraph capture. No floating-point atomics: results
// are bitwise reproducible.
//
// The fused one-token step (dtf_dense_skinny_fused, dtf_attn_decode_fused) moves the small launches of a decode layer
// into their neighbours: LayerNorm becomes a prologue of the projection that reads it (the normalised rows go through
// LDS once per block, the weight stream is untouched), the residual add and the cache append become epilogues, and the
// split-KV merge is done by whichever block of a head finishes last (an int32 ticket per head; no block waits).
#include "attn_decode.h"

namespace {

// K and V thirds of qkv[B, S, 3*H*64] -> cache rows lens[b] + s (rows at or past Smax are dropped). One 16-byte piece
// per thread and iteration.
__global__ void __launch_bounds__(256) kv_store_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ kc,
                                                       bf16_t* __restrict__ vc, const long* __restrict__ lens, int B,
                                                       int S, int H, int Smax) {
  const long HD = (long)H * 64;
  const long total = (long)B * S * H * 16;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i & 7), kv = (int)((i >> 3) & 1);
    long t = i >> 4;
    const int h = (int)(t % H);
    t /= H;
    const int s = (int)(t % S), b = (int)(t / S);
    const long pos = lens[b] + s;
    if (pos < 0 || pos >= Smax) continue;
    const uint4 v = *reinterpret_cast<const uint4*>(qkv + ((long)b * S + s) * 3 * HD + (1 + kv) * HD + h * 64 + c * 8);
    bf16_t* dst = (kv ? vc : kc) + (((long)b * H + h) * Smax + pos) * 64 + c * 8;
    *reinterpret_cast<uint4*>(dst) = v;
  }
}

// Merge the partials of one (b, h) in chunk order; thread = output dim.
__global__ void __launch_bounds__(64) attn_decode_merge_kernel(const float* __restrict__ scratch,
                                                               bf16_t* __restrict__ out, int nchunks) {
  const int bh = blockIdx.x, d = threadIdx.x;
  out[(long)bh * 64 + d] = merge_partials(scratch + (long)bh * nchunks * AD_PART, nchunks, d);
}

}  // namespace

DTF_API int dtf_attn_decode_chunk() { return AD_CHUNK; }

// qkv [B, S, 3*H*64] bf16 (packed [q | k | v] per token) -> k_cache / v_cache [B, H, Smax, 64] at positions
// lens[b] + s. lens is not changed.
DTF_API int dtf_kv_store(const void* qkv, void* k_cache, void* v_cache, const long* lens, int B, int S, int H,
                         int Smax, void* stream) {
  if (!qkv || !k_cache || !v_cache || !lens || B < 1 || S < 1 || H < 1 || Smax < 1) return -1;
  if (!aligned16(qkv) || !aligned16(k_cache) || !aligned16(v_cache)) return -1;
  const long total = (long)B * S * H * 16;
  hipLaunchKernelGGL(kv_store_kernel, dim3(stream_grid(total, 256)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)qkv, (bf16_t*)k_cache, (bf16_t*)v_cache, lens, B, S, H, Smax);
  return (int)hipGetLastError();
}

// One query row per (b, h) from qkv [B, 1, 3*H*64]; out [B, 1, H*64] bf16; scratch: B*H*ceil(Smax/chunk)*66 f32.
DTF_API int dtf_attn_decode(const void* qkv, const void* k_cache, const void* v_cache, const long* lens, void* out,
                            float* scratch, int B, int H, int Smax, float scale, void* stream) {
  if (!qkv || !k_cache || !v_cache || !lens || !out || !scratch || B < 1 || H < 1 || Smax < 1) return -1;
  if (!aligned16(qkv) || !aligned16(k_cache) || !aligned16(v_cache)) return -1;
  const int nchunks = cdiv(Smax, AD_CHUNK);
  if (nchunks > 65535) return -1;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(attn_decode_part_kernel<false>, dim3(B * H, nchunks), dim3(AD_WAVES * 64), 0, st,
                     (const bf16_t*)qkv, (const bf16_t*)k_cache, (const bf16_t*)v_cache, lens, scratch, H, Smax, nchunks,
                     scale, (int*)nullptr, (bf16_t*)nullptr);
  hipLaunchKernelGGL(attn_decode_merge_kernel, dim3(B * H), dim3(64), 0, st, (const float*)scratch, (bf16_t*)out,
                     nchunks);
  count_launch(LC_ATTN_DECODE);
  return (int)hipGetLastError();
}

// out[M, N] = act(x[M, K] w[N, K]^T + bias) for 1 <= M <= 16; x, w, out bf16 (row-major, dense), bias f32 or null;
// act: 0 none, 1 relu, 2 tanh-GELU. Rows per block by N alone, so that N = 1024 still gives 256 blocks.
DTF_API int dtf_dense_skinny(const void* x, const void* w, const float* bias, void* out, int M, int N, int K, int act,
                             void* stream) {
  if (!skinny_args_ok(x, w, out, M, N, K, act)) return -1;
  launch_skinny<false, false, false>((const bf16_t*)x, (const bf16_t*)w, bias, (bf16_t*)out, M, N, K, act,
                                     SkinnyExtra{}, (hipStream_t)stream);
  count_launch(LC_DENSE_SKINNY);
  return (int)hipGetLastError();
}
