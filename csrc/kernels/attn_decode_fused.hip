// The fused one-token decode step: dtf_dense_skinny_fused and dtf_attn_decode_fused (device code in attn_decode.h).
#include "attn_decode.h"

// dtf_attn_decode in one launch: the block of each head that finishes last merges it (attn_decode_part_kernel<true>).
// counters: B*H int32, zero before the first call; every call leaves them zero. Same bits as dtf_attn_decode.
DTF_API int dtf_attn_decode_fused(const void* qkv, const void* k_cache, const void* v_cache, const long* lens,
                                  void* out, float* scratch, int* counters, int B, int H, int Smax, float scale,
                                  void* stream) {
  if (!qkv || !k_cache || !v_cache || !lens || !out || !scratch || !counters || B < 1 || H < 1 || Smax < 1) return -1;
  if (!aligned16(qkv) || !aligned16(k_cache) || !aligned16(v_cache)) return -1;
  const int nchunks = cdiv(Smax, AD_CHUNK);
  if (nchunks > 65535) return -1;
  hipLaunchKernelGGL(attn_decode_part_kernel<true>, dim3(B * H, nchunks), dim3(AD_WAVES * 64), 0, (hipStream_t)stream,
                     (const bf16_t*)qkv, (const bf16_t*)k_cache, (const bf16_t*)v_cache, lens, scratch, H, Smax,
                     nchunks, scale, counters, (bf16_t*)out);
  count_launch(LC_ATTN_DECODE_FUSED);
  return (int)hipGetLastError();
}

DTF_API int dtf_dense_skinny_ln_max_k() { return LN_MAX_K; }

// dtf_dense_skinny with the prologue and epilogues of the fused decode step (dense_skinny_kernel's options), each
// switched on by its pointers:
//  gamma, beta (f32 [K]), eps  x is normalised per row before the projection; K <= dtf_dense_skinny_ln_max_k()
//  res (bf16 [M, N])           out = bf16(res + bf16(act(x w^T + bias)))
//  k_cache, v_cache ([M, H, Smax, 64] bf16), lens (int64 [M], device)   N == 3*H*64: the K and V thirds of out also go
//                              to cache row lens[m] (dropped outside [0, Smax)); lens is not changed
// Same contract as dtf_dense_skinny otherwise: -1 on anything it cannot run, no allocation, no synchronisation, no
// device value read on the host.
DTF_API int dtf_dense_skinny_fused(const void* x, const void* w, const float* bias, void* out, int M, int N, int K,
                                   int act, const float* gamma, const float* beta, float eps, const void* res,
                                   void* k_cache, void* v_cache, const long* lens, int H, int Smax, void* stream) {
  if (!skinny_args_ok(x, w, out, M, N, K, act)) return -1;
  const bool ln = gamma || beta, store = k_cache || v_cache || lens;
  if (ln && (!gamma || !beta || !aligned16(gamma) || !aligned16(beta) || K > LN_MAX_K || !(eps >= 0.f))) return -1;
  if (res && ((uintptr_t)res & 1)) return -1;  // read element by element, like out is written
  if (store && (!k_cache || !v_cache || !lens || H < 1 || Smax < 1 || (long)N != 3L * H * 64 || ((uintptr_t)lens & 7) ||
                ((uintptr_t)k_cache & 1) || ((uintptr_t)v_cache & 1)))
    return -1;
  SkinnyExtra ex{gamma, beta, eps, (const bf16_t*)res, (bf16_t*)k_cache, (bf16_t*)v_cache, lens, H, Smax};
  const bf16_t *xb = (const bf16_t*)x, *wb = (const bf16_t*)w;
  bf16_t* ob = (bf16_t*)out;
  hipStream_t st = (hipStream_t)stream;
  switch ((ln ? 4 : 0) | (res ? 2 : 0) | (store ? 1 : 0)) {
    case 0: launch_skinny<false, false, false>(xb, wb, bias, ob, M, N, K, act, ex, st); break;
    case 1: launch_skinny<false, false, true>(xb, wb, bias, ob, M, N, K, act, ex, st); break;
    case 2: launch_skinny<false, true, false>(xb, wb, bias, ob, M, N, K, act, ex, st); break;
    case 3: launch_skinny<false, true, true>(xb, wb, bias, ob, M, N, K, act, ex, st); break;
    case 4: launch_skinny<true, false, false>(xb, wb, bias, ob, M, N, K, act, ex, st); break;
    case 5: launch_skinny<true, false, true>(xb, wb, bias, ob, M, N, K, act, ex, st); break;
    case 6: launch_skinny<true, true, false>(xb, wb, bias, ob, M, N, K, act, ex, st); break;
    default: launch_skinny<true, true, true>(xb, wb, bias, ob, M, N, K, act, ex, st); break;
  }
  count_launch(LC_DENSE_SKINNY_FUSED);
  return (int)hipGetLastError();
}
