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
// the cache capacity, so a launch is identical eagerly and under hipGraph capture. No atomics: results are bitwise
// reproducible.
#include "common.h"
#include "routes.h"

namespace {

constexpr int AD_CHUNK = 128;               // keys per block of the split-KV pass
constexpr int AD_WAVES = 4;                 // waves per block, AD_CHUNK / AD_WAVES = 32 keys each (8 per load x 4)
constexpr int AD_PART = 66;                 // f32 per partial: running max, running sum, 64 output dims

__device__ __forceinline__ void unpack8(const uint4& v, float* f) {
  f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u);
  f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xffff0000u);
  f[4] = __uint_as_float(v.z << 16); f[5] = __uint_as_float(v.z & 0xffff0000u);
  f[6] = __uint_as_float(v.w << 16); f[7] = __uint_as_float(v.w & 0xffff0000u);
}

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

// Split-KV pass: block (b*H + h, chunk) reduces keys [chunk*128, chunk*128 + 128) of one head to a partial
// (max, sum, 64-wide output) in f32. Lane = (key sub-index g = lane / 8, 16-byte piece c = lane % 8): one load
// instruction of a wave covers 8 whole key rows. Keys at or past the valid length are loaded from a clamped (in-bounds)
// row and never reach the arithmetic: the cache is uninitialised memory there, so both the score and the V
// contribution are masked by select.
__global__ void __launch_bounds__(AD_WAVES * 64) attn_decode_part_kernel(
    const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ kc, const bf16_t* __restrict__ vc,
    const long* __restrict__ lens, float* __restrict__ scratch, int H, int Smax, int nchunks, float scale) {
  __shared__ float sm[AD_WAVES][AD_PART];
  const int bh = blockIdx.x, chunk = blockIdx.y;
  const int b = bh / H, h = bh - b * H;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  long len = lens[b];
  len = len < 0 ? 0 : len;
  const int n = (int)(len < Smax - 1 ? len : Smax - 1) + 1;  // valid keys: 0 .. n-1
  float* part = scratch + ((long)bh * nchunks + chunk) * AD_PART;
  const int k0 = chunk * AD_CHUNK;
  if (k0 >= n) {  // nothing valid in this chunk: the "empty" partial
    if (tid < AD_PART) part[tid] = tid == 0 ? -INFINITY : 0.f;
    return;
  }
  const int g = lane >> 3, c = lane & 7;
  const bf16_t* kb = kc + (long)bh * Smax * 64 + c * 8;
  const bf16_t* vb = vc + (long)bh * Smax * 64 + c * 8;
  const int kw = k0 + wave * 32 + g;
  uint4 kr[4], vr[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int key = kw + j * 8;
    const long row = key < Smax ? key : Smax - 1;
    kr[j] = *reinterpret_cast<const uint4*>(kb + row * 64);
    vr[j] = *reinterpret_cast<const uint4*>(vb + row * 64);
  }
  float q[8];
  load8(qkv + (long)b * 3 * H * 64 + h * 64 + c * 8, q);

  float s[4];
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float k[8];
    unpack8(kr[j], k);
    float d = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) d += q[e] * k[e];
    d += __shfl_xor(d, 1, 64);
    d += __shfl_xor(d, 2, 64);
    d += __shfl_xor(d, 4, 64);
    s[j] = (kw + j * 8 < n) ? d * scale : -INFINITY;
    m = fmaxf(m, s[j]);
  }
  m = fmaxf(m, __shfl_xor(m, 8, 64));
  m = fmaxf(m, __shfl_xor(m, 16, 64));
  m = fmaxf(m, __shfl_xor(m, 32, 64));

  float l = 0.f, acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bool valid = kw + j * 8 < n;
    const float p = valid ? __expf(s[j] - m) : 0.f;
    float v[8];
    unpack8(vr[j], v);
    l += p;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += p * (valid ? v[e] : 0.f);
  }
#pragma unroll
  for (int o = 8; o < 64; o <<= 1) {
    l += __shfl_xor(l, o, 64);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += __shfl_xor(acc[e], o, 64);
  }
  if (lane == 0) {
    sm[wave][0] = m;
    sm[wave][1] = l;
  }
  if (g == 0) {
#pragma unroll
    for (int e = 0; e < 8; ++e) sm[wave][2 + c * 8 + e] = acc[e];
  }
  __syncthreads();
  if (tid < 64) {  // merge the four waves in wave order (wave 0 always holds a valid key here)
    float mm = sm[0][0];
#pragma unroll
    for (int w = 1; w < AD_WAVES; ++w) mm = fmaxf(mm, sm[w][0]);
    float ll = 0.f, a = 0.f;
#pragma unroll
    for (int w = 0; w < AD_WAVES; ++w) {
      const float mw = sm[w][0];
      const float f = mw == -INFINITY ? 0.f : __expf(mw - mm);
      ll += f * sm[w][1];
      a += f * sm[w][2 + tid];
    }
    part[2 + tid] = a;
    if (tid == 0) {
      part[0] = mm;
      part[1] = ll;
    }
  }
}

// Merge the partials of one (b, h) in chunk order; thread = output dim.
__global__ void __launch_bounds__(64) attn_decode_merge_kernel(const float* __restrict__ scratch,
                                                               bf16_t* __restrict__ out, int nchunks) {
  const int bh = blockIdx.x, d = threadIdx.x;
  const float* part = scratch + (long)bh * nchunks * AD_PART;
  float mm = -INFINITY;
  for (int c = 0; c < nchunks; ++c) mm = fmaxf(mm, part[c * AD_PART]);
  float l = 0.f, a = 0.f;
  for (int c = 0; c < nchunks; ++c) {
    const float mc = part[c * AD_PART];
    const float f = mc == -INFINITY ? 0.f : __expf(mc - mm);
    l += f * part[c * AD_PART + 1];
    a += f * part[c * AD_PART + 2 + d];
  }
  out[(long)bh * 64 + d] = f2bf(a / l);  // chunk 0 always holds key 0: l > 0
}

// same formula as the GEMM epilogue (gemm_core.h gelu_tanh): x * sigmoid(2u)
__device__ __forceinline__ float skinny_gelu(float x) {
  const float k0 = 0.7978845608028654f, k1 = 0.044715f;
  const float u = k0 * (x + k1 * x * x * x);
  return x * __builtin_amdgcn_rcpf(1.f + __expf(-2.f * u));
}

// out[M, N] = act(x[M, K] w[N, K]^T + bias), M <= 16: a weight stream on the 16x16x32 bf16 MFMA with x as the
// (zero-padded) 16-column operand. A block owns R weight rows; its four waves interleave over K and are summed in wave
// order through LDS. To keep every lane's 16-byte load on the weight stream with fewer than 16 rows per block, the 16
// tile rows of the MFMA's first operand hold the block's R weight rows at 16/R consecutive 32-element K sub-ranges
// (tile row = sub * R + row); one MFMA per sub-range multiplies the tile with x at that sub-range into its own
// accumulator, of which only the rows of that sub-range are meaningful (the others pair a weight piece with the
// x of another K range and are never read). R = 4 reads four 256-byte pieces per load and wave, R = 8 eight full
// 128-byte lines, R = 16 sixteen half lines (the next step of the same wave finishes them). A block owns T such row
// groups (R * T rows), which share every x load: T = 2 for the widest layers, where x traffic per weight byte showed.
template <int R, int T>
__global__ void __launch_bounds__(256) dense_skinny_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
                                                           const float* __restrict__ bias, bf16_t* __restrict__ out,
                                                           int M, int N, int K, int act) {
  constexpr int S = 16 / R;
  constexpr int KW = 32 * S;  // K elements of each weight row per wave step
  __shared__ float red[4][T * S][256];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r = lane & 15, g = lane >> 4;
  const int sub = r / R, row = r - sub * R;
  const int n0 = blockIdx.x * R * T;
  const bf16_t* wp[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int nrow = n0 + t * R + row;
    wp[t] = w + (long)(nrow < N ? nrow : N - 1) * K;
  }
  const bool xrow = r < M;
  const bf16_t* xp = x + (long)(xrow ? r : 0) * K;
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
  v4f acc[T][S];
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int s = 0; s < S; ++s) acc[t][s] = (v4f){0.f, 0.f, 0.f, 0.f};
  const int nsteps = (K + KW - 1) / KW;
  // U steps of a wave per iteration, all their loads issued before the first MFMA; a step past K loads a clamped
  // (in-bounds) address and contributes zeros
  constexpr int U = R == 4 ? 2 : 4;
  for (int st = wave; st < nsteps; st += 4 * U) {
    uint4 av[U][T], bv[U][S];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int kb = (st + 4 * u) * KW + g * 8;
      const int ka = kb + sub * 32;
#pragma unroll
      for (int t = 0; t < T; ++t) av[u][t] = *reinterpret_cast<const uint4*>(wp[t] + (ka < K ? ka : K - 8));
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const int kx = kb + s * 32;
        bv[u][s] = *reinterpret_cast<const uint4*>(xp + (kx < K ? kx : K - 8));
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int kb = (st + 4 * u) * KW + g * 8;
#pragma unroll
      for (int s = 0; s < S; ++s)
        if (kb + s * 32 >= K || !xrow) bv[u][s] = zero;
#pragma unroll
      for (int t = 0; t < T; ++t) {
        if (kb + sub * 32 >= K) av[u][t] = zero;
#pragma unroll
        for (int s = 0; s < S; ++s)
          acc[t][s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, av[u][t]),
                                                              __builtin_bit_cast(v8bf, bv[u][s]), acc[t][s], 0, 0, 0);
      }
    }
  }
  // accumulator layout: lane holds D[i = 4 * g + v][j = r]  (i: tile row, j: x row)
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
      for (int v = 0; v < 4; ++v) red[wave][t * S + s][(4 * g + v) * 16 + r] = acc[t][s][v];
  __syncthreads();
  if (tid < R * 16) {
    const int orow = tid >> 4, m = tid & 15;
#pragma unroll
    for (int t = 0; t < T; ++t) {
      float val = 0.f;
#pragma unroll
      for (int s = 0; s < S; ++s)
#pragma unroll
        for (int wv = 0; wv < 4; ++wv) val += red[wv][t * S + s][(s * R + orow) * 16 + m];
      const int n = n0 + t * R + orow;
      if (m < M && n < N) {
        if (bias) val += bias[n];
        if (act == 1) val = fmaxf(val, 0.f);
        else if (act == 2) val = skinny_gelu(val);
        out[(long)m * N + n] = f2bf(val);
      }
    }
  }
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
  hipLaunchKernelGGL(attn_decode_part_kernel, dim3(B * H, nchunks), dim3(AD_WAVES * 64), 0, st, (const bf16_t*)qkv,
                     (const bf16_t*)k_cache, (const bf16_t*)v_cache, lens, scratch, H, Smax, nchunks, scale);
  hipLaunchKernelGGL(attn_decode_merge_kernel, dim3(B * H), dim3(64), 0, st, (const float*)scratch, (bf16_t*)out,
                     nchunks);
  count_launch(LC_ATTN_DECODE);
  return (int)hipGetLastError();
}

// out[M, N] = act(x[M, K] w[N, K]^T + bias) for 1 <= M <= 16; x, w, out bf16 (row-major, dense), bias f32 or null;
// act: 0 none, 1 relu, 2 tanh-GELU. Rows per block by N alone, so that N = 1024 still gives 256 blocks.
DTF_API int dtf_dense_skinny(const void* x, const void* w, const float* bias, void* out, int M, int N, int K, int act,
                             void* stream) {
  if (!x || !w || !out || M < 1 || M > 16 || N < 8 || K < 8 || (N & 7) || (K & 7) || act < 0 || act > 2) return -1;
  if (!aligned16(x) || !aligned16(w)) return -1;
  hipStream_t st = (hipStream_t)stream;
#define SKINNY(R, T)                                                                                   \
  hipLaunchKernelGGL((dense_skinny_kernel<R, T>), dim3(cdiv(N, R * T)), dim3(256), 0, st, (const bf16_t*)x, \
                     (const bf16_t*)w, bias, (bf16_t*)out, M, N, K, act)
  if (N >= 16384) SKINNY(16, 2);
  else if (N >= 4096) SKINNY(8, 1);
  else SKINNY(4, 1);
#undef SKINNY
  count_launch(LC_DENSE_SKINNY);
  return (int)hipGetLastError();
}
