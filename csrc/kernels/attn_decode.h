// Device code shared by attn_decode.hip (the default decode kernels) and attn_decode_fused.hip (the fused one-token
// step): the split-KV pass and its merge, and the M <= 16 weight-streaming dense kernel with its compile-time options.
#pragma once
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

// Merge the partials of one (b, h) in chunk order -> output dim d (chunk 0 always holds key 0: l > 0).
__device__ __forceinline__ bf16_t merge_partials(const float* part, int nchunks, int d) {
  float mm = -INFINITY;
  for (int c = 0; c < nchunks; ++c) mm = fmaxf(mm, part[c * AD_PART]);
  float l = 0.f, a = 0.f;
  for (int c = 0; c < nchunks; ++c) {
    const float mc = part[c * AD_PART];
    const float f = mc == -INFINITY ? 0.f : __expf(mc - mm);
    l += f * part[c * AD_PART + 1];
    a += f * part[c * AD_PART + 2 + d];
  }
  return f2bf(a / l);
}

// Split-KV pass: block (b*H + h, chunk) reduces keys [chunk*128, chunk*128 + 128) of one head to a partial
// (max, sum, 64-wide output) in f32. Lane = (key sub-index g = lane / 8, 16-byte piece c = lane % 8): one load
// instruction of a wave covers 8 whole key rows. Keys at or past the valid length are loaded from a clamped (in-bounds)
// row and never reach the arithmetic: the cache is uninitialised memory there, so both the score and the V
// contribution are masked by select.
//
// FUSED: the merge rides in the same launch. A block that has written its partial takes a ticket from the head's int32
// counter behind an agent-scope release (the partials of one head come from blocks on different XCDs, each behind its
// own L2); the block that draws the last ticket acquires, merges the head in chunk order with merge_partials (the bits
// of the two-launch route) and puts the counter back to 0 for the next call or replay. Every other block returns:
// nobody waits.
template <bool FUSED>
__global__ void __launch_bounds__(AD_WAVES * 64) attn_decode_part_kernel(
    const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ kc, const bf16_t* __restrict__ vc,
    const long* __restrict__ lens, float* __restrict__ scratch, int H, int Smax, int nchunks, float scale,
    int* counters, bf16_t* __restrict__ out) {
  __shared__ float sm[AD_WAVES][AD_PART];
  __shared__ int last;
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
    if (!FUSED) return;
  }
  if (FUSED ? k0 < n : true) {
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
  if (FUSED) {
    __syncthreads();  // the block's partial is complete (workgroup scope) ...
    if (tid == 0) {   // ... and one thread's agent-scope release carries it out of this XCD's L2: one write-back a block
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      last = __hip_atomic_fetch_add(counters + bh, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nchunks - 1;
    }
    __syncthreads();
    if (!last || tid >= 64) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    out[(long)bh * 64 + tid] = merge_partials(scratch + (long)bh * nchunks * AD_PART, nchunks, tid);
    if (tid == 0) __hip_atomic_store(counters + bh, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
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
//
// Three compile-time options make the variants of the fused decode step (dtf_dense_skinny_fused); with all three off
// this is dtf_dense_skinny's kernel (the main loop and arithmetic it always had), and none of them touches the main
// loop's arithmetic or the order of the reduction:
//  LN     x is the bf16 residual stream and the operand is LayerNorm(x). Before the main loop each wave normalises its
//         rows (m = wave, wave + 4, ...): the row sits in registers as 16-byte pieces (lane, lane + 64, ...), the mean
//         and then the sum of squared deviations are taken from those registers in f32 (two passes, no E[x^2] - mean^2),
//         and the normalised row goes to LDS as bf16, [16][K + pad], rows >= M zero. The main loop takes its x
//         fragments from that tile (ds_read_b128) instead of global memory. The 16 lanes of one k-group read 16 rows at
//         the same k, so the row stride is an odd number of 16-byte units (pad 8 or 16 elements): the 16 reads fall on
//         16 different 16-byte bank groups. The first weight loads of every wave are issued before the prologue, so the
//         stream is in flight while the rows are normalised.
//  RES    out = bf16(res + bf16(act(acc + bias))): the projection is rounded to bf16 first, the bits of a separate add.
//  STORE  N = 3*H*64 (the packed QKV projection, M = B): the threads that hold a column of the K or V third also write
//         it to row lens[m] of the layer's cache (rows outside [0, Smax) are dropped, dtf_kv_store's rule).
struct SkinnyExtra {
  const float *gamma, *beta;  // LN
  float eps;
  const bf16_t* res;          // RES [M, N]
  bf16_t *kc, *vc;            // STORE [M, H, Smax, 64]
  const long* lens;
  int H, Smax;
};

constexpr int LN_PIECES = 3;                    // 16-byte pieces of a row per lane: K <= 8 * 64 * 3
constexpr int LN_TILE_BYTES = 48 << 10;         // with the 16 KB of `red` (R = 4): the 64 KB a block has by default
__host__ __device__ inline int ln_ld(int K) { return K + ((K >> 3) & 1 ? 16 : 8); }

template <int R, int T, bool LN, bool RES, bool STORE>
__global__ void __launch_bounds__(256) dense_skinny_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
                                                           const float* __restrict__ bias, bf16_t* __restrict__ out,
                                                           int M, int N, int K, int act, SkinnyExtra ex) {
  constexpr int S = 16 / R;
  constexpr int KW = 32 * S;  // K elements of each weight row per wave step
  __shared__ float red[4][T * S][256];
  extern __shared__ __attribute__((aligned(16))) bf16_t xs[];  // LN: [16][ld]
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
  const int ld = LN ? ln_ld(K) : K;
  const bf16_t* xp = LN ? xs + r * ld : x + (long)(xrow ? r : 0) * K;
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
  uint4 av[U][T], bv[U][S];
  auto load_w = [&](int st) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int ka = (st + 4 * u) * KW + g * 8 + sub * 32;
#pragma unroll
      for (int t = 0; t < T; ++t) av[u][t] = *reinterpret_cast<const uint4*>(wp[t] + (ka < K ? ka : K - 8));
    }
  };
  if (LN) {
    load_w(wave);
    const int np = K >> 3;
    for (int m = wave; m < 16; m += 4) {
      bf16_t* dst = xs + m * ld;
      if (m >= M) {
        for (int p = lane; p < np; p += 64) *reinterpret_cast<uint4*>(dst + p * 8) = zero;
        continue;
      }
      float f[LN_PIECES][8];
      float sum = 0.f;
#pragma unroll
      for (int i = 0; i < LN_PIECES; ++i) {
        const int p = lane + 64 * i;
        if (p < np) {
          load8(x + (long)m * K + p * 8, f[i]);
#pragma unroll
          for (int e = 0; e < 8; ++e) sum += f[i][e];
        }
      }
      const float mean = wave_sum(sum) / (float)K;
      float sq = 0.f;
#pragma unroll
      for (int i = 0; i < LN_PIECES; ++i)
        if (lane + 64 * i < np) {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            f[i][e] -= mean;
            sq += f[i][e] * f[i][e];
          }
        }
      const float rstd = rsqrtf(wave_sum(sq) / (float)K + ex.eps);
#pragma unroll
      for (int i = 0; i < LN_PIECES; ++i) {
        const int p = lane + 64 * i;
        if (p < np) {
          const float4 g0 = *reinterpret_cast<const float4*>(ex.gamma + p * 8);
          const float4 g1 = *reinterpret_cast<const float4*>(ex.gamma + p * 8 + 4);
          const float4 b0 = *reinterpret_cast<const float4*>(ex.beta + p * 8);
          const float4 b1 = *reinterpret_cast<const float4*>(ex.beta + p * 8 + 4);
          const float ga[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
          const float be[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
          float y[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) y[e] = f[i][e] * rstd * ga[e] + be[e];
          store8(dst + p * 8, y);
        }
      }
    }
    __syncthreads();
  }
  for (int st = wave; st < nsteps; st += 4 * U) {
    if (!LN || st != wave) load_w(st);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int kb = (st + 4 * u) * KW + g * 8;
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
        if (kb + s * 32 >= K || (!LN && !xrow)) bv[u][s] = zero;  // (LN: the tile's rows >= M are zero already)
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
    long pos = 0;
    if (STORE && m < M) pos = ex.lens[m];  // one load per output thread, also where its columns are all in the Q third
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
        bf16_t o = f2bf(val);
        if (RES) o = f2bf(bf2f(ex.res[(long)m * N + n]) + bf2f(o));
        out[(long)m * N + n] = o;
        if (STORE) {
          const int HD = ex.H * 64;
          if (n >= HD && pos >= 0 && pos < ex.Smax) {
            const int kv = n >= 2 * HD, c = n - (1 + kv) * HD;  // c = h * 64 + d
            bf16_t* dst = kv ? ex.vc : ex.kc;
            dst[(((long)m * ex.H + (c >> 6)) * ex.Smax + pos) * 64 + (c & 63)] = o;
          }
        }
      }
    }
  }
}

template <bool LN, bool RES, bool STORE>
void launch_skinny(const bf16_t* x, const bf16_t* w, const float* bias, bf16_t* out, int M, int N, int K, int act,
                   const SkinnyExtra& ex, hipStream_t st) {
  const size_t lds = LN ? (size_t)16 * ln_ld(K) * sizeof(bf16_t) : 0;
#define SKINNY(R, T)                                                                                              \
  hipLaunchKernelGGL((dense_skinny_kernel<R, T, LN, RES, STORE>), dim3(cdiv(N, R * T)), dim3(256), lds, st, x, w, \
                     bias, out, M, N, K, act, ex)
  if (N >= 16384) SKINNY(16, 2);
  else if (N >= 4096) SKINNY(8, 1);
  else SKINNY(4, 1);
#undef SKINNY
}

bool skinny_args_ok(const void* x, const void* w, const void* out, int M, int N, int K, int act) {
  if (!x || !w || !out || M < 1 || M > 16 || N < 8 || K < 8 || (N & 7) || (K & 7) || act < 0 || act > 2) return false;
  return aligned16(x) && aligned16(w);
}

// Largest K of the LayerNorm prologue: the bf16 tile [16][K + pad] has to fit LN_TILE_BYTES (48 KB; with the 16 KB
// of the cross-wave reduction that is the 64 KB of LDS a block may use without raising the function's limit, and three
// blocks still share a CU's 160 KB), and a lane holds at most LN_PIECES pieces of a row.
constexpr int LN_MAX_K = 1520;
static_assert(16 * (LN_MAX_K + 16) * 2 <= LN_TILE_BYTES && LN_MAX_K <= 8 * 64 * LN_PIECES, "LN tile");

}  // namespace
