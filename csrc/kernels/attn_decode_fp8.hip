// fp8 KV cache: the store and the split-KV decode pass of attn_decode.hip on 64-byte rows.
//
// Format, the same for K and V, per cached row (one (layer, b, h, position), 64 values): 64 OCP e4m3fn codes and one
// f32 scale that is an exact power of two 2^e, 68 bytes against bf16's 128. With a the largest finite |v| of the row,
// a = m * 2^x, 1 <= m < 2: e = x - 8 for m <= 1.75, else x - 7 (the smallest e with a * 2^-e <= 448), at least -64, and
// 0 for a == 0; x and m come from the bf16 exponent and mantissa fields, no log2. A code is v * 2^-e (exact in f32)
// clamped to +-448 and rounded to nearest even by v_cvt_pk_fp8_f32; NaN stays a NaN code, +-inf saturates.
// Dequantization code * 2^e is exact in bf16 (4 significant bits), so everything here is defined bit for bit.
//
// Store: thread = one 16-byte bf16 piece of a row, as in kv_store_kernel; the 8 lanes of a row take its amax with three
// __shfl_xor steps on the 15-bit magnitude (integer max is the float max for finite values), form e, convert and write
// 8 code bytes each; the lane of piece 0 writes the scale.
//
// Decode: grid (B*H, cdiv(Smax, AD_CHUNK)), 128 keys a block and the 66-float partial of attn_decode.h, so the cache's
// scratch and merge_partials are shared with the bf16 route. Lane = (key sub-index g = lane / 4, 16-byte piece
// c = lane % 4): one load instruction of a wave covers 16 whole key rows (1 KB contiguous), a wave's 32 keys are two K
// and two V loads plus four dword scale loads, all issued with the lane's 16 q values before the first use.
// score = (q . k_codes) * k_scale * scale with the dot closed over the quad by two DPP adds; V's scale is folded into
// the probability (w = p * v_scale, acc += w * v_codes; the running sum adds p). Rows at or past the valid length are
// uninitialised memory (NaN codes, garbage scales): score, weight and V values are masked by select, never by * 0.
//
// Cross-key-group reduction of the 16 accumulators a lane holds (16 key groups on lane bits 2..5): recursive halving,
// not an all-reduce. At the step of lane bit o a lane keeps the half of its accumulators that its bit selects and
// receives the partner's copy of that half, so the steps move 8 + 4 + 2 + 1 = 15 values (15 ds_bpermute and 15 adds a
// lane) and leave every lane with one output dim, against 4 x 16 = 64 for the butterfly that leaves all 16 dims in
// every lane. A pass through LDS would cost 4 ds_write_b128 and 16 ds_read_b32 a lane plus a barrier, also more LDS
// instructions than 15, so the shuffles stay. The order is fixed and there are no float atomics: same inputs, same bits.
#include "attn_decode.h"

namespace {

// power-of-two exponent of a row's scale from the bf16 magnitude bits of its amax (finite): see the header
__device__ __forceinline__ int kv_scale_exp(uint32_t amax_bits) {
  if (amax_bits == 0) return 0;
  const int x = (int)(amax_bits >> 7) - 127, mant = (int)(amax_bits & 0x7f);  // (a bf16 subnormal: x = -127 -> -64)
  const int e = x - 8 + (mant > 0x60);                                         // 0x60: m = 1.75
  return e < -64 ? -64 : e;
}

// NaN-keeping clamp to +-448 (v_minimum3 / v_maximum3: fminf / fmaxf would turn NaN into the bound)
__device__ __forceinline__ float sat448(float y) {
  return __builtin_elementwise_minimum(__builtin_elementwise_maximum(y, -448.f), 448.f);
}

__device__ __forceinline__ uint32_t max_mag(uint32_t m, uint32_t w) {  // one bf16 (low 16 bits of w), finite only
  const uint32_t a = w & 0x7fffu;
  return a < 0x7f80u && a > m ? a : m;
}

__global__ void __launch_bounds__(256) kv_store_fp8_kernel(const bf16_t* __restrict__ qkv, uint8_t* __restrict__ kc,
                                                           uint8_t* __restrict__ vc, float* __restrict__ ksc,
                                                           float* __restrict__ vsc, const long* __restrict__ lens, int B,
                                                           int S, int H, int Smax) {
  const long HD = (long)H * 64;
  const long total = (long)B * S * H * 16;  // a multiple of 8: the 8 lanes of a row enter and leave the loop together
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i & 7), kv = (int)((i >> 3) & 1);
    long t = i >> 4;
    const int h = (int)(t % H);
    t /= H;
    const int s = (int)(t % S), b = (int)(t / S);
    const long pos = lens[b] + s;
    if (pos < 0 || pos >= Smax) continue;  // uniform over the row's 8 lanes
    const uint4 v = *reinterpret_cast<const uint4*>(qkv + ((long)b * S + s) * 3 * HD + (1 + kv) * HD + h * 64 + c * 8);
    uint32_t am = 0;
    am = max_mag(am, v.x); am = max_mag(am, v.x >> 16);
    am = max_mag(am, v.y); am = max_mag(am, v.y >> 16);
    am = max_mag(am, v.z); am = max_mag(am, v.z >> 16);
    am = max_mag(am, v.w); am = max_mag(am, v.w >> 16);
    am = max(am, (uint32_t)__shfl_xor((int)am, 1, 64));
    am = max(am, (uint32_t)__shfl_xor((int)am, 2, 64));
    am = max(am, (uint32_t)__shfl_xor((int)am, 4, 64));
    const int e = kv_scale_exp(am);
    const float inv = __uint_as_float((uint32_t)(127 - e) << 23);  // 2^-e, e in [-64, 120]
    float f[8];
    unpack8(v, f);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = sat448(f[j] * inv);
    int lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], 0, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
    int hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], 0, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
    const long row = ((long)b * H + h) * Smax + pos;
    *reinterpret_cast<uint2*>((kv ? vc : kc) + row * 64 + c * 8) = make_uint2((uint32_t)lo, (uint32_t)hi);
    if (c == 0) (kv ? vsc : ksc)[row] = __uint_as_float((uint32_t)(127 + e) << 23);
  }
}

// 16 e4m3 codes -> 16 floats
__device__ __forceinline__ void decode16(const uint4& v, float* f) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false);
    const f32x2_t hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
    f[4 * i + 0] = lo[0]; f[4 * i + 1] = lo[1];
    f[4 * i + 2] = hi[0]; f[4 * i + 3] = hi[1];
  }
}

// sum over the 4 lanes of a DPP quad, result in all four (quad_perm [1,0,3,2], [2,3,0,1])
__device__ __forceinline__ float quad_sum(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, false));
  return v;
}

// One halving step of the cross-group reduction over lane bit O: acc[0 .. N/2) becomes the sum over the lane pair of the
// half that the lane's bit selects (bit set: the upper half).
template <int N, int O>
__device__ __forceinline__ void halve(float* acc, bool up) {
#pragma unroll
  for (int i = 0; i < N / 2; ++i) {
    const float keep = up ? acc[i + N / 2] : acc[i];
    const float send = up ? acc[i] : acc[i + N / 2];
    acc[i] = keep + __shfl_xor(send, O, 64);
  }
}

constexpr int ADF_KEYS = 16;  // key rows per load instruction of a wave (4 lanes x 16 bytes a row)

__global__ void __launch_bounds__(AD_WAVES * 64) attn_decode_fp8_part_kernel(
    const bf16_t* __restrict__ qkv, const uint8_t* __restrict__ kc, const uint8_t* __restrict__ vc,
    const float* __restrict__ ksc, const float* __restrict__ vsc, const long* __restrict__ lens,
    float* __restrict__ scratch, int H, int Smax, int nchunks, float scale) {
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
  const int g = lane >> 2, c = lane & 3;
  const long base = (long)bh * Smax;
  const int kw = k0 + wave * 32 + g;
  const bf16_t* qp = qkv + (long)b * 3 * H * 64 + h * 64 + c * 16;
  const uint4 qr[2] = {*reinterpret_cast<const uint4*>(qp), *reinterpret_cast<const uint4*>(qp + 8)};
  uint4 kr[2], vr[2];
  float ks[2], vs[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int key = kw + j * ADF_KEYS;
    const long row = base + (key < Smax ? key : Smax - 1);  // clamped: in bounds, masked below
    kr[j] = *reinterpret_cast<const uint4*>(kc + row * 64 + c * 16);
    vr[j] = *reinterpret_cast<const uint4*>(vc + row * 64 + c * 16);
    ks[j] = ksc[row];
    vs[j] = vsc[row];
  }
  __builtin_amdgcn_sched_barrier(0);  // the compiler otherwise sinks the V and scale loads below the K arithmetic
  float q[16];
  unpack8(qr[0], q);
  unpack8(qr[1], q + 8);

  float s[2];
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    float k[16];
    decode16(kr[j], k);
    float d = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) d += q[e] * k[e];
    d = quad_sum(d);
    s[j] = (kw + j * ADF_KEYS < n) ? d * ks[j] * scale : -INFINITY;
    m = fmaxf(m, s[j]);
  }
#pragma unroll
  for (int o = 4; o < 64; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, 64));

  float l = 0.f, acc[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const bool valid = kw + j * ADF_KEYS < n;
    const float p = valid ? __expf(s[j] - m) : 0.f;
    const float w = valid ? p * vs[j] : 0.f;
    float v[16];
    decode16(vr[j], v);
    l += p;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] += w * (valid ? v[e] : 0.f);
  }
#pragma unroll
  for (int o = 4; o < 64; o <<= 1) l += __shfl_xor(l, o, 64);
  halve<16, 4>(acc, g & 1);
  halve<8, 8>(acc, g & 2);
  halve<4, 16>(acc, g & 4);
  halve<2, 32>(acc, g & 8);
  // the lane's one output dim: the halves it kept, most significant first
  const int dim = c * 16 + ((g & 1) << 3 | (g & 2) << 1 | (g & 4) >> 1 | (g & 8) >> 3);
  if (lane == 0) {
    sm[wave][0] = m;
    sm[wave][1] = l;
  }
  sm[wave][2 + dim] = acc[0];
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
__global__ void __launch_bounds__(64) attn_decode_fp8_merge_kernel(const float* __restrict__ scratch,
                                                                   bf16_t* __restrict__ out, int nchunks) {
  const int bh = blockIdx.x, d = threadIdx.x;
  out[(long)bh * 64 + d] = merge_partials(scratch + (long)bh * nchunks * AD_PART, nchunks, d);
}

}  // namespace

// dtf_kv_store for an fp8 cache: qkv [B, S, 3*H*64] bf16 -> codes k / v [B, H, Smax, 64] uint8 and scales
// k_scale / v_scale [B, H, Smax] f32 at positions lens[b] + s (outside [0, Smax): dropped). lens is not changed.
DTF_API int dtf_kv_store_fp8(const void* qkv, void* k, void* v, float* k_scale, float* v_scale, const long* lens, int B,
                             int S, int H, int Smax, void* stream) {
  if (!qkv || !k || !v || !k_scale || !v_scale || !lens || B < 1 || S < 1 || H < 1 || Smax < 1) return -1;
  if (!aligned16(qkv) || !aligned16(k) || !aligned16(v) || ((uintptr_t)k_scale & 3) || ((uintptr_t)v_scale & 3))
    return -1;
  const long total = (long)B * S * H * 16;
  hipLaunchKernelGGL(kv_store_fp8_kernel, dim3(stream_grid(total, 256)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)qkv, (uint8_t*)k, (uint8_t*)v, k_scale, v_scale, lens, B, S, H, Smax);
  return (int)hipGetLastError();
}

// dtf_attn_decode over an fp8 cache; scratch as dtf_attn_decode's: B*H*ceil(Smax/chunk)*66 f32.
DTF_API int dtf_attn_decode_fp8(const void* qkv, const void* k, const void* v, const float* k_scale,
                                const float* v_scale, const long* lens, void* out, float* scratch, int B, int H,
                                int Smax, float scale, void* stream) {
  if (!qkv || !k || !v || !k_scale || !v_scale || !lens || !out || !scratch || B < 1 || H < 1 || Smax < 1) return -1;
  if (!aligned16(qkv) || !aligned16(k) || !aligned16(v) || ((uintptr_t)k_scale & 3) || ((uintptr_t)v_scale & 3))
    return -1;
  const int nchunks = cdiv(Smax, AD_CHUNK);
  if (nchunks > 65535) return -1;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(attn_decode_fp8_part_kernel, dim3(B * H, nchunks), dim3(AD_WAVES * 64), 0, st, (const bf16_t*)qkv,
                     (const uint8_t*)k, (const uint8_t*)v, k_scale, v_scale, lens, scratch, H, Smax, nchunks, scale);
  hipLaunchKernelGGL(attn_decode_fp8_merge_kernel, dim3(B * H), dim3(64), 0, st, (const float*)scratch, (bf16_t*)out,
                     nchunks);
  count_launch(LC_ATTN_DECODE_FP8);
  return (int)hipGetLastError();
}
