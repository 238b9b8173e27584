// Shared-prefix decode attention: G samples of one prompt read the prompt's K/V once.
//
// Batch row b of B0*G belongs to group g = b / G. With lim = min(lens[b], Smax_own - 1) and P = min(plens[g], lim),
// query b attends positions 0 .. lim: p < P from row g of the prefix cache [B0, H, Smax_prefix, 64], P <= p <= lim from
// row b of its own cache [B0*G, H, Smax_own, 64] (bf16 both). The token's own key (position lens[b], dtf_kv_store)
// therefore always comes from the own row, and the suffix is never empty. Three launches, all producing or consuming the
// 66-float (max, sum, o[64]) partials of attn_decode.h; the scratch has a prefix half and a suffix half of
// B0*G*H*nchunks partials each (the chunk that P falls into has one of either), nchunks = ceil(Smax_own / 128).
//
// Prefix pass, block (g*H + h, chunk): 128 prefix keys against all G queries of the group on the 16x16x32 bf16 MFMA.
//  * S^T = K Q^T: the K chunk goes from global memory straight into A-operand fragments (lane (r = lane % 16,
//    q4 = lane / 16) loads 16 bytes: key tile row r, dims 32 half + 8 q4 ..), a wave owns two 16-key tiles, d = 64 is
//    two MFMAs a tile, and all four K loads of a lane are issued before the first use. The B operand is the group's
//    query rows, columns >= G zero (never stored).
//  * accumulator layout: lane (r, q4) holds S^T[key 4 q4 + v][query r], v = 0..3, of both tiles: eight scores of one
//    query. Max and sum over the wave's 32 keys: in the lane, then over lane bits 4 and 5.
//  * O^T[64 dims x 16 queries] = V^T P^T, contraction over the wave's 32 keys. The eight probabilities a lane holds are
//    directly its B-operand fragment if contraction slot 8 q4 + 4 t + v stands for key 16 t + 4 q4 + v (any assignment
//    of keys to slots is valid as long as both operands use it). The V chunk (16 KB) is staged once per block by LDS-DMA
//    (rows at or past the group's prefix length are fetched out of the descriptor's range: zeros, so uninitialised
//    memory never arrives) and read back transposed with ds_read_b64_tr_b16 under the same key permutation: lane
//    (r, q4) addresses key row 16 t + 4 q4 + r / 4, dims 16 dt + 4 (r % 4) .., and receives dim 16 dt + r of the four
//    keys 16 t + 4 q4 + 0..3. 32-byte units of a row are XORed with (row / 2) % 4: the eight rows that two lane groups
//    read together fall on different banks.
//  * the four waves are merged in wave order through LDS; one partial per (row of the group, h, chunk).
// A key at or past a row's P is masked by select on the score and the probability; K rows are loaded from a clamped
// (in-bounds) address.
//
// Suffix pass: the split-KV pass of attn_decode.h over the row's own cache with the lower bound P; blocks whose chunk
// lies wholly outside [P, lim] exit. Merge: per (b, h) the prefix chunks 0 .. ceil(P/128)-1, then the suffix chunks
// floor(P/128) .. lim/128, in that order. Grids are sized by capacity only, nothing reads a device value on the host,
// no floating-point atomics: capturable and bitwise reproducible.
#include "attn_decode.h"
#include "lds_async.h"

namespace {

using namespace dtf;

constexpr int ADS_LDO = 68;  // f32 row stride of the cross-wave O tile: 16-byte aligned, 16 rows on 16 bank groups

struct SharedLens {
  int lim, P;
};
// lim and P of batch row b (group g): every bound clamped, so no index derived from them leaves a cache
__device__ __forceinline__ SharedLens shared_lens(const long* plens, const long* lens, int g, int b, int Smax_prefix,
                                                  int Smax_own) {
  long len = lens[b], pl = plens[g];
  len = len < 0 ? 0 : len;
  pl = pl < 0 ? 0 : pl;
  SharedLens s;
  s.lim = (int)(len < Smax_own - 1 ? len : Smax_own - 1);
  pl = pl < Smax_prefix ? pl : Smax_prefix;
  s.P = (int)(pl < s.lim ? pl : s.lim);
  return s;
}

__device__ __forceinline__ v8bf pack8bf(const float* f) {
  const uint4 u = make_uint4(pack2bf(f[0], f[1]), pack2bf(f[2], f[3]), pack2bf(f[4], f[5]), pack2bf(f[6], f[7]));
  return __builtin_bit_cast(v8bf, u);
}

__global__ void __launch_bounds__(AD_WAVES * 64) attn_shared_prefix_kernel(
    const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ kp, const bf16_t* __restrict__ vp,
    const long* __restrict__ plens, const long* __restrict__ lens, float* __restrict__ scratch, int G, int H,
    int Smax_prefix, int Smax_own, int nchunks, float scale) {
  __shared__ __attribute__((aligned(16))) char vs[AD_CHUNK * 128];  // V chunk [128 keys][64 dims] bf16, swizzled
  __shared__ __attribute__((aligned(16))) float so[AD_WAVES][16][ADS_LDO];
  __shared__ float sml[AD_WAVES][2][16];
  const int gh = blockIdx.x, chunk = blockIdx.y;
  const int g0 = gh / H, h = gh - g0 * H;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r = lane & 15, q4 = lane >> 4;
  const int k0 = chunk * AD_CHUNK;
  long pl = plens[g0];
  const int Pg = (int)(pl < 0 ? 0 : (pl < Smax_prefix ? pl : Smax_prefix));  // initialised rows of the group's prefix
  if (k0 >= Pg) return;

  // K fragments: tile t, dim half d2
  const bf16_t* kb = kp + (long)gh * Smax_prefix * 64 + q4 * 8;
  const int kw = k0 + wave * 32;
  uint4 kr[2][2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int key = kw + t * 16 + r;
    const long row = key < Smax_prefix ? key : Smax_prefix - 1;
#pragma unroll
    for (int d2 = 0; d2 < 2; ++d2) kr[t][d2] = *reinterpret_cast<const uint4*>(kb + row * 64 + d2 * 32);
  }
  // the query of column r (columns >= G: row 0 of the group, zeroed below)
  const bool col = r < G;
  const int b = g0 * G + (col ? r : 0);
  const bf16_t* qp = qkv + (long)b * 3 * H * 64 + h * 64 + q4 * 8;
  uint4 qr[2];
#pragma unroll
  for (int d2 = 0; d2 < 2; ++d2) qr[d2] = *reinterpret_cast<const uint4*>(qp + d2 * 32);
  // V chunk -> LDS: four DMA instructions a thread, each lane fetching the logical piece of its physical slot
  {
    const __amdgpu_buffer_rsrc_t rsrc = buf_rsrc(vp + (long)gh * Smax_prefix * 64, Smax_prefix * 128);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int pb = i * 4096 + tid * 16;
      const int row = pb >> 7, pc = (pb >> 4) & 7;
      const int c = pc ^ (((row >> 1) & 3) << 1);
      const uint32_t off = k0 + row < Pg ? (uint32_t)((k0 + row) * 128 + c * 16) : OOB_OFF;
      dma16(rsrc, vs + i * 4096 + wave * 1024, off);
    }
  }
  const SharedLens sl = shared_lens(plens, lens, g0, b, Smax_prefix, Smax_own);
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
  if (!col) qr[0] = qr[1] = zero;

  float s[2][4];
  float m = -INFINITY;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    v4f acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int d2 = 0; d2 < 2; ++d2)
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, kr[t][d2]),
                                                    __builtin_bit_cast(v8bf, qr[d2]), acc, 0, 0, 0);
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      s[t][v] = (kw + t * 16 + 4 * q4 + v < sl.P) ? acc[v] * scale : -INFINITY;
      m = fmaxf(m, s[t][v]);
    }
  }
  m = fmaxf(m, __shfl_xor(m, 16, 64));
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  float p[8];
  float l = 0.f;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      p[t * 4 + v] = (kw + t * 16 + 4 * q4 + v < sl.P) ? __expf(s[t][v] - m) : 0.f;
      l += p[t * 4 + v];
    }
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  const v8bf pf = pack8bf(p);

  vm_wait<0>();     // this thread's DMA has landed ...
  __syncthreads();  // ... and everybody's
  v4f o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    v4s vr[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int row = wave * 32 + t * 16 + 4 * q4 + (r >> 2);
      const int gr = (dt * 4 + (r & 3)) ^ (((row >> 1) & 3) << 2);
      vr[t] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(v4s, vs + row * 128 + gr * 8));
    }
    const v8s both = __builtin_shufflevector(vr[0], vr[1], 0, 1, 2, 3, 4, 5, 6, 7);
    o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, both), pf,
                                                    (v4f){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
  }
  // lane (r, q4) holds O^T[dim 16 dt + 4 q4 + v][query r]
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) *reinterpret_cast<v4f*>(&so[wave][r][dt * 16 + 4 * q4]) = o[dt];
  if (q4 == 0) {
    sml[wave][0][r] = m;
    sml[wave][1][r] = l;
  }
  __syncthreads();
  const int d = tid & 63;
  for (int j = tid >> 6; j < G; j += AD_WAVES) {  // merge the four waves of query j in wave order
    float mm = sml[0][0][j];
#pragma unroll
    for (int w = 1; w < AD_WAVES; ++w) mm = fmaxf(mm, sml[w][0][j]);
    float ll = 0.f, a = 0.f;
#pragma unroll
    for (int w = 0; w < AD_WAVES; ++w) {
      const float mw = sml[w][0][j];
      const float f = mw == -INFINITY ? 0.f : __expf(mw - mm);
      ll += f * sml[w][1][j];
      a += f * so[w][j][d];
    }
    float* part = scratch + (((long)(g0 * G + j) * H + h) * nchunks + chunk) * AD_PART;
    part[2 + d] = a;
    if (d == 0) {
      part[0] = mm;
      part[1] = ll;
    }
  }
}

// attn_decode_part_kernel's stream over keys max(P, chunk*128) .. min(lim, chunk*128 + 127) of the row's own cache.
// BEAM (dtf_attn_decode_beam): the key and value of position p are those of physical row (b / G) * G + slots[b, p] of
// the own cache, slots [B0*G, Smax] uint8, except position lens[b] (the token dtf_kv_store has just put there), which
// is row b's own. A lane fetches the table byte of each of its four keys (at the clamped position, and clamped to
// G - 1: the address stays inside the group's rows whatever the table holds), then issues all eight loads as before.
template <bool BEAM>
__global__ void __launch_bounds__(AD_WAVES * 64) attn_shared_suffix_kernel(
    const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ kc, const bf16_t* __restrict__ vc,
    const long* __restrict__ plens, const long* __restrict__ lens, float* __restrict__ part0, int G, int H,
    int Smax_prefix, int Smax, int nchunks, float scale, const unsigned char* __restrict__ slots) {
  __shared__ float sm[AD_WAVES][AD_PART];
  const int bh = blockIdx.x, chunk = blockIdx.y;
  const int b = bh / H, h = bh - b * H;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const SharedLens sl = shared_lens(plens, lens, b / G, b, Smax_prefix, Smax);
  const int k0 = chunk * AD_CHUNK;
  if (k0 > sl.lim || k0 + AD_CHUNK <= sl.P) return;  // the merge reads chunks P/128 .. lim/128 only
  const int g = lane >> 3, c = lane & 7;
  const bf16_t* kb = kc + (long)bh * Smax * 64 + c * 8;
  const bf16_t* vb = vc + (long)bh * Smax * 64 + c * 8;
  const int kw = k0 + wave * 32 + g;
  uint4 kr[4], vr[4];
  if (BEAM) {
    const long own = lens[b];
    const int r0 = b / G * G;
    int slot[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int key = kw + j * 8;
      slot[j] = slots[(long)b * Smax + (key < Smax ? key : Smax - 1)];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int key = kw + j * 8;
      const long row = key < Smax ? key : Smax - 1;
      const int src = row == own ? b : r0 + (slot[j] < G ? slot[j] : G - 1);
      const long at = (((long)src * H + h) * Smax + row) * 64 + c * 8;
      kr[j] = *reinterpret_cast<const uint4*>(kc + at);
      vr[j] = *reinterpret_cast<const uint4*>(vc + at);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int key = kw + j * 8;
      const long row = key < Smax ? key : Smax - 1;
      kr[j] = *reinterpret_cast<const uint4*>(kb + row * 64);
      vr[j] = *reinterpret_cast<const uint4*>(vb + row * 64);
    }
  }
  float q[8];
  load8(qkv + (long)b * 3 * H * 64 + h * 64 + c * 8, q);

  float s[4];
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int key = kw + j * 8;
    float k[8];
    unpack8(kr[j], k);
    float d = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) d += q[e] * k[e];
    d += __shfl_xor(d, 1, 64);
    d += __shfl_xor(d, 2, 64);
    d += __shfl_xor(d, 4, 64);
    s[j] = (key >= sl.P && key <= sl.lim) ? d * scale : -INFINITY;
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
    const int key = kw + j * 8;
    const bool valid = key >= sl.P && key <= sl.lim;
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
  if (tid < 64) {  // the four waves in wave order (a wave without a valid key holds max -inf, sum 0)
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
    float* part = part0 + ((long)bh * nchunks + chunk) * AD_PART;
    part[2 + tid] = a;
    if (tid == 0) {
      part[0] = mm;
      part[1] = ll;
    }
  }
}

// Per (b, h): prefix partials 0 .. ceil(P/128)-1, then suffix partials P/128 .. lim/128; thread = output dim.
__global__ void __launch_bounds__(64) attn_shared_merge_kernel(const float* __restrict__ scratch,
                                                               const long* __restrict__ plens,
                                                               const long* __restrict__ lens, bf16_t* __restrict__ out,
                                                               int G, int H, int Smax_prefix, int Smax_own, int nchunks,
                                                               long half) {
  const int bh = blockIdx.x, d = threadIdx.x;
  const int b = bh / H;
  const SharedLens sl = shared_lens(plens, lens, b / G, b, Smax_prefix, Smax_own);
  const float* pre = scratch + (long)bh * nchunks * AD_PART;
  const float* suf = pre + half;
  const int npre = (sl.P + AD_CHUNK - 1) / AD_CHUNK, s0 = sl.P / AD_CHUNK, s1 = sl.lim / AD_CHUNK;
  float mm = -INFINITY;
  for (int c = 0; c < npre; ++c) mm = fmaxf(mm, pre[c * AD_PART]);
  for (int c = s0; c <= s1; ++c) mm = fmaxf(mm, suf[c * AD_PART]);
  float l = 0.f, a = 0.f;
  for (int c = 0; c < npre; ++c) {
    const float mc = pre[c * AD_PART];
    const float f = mc == -INFINITY ? 0.f : __expf(mc - mm);
    l += f * pre[c * AD_PART + 1];
    a += f * pre[c * AD_PART + 2 + d];
  }
  for (int c = s0; c <= s1; ++c) {
    const float mc = suf[c * AD_PART];
    const float f = mc == -INFINITY ? 0.f : __expf(mc - mm);
    l += f * suf[c * AD_PART + 1];
    a += f * suf[c * AD_PART + 2 + d];
  }
  out[(long)bh * 64 + d] = f2bf(a / l);  // position lim is a suffix key: l > 0
}

// slots: null (every row reads its own cache) or the beam table of the suffix pass
int launch_shared(const void* qkv, const void* k_prefix, const void* v_prefix, const void* k_own, const void* v_own,
                  const long* plens, const long* lens, void* out, float* scratch, int B0, int G, int H,
                  int Smax_prefix, int Smax_own, float scale, const unsigned char* slots, void* stream) {
  if (!qkv || !k_prefix || !v_prefix || !k_own || !v_own || !plens || !lens || !out || !scratch) return -1;
  if (B0 < 1 || G < 2 || G > 16 || H < 1 || Smax_prefix < 1 || Smax_own < 1) return -1;
  if (!aligned16(qkv) || !aligned16(k_prefix) || !aligned16(v_prefix) || !aligned16(k_own) || !aligned16(v_own))
    return -1;
  const int nchunks = cdiv(Smax_own, AD_CHUNK);
  if (nchunks > 65535 || (long)Smax_prefix * 128 >= (1L << 31)) return -1;  // (the V slab of a head: one descriptor)
  hipStream_t st = (hipStream_t)stream;
  const int B = B0 * G;
  const long half = (long)B * H * nchunks * AD_PART;
  hipLaunchKernelGGL(attn_shared_prefix_kernel, dim3(B0 * H, nchunks), dim3(AD_WAVES * 64), 0, st, (const bf16_t*)qkv,
                     (const bf16_t*)k_prefix, (const bf16_t*)v_prefix, plens, lens, scratch, G, H, Smax_prefix,
                     Smax_own, nchunks, scale);
  if (slots)
    hipLaunchKernelGGL(attn_shared_suffix_kernel<true>, dim3(B * H, nchunks), dim3(AD_WAVES * 64), 0, st,
                       (const bf16_t*)qkv, (const bf16_t*)k_own, (const bf16_t*)v_own, plens, lens, scratch + half, G,
                       H, Smax_prefix, Smax_own, nchunks, scale, slots);
  else
    hipLaunchKernelGGL(attn_shared_suffix_kernel<false>, dim3(B * H, nchunks), dim3(AD_WAVES * 64), 0, st,
                       (const bf16_t*)qkv, (const bf16_t*)k_own, (const bf16_t*)v_own, plens, lens, scratch + half, G,
                       H, Smax_prefix, Smax_own, nchunks, scale, slots);
  hipLaunchKernelGGL(attn_shared_merge_kernel, dim3(B * H), dim3(64), 0, st, (const float*)scratch, plens, lens,
                     (bf16_t*)out, G, H, Smax_prefix, Smax_own, nchunks, half);
  return (int)hipGetLastError();
}

}  // namespace

// One query row per (b, h) from qkv [B0*G, 1, 3*H*64]; k_prefix / v_prefix [B0, H, Smax_prefix, 64] shared by the G rows
// of a group up to plens[B0], k_own / v_own [B0*G, H, Smax_own, 64] behind it up to lens[B0*G]; out [B0*G, 1, H*64]
// bf16; scratch: B0*G*H*2*ceil(Smax_own/chunk)*66 f32.
DTF_API int dtf_attn_decode_shared(const void* qkv, const void* k_prefix, const void* v_prefix, const void* k_own,
                                   const void* v_own, const long* plens, const long* lens, void* out, float* scratch,
                                   int B0, int G, int H, int Smax_prefix, int Smax_own, float scale, void* stream) {
  return launch_shared(qkv, k_prefix, v_prefix, k_own, v_own, plens, lens, out, scratch, B0, G, H, Smax_prefix,
                       Smax_own, scale, nullptr, stream);
}

// The same for beams: slots [B0*G, Smax_own] uint8 names, per row and own position, the physical row of the group
// (0 .. G-1) whose k_own / v_own hold that position; position lens[b] is always row b's own.
DTF_API int dtf_attn_decode_beam(const void* qkv, const void* k_prefix, const void* v_prefix, const void* k_own,
                                 const void* v_own, const long* plens, const long* lens, const void* slots, void* out,
                                 float* scratch, int B0, int G, int H, int Smax_prefix, int Smax_own, float scale,
                                 void* stream) {
  if (!slots) return -1;
  const int rc = launch_shared(qkv, k_prefix, v_prefix, k_own, v_own, plens, lens, out, scratch, B0, G, H,
                               Smax_prefix, Smax_own, scale, (const unsigned char*)slots, stream);
  if (rc == 0) count_launch(LC_ATTN_DECODE_BEAM);
  return rc;
}
