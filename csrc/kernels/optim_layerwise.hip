// Layer-wise adaptive optimizers (LARS, LAMB) over flat parameter arenas.
//
// Both rules scale each variable's step by a ratio of per-variable L2 norms, so one elementwise launch (optim.hip)
// is not enough. The arena is cut once, on the host, into a static TILE TABLE: rows of
//   (param offset, grad offset, length, variable index)
// that never cross a variable boundary, hold at most LW_TILE elements, have lengths that are multiples of 16 and
// list a variable's tiles consecutively (variable indices never decrease along the table). A tile may cover the
// variable's zero padding: padding has w = g = slots = 0, adds 0 to every norm and stays 0 under both rules.
// One step is three launches over that table:
//   pass 1    grid-stride over tiles. LAMB: m, v updated, the un-scaled step u written INTO THE GRADIENT BUFFER
//             (the step zeroes it anyway), partial sum w^2 / sum u^2 per tile. LARS: partial sum w^2 / sum g^2 only.
//   finalize  one wave per variable: the variable's tile partials summed in table order, scale[var] = trust ratio.
//             For sharded optimizer state (ZeRO-1) it runs in two halves (sum -> [nvars][2], all-reduce, scale).
//   pass 2    grid-stride over the same tiles. LAMB: w -= lr*scale*u. LARS: the momentum rule of optim.hip with
//             lr*scale. Both write the bf16 copy and zero the gradient.
// Reductions are deterministic: a fixed shuffle tree per block, one partial per tile, ordered sums per variable; no
// float atomics. Per-step scalars come from the same device row as optim.hip (hp[0] lr, hp[1] grad scale, hp[2]
// clip threshold) plus hp[4] = 1/(1-b1^t) and hp[5] = 1/(1-b2^t) for LAMB; every launch reads the step's abort flag
// and applies nothing when it is set.
#include "common.h"

namespace {

constexpr int LW_TILE = 4096;             // elements per tile at most
constexpr int LW_U = 2;                   // float4 groups per thread per trip, all loads before the math
constexpr int LW_TRIP = 256 * LW_U;       // float4 groups per block per trip (LW_TILE / 4 / LW_TRIP trips a tile)

enum LwKind : int { LW_LAMB = 6, LW_LARS = 7 };  // numbering continues optim.hip's OptKind
enum LwFlag : int { LW_DECAY = 1, LW_ADAPT = 2 };
enum LwMode : int { LW_SUM = 1, LW_SCALE = 2 };

struct LwTile {
  long po, go, len, var;
};

struct LwArgs {
  const LwTile* tiles;
  int ntiles, nvars;
  float* p;
  float* g;
  float* s1;
  float* s2;
  bf16_t* p16;
  const int* flags;   // [nvars] LwFlag bits
  float* partials;    // [ntiles][2]
  float* sums;        // [nvars][2] (optional outside ZeRO-1)
  float* scale;       // [nvars]
  float b1, b2, omb1, omb2, eps, wd, mom, eeta;  // omb = 1 - b, rounded once from the host's double
  int nesterov, zero_grad;
  const float* hp;
  const float* sumsq;
  const int* abort;
};

typedef float nt4f __attribute__((ext_vector_type(4)));
typedef unsigned int nt2u __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float4 ld_nt(const float* p, long i) {
  const nt4f v = __builtin_nontemporal_load(reinterpret_cast<const nt4f*>(p) + i);
  return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void st_nt(float* p, long i, float4 v) {
  __builtin_nontemporal_store((nt4f){v.x, v.y, v.z, v.w}, reinterpret_cast<nt4f*>(p) + i);
}

__device__ __forceinline__ bool aborted(const LwArgs& a) {
  return a.abort && __hip_atomic_load(a.abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// gradient scale with the global-norm clip factor folded in, exactly as optim_kernel computes it
__device__ __forceinline__ float grad_scale(const LwArgs& a) {
  float gs = a.hp[1];
  if (a.sumsq && a.hp[2] > 0.f) {
    float nrm = sqrtf(*a.sumsq) * gs;
    if (nrm > a.hp[2]) gs *= a.hp[2] / nrm;
  }
  return gs;
}

__device__ __forceinline__ float sq4(float4 v) { return v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w; }

__device__ __forceinline__ void lamb1(const LwArgs& a, float gs, float c1, float c2, float wd, float w, float& g,
                                      float& m, float& v) {
  g *= gs;
  m = a.b1 * m + a.omb1 * g;
  v = a.b2 * v + a.omb2 * g * g;
  g = (m * c1) / (sqrtf(v * c2) + a.eps) + wd * w;  // u, kept in the gradient's register
}

template <int KIND>
__global__ void __launch_bounds__(256) lw_pass1_kernel(LwArgs a) {
  __shared__ float red[16];
  if (aborted(a)) return;
  const float gs = grad_scale(a);
  const float c1 = a.hp[4], c2 = a.hp[5];
  for (int t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    const LwTile tl = a.tiles[t];
    const long p4 = tl.po >> 2, g4 = tl.go >> 2;
    const int n4 = (int)(tl.len >> 2);
    const float wd = (a.flags[tl.var] & LW_DECAY) ? a.wd : 0.f;
    float sw = 0.f, sx = 0.f;
#pragma unroll 1
    for (int i0 = threadIdx.x; i0 < n4; i0 += LW_TRIP) {
      float4 w[LW_U], g[LW_U], m[LW_U], v[LW_U];
#pragma unroll
      for (int u = 0; u < LW_U; ++u) {
        const int i = i0 + u * 256;
        if (i < n4) {
          w[u] = ld_nt(a.p, p4 + i);
          g[u] = ld_nt(a.g, g4 + i);
          if (KIND == LW_LAMB) {
            m[u] = ld_nt(a.s1, p4 + i);
            v[u] = ld_nt(a.s2, p4 + i);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < LW_U; ++u) {
        const int i = i0 + u * 256;
        if (i >= n4) break;
        if (KIND == LW_LAMB) {
          lamb1(a, gs, c1, c2, wd, w[u].x, g[u].x, m[u].x, v[u].x);
          lamb1(a, gs, c1, c2, wd, w[u].y, g[u].y, m[u].y, v[u].y);
          lamb1(a, gs, c1, c2, wd, w[u].z, g[u].z, m[u].z, v[u].z);
          lamb1(a, gs, c1, c2, wd, w[u].w, g[u].w, m[u].w, v[u].w);
          st_nt(a.s1, p4 + i, m[u]);
          st_nt(a.s2, p4 + i, v[u]);
          st_nt(a.g, g4 + i, g[u]);
        } else {
          g[u].x *= gs; g[u].y *= gs; g[u].z *= gs; g[u].w *= gs;
        }
        sw += sq4(w[u]);
        sx += sq4(g[u]);
      }
    }
    sw = block_sum(sw, red);
    sx = block_sum(sx, red);
    if (threadIdx.x == 0) {
      a.partials[2 * (long)t] = sw;
      a.partials[2 * (long)t + 1] = sx;
    }
  }
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// first tile whose variable index is >= var (the table's variable indices never decrease)
__device__ __forceinline__ int first_tile_of(const LwTile* tiles, int ntiles, long var) {
  int lo = 0, hi = ntiles;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tiles[mid].var < var) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// one wave per variable
__global__ void __launch_bounds__(256) lw_finalize_kernel(LwArgs a, int kind, int mode) {
  if (aborted(a)) return;
  const int var = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (var >= a.nvars) return;
  float A, B;
  if (mode & LW_SUM) {
    const int lo = first_tile_of(a.tiles, a.ntiles, var), hi = first_tile_of(a.tiles, a.ntiles, var + 1);
    double sa = 0.0, sb = 0.0;
    // lane l adds tiles lo+l, lo+l+64, ... in that order; four loads in flight per trip
    const float2* part = reinterpret_cast<const float2*>(a.partials);
    for (int t = lo + lane; t < hi; t += 256) {
      float2 q[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) q[k] = t + 64 * k < hi ? part[t + 64 * k] : make_float2(0.f, 0.f);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        sa += (double)q[k].x;
        sb += (double)q[k].y;
      }
    }
    A = (float)wave_sum_f64(sa);
    B = (float)wave_sum_f64(sb);
    if (a.sums && lane == 0) {
      a.sums[2 * var] = A;
      a.sums[2 * var + 1] = B;
    }
  } else {
    A = a.sums[2 * var];
    B = a.sums[2 * var + 1];
  }
  if ((mode & LW_SCALE) && lane == 0) {
    const int f = a.flags[var];
    float r = 1.f;
    if ((f & LW_ADAPT) && A > 0.f && B > 0.f) {
      const float wn = sqrtf(A), xn = sqrtf(B);
      if (kind == LW_LAMB) r = wn / xn;
      else r = a.eeta * wn / (xn + ((f & LW_DECAY) ? a.wd : 0.f) * wn + a.eps);
    }
    a.scale[var] = r;
  }
}

// optim.hip's OPT_SGD momentum rule with lr*scale in place of lr
__device__ __forceinline__ void lars1(const LwArgs& a, float r, float gs, float wd, float& w, float g, float& m) {
  g *= gs;
  if (wd != 0.f) g += wd * w;
  m = a.mom * m + g;
  w -= r * (a.nesterov ? g + a.mom * m : m);
}

template <int KIND>
__global__ void __launch_bounds__(256) lw_pass2_kernel(LwArgs a) {
  if (aborted(a)) return;
  const float lr = a.hp[0];
  const float gs = KIND == LW_LARS ? grad_scale(a) : 1.f;
  for (int t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    const LwTile tl = a.tiles[t];
    const long p4 = tl.po >> 2, g4 = tl.go >> 2;
    const int n4 = (int)(tl.len >> 2);
    const float r = lr * a.scale[tl.var];
    const float wd = (a.flags[tl.var] & LW_DECAY) ? a.wd : 0.f;
#pragma unroll 1
    for (int i0 = threadIdx.x; i0 < n4; i0 += LW_TRIP) {
      float4 w[LW_U], g[LW_U], m[LW_U];
#pragma unroll
      for (int u = 0; u < LW_U; ++u) {
        const int i = i0 + u * 256;
        if (i < n4) {
          w[u] = ld_nt(a.p, p4 + i);
          g[u] = ld_nt(a.g, g4 + i);
          if (KIND == LW_LARS) m[u] = ld_nt(a.s1, p4 + i);
        }
      }
#pragma unroll
      for (int u = 0; u < LW_U; ++u) {
        const int i = i0 + u * 256;
        if (i >= n4) break;
        if (KIND == LW_LAMB) {
          w[u].x -= r * g[u].x;
          w[u].y -= r * g[u].y;
          w[u].z -= r * g[u].z;
          w[u].w -= r * g[u].w;
        } else {
          lars1(a, r, gs, wd, w[u].x, g[u].x, m[u].x);
          lars1(a, r, gs, wd, w[u].y, g[u].y, m[u].y);
          lars1(a, r, gs, wd, w[u].z, g[u].z, m[u].z);
          lars1(a, r, gs, wd, w[u].w, g[u].w, m[u].w);
        }
        st_nt(a.p, p4 + i, w[u]);
        if (KIND == LW_LARS) st_nt(a.s1, p4 + i, m[u]);
        if (a.zero_grad) st_nt(a.g, g4 + i, make_float4(0, 0, 0, 0));
        if (a.p16) {
          __builtin_nontemporal_store((nt2u){pack2bf(w[u].x, w[u].y), pack2bf(w[u].z, w[u].w)},
                                      reinterpret_cast<nt2u*>(a.p16) + p4 + i);
        }
      }
    }
  }
}

// A bad table must never reach the GPU: every tile inside both buffers, 16-byte accesses, variable index in range
// and never decreasing (a variable's tiles are consecutive).
bool table_ok(const long* th, int ntiles, int nvars, long n_param, long n_grad) {
  if (!th || ntiles < 1 || nvars < 1 || n_param < 0 || n_grad < 0) return false;
  long prev = 0;
  for (int t = 0; t < ntiles; ++t) {
    const long po = th[4 * t], go = th[4 * t + 1], len = th[4 * t + 2], var = th[4 * t + 3];
    if (len < 0 || len > LW_TILE || ((po | go | len) & 3)) return false;
    if (po < 0 || po > n_param - len || go < 0 || go > n_grad - len) return false;
    if (var < prev || var >= nvars) return false;
    prev = var;
  }
  return true;
}

int tile_grid(int ntiles) { return ntiles < 2048 ? ntiles : 2048; }

}  // namespace

DTF_API int dtf_lw_tile_elems() { return LW_TILE; }

DTF_API int dtf_lw_pass1(int kind, const long* tiles_host, const void* tiles_dev, int ntiles, int nvars,
                         long n_param, long n_grad, float* p, float* g, float* s1, float* s2, const int* flags,
                         float* partials, float b1, float b2, float omb1, float omb2, float eps, float wd,
                         const float* hp, const float* sumsq, const int* abort, void* stream) {
  if (kind != LW_LAMB && kind != LW_LARS) return -1;
  if (!table_ok(tiles_host, ntiles, nvars, n_param, n_grad)) return -1;
  if (!tiles_dev || !p || !g || !flags || !partials || !hp || !aligned16(p) || !aligned16(g)) return -1;
  if (kind == LW_LAMB && (!s1 || !s2 || !aligned16(s1) || !aligned16(s2))) return -1;
  LwArgs a = {};
  a.tiles = (const LwTile*)tiles_dev; a.ntiles = ntiles; a.nvars = nvars;
  a.p = p; a.g = g; a.s1 = s1; a.s2 = s2; a.flags = flags; a.partials = partials;
  a.b1 = b1; a.b2 = b2; a.omb1 = omb1; a.omb2 = omb2; a.eps = eps; a.wd = wd; a.hp = hp; a.sumsq = sumsq; a.abort = abort;
  const dim3 grid(tile_grid(ntiles)), block(256);
  if (kind == LW_LAMB) hipLaunchKernelGGL((lw_pass1_kernel<LW_LAMB>), grid, block, 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((lw_pass1_kernel<LW_LARS>), grid, block, 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

DTF_API int dtf_lw_finalize(int kind, int mode, const long* tiles_host, const void* tiles_dev, int ntiles, int nvars,
                            long n_param, long n_grad, const float* partials, float* sums, const int* flags,
                            float* scale, float wd, float eeta, float eps, const int* abort, void* stream) {
  if (kind != LW_LAMB && kind != LW_LARS) return -1;
  if (mode < 1 || mode > (LW_SUM | LW_SCALE)) return -1;
  if (!table_ok(tiles_host, ntiles, nvars, n_param, n_grad)) return -1;
  if (!tiles_dev || !partials || !flags) return -1;
  if ((mode & LW_SCALE) && !scale) return -1;
  if (mode != (LW_SUM | LW_SCALE) && !sums) return -1;
  LwArgs a = {};
  a.tiles = (const LwTile*)tiles_dev; a.ntiles = ntiles; a.nvars = nvars;
  a.partials = const_cast<float*>(partials); a.sums = sums; a.flags = flags; a.scale = scale;
  a.wd = wd; a.eeta = eeta; a.eps = eps; a.abort = abort;
  hipLaunchKernelGGL(lw_finalize_kernel, dim3(cdiv(nvars, 4)), dim3(256), 0, (hipStream_t)stream, a, kind, mode);
  return (int)hipGetLastError();
}

DTF_API int dtf_lw_pass2(int kind, const long* tiles_host, const void* tiles_dev, int ntiles, int nvars,
                         long n_param, long n_grad, float* p, float* g, float* s1, void* p16, const float* scale,
                         const int* flags, float wd, float mom, int nesterov, int zero_grad, const float* hp,
                         const float* sumsq, const int* abort, void* stream) {
  if (kind != LW_LAMB && kind != LW_LARS) return -1;
  if (!table_ok(tiles_host, ntiles, nvars, n_param, n_grad)) return -1;
  if (!tiles_dev || !p || !g || !scale || !flags || !hp || !aligned16(p) || !aligned16(g)) return -1;
  if (kind == LW_LARS && (!s1 || !aligned16(s1))) return -1;
  if (p16 && ((uintptr_t)p16 & 7)) return -1;
  LwArgs a = {};
  a.tiles = (const LwTile*)tiles_dev; a.ntiles = ntiles; a.nvars = nvars;
  a.p = p; a.g = g; a.s1 = s1; a.p16 = (bf16_t*)p16; a.scale = const_cast<float*>(scale); a.flags = flags;
  a.wd = wd; a.mom = mom; a.nesterov = nesterov; a.zero_grad = zero_grad;
  a.hp = hp; a.sumsq = sumsq; a.abort = abort;
  const dim3 grid(tile_grid(ntiles)), block(256);
  if (kind == LW_LAMB) hipLaunchKernelGGL((lw_pass2_kernel<LW_LAMB>), grid, block, 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((lw_pass2_kernel<LW_LARS>), grid, block, 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}
