// The weight-streaming dense layer of a decode step with 17 to 64 rows (accepted from 1 row): dtf_dense_wide.
//
// out[M, N] = act(x[M, K] w[N, K]^T + bias), 1 <= M <= 64; x, w, out bf16 (row-major, dense), bias f32 or null, f32
// accumulation. The principle is dense_skinny_kernel's (attn_decode.h): the weights are a stream read exactly once from
// HBM in 16-byte loads that go straight to VGPRs, as the first operand of the 16x16x32 bf16 MFMA; x is the 16-column
// second operand. Here x spans MT = cdiv(M, 16) column tiles (a compile-time parameter: a 17-row call runs two tiles,
// not four), and every weight fragment feeds MT MFMAs into MT accumulators. Rows >= M of the last tile are loaded from
// row 0 (in bounds) and made zero by select.
//
// Form kept: (a) of the two the design considered. A block owns R * T weight rows over the full K; its four waves split
// K (wave w takes the K pieces (4 * it + w) * U .. + U - 1, U consecutive pieces of KW = 32 * S elements, so a wave
// reads U * KW * 2 contiguous bytes of each of its rows per batch), every wave loads its own x fragments from global
// memory (x is at most 64 * K * 2 bytes and stays in L2), and the four partial sums are added in wave order through
// LDS. Each x fragment a wave loads is used by all T row groups of the block. Form (b), the waves on different rows
// sharing x through an LDS tile, was not built: with 64 * T rows a block it leaves N = 1024 with at most 16 blocks
// unless K is also split across blocks, and this entry point has no scratch for slabs.
//
// R = 16: the 16 tile rows are 16 weight rows (S = 1). R = 8: dense_skinny's sub-range layout with S = 2 (tile row =
// sub * 8 + row, the two halves of the tile hold the same 8 rows at two consecutive 32-element K sub-ranges, one MFMA
// per sub-range and tile of x, of whose result only the rows of that sub-range are read); it halves the rows per block
// where N is small. S = 4 is not offered: its reduction buffer alone would be 64 KB at MT = 4.
//
// Loads run one batch ahead in registers: the loads of batch it + 1 (weights and x) are issued before the MFMAs of
// batch it, in two register sets that alternate, so a wave always has a batch in flight while it computes.
//
// x bytes read (from L2) per weight byte read (from HBM) by a block, 16 * MT * S / (R * T):
//   (R, T)    MT=1   MT=2   MT=3   MT=4      rows per block
//   ( 8, 1)    4      8     12     16          8
//   (16, 1)    1      2      3      4         16
//   (16, 2)    0.5    1      1.5    2         32
//   (16, 4)    0.25   0.5    0.75   1         64
//
// The cross-wave reduction goes row group by row group: red[4][S * MT][256] f32 (at most 32 KB static LDS, nothing
// dynamic) is filled and summed T times. Summation order: the K pieces of a wave in order inside the MFMA accumulator,
// then sub-range 0, 1, each over waves 0, 1, 2, 3. No atomics; nothing is read on the host; the launch depends on
// (M, N, K) alone, so two calls, and an eager call and a captured replay, give the same bits.
#include "attn_decode.h"

namespace {

template <int R, int T, int MT>
__global__ void __launch_bounds__(256) dense_wide_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
                                                         const float* __restrict__ bias, bf16_t* __restrict__ out,
                                                         int M, int N, int K, int act) {
  constexpr int S = 16 / R;
  constexpr int KW = 32 * S;                      // K elements of each weight row per piece
  constexpr int U = (T == 1 && S == 1) ? 4 : 2;   // pieces per batch of a wave
  static_assert(S == 1 || S == 2, "the reduction buffer is sized for S <= 2");
  __shared__ __attribute__((aligned(16))) float red[4][S * MT][256];
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
  const bf16_t* xp[MT];
  bool xok[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    xok[mt] = mt * 16 + r < M;
    xp[mt] = x + (long)(xok[mt] ? mt * 16 + r : 0) * K;
  }
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
  v4f acc[T][S][MT];
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[t][s][mt] = (v4f){0.f, 0.f, 0.f, 0.f};

  struct Batch {
    uint4 a[U][T], b[U][S][MT];
  };
  // a piece past K loads a clamped (in-bounds) address; `mma` makes it zero
  auto load = [&](Batch& q, int it) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k0 = ((it * 4 + wave) * U + u) * KW + g * 8;
      const int ka = k0 + sub * 32;
#pragma unroll
      for (int t = 0; t < T; ++t) q.a[u][t] = *reinterpret_cast<const uint4*>(wp[t] + (ka < K ? ka : K - 8));
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const int kx = k0 + s * 32;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
          q.b[u][s][mt] = *reinterpret_cast<const uint4*>(xp[mt] + (kx < K ? kx : K - 8));
      }
    }
  };
  auto mma = [&](Batch& q, int it) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k0 = ((it * 4 + wave) * U + u) * KW + g * 8;
#pragma unroll
      for (int s = 0; s < S; ++s)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
          if (k0 + s * 32 >= K || !xok[mt]) q.b[u][s][mt] = zero;
#pragma unroll
      for (int t = 0; t < T; ++t) {
        if (k0 + sub * 32 >= K) q.a[u][t] = zero;
#pragma unroll
        for (int s = 0; s < S; ++s)
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
            acc[t][s][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                __builtin_bit_cast(v8bf, q.a[u][t]), __builtin_bit_cast(v8bf, q.b[u][s][mt]), acc[t][s][mt], 0, 0, 0);
      }
    }
  };
  const int nbatch = (K + 4 * U * KW - 1) / (4 * U * KW);  // the same count for every wave
  Batch q0, q1;
  load(q0, 0);
  for (int it = 0; it < nbatch; it += 2) {
    load(q1, it + 1);  // (past the last batch: clamped loads that are never used)
    mma(q0, it);
    if (it + 1 < nbatch) {
      load(q0, it + 2);
      mma(q1, it + 1);
    }
  }

  // accumulator layout: lane holds D[i = 4 * g + v][j = r] (i: tile row, j: x row of the tile); red is [j][i], so a
  // lane stores its four values as one 16-byte piece and thread tid reads element tid
  const int i = tid & 15, j = tid >> 4;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    if (t) __syncthreads();
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) *reinterpret_cast<v4f*>(&red[wave][s * MT + mt][r * 16 + 4 * g]) = acc[t][s][mt];
    __syncthreads();
    const int n = n0 + t * R + i;
    if (i < R && n < N) {
      const float bv = bias ? bias[n] : 0.f;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int m = mt * 16 + j;
        float val = 0.f;
#pragma unroll
        for (int s = 0; s < S; ++s)
#pragma unroll
          for (int wv = 0; wv < 4; ++wv) val += red[wv][s * MT + mt][j * 16 + s * R + i];
        if (m < M) {
          val += bv;
          if (act == 1) val = fmaxf(val, 0.f);
          else if (act == 2) val = skinny_gelu(val);
          out[(long)m * N + n] = f2bf(val);
        }
      }
    }
  }
}

constexpr int WIDE_VARIANTS = 4;  // (R, T): 0 (8, 1), 1 (16, 1), 2 (16, 2), 3 (16, 4)

template <int MT>
void launch_wide(int variant, const bf16_t* x, const bf16_t* w, const float* bias, bf16_t* out, int M, int N, int K,
                 int act, hipStream_t st) {
#define WIDE(R, T)                                                                                              \
  hipLaunchKernelGGL((dense_wide_kernel<R, T, MT>), dim3(cdiv(N, R * T)), dim3(256), 0, st, x, w, bias, out, M, \
                     N, K, act)
  switch (variant) {
    case 0: WIDE(8, 1); break;
    case 1: WIDE(16, 1); break;
    case 2: WIDE(16, 2); break;
    default: WIDE(16, 4); break;
  }
#undef WIDE
}

// Rows per block from N and the number of x tiles, read off profiles/generate_decode.txt section 7 (GPT-2-medium
// shapes at M = 17, 32, 48, 64): N = 1024 is fastest on (8, 1) at K = 1024 and K = 4096 (128 blocks; (16, 1) is 4 to 16%
// behind), N = 3072 and 4096 on (16, 1) for every M, N = 50304 on (16, 2) at M = 17 and on (16, 4) from M = 32 on
// (by 4% at M = 32, which shares MT = 2 with M = 17 and stays on (16, 2); by 6 to 9% at M = 48 and 64).
// The thresholds between the measured N (2048, 16384) and MT = 1 are not measured.
int wide_variant(int N, int MT) {
  if (N >= 16384) return MT >= 3 ? 3 : 2;
  if (N >= 2048) return 1;
  return 0;
}

bool wide_args_ok(const void* x, const void* w, const void* out, int M, int N, int K, int act) {
  if (!x || !w || !out || M < 1 || M > 64 || N < 8 || K < 8 || (N & 7) || (K & 7) || act < 0 || act > 2) return false;
  return aligned16(x) && aligned16(w) && !((uintptr_t)out & 1);
}

}  // namespace

// variant: one of the WIDE_VARIANTS (R, T) above, or -1 for the measured choice (what dtf_dense_wide runs); the other
// values exist for tools/bench_generate.py, which times every variant. -1 on anything the kernel cannot run; no
// allocation, no synchronisation, no device value read on the host.
DTF_API int dtf_dense_wide_variant(const void* x, const void* w, const float* bias, void* out, int M, int N, int K,
                                   int act, int variant, void* stream) {
  if (!wide_args_ok(x, w, out, M, N, K, act) || variant < -1 || variant >= WIDE_VARIANTS) return -1;
  const int MT = cdiv(M, 16);
  if (variant < 0) variant = wide_variant(N, MT);
  const bf16_t *xb = (const bf16_t*)x, *wb = (const bf16_t*)w;
  bf16_t* ob = (bf16_t*)out;
  hipStream_t st = (hipStream_t)stream;
  switch (MT) {
    case 1: launch_wide<1>(variant, xb, wb, bias, ob, M, N, K, act, st); break;
    case 2: launch_wide<2>(variant, xb, wb, bias, ob, M, N, K, act, st); break;
    case 3: launch_wide<3>(variant, xb, wb, bias, ob, M, N, K, act, st); break;
    default: launch_wide<4>(variant, xb, wb, bias, ob, M, N, K, act, st); break;
  }
  count_launch(LC_DENSE_WIDE);
  return (int)hipGetLastError();
}

DTF_API int dtf_dense_wide(const void* x, const void* w, const float* bias, void* out, int M, int N, int K, int act,
                           void* stream) {
  return dtf_dense_wide_variant(x, w, bias, out, M, N, K, act, -1, stream);
}
