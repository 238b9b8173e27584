// The weight-streaming dense layer of a decode step with 65 to 256 rows (accepted from 1 row): dtf_dense_tall.
//
// out[M, N] = act(x[M, K] w[N, K]^T + bias), 1 <= M <= 256; x, w, out bf16 (row-major, dense), bias f32 or null, f32
// accumulation. This is form (b) of dense_wide.hip's header, built as a kernel of its own: at 2 * M FLOP per weight
// byte the problem is a small GEMM near the ridge, but one in which every weight byte still comes from HBM once.
//
// Design kept. A block of four waves owns BN = 64 * WF weight rows, BM = 16 * XT rows of x and one range of K-tiles
// (grid = N tiles x M tiles x K splits).
//   weights  wave w owns the WF 16-row fragments (w * WF + f) of the block's rows over all of the block's x tiles. A
//            lane's 16-byte global load (row = lane % 16, 8 k at (lane / 16) * 8 of a 32-wide k-step) is the first
//            operand of the 16x16x32 bf16 MFMA as it arrives: no LDS staging, every weight byte of the block's K range
//            is read exactly once. Two register sets alternate: the loads of K-tile t + 1 are issued before the MFMAs
//            of tile t. Pieces past K load a clamped address and are made zero just before their MFMA (not at the load,
//            which would wait for it).
//   x        a K-tile [BM][KT] of the block's x rows is staged global -> registers -> LDS (the global loads of tile
//            t + 1 are issued with the weight loads, before the MFMAs of tile t, and stored after them into the other
//            of two buffers: one barrier a tile). Rows at or past M and pieces past K load a clamped address and are
//            stored as zero. The row stride is KT + 8 elements, an odd number of 16-byte units, so the 16 rows that
//            the lanes of one k-group read fall on 16 different 16-byte bank groups. Each wave reads an x fragment
//            with one 16-byte LDS read per lane and feeds it to WF = 2 MFMAs (its two weight fragments); x tiles
//            wholly past M are skipped. The accumulators (WF * XT tiles of 4 f32, 128 registers at XT = 16) are left
//            to the compiler, which places them in the AGPR half of the register file.
//   split    K-tiles are dealt to `splits` blocks in contiguous ranges. With one split the block applies bias and act
//            and stores bf16 itself. Otherwise it stores its f32 partial tile to slab [split][M][N] and a second launch
//            (dense_tall_reduce_kernel) sums the slabs in split order, adds the bias, applies act and stores bf16. No
//            atomics, no ticket, nobody waits: the second launch was kept over the last-block ticket because the
//            scratch is a fresh allocation per call and a ticket needs memory that is zero before the first launch.
//   rule     splits = min(cdiv(512, tiles), budget * K / (4 * M), K-tiles): up to two blocks for each of the 256 CUs,
//            but slab bytes (8 * splits * M * N, written then read) at most `budget` times the weight bytes
//            (2 * N * K). Tile sizes, splits and grid depend on (M, N, K) alone, so two calls, and an eager call and
//            a captured replay, give the same bits.
// Summation order: the K-tiles of a split in order inside the MFMA accumulator, then the splits in order.
//
// Variants (BN x BM, KT, budget), dtf_dense_tall_variant: 0 128x128 KT 64 b1, 1 128x256 KT 32 b1, 2 128x64 KT 64 b1,
// 3..5 the same shapes with budget 2, 6..8 with budget 4. KT is 32 at 256 rows so that the two x buffers stay inside
// 64 KB of static LDS (2 * 256 * 80 B = 40 KB; at KT = 64: 2 * 128 * 144 B = 36 KB). All nine stay as variants for
// the benchmark; 128x128 and 128x256 lost to 128x64 at every measured shape and are not launched by default.
// Dropped: 64 weight rows a block (one fragment a wave: one MFMA per 1 KB LDS read, LDS-bound at 256 rows; with the
// waves 2 x 2 over rows and K it needs a cross-wave reduction of up to 32 KB), LDS-DMA staging of x (not measured:
// the register form already issues its loads a tile ahead, and DMA next to plain LDS reads makes hipcc drain the
// in-flight DMA), the 32x32x16 MFMA (the same bytes per MFMA as two 16-row fragments).
//
// Bytes for the GPT-2-medium projections (K -> N), budget 1. HBM: weight bytes 2NK, read once per M tile (re-reads of
// the same rows by the other M tiles come from L2 / MALL); x: bytes read from L2, 2 * M * K per N tile; slab: 8 *
// splits * M * N (0 at one split); MB = 1e6 bytes.
//   shape        M    variant   tiles x splits = blocks   HBM w   L2 w re-read   L2 x    slab
//   1024->3072  128   128x128    24 x 2 =  48              6.3      0             6.3     6.3
//   1024->3072  128   128x64     48 x 2 =  96              6.3      6.3           6.3     6.3
//   1024->3072  256   128x128    48 x 1 =  48              6.3      6.3          12.6     0
//   1024->3072  256   128x256    24 x 1 =  24              6.3      0            12.6     0
//   1024->3072  256   128x64     96 x 1 =  96              6.3     18.9          12.6     0
//   1024->1024  128   128x128     8 x 2 =  16              2.1      0             2.1     2.1
//   1024->1024  128   128x64     16 x 2 =  32              2.1      2.1           2.1     2.1
//   1024->1024  256   128x128    16 x 1 =  16              2.1      2.1           4.2     0
//   1024->1024  256   128x256     8 x 1 =   8              2.1      0             4.2     0
//   1024->1024  256   128x64     32 x 1 =  32              2.1      6.3           4.2     0
//   1024->4096  128   128x128    32 x 2 =  64              8.4      0             8.4     8.4
//   1024->4096  128   128x64     64 x 2 = 128              8.4      8.4           8.4     8.4
//   1024->4096  256   128x128    64 x 1 =  64              8.4      8.4          16.8     0
//   1024->4096  256   128x256    32 x 1 =  32              8.4      0            16.8     0
//   1024->4096  256   128x64    128 x 1 = 128              8.4     25.2          16.8     0
//   4096->1024  128   128x128     8 x 8 =  64              8.4      0             8.4     8.4
//   4096->1024  128   128x64     16 x 8 = 128              8.4      8.4           8.4     8.4
//   4096->1024  256   128x128    16 x 4 =  64              8.4      8.4          16.8     8.4
//   4096->1024  256   128x256     8 x 4 =  32              8.4      0            16.8     8.4
//   4096->1024  256   128x64     32 x 4 = 128              8.4     25.2          16.8     8.4
// At K = 1024 and 256 rows budget 1 allows no split at all: only tiling M brings blocks, at the price of the L2
// re-reads. The default (tall_variant below) is read off the measurement, not off this table: the kernel's time is
// set by the latency of a block's chain of K-tiles (10 to 18 us for 2 to 8 MB), not by these bytes, so more and
// shorter blocks win: 128x64 with budget 2 (twice the slab bytes of the rows above).
#include "attn_decode.h"

namespace {

template <int WF, int XT, int KT>
__global__ void __launch_bounds__(256) dense_tall_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
                                                         const float* __restrict__ bias, bf16_t* __restrict__ out,
                                                         float* __restrict__ slabs, int M, int N, int K, int act,
                                                         int tps) {
  constexpr int BM = 16 * XT, BN = 64 * WF;
  constexpr int KS = KT / 32;            // 32-wide k-steps (MFMAs per fragment pair) of a K-tile
  constexpr int PR = KT / 8;             // 16-byte pieces of a tile row
  constexpr int LD = KT + 8;             // row stride in LDS: an odd number of 16-byte units
  constexpr int XP = BM * PR / 256;      // pieces of x a thread stages per tile
  static_assert(BM * PR % 256 == 0 && (PR & (PR - 1)) == 0 && XT % (XT < 4 ? XT : 4) == 0, "x staging");
  static_assert(2 * BM * LD * 2 <= 64 << 10, "static LDS");
  __shared__ __attribute__((aligned(16))) bf16_t xs[2][BM * LD];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * BN + wave * WF * 16, m0 = blockIdx.y * BM;
  const int nkt = (K + KT - 1) / KT;
  const int kt0 = blockIdx.z * tps, kt1 = min(nkt, kt0 + tps);
  const int nxt = min(XT, (M - m0 + 15) >> 4);  // x tiles of this block with a row below M
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);

  const bf16_t* wp[WF];
#pragma unroll
  for (int f = 0; f < WF; ++f) {
    const int nrow = n0 + f * 16 + r;
    wp[f] = w + (long)(nrow < N ? nrow : N - 1) * K;
  }
  const bf16_t* xp[XP];
  bool xok[XP];
  int xc[XP], xo[XP];
#pragma unroll
  for (int i = 0; i < XP; ++i) {
    const int p = tid + 256 * i, row = p / PR;
    xc[i] = (p & (PR - 1)) * 8;
    xo[i] = row * LD + xc[i];
    xok[i] = m0 + row < M;
    xp[i] = x + (long)(xok[i] ? m0 + row : 0) * K;
  }
  v4f acc[WF][XT];
#pragma unroll
  for (int f = 0; f < WF; ++f)
#pragma unroll
    for (int t = 0; t < XT; ++t) acc[f][t] = (v4f){0.f, 0.f, 0.f, 0.f};

  struct WSet {
    uint4 a[WF][KS];
  };
  uint4 gx[XP];
  // Loads are unconditional and clamped (in bounds); a tile past the block's range is loaded and never used. x goes
  // first: vmcnt counts in order, so `store_x` waits for the x pieces alone and leaves the weights in flight. Zeros
  // come later, at `store_x` and `mma` (a select at the load would wait for it).
  auto load = [&](WSet& q, int kt) {
#pragma unroll
    for (int i = 0; i < XP; ++i) {
      const int k = kt * KT + xc[i];
      gx[i] = *reinterpret_cast<const uint4*>(xp[i] + (k < K ? k : K - 8));
    }
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int k = kt * KT + s * 32 + g * 8;
#pragma unroll
      for (int f = 0; f < WF; ++f) q.a[f][s] = *reinterpret_cast<const uint4*>(wp[f] + (k < K ? k : K - 8));
    }
  };
  auto store_x = [&](int buf, int kt) {
#pragma unroll
    for (int i = 0; i < XP; ++i) {
      if (!xok[i] || kt * KT + xc[i] >= K) gx[i] = zero;
      *reinterpret_cast<uint4*>(&xs[buf][xo[i]]) = gx[i];
    }
  };
  // x tiles go in chunks of CH: the chunk's LDS reads are issued together, then its WF * CH MFMAs. A chunk with no
  // row below M is skipped; the tiles past M inside a chunk that runs hold zeros.
  constexpr int CH = XT < 4 ? XT : 4;
  auto mma = [&](WSet& q, int buf, int kt) {
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      if (kt * KT + s * 32 + g * 8 >= K) {
#pragma unroll
        for (int f = 0; f < WF; ++f) q.a[f][s] = zero;
      }
#pragma unroll
      for (int c = 0; c < XT / CH; ++c)
        if (c * CH < nxt) {
          v8bf b[CH];
#pragma unroll
          for (int i = 0; i < CH; ++i)
            b[i] = *reinterpret_cast<const v8bf*>(&xs[buf][((c * CH + i) * 16 + r) * LD + s * 32 + g * 8]);
#pragma unroll
          for (int i = 0; i < CH; ++i)
#pragma unroll
            for (int f = 0; f < WF; ++f)
              acc[f][c * CH + i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, q.a[f][s]), b[i],
                                                                           acc[f][c * CH + i], 0, 0, 0);
        }
    }
  };

  // every condition below is the same for the whole block; one barrier a tile: it ends the writes of the next buffer
  // and the reads of the current one
  WSet q0, q1;
  if (kt0 < kt1) {
    load(q0, kt0);
    store_x(0, kt0);
    __syncthreads();
  }
  for (int kt = kt0; kt < kt1; kt += 2) {
    load(q1, kt + 1);
    mma(q0, 0, kt);
    store_x(1, kt + 1);
    __syncthreads();
    if (kt + 1 >= kt1) break;
    load(q0, kt + 2);
    mma(q1, 1, kt + 1);
    store_x(0, kt + 2);
    __syncthreads();
  }

  // accumulator layout: lane holds D[i = 4 * g + v][j = r] (i: weight row of the fragment, j: x row of the tile), so
  // its four values are four consecutive columns of one output row
#pragma unroll
  for (int f = 0; f < WF; ++f) {
    const int n = n0 + f * 16 + 4 * g;  // N % 8 == 0: n < N holds for n .. n + 3 together
#pragma unroll
    for (int t = 0; t < XT; ++t) {
      const int m = m0 + t * 16 + r;
      if (t >= nxt || m >= M || n >= N) continue;
      if (slabs) {
        *reinterpret_cast<v4f*>(slabs + ((long)blockIdx.z * M + m) * N + n) = acc[f][t];
        continue;
      }
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = acc[f][t][e] + (bias ? bias[n + e] : 0.f);
        if (act == 1) v[e] = fmaxf(v[e], 0.f);
        else if (act == 2) v[e] = skinny_gelu(v[e]);
      }
      *reinterpret_cast<uint2*>(out + (long)m * N + n) = make_uint2(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]));
    }
  }
}

// out = bf16(act(slab 0 + slab 1 + ... + bias)), four columns a thread
__global__ void __launch_bounds__(256) dense_tall_reduce_kernel(const float* __restrict__ slabs,
                                                                const float* __restrict__ bias,
                                                                bf16_t* __restrict__ out, long MN, int N, int splits,
                                                                int act) {
  const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= MN) return;
  v4f s = *reinterpret_cast<const v4f*>(slabs + i);
  for (int z = 1; z < splits; ++z) {
    const v4f p = *reinterpret_cast<const v4f*>(slabs + z * MN + i);
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] += p[e];
  }
  const int n = (int)(i % N);
  float v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    v[e] = s[e] + (bias ? bias[n + e] : 0.f);
    if (act == 1) v[e] = fmaxf(v[e], 0.f);
    else if (act == 2) v[e] = skinny_gelu(v[e]);
  }
  *reinterpret_cast<uint2*>(out + i) = make_uint2(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]));
}

constexpr int TALL_SHAPES = 3;                 // (BN, BM, KT): 0 (128, 128, 64), 1 (128, 256, 32), 2 (128, 64, 64)
constexpr int TALL_VARIANTS = 3 * TALL_SHAPES; // variant = shape + TALL_SHAPES * b, slab budget 1, 2, 4 (b = 0, 1, 2)
constexpr int TALL_BLOCKS = 512;               // blocks the split aims at: two a CU, so a CU has loads of two in flight

struct TallPlan {
  int nt, mt, splits, tps;
};

TallPlan tall_plan(int M, int N, int K, int variant) {
  const int shape = variant % TALL_SHAPES, budget = 1 << (variant / TALL_SHAPES);
  const int BM = shape == 0 ? 128 : shape == 1 ? 256 : 64, KT = shape == 1 ? 32 : 64;
  TallPlan p;
  p.nt = cdiv(N, 128);
  p.mt = cdiv(M, BM);
  const int nkt = cdiv(K, KT);
  int s = cdiv(TALL_BLOCKS, (long)p.nt * p.mt);
  s = min(s, budget * K / (4 * M));
  s = max(1, min(s, nkt));
  p.tps = cdiv(nkt, s);
  p.splits = cdiv(nkt, p.tps);  // no split without a K-tile
  return p;
}

// The default, read off profiles/generate_decode.txt section 10 (GPT-2-medium shapes at M = 65, 128, 192, 256): the
// 128 x 64 block is the fastest shape or within 4% of it for every layer projection and row count, so M is always
// tiled by 64 and the weight re-reads are left to L2. Budget 2 wins from M = 128 on (1024 -> 3072 at M = 256: 16.3 us
// against 21.8 with budget 1 and 18.3 with budget 4); at M = 65 budget 1 is ahead on the sum of the four projections
// (4096 -> 1024: 14.5 us against 18.1). The threshold between 65 and 128 rows is not measured.
int tall_variant(int M, int N, int K) {
  (void)N;
  (void)K;
  return M < 128 ? 2 : 2 + TALL_SHAPES;
}

bool tall_args_ok(const void* x, const void* w, const void* out, int M, int N, int K, int act) {
  if (!x || !w || !out || M < 1 || M > 256 || N < 8 || K < 8 || (N & 7) || (K & 7) || act < 0 || act > 2) return false;
  return aligned16(x) && aligned16(w) && aligned16(out);
}

}  // namespace

// f32 elements of scratch that dtf_dense_tall / dtf_dense_tall_variant may need for (M, N, K): the largest over the
// variants (0 where none splits K); -1 for a shape the kernel does not take.
DTF_API long dtf_dense_tall_slab_elems(int M, int N, int K) {
  if (M < 1 || M > 256 || N < 8 || K < 8 || (N & 7) || (K & 7)) return -1;
  long most = 0;
  for (int v = 0; v < TALL_VARIANTS; ++v) {
    const TallPlan p = tall_plan(M, N, K, v);
    if (p.splits > 1) most = max(most, (long)p.splits * M * N);
  }
  return most;
}

// variant: one of the TALL_VARIANTS above, or -1 for the measured choice (what dtf_dense_tall runs); the other values
// exist for tools/bench_generate.py, which times every variant. slabs: f32 scratch of slab_elems elements, at least
// what the variant's split needs (dtf_dense_tall_slab_elems covers every variant). -1 on anything the kernel cannot
// run, before any launch; no allocation, no synchronisation, no device value read on the host.
DTF_API int dtf_dense_tall_variant(const void* x, const void* w, const float* bias, void* out, float* slabs,
                                   long slab_elems, int M, int N, int K, int act, int variant, void* stream) {
  if (!tall_args_ok(x, w, out, M, N, K, act) || variant < -1 || variant >= TALL_VARIANTS) return -1;
  if (variant < 0) variant = tall_variant(M, N, K);
  const TallPlan p = tall_plan(M, N, K, variant);
  const long MN = (long)M * N;
  if (p.splits > 1 && (!slabs || !aligned16(slabs) || slab_elems < p.splits * MN)) return -1;
  const bf16_t *xb = (const bf16_t*)x, *wb = (const bf16_t*)w;
  bf16_t* ob = (bf16_t*)out;
  float* sl = p.splits > 1 ? slabs : nullptr;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(p.nt, p.mt, p.splits);
#define TALL(WF, XT, KT) \
  hipLaunchKernelGGL((dense_tall_kernel<WF, XT, KT>), grid, dim3(256), 0, st, xb, wb, bias, ob, sl, M, N, K, act, p.tps)
  switch (variant % TALL_SHAPES) {
    case 0: TALL(2, 8, 64); break;
    case 1: TALL(2, 16, 32); break;
    default: TALL(2, 4, 64); break;
  }
#undef TALL
  if (sl)
    hipLaunchKernelGGL(dense_tall_reduce_kernel, dim3(cdiv(MN, 1024)), dim3(256), 0, st, sl, bias, ob, MN, N, p.splits,
                       act);
  count_launch(LC_DENSE_TALL);
  return (int)hipGetLastError();
}

DTF_API int dtf_dense_tall(const void* x, const void* w, const float* bias, void* out, float* slabs, long slab_elems,
                           int M, int N, int K, int act, void* stream) {
  return dtf_dense_tall_variant(x, w, bias, out, slabs, slab_elems, M, N, K, act, -1, stream);
}
