// What the kernel files call in each other, declared once: every file that defines one of these includes this header
// and so does every file that calls one, so a parameter list that drifts is a compile error at the definition (a
// conflicting extern "C" declaration, or an ambiguous call / undefined symbol of our own that _build.py refuses).
#pragma once
#include <cstdlib>

#include "common.h"

// ---- shared C entry points
// Deterministic two-level reduction of `nrows` f32 rows (stride `stride`) into out (+= when accumulate); the rows are
// used as scratch. gemm.hip
DTF_API void dtf_sum_rows(float* rows, long stride, int nrows, long W, float* out, int accumulate, void* stream);
// One launch: sum groups of rows into <= target leader rows; returns their count, *out_stride their stride. gemm.hip
DTF_API int dtf_group_rows_once(float* rows, long stride, int nrows, long W, int target, long* out_stride,
                                void* stream);
// BatchNorm statistics from T partial rows [sum | sum of squares][C]. norm.hip
DTF_API int dtf_bn_finalize(float* part, int T, const float* gamma, const float* beta, float* running_mean,
                            float* running_var, long M, int C, float momentum, float eps, float* scale,
                            float* shift, float* mean_out, float* invstd_out, void* stream);
// The space-to-depth ResNet stem forward; -1 when the shape is not its own. stem.hip
DTF_API int dtf_stem_fwd(const void* X, const void* Wt, void* Y, float* part, int* rows, int N, int Hs, int Ws, int C,
                         int K, int R, int S, int P, int Q, void* stream);

// Host-side launch counters: which GEMM kernel a call reached (read by the tests through dtf_launch_counts, so a
// test named for a kernel fails when a dispatch change routes its call elsewhere). Incremented at launch sites on
// the host only; no device code touches them.
enum LaunchCounter : int {
  LC_W4_256 = 0,      // gemm_w4.hip, 256x256 tiles
  LC_W4_128 = 1,      // gemm_w4.hip, 256x128 tiles
  LC_GEMM256 = 2,     // gemm256.hip (8-wave)
  LC_GEMM_TILE = 3,   // gemm_core.h gemm_kernel (128/64-row tiles)
  LC_GEMM_DACT = 4,   // dtf_gemm_dact (activation backward in the data-gradient epilogue)
  LC_BETA_BF16 = 5,   // bf16 GEMM accumulating into C (beta != 0)
  LC_SPLITK = 6,      // split-K GEMM (f32 slabs + ordered reduction)
  LC_W4F8_256 = 7,    // gemm_w4_fp8.hip, 256x256 tiles
  LC_W4F8_128 = 8,    // gemm_w4_fp8.hip, 256x128 tiles
  LC_GEMM256_FP8 = 9, // gemm256.hip with fp8 operands
  LC_ATTN_DECODE = 10,  // attn_decode.hip, split-KV single-token attention (partials + merge count as one)
  LC_DENSE_SKINNY = 11, // attn_decode.hip, M <= 16 weight-streaming dense
  LC_SAMPLE = 12,       // sample.hip, the fused token sampler
  LC_ATTN_APPEND = 13,  // attention.hip, multi-token append attention over a KV cache
  LC_COUNT = 16
};
DTF_API long* dtf_launch_counters();  // gemm.hip
inline void count_launch(int c) { dtf_launch_counters()[c]++; }

// ---- kernel routes: each launches and returns its "taken" code, or launches nothing (see the definitions)
namespace dtf {
struct GemmArgs;
int gemm256_try(GemmArgs& a, int amode, int bmode, hipStream_t st, int fp8 = 0, int bn = 256);  // gemm256.hip
int gemm_w4_try(GemmArgs& a, int amode, int bmode, hipStream_t st, int bn);                     // gemm_w4.hip
int gemm_w4_fp8_try(GemmArgs& a, int fp8, hipStream_t st, int bn);                              // gemm_w4_fp8.hip
int conv256_try(GemmArgs& a, int amode, int bmode, int cfg, hipStream_t st, bool force);        // conv256.hip
bool conv256_on();                                                                               // conv256.hip
int pwconv_try(const void* X, const void* W, void* Y, float* stats, long M, int C, int K, hipStream_t st);  // pwconv.hip
int pwconv_dgrad_try(const void* dY, const void* Wck, void* dX, float beta, const void* betamask, const void* bnx,
                     const void* bnmask, const float* bnmean, float* part, long M, int Kc, int N, const void* bsrc2,
                     int H, int W, hipStream_t st, const void* bnrx, const void* bnrw);  // pwconv.hip
int pw_wgrad_try(const void* X, const void* dY, float* dW, long P, int C, int K, int accumulate, float* ws,
                 long ws_elems, hipStream_t st, bool split_out);  // pwwgrad.hip
int c3_wgrad_try(const void* X, const void* dY, float* dW, int N, int H, int W, int accumulate, float* ws,
                 long ws_elems, hipStream_t st);  // c3wgrad.hip

// A/B switch of a route: an environment variable read on first use, or set by a dtf_set_* entry point. level: the value
// is an integer (atoi; unset: dflt); else on / off, off only when the value begins with '0' (unset: dflt).
struct RouteSwitch {
  const char* env;
  int dflt;
  bool level;
  int v = -1;  // < 0: not read yet
  int get() {
    if (v < 0) {
      const char* e = getenv(env);
      v = level ? (e ? atoi(e) : dflt) : (e ? e[0] != '0' : dflt != 0);
    }
    return v;
  }
  bool on() { return get() != 0; }
  int set(int x) {
    v = level ? x : (x ? 1 : 0);
    return 0;
  }
};
}  // namespace dtf
