// What csrc/ssim.hip (SSIM and multi-scale SSIM forward) and csrc/ssim_grad.hip (their gradients) both need, once: the tile geometry,
// the argument and envelope predicates of the four entries, the pyramid layout, the window fill of the args structs and the clamp.
// No kernels here.
#pragma once
#include "common.h"

#define SS_TH 16             // tile: window positions (forward), pixels (backward)
#define SS_TW 32
#define SS_THREADS 256
#define SS_MAX_K 31          // forward taps per axis
#define SS_MAX_KG 15         // backward taps per axis
#define SS_MAX_S 8           // scales
#define SS_PARTS 256         // workgroups of the range pass at most
#define SS_HEAD 4            // state: sum, count, two unused words, then 4 x SS_PARTS doubles of range partials

// the stagings map a lane to a staged column
static_assert(SS_TW + 2 * (SS_MAX_KG - 1) <= 64 && SS_TW + SS_MAX_K - 1 <= 64, "one lane per staged column");
static_assert(SS_TH % 2 == 0 && SS_TW % 2 == 0, "a pooling cell has one owner");

// forward: tiles of window positions; backward: tiles of pixels
static inline int64_t ssim_tiles(int H, int W, int kh, int kw) { return (int64_t)cdiv(H - kh + 1, SS_TH) * cdiv(W - kw + 1, SS_TW); }
static inline int64_t ssim_grad_tiles(int H, int W) { return (int64_t)cdiv(H, SS_TH) * cdiv(W, SS_TW); }

// S scales: the coarsest must still hold a window (a scale count past the envelope is the envelope's refusal, not this one's)
static inline bool ssim_args_ok(int B, int C, int H, int W, int kh, int kw, int S = 1) {
    return B > 0 && C > 0 && kh > 0 && kw > 0 && (kh & 1) && (kw & 1) && S >= 1 &&
           (S > SS_MAX_S || ((H >> (S - 1)) >= kh && (W >> (S - 1)) >= kw));
}

// the envelopes: taps per axis, plane and grid sizes below 2^31
static inline bool ssim_sizes_ok(int H, int W, int kh, int kw, int max_k, int64_t blocks) {
    return kh <= max_k && kw <= max_k && (int64_t)H * W < ((int64_t)1 << 31) && blocks < ((int64_t)1 << 31);
}
static inline bool ssim_supported(int B, int C, int H, int W, int kh, int kw) {
    return ssim_sizes_ok(H, W, kh, kw, SS_MAX_K, (int64_t)B * C * ssim_tiles(H, W, kh, kw));
}
static inline bool ssim_grad_supported(int B, int C, int H, int W, int kh, int kw) {
    return ssim_sizes_ok(H, W, kh, kw, SS_MAX_KG, (int64_t)B * C * ssim_grad_tiles(H, W));
}
// max_k: SS_MAX_K forward, SS_MAX_KG backward; either way both grids must fit (a loss runs both)
static inline bool ms_ssim_supported(int B, int C, int H, int W, int kh, int kw, int S, int max_k) {
    return S <= SS_MAX_S && ssim_sizes_ok(H, W, kh, kw, max_k, (int64_t)B * C * ssim_tiles(H, W, kh, kw)) &&
           (int64_t)B * C * ssim_grad_tiles(H, W) < ((int64_t)1 << 31);
}

// elements of scale s of a [B][C][H][W] tensor, and of one image's pyramid: scales 1 .. S - 1
static inline int64_t ssim_scale_elems(int B, int C, int H, int W, int s) { return (int64_t)B * C * (H >> s) * (W >> s); }
static inline int64_t ssim_pyramid_elems(int B, int C, int H, int W, int S) {
    int64_t n = 0;
    for (int s = 1; s < S; ++s) n += ssim_scale_elems(B, C, H, W, s);
    return n;
}

// the window of an args struct: fp32 taps, zero past the window
template <int N>
static inline void ssim_fill_window(float (&wh)[N], float (&ww)[N], const double* h, const double* w, int kh, int kw) {
    for (int i = 0; i < N; ++i) wh[i] = i < kh ? (float)h[i] : 0.f, ww[i] = i < kw ? (float)w[i] : 0.f;
}

template <typename TIN>
__device__ __forceinline__ TIN ssim_clamp(TIN v, TIN lo, TIN hi) {   // a NaN stays a NaN
    return v < lo ? lo : (v > hi ? hi : v);
}
