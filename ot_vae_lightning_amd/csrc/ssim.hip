// StructuralSimilarityIndexMeasure on the device (the package's metrics/ssim.py; formula and state layout: include/otvae.h,
// otvae_ssim_accum).  Each image pair is read from memory once; everything is reduced in a fixed order (no float atomics, no host
// read): results are run-to-run identical and every entry can be captured into a hipGraph.
//
//   ss_range_kernel (range_mode 2 only)  up to SS_PARTS workgroups stride over both tensors and leave their minima / maxima in the
//                                        state's scratch; the tile kernel's workgroups fold them themselves (min / max are exact,
//                                        so every workgroup arrives at the same R).
//   ss_tile_kernel                       one workgroup per (image, channel, SS_TH x SS_TW tile of window positions):
//     * the p and t tile with its k - 1 halo goes to LDS once, as fp32 DIFFERENCES from the tile's first pixel (the subtraction is
//       done in the input's precision; clamping, range_mode 1, before it).  Variance and covariance are shift-invariant, so the
//       second moments of the differences are those of the pixels, without the cancellation of E[x^2] - mu^2 on narrow-range images;
//     * horizontal pass: the five row sums (p, t, p p, t t, p t) of every staged row, kw taps each, into LDS; vertical pass: kh taps
//       per quantity -- kh + kw FMAs per quantity and position instead of kh kw.  The default 11 x 11 window is a compile-time
//       instantiation (four neighbouring row sums per thread from 14 pixels in registers, then two positions from 12 rows of row
//       sums); every other window runs the same passes with run-time loops, one position per thread;
//     * the map is evaluated in fp64 from the five fp32 moments (the pivots go back into mu there), summed per thread, per wave
//       (xor tree) and over the four waves: one double per workgroup into the workspace.
//     Rows and columns past the image are never staged and never read: positions outside the map are skipped, not masked.
//   ss_fold_kernel                       one workgroup: image b's C * tiles partials are summed by G lanes (G from C * tiles alone) in
//                                        a fixed order -> ssim_b; state[0] += sum_b ssim_b, state[1] += B.
// The tile and partial layout depend on C, H, W, kh, kw only: ssim_b has the same bits whatever B is and wherever b sits in the batch.
// LDS per workgroup: 128 + 4 (2 SR SC + 5 SR 32) bytes with SR = 15 + kh, SC = 31 + kw: 25.5 KiB for the 11 x 11 window (6 workgroups
// per CU), 51.2 KiB at 31 x 31 (3 per CU).
#include "common.h"

#define SS_TH 16
#define SS_TW 32
#define SS_MAX_K 31
#define SS_THREADS 256
#define SS_PARTS 256         // workgroups of the range pass at most
#define SS_HEAD 4            // state: sum, count, two unused words, then 4 x SS_PARTS doubles of range partials

extern "C" int otvae_ssim_state_words(void) { return SS_HEAD + 4 * SS_PARTS; }

static int64_t ss_tiles(int H, int W, int kh, int kw) { return (int64_t)cdiv(H - kh + 1, SS_TH) * cdiv(W - kw + 1, SS_TW); }
static bool ss_args_ok(int B, int C, int H, int W, int kh, int kw) {
    return B > 0 && C > 0 && kh > 0 && kw > 0 && (kh & 1) && (kw & 1) && H >= kh && W >= kw;
}
static bool ss_supported(int B, int C, int H, int W, int kh, int kw) {
    return kh <= SS_MAX_K && kw <= SS_MAX_K && (int64_t)H * W < ((int64_t)1 << 31) &&
           (int64_t)B * C * ss_tiles(H, W, kh, kw) < ((int64_t)1 << 31);
}

extern "C" int64_t otvae_ssim_ws(int B, int C, int H, int W, int kh, int kw) {
    if (!ss_args_ok(B, C, H, W, kh, kw) || !ss_supported(B, C, H, W, kh, kw)) return -1;
    return (int64_t)B * C * ss_tiles(H, W, kh, kw) * (int64_t)sizeof(double);
}

// min / max that keep a NaN once they have met one (torch's amin / amax do)
__device__ __forceinline__ double ss_min(double a, double b) { return (b < a || b != b) ? b : a; }
__device__ __forceinline__ double ss_max(double a, double b) { return (b > a || b != b) ? b : a; }

// v = {min p, max p, min t, max t} over the block; red: 16 doubles of LDS.  Ends with every thread holding the result.
__device__ __forceinline__ void ss_block_minmax(double (&v)[4], double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        v[0] = ss_min(v[0], __shfl_xor(v[0], o, 64));
        v[1] = ss_max(v[1], __shfl_xor(v[1], o, 64));
        v[2] = ss_min(v[2], __shfl_xor(v[2], o, 64));
        v[3] = ss_max(v[3], __shfl_xor(v[3], o, 64));
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) red[q * 4 + w] = v[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double a = red[q * 4], b = red[q * 4 + 1], c = red[q * 4 + 2], d = red[q * 4 + 3];
        v[q] = (q & 1) ? ss_max(ss_max(a, b), ss_max(c, d)) : ss_min(ss_min(a, b), ss_min(c, d));
    }
    __syncthreads();
}

// range[q * SS_PARTS + block], q = min p, max p, min t, max t
template <typename TIN>
__global__ __launch_bounds__(SS_THREADS) void ss_range_kernel(const TIN* __restrict__ p, const TIN* __restrict__ t, int64_t numel,
                                                              double* __restrict__ range) {
    __shared__ double red[16];
    double v[4] = {INFINITY, -INFINITY, INFINITY, -INFINITY};
    for (int64_t e = (int64_t)blockIdx.x * SS_THREADS + threadIdx.x; e < numel; e += (int64_t)gridDim.x * SS_THREADS) {
        const double pv = (double)p[e], tv = (double)t[e];
        v[0] = ss_min(v[0], pv);
        v[1] = ss_max(v[1], pv);
        v[2] = ss_min(v[2], tv);
        v[3] = ss_max(v[3], tv);
    }
    ss_block_minmax(v, red);
    if (threadIdx.x < 4) range[threadIdx.x * SS_PARTS + blockIdx.x] = v[threadIdx.x];
}

struct SsimArgs {
    const void* p;
    const void* t;
    int C, H, W, kh, kw;
    int Ho, Wo, ntx, tiles;
    int mode, parts;
    double lo, hi, k1, k2;
    const double* range;   // mode 2: the range pass's partials
    double* ws;
    float wh[SS_MAX_K], ww[SS_MAX_K];
};

static size_t ss_lds_bytes(int kh, int kw) {
    const size_t SR = SS_TH + kh - 1, SC = SS_TW + kw - 1;
    return 16 * sizeof(double) + (2 * SR * SC + 5 * SR * SS_TW) * sizeof(float);
}

template <typename TIN>
__device__ __forceinline__ TIN ss_clamp(TIN v, TIN lo, TIN hi) {   // a NaN stays a NaN
    return v < lo ? lo : (v > hi ? hi : v);
}

// one position of the map in fp64 from the five fp32 moments of the differences; the pivots go back into the means here
__device__ __forceinline__ double ss_map(const float (&m)[5], double piv_p, double piv_t, double c1, double c2) {
    const double dp = (double)m[0], dt = (double)m[1];
    const double spp = (double)m[2] - dp * dp, stt = (double)m[3] - dt * dt, spt = (double)m[4] - dp * dt;
    const double mp = dp + piv_p, mt = dt + piv_t;
    const double num = (2.0 * mp * mt + c1) * (2.0 * spt + c2);
    const double den = (mp * mp + mt * mt + c1) * (spp + stt + c2);
    return num / den;
}

// K > 0: a K x K window known at compile time (the default 11 x 11): both passes are unrolled and register-blocked, weights in
// SGPRs.  K == 0: window sizes from the arguments, one position per thread and pass.
template <typename TIN, int K>
__global__ __launch_bounds__(SS_THREADS) void ss_tile_kernel(const SsimArgs a) {
    extern __shared__ __attribute__((aligned(16))) char ss_smem[];
    double* red = reinterpret_cast<double*>(ss_smem);   // 16 doubles
    const int kh = K ? K : a.kh, kw = K ? K : a.kw;
    const int SR = SS_TH + kh - 1, SC = SS_TW + kw - 1;
    float* sp = reinterpret_cast<float*>(ss_smem + 16 * sizeof(double));   // [SR][SC] p - pivot
    float* st = sp + SR * SC;                                              // [SR][SC] t - pivot
    float* hq = st + SR * SC;                                              // [5][SR][SS_TW] row sums
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    const unsigned plane = blockIdx.x / (unsigned)a.tiles, tile = blockIdx.x % (unsigned)a.tiles;
    const int r0 = (int)(tile / (unsigned)a.ntx) * SS_TH, c0 = (int)(tile % (unsigned)a.ntx) * SS_TW;
    const int nvr = min(SS_TH, a.Ho - r0), nvc = min(SS_TW, a.Wo - c0);   // positions of this tile, >= 1 each
    const int rows = nvr + kh - 1, cols = nvc + kw - 1;                    // staged pixels: r0 + rows <= H, c0 + cols <= W

    double R = a.hi - a.lo;
    if (a.mode == 2) {
        double v[4] = {INFINITY, -INFINITY, INFINITY, -INFINITY};
        if (tid < a.parts) {
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = a.range[q * SS_PARTS + tid];
        }
        ss_block_minmax(v, red);
        R = ss_max(v[1] - v[0], v[3] - v[2]);
    }
    const double c1 = (a.k1 * R) * (a.k1 * R), c2 = (a.k2 * R) * (a.k2 * R);

    const TIN* __restrict__ pp = static_cast<const TIN*>(a.p) + (size_t)plane * a.H * a.W + (size_t)r0 * a.W + c0;
    const TIN* __restrict__ tt = static_cast<const TIN*>(a.t) + (size_t)plane * a.H * a.W + (size_t)r0 * a.W + c0;
    const bool clamp = a.mode == 1;
    const TIN lo = (TIN)a.lo, hi = (TIN)a.hi;
    TIN piv_p = pp[0], piv_t = tt[0];
    if (clamp) piv_p = ss_clamp(piv_p, lo, hi), piv_t = ss_clamp(piv_t, lo, hi);

    // stage: wave w takes rows w, w + 4, ...; lane = column (SC <= 62).  All of a thread's loads (and the pivots') are issued
    // before the first is used: one trip to memory per workgroup, not one per row.  Threads past the tile load its last row /
    // column again (an address inside the image, no branch around the load) and store nothing.
    constexpr int NST = (SS_TH + (K ? K : SS_MAX_K) - 1 + 3) / 4;
    TIN xs[NST], ys[NST];
    const int lane_c = min(lane, cols - 1);
#pragma unroll
    for (int u = 0; u < NST; ++u) {
        const size_t at = (size_t)min(wave + 4 * u, rows - 1) * a.W + lane_c;
        xs[u] = pp[at];
        ys[u] = tt[at];
    }
#pragma unroll
    for (int u = 0; u < NST; ++u) {
        const int r = wave + 4 * u;
        if (lane < cols && r < rows) {
            TIN x = xs[u], y = ys[u];
            if (clamp) x = ss_clamp(x, lo, hi), y = ss_clamp(y, lo, hi);
            sp[r * SC + lane] = (float)(x - piv_p);
            st[r * SC + lane] = (float)(y - piv_t);
        }
    }
    __syncthreads();

    const int col = tid & (SS_TW - 1);
    double acc = 0.0;
    if constexpr (K > 0) {
        // horizontal pass: thread -> (staged row, four neighbouring positions).  The 4 + K - 1 pixels of both images and their three
        // products are formed once and serve all four positions.  A group that reaches past the tile's positions reads LDS that
        // was not staged (inside the row's SC slots); what it makes of it lands in columns >= nvc, which nobody reads.
        constexpr int NO = 4, NP = NO + K - 1;
        static_assert(SS_TW % NO == 0 && (2 * (SS_TH + K - 1) * (SS_TW + K - 1)) % 4 == 0, "16-byte stores of the row sums");
        float wgt[K];
#pragma unroll
        for (int j = 0; j < K; ++j) wgt[j] = a.ww[j];
        const int c4 = (tid & (SS_TW / NO - 1)) * NO;
        if (c4 < nvc) {
            for (int r = tid / (SS_TW / NO); r < rows; r += SS_THREADS / (SS_TW / NO)) {
                const float* __restrict__ xa = sp + r * SC + c4;
                const float* __restrict__ ya = st + r * SC + c4;
                float x[NP], y[NP], xx[NP], yy[NP], xy[NP];
#pragma unroll
                for (int i = 0; i < NP; ++i) {
                    x[i] = xa[i];
                    y[i] = ya[i];
                    xx[i] = x[i] * x[i];
                    yy[i] = y[i] * y[i];
                    xy[i] = x[i] * y[i];
                }
                f32x4 s[5];
#pragma unroll
                for (int o = 0; o < NO; ++o) {
                    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
#pragma unroll
                    for (int j = 0; j < K; ++j) {
                        s0 = fmaf(wgt[j], x[o + j], s0);
                        s1 = fmaf(wgt[j], y[o + j], s1);
                        s2 = fmaf(wgt[j], xx[o + j], s2);
                        s3 = fmaf(wgt[j], yy[o + j], s3);
                        s4 = fmaf(wgt[j], xy[o + j], s4);
                    }
                    s[0][o] = s0, s[1][o] = s1, s[2][o] = s2, s[3][o] = s3, s[4][o] = s4;
                }
#pragma unroll
                for (int q = 0; q < 5; ++q) *reinterpret_cast<f32x4*>(hq + (q * SR + r) * SS_TW + c4) = s[q];
            }
        }
        __syncthreads();

        // vertical pass and the map: thread -> positions (2 (tid / 32), col) and the one below it, from K + 1 rows of row sums.  The
        // lower position may lie past the tile (then its last row was never written): it is computed and dropped.
#pragma unroll
        for (int j = 0; j < K; ++j) wgt[j] = a.wh[j];
        const int o0 = 2 * (tid >> 5);
        if (col < nvc && o0 < nvr) {
            const float* __restrict__ h = hq + o0 * SS_TW + col;
            float m0[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, m1[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i <= K; ++i) {
#pragma unroll
                for (int q = 0; q < 5; ++q) {
                    const float v = h[(q * SR + i) * SS_TW];
                    if (i < K) m0[q] = fmaf(wgt[i], v, m0[q]);
                    if (i > 0) m1[q] = fmaf(wgt[i - 1], v, m1[q]);
                }
            }
            acc = ss_map(m0, (double)piv_p, (double)piv_t, c1, c2);
            const double below = ss_map(m1, (double)piv_p, (double)piv_t, c1, c2);
            if (o0 + 1 < nvr) acc += below;
        }
    } else {
        // horizontal pass: thread -> (staged row, position column)
        if (col < nvc) {
            for (int r = tid >> 5; r < rows; r += SS_THREADS / SS_TW) {
                const float* __restrict__ xa = sp + r * SC + col;
                const float* __restrict__ ya = st + r * SC + col;
                float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
                for (int j = 0; j < kw; ++j) {
                    const float w = a.ww[j], x = xa[j], y = ya[j];
                    const float wx = w * x, wy = w * y;
                    s0 += wx;
                    s1 += wy;
                    s2 = fmaf(wx, x, s2);
                    s3 = fmaf(wy, y, s3);
                    s4 = fmaf(wx, y, s4);
                }
                float* h = hq + r * SS_TW + col;
                h[0] = s0;
                h[SR * SS_TW] = s1;
                h[2 * SR * SS_TW] = s2;
                h[3 * SR * SS_TW] = s3;
                h[4 * SR * SS_TW] = s4;
            }
        }
        __syncthreads();

        // vertical pass and the map: thread -> positions (tid / 32 + 8 u, col)
        if (col < nvc) {
            for (int orow = tid >> 5; orow < nvr; orow += SS_THREADS / SS_TW) {
                const float* __restrict__ h = hq + orow * SS_TW + col;
                float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
                for (int i = 0; i < kh; ++i) {
                    const float w = a.wh[i];
#pragma unroll
                    for (int q = 0; q < 5; ++q) m[q] = fmaf(w, h[(q * SR + i) * SS_TW], m[q]);
                }
                acc += ss_map(m, (double)piv_p, (double)piv_t, c1, c2);
            }
        }
    }
    acc = wave_sum(acc);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (tid == 0) a.ws[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// one workgroup.  G (a power of two <= 64, from P alone) lanes share an image: lane g sums partials g, g + G, ... and an xor tree
// joins them; a group's images are added to its running sum in batch order, the groups' sums in group order.
__global__ __launch_bounds__(SS_THREADS) void ss_fold_kernel(const double* __restrict__ ws, int B, int P, int G, double count,
                                                             double* __restrict__ per_image, double* __restrict__ state) {
    __shared__ double s[SS_THREADS];
    const int tid = threadIdx.x, g = tid & (G - 1), grp = tid / G, ngrp = SS_THREADS / G;
    double run = 0.0;
    for (int b0 = 0; b0 < B; b0 += 4 * ngrp) {   // four images per group and trip: their loads are in flight together
        double v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int b = b0 + u * ngrp + grp;
            v[u] = 0.0;
            if (P <= G) {
                if (b < B && g < P) v[u] = ws[(size_t)b * P + g];
            } else if (b < B) {
                const double* __restrict__ w = ws + (size_t)b * P;
                for (int i = g; i < P; i += G) v[u] += w[i];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int b = b0 + u * ngrp + grp;
            double t = v[u];
            for (int o = G >> 1; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
            if (b < B) {
                t /= count;
                run += t;
                if (g == 0 && per_image) per_image[b] = t;
            }
        }
    }
    s[tid] = run;
    __syncthreads();
    if (tid == 0) {
        double tot = 0.0;
        for (int i = 0; i < ngrp; ++i) tot += s[i * G];
        state[0] += tot;
        state[1] += (double)B;
    }
}

extern "C" int otvae_ssim_accum(int in_dtype, const void* preds, const void* target, int B, int C, int H, int W, int kh, int kw,
                                const double* wh, const double* ww, double k1, double k2, int range_mode, double range_lo,
                                double range_hi, double* per_image, double* state, void* ws, void* stream) {
    OTVAE_REQUIRE(preds && target && wh && ww && state && ws, "otvae_ssim_accum: null argument");
    OTVAE_REQUIRE(in_dtype == 0 || in_dtype == 1, "otvae_ssim_accum: in_dtype must be 0 (fp32) or 1 (fp64)");
    OTVAE_REQUIRE(ss_args_ok(B, C, H, W, kh, kw),
                  "otvae_ssim_accum: need B, C >= 1, odd windows and H >= kh, W >= kw (got B %d, C %d, %d x %d images, %d x %d window)", B, C,
                  H, W, kh, kw);
    OTVAE_REQUIRE(range_mode >= 0 && range_mode <= 2, "otvae_ssim_accum: range_mode must be 0, 1 or 2");
    OTVAE_REQUIRE(range_mode == 2 || range_hi > range_lo, "otvae_ssim_accum: range_hi must exceed range_lo");
    OTVAE_REQUIRE(k1 >= 0.0 && k2 >= 0.0, "otvae_ssim_accum: k1 and k2 must not be negative");
    if (!ss_supported(B, C, H, W, kh, kw)) {
        otvae_set_error("otvae_ssim_accum: a %d x %d window on %d x %d x %d x %d is beyond the envelope (%d taps per axis, 2^31 tiles)", kh,
                        kw, B, C, H, W, SS_MAX_K);
        return OTVAE_EUNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    SsimArgs a;
    a.p = preds, a.t = target;
    a.C = C, a.H = H, a.W = W, a.kh = kh, a.kw = kw;
    a.Ho = H - kh + 1, a.Wo = W - kw + 1;
    a.ntx = cdiv(a.Wo, SS_TW);
    a.tiles = (int)ss_tiles(H, W, kh, kw);
    a.mode = range_mode;
    a.lo = range_mode == 2 ? 0.0 : range_lo, a.hi = range_mode == 2 ? 0.0 : range_hi;
    a.k1 = k1, a.k2 = k2;
    a.range = state + SS_HEAD;
    a.ws = (double*)ws;
    for (int i = 0; i < SS_MAX_K; ++i) a.wh[i] = i < kh ? (float)wh[i] : 0.f, a.ww[i] = i < kw ? (float)ww[i] : 0.f;
    const int64_t numel = (int64_t)B * C * H * W;
    a.parts = imax(1, imin(SS_PARTS, cdiv(numel, SS_THREADS * 16)));
    if (range_mode == 2) {
        if (in_dtype == 0) ss_range_kernel<float><<<a.parts, SS_THREADS, 0, st>>>((const float*)preds, (const float*)target, numel, state + SS_HEAD);
        else ss_range_kernel<double><<<a.parts, SS_THREADS, 0, st>>>((const double*)preds, (const double*)target, numel, state + SS_HEAD);
    }
    const unsigned blocks = (unsigned)((int64_t)B * C * a.tiles);
    const size_t lds = ss_lds_bytes(kh, kw);
    const bool k11 = kh == 11 && kw == 11;   // the default window: the unrolled instantiation
    if (in_dtype == 0) {
        if (k11) ss_tile_kernel<float, 11><<<blocks, SS_THREADS, lds, st>>>(a);
        else ss_tile_kernel<float, 0><<<blocks, SS_THREADS, lds, st>>>(a);
    } else {
        if (k11) ss_tile_kernel<double, 11><<<blocks, SS_THREADS, lds, st>>>(a);
        else ss_tile_kernel<double, 0><<<blocks, SS_THREADS, lds, st>>>(a);
    }
    const int P = C * a.tiles;
    int G = 1;
    while (G < 64 && G < P) G <<= 1;
    ss_fold_kernel<<<1, SS_THREADS, 0, st>>>((const double*)ws, B, P, G, (double)C * a.Ho * a.Wo, per_image, state);
    OTVAE_CHECK_LAUNCH("otvae_ssim_accum");
    return OTVAE_OK;
}
