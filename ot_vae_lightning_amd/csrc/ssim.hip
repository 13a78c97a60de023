// StructuralSimilarityIndexMeasure and its multi-scale form on the device (metrics/ssim.py, metrics/ms_ssim.py, the forwards of
// losses.py's SSIMLoss / MSSSIMLoss; formulas, state layouts and envelopes: include/otvae.h, otvae_ssim_accum / otvae_ms_ssim_accum).
// Each image pair is read from memory once; everything is reduced in a fixed order (no float atomics, no host read): results are
// run-to-run identical and every entry can be captured into a hipGraph.
//
//   ss_range_kernel (range_mode 2 only)  up to SS_PARTS workgroups stride over both tensors and leave their minima / maxima in the
//                                        state's scratch; the tile kernel's workgroups fold them themselves (min / max are exact,
//                                        so every workgroup arrives at the same R).  Multi-scale: in front of each scale's launch.
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
//   ms_tile_kernel   one launch per scale, the tiles, passes (the ss_* functions below, written once for both kernels) and LDS of
//                    ss_tile_kernel.  From the same five moments it evaluates cs = A2 / B2 and ssim = A1 A2 / (B1 B2) with ONE fp64
//                    division (r = 1 / (B1 B2); ssim = A1 A2 r, cs = A2 B1 r) and leaves two doubles per workgroup, {sum cs, sum ssim}.
//                    A wave stages row PAIRS (rows 2 w, 2 w + 1, 2 w + 8, 2 w + 9, ... of the tile), so a thread holds both rows of a
//                    2 x 2 pooling cell of its column in registers; the neighbouring column comes by one lane shift.  The workgroup
//                    writes the pooled pair of the next scale from the RAW (unclamped) pixels it owns, in the input's type: a tile owns
//                    its SS_TH x SS_TW pixels, the last tile row / column all pixels up to H / W (they are all staged there).  Tiles
//                    start at even coordinates, so no cell straddles two owners: every pooled element is written exactly once, and
//                    the scale's pair is read from memory once.
//   ms_fold_kernel   one workgroup, all scales: G <= 16 lanes (G from scale 0's partial count alone) share an image and sum each
//                    scale's partials in a fixed order -> v_s[b]; msssim_b = prod_s f(v_s)^beta_s and w_s[b] = d msssim_b / d v_s[b] in fp64;
//                    state[0] += sum_b msssim_b, state[1] += B.
// The two tile kernels differ where their results do: the staging order, the pooled store, the map (ss_map divides, ms_map multiplies
// by one reciprocal) and the p t row sum of the generic horizontal pass; the two folds differ in G, the order of summation and pow, so
// one-scale MS-SSIM keeps its own bits.
// The tile and partial layout depend on C, H, W, kh, kw only: ssim_b has the same bits whatever B is and wherever b sits in the batch.
// LDS per workgroup: 128 + 4 (2 SR SC + 5 SR 32) bytes with SR = 15 + kh, SC = 31 + kw: 25.5 KiB for the 11 x 11 window (6 workgroups
// per CU), 51.2 KiB at 31 x 31 (3 per CU).  Registers and occupancy: DESIGN.md.
#include "ssim_common.h"

extern "C" int otvae_ssim_state_words(void) { return SS_HEAD + 4 * SS_PARTS; }
extern "C" int otvae_ms_ssim_state_words(void) { return SS_HEAD + 4 * SS_PARTS; }

extern "C" int64_t otvae_ssim_ws(int B, int C, int H, int W, int kh, int kw) {
    if (!ssim_args_ok(B, C, H, W, kh, kw) || !ssim_supported(B, C, H, W, kh, kw)) return -1;
    return (int64_t)B * C * ssim_tiles(H, W, kh, kw) * (int64_t)sizeof(double);
}

extern "C" int64_t otvae_ms_ssim_pyramid(int in_dtype, int B, int C, int H, int W, int S) {
    if ((in_dtype != 0 && in_dtype != 1) || B <= 0 || C <= 0 || H <= 0 || W <= 0 || S < 1 || S > SS_MAX_S) return -1;
    return ssim_pyramid_elems(B, C, H, W, S) * (in_dtype == 0 ? 4 : 8);
}

extern "C" int64_t otvae_ms_ssim_ws(int B, int C, int H, int W, int kh, int kw, int S) {
    if (!ssim_args_ok(B, C, H, W, kh, kw, S) || !ms_ssim_supported(B, C, H, W, kh, kw, S, SS_MAX_K)) return -1;
    int64_t n = 0;
    for (int s = 0; s < S; ++s) n += 2 * (int64_t)B * C * ssim_tiles(H >> s, W >> s, kh, kw);
    return n * (int64_t)sizeof(double);
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
    int Ho, Wo, ntx, nty, tiles;
    int mode, parts;
    double lo, hi, k1, k2;
    const double* range;   // mode 2: the range pass's partials
    double* ws;            // per workgroup: one double (ss_tile_kernel), {sum cs, sum ssim} (ms_tile_kernel)
    float wh[SS_MAX_K], ww[SS_MAX_K];
};
struct MsArgs : SsimArgs {
    void* pool_p;          // the next scale's pair [planes][Hp][Wp]; NULL at the last scale
    void* pool_t;
    int Hp, Wp;
};

static size_t ss_lds_bytes(int kh, int kw) {
    const size_t SR = SS_TH + kh - 1, SC = SS_TW + kw - 1;
    return 16 * sizeof(double) + (2 * SR * SC + 5 * SR * SS_TW) * sizeof(float);
}

// ---- the pieces of a tile kernel that do not know which one they are in ---------------------------------------------------------------
// c1, c2 of the map: from the fixed range, or (mode 2) from the range pass's partials, folded by every workgroup for itself
__device__ __forceinline__ void ss_constants(const SsimArgs& a, double* red, double& c1, double& c2) {
    double R = a.hi - a.lo;
    if (a.mode == 2) {
        double v[4] = {INFINITY, -INFINITY, INFINITY, -INFINITY};
        const int tid = threadIdx.x;
        if (tid < a.parts) {
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = a.range[q * SS_PARTS + tid];
        }
        ss_block_minmax(v, red);
        R = ss_max(v[1] - v[0], v[3] - v[2]);
    }
    c1 = (a.k1 * R) * (a.k1 * R), c2 = (a.k2 * R) * (a.k2 * R);
}

// horizontal pass, K x K window known at compile time: thread -> (staged row, four neighbouring positions), weights in SGPRs.  The
// 4 + K - 1 pixels of both images and their three products are formed once and serve all four positions.  A group that reaches past
// the tile's positions reads LDS that was not staged (inside the row's SC slots); what it makes of it lands in columns >= nvc, which
// nobody reads.  sp, st: [SR][SC] staged differences; hq: [5][SR][SS_TW] row sums.
template <int K>
__device__ __forceinline__ void ss_hpass_fixed(const float* ww, const float* sp, const float* st, float* hq, int nvc, int rows) {
    constexpr int NO = 4, NP = NO + K - 1, SR = SS_TH + K - 1, SC = SS_TW + K - 1;
    static_assert(SS_TW % NO == 0 && (2 * SR * SC) % 4 == 0, "16-byte stores of the row sums");
    const int tid = threadIdx.x;
    float wgt[K];
#pragma unroll
    for (int j = 0; j < K; ++j) wgt[j] = ww[j];
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
}

// vertical pass, K taps known at compile time: the moments m0 of the position whose row sums start at h and m1 of the one below it,
// from K + 1 rows of row sums.  The lower position may lie past the tile (then its last row was never written): the caller drops it.
template <int K>
__device__ __forceinline__ void ss_vmoments_fixed(const float* wh, const float* __restrict__ h, float (&m0)[5], float (&m1)[5]) {
    constexpr int SR = SS_TH + K - 1;
    float wgt[K];
#pragma unroll
    for (int j = 0; j < K; ++j) wgt[j] = wh[j];
#pragma unroll
    for (int q = 0; q < 5; ++q) m0[q] = m1[q] = 0.f;
#pragma unroll
    for (int i = 0; i <= K; ++i) {
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const float v = h[(q * SR + i) * SS_TW];
            if (i < K) m0[q] = fmaf(wgt[i], v, m0[q]);
            if (i > 0) m1[q] = fmaf(wgt[i - 1], v, m1[q]);
        }
    }
}

// vertical pass, kh taps from the arguments: the moments of the position whose row sums start at h
__device__ __forceinline__ void ss_vmoments(const float* wh, int kh, const float* __restrict__ h, int SR, float (&m)[5]) {
#pragma unroll
    for (int q = 0; q < 5; ++q) m[q] = 0.f;
    for (int i = 0; i < kh; ++i) {
        const float w = wh[i];
#pragma unroll
        for (int q = 0; q < 5; ++q) m[q] = fmaf(w, h[(q * SR + i) * SS_TW], m[q]);
    }
}

// the workgroup's N sums: per wave (xor tree), then over the four waves; thread n < N writes out[n].  red: 4 N doubles of LDS.
template <int N>
__device__ __forceinline__ void ss_block_sums(double (&acc)[N], double* red, double* __restrict__ out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int n = 0; n < N; ++n) acc[n] = wave_sum(acc[n]);
    if (lane == 0) {
#pragma unroll
        for (int n = 0; n < N; ++n) red[4 * n + wave] = acc[n];
    }
    __syncthreads();
    if (tid < N) out[tid] = (red[4 * tid] + red[4 * tid + 1]) + (red[4 * tid + 2] + red[4 * tid + 3]);
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

// the same position for multi-scale SSIM: cs and ssim from one reciprocal, added to their running sums acc = {cs, ssim}
__device__ __forceinline__ void ms_map(const float (&m)[5], double piv_p, double piv_t, double c1, double c2, double& cs, double& ss) {
    const double dp = (double)m[0], dt = (double)m[1];
    const double spp = (double)m[2] - dp * dp, stt = (double)m[3] - dt * dt, spt = (double)m[4] - dp * dt;
    const double mp = dp + piv_p, mt = dt + piv_t;
    const double A1 = 2.0 * mp * mt + c1, A2 = 2.0 * spt + c2;
    const double B1 = mp * mp + mt * mt + c1, B2 = spp + stt + c2;
    const double r = 1.0 / (B1 * B2);
    ss += A1 * A2 * r;
    cs += A2 * B1 * r;
}

// K > 0: a K x K window known at compile time (the default 11 x 11): both passes are unrolled and register-blocked.  K == 0: window
// sizes from the arguments, one position per thread and pass.
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

    double c1, c2;
    ss_constants(a, red, c1, c2);

    const TIN* __restrict__ pp = static_cast<const TIN*>(a.p) + (size_t)plane * a.H * a.W + (size_t)r0 * a.W + c0;
    const TIN* __restrict__ tt = static_cast<const TIN*>(a.t) + (size_t)plane * a.H * a.W + (size_t)r0 * a.W + c0;
    const bool clamp = a.mode == 1;
    const TIN lo = (TIN)a.lo, hi = (TIN)a.hi;
    TIN piv_p = pp[0], piv_t = tt[0];
    if (clamp) piv_p = ssim_clamp(piv_p, lo, hi), piv_t = ssim_clamp(piv_t, lo, hi);

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
            if (clamp) x = ssim_clamp(x, lo, hi), y = ssim_clamp(y, lo, hi);
            sp[r * SC + lane] = (float)(x - piv_p);
            st[r * SC + lane] = (float)(y - piv_t);
        }
    }
    __syncthreads();

    const int col = tid & (SS_TW - 1);
    double acc[1] = {0.0};
    if constexpr (K > 0) {
        ss_hpass_fixed<K>(a.ww, sp, st, hq, nvc, rows);
        __syncthreads();
        // the map: thread -> positions (2 (tid / 32), col) and the one below it
        const int o0 = 2 * (tid >> 5);
        if (col < nvc && o0 < nvr) {
            float m0[5], m1[5];
            ss_vmoments_fixed<K>(a.wh, hq + o0 * SS_TW + col, m0, m1);
            acc[0] = ss_map(m0, (double)piv_p, (double)piv_t, c1, c2);
            const double below = ss_map(m1, (double)piv_p, (double)piv_t, c1, c2);
            if (o0 + 1 < nvr) acc[0] += below;
        }
    } else {
        // horizontal pass: thread -> (staged row, position column).  (Written out in both tile kernels: as a shared function it
        // costs ms_tile_kernel<.., 0> a wave of occupancy, 61 -> 68 and 71 -> 74 VGPRs, whatever its signature.)
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
        // the map: thread -> positions (tid / 32 + 8 u, col)
        if (col < nvc) {
            for (int orow = tid >> 5; orow < nvr; orow += SS_THREADS / SS_TW) {
                float m[5];
                ss_vmoments(a.wh, kh, hq + orow * SS_TW + col, SR, m);
                acc[0] += ss_map(m, (double)piv_p, (double)piv_t, c1, c2);
            }
        }
    }
    ss_block_sums(acc, red, a.ws + blockIdx.x);
}

// the multi-scale tile kernel: ss_tile_kernel with row-pair staging, the pooled store and ms_map
template <typename TIN, int K>
__global__ __launch_bounds__(SS_THREADS) void ms_tile_kernel(const MsArgs a) {
    extern __shared__ __attribute__((aligned(16))) char ms_smem[];
    double* red = reinterpret_cast<double*>(ms_smem);   // 16 doubles
    const int kh = K ? K : a.kh, kw = K ? K : a.kw;
    const int SR = SS_TH + kh - 1, SC = SS_TW + kw - 1;
    float* sp = reinterpret_cast<float*>(ms_smem + 16 * sizeof(double));   // [SR][SC] p - pivot
    float* st = sp + SR * SC;                                              // [SR][SC] t - pivot
    float* hq = st + SR * SC;                                              // [5][SR][SS_TW] row sums
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    const unsigned plane = blockIdx.x / (unsigned)a.tiles, tile = blockIdx.x % (unsigned)a.tiles;
    const int ty = (int)(tile / (unsigned)a.ntx), tx = (int)(tile % (unsigned)a.ntx);
    const int r0 = ty * SS_TH, c0 = tx * SS_TW;
    const int nvr = min(SS_TH, a.Ho - r0), nvc = min(SS_TW, a.Wo - c0);   // positions of this tile, >= 1 each
    const int rows = nvr + kh - 1, cols = nvc + kw - 1;                    // staged pixels: r0 + rows <= H, c0 + cols <= W

    double c1, c2;
    ss_constants(a, red, c1, c2);

    const TIN* __restrict__ pp = static_cast<const TIN*>(a.p) + (size_t)plane * a.H * a.W + (size_t)r0 * a.W + c0;
    const TIN* __restrict__ tt = static_cast<const TIN*>(a.t) + (size_t)plane * a.H * a.W + (size_t)r0 * a.W + c0;
    const bool clamp = a.mode == 1;
    const TIN lo = (TIN)a.lo, hi = (TIN)a.hi;
    TIN piv_p = pp[0], piv_t = tt[0];
    if (clamp) piv_p = ssim_clamp(piv_p, lo, hi), piv_t = ssim_clamp(piv_t, lo, hi);

    // stage: wave w takes the row pairs (2 w, 2 w + 1), (2 w + 8, 2 w + 9), ...; lane = column (SC <= 62).  All of a thread's loads
    // are issued before the first is used.  Threads past the tile load its last row / column again (an address inside the image, no
    // branch around the load) and store nothing.
    constexpr int NST = 2 * ((SS_TH + (K ? K : SS_MAX_K) - 1 + 7) / 8);
    TIN xs[NST], ys[NST];
    const int lane_c = min(lane, cols - 1);
#pragma unroll
    for (int u = 0; u < NST; ++u) {
        const size_t at = (size_t)min(8 * (u >> 1) + 2 * wave + (u & 1), rows - 1) * a.W + lane_c;
        xs[u] = pp[at];
        ys[u] = tt[at];
    }
#pragma unroll
    for (int u = 0; u < NST; ++u) {
        const int r = 8 * (u >> 1) + 2 * wave + (u & 1);
        if (lane < cols && r < rows) {
            TIN x = xs[u], y = ys[u];
            if (clamp) x = ssim_clamp(x, lo, hi), y = ssim_clamp(y, lo, hi);
            sp[r * SC + lane] = (float)(x - piv_p);
            st[r * SC + lane] = (float)(y - piv_t);
        }
    }
    // the next scale's pair from the raw pixels this tile owns: rows r, r + 1 are xs[u], xs[u + 1], column lane + 1 is one lane up.
    // A cell is written only if it lies inside the pooled image (pr < Hp, pc < Wp: then both of its rows and columns are inside this
    // tile's staged block) and its first pixel is owned here.
    if (a.pool_p) {   // (uniform over the launch)
        const int own_r = ty == a.nty - 1 ? rows : SS_TH, own_c = tx == a.ntx - 1 ? cols : SS_TW;
        TIN* __restrict__ qp = static_cast<TIN*>(a.pool_p) + (size_t)plane * a.Hp * a.Wp;
        TIN* __restrict__ qt = static_cast<TIN*>(a.pool_t) + (size_t)plane * a.Hp * a.Wp;
        const int pc = (c0 + lane) >> 1;
#pragma unroll
        for (int u = 0; u < NST; u += 2) {
            const int r = 8 * (u >> 1) + 2 * wave;
            TIN sx = xs[u] + xs[u + 1], sy = ys[u] + ys[u + 1];
            sx += __shfl_down(sx, 1, 64);
            sy += __shfl_down(sy, 1, 64);
            const int pr = (r0 + r) >> 1;
            if (!(lane & 1) && r < own_r && lane < own_c && pr < a.Hp && pc < a.Wp) {
                qp[(size_t)pr * a.Wp + pc] = sx * (TIN)0.25;
                qt[(size_t)pr * a.Wp + pc] = sy * (TIN)0.25;
            }
        }
    }
    __syncthreads();

    const int col = tid & (SS_TW - 1);
    double acc[2] = {0.0, 0.0};   // cs, ssim
    if constexpr (K > 0) {
        ss_hpass_fixed<K>(a.ww, sp, st, hq, nvc, rows);
        __syncthreads();
        // the map: thread -> positions (2 (tid / 32), col) and the one below it
        const int o0 = 2 * (tid >> 5);
        if (col < nvc && o0 < nvr) {
            float m0[5], m1[5];
            ss_vmoments_fixed<K>(a.wh, hq + o0 * SS_TW + col, m0, m1);
            ms_map(m0, (double)piv_p, (double)piv_t, c1, c2, acc[0], acc[1]);
            double below[2] = {0.0, 0.0};
            ms_map(m1, (double)piv_p, (double)piv_t, c1, c2, below[0], below[1]);
            if (o0 + 1 < nvr) acc[0] += below[0], acc[1] += below[1];
        }
    } else {
        // horizontal pass: thread -> (staged row, position column).  As ss_tile_kernel's but for the p t row sum.
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
                    s4 = fmaf(w, x * y, s4);   // (not wx * y: exchanging the two images must give the same bits)
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
        // the map: thread -> positions (tid / 32 + 8 u, col)
        if (col < nvc) {
            for (int orow = tid >> 5; orow < nvr; orow += SS_THREADS / SS_TW) {
                float m[5];
                ss_vmoments(a.wh, kh, hq + orow * SS_TW + col, SR, m);
                ms_map(m, (double)piv_p, (double)piv_t, c1, c2, acc[0], acc[1]);
            }
        }
    }
    ss_block_sums(acc, red, a.ws + 2 * (size_t)blockIdx.x);
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

struct MsFoldArgs {
    int S, B, G, normalize;      // normalize 0: none, 1: relu, 2: simple
    int P[SS_MAX_S];             // partial pairs per image at scale s
    long long off[SS_MAX_S];     // where scale s begins in the workspace, in doubles
    double count[SS_MAX_S], beta[SS_MAX_S];
};

#define MS_FOLD_U 4          // images per group and trip: their loads are in flight together

// one workgroup.  G (a power of two <= 16, from scale 0's P alone) lanes share an image: lane g sums partials g, g + G, ... of each
// scale (cs below the last scale, ssim at it) and an xor tree joins them; a group's images are added to its running sum in batch order,
// the groups' sums in group order.
__global__ __launch_bounds__(SS_THREADS) void ms_fold_kernel(const double* __restrict__ ws, const MsFoldArgs f,
                                                             double* __restrict__ per_image, double* __restrict__ wgt,
                                                             double* __restrict__ state) {
    __shared__ double sh[SS_THREADS];
    const int tid = threadIdx.x, G = f.G, g = tid & (G - 1), grp = tid / G, ngrp = SS_THREADS / G;
    double run = 0.0;
    for (int b0 = 0; b0 < f.B; b0 += MS_FOLD_U * ngrp) {
        double v[MS_FOLD_U][SS_MAX_S];
#pragma unroll
        for (int s = 0; s < SS_MAX_S; ++s) {
            if (s < f.S) {
                const int P = f.P[s];
                const double* __restrict__ w = ws + f.off[s] + (s == f.S - 1 ? 1 : 0);
                size_t at[MS_FOLD_U];
                double t[MS_FOLD_U];
#pragma unroll
                for (int u = 0; u < MS_FOLD_U; ++u) {   // an image past the batch reads the last one again and is dropped below
                    at[u] = 2 * (size_t)min(b0 + u * ngrp + grp, f.B - 1) * P;
                    t[u] = 0.0;
                }
                for (int i = g; i < P; i += G) {
#pragma unroll
                    for (int u = 0; u < MS_FOLD_U; ++u) t[u] += w[at[u] + 2 * (size_t)i];
                }
#pragma unroll
                for (int u = 0; u < MS_FOLD_U; ++u) {
                    for (int o = G >> 1; o > 0; o >>= 1) t[u] += __shfl_xor(t[u], o, 64);
                    v[u][s] = t[u] / f.count[s];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < MS_FOLD_U; ++u) {
            const int b = b0 + u * ngrp + grp;
            if (b < f.B) {
                double fv[SS_MAX_S], ms = 1.0;
#pragma unroll
                for (int s = 0; s < SS_MAX_S; ++s) {
                    if (s < f.S) {
                        fv[s] = f.normalize == 1 ? (v[u][s] < 0.0 ? 0.0 : v[u][s]) : (f.normalize == 2 ? 0.5 * (v[u][s] + 1.0) : v[u][s]);
                        ms *= pow(fv[s], f.beta[s]);
                    }
                }
                run += ms;
                if (g == 0) {
                    if (per_image) per_image[b] = ms;
                    if (wgt) {
#pragma unroll
                        for (int s = 0; s < SS_MAX_S; ++s) {
                            if (s < f.S) {
                                // d msssim / d v_s = beta_s msssim f'(v_s) / f(v_s); a scale at f = 0 passes nothing (and with a
                                // positive beta it has made msssim, hence every other scale's weight, zero): a dead image has no gradient
                                double d = f.beta[s] * ms / fv[s];
                                if (f.normalize == 2) d *= 0.5;
                                if (f.normalize != 0 && fv[s] == 0.0) d = 0.0;
                                wgt[(size_t)s * f.B + b] = d;
                            }
                        }
                    }
                }
            }
        }
    }
    sh[tid] = run;
    __syncthreads();
    if (tid == 0) {
        double tot = 0.0;
        for (int i = 0; i < ngrp; ++i) tot += sh[i * G];
        state[0] += tot;
        state[1] += (double)f.B;
    }
}

// ---- host: what both entries put into their args and launch the same way -----------------------------------------------------------
static void ss_args_window(SsimArgs& a, int C, int kh, int kw, const double* wh, const double* ww, double k1, double k2, int range_mode,
                           double range_lo, double range_hi, double* state) {
    a.C = C, a.kh = kh, a.kw = kw;
    a.mode = range_mode;
    a.lo = range_mode == 2 ? 0.0 : range_lo, a.hi = range_mode == 2 ? 0.0 : range_hi;
    a.k1 = k1, a.k2 = k2;
    a.range = state + SS_HEAD;
    ssim_fill_window(a.wh, a.ww, wh, ww, kh, kw);
}

// one [B][C][H][W] pair: its geometry into the args, the range pass in front of the tile launch (range_mode 2); returns the grid
static unsigned ss_args_pair(SsimArgs& a, int in_dtype, const void* p, const void* t, int B, int H, int W, double* ws, hipStream_t st) {
    a.p = p, a.t = t, a.ws = ws;
    a.H = H, a.W = W, a.Ho = H - a.kh + 1, a.Wo = W - a.kw + 1;
    a.ntx = cdiv(a.Wo, SS_TW), a.nty = cdiv(a.Ho, SS_TH), a.tiles = a.ntx * a.nty;
    const int64_t numel = (int64_t)B * a.C * H * W;
    a.parts = imax(1, imin(SS_PARTS, cdiv(numel, SS_THREADS * 16)));
    double* range = const_cast<double*>(a.range);
    if (a.mode == 2) {
        if (in_dtype == 0) ss_range_kernel<float><<<a.parts, SS_THREADS, 0, st>>>((const float*)p, (const float*)t, numel, range);
        else ss_range_kernel<double><<<a.parts, SS_THREADS, 0, st>>>((const double*)p, (const double*)t, numel, range);
    }
    return (unsigned)((int64_t)B * a.C * a.tiles);
}

extern "C" int otvae_ssim_accum(int in_dtype, const void* preds, const void* target, int B, int C, int H, int W, int kh, int kw,
                                const double* wh, const double* ww, double k1, double k2, int range_mode, double range_lo,
                                double range_hi, double* per_image, double* state, void* ws, void* stream) {
    OTVAE_REQUIRE(preds && target && wh && ww && state && ws, "otvae_ssim_accum: null argument");
    OTVAE_REQUIRE(in_dtype == 0 || in_dtype == 1, "otvae_ssim_accum: in_dtype must be 0 (fp32) or 1 (fp64)");
    OTVAE_REQUIRE(ssim_args_ok(B, C, H, W, kh, kw),
                  "otvae_ssim_accum: need B, C >= 1, odd windows and H >= kh, W >= kw (got B %d, C %d, %d x %d images, %d x %d window)", B, C,
                  H, W, kh, kw);
    OTVAE_REQUIRE(range_mode >= 0 && range_mode <= 2, "otvae_ssim_accum: range_mode must be 0, 1 or 2");
    OTVAE_REQUIRE(range_mode == 2 || range_hi > range_lo, "otvae_ssim_accum: range_hi must exceed range_lo");
    OTVAE_REQUIRE(k1 >= 0.0 && k2 >= 0.0, "otvae_ssim_accum: k1 and k2 must not be negative");
    if (!ssim_supported(B, C, H, W, kh, kw)) {
        otvae_set_error("otvae_ssim_accum: a %d x %d window on %d x %d x %d x %d is beyond the envelope (%d taps per axis, 2^31 tiles)", kh,
                        kw, B, C, H, W, SS_MAX_K);
        return OTVAE_EUNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    SsimArgs a;
    ss_args_window(a, C, kh, kw, wh, ww, k1, k2, range_mode, range_lo, range_hi, state);
    const unsigned blocks = ss_args_pair(a, in_dtype, preds, target, B, H, W, (double*)ws, st);
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

extern "C" int otvae_ms_ssim_accum(int in_dtype, const void* preds, const void* target, int B, int C, int H, int W, int kh, int kw,
                                   const double* wh, const double* ww, double k1, double k2, int range_mode, double range_lo,
                                   double range_hi, int S, const double* betas, int normalize, double* per_image, double* w,
                                   void* pyr_preds, void* pyr_target, double* state, void* ws, void* stream) {
    OTVAE_REQUIRE(preds && target && wh && ww && betas && state && ws, "otvae_ms_ssim_accum: null argument");
    OTVAE_REQUIRE(in_dtype == 0 || in_dtype == 1, "otvae_ms_ssim_accum: in_dtype must be 0 (fp32) or 1 (fp64)");
    OTVAE_REQUIRE(ssim_args_ok(B, C, H, W, kh, kw, S),
                  "otvae_ms_ssim_accum: need B, C, S >= 1, odd windows and H >> (S - 1) >= kh, W >> (S - 1) >= kw (got B %d, C %d, %d x %d "
                  "images, %d x %d window, %d scales)", B, C, H, W, kh, kw, S);
    OTVAE_REQUIRE(S == 1 || (pyr_preds && pyr_target), "otvae_ms_ssim_accum: more than one scale needs the two pyramids");
    OTVAE_REQUIRE(range_mode >= 0 && range_mode <= 2, "otvae_ms_ssim_accum: range_mode must be 0, 1 or 2");
    OTVAE_REQUIRE(range_mode == 2 || range_hi > range_lo, "otvae_ms_ssim_accum: range_hi must exceed range_lo");
    OTVAE_REQUIRE(k1 >= 0.0 && k2 >= 0.0, "otvae_ms_ssim_accum: k1 and k2 must not be negative");
    OTVAE_REQUIRE(normalize >= 0 && normalize <= 2, "otvae_ms_ssim_accum: normalize must be 0 (none), 1 (relu) or 2 (simple)");
    if (!ms_ssim_supported(B, C, H, W, kh, kw, S, SS_MAX_K)) {
        otvae_set_error("otvae_ms_ssim_accum: %d scales of a %d x %d window on %d x %d x %d x %d are beyond the envelope (%d scales, %d "
                        "taps per axis, 2^31 tiles)", S, kh, kw, B, C, H, W, SS_MAX_S, SS_MAX_K);
        return OTVAE_EUNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    const size_t esz = in_dtype == 0 ? 4 : 8;
    MsArgs a;
    ss_args_window(a, C, kh, kw, wh, ww, k1, k2, range_mode, range_lo, range_hi, state);
    MsFoldArgs f;
    f.S = S, f.B = B, f.normalize = normalize;
    const size_t lds = ss_lds_bytes(kh, kw);
    const bool k11 = kh == 11 && kw == 11;   // the default window: the unrolled instantiation
    const char *cur_p = (const char*)preds, *cur_t = (const char*)target;
    char *nxt_p = (char*)pyr_preds, *nxt_t = (char*)pyr_target;
    int64_t off = 0;
    for (int s = 0; s < S; ++s) {
        const unsigned blocks = ss_args_pair(a, in_dtype, cur_p, cur_t, B, H >> s, W >> s, (double*)ws + off, st);
        a.pool_p = s + 1 < S ? nxt_p : nullptr, a.pool_t = s + 1 < S ? nxt_t : nullptr;
        a.Hp = a.H >> 1, a.Wp = a.W >> 1;
        if (in_dtype == 0) {
            if (k11) ms_tile_kernel<float, 11><<<blocks, SS_THREADS, lds, st>>>(a);
            else ms_tile_kernel<float, 0><<<blocks, SS_THREADS, lds, st>>>(a);
        } else {
            if (k11) ms_tile_kernel<double, 11><<<blocks, SS_THREADS, lds, st>>>(a);
            else ms_tile_kernel<double, 0><<<blocks, SS_THREADS, lds, st>>>(a);
        }
        f.P[s] = C * a.tiles, f.off[s] = off, f.count[s] = (double)C * a.Ho * a.Wo, f.beta[s] = betas[s];
        off += 2 * (int64_t)B * C * a.tiles;
        cur_p = nxt_p, cur_t = nxt_t;
        nxt_p += (size_t)ssim_scale_elems(B, C, H, W, s + 1) * esz, nxt_t += (size_t)ssim_scale_elems(B, C, H, W, s + 1) * esz;
    }
    int G = 1;
    while (G < 16 && G < f.P[0]) G <<= 1;
    f.G = G;
    ms_fold_kernel<<<1, SS_THREADS, 0, st>>>((const double*)ws, f, per_image, w, state);
    OTVAE_CHECK_LAUNCH("otvae_ms_ssim_accum");
    return OTVAE_OK;
}
