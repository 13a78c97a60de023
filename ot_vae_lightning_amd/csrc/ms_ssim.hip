// Multi-scale SSIM on the device (metrics/ms_ssim.py, losses.py's MSSSIMLoss; formulas, layouts and envelope: include/otvae.h,
// otvae_ms_ssim_accum / otvae_ms_ssim_grad).  The numerical method is that of csrc/ssim.hip and csrc/ssim_grad.hip -- fp32 differences
// from a pixel of the tile in LDS, separable passes, the map in fp64 from the five fp32 moments, fixed-order sums, no atomics, no host
// read -- and those two files are left as they are: their entries keep their code objects bit for bit.  What is new here:
//
//   ms_tile_kernel   forward, one launch per scale; one workgroup per (image, channel, MS_TH x MS_TW tile of window positions), as
//                    ss_tile_kernel.  From the same five moments it evaluates cs = A2 / B2 and ssim = A1 A2 / (B1 B2) with ONE fp64
//                    division (r = 1 / (B1 B2); ssim = A1 A2 r, cs = A2 B1 r) and leaves two doubles per workgroup, {sum cs, sum ssim}.
//                    A wave stages row PAIRS (rows 2 w, 2 w + 1, 2 w + 8, 2 w + 9, ... of the tile), so a thread holds both rows of a
//                    2 x 2 pooling cell of its column in registers; the neighbouring column comes by one lane shift.  The workgroup
//                    writes the pooled pair of the next scale from the RAW (unclamped) pixels it owns, in the input's type: a tile owns
//                    its MS_TH x MS_TW pixels, the last tile row / column all pixels up to H / W (they are all staged there).  Tiles
//                    start at even coordinates, so no cell straddles two owners: every pooled element is written exactly once, and
//                    the scale's pair is read from memory once.
//   ms_range_kernel  range_mode 2: the per-scale range pass of csrc/ssim.hip, in front of each scale's launch.
//   ms_fold_kernel   one workgroup, all scales: G <= 16 lanes (G from scale 0's partial count alone) share an image and sum each
//                    scale's partials in a fixed order -> v_s[b]; msssim_b = prod_s f(v_s)^beta_s and w_s[b] = d msssim_b / d v_s[b] in fp64;
//                    state[0] += sum_b msssim_b, state[1] += B.
//   msg_tile_kernel  backward, one launch per scale from the coarsest to the finest; ssg_tile_kernel with the scale's weight
//                    g[b] w_s[b] / n_s in front of the coefficients, the cs coefficients (dS/dmu = 0, b = -cs / B2, c = 2 / B2) or the
//                    ssim ones by a flag, and 1/4 of the coarser scale's gradient added at the store.  Every element is written.
// LDS per workgroup (dynamic, as launched): forward 128 + 4 (2 SR SC + 5 SR 32) bytes, SR = 15 + kh, SC = 31 + kw: 25.5 KiB for the
// 11 x 11 window, 51.2 KiB at 31 x 31; backward 4 (2 SR SC + max(5 SR PC, 3 PR (PC + 32))) bytes with SR = 16 + 2 (kh - 1),
// SC = 32 + 2 (kw - 1), PR = 15 + kh, PC = 31 + kw: 44.2 KiB for 11 x 11, 60.2 KiB at 15 x 15.  Registers and occupancy: DESIGN.md.
#include "common.h"

#define MS_TH 16
#define MS_TW 32
#define MS_MAX_K 31          // forward taps per axis
#define MS_MAX_KG 15         // backward taps per axis
#define MS_MAX_S 8
#define MS_THREADS 256
#define MS_PARTS 256         // workgroups of the range pass at most
#define MS_HEAD 4            // state: sum, count, two unused words, then 4 x MS_PARTS doubles of range partials

static_assert(MS_TW + 2 * (MS_MAX_KG - 1) <= 64 && MS_TW + MS_MAX_K - 1 <= 64, "one lane per staged column");
static_assert(MS_TH % 2 == 0 && MS_TW % 2 == 0, "a pooling cell has one owner");

extern "C" int otvae_ms_ssim_state_words(void) { return MS_HEAD + 4 * MS_PARTS; }

static int64_t ms_tiles(int H, int W, int kh, int kw) { return (int64_t)cdiv(H - kh + 1, MS_TH) * cdiv(W - kw + 1, MS_TW); }
static int64_t msg_tiles(int H, int W) { return (int64_t)cdiv(H, MS_TH) * cdiv(W, MS_TW); }
static bool ms_args_ok(int B, int C, int H, int W, int kh, int kw, int S) {
    return B > 0 && C > 0 && kh > 0 && kw > 0 && (kh & 1) && (kw & 1) && S >= 1 &&
           (S > MS_MAX_S || ((H >> (S - 1)) >= kh && (W >> (S - 1)) >= kw));
}
static bool ms_supported(int B, int C, int H, int W, int kh, int kw, int S, int max_k) {
    return S <= MS_MAX_S && kh <= max_k && kw <= max_k && (int64_t)H * W < ((int64_t)1 << 31) &&
           (int64_t)B * C * ms_tiles(H, W, kh, kw) < ((int64_t)1 << 31) && (int64_t)B * C * msg_tiles(H, W) < ((int64_t)1 << 31);
}
// elements of one image's pyramid: scales 1 .. S - 1 of [B][C][H >> s][W >> s]
static int64_t ms_pyramid_elems(int B, int C, int H, int W, int S) {
    int64_t n = 0;
    for (int s = 1; s < S; ++s) n += (int64_t)B * C * (H >> s) * (W >> s);
    return n;
}

extern "C" int64_t otvae_ms_ssim_pyramid(int in_dtype, int B, int C, int H, int W, int S) {
    if ((in_dtype != 0 && in_dtype != 1) || B <= 0 || C <= 0 || H <= 0 || W <= 0 || S < 1 || S > MS_MAX_S) return -1;
    return ms_pyramid_elems(B, C, H, W, S) * (in_dtype == 0 ? 4 : 8);
}

extern "C" int64_t otvae_ms_ssim_ws(int B, int C, int H, int W, int kh, int kw, int S) {
    if (!ms_args_ok(B, C, H, W, kh, kw, S) || !ms_supported(B, C, H, W, kh, kw, S, MS_MAX_K)) return -1;
    int64_t n = 0;
    for (int s = 0; s < S; ++s) n += 2 * (int64_t)B * C * ms_tiles(H >> s, W >> s, kh, kw);
    return n * (int64_t)sizeof(double);
}

extern "C" int64_t otvae_ms_ssim_grad_ws(int in_dtype, int B, int C, int H, int W, int kh, int kw, int S) {
    if ((in_dtype != 0 && in_dtype != 1) || !ms_args_ok(B, C, H, W, kh, kw, S) || !ms_supported(B, C, H, W, kh, kw, S, MS_MAX_KG)) return -1;
    // the gradients of scales 1 .. S - 1 alternate between two buffers: odd scales in the first, even ones in the second
    const int64_t n1 = S > 1 ? (int64_t)B * C * (H >> 1) * (W >> 1) : 0, n2 = S > 2 ? (int64_t)B * C * (H >> 2) * (W >> 2) : 0;
    return (n1 + n2) * (in_dtype == 0 ? 4 : 8);
}

// min / max that keep a NaN once they have met one (torch's amin / amax do)
__device__ __forceinline__ double ms_min(double a, double b) { return (b < a || b != b) ? b : a; }
__device__ __forceinline__ double ms_max(double a, double b) { return (b > a || b != b) ? b : a; }

// v = {min p, max p, min t, max t} over the block; red: 16 doubles of LDS.  Ends with every thread holding the result.
__device__ __forceinline__ void ms_block_minmax(double (&v)[4], double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        v[0] = ms_min(v[0], __shfl_xor(v[0], o, 64));
        v[1] = ms_max(v[1], __shfl_xor(v[1], o, 64));
        v[2] = ms_min(v[2], __shfl_xor(v[2], o, 64));
        v[3] = ms_max(v[3], __shfl_xor(v[3], o, 64));
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
        v[q] = (q & 1) ? ms_max(ms_max(a, b), ms_max(c, d)) : ms_min(ms_min(a, b), ms_min(c, d));
    }
    __syncthreads();
}

// range[q * MS_PARTS + block], q = min p, max p, min t, max t
template <typename TIN>
__global__ __launch_bounds__(MS_THREADS) void ms_range_kernel(const TIN* __restrict__ p, const TIN* __restrict__ t, int64_t numel,
                                                              double* __restrict__ range) {
    __shared__ double red[16];
    double v[4] = {INFINITY, -INFINITY, INFINITY, -INFINITY};
    for (int64_t e = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x; e < numel; e += (int64_t)gridDim.x * MS_THREADS) {
        const double pv = (double)p[e], tv = (double)t[e];
        v[0] = ms_min(v[0], pv);
        v[1] = ms_max(v[1], pv);
        v[2] = ms_min(v[2], tv);
        v[3] = ms_max(v[3], tv);
    }
    ms_block_minmax(v, red);
    if (threadIdx.x < 4) range[threadIdx.x * MS_PARTS + blockIdx.x] = v[threadIdx.x];
}

struct MsArgs {
    const void* p;
    const void* t;
    void* pool_p;          // the next scale's pair [planes][Hp][Wp]; NULL at the last scale
    void* pool_t;
    int C, H, W, kh, kw;
    int Ho, Wo, ntx, nty, tiles;
    int Hp, Wp;
    int mode, parts;
    double lo, hi, k1, k2;
    const double* range;   // mode 2: the range pass's partials
    double* ws;            // [workgroup][2]
    float wh[MS_MAX_K], ww[MS_MAX_K];
};

static size_t ms_lds_bytes(int kh, int kw) {
    const size_t SR = MS_TH + kh - 1, SC = MS_TW + kw - 1;
    return 16 * sizeof(double) + (2 * SR * SC + 5 * SR * MS_TW) * sizeof(float);
}

template <typename TIN>
__device__ __forceinline__ TIN ms_clamp(TIN v, TIN lo, TIN hi) {   // a NaN stays a NaN
    return v < lo ? lo : (v > hi ? hi : v);
}

// one position in fp64 from the five fp32 moments of the differences (the pivots go back into the means here): cs and ssim are added
// to their running sums
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
__global__ __launch_bounds__(MS_THREADS) void ms_tile_kernel(const MsArgs a) {
    extern __shared__ __attribute__((aligned(16))) char ms_smem[];
    double* red = reinterpret_cast<double*>(ms_smem);   // 16 doubles
    const int kh = K ? K : a.kh, kw = K ? K : a.kw;
    const int SR = MS_TH + kh - 1, SC = MS_TW + kw - 1;
    float* sp = reinterpret_cast<float*>(ms_smem + 16 * sizeof(double));   // [SR][SC] p - pivot
    float* st = sp + SR * SC;                                              // [SR][SC] t - pivot
    float* hq = st + SR * SC;                                              // [5][SR][MS_TW] row sums
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    const unsigned plane = blockIdx.x / (unsigned)a.tiles, tile = blockIdx.x % (unsigned)a.tiles;
    const int ty = (int)(tile / (unsigned)a.ntx), tx = (int)(tile % (unsigned)a.ntx);
    const int r0 = ty * MS_TH, c0 = tx * MS_TW;
    const int nvr = min(MS_TH, a.Ho - r0), nvc = min(MS_TW, a.Wo - c0);   // positions of this tile, >= 1 each
    const int rows = nvr + kh - 1, cols = nvc + kw - 1;                    // staged pixels: r0 + rows <= H, c0 + cols <= W

    double R = a.hi - a.lo;
    if (a.mode == 2) {
        double v[4] = {INFINITY, -INFINITY, INFINITY, -INFINITY};
        if (tid < a.parts) {
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = a.range[q * MS_PARTS + tid];
        }
        ms_block_minmax(v, red);
        R = ms_max(v[1] - v[0], v[3] - v[2]);
    }
    const double c1 = (a.k1 * R) * (a.k1 * R), c2 = (a.k2 * R) * (a.k2 * R);

    const TIN* __restrict__ pp = static_cast<const TIN*>(a.p) + (size_t)plane * a.H * a.W + (size_t)r0 * a.W + c0;
    const TIN* __restrict__ tt = static_cast<const TIN*>(a.t) + (size_t)plane * a.H * a.W + (size_t)r0 * a.W + c0;
    const bool clamp = a.mode == 1;
    const TIN lo = (TIN)a.lo, hi = (TIN)a.hi;
    TIN piv_p = pp[0], piv_t = tt[0];
    if (clamp) piv_p = ms_clamp(piv_p, lo, hi), piv_t = ms_clamp(piv_t, lo, hi);

    // stage: wave w takes the row pairs (2 w, 2 w + 1), (2 w + 8, 2 w + 9), ...; lane = column (SC <= 62).  All of a thread's loads
    // are issued before the first is used.  Threads past the tile load its last row / column again (an address inside the image, no
    // branch around the load) and store nothing.
    constexpr int NST = 2 * ((MS_TH + (K ? K : MS_MAX_K) - 1 + 7) / 8);
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
            if (clamp) x = ms_clamp(x, lo, hi), y = ms_clamp(y, lo, hi);
            sp[r * SC + lane] = (float)(x - piv_p);
            st[r * SC + lane] = (float)(y - piv_t);
        }
    }
    // the next scale's pair from the raw pixels this tile owns: rows r, r + 1 are xs[u], xs[u + 1], column lane + 1 is one lane up.
    // A cell is written only if it lies inside the pooled image (pr < Hp, pc < Wp: then both of its rows and columns are inside this
    // tile's staged block) and its first pixel is owned here.
    if (a.pool_p) {   // (uniform over the launch)
        const int own_r = ty == a.nty - 1 ? rows : MS_TH, own_c = tx == a.ntx - 1 ? cols : MS_TW;
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

    const int col = tid & (MS_TW - 1);
    double acc_cs = 0.0, acc_ss = 0.0;
    if constexpr (K > 0) {
        // horizontal pass: thread -> (staged row, four neighbouring positions).  A group that reaches past the tile's positions reads
        // LDS that was not staged (inside the row's SC slots); what it makes of it lands in columns >= nvc, which nobody reads.
        constexpr int NO = 4, NP = NO + K - 1;
        static_assert(MS_TW % NO == 0 && (2 * (MS_TH + K - 1) * (MS_TW + K - 1)) % 4 == 0, "16-byte stores of the row sums");
        float wgt[K];
#pragma unroll
        for (int j = 0; j < K; ++j) wgt[j] = a.ww[j];
        const int c4 = (tid & (MS_TW / NO - 1)) * NO;
        if (c4 < nvc) {
            for (int r = tid / (MS_TW / NO); r < rows; r += MS_THREADS / (MS_TW / NO)) {
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
                for (int q = 0; q < 5; ++q) *reinterpret_cast<f32x4*>(hq + (q * SR + r) * MS_TW + c4) = s[q];
            }
        }
        __syncthreads();

        // vertical pass and the map: thread -> positions (2 (tid / 32), col) and the one below it, from K + 1 rows of row sums.  The
        // lower position may lie past the tile (then its last row was never written): it is computed and dropped.
#pragma unroll
        for (int j = 0; j < K; ++j) wgt[j] = a.wh[j];
        const int o0 = 2 * (tid >> 5);
        if (col < nvc && o0 < nvr) {
            const float* __restrict__ h = hq + o0 * MS_TW + col;
            float m0[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, m1[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i <= K; ++i) {
#pragma unroll
                for (int q = 0; q < 5; ++q) {
                    const float v = h[(q * SR + i) * MS_TW];
                    if (i < K) m0[q] = fmaf(wgt[i], v, m0[q]);
                    if (i > 0) m1[q] = fmaf(wgt[i - 1], v, m1[q]);
                }
            }
            ms_map(m0, (double)piv_p, (double)piv_t, c1, c2, acc_cs, acc_ss);
            double below_cs = 0.0, below_ss = 0.0;
            ms_map(m1, (double)piv_p, (double)piv_t, c1, c2, below_cs, below_ss);
            if (o0 + 1 < nvr) acc_cs += below_cs, acc_ss += below_ss;
        }
    } else {
        // horizontal pass: thread -> (staged row, position column)
        if (col < nvc) {
            for (int r = tid >> 5; r < rows; r += MS_THREADS / MS_TW) {
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
                float* h = hq + r * MS_TW + col;
                h[0] = s0;
                h[SR * MS_TW] = s1;
                h[2 * SR * MS_TW] = s2;
                h[3 * SR * MS_TW] = s3;
                h[4 * SR * MS_TW] = s4;
            }
        }
        __syncthreads();

        // vertical pass and the map: thread -> positions (tid / 32 + 8 u, col)
        if (col < nvc) {
            for (int orow = tid >> 5; orow < nvr; orow += MS_THREADS / MS_TW) {
                const float* __restrict__ h = hq + orow * MS_TW + col;
                float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
                for (int i = 0; i < kh; ++i) {
                    const float w = a.wh[i];
#pragma unroll
                    for (int q = 0; q < 5; ++q) m[q] = fmaf(w, h[(q * SR + i) * MS_TW], m[q]);
                }
                ms_map(m, (double)piv_p, (double)piv_t, c1, c2, acc_cs, acc_ss);
            }
        }
    }
    acc_cs = wave_sum(acc_cs);
    acc_ss = wave_sum(acc_ss);
    if (lane == 0) red[wave] = acc_cs, red[4 + wave] = acc_ss;
    __syncthreads();
    if (tid < 2) a.ws[2 * (size_t)blockIdx.x + tid] = (red[4 * tid] + red[4 * tid + 1]) + (red[4 * tid + 2] + red[4 * tid + 3]);
}

struct MsFoldArgs {
    int S, B, G, normalize;      // normalize 0: none, 1: relu, 2: simple
    int P[MS_MAX_S];             // partial pairs per image at scale s
    long long off[MS_MAX_S];     // where scale s begins in the workspace, in doubles
    double count[MS_MAX_S], beta[MS_MAX_S];
};

#define MS_FOLD_U 4          // images per group and trip: their loads are in flight together

// one workgroup.  G (a power of two <= 16, from scale 0's P alone) lanes share an image: lane g sums partials g, g + G, ... of each
// scale (cs below the last scale, ssim at it) and an xor tree joins them; a group's images are added to its running sum in batch order,
// the groups' sums in group order.
__global__ __launch_bounds__(MS_THREADS) void ms_fold_kernel(const double* __restrict__ ws, const MsFoldArgs f,
                                                             double* __restrict__ per_image, double* __restrict__ wgt,
                                                             double* __restrict__ state) {
    __shared__ double sh[MS_THREADS];
    const int tid = threadIdx.x, G = f.G, g = tid & (G - 1), grp = tid / G, ngrp = MS_THREADS / G;
    double run = 0.0;
    for (int b0 = 0; b0 < f.B; b0 += MS_FOLD_U * ngrp) {
        double v[MS_FOLD_U][MS_MAX_S];
#pragma unroll
        for (int s = 0; s < MS_MAX_S; ++s) {
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
                double fv[MS_MAX_S], ms = 1.0;
#pragma unroll
                for (int s = 0; s < MS_MAX_S; ++s) {
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
                        for (int s = 0; s < MS_MAX_S; ++s) {
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

extern "C" int otvae_ms_ssim_accum(int in_dtype, const void* preds, const void* target, int B, int C, int H, int W, int kh, int kw,
                                   const double* wh, const double* ww, double k1, double k2, int range_mode, double range_lo,
                                   double range_hi, int S, const double* betas, int normalize, double* per_image, double* w,
                                   void* pyr_preds, void* pyr_target, double* state, void* ws, void* stream) {
    OTVAE_REQUIRE(preds && target && wh && ww && betas && state && ws, "otvae_ms_ssim_accum: null argument");
    OTVAE_REQUIRE(in_dtype == 0 || in_dtype == 1, "otvae_ms_ssim_accum: in_dtype must be 0 (fp32) or 1 (fp64)");
    OTVAE_REQUIRE(ms_args_ok(B, C, H, W, kh, kw, S),
                  "otvae_ms_ssim_accum: need B, C, S >= 1, odd windows and H >> (S - 1) >= kh, W >> (S - 1) >= kw (got B %d, C %d, %d x %d "
                  "images, %d x %d window, %d scales)", B, C, H, W, kh, kw, S);
    OTVAE_REQUIRE(S == 1 || (pyr_preds && pyr_target), "otvae_ms_ssim_accum: more than one scale needs the two pyramids");
    OTVAE_REQUIRE(range_mode >= 0 && range_mode <= 2, "otvae_ms_ssim_accum: range_mode must be 0, 1 or 2");
    OTVAE_REQUIRE(range_mode == 2 || range_hi > range_lo, "otvae_ms_ssim_accum: range_hi must exceed range_lo");
    OTVAE_REQUIRE(k1 >= 0.0 && k2 >= 0.0, "otvae_ms_ssim_accum: k1 and k2 must not be negative");
    OTVAE_REQUIRE(normalize >= 0 && normalize <= 2, "otvae_ms_ssim_accum: normalize must be 0 (none), 1 (relu) or 2 (simple)");
    if (!ms_supported(B, C, H, W, kh, kw, S, MS_MAX_K)) {
        otvae_set_error("otvae_ms_ssim_accum: %d scales of a %d x %d window on %d x %d x %d x %d are beyond the envelope (%d scales, %d "
                        "taps per axis, 2^31 tiles)", S, kh, kw, B, C, H, W, MS_MAX_S, MS_MAX_K);
        return OTVAE_EUNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    const size_t esz = in_dtype == 0 ? 4 : 8;
    MsArgs a;
    a.C = C, a.kh = kh, a.kw = kw;
    a.mode = range_mode;
    a.lo = range_mode == 2 ? 0.0 : range_lo, a.hi = range_mode == 2 ? 0.0 : range_hi;
    a.k1 = k1, a.k2 = k2;
    a.range = state + MS_HEAD;
    for (int i = 0; i < MS_MAX_K; ++i) a.wh[i] = i < kh ? (float)wh[i] : 0.f, a.ww[i] = i < kw ? (float)ww[i] : 0.f;
    MsFoldArgs f;
    f.S = S, f.B = B, f.normalize = normalize;
    const size_t lds = ms_lds_bytes(kh, kw);
    const bool k11 = kh == 11 && kw == 11;   // the default window: the unrolled instantiation
    const char *cur_p = (const char*)preds, *cur_t = (const char*)target;
    char *nxt_p = (char*)pyr_preds, *nxt_t = (char*)pyr_target;
    int64_t off = 0;
    for (int s = 0; s < S; ++s) {
        const int Hs = H >> s, Ws = W >> s;
        a.p = cur_p, a.t = cur_t;
        a.pool_p = s + 1 < S ? nxt_p : nullptr, a.pool_t = s + 1 < S ? nxt_t : nullptr;
        a.H = Hs, a.W = Ws, a.Ho = Hs - kh + 1, a.Wo = Ws - kw + 1;
        a.ntx = cdiv(a.Wo, MS_TW), a.nty = cdiv(a.Ho, MS_TH), a.tiles = a.ntx * a.nty;
        a.Hp = Hs >> 1, a.Wp = Ws >> 1;
        a.ws = (double*)ws + off;
        const int64_t numel = (int64_t)B * C * Hs * Ws;
        a.parts = imax(1, imin(MS_PARTS, cdiv(numel, MS_THREADS * 16)));
        if (range_mode == 2) {
            if (in_dtype == 0) ms_range_kernel<float><<<a.parts, MS_THREADS, 0, st>>>((const float*)cur_p, (const float*)cur_t, numel, state + MS_HEAD);
            else ms_range_kernel<double><<<a.parts, MS_THREADS, 0, st>>>((const double*)cur_p, (const double*)cur_t, numel, state + MS_HEAD);
        }
        const unsigned blocks = (unsigned)((int64_t)B * C * a.tiles);
        if (in_dtype == 0) {
            if (k11) ms_tile_kernel<float, 11><<<blocks, MS_THREADS, lds, st>>>(a);
            else ms_tile_kernel<float, 0><<<blocks, MS_THREADS, lds, st>>>(a);
        } else {
            if (k11) ms_tile_kernel<double, 11><<<blocks, MS_THREADS, lds, st>>>(a);
            else ms_tile_kernel<double, 0><<<blocks, MS_THREADS, lds, st>>>(a);
        }
        f.P[s] = C * a.tiles, f.off[s] = off, f.count[s] = (double)C * a.Ho * a.Wo, f.beta[s] = betas[s];
        off += 2 * (int64_t)B * C * a.tiles;
        cur_p = nxt_p, cur_t = nxt_t;
        nxt_p += (size_t)B * C * a.Hp * a.Wp * esz, nxt_t += (size_t)B * C * a.Hp * a.Wp * esz;
    }
    int G = 1;
    while (G < 16 && G < f.P[0]) G <<= 1;
    f.G = G;
    ms_fold_kernel<<<1, MS_THREADS, 0, st>>>((const double*)ws, f, per_image, w, state);
    OTVAE_CHECK_LAUNCH("otvae_ms_ssim_accum");
    return OTVAE_OK;
}

// ------------------------------------------------------------------------------------------------------------------ the gradient
struct MsGradArgs {
    const void* p;
    const void* t;
    const void* coarse;    // the next coarser scale's gradient [planes][Hc][Wc]; NULL at the last scale
    void* grad;
    const double* g;       // [B] upstream
    const double* w;       // [B] d msssim_b / d v_s[b] of this scale
    int B, C, H, W, kh, kw;
    int Ho, Wo, ntx, tiles;
    int Hc, Wc;
    int mode, cs_only;
    double lo, hi, k1, k2;
    float wh[MS_MAX_KG], ww[MS_MAX_KG];
};

static size_t msg_lds_bytes(int kh, int kw) {
    const size_t SR = MS_TH + 2 * (kh - 1), SC = MS_TW + 2 * (kw - 1), PR = MS_TH + kh - 1, PC = MS_TW + kw - 1;
    const size_t sums = 5 * SR * PC, coef = 3 * PR * (PC + MS_TW);
    return (2 * SR * SC + (sums > coef ? sums : coef)) * sizeof(float);
}

// K > 0: a K x K window known at compile time (the default 11 x 11).  K == 0: window sizes from the arguments.
template <typename TIN, int K>
__global__ __launch_bounds__(MS_THREADS) void msg_tile_kernel(const MsGradArgs a) {
    extern __shared__ __attribute__((aligned(16))) char msg_smem[];
    const int kh = K ? K : a.kh, kw = K ? K : a.kw;
    const int SR = MS_TH + 2 * (kh - 1), SC = MS_TW + 2 * (kw - 1);   // staged pixels at most
    const int PR = MS_TH + kh - 1, PC = MS_TW + kw - 1;               // positions at most
    float* sp = reinterpret_cast<float*>(msg_smem);   // [SR][SC] p - pivot
    float* st = sp + SR * SC;                         // [SR][SC] t - pivot
    float* hq = st + SR * SC;                         // [5][SR][PC] row sums; later:
    float* cf = hq;                                   // [3][PR][PC] coefficients
    float* th = cf + 3 * PR * PC;                     // [3][PR][MS_TW] their horizontal adjoint
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    const unsigned plane = blockIdx.x / (unsigned)a.tiles, tile = blockIdx.x % (unsigned)a.tiles;
    const int y0 = (int)(tile / (unsigned)a.ntx) * MS_TH, x0 = (int)(tile % (unsigned)a.ntx) * MS_TW;
    const int ph = min(MS_TH, a.H - y0), pw = min(MS_TW, a.W - x0);                 // pixels of this tile, >= 1 each
    const int ur0 = max(0, y0 - kh + 1), uc0 = max(0, x0 - kw + 1);                  // first position that reaches the tile
    const int npr = min(a.Ho - 1, y0 + ph - 1) - ur0 + 1, npc = min(a.Wo - 1, x0 + pw - 1) - uc0 + 1;   // positions, 1 .. PR / PC
    const int rows = npr + kh - 1, cols = npc + kw - 1;                              // staged pixels: ur0 + rows <= H, uc0 + cols <= W

    const double R = a.hi - a.lo;
    const double c1 = (a.k1 * R) * (a.k1 * R), c2 = (a.k2 * R) * (a.k2 * R);
    const unsigned img = plane / (unsigned)a.C;
    const double gscale = a.g[img] * a.w[img] / ((double)a.C * a.Ho * a.Wo);
    const bool cs_only = a.cs_only != 0;

    const size_t plane_at = (size_t)plane * a.H * a.W;
    const TIN* __restrict__ pp = static_cast<const TIN*>(a.p) + plane_at + (size_t)ur0 * a.W + uc0;
    const TIN* __restrict__ tt = static_cast<const TIN*>(a.t) + plane_at + (size_t)ur0 * a.W + uc0;
    const bool clamp = a.mode == 1;
    const TIN lo = (TIN)a.lo, hi = (TIN)a.hi;
    TIN piv_p = pp[0], piv_t = tt[0];
    if (clamp) piv_p = ms_clamp(piv_p, lo, hi), piv_t = ms_clamp(piv_t, lo, hi);

    // stage: wave w takes rows w, w + 4, ...; lane = column (SC <= 64).  All loads are issued before the first is used; threads past
    // the staged block load its last row / column again (an address inside the image) and store nothing.
    constexpr int NST = (MS_TH + 2 * ((K ? K : MS_MAX_KG) - 1) + 3) / 4;
    {
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
                if (clamp) x = ms_clamp(x, lo, hi), y = ms_clamp(y, lo, hi);
                sp[r * SC + lane] = (float)(x - piv_p);
                st[r * SC + lane] = (float)(y - piv_t);
            }
        }
    }
    __syncthreads();

    // horizontal pass: (staged row r, position column c) -> five row sums
    for (int idx = tid; idx < rows * PC; idx += MS_THREADS) {
        const int r = idx / PC, c = idx - r * PC;
        if (c < npc) {
            const float* __restrict__ xa = sp + r * SC + c;
            const float* __restrict__ ya = st + r * SC + c;
            float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
#pragma unroll
            for (int j = 0; j < kw; ++j) {
                const float w = a.ww[j], x = xa[j], y = ya[j];
                const float wx = w * x, wy = w * y;
                s0 += wx;
                s1 += wy;
                s2 = fmaf(wx, x, s2);
                s3 = fmaf(wy, y, s3);
                s4 = fmaf(wx, y, s4);
            }
            float* h = hq + r * PC + c;
            h[0] = s0;
            h[SR * PC] = s1;
            h[2 * SR * PC] = s2;
            h[3 * SR * PC] = s3;
            h[4 * SR * PC] = s4;
        }
    }
    __syncthreads();

    // vertical pass and the three coefficients of each position, held in registers until every thread is done with the row sums.
    // With V the scale's map (cs or ssim) and d mu the windowed mean of the differences,
    //   b = dV/ds_pp, c = dV/ds_pt, a' = dV/dmu_p (at fixed variances) - 2 b dmu_p - c dmu_t;
    //   ssim: dV/dmu_p = 2 mu_t A2 / (B1 B2) - 2 mu_p S / B1, b = -S / B2, c = 2 A1 / (B1 B2);   cs: dV/dmu_p = 0, b = -cs / B2, c = 2 / B2.
    constexpr int PMAX = MS_TH + (K ? K : MS_MAX_KG) - 1, QMAX = MS_TW + (K ? K : MS_MAX_KG) - 1;
    constexpr int NPOS = (PMAX * QMAX + MS_THREADS - 1) / MS_THREADS;
    float co[NPOS][3];
#pragma unroll
    for (int u = 0; u < NPOS; ++u) {
        const int idx = tid + u * MS_THREADS;
        const int r = idx / PC, c = idx - r * PC;
        co[u][0] = co[u][1] = co[u][2] = 0.f;
        if (r < npr && c < npc) {
            const float* __restrict__ h = hq + r * PC + c;
            float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < kh; ++i) {
                const float w = a.wh[i];
#pragma unroll
                for (int q = 0; q < 5; ++q) m[q] = fmaf(w, h[(q * SR + i) * PC], m[q]);
            }
            const double dp = (double)m[0], dt = (double)m[1];
            const double spp = (double)m[2] - dp * dp, stt = (double)m[3] - dt * dt, spt = (double)m[4] - dp * dt;
            const double A2 = 2.0 * spt + c2, iB2 = 1.0 / (spp + stt + c2);
            double dmu, bco, cco;
            if (cs_only) {
                dmu = 0.0;
                bco = -A2 * iB2 * iB2, cco = 2.0 * iB2;
            } else {
                const double mp = dp + (double)piv_p, mt = dt + (double)piv_t;
                const double A1 = 2.0 * mp * mt + c1, iB1 = 1.0 / (mp * mp + mt * mt + c1);
                const double S = A1 * A2 * iB1 * iB2;
                dmu = 2.0 * mt * A2 * iB1 * iB2 - 2.0 * mp * S * iB1;
                bco = -S * iB2, cco = 2.0 * A1 * iB1 * iB2;
            }
            co[u][0] = (float)((dmu - 2.0 * bco * dp - cco * dt) * gscale);
            co[u][1] = (float)(bco * gscale);
            co[u][2] = (float)(cco * gscale);
        }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NPOS; ++u) {
        const int idx = tid + u * MS_THREADS;
        const int r = idx / PC, c = idx - r * PC;
        if (r < npr && c < npc) {
#pragma unroll
            for (int q = 0; q < 3; ++q) cf[(q * PR + r) * PC + c] = co[u][q];
        }
    }
    __syncthreads();

    // adjoint horizontal pass: (position row r, pixel column x) <- the positions uc0 + cl with x0 + x - kw + 1 <= uc0 + cl <= x0 + x
    const int xoff = x0 - uc0;
    for (int idx = tid; idx < npr * MS_TW; idx += MS_THREADS) {
        const int r = idx / MS_TW, x = idx % MS_TW;
        if (x < pw) {
            const float* __restrict__ crow = cf + r * PC;
            float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int j = 0; j < kw; ++j) {
                const int cl = xoff + x - j;
                if ((unsigned)cl < (unsigned)npc) {
                    const float w = a.ww[j];
                    s0 = fmaf(w, crow[cl], s0);
                    s1 = fmaf(w, crow[PR * PC + cl], s1);
                    s2 = fmaf(w, crow[2 * PR * PC + cl], s2);
                }
            }
            float* o = th + r * MS_TW + x;
            o[0] = s0;
            o[PR * MS_TW] = s1;
            o[2 * PR * MS_TW] = s2;
        }
    }
    __syncthreads();

    // adjoint vertical pass and the pixel: the own-scale term (0 where range_mode 1 clamped the pixel), plus a quarter of the coarser
    // scale's gradient at the pooled pixel above it (none above a dropped odd row / column)
    const int yoff = y0 - ur0;
    TIN* __restrict__ gout = static_cast<TIN*>(a.grad) + plane_at;
    const TIN* __restrict__ praw = static_cast<const TIN*>(a.p) + plane_at;
    const TIN* __restrict__ gc = a.coarse ? static_cast<const TIN*>(a.coarse) + (size_t)plane * a.Hc * a.Wc : nullptr;
    for (int idx = tid; idx < ph * MS_TW; idx += MS_THREADS) {
        const int y = idx / MS_TW, x = idx % MS_TW;
        if (x < pw) {
            float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int i = 0; i < kh; ++i) {
                const int rl = yoff + y - i;
                if ((unsigned)rl < (unsigned)npr) {
                    const float w = a.wh[i];
                    const float* __restrict__ v = th + rl * MS_TW + x;
                    s0 = fmaf(w, v[0], s0);
                    s1 = fmaf(w, v[PR * MS_TW], s1);
                    s2 = fmaf(w, v[2 * PR * MS_TW], s2);
                }
            }
            const int at = (yoff + y) * SC + xoff + x;
            double grad = (double)s0 + 2.0 * (double)sp[at] * (double)s1 + (double)st[at] * (double)s2;
            const size_t q = (size_t)(y0 + y) * a.W + x0 + x;
            if (clamp) {
                const TIN raw = praw[q];
                if (raw < lo || raw > hi) grad = 0.0;
            }
            const int yc = (y0 + y) >> 1, xc = (x0 + x) >> 1;
            if (gc && yc < a.Hc && xc < a.Wc) grad += 0.25 * (double)gc[(size_t)yc * a.Wc + xc];
            gout[q] = (TIN)grad;
        }
    }
}

extern "C" int otvae_ms_ssim_grad(int in_dtype, const void* preds, const void* target, const void* pyr_preds, const void* pyr_target,
                                  int B, int C, int H, int W, int kh, int kw, const double* wh, const double* ww, double k1, double k2,
                                  int range_mode, double range_lo, double range_hi, int S, const double* g, const double* w,
                                  void* grad_preds, void* ws, void* stream) {
    OTVAE_REQUIRE(preds && target && wh && ww && g && w && grad_preds, "otvae_ms_ssim_grad: null argument");
    OTVAE_REQUIRE(in_dtype == 0 || in_dtype == 1, "otvae_ms_ssim_grad: in_dtype must be 0 (fp32) or 1 (fp64)");
    OTVAE_REQUIRE(ms_args_ok(B, C, H, W, kh, kw, S),
                  "otvae_ms_ssim_grad: need B, C, S >= 1, odd windows and H >> (S - 1) >= kh, W >> (S - 1) >= kw (got B %d, C %d, %d x %d "
                  "images, %d x %d window, %d scales)", B, C, H, W, kh, kw, S);
    OTVAE_REQUIRE(S == 1 || (pyr_preds && pyr_target && ws), "otvae_ms_ssim_grad: more than one scale needs the two pyramids and ws");
    OTVAE_REQUIRE(range_mode == 0 || range_mode == 1,
                  "otvae_ms_ssim_grad: range_mode must be 0 or 1 (got %d): a range taken from the batch depends on the data, a loss needs "
                  "a fixed scale", range_mode);
    OTVAE_REQUIRE(range_hi > range_lo, "otvae_ms_ssim_grad: range_hi must exceed range_lo");
    OTVAE_REQUIRE(k1 >= 0.0 && k2 >= 0.0, "otvae_ms_ssim_grad: k1 and k2 must not be negative");
    if (!ms_supported(B, C, H, W, kh, kw, S, MS_MAX_KG)) {
        otvae_set_error("otvae_ms_ssim_grad: %d scales of a %d x %d window on %d x %d x %d x %d are beyond the envelope (%d scales, %d "
                        "taps per axis, 2^31 tiles)", S, kh, kw, B, C, H, W, MS_MAX_S, MS_MAX_KG);
        return OTVAE_EUNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    const size_t esz = in_dtype == 0 ? 4 : 8;
    MsGradArgs a;
    a.g = g;
    a.B = B, a.C = C, a.kh = kh, a.kw = kw;
    a.mode = range_mode;
    a.lo = range_lo, a.hi = range_hi;
    a.k1 = k1, a.k2 = k2;
    for (int i = 0; i < MS_MAX_KG; ++i) a.wh[i] = i < kh ? (float)wh[i] : 0.f, a.ww[i] = i < kw ? (float)ww[i] : 0.f;
    // where scale s's pair and its gradient live
    size_t pyr_at[MS_MAX_S + 1];
    pyr_at[0] = pyr_at[1] = 0;
    for (int s = 1; s < S; ++s) pyr_at[s + 1] = pyr_at[s] + (size_t)B * C * (H >> s) * (W >> s) * esz;
    char* buf[2] = {(char*)ws + (S > 1 ? (size_t)B * C * (H >> 1) * (W >> 1) * esz : 0), (char*)ws};   // even scales, odd scales
    const size_t lds = msg_lds_bytes(kh, kw);
    const bool k11 = kh == 11 && kw == 11;
    for (int s = S - 1; s >= 0; --s) {
        const int Hs = H >> s, Ws = W >> s;
        a.p = s ? (const char*)pyr_preds + pyr_at[s] : (const char*)preds;
        a.t = s ? (const char*)pyr_target + pyr_at[s] : (const char*)target;
        a.coarse = s + 1 < S ? buf[(s + 1) & 1] : nullptr;
        a.grad = s ? (void*)buf[s & 1] : grad_preds;
        a.w = w + (size_t)s * B;
        a.H = Hs, a.W = Ws, a.Ho = Hs - kh + 1, a.Wo = Ws - kw + 1;
        a.Hc = Hs >> 1, a.Wc = Ws >> 1;
        a.ntx = cdiv(Ws, MS_TW);
        a.tiles = (int)msg_tiles(Hs, Ws);
        a.cs_only = s < S - 1;
        const unsigned blocks = (unsigned)((int64_t)B * C * a.tiles);
        if (in_dtype == 0) {
            if (k11) msg_tile_kernel<float, 11><<<blocks, MS_THREADS, lds, st>>>(a);
            else msg_tile_kernel<float, 0><<<blocks, MS_THREADS, lds, st>>>(a);
        } else {
            if (k11) msg_tile_kernel<double, 11><<<blocks, MS_THREADS, lds, st>>>(a);
            else msg_tile_kernel<double, 0><<<blocks, MS_THREADS, lds, st>>>(a);
        }
    }
    OTVAE_CHECK_LAUNCH("otvae_ms_ssim_grad");
    return OTVAE_OK;
}
