// The gradients of the per-image SSIM and multi-scale SSIM (losses.py's SSIMLoss / MSSSIMLoss; formulas, envelopes and arguments:
// include/otvae.h, otvae_ssim_grad / otvae_ms_ssim_grad).  One launch per scale, no atomics, no host read: every pixel of grad_preds is
// written by exactly one thread from sums in a fixed order, so the entries are run-to-run identical, depend for image b on image b,
// g[b] (and w_s[b]) alone and can be captured into a hipGraph.
//
//   ssg_tile_kernel   one workgroup per (image, channel, SS_TH x SS_TW tile of PIXELS).  The window positions whose window reaches
//   one of the tile's pixels form a (SS_TH + kh - 1) x (SS_TW + kw - 1) block (cut at the map's border); the workgroup recomputes
//   their moments itself rather than reading coefficient maps another launch left (the two-launch form costs 24 B per position of
//   extra traffic and a second launch; on a 32 x 32 plane, one tile, nothing is recomputed at all).
//     * stage   the p and t pixels under those positions (tile + 2 (k - 1) halo) go to LDS as fp32 DIFFERENCES dp, dt from the first
//               staged pixel, clamped first in range_mode 1 -- the forward kernel's staging (csrc/ssim.hip);
//     * moments horizontal pass (five row sums, kw taps) and vertical pass (kh taps), as in the forward;
//     * coefficients, in fp64 from the five fp32 moments, the pivots put back into the means.  S depends on p through mu_p, s_pp and
//               s_pt; with d mu the windowed mean of the differences,
//                   dS/dp_q = sum_u w(q - u) [ a'(u) + 2 dp_q b(u) + dt_q c(u) ],
//                   b = dS/ds_pp = -S / B2,  c = dS/ds_pt = 2 A1 / (B1 B2),
//                   a' = dS/dmu_p (at fixed variances) - 2 b dmu_p - c dmu_t,   dS/dmu_p = 2 mu_t A2 / (B1 B2) - 2 mu_p S / B1.
//               This is the header's alpha + 2 p beta + t gamma with p, t, E[pp], E[pt] all taken about the pivot: the same value,
//               without the cancellation between alpha and 2 p beta on narrow-range images.  a', b, c are scaled by g_b / n and
//               kept in registers over a barrier, then stored as fp32 over the (now dead) row sums;
//     * adjoint horizontal pass: th_q[r][x] = sum_j ww[j] coef_q[r][x - j] for the tile's SS_TW pixel columns;
//     * adjoint vertical pass and the pixel: alpha', beta, gamma = sum_i wh[i] th[y - i][x]; grad = alpha' + 2 dp beta + dt gamma in
//               fp64, 0 where range_mode 1 clamped the pixel (strictly outside [lo, hi]: torch.clamp's rule), cast to the input's type.
//   Positions outside the map and pixels outside the image are skipped by the loop bounds and index guards, never read.
//   ssg_tile_kernel<.., MS = true> is the multi-scale form, launched per scale from the coarsest to the finest: the scale's weight
//   g[b] w_s[b] / n_s in front of the coefficients, the cs coefficients (dS/dmu = 0, b = -cs / B2, c = 2 / B2) or the ssim ones by a
//   flag, and 1/4 of the coarser scale's gradient added at the store.  Every element is written.
// LDS per workgroup: 4 (2 SR SC + max(5 SR PC, 3 PR (PC + SS_TW))) bytes with SR = 16 + 2 (kh - 1), SC = 32 + 2 (kw - 1), PR = 15 + kh,
// PC = 31 + kw: 44.2 KiB for the 11 x 11 window (3 workgroups per CU), 60.2 KiB at the envelope's 15 x 15 (2 per CU) -- inside the
// 64 KiB a launch gets without asking.  The staging maps a lane to a staged column, so SC <= 64 as well: 15 taps per axis.
#include "ssim_common.h"

extern "C" int64_t otvae_ssim_grad_ws(int B, int C, int H, int W, int kh, int kw) {
    if (!ssim_args_ok(B, C, H, W, kh, kw) || !ssim_grad_supported(B, C, H, W, kh, kw)) return -1;
    return 0;   // the one-launch form keeps everything in LDS
}

extern "C" int64_t otvae_ms_ssim_grad_ws(int in_dtype, int B, int C, int H, int W, int kh, int kw, int S) {
    if ((in_dtype != 0 && in_dtype != 1) || !ssim_args_ok(B, C, H, W, kh, kw, S) || !ms_ssim_supported(B, C, H, W, kh, kw, S, SS_MAX_KG))
        return -1;
    // the gradients of scales 1 .. S - 1 alternate between two buffers: odd scales in the first, even ones in the second
    const int64_t n1 = S > 1 ? ssim_scale_elems(B, C, H, W, 1) : 0, n2 = S > 2 ? ssim_scale_elems(B, C, H, W, 2) : 0;
    return (n1 + n2) * (in_dtype == 0 ? 4 : 8);
}

struct SsimGradArgs {
    const void* p;
    const void* t;
    const void* coarse;    // MS: the next coarser scale's gradient [planes][Hc][Wc]; NULL at the last scale
    void* grad;
    const double* g;       // [B] upstream
    const double* w;       // MS: [B] d msssim_b / d v_s[b] of this scale
    int C, H, W, kh, kw;
    int Ho, Wo, ntx, tiles;
    int Hc, Wc;            // MS
    int mode, cs_only;     // cs_only: MS
    double lo, hi, k1, k2;
    float wh[SS_MAX_KG], ww[SS_MAX_KG];
};

static size_t sg_lds_bytes(int kh, int kw) {
    const size_t SR = SS_TH + 2 * (kh - 1), SC = SS_TW + 2 * (kw - 1), PR = SS_TH + kh - 1, PC = SS_TW + kw - 1;
    const size_t sums = 5 * SR * PC, coef = 3 * PR * (PC + SS_TW);
    return (2 * SR * SC + (sums > coef ? sums : coef)) * sizeof(float);
}

// K > 0: a K x K window known at compile time (the default 11 x 11): every tap loop and every index division has constant bounds.
// K == 0: window sizes from the arguments.  MS: one scale of the multi-scale gradient.
template <typename TIN, int K, bool MS>
__global__ __launch_bounds__(SS_THREADS) void ssg_tile_kernel(const SsimGradArgs a) {
    extern __shared__ __attribute__((aligned(16))) char sg_smem[];
    const int kh = K ? K : a.kh, kw = K ? K : a.kw;
    const int SR = SS_TH + 2 * (kh - 1), SC = SS_TW + 2 * (kw - 1);   // staged pixels at most
    const int PR = SS_TH + kh - 1, PC = SS_TW + kw - 1;               // positions at most
    float* sp = reinterpret_cast<float*>(sg_smem);   // [SR][SC] p - pivot
    float* st = sp + SR * SC;                        // [SR][SC] t - pivot
    float* hq = st + SR * SC;                        // [5][SR][PC] row sums; later:
    float* cf = hq;                                  // [3][PR][PC] coefficients
    float* th = cf + 3 * PR * PC;                    // [3][PR][SS_TW] their horizontal adjoint
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    const unsigned plane = blockIdx.x / (unsigned)a.tiles, tile = blockIdx.x % (unsigned)a.tiles;
    const int y0 = (int)(tile / (unsigned)a.ntx) * SS_TH, x0 = (int)(tile % (unsigned)a.ntx) * SS_TW;
    const int ph = min(SS_TH, a.H - y0), pw = min(SS_TW, a.W - x0);                 // pixels of this tile, >= 1 each
    const int ur0 = max(0, y0 - kh + 1), uc0 = max(0, x0 - kw + 1);                  // first position that reaches the tile
    const int npr = min(a.Ho - 1, y0 + ph - 1) - ur0 + 1, npc = min(a.Wo - 1, x0 + pw - 1) - uc0 + 1;   // positions, 1 .. PR / PC
    const int rows = npr + kh - 1, cols = npc + kw - 1;                              // staged pixels: ur0 + rows <= H, uc0 + cols <= W

    const double R = a.hi - a.lo;
    const double c1 = (a.k1 * R) * (a.k1 * R), c2 = (a.k2 * R) * (a.k2 * R);
    const unsigned img = plane / (unsigned)a.C;
    double gscale;
    if constexpr (MS) gscale = a.g[img] * a.w[img] / ((double)a.C * a.Ho * a.Wo);
    else gscale = a.g[img] / ((double)a.C * a.Ho * a.Wo);
    const bool cs_only = MS && a.cs_only != 0;

    const size_t plane_at = (size_t)plane * a.H * a.W;
    const TIN* __restrict__ pp = static_cast<const TIN*>(a.p) + plane_at + (size_t)ur0 * a.W + uc0;
    const TIN* __restrict__ tt = static_cast<const TIN*>(a.t) + plane_at + (size_t)ur0 * a.W + uc0;
    const bool clamp = a.mode == 1;
    const TIN lo = (TIN)a.lo, hi = (TIN)a.hi;
    TIN piv_p = pp[0], piv_t = tt[0];
    if (clamp) piv_p = ssim_clamp(piv_p, lo, hi), piv_t = ssim_clamp(piv_t, lo, hi);

    // stage: wave w takes rows w, w + 4, ...; lane = column (SC <= 64).  All loads are issued before the first is used; threads past
    // the staged block load its last row / column again (an address inside the image) and store nothing.
    constexpr int NST = (SS_TH + 2 * ((K ? K : SS_MAX_KG) - 1) + 3) / 4;
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
                if (clamp) x = ssim_clamp(x, lo, hi), y = ssim_clamp(y, lo, hi);
                sp[r * SC + lane] = (float)(x - piv_p);
                st[r * SC + lane] = (float)(y - piv_t);
            }
        }
    }
    __syncthreads();

    // horizontal pass: (staged row r, position column c) -> five row sums
    for (int idx = tid; idx < rows * PC; idx += SS_THREADS) {
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
    constexpr int PMAX = SS_TH + (K ? K : SS_MAX_KG) - 1, QMAX = SS_TW + (K ? K : SS_MAX_KG) - 1;
    constexpr int NPOS = (PMAX * QMAX + SS_THREADS - 1) / SS_THREADS;
    float co[NPOS][3];
#pragma unroll
    for (int u = 0; u < NPOS; ++u) {
        const int idx = tid + u * SS_THREADS;
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
        const int idx = tid + u * SS_THREADS;
        const int r = idx / PC, c = idx - r * PC;
        if (r < npr && c < npc) {
#pragma unroll
            for (int q = 0; q < 3; ++q) cf[(q * PR + r) * PC + c] = co[u][q];
        }
    }
    __syncthreads();

    // adjoint horizontal pass: (position row r, pixel column x) <- the positions uc0 + cl with x0 + x - kw + 1 <= uc0 + cl <= x0 + x
    const int xoff = x0 - uc0;
    for (int idx = tid; idx < npr * SS_TW; idx += SS_THREADS) {
        const int r = idx / SS_TW, x = idx % SS_TW;
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
            float* o = th + r * SS_TW + x;
            o[0] = s0;
            o[PR * SS_TW] = s1;
            o[2 * PR * SS_TW] = s2;
        }
    }
    __syncthreads();

    // adjoint vertical pass and the pixel: the own-scale term (0 where range_mode 1 clamped the pixel), plus (MS) a quarter of the
    // coarser scale's gradient at the pooled pixel above it (none above a dropped odd row / column)
    const int yoff = y0 - ur0;
    TIN* __restrict__ gout = static_cast<TIN*>(a.grad) + plane_at;
    const TIN* __restrict__ praw = static_cast<const TIN*>(a.p) + plane_at;
    const TIN* __restrict__ gc = MS && a.coarse ? static_cast<const TIN*>(a.coarse) + (size_t)plane * a.Hc * a.Wc : nullptr;
    for (int idx = tid; idx < ph * SS_TW; idx += SS_THREADS) {
        const int y = idx / SS_TW, x = idx % SS_TW;
        if (x < pw) {
            float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int i = 0; i < kh; ++i) {
                const int rl = yoff + y - i;
                if ((unsigned)rl < (unsigned)npr) {
                    const float w = a.wh[i];
                    const float* __restrict__ v = th + rl * SS_TW + x;
                    s0 = fmaf(w, v[0], s0);
                    s1 = fmaf(w, v[PR * SS_TW], s1);
                    s2 = fmaf(w, v[2 * PR * SS_TW], s2);
                }
            }
            const int at = (yoff + y) * SC + xoff + x;
            double grad = (double)s0 + 2.0 * (double)sp[at] * (double)s1 + (double)st[at] * (double)s2;
            const size_t q = (size_t)(y0 + y) * a.W + x0 + x;
            if (clamp) {
                const TIN raw = praw[q];
                if (raw < lo || raw > hi) grad = 0.0;
            }
            if constexpr (MS) {
                const int yc = (y0 + y) >> 1, xc = (x0 + x) >> 1;
                if (gc && yc < a.Hc && xc < a.Wc) grad += 0.25 * (double)gc[(size_t)yc * a.Wc + xc];
            }
            gout[q] = (TIN)grad;
        }
    }
}

// what both entries put into the args once, and one [B][C][H][W] launch
static void sg_args_window(SsimGradArgs& a, int C, int kh, int kw, const double* wh, const double* ww, double k1, double k2,
                           int range_mode, double range_lo, double range_hi, const double* g) {
    a.g = g;
    a.C = C, a.kh = kh, a.kw = kw;
    a.mode = range_mode;
    a.lo = range_lo, a.hi = range_hi;
    a.k1 = k1, a.k2 = k2;
    ssim_fill_window(a.wh, a.ww, wh, ww, kh, kw);
    a.coarse = nullptr, a.w = nullptr, a.Hc = a.Wc = a.cs_only = 0;
}

template <bool MS>
static void sg_launch(SsimGradArgs& a, int in_dtype, int B, int H, int W, hipStream_t st) {
    a.H = H, a.W = W, a.Ho = H - a.kh + 1, a.Wo = W - a.kw + 1;
    a.ntx = cdiv(W, SS_TW);
    a.tiles = (int)ssim_grad_tiles(H, W);
    const unsigned blocks = (unsigned)((int64_t)B * a.C * a.tiles);
    const size_t lds = sg_lds_bytes(a.kh, a.kw);
    const bool k11 = a.kh == 11 && a.kw == 11;   // the default window: the unrolled instantiation
    if (in_dtype == 0) {
        if (k11) ssg_tile_kernel<float, 11, MS><<<blocks, SS_THREADS, lds, st>>>(a);
        else ssg_tile_kernel<float, 0, MS><<<blocks, SS_THREADS, lds, st>>>(a);
    } else {
        if (k11) ssg_tile_kernel<double, 11, MS><<<blocks, SS_THREADS, lds, st>>>(a);
        else ssg_tile_kernel<double, 0, MS><<<blocks, SS_THREADS, lds, st>>>(a);
    }
}

extern "C" int otvae_ssim_grad(int in_dtype, const void* preds, const void* target, int B, int C, int H, int W, int kh, int kw,
                               const double* wh, const double* ww, double k1, double k2, int range_mode, double range_lo, double range_hi,
                               const double* g, void* grad_preds, void* ws, void* stream) {
    (void)ws;
    OTVAE_REQUIRE(preds && target && wh && ww && g && grad_preds, "otvae_ssim_grad: null argument");
    OTVAE_REQUIRE(in_dtype == 0 || in_dtype == 1, "otvae_ssim_grad: in_dtype must be 0 (fp32) or 1 (fp64)");
    OTVAE_REQUIRE(ssim_args_ok(B, C, H, W, kh, kw),
                  "otvae_ssim_grad: need B, C >= 1, odd windows and H >= kh, W >= kw (got B %d, C %d, %d x %d images, %d x %d window)", B, C,
                  H, W, kh, kw);
    OTVAE_REQUIRE(range_mode == 0 || range_mode == 1,
                  "otvae_ssim_grad: range_mode must be 0 or 1 (got %d): a range taken from the batch depends on the data, a loss needs a "
                  "fixed scale", range_mode);
    OTVAE_REQUIRE(range_hi > range_lo, "otvae_ssim_grad: range_hi must exceed range_lo");
    OTVAE_REQUIRE(k1 >= 0.0 && k2 >= 0.0, "otvae_ssim_grad: k1 and k2 must not be negative");
    if (!ssim_grad_supported(B, C, H, W, kh, kw)) {
        otvae_set_error("otvae_ssim_grad: a %d x %d window on %d x %d x %d x %d is beyond the envelope (%d taps per axis, 2^31 tiles)", kh,
                        kw, B, C, H, W, SS_MAX_KG);
        return OTVAE_EUNSUPPORTED;
    }
    SsimGradArgs a;
    sg_args_window(a, C, kh, kw, wh, ww, k1, k2, range_mode, range_lo, range_hi, g);
    a.p = preds, a.t = target, a.grad = grad_preds;
    sg_launch<false>(a, in_dtype, B, H, W, (hipStream_t)stream);
    OTVAE_CHECK_LAUNCH("otvae_ssim_grad");
    return OTVAE_OK;
}

extern "C" int otvae_ms_ssim_grad(int in_dtype, const void* preds, const void* target, const void* pyr_preds, const void* pyr_target,
                                  int B, int C, int H, int W, int kh, int kw, const double* wh, const double* ww, double k1, double k2,
                                  int range_mode, double range_lo, double range_hi, int S, const double* g, const double* w,
                                  void* grad_preds, void* ws, void* stream) {
    OTVAE_REQUIRE(preds && target && wh && ww && g && w && grad_preds, "otvae_ms_ssim_grad: null argument");
    OTVAE_REQUIRE(in_dtype == 0 || in_dtype == 1, "otvae_ms_ssim_grad: in_dtype must be 0 (fp32) or 1 (fp64)");
    OTVAE_REQUIRE(ssim_args_ok(B, C, H, W, kh, kw, S),
                  "otvae_ms_ssim_grad: need B, C, S >= 1, odd windows and H >> (S - 1) >= kh, W >> (S - 1) >= kw (got B %d, C %d, %d x %d "
                  "images, %d x %d window, %d scales)", B, C, H, W, kh, kw, S);
    OTVAE_REQUIRE(S == 1 || (pyr_preds && pyr_target && ws), "otvae_ms_ssim_grad: more than one scale needs the two pyramids and ws");
    OTVAE_REQUIRE(range_mode == 0 || range_mode == 1,
                  "otvae_ms_ssim_grad: range_mode must be 0 or 1 (got %d): a range taken from the batch depends on the data, a loss needs "
                  "a fixed scale", range_mode);
    OTVAE_REQUIRE(range_hi > range_lo, "otvae_ms_ssim_grad: range_hi must exceed range_lo");
    OTVAE_REQUIRE(k1 >= 0.0 && k2 >= 0.0, "otvae_ms_ssim_grad: k1 and k2 must not be negative");
    if (!ms_ssim_supported(B, C, H, W, kh, kw, S, SS_MAX_KG)) {
        otvae_set_error("otvae_ms_ssim_grad: %d scales of a %d x %d window on %d x %d x %d x %d are beyond the envelope (%d scales, %d "
                        "taps per axis, 2^31 tiles)", S, kh, kw, B, C, H, W, SS_MAX_S, SS_MAX_KG);
        return OTVAE_EUNSUPPORTED;
    }
    const size_t esz = in_dtype == 0 ? 4 : 8;
    SsimGradArgs a;
    sg_args_window(a, C, kh, kw, wh, ww, k1, k2, range_mode, range_lo, range_hi, g);
    // the gradients of scales 1 .. S - 1: even scales behind the odd ones
    char* buf[2] = {(char*)ws + (S > 1 ? (size_t)ssim_scale_elems(B, C, H, W, 1) * esz : 0), (char*)ws};
    for (int s = S - 1; s >= 0; --s) {
        const size_t pyr_at = (size_t)ssim_pyramid_elems(B, C, H, W, s) * esz;   // where scale s's pair begins in a pyramid
        a.p = s ? (const char*)pyr_preds + pyr_at : (const char*)preds;
        a.t = s ? (const char*)pyr_target + pyr_at : (const char*)target;
        a.coarse = s + 1 < S ? buf[(s + 1) & 1] : nullptr;
        a.grad = s ? (void*)buf[s & 1] : grad_preds;
        a.w = w + (size_t)s * B;
        a.Hc = H >> (s + 1), a.Wc = W >> (s + 1);
        a.cs_only = s < S - 1;
        sg_launch<true>(a, in_dtype, B, H >> s, W >> s, (hipStream_t)stream);
    }
    OTVAE_CHECK_LAUNCH("otvae_ms_ssim_grad");
    return OTVAE_OK;
}
