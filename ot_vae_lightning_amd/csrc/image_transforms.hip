// Image transforms around the model (the package's transforms.py and utils/collage.py):
//   * otvae_gaussian_blur_fwd / _bwd -- torchvision.transforms.functional.gaussian_blur (the degradation of the reference's latent
//     transport experiments, tests/test_latent_transport.py:35) and its adjoint;
//   * otvae_collage -- Collage.list_to_collage (utils/collage.py:112-121): cat on width, clamp, make_grid(nrow=1), optionally the
//     uint8 HWC quantisation of torchvision.utils.save_image.
// No atomics, no host synchronisation, plain vector stores only: every entry can be captured into a hipGraph.
//
// The blur: one launch, no padded copy.  A workgroup of 256 threads owns a TH x TW tile of one *row space*:
//   NCHW                      a plane (n, c): rows of W floats, neighbouring pixels 1 float apart            (CI = 1)
//   channels-last             an image n: rows of W * C floats, neighbouring pixels of a channel C floats apart (CI = C) -- the rows
//                             are read and written as they lie in memory, 64 consecutive floats per wave, whatever C is
//   channels-last, wide halo  when (k / 2) * C columns of halo no longer fit LDS: a plane (n, c) again, pixels C floats apart in memory
// It stages the tile plus a halo of ky / 2 rows and (kx / 2) * CI columns in LDS -- the forward pass with the reflection applied to
// the global address, the backward pass with zeros outside the image --, runs the horizontal pass LDS -> LDS over all staged rows and
// the vertical pass LDS -> global.  Lanes walk consecutive columns in every phase: LDS reads and writes are conflict-free b32
// accesses, global accesses are coalesced.  The 1-D weights arrive in the kernel's argument block (read through scalar loads).
// Every output element is one fixed chain  w[0] * v0, fma(w[1], v1, .), ...  over the taps in index order, first along x then along
// y: its bits depend on the plane's values only -- not on the tile, the batch size or the plane's place in the batch.
//
// The adjoint (reflect padding p = k / 2 per axis, g extended by zeros):  G(m) = sum_t w[t] g[m + p - t]  for m in [-p, H-1+p], and
//   gx[i] = G(i) + [1 <= i <= p] G(-i) + [H-1-p <= i <= H-2] G(2 (H-1) - i).
// Every g a fold term reads lies within p of i (0 <= s <= p - i for the first, i - p <= .. <= H-1 for the second), i.e. inside the
// halo the main term needs anyway: the backward kernel is the forward kernel with a zero halo, flipped taps and the two folds added
// when a value leaves LDS.  A gather: no atomics, fixed order.
#include "common.h"

#define BLUR_MAX_K 31
#define BLUR_THREADS 256
#define BLUR_LDS_MAX (64 * 1024)

struct BlurArgs {
    const float* src;
    float* dst;
    int H, W, CI, RW;        // RW = W * CI: floats per row of the row space
    int cdiv;                // planes per outer block (C in the wide-halo channels-last mode, else 1)
    long long outer, inner;  // base of row space P = (P / cdiv) * outer + (P % cdiv) * inner
    long long row_stride;
    int col_stride;
    int kx, ky;
    int TW, TH, LW, LH;      // tile (TW a power of two), staged tile (LW = TW + 2 (kx/2) CI, LH = TH + 2 (ky/2))
    int tw_shift;            // log2 TW
    int tiles_x, tiles_y;
    float wx[BLUR_MAX_K], wy[BLUR_MAX_K];
};

// grid: planes * tiles_y * tiles_x workgroups (x fastest); dynamic LDS: LH * (LW + TW) floats
template <bool BWD>
__global__ __launch_bounds__(BLUR_THREADS) void blur_tile_kernel(const BlurArgs a) {
    extern __shared__ __attribute__((aligned(16))) float blur_lds[];
    float* s_in = blur_lds;                 // [LH][LW]
    float* s_mid = blur_lds + a.LH * a.LW;  // [LH][TW]
    const int tid = threadIdx.x;
    int b = blockIdx.x;
    const int tx = b % a.tiles_x;
    b /= a.tiles_x;
    const int ty = b % a.tiles_y;
    const int P = b / a.tiles_y;
    const long long base = (long long)(P / a.cdiv) * a.outer + (long long)(P % a.cdiv) * a.inner;
    const int H = a.H, W = a.W, CI = a.CI, RW = a.RW, LW = a.LW, LH = a.LH, TW = a.TW, TH = a.TH;
    const int kx = a.kx, ky = a.ky, px = kx >> 1, py = ky >> 1;
    const int j0 = tx * TW, y0 = ty * TH;
    const int jstart = j0 - px * CI, ystart = y0 - py;
    const float* __restrict__ src = a.src + base;

    // ---- stage the tile and its halo
    {
        const int total = LH * LW, dr = BLUR_THREADS / LW, dc = BLUR_THREADS % LW;
        int r = tid / LW, c = tid - r * LW;
        for (int i = tid; i < total; i += BLUR_THREADS) {
            int y = ystart + r, jj = jstart + c;
            bool ok;
            if (BWD) {
                ok = y >= 0 && y < H && jj >= 0 && jj < RW;
            } else {
                ok = y >= -py && y <= H - 1 + py && jj >= -px * CI && jj < RW + px * CI;
                if (ok) {
                    if (y < 0) y = -y;
                    else if (y > H - 1) y = 2 * (H - 1) - y;
                    if (jj < 0 || jj >= RW) {
                        int x = jj >= 0 ? jj / CI : -((-jj + CI - 1) / CI);   // floor
                        const int ch = jj - x * CI;
                        x = x < 0 ? -x : 2 * (W - 1) - x;
                        jj = x * CI + ch;
                    }
                }
            }
            s_in[i] = ok ? src[(long long)y * a.row_stride + (long long)jj * a.col_stride] : 0.f;
            c += dc;
            r += dr;
            if (c >= LW) {
                c -= LW;
                ++r;
            }
        }
    }
    __syncthreads();

    // ---- horizontal pass over every staged row: s_in -> s_mid
    {
        const int total = LH * TW;
        for (int i = tid; i < total; i += BLUR_THREADS) {
            const int r = i >> a.tw_shift, c = i & (TW - 1);
            const float* row = s_in + r * LW;
            float acc;
            if (!BWD) {
                acc = a.wx[0] * row[c];
                for (int t = 1; t < kx; ++t) acc = fmaf(a.wx[t], row[c + t * CI], acc);
            } else {
                acc = a.wx[0] * row[c + 2 * px * CI];
                for (int t = 1; t < kx; ++t) acc = fmaf(a.wx[t], row[c + (2 * px - t) * CI], acc);
                const int j = j0 + c;
                if (px > 0 && j < RW && (j < (px + 1) * CI || j >= (W - 1 - px) * CI)) {
                    const int x = j / CI, ch = j - x * CI;
#pragma unroll
                    for (int side = 0; side < 2; ++side) {
                        const bool on = side == 0 ? (x >= 1 && x <= px) : (x >= W - 1 - px && x <= W - 2);
                        if (!on) continue;
                        const int m = side == 0 ? -x : 2 * (W - 1) - x;
                        float f = 0.f;
                        for (int t = 0; t < kx; ++t) {
                            const int s = m + px - t;
                            const int lc = s * CI + ch - jstart;
                            if (s >= 0 && s < W && lc >= 0 && lc < LW) f = fmaf(a.wx[t], row[lc], f);
                        }
                        acc += f;
                    }
                }
            }
            s_mid[i] = acc;
        }
    }
    __syncthreads();

    // ---- vertical pass: s_mid -> global
    {
        float* __restrict__ dst = a.dst + base;
        const int total = TH * TW;
        for (int i = tid; i < total; i += BLUR_THREADS) {
            const int r = i >> a.tw_shift, c = i & (TW - 1);
            const int y = y0 + r, j = j0 + c;
            if (y >= H || j >= RW) continue;
            const float* col = s_mid + c;
            float acc;
            if (!BWD) {
                acc = a.wy[0] * col[r * TW];
                for (int t = 1; t < ky; ++t) acc = fmaf(a.wy[t], col[(r + t) * TW], acc);
            } else {
                acc = a.wy[0] * col[(r + 2 * py) * TW];
                for (int t = 1; t < ky; ++t) acc = fmaf(a.wy[t], col[(r + 2 * py - t) * TW], acc);
#pragma unroll
                for (int side = 0; side < 2; ++side) {
                    const bool on = side == 0 ? (y >= 1 && y <= py) : (y >= H - 1 - py && y <= H - 2);
                    if (!on) continue;
                    const int m = side == 0 ? -y : 2 * (H - 1) - y;
                    float f = 0.f;
                    for (int t = 0; t < ky; ++t) {
                        const int s = m + py - t;
                        const int lr = s - ystart;
                        if (s >= 0 && s < H && lr >= 0 && lr < LH) f = fmaf(a.wy[t], col[lr * TW], f);
                    }
                    acc += f;
                }
            }
            dst[(long long)y * a.row_stride + (long long)j * a.col_stride] = acc;
        }
    }
}

static size_t blur_lds_bytes(int TH, int TW, int CI, int kx, int ky) {
    const size_t LH = (size_t)TH + 2 * (ky / 2), LW = (size_t)TW + 2 * (size_t)(kx / 2) * CI;
    return LH * (LW + TW) * sizeof(float);
}

static int blur_launch(const char* who, bool bwd, const float* x, int N, int C, int H, int W, int channels_last, int kx, int ky,
                       const float* wx, const float* wy, float* y, void* stream) {
    OTVAE_REQUIRE(x && y && wx && wy, "%s: null pointer", who);
    OTVAE_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, "%s: empty tensor [%d][%d][%d][%d]", who, N, C, H, W);
    OTVAE_REQUIRE(kx > 0 && ky > 0 && (kx & 1) && (ky & 1), "%s: kernel sizes must be odd and positive, got (%d, %d)", who, kx, ky);
    OTVAE_REQUIRE(channels_last == 0 || channels_last == 1, "%s: channels_last must be 0 or 1", who);
    if (kx > BLUR_MAX_K || ky > BLUR_MAX_K) {
        otvae_set_error("%s: kernel size (%d, %d) beyond the supported %d per axis", who, kx, ky, BLUR_MAX_K);
        return OTVAE_EUNSUPPORTED;
    }
    if (kx / 2 >= W || ky / 2 >= H) {
        otvae_set_error("%s: reflect padding (%d, %d) must be smaller than the map %d x %d", who, kx / 2, ky / 2, H, W);
        return OTVAE_EUNSUPPORTED;
    }
    if ((int64_t)N * C * H * W >= ((int64_t)1 << 31)) {
        otvae_set_error("%s: %lld elements, the kernel indexes below 2^31", who, (long long)N * C * H * W);
        return OTVAE_EUNSUPPORTED;
    }
    BlurArgs a{};
    a.src = x;
    a.dst = y;
    a.H = H;
    a.W = W;
    a.kx = kx;
    a.ky = ky;
    a.TH = H <= 16 ? 16 : 32;
    int64_t planes;
    const bool cl = channels_last && C > 1;
    // channels-last rows are walked as they lie in memory when the (kx / 2) * C columns of halo fit LDS
    const bool interleaved = cl && blur_lds_bytes(a.TH, 64, C, kx, ky) <= BLUR_LDS_MAX;
    if (!cl) {
        a.CI = 1, a.cdiv = 1, a.outer = (long long)H * W, a.inner = 0, a.row_stride = W, a.col_stride = 1;
        planes = (int64_t)N * C;
    } else if (interleaved) {
        a.CI = C, a.cdiv = 1, a.outer = (long long)H * W * C, a.inner = 0, a.row_stride = (long long)W * C, a.col_stride = 1;
        planes = N;
    } else {
        a.CI = 1, a.cdiv = C, a.outer = (long long)H * W * C, a.inner = 1, a.row_stride = (long long)W * C, a.col_stride = C;
        planes = (int64_t)N * C;
    }
    a.RW = W * a.CI;
    a.TW = a.RW <= 32 ? 32 : 64;
    a.tw_shift = a.RW <= 32 ? 5 : 6;
    a.LW = a.TW + 2 * (kx / 2) * a.CI;
    a.LH = a.TH + 2 * (ky / 2);
    a.tiles_x = cdiv(a.RW, a.TW);
    a.tiles_y = cdiv(H, a.TH);
    const size_t lds = blur_lds_bytes(a.TH, a.TW, a.CI, kx, ky);
    const int64_t blocks = planes * a.tiles_x * a.tiles_y;
    if (lds > BLUR_LDS_MAX || blocks >= ((int64_t)1 << 31)) {
        otvae_set_error("%s: tile of %zu bytes / %lld workgroups is beyond the launch limits", who, lds, (long long)blocks);
        return OTVAE_EUNSUPPORTED;
    }
    for (int t = 0; t < kx; ++t) a.wx[t] = wx[t];
    for (int t = 0; t < ky; ++t) a.wy[t] = wy[t];
    if (bwd) blur_tile_kernel<true><<<(unsigned)blocks, BLUR_THREADS, lds, (hipStream_t)stream>>>(a);
    else blur_tile_kernel<false><<<(unsigned)blocks, BLUR_THREADS, lds, (hipStream_t)stream>>>(a);
    OTVAE_CHECK_LAUNCH(who);
    return OTVAE_OK;
}

extern "C" int otvae_gaussian_blur_fwd(const float* x, int N, int C, int H, int W, int channels_last, int kx, int ky,
                                       const float* wx, const float* wy, float* y, void* stream) {
    return blur_launch("otvae_gaussian_blur_fwd", false, x, N, C, H, W, channels_last, kx, ky, wx, wy, y, stream);
}

extern "C" int otvae_gaussian_blur_bwd(const float* gy, int N, int C, int H, int W, int channels_last, int kx, int ky,
                                       const float* wx, const float* wy, float* gx, void* stream) {
    return blur_launch("otvae_gaussian_blur_bwd", true, gy, N, C, H, W, channels_last, kx, ky, wx, wy, gx, stream);
}

// ================================================================================================ collage
#define COLLAGE_MAX 16
#define COLLAGE_PAD 2

struct CollageArgs {
    const float* src[COLLAGE_MAX];
    long long sn[COLLAGE_MAX], sc[COLLAGE_MAX], sy[COLLAGE_MAX], sx[COLLAGE_MAX];
    int w[COLLAGE_MAX], off[COLLAGE_MAX];
    int L, n, C, Cout, H, OH, OW, pad, as_u8;
    void* dst;
};

__device__ __forceinline__ void collage_store(const CollageArgs& a, int ch, int oy, int ox, float v) {
    if (a.as_u8) {
        float q = __fadd_rn(__fmul_rn(v, 255.f), 0.5f);   // save_image: mul(255).add_(0.5).clamp_(0, 255).to(uint8), two roundings
        q = q < 0.f ? 0.f : (q > 255.f ? 255.f : q);
        ((unsigned char*)a.dst)[((size_t)oy * a.OW + ox) * a.Cout + ch] = (unsigned char)q;
    } else {
        ((float*)a.dst)[((size_t)ch * a.OH + oy) * a.OW + ox] = v;
    }
}

// grid (blocks, L + 1): row l < L of the grid copies map l to its columns of every sample's band; row L writes the zero border and
// the padding bands between the samples (nothing when a single sample is laid out bare).
__global__ __launch_bounds__(256) void collage_kernel(const CollageArgs a) {
    const int l = blockIdx.y;
    const long long step = (long long)gridDim.x * 256;
    if (l == a.L) {
        if (!a.pad) return;
        const long long total = (long long)a.Cout * a.OH * a.OW;
        for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += step) {
            const int ox = (int)(e % a.OW);
            const long long q = e / a.OW;
            const int oy = (int)(q % a.OH), ch = (int)(q / a.OH);
            const int ry = (oy - a.pad) % (a.H + a.pad);
            const bool inside = oy >= a.pad && ry < a.H && ox >= a.pad && ox < a.OW - a.pad;
            if (!inside) collage_store(a, ch, oy, ox, 0.f);
        }
        return;
    }
    const float* __restrict__ src = a.src[l];
    const int w = a.w[l], off = a.off[l];
    const long long sn = a.sn[l], sc = a.sc[l], sy = a.sy[l], sx = a.sx[l];
    const long long total = (long long)a.n * a.Cout * a.H * w;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += step) {
        const int rx = (int)(e % w);
        long long q = e / w;
        const int ry = (int)(q % a.H);
        q /= a.H;
        const int ch = (int)(q % a.Cout), k = (int)(q / a.Cout);
        float v = src[k * sn + (a.C == 1 ? 0 : ch) * sc + ry * sy + rx * sx];
        v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);   // NaN stays NaN, as torch.clamp
        collage_store(a, ch, k * (a.H + a.pad) + a.pad + ry, a.pad + off + rx, v);
    }
}

extern "C" int otvae_collage(const float* const* maps, const int64_t* strides, const int* widths, int L, int n, int C, int H,
                             int as_uint8, void* out, void* stream) {
    OTVAE_REQUIRE(maps && strides && widths && out, "otvae_collage: null pointer");
    OTVAE_REQUIRE(n > 0 && C > 0 && H > 0 && L > 0, "otvae_collage: empty collage (L = %d, n = %d, C = %d, H = %d)", L, n, C, H);
    if (L > COLLAGE_MAX) {
        otvae_set_error("otvae_collage: %d maps, at most %d are laid out side by side", L, COLLAGE_MAX);
        return OTVAE_EUNSUPPORTED;
    }
    CollageArgs a{};
    int64_t wsum = 0, wmax = 0;
    for (int l = 0; l < L; ++l) {
        OTVAE_REQUIRE(maps[l] && widths[l] > 0, "otvae_collage: map %d is empty", l);
        a.src[l] = maps[l];
        a.sn[l] = strides[4 * l], a.sc[l] = strides[4 * l + 1], a.sy[l] = strides[4 * l + 2], a.sx[l] = strides[4 * l + 3];
        a.w[l] = widths[l];
        a.off[l] = (int)wsum;
        wsum += widths[l];
        wmax = widths[l] > wmax ? widths[l] : wmax;
    }
    a.L = L, a.n = n, a.C = C, a.Cout = C == 1 ? 3 : C, a.H = H, a.as_u8 = as_uint8 ? 1 : 0, a.dst = out;
    a.pad = n == 1 ? 0 : COLLAGE_PAD;   // make_grid returns a single image as it is
    const int64_t OH = (int64_t)n * (H + a.pad) + a.pad, OW = wsum + 2 * a.pad;
    if (OH * OW * a.Cout >= ((int64_t)1 << 31)) {
        otvae_set_error("otvae_collage: a %lld x %lld collage is beyond 2^31 elements", (long long)OH, (long long)OW);
        return OTVAE_EUNSUPPORTED;
    }
    a.OH = (int)OH, a.OW = (int)OW;
    const int64_t per_map = (int64_t)n * a.Cout * H * wmax;
    const int blocks = imax(1, imin(1024, cdiv(per_map, 256 * 4)));
    collage_kernel<<<dim3(blocks, L + 1), 256, 0, (hipStream_t)stream>>>(a);
    OTVAE_CHECK_LAUNCH("otvae_collage");
    return OTVAE_OK;
}
