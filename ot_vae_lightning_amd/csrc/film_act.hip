// FiLM conditioning fused with the layer's activation, and the Fourier features of the time embedding: what a class / time
// conditioned AutoEncoder (reference networks/cnn.py:540-591, nets_utils.py:22-52) puts on EVERY ConvLayer of the network.
//
//   forward    out = act(fmaf(x, scale[n][c], bias[n][c]))                                   one pass over the map
//   backward   v = fmaf(x, s, b);  ga = g * act'(v);  gx = ga * s;                           one pass over the map
//              gscale[n][c] = sum_hw ga * x;  gbias[n][c] = sum_hw ga
//
// x, out, g, gx: [N][HW][C] channels-last; scale, bias, gscale, gbias: [N][C].  The same fmaf and the same act_fwd / act_grad as
// otvae_film_fwd + otvae_bn_act_fwd (film_dropout2d.hip, activation.hip), which this pair replaces in functional._conv_layer_general:
// the forward result has the same bits.
//
// Thread layout (both directions): C % 4 == 0 -> a thread owns one float4 of channels (16-byte loads, a wave reads 1 KB of contiguous
// memory), else one channel.  With U such units per row (C / 4 or C) a workgroup is CW = min(U, 256) unit lanes x RW = 256 / CW row
// lanes: at C = 8 that is 2 x 128, every lane busy, consecutive lanes on consecutive addresses.
//
// Backward reduction: each thread adds its rows in fp64 in increasing row order, the RW row lanes of a unit are summed by a binary
// tree in LDS (fixed shape), and -- only when the batch alone cannot fill the chip -- the rows of a sample are cut into S chunks whose
// fp64 partials go through `ws` and are added in chunk order by a second small kernel of the same call.  No floating-point atomics
// anywhere: the result does not depend on scheduling, inside or outside a captured graph.
#include "common.h"

#include "act.h"

#define FA_THREADS 256
#define FA_TARGET_BLOCKS 1024   // workgroups wanted before the rows of a sample are worth cutting (256 CUs x 4)
#define FA_MIN_ROWS 64          // rows per chunk at least

template <int KIND, bool VEC>
__global__ __launch_bounds__(FA_THREADS) void film_act_fwd_kernel(const float* __restrict__ x, const float* __restrict__ s,
                                                                  const float* __restrict__ b, int HW, int C,
                                                                  float* __restrict__ out) {
    constexpr int W = VEC ? 4 : 1;
    const int U = C / W;                 // units per row
    const int per = HW * U;              // units per sample (HW * C < 2^31: checked by the launcher)
    const int n = blockIdx.y;
    const size_t base = (size_t)n * HW * C;
    const float* sn = s + (size_t)n * C;
    const float* bn = b + (size_t)n * C;
    for (int j = blockIdx.x * FA_THREADS + threadIdx.x; j < per; j += gridDim.x * FA_THREADS) {
        const int c = (j % U) * W;
        const size_t o = base + (size_t)j * W;
        if constexpr (VEC) {
            const f32x4 xv = *reinterpret_cast<const f32x4*>(x + o);
            const f32x4 sv = *reinterpret_cast<const f32x4*>(sn + c);
            const f32x4 bv = *reinterpret_cast<const f32x4*>(bn + c);
            f32x4 r;
#pragma unroll
            for (int k = 0; k < 4; ++k) r[k] = act_fwd(fmaf(xv[k], sv[k], bv[k]), KIND);
            *reinterpret_cast<f32x4*>(out + o) = r;
        } else {
            out[o] = act_fwd(fmaf(x[o], sn[c], bn[c]), KIND);
        }
    }
}

// (both kernels: blockIdx.y = the sample, N <= 65535)
// grid (S, N): block (chunk, n) owns rows [chunk * rpc, min(HW, (chunk + 1) * rpc)) of sample n.
// S == 1: gs / gb are written here; S > 1: part[((n * S + chunk) * 2 + {0: scale, 1: bias}) * C + c] (fp64) for film_act_bwd_sum_kernel.
// gs == NULL (the embedding takes no gradient): only gx.
template <int KIND, bool VEC>
__global__ __launch_bounds__(FA_THREADS) void film_act_bwd_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                                  const float* __restrict__ s, const float* __restrict__ b, int HW, int C,
                                                                  int rpc, float* __restrict__ gx, float* __restrict__ gs,
                                                                  float* __restrict__ gb, double* __restrict__ part) {
    constexpr int W = VEC ? 4 : 1;
    __shared__ double red[2 * W][FA_THREADS];
    const int n = blockIdx.y, chunk = blockIdx.x, S = gridDim.x;
    const int U = C / W;
    const int CW = U < FA_THREADS ? U : FA_THREADS;   // unit lanes
    const int RW = FA_THREADS / CW;                   // row lanes
    const int cq = threadIdx.x % CW, rq = threadIdx.x / CW;
    const int r0 = chunk * rpc;
    const int r1 = r0 + rpc < HW ? r0 + rpc : HW;
    const size_t base = (size_t)n * HW * C;
    for (int u0 = 0; u0 < U; u0 += CW) {   // one pass per group of 256 units (block-uniform trip count)
        const int c = (u0 + cq) * W;
        const bool live = u0 + cq < U && rq < RW;
        double a1[W], a2[W];                // sum ga * x, sum ga
#pragma unroll
        for (int k = 0; k < W; ++k) a1[k] = a2[k] = 0.0;
        if (live) {
            if constexpr (VEC) {
                const f32x4 sv = *reinterpret_cast<const f32x4*>(s + (size_t)n * C + c);
                const f32x4 bv = *reinterpret_cast<const f32x4*>(b + (size_t)n * C + c);
#pragma unroll 2
                for (int r = r0 + rq; r < r1; r += RW) {
                    const size_t o = base + (size_t)r * C + c;
                    const f32x4 xv = *reinterpret_cast<const f32x4*>(x + o);
                    const f32x4 gv = *reinterpret_cast<const f32x4*>(g + o);
                    f32x4 dx;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float ga = gv[k] * act_grad(fmaf(xv[k], sv[k], bv[k]), KIND);
                        dx[k] = ga * sv[k];
                        a1[k] += (double)ga * (double)xv[k];
                        a2[k] += (double)ga;
                    }
                    *reinterpret_cast<f32x4*>(gx + o) = dx;
                }
            } else {
                const float sc = s[(size_t)n * C + c], bc = b[(size_t)n * C + c];
#pragma unroll 2
                for (int r = r0 + rq; r < r1; r += RW) {
                    const size_t o = base + (size_t)r * C + c;
                    const float xv = x[o];
                    const float ga = g[o] * act_grad(fmaf(xv, sc, bc), KIND);
                    gx[o] = ga * sc;
                    a1[0] += (double)ga * (double)xv;
                    a2[0] += (double)ga;
                }
            }
        }
        if (gs) {   // kernel argument: block-uniform
            __syncthreads();   // (the previous group's readers are done with red)
#pragma unroll
            for (int k = 0; k < W; ++k) {
                red[k][threadIdx.x] = a1[k];
                red[W + k][threadIdx.x] = a2[k];
            }
            __syncthreads();
            int cnt = RW;      // row lanes still holding a partial sum
            int st = 1;
            while (st < RW) st <<= 1;
            for (st >>= 1; st > 0; st >>= 1) {   // binary tree over the row lanes: the same shape for every launch
                if (live && rq < st && rq + st < cnt) {
#pragma unroll
                    for (int k = 0; k < 2 * W; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + st * CW];
                }
                cnt = cnt < st ? cnt : st;
                __syncthreads();
            }
            if (live && rq == 0) {
#pragma unroll
                for (int k = 0; k < W; ++k) {
                    const double t1 = red[k][threadIdx.x], t2 = red[W + k][threadIdx.x];
                    if (S == 1) {
                        gs[(size_t)n * C + c + k] = (float)t1;
                        gb[(size_t)n * C + c + k] = (float)t2;
                    } else {
                        part[(((size_t)n * S + chunk) * 2 + 0) * C + c + k] = t1;
                        part[(((size_t)n * S + chunk) * 2 + 1) * C + c + k] = t2;
                    }
                }
            }
        }
    }
}

// gs / gb [n][c] = the S chunk partials added in chunk order
__global__ __launch_bounds__(FA_THREADS) void film_act_bwd_sum_kernel(const double* __restrict__ part, int N, int S, int C,
                                                                      float* __restrict__ gs, float* __restrict__ gb) {
    const int64_t total = (int64_t)N * C;
    for (int64_t i = blockIdx.x * (int64_t)FA_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * FA_THREADS) {
        const int64_t n = i / C;
        const int c = (int)(i % C);
        double t1 = 0.0, t2 = 0.0;
        for (int k = 0; k < S; ++k) {
            t1 += part[(((size_t)n * S + k) * 2 + 0) * C + c];
            t2 += part[(((size_t)n * S + k) * 2 + 1) * C + c];
        }
        gs[i] = (float)t1;
        gb[i] = (float)t2;
    }
}

// rows of a sample per workgroup: the whole sample once the batch fills the chip on its own
static inline int film_act_rows(int N, int HW) {
    const int want = cdiv(FA_TARGET_BLOCKS, N);   // chunks per sample that would fill the chip
    return imin(HW, imax(FA_MIN_ROWS, cdiv(HW, want)));
}

static inline bool film_act_shape_ok(int N, int HW, int C) {
    return N > 0 && N <= 65535 && HW > 0 && C > 0 && (int64_t)HW * C < ((int64_t)1 << 31);
}

#define FA_DISPATCH(KERNEL, kind, vec, ...)                                                    \
    do {                                                                                       \
        switch ((kind) * 2 + ((vec) ? 1 : 0)) {                                                \
            case 0: KERNEL<ACT_NONE, false> __VA_ARGS__; break;                                \
            case 1: KERNEL<ACT_NONE, true> __VA_ARGS__; break;                                 \
            case 2: KERNEL<ACT_RELU, false> __VA_ARGS__; break;                                \
            case 3: KERNEL<ACT_RELU, true> __VA_ARGS__; break;                                 \
            case 4: KERNEL<ACT_LEAKY, false> __VA_ARGS__; break;                               \
            case 5: KERNEL<ACT_LEAKY, true> __VA_ARGS__; break;                                \
            case 6: KERNEL<ACT_SELU, false> __VA_ARGS__; break;                                \
            case 7: KERNEL<ACT_SELU, true> __VA_ARGS__; break;                                 \
            case 8: KERNEL<ACT_GELU, false> __VA_ARGS__; break;                                \
            case 9: KERNEL<ACT_GELU, true> __VA_ARGS__; break;                                 \
            case 10: KERNEL<ACT_SILU, false> __VA_ARGS__; break;                               \
            default: KERNEL<ACT_SILU, true> __VA_ARGS__; break;                                \
        }                                                                                      \
    } while (0)

// 16-byte loads need 16-byte rows: C % 4 == 0 and aligned bases
static inline bool film_act_vec(int C, const void* a, const void* b, const void* c, const void* d, const void* e) {
    return C % 4 == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d | (uintptr_t)e) & 15) == 0;
}

extern "C" int otvae_film_act_fwd(const float* x, const float* scale, const float* bias, int N, int HW, int C, int act_kind, float* out,
                                  void* stream) {
    OTVAE_REQUIRE(x && scale && bias && out && film_act_shape_ok(N, HW, C), "otvae_film_act_fwd: bad argument");
    OTVAE_REQUIRE(act_kind >= ACT_NONE && act_kind <= ACT_SILU, "otvae_film_act_fwd: unknown activation %d", act_kind);
    const bool vec = film_act_vec(C, x, scale, bias, out, nullptr);
    const int per = HW * (vec ? C / 4 : C);
    const dim3 grid(imax(1, imin(cdiv(per, FA_THREADS), cdiv(4096, N))), N);   // grid-stride inside a sample beyond ~4096 blocks
    FA_DISPATCH(film_act_fwd_kernel, act_kind, vec, <<<grid, FA_THREADS, 0, (hipStream_t)stream>>>(x, scale, bias, HW, C, out));
    OTVAE_CHECK_LAUNCH("otvae_film_act_fwd");
    return OTVAE_OK;
}

extern "C" int64_t otvae_film_act_bwd_ws(int N, int HW, int C) {
    if (!film_act_shape_ok(N, HW, C)) return 0;
    const int S = cdiv(HW, film_act_rows(N, HW));
    return S > 1 ? (int64_t)N * S * 2 * C * (int64_t)sizeof(double) : 0;
}

extern "C" int otvae_film_act_bwd(const float* g, const float* x, const float* scale, const float* bias, int N, int HW, int C,
                                  int act_kind, float* gx, float* gscale, float* gbias, void* ws, void* stream) {
    OTVAE_REQUIRE(g && x && scale && bias && gx && film_act_shape_ok(N, HW, C), "otvae_film_act_bwd: bad argument");
    OTVAE_REQUIRE((gscale == nullptr) == (gbias == nullptr), "otvae_film_act_bwd: gscale and gbias come together");
    OTVAE_REQUIRE(act_kind >= ACT_NONE && act_kind <= ACT_SILU, "otvae_film_act_bwd: unknown activation %d", act_kind);
    const int rpc = film_act_rows(N, HW);
    const int S = cdiv(HW, rpc);
    OTVAE_REQUIRE(!(gscale && S > 1) || (ws && ((uintptr_t)ws & 7) == 0),
                  "otvae_film_act_bwd: this shape needs the workspace of otvae_film_act_bwd_ws (8-byte aligned)");
    const bool vec = film_act_vec(C, g, x, scale, bias, gx);
    double* part = (gscale && S > 1) ? (double*)ws : nullptr;
    FA_DISPATCH(film_act_bwd_kernel, act_kind, vec,
                <<<dim3(S, N), FA_THREADS, 0, (hipStream_t)stream>>>(g, x, scale, bias, HW, C, rpc, gx, gscale, gbias, part));
    OTVAE_CHECK_LAUNCH("otvae_film_act_bwd");
    if (part) {
        film_act_bwd_sum_kernel<<<imin(cdiv((int64_t)N * C, FA_THREADS), 1024), FA_THREADS, 0, (hipStream_t)stream>>>(part, N, S, C, gscale,
                                                                                                                 gbias);
        OTVAE_CHECK_LAUNCH("otvae_film_act_bwd (chunk sum)");
    }
    return OTVAE_OK;
}

// ---- Gaussian Fourier features of the time embedding (reference nets_utils.py:51-52) ------------------------------------------------
// out[n][j] = sin(p), out[n][half + j] = cos(p), p = ((t[n] * w[j]) * 2) * pi evaluated in fp32 in exactly that order (the reference
// writes `input.unsqueeze(-1) * self.weight * 2 * np.pi`; with scale = 30 the arguments reach hundreds of radians, where another
// association moves sin / cos by more than 1e-5).  The accurate sinf / cosf (full argument reduction), not the fast intrinsics.
__global__ __launch_bounds__(FA_THREADS) void fourier_features_kernel(const float* __restrict__ t, const float* __restrict__ w, int N,
                                                                      int half, float* __restrict__ out) {
    const int64_t total = (int64_t)N * half;
    for (int64_t i = blockIdx.x * (int64_t)FA_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * FA_THREADS) {
        const int64_t n = i / half;
        const int j = (int)(i % half);
        const float p = __fmul_rn(__fmul_rn(__fmul_rn(t[n], w[j]), 2.f), 3.14159265358979323846f);
        out[n * 2 * half + j] = sinf(p);
        out[n * 2 * half + half + j] = cosf(p);
    }
}

extern "C" int otvae_fourier_features(const float* t, const float* w, int N, int half, float* out, void* stream) {
    OTVAE_REQUIRE(t && w && out && N > 0 && half > 0, "otvae_fourier_features: bad argument");
    fourier_features_kernel<<<imin(cdiv((int64_t)N * half, FA_THREADS), 2048), FA_THREADS, 0, (hipStream_t)stream>>>(t, w, N, half, out);
    OTVAE_CHECK_LAUNCH("otvae_fourier_features");
    return OTVAE_OK;
}
