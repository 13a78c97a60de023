// ConvLayer kernels for the few layers whose channel counts are tiny (1, 3 or <= 8 on both sides): the image-side
// layers of the CNN (first encoder block: 1 -> 8 channels at 32x32; last decoder block: 8 -> 1, 1 -> 1, 1 -> 3 at 32x32).
// There an MFMA tile would be >= 75 % padding and the LDS-staged gather cannot use vector loads, so these layers --
// the highest-resolution, purely HBM-bound ones -- run as direct VALU convolutions: one lane per output position,
// weights broadcast from LDS, same fused prologue (BatchNorm-apply, ReLU, nearest up-sampling, zero padding) and
// epilogues (bias, residual; ReLU mask + BatchNorm-backward sums in fp64) as the implicit-GEMM kernels in conv.hip.
// Reference arithmetic: networks/cnn.py:183-192 and its autograd backward.
#include "common.h"
#include "conv_small.h"
#include <type_traits>

#define SMALL_MAXC 16
// The weights stay in LDS: left alone the compiler hoists the (loop-invariant) LDS weight reads of the unrolled tap loops
// out of the position loop into 130-330 registers, which costs the occupancy these latency-bound kernels live on.
#define SMALL_REREAD_LDS() asm volatile("" ::: "memory")
#define SMALL_OCC
#define SMALL_MAXW 1024

bool conv_small_ok(const SmallGeom& g) {
    if (g.KH * g.KW * g.Cs * g.Cn > SMALL_MAXW) return false;
    if (g.Cs <= 8 && g.Cn <= 8) return !((g.Cs % 4 == 0) && (g.Cn % 4 == 0));  // those the vectorised MFMA path handles well
    // the RGB image-side layers of the capacity-16 (CIFAR) network: 3 -> 16, 16 -> 3, 3 -> 9 (qkv); otherwise they fall to
    // the scalar-gather implicit GEMM (3 channels cannot be loaded as float4)
    return (g.Cs == 3 && (g.Cn == 16 || g.Cn == 9)) || (g.Cs == 16 && g.Cn == 3);
}

// (image, y, x) of a flat position index: one multiply per division while the index is below 2^22 (see fast_div in
// conv.hip), the udiv expansion (~25 instructions each, a third of a 1-channel layer's per-pixel work) otherwise
__device__ __forceinline__ unsigned sdiv(unsigned k, unsigned d, float inv_d, bool small) {
    return small ? (unsigned)(int)(((float)(int)k + 0.5f) * inv_d) : k / d;
}

__device__ __forceinline__ float act1(float v, float sc, float sh, bool affine, int relu) {
    if (affine) v = fmaf(v, sc, sh);
    if (relu) v = fmaxf(v, 0.f);
    return v;
}

// ------------------------------------------------------------------------------------------------ forward
// CS / CN > 0: channel counts known at compile time (inner loops fully unrolled, channel vectors loaded as one 16/32-byte
// access); 0: read from the geometry (any Cs, Cn <= SMALL_MAXC).
template <int C>
__device__ __forceinline__ void load_chan(const float* __restrict__ p, float (&v)[C ? C : SMALL_MAXC], int n) {
    if constexpr (C == 16) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 a = reinterpret_cast<const float4*>(p)[q];
            v[4 * q] = a.x; v[4 * q + 1] = a.y; v[4 * q + 2] = a.z; v[4 * q + 3] = a.w;
        }
    } else if constexpr (C == 8) {
        const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else if constexpr (C == 4) {
        const float4 a = *reinterpret_cast<const float4*>(p);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    } else if constexpr (C > 0) {
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = p[c];
    } else {
#pragma unroll
        for (int c = 0; c < SMALL_MAXC; ++c) v[c] = c < n ? p[c] : 0.f;
    }
}

template <int C>
__device__ __forceinline__ void store_chan(float* __restrict__ p, const float (&v)[C ? C : SMALL_MAXC], int n) {
    if constexpr (C == 16) {
#pragma unroll
        for (int q = 0; q < 4; ++q) reinterpret_cast<float4*>(p)[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
    } else if constexpr (C == 8) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
    } else if constexpr (C == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else if constexpr (C > 0) {
#pragma unroll
        for (int c = 0; c < C; ++c) p[c] = v[c];
    } else {
#pragma unroll
        for (int c = 0; c < SMALL_MAXC; ++c)
            if (c < n) p[c] = v[c];
    }
}

// KS > 0 (with CS, CN > 0): square KS x KS kernel known at compile time.  The taps' loads are then issued back to back
// from clamped (always valid) addresses and masked afterwards; the generic tap loop below branches around out-of-image
// taps, which makes every tap's load wait for the previous tap's arithmetic (9-16 exposed L2 latencies per position:
// the layers at 32x32 ran at 0.7-1.7 TB/s).
struct SmallFwdSmem {
    float w[SMALL_MAXW];  // [tap][c][CNM]  (row padded to CNM when CN is generic)
    double red[4][2][SMALL_MAXC];
    float sc[SMALL_MAXC], sh[SMALL_MAXC], b[SMALL_MAXC];
};

// The body of workgroup `vb` of `nb`: blockIdx.x / gridDim.x in the one-job kernel, the job-local values in the two-job kernel.
template <int CS, int CN, int KS>
__device__ __forceinline__ void conv_small_fwd_body(const SmallGeom& g, const float* __restrict__ x,
                                                    const float* __restrict__ scale, const float* __restrict__ shift,
                                                    int relu, const float* __restrict__ wT,
                                                    const float* __restrict__ bias, const float* __restrict__ res,
                                                    float* __restrict__ y, double* __restrict__ partial, int CnPad,
                                                    const BnFold& fold, SmallFwdSmem& sm, unsigned vb, unsigned nb) {
    float* const w_s = sm.w;
    double(*const redf)[2][SMALL_MAXC] = sm.red;
    float *const sc_s = sm.sc, *const sh_s = sm.sh, *const b_s = sm.b;
#define SMALL_VB vb
#define SMALL_NB nb
#include "conv_small_fwd_body.h"
#undef SMALL_VB
#undef SMALL_NB
}

template <int CS, int CN, int KS>
__global__ __launch_bounds__(256) SMALL_OCC void conv_small_fwd_kernel(SmallGeom g, const float* __restrict__ x,
                                                             const float* __restrict__ scale, const float* __restrict__ shift,
                                                             int relu, const float* __restrict__ wT,
                                                             const float* __restrict__ bias, const float* __restrict__ res,
                                                             float* __restrict__ y, double* __restrict__ partial, int CnPad,
                                                             BnFold fold) {
    __shared__ __align__(16) float w_s[SMALL_MAXW];  // [tap][c][CNM]  (row padded to CNM when CN is generic)
    __shared__ double redf[4][2][SMALL_MAXC];
    __shared__ float sc_s[SMALL_MAXC], sh_s[SMALL_MAXC], b_s[SMALL_MAXC];
#define SMALL_VB blockIdx.x
#define SMALL_NB gridDim.x
#include "conv_small_fwd_body.h"
#undef SMALL_VB
#undef SMALL_NB
}

// Two independent forward jobs (the two branches of a ConvBlock head) in ONE launch: job 0's workgroups, then job 1's; each runs its
// own job's body -- unchanged -- with its job-local block index and block count.  Two equal bodies are one body called with the
// selected job's arguments; two different bodies sit in the two arms of a branch.
template <int CS0, int CN0, int KS0, int CS1, int CN1, int KS1>
__global__ __launch_bounds__(256) SMALL_OCC void conv_small_fwd_pair_kernel(SmallFwdArgs a, SmallFwdArgs b) {
    __shared__ __align__(16) SmallFwdSmem sm;
    if constexpr (CS0 == CS1 && CN0 == CN1 && KS0 == KS1) {
        // one body serves both jobs: select the job's arguments (a uniform address into the kernel arguments), not the code
        const bool second = blockIdx.x >= (unsigned)a.nblocks;
        const SmallFwdArgs& j = second ? b : a;
        conv_small_fwd_body<CS0, CN0, KS0>(j.g, j.x, j.scale, j.shift, j.relu, j.wT, j.bias, j.res, j.y, j.partial, j.CnPad, j.fold, sm,
                                           blockIdx.x - (second ? a.nblocks : 0), j.nblocks);
    } else if (blockIdx.x < (unsigned)a.nblocks) {
        conv_small_fwd_body<CS0, CN0, KS0>(a.g, a.x, a.scale, a.shift, a.relu, a.wT, a.bias, a.res, a.y, a.partial, a.CnPad, a.fold, sm,
                                           blockIdx.x, a.nblocks);
    } else {
        conv_small_fwd_body<CS1, CN1, KS1>(b.g, b.x, b.scale, b.shift, b.relu, b.wT, b.bias, b.res, b.y, b.partial, b.CnPad, b.fold, sm,
                                           blockIdx.x - a.nblocks, b.nblocks);
    }
}

// channel-count specialisations: the MNIST (1 <-> 8, 1 -> 1, 1 -> 3) and RGB (3 <-> 8, 3 -> 3) image-side layers
#define SMALL_DISPATCH(KERNEL, ...)                                            \
    do {                                                                       \
        if (g.Cs == 1 && g.Cn == 8) KERNEL<1, 8, 0> __VA_ARGS__;               \
        else if (g.Cs == 8 && g.Cn == 1) KERNEL<8, 1, 0> __VA_ARGS__;          \
        else if (g.Cs == 1 && g.Cn == 1) KERNEL<1, 1, 0> __VA_ARGS__;          \
        else if (g.Cs == 1 && g.Cn == 3) KERNEL<1, 3, 0> __VA_ARGS__;          \
        else if (g.Cs == 3 && g.Cn == 8) KERNEL<3, 8, 0> __VA_ARGS__;          \
        else if (g.Cs == 8 && g.Cn == 3) KERNEL<8, 3, 0> __VA_ARGS__;          \
        else if (g.Cs == 3 && g.Cn == 3) KERNEL<3, 3, 0> __VA_ARGS__;          \
        else if (g.Cs == 3 && g.Cn == 16) KERNEL<3, 16, 0> __VA_ARGS__;        \
        else if (g.Cs == 16 && g.Cn == 3) KERNEL<16, 3, 0> __VA_ARGS__;        \
        else if (g.Cs == 3 && g.Cn == 9) KERNEL<3, 9, 0> __VA_ARGS__;          \
        else KERNEL<0, 0, 0> __VA_ARGS__;                                      \
    } while (0)
// (Cs, Cn, kernel size) of the layers the two configurations really have: tap loops unrolled, loads up front
#define SMALL_KS_CASES(X) \
    X(1, 8, 4) X(8, 1, 3) X(8, 1, 1) X(1, 1, 3) X(1, 1, 1) X(1, 3, 1) X(3, 3, 3) X(3, 3, 1) X(3, 16, 4) X(16, 3, 3) X(16, 3, 1) X(3, 9, 1)

int conv_small_fwd(const SmallGeom& g, int nblocks, const float* x, const float* scale, const float* shift, int relu,
                   const float* wT, const float* bias, const float* res, float* y, double* partial, int CnPad,
                   const BnFold& fold, hipStream_t st) {
#define X(CS_, CN_, KS_)                                                                                          \
    if (g.Cs == CS_ && g.Cn == CN_ && g.KH == KS_ && g.KW == KS_) {                                               \
        conv_small_fwd_kernel<CS_, CN_, KS_><<<nblocks, 256, 0, st>>>(g, x, scale, shift, relu, wT, bias, res, y, partial, \
                                                                       CnPad, fold);                              \
        return 0;                                                                                                 \
    }
    SMALL_KS_CASES(X)
#undef X
    SMALL_DISPATCH(conv_small_fwd_kernel, <<<nblocks, 256, 0, st>>>(g, x, scale, shift, relu, wT, bias, res, y, partial, CnPad, fold));
    return 0;
}

// ------------------------------------------------------------------------------------------------ data gradient
// one lane per SOURCE position (parent pixel when up == 2): all Cs channels, children summed in registers
// KSU = 0: generic tap loops.  KSU = KS * 16 + STRIDE * 4 + UP (all > 0): square kernel, stride and up-sampling factor
// known at compile time; the (children x parity-class taps) loads are issued up front from clamped addresses and masked.
// The statements are in conv_small_dgrad_body.h: once here as a device function of a job-local block index and block count (vb, nb),
// for the two-job kernel, and once in the one-job kernel below.
template <int CS, int CN, int KSU>
__device__ __forceinline__ void conv_small_dgrad_body(const SmallGeom& g, const float* __restrict__ gy,
                                                      const float* __restrict__ wD, const float* __restrict__ x,
                                                      const float* __restrict__ scale, const float* __restrict__ shift,
                                                      int relu, const float* __restrict__ mean,
                                                      const float* __restrict__ invstd, float* __restrict__ gv,
                                                      double* __restrict__ partial, int CsPad, float* w_s,
                                                      double (*red)[2][SMALL_MAXC], unsigned vb, unsigned nb) {
#define SMALL_VB vb
#define SMALL_NB nb
#include "conv_small_dgrad_body.h"
#undef SMALL_VB
#undef SMALL_NB
}

template <int CS, int CN, int KSU>
__global__ __launch_bounds__(256) SMALL_OCC void conv_small_dgrad_kernel(SmallGeom g, const float* __restrict__ gy,
                                                               const float* __restrict__ wD, const float* __restrict__ x,
                                                               const float* __restrict__ scale, const float* __restrict__ shift,
                                                               int relu, const float* __restrict__ mean,
                                                               const float* __restrict__ invstd, float* __restrict__ gv,
                                                               double* __restrict__ partial, int CsPad) {
    __shared__ __align__(16) float w_s[SMALL_MAXW];  // wD[t][co][c]
    __shared__ double red[4][2][SMALL_MAXC];
#define SMALL_VB blockIdx.x
#define SMALL_NB gridDim.x
#include "conv_small_dgrad_body.h"
#undef SMALL_VB
#undef SMALL_NB
}

// The two-job form, as conv_small_fwd_pair_kernel, but with every pointer a kernel parameter of its own: the per-channel scale / shift /
// mean / invstd reads of the body are scalar loads hoisted out of the position loop only when their pointers are __restrict__ kernel
// parameters -- through pointers held in a by-value struct they stayed vector loads inside the loop, 182 registers for the 3x3
// body's 120.
#define SMALL_DGRAD_PARAMS(s)                                                                                                         \
    SmallGeom g##s, const float *__restrict__ gy##s, const float *__restrict__ wD##s, const float *__restrict__ x##s,                  \
        const float *__restrict__ scale##s, const float *__restrict__ shift##s, int relu##s, const float *__restrict__ mean##s,       \
        const float *__restrict__ invstd##s, float *__restrict__ gv##s, double *__restrict__ partial##s, int CsPad##s, unsigned nb##s
#define SMALL_DGRAD_ARGS(a) a.g, a.gy, a.wD, a.x, a.scale, a.shift, a.relu, a.mean, a.invstd, a.gv, a.partial, a.CsPad, (unsigned)a.nblocks

template <int CS0, int CN0, int KSU0, int CS1, int CN1, int KSU1>
__global__ __launch_bounds__(256) SMALL_OCC void conv_small_dgrad_pair_kernel(SMALL_DGRAD_PARAMS(0), SMALL_DGRAD_PARAMS(1)) {
    __shared__ __align__(16) float w_s[SMALL_MAXW];
    __shared__ double red[4][2][SMALL_MAXC];
    if constexpr (CS0 == CS1 && CN0 == CN1 && KSU0 == KSU1) {  // one body: select the job's arguments, not the code
        const bool j = blockIdx.x >= nb0;
        conv_small_dgrad_body<CS0, CN0, KSU0>(j ? g1 : g0, j ? gy1 : gy0, j ? wD1 : wD0, j ? x1 : x0, j ? scale1 : scale0,
                                              j ? shift1 : shift0, j ? relu1 : relu0, j ? mean1 : mean0, j ? invstd1 : invstd0,
                                              j ? gv1 : gv0, j ? partial1 : partial0, j ? CsPad1 : CsPad0, w_s, red,
                                              blockIdx.x - (j ? nb0 : 0), j ? nb1 : nb0);
    } else if (blockIdx.x < nb0)
        conv_small_dgrad_body<CS0, CN0, KSU0>(g0, gy0, wD0, x0, scale0, shift0, relu0, mean0, invstd0, gv0, partial0, CsPad0, w_s, red,
                                              blockIdx.x, nb0);
    else
        conv_small_dgrad_body<CS1, CN1, KSU1>(g1, gy1, wD1, x1, scale1, shift1, relu1, mean1, invstd1, gv1, partial1, CsPad1, w_s, red,
                                              blockIdx.x - nb0, nb1);
}

// The pairs the ConvBlock heads at the image side are made of: two equal 1 -> 8 4x4 stride-2 branches (first encoder block), and the
// 8 -> 1 up-sampling 3x3 with its 1x1 skip (last decoder block).  (CS, CN, KS) of job 0, of job 1, stride, up.
#define SMALL_PAIR_CASES(X) X(1, 8, 4, 1, 8, 4, 2, 1) X(8, 1, 3, 8, 1, 1, 1, 2)

static bool small_pair_match(const SmallGeom& a, const SmallGeom& b, int cs0, int cn0, int ks0, int cs1, int cn1, int ks1, int stride,
                             int up) {
    return a.Cs == cs0 && a.Cn == cn0 && a.KH == ks0 && a.KW == ks0 && b.Cs == cs1 && b.Cn == cn1 && b.KH == ks1 && b.KW == ks1 &&
           a.stride == stride && b.stride == stride && a.up == up && b.up == up;
}

int conv_small_fwd_pair(const SmallFwdArgs& a, const SmallFwdArgs& b, hipStream_t st) {
#define X(CS0_, CN0_, KS0_, CS1_, CN1_, KS1_, S_, U_)                                                              \
    if (small_pair_match(a.g, b.g, CS0_, CN0_, KS0_, CS1_, CN1_, KS1_, S_, U_)) {                                  \
        conv_small_fwd_pair_kernel<CS0_, CN0_, KS0_, CS1_, CN1_, KS1_><<<a.nblocks + b.nblocks, 256, 0, st>>>(a, b); \
        return 0;                                                                                                  \
    }
    SMALL_PAIR_CASES(X)
#undef X
    return -1;
}

int conv_small_dgrad_pair(const SmallDgradArgs& a, const SmallDgradArgs& b, hipStream_t st) {
#define X(CS0_, CN0_, KS0_, CS1_, CN1_, KS1_, S_, U_)                                                              \
    if (small_pair_match(a.g, b.g, CS0_, CN0_, KS0_, CS1_, CN1_, KS1_, S_, U_)) {                                  \
        conv_small_dgrad_pair_kernel<CS0_, CN0_, KS0_ * 16 + S_ * 4 + U_, CS1_, CN1_, KS1_ * 16 + S_ * 4 + U_>     \
            <<<a.nblocks + b.nblocks, 256, 0, st>>>(SMALL_DGRAD_ARGS(a), SMALL_DGRAD_ARGS(b));                     \
        return 0;                                                                                                  \
    }
    SMALL_PAIR_CASES(X)
#undef X
    return -1;
}

int conv_small_dgrad(const SmallGeom& g, int nblocks, const float* gy, const float* wD, const float* x, const float* scale,
                     const float* shift, int relu, const float* mean, const float* invstd, float* gv, double* partial,
                     int CsPad, hipStream_t st) {
#define X(CS_, CN_, KS_)                                                                                             \
    if (g.Cs == CS_ && g.Cn == CN_ && g.KH == KS_ && g.KW == KS_ && g.stride <= 2 && g.up <= 2) {                    \
        constexpr int K16 = KS_ * 16;                                                                                \
        auto go = [&](auto tag) {                                                                                    \
            conv_small_dgrad_kernel<CS_, CN_, decltype(tag)::value><<<nblocks, 256, 0, st>>>(                        \
                g, gy, wD, x, scale, shift, relu, mean, invstd, gv, partial, CsPad);                                 \
        };                                                                                                           \
        if (g.stride == 1 && g.up == 1) go(std::integral_constant<int, K16 + 4 + 1>{});                              \
        else if (g.stride == 1 && g.up == 2) go(std::integral_constant<int, K16 + 4 + 2>{});                         \
        else if (g.stride == 2 && g.up == 1) go(std::integral_constant<int, K16 + 8 + 1>{});                         \
        else go(std::integral_constant<int, K16 + 8 + 2>{});                                                         \
        return 0;                                                                                                    \
    }
    SMALL_KS_CASES(X)
#undef X
    SMALL_DISPATCH(conv_small_dgrad_kernel,
                   <<<nblocks, 256, 0, st>>>(g, gy, wD, x, scale, shift, relu, mean, invstd, gv, partial, CsPad));
    return 0;
}

// ------------------------------------------------------------------------------------------------ weight gradient
// one lane per output pixel (grid-stride), every weight element accumulated in a register, then one fixed-order
// wave/LDS reduction per block -> partial[block][K+hasb][Cn] (reduced over blocks by wgrad_reduce_kernel)
template <int T, int CS, int CN>
__global__ __launch_bounds__(256) SMALL_OCC void conv_small_wgrad_kernel(SmallGeom g, const float* __restrict__ x,
                                                               const float* __restrict__ scale, const float* __restrict__ shift,
                                                               int relu, const float* __restrict__ gy,
                                                               float* __restrict__ partial, int has_bias, unsigned chunk) {
    constexpr int NA = T * CS * CN;
    __shared__ float red[4][NA + CN];
    const bool affine = scale != nullptr;
    float sc[CS], sh[CS];
#pragma unroll
    for (int c = 0; c < CS; ++c) {
        sc[c] = affine ? scale[c] : 1.f;
        sh[c] = affine ? shift[c] : 0.f;
    }
    float acc[T][CS][CN], accb[CN];
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int c = 0; c < CS; ++c)
#pragma unroll
            for (int j = 0; j < CN; ++j) acc[t][c][j] = 0.f;
#pragma unroll
    for (int j = 0; j < CN; ++j) accb[j] = 0.f;

    const int Hu = g.Hs * g.up, Wu = g.Ws * g.up, ush = g.up - 1;
    const unsigned M = (unsigned)g.N * g.Ho * g.Wo;
    const float inv_wo = 1.0f / (float)g.Wo, inv_ho = 1.0f / (float)g.Ho;
    const bool small = M < (1u << 22);
    const unsigned mbeg = blockIdx.x * chunk, mend = min(M, mbeg + chunk);
    for (unsigned m = mbeg + threadIdx.x; m < mend; m += 256) {
        const unsigned t0 = sdiv(m, g.Wo, inv_wo, small);
        const int ox = m - t0 * g.Wo;
        const int n = sdiv(t0, g.Ho, inv_ho, small);
        const int oy = t0 - (unsigned)n * g.Ho;
        float gg[CN];
#pragma unroll
        for (int j = 0; j < CN; ++j) {
            gg[j] = gy[(size_t)m * CN + j];
            accb[j] += gg[j];
        }
        // the taps' loads are issued from clamped (always valid) addresses ahead of the arithmetic, in groups of <= 32
        // registers, and out-of-image taps are masked afterwards: a branch per tap exposes one load latency per tap
        constexpr int GS = (T * CS <= 32) ? T : (T % 3 == 0 ? 3 : (T % 4 == 0 ? 4 : 1));
#pragma unroll
        for (int t0g = 0; t0g < T; t0g += GS) {
            asm volatile("" ::: "memory");
            float xv[GS][CS];
            int ok[GS];  // all-ones / zero bit mask
#pragma unroll
            for (int i = 0; i < GS; ++i) {
                const int t = t0g + i;
                const int kh = t / g.KW, kw = t - kh * g.KW;
                const int iy = oy * g.stride + kh - g.pad, ix = ox * g.stride + kw - g.pad;
                ok[i] = ((unsigned)iy < (unsigned)Hu && (unsigned)ix < (unsigned)Wu) ? -1 : 0;
                const int cy = min(max(iy, 0), Hu - 1) >> ush, cx = min(max(ix, 0), Wu - 1) >> ush;
                load_chan<CS>(x + ((size_t)((unsigned)n * g.Hs + cy) * g.Ws + cx) * CS, xv[i], CS);
            }
#pragma unroll
            for (int i = 0; i < GS; ++i) {
#pragma unroll
                for (int c = 0; c < CS; ++c) {
                    const float a = __int_as_float(__float_as_int(act1(xv[i][c], sc[c], sh[c], affine, relu)) & ok[i]);
#pragma unroll
                    for (int j = 0; j < CN; ++j) acc[t0g + i][c][j] = fmaf(a, gg[j], acc[t0g + i][c][j]);
                }
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int c = 0; c < CS; ++c)
#pragma unroll
            for (int j = 0; j < CN; ++j) {
                const float s = wave_sum(acc[t][c][j]);
                if (lane == 0) red[wave][(t * CS + c) * CN + j] = s;
            }
#pragma unroll
    for (int j = 0; j < CN; ++j) {
        const float s = wave_sum(accb[j]);
        if (lane == 0) red[wave][NA + j] = s;
    }
    __syncthreads();
    const int Kp = T * CS + (has_bias ? 1 : 0);
    float* out = partial + (size_t)blockIdx.x * Kp * CN;
    for (int e = threadIdx.x; e < Kp * CN; e += 256) out[e] = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
}

bool conv_small_wgrad_ok(const SmallGeom& g) {
    if (!conv_small_ok(g)) return false;
    const int T = g.KH * g.KW;
    return (T == 16 && g.Cs == 1 && g.Cn == 8) || (T == 9 && g.Cs == 8 && g.Cn == 1) || (T == 9 && g.Cs == 1 && g.Cn == 1) ||
           (T == 1 && g.Cs == 1 && g.Cn == 3) || (T == 1 && g.Cs == 1 && g.Cn == 1) || (T == 1 && g.Cs == 8 && g.Cn == 1) ||
           // RGB image side (every weight element in a register: T * Cs * Cn <= 81)
           (T == 9 && g.Cs == 3 && g.Cn == 3) || (T == 1 && g.Cs == 3 && g.Cn == 3) || (T == 1 && g.Cs == 3 && g.Cn == 9) ||
           (T == 1 && g.Cs == 16 && g.Cn == 3);
}

void conv_small_wgrad_plan(const SmallGeom& g, int& P, unsigned& chunk) {
    const unsigned M = (unsigned)g.N * g.Ho * g.Wo;
    P = imax(1, imin(512, (int)(M / 1024)));
    chunk = (M + P - 1) / P;
    P = cdiv(M, chunk);
}

int conv_small_wgrad(const SmallGeom& g, const float* x, const float* scale, const float* shift, int relu, const float* gy,
                     int has_bias, float* partial, hipStream_t st) {
    int P;
    unsigned chunk;
    conv_small_wgrad_plan(g, P, chunk);
    const int T = g.KH * g.KW;
#define SW(T_, CS_, CN_) \
    conv_small_wgrad_kernel<T_, CS_, CN_><<<P, 256, 0, st>>>(g, x, scale, shift, relu, gy, partial, has_bias, chunk)
    if (T == 16 && g.Cs == 1 && g.Cn == 8) SW(16, 1, 8);
    else if (T == 9 && g.Cs == 8 && g.Cn == 1) SW(9, 8, 1);
    else if (T == 9 && g.Cs == 1 && g.Cn == 1) SW(9, 1, 1);
    else if (T == 1 && g.Cs == 1 && g.Cn == 3) SW(1, 1, 3);
    else if (T == 1 && g.Cs == 1 && g.Cn == 1) SW(1, 1, 1);
    else if (T == 1 && g.Cs == 8 && g.Cn == 1) SW(1, 8, 1);
    else if (T == 9 && g.Cs == 3 && g.Cn == 3) SW(9, 3, 3);
    else if (T == 1 && g.Cs == 3 && g.Cn == 3) SW(1, 3, 3);
    else if (T == 1 && g.Cs == 3 && g.Cn == 9) SW(1, 3, 9);
    else if (T == 1 && g.Cs == 16 && g.Cn == 3) SW(1, 16, 3);
    else return -1;
#undef SW
    return P;
}
