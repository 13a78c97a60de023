// Sliced Wasserstein-2 between the latents of a minibatch and as many prior draws (SlicedWassersteinPrior; DESIGN.md "Sliced W2").
//
// Forward, one workgroup per projection l (plain fp32 FMA, no matrix cores: a workgroup owns ONE direction, so the projection is a
// matrix-vector product and streams z and y once from L2):
//   1. |g_l|^2 by the block in a fixed order -> theta_l = g_l / |g_l| (written for the backward);
//   2. p_i = z_i . theta_l, q_i = y_i . theta_l: 8 lanes per row, each lane 16 contiguous bytes of the row per step (a row group reads
//      whole 128-byte lines), reduced by three lane exchanges;
//   3. keys into LDS: z as 64-bit (order-preserving image of p) << 32 | row, y as the 32-bit image of q; rows N .. P - 1 (P = N rounded
//      up to a power of two) hold the image of +inf with row >= N.  Integer compares: ties fall to the smaller row, and a NaN cannot
//      derail the network.  A projection that is not finite takes the key of +inf (it stays among the first N) and raises the
//      workgroup's poison flag;
//   4. one bitonic network over P elements, both arrays in the same pass; steps whose distance is <= 64 stay inside a wave's own
//      128-element chunks and are separated by a wave-level fence instead of a block barrier;
//   5. sorted position k < N pairs p_(k) with q_(k): resid[l][row] = p - q, sum of squares in fp64 in a fixed order -> ws[l]
//      (NaN when poisoned).
// A second one-block launch adds ws[0 .. L) in index order and writes the replicated loss: bit-reproducible, no float atomics.
// LDS: 12 bytes per padded row (48 KiB at N = 4096) + 144 bytes of reduction scratch and the poison flag.
//
// Backward: gz = gadd + c * resid^T theta on the matrix cores (16 x 16 x 4 fp32 MFMA, one wave per 16 x 16 tile of gz, both operands
// read straight from global memory: resid is [L][N], i.e. already K-major, and theta is [L][D]), one launch.
#include "common.h"
#include "ordered_key.h"

#define SW_MAX_N 4096
#define SW_LANES_PER_ROW 8

// block-wide sum in a fixed order (lane tree, then the waves in index order); every thread gets the total.  red: LDS, 16 entries
template <typename T>
__device__ __forceinline__ T sw_block_sum(T v, T* red) {
    v = wave_sum(v);
    __syncthreads();  // red may still be read from an earlier call
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    T t = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += red[w];
    return t;
}

template <bool VEC4>
__global__ void __launch_bounds__(1024)
sliced_w2_fwd_kernel(const float* __restrict__ z, const float* __restrict__ y, const float* __restrict__ dirs, int N, int D, int P,
                     float* __restrict__ theta, float* __restrict__ resid, double* __restrict__ partial) {
    extern __shared__ __align__(16) unsigned long long sw_smem[];
    unsigned long long* zk = sw_smem;                          // [P] (ord(p) << 32) | row
    unsigned* yk = reinterpret_cast<unsigned*>(sw_smem + P);   // [P] ord(q)
    __shared__ double red[16];
    __shared__ int s_bad;
    const int tid = threadIdx.x, T = blockDim.x;
    const size_t l = blockIdx.x;
    const float* g = dirs + l * D;
    if (tid == 0) s_bad = 0;

    // 1. the direction's norm, theta_l for the backward
    float ss = 0.f;
    for (int d = tid; d < D; d += T) ss = fmaf(g[d], g[d], ss);
    ss = sw_block_sum(ss, reinterpret_cast<float*>(red));
    const float inv = 1.f / sqrtf(ss);   // g_l = 0: inf -> theta, p, q are NaN -> the loss is NaN
    for (int d = tid; d < D; d += T) theta[l * D + d] = g[d] * inv;

    // 2. + 3. projections and keys
    const int s = tid & (SW_LANES_PER_ROW - 1), slot = tid / SW_LANES_PER_ROW, slots = T / SW_LANES_PER_ROW;
    const unsigned ord_inf = ord_f32(__uint_as_float(0x7f800000u));
    for (int base = 0; base < N; base += slots) {   // block-uniform trip count: the lane exchanges below are never divergent
        const int i = base + slot;
        const bool live = i < N;
        float az = 0.f, ay = 0.f;
        if (live) {
            if (VEC4) {
                const float4* zr = reinterpret_cast<const float4*>(z + (size_t)i * D);
                const float4* yr = reinterpret_cast<const float4*>(y + (size_t)i * D);
                const float4* g4 = reinterpret_cast<const float4*>(g);
                const int D4 = D >> 2;
#pragma unroll 4
                for (int c = s; c < D4; c += SW_LANES_PER_ROW) {
                    const float4 a = zr[c], b = yr[c], t = g4[c];
                    const float t0 = t.x * inv, t1 = t.y * inv, t2 = t.z * inv, t3 = t.w * inv;   // the bits of theta
                    az = fmaf(a.x, t0, az); az = fmaf(a.y, t1, az); az = fmaf(a.z, t2, az); az = fmaf(a.w, t3, az);
                    ay = fmaf(b.x, t0, ay); ay = fmaf(b.y, t1, ay); ay = fmaf(b.z, t2, ay); ay = fmaf(b.w, t3, ay);
                }
            } else {
                const float* zr = z + (size_t)i * D;
                const float* yr = y + (size_t)i * D;
#pragma unroll 4
                for (int d = s; d < D; d += SW_LANES_PER_ROW) {
                    const float t = g[d] * inv;
                    az = fmaf(zr[d], t, az);
                    ay = fmaf(yr[d], t, ay);
                }
            }
        }
#pragma unroll
        for (int o = 1; o < SW_LANES_PER_ROW; o <<= 1) {
            az += __shfl_xor(az, o, 64);
            ay += __shfl_xor(ay, o, 64);
        }
        if (live && s == 0) {
            az += 0.f;   // -0 -> +0: equal as floats, so equal as keys
            ay += 0.f;
            const bool fz = isfinite(az), fy = isfinite(ay);
            if (!(fz && fy)) atomicOr(&s_bad, 1);
            zk[i] = ((unsigned long long)(fz ? ord_f32(az) : ord_inf) << 32) | (unsigned)i;
            yk[i] = fy ? ord_f32(ay) : ord_inf;
        }
    }
    for (int i = N + tid; i < P; i += T) {   // padding: +inf behind every real row
        zk[i] = ((unsigned long long)ord_inf << 32) | (unsigned)i;
        yk[i] = ord_inf;
    }
    __syncthreads();

    // 4. bitonic network on both arrays
    const int half = P >> 1;
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < half; t += T) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int hi = lo | j;
                const bool up = (lo & k) == 0;
                const unsigned long long a = zk[lo], b = zk[hi];
                const unsigned c = yk[lo], e = yk[hi];
                const bool sz = (a > b) == up, sy = (c > e) == up;   // all four loads first, stores without a branch
                zk[lo] = sz ? b : a;
                zk[hi] = sz ? a : b;
                yk[lo] = sy ? e : c;
                yk[hi] = sy ? c : e;
            }
            // pairs t = tid + m T of one wave lie, for j <= 64, in 128-element chunks no other wave touches: between two such steps the
            // wave's own LDS accesses, which complete in issue order, are all that has to be ordered
            const int jn = j > 1 ? j >> 1 : k;   // the next step's distance
            if (j > 64 || jn > 64) __syncthreads();
            else wave_lds_sync();
        }
    }
    __syncthreads();

    // 5. match, residuals in original row order, this projection's sum of squares
    const bool bad = s_bad != 0;
    const float nanf_ = __uint_as_float(0x7fc00000u);
    double acc = 0.0;
    for (int k = tid; k < N; k += T) {
        const unsigned long long e = zk[k];
        const unsigned row = (unsigned)e;
        const float r = unord_f32((unsigned)(e >> 32)) - unord_f32(yk[k]);
        if (row < (unsigned)N) resid[l * N + row] = bad ? nanf_ : r;   // (always true: the real rows are the first N)
        acc += (double)r * (double)r;
    }
    acc = sw_block_sum(acc, red);
    if (tid == 0) partial[l] = bad ? __longlong_as_double(0x7ff8000000000000LL) : acc;
}

// loss[0 .. rep) = coef * (partial[0] + ... + partial[L - 1]), the sum in a fixed order
__global__ void __launch_bounds__(256)
sliced_w2_finish_kernel(const double* __restrict__ partial, int L, double coef, int rep, float* __restrict__ loss) {
    __shared__ double red[16];
    double a = 0.0;
    for (int l = threadIdx.x; l < L; l += 256) a += partial[l];
    a = sw_block_sum(a, red);
    const float v = (float)(coef * a);
    for (int b = threadIdx.x; b < rep; b += 256) loss[b] = v;
}

// gz[i][d] = gadd[i][d] + c sum_l resid[l][i] theta[l][d]: wave w of a block owns the 16 x 16 tile at rows 16 blockIdx.y, columns
// 16 (4 blockIdx.x + w); two accumulators take alternate K-steps (the dependent-accumulator latency of the MFMA), fixed order.
__global__ void __launch_bounds__(256)
sliced_w2_bwd_kernel(const float* __restrict__ gout, const float* __restrict__ gadd, const float* __restrict__ resid,
                     const float* __restrict__ theta, int N, int D, int L, float coef, float* __restrict__ gz) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int i0 = blockIdx.y * 16, j0 = (blockIdx.x * 4 + w) * 16;
    if (j0 >= D) return;
    const int fr = lane & 15, fq = lane >> 4;
    const bool row_ok = i0 + fr < N, col_ok = j0 + fr < D;
    const float* a_ptr = resid + (i0 + fr);
    const float* b_ptr = theta + (j0 + fr);
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < L; k0 += 8) {
        const int ka = k0 + fq, kb = k0 + 4 + fq;
        const float a0 = (row_ok && ka < L) ? a_ptr[(size_t)ka * N] : 0.f;
        const float b0 = (col_ok && ka < L) ? b_ptr[(size_t)ka * D] : 0.f;
        const float a1 = (row_ok && kb < L) ? a_ptr[(size_t)kb * N] : 0.f;
        const float b1 = (col_ok && kb < L) ? b_ptr[(size_t)kb * D] : 0.f;
        acc0 = mfma16(a0, b0, acc0);
        acc1 = mfma16(a1, b1, acc1);
    }
    float gs = 0.f;   // sum of the upstream gradients of the loss replicas: lanes take every 64th, fixed exchange tree
    for (int q = lane; q < N; q += 64) gs += gout[q];
    gs = wave_sum(gs);
    const float c = coef * gs;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = i0 + fq * 4 + r;
        if (i < N && col_ok) {
            const size_t e = (size_t)i * D + j0 + fr;
            const float v = __fmul_rn(c, acc0[r] + acc1[r]);   // rounded on its own: gadd is ADDED to the same bits, never fused in
            gz[e] = gadd ? gadd[e] + v : v;
        }
    }
}

static inline int sw_pow2(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

extern "C" int64_t otvae_sliced_w2_ws(int N, int L) {
    if (N < 1 || N > SW_MAX_N || L < 1) return -1;
    return (int64_t)L * (int64_t)sizeof(double);
}

extern "C" int otvae_sliced_w2_fwd(const float* z, const float* y, const float* dirs, int N, int D, int L, double scale, int loss_rep,
                                   void* ws, float* theta, float* resid, float* loss, void* stream) {
    OTVAE_REQUIRE(z && y && dirs && ws && theta && resid && loss, "otvae_sliced_w2_fwd: NULL argument");
    OTVAE_REQUIRE(N > 0 && D > 0 && L > 0 && loss_rep > 0, "otvae_sliced_w2_fwd: bad sizes (N %d, D %d, L %d, loss_rep %d)", N, D, L, loss_rep);
    OTVAE_REQUIRE((uintptr_t)ws % 8 == 0, "otvae_sliced_w2_fwd: the workspace must be 8-byte aligned");
    if (N > SW_MAX_N) {
        otvae_set_error("otvae_sliced_w2_fwd: N = %d is beyond the %d rows one workgroup sorts in LDS", N, SW_MAX_N);
        return OTVAE_EUNSUPPORTED;
    }
    const int P = sw_pow2(N);
    const int threads = imin(1024, imax(64, P / 2));
    const size_t lds = (size_t)P * 12;
    const bool vec4 = D % 4 == 0 && (uintptr_t)z % 16 == 0 && (uintptr_t)y % 16 == 0 && (uintptr_t)dirs % 16 == 0;
    hipStream_t st = (hipStream_t)stream;
    if (vec4)
        sliced_w2_fwd_kernel<true><<<dim3(L), threads, lds, st>>>(z, y, dirs, N, D, P, theta, resid, (double*)ws);
    else
        sliced_w2_fwd_kernel<false><<<dim3(L), threads, lds, st>>>(z, y, dirs, N, D, P, theta, resid, (double*)ws);
    OTVAE_CHECK_LAUNCH("otvae_sliced_w2_fwd(sort and match)");
    sliced_w2_finish_kernel<<<1, 256, 0, st>>>((const double*)ws, L, scale / ((double)L * (double)N), loss_rep, loss);
    OTVAE_CHECK_LAUNCH("otvae_sliced_w2_fwd(loss)");
    return OTVAE_OK;
}

extern "C" int otvae_sliced_w2_bwd(const float* gout, const float* gadd, const float* resid, const float* theta, int N, int D, int L,
                                   double scale, float* gz, void* stream) {
    OTVAE_REQUIRE(gout && resid && theta && gz, "otvae_sliced_w2_bwd: NULL argument");
    OTVAE_REQUIRE(N > 0 && D > 0 && L > 0, "otvae_sliced_w2_bwd: bad sizes (N %d, D %d, L %d)", N, D, L);
    OTVAE_REQUIRE(cdiv(N, 16) <= 65535, "otvae_sliced_w2_bwd: N = %d is beyond the launch grid", N);
    const float coef = (float)(2.0 * scale / ((double)L * (double)N));
    sliced_w2_bwd_kernel<<<dim3(cdiv(D, 64), cdiv(N, 16)), 256, 0, (hipStream_t)stream>>>(gout, gadd, resid, theta, N, D, L, coef, gz);
    OTVAE_CHECK_LAUNCH("otvae_sliced_w2_bwd");
    return OTVAE_OK;
}
