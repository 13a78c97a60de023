// The arithmetic of one log-domain Sinkhorn iteration, written once for the solver (sinkhorn.hip) and the tape-recording forward
// (sinkhorn_diff.hip): the Cr / Cr^T / log-marginal initialisation, the row log-sum-exp in its streaming form (a launch per
// half-iteration) and its register form (the persistent kernels), the stopping test and the plan row.  Every solver route must
// give identical bits, so the order of the floating-point operations here is fixed: row[l] + add[l], x - mx,
// logm - (mx + log s), u + v + cr, and the double-precision reduction tree of the stopping test.
// The library is built without relocatable device code: a kernel lives in the code object of the file that launches it, hence
// the unnamed namespace (each including file gets its own copy of the kernels).
#pragma once
#include "common.h"

namespace {

template <typename T>
struct MathT;
template <>
struct MathT<float> {
    static __device__ __forceinline__ float exp(float x) { return __expf(x); }
    static __device__ __forceinline__ float log(float x) { return __logf(x); }
    static __device__ __forceinline__ float ninf() { return -INFINITY; }
};
template <>
struct MathT<double> {
    static __device__ __forceinline__ double exp(double x) { return ::exp(x); }
    static __device__ __forceinline__ double log(double x) { return ::log(x); }
    static __device__ __forceinline__ double ninf() { return -(double)INFINITY; }
};

struct SkCtl {           // the last 256 bytes of the solver's workspace and of the tape
    int done;            // set by sk_check when the batch-min difference drops below the threshold
    int iters;           // iterations actually performed
    unsigned bar_count;  // persistent kernel: monotone arrival counter of the grid barrier
    int timeout;         // persistent kernel: a wait ran out (the plan, the potentials and the cost are poisoned with NaN; iters = -1)
    unsigned spin_limit; // persistent kernel: polls a wait may spend before it gives up (OTVAE_SK_SPIN_LIMIT, default 2^22)
};

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Cr = -C/(reg * cmax) (row major, into `cr`) and its transpose (into `crt`), 32x32 tiles through LDS.  cmax = the
// maximum of problem b's cost matrix, reduced here from the P partial maxima its producer left (otvae_sqdist's epilogue),
// or 1 when pmax == NULL: the `cost_matrix / max_per_mat` of batch_ot_gmm (ot/w2_utils.py:265-266) without a pass of its
// own.  The blocks of the first tile row / column also initialise the potentials and the log-marginals (a, b == NULL:
// uniform 1/N, 1/M), block (0,0,0) the control block.  tu, tv, scale_out may be NULL.
template <typename T>
__global__ __launch_bounds__(256) void sk_init_mat(const T* __restrict__ Cm, int N, int M, T inv_reg, const T* __restrict__ pmax, int P,
                                                   T* __restrict__ cr, T* __restrict__ crt, const T* __restrict__ a,
                                                   const T* __restrict__ b, T* __restrict__ loga, T* __restrict__ logb,
                                                   T* __restrict__ u, T* __restrict__ v, SkCtl* ctl, int preset_iters,
                                                   unsigned spin_limit, unsigned long long* __restrict__ tu,
                                                   unsigned long long* __restrict__ tv, T* __restrict__ scale_out) {
    __shared__ T tile[32][33];
    __shared__ T s_red[4];
    const int pb = blockIdx.z;
    const size_t boff = (size_t)pb * N * M;
    const int i0 = blockIdx.y * 32, j0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    T neg_scale = -inv_reg;
    if (pmax) {
        T mx = MathT<T>::ninf();
        for (int i = threadIdx.x; i < P; i += 256) {
            const T q = pmax[(size_t)pb * P + i];
            mx = q > mx ? q : mx;
        }
        mx = wave_max(mx);
        if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = mx;
        __syncthreads();
        const T m01 = s_red[0] > s_red[1] ? s_red[0] : s_red[1], m23 = s_red[2] > s_red[3] ? s_red[2] : s_red[3];
        const T cmax = m01 > m23 ? m01 : m23;
        neg_scale = -inv_reg / cmax;
        if (scale_out && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) scale_out[pb] = cmax;
    }
    for (int r = ty; r < 32; r += 8) {
        const int i = i0 + r, j = j0 + tx;
        if (i < N && j < M) {
            const T val = Cm[boff + (size_t)i * M + j] * neg_scale;
            cr[boff + (size_t)i * M + j] = val;
            tile[r][tx] = val;
        }
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int j = j0 + r, i = i0 + tx;
        if (i < N && j < M) crt[boff + (size_t)j * N + i] = tile[tx][r];
    }
    if (blockIdx.x == 0 && threadIdx.x < 32 && i0 + (int)threadIdx.x < N) {
        const size_t i = (size_t)pb * N + i0 + threadIdx.x;
        loga[i] = MathT<T>::log((a ? a[i] : (T)1 / (T)N) + (T)1e-8);
        u[i] = (T)0;
        if (tu) tu[i] = 0ull;  // {epoch 0, +0.0f}: the tagged potentials of sk_persistent_tagged
    }
    if (blockIdx.y == 0 && threadIdx.x >= 64 && threadIdx.x < 96 && j0 + (int)threadIdx.x - 64 < M) {
        const size_t j = (size_t)pb * M + j0 + threadIdx.x - 64;
        logb[j] = MathT<T>::log((b ? b[j] : (T)1 / (T)M) + (T)1e-8);
        v[j] = (T)0;
        if (tv) tv[j] = 0ull;
    }
    if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 128) {
        ctl->done = 0;
        ctl->iters = preset_iters;
        ctl->bar_count = 0;
        ctl->timeout = 0;
        ctl->spin_limit = spin_limit;
    }
}

// Streaming row pass: out[r] = logm[r] - LSE_l(mat[r][l] + add[l]);  absd[r] = |out[r] - prev[r]| (absd may be NULL).  One wave
// per row.  `prev` is where the previous value of the potential lies: `out` itself in the solver (hence no __restrict__ on the
// pair, and the read before the write), the previous history slice in the tape.
template <typename T>
__global__ __launch_bounds__(256) void sk_pass(const T* __restrict__ mat, const T* __restrict__ add, const T* __restrict__ logm,
                                               int R, int L, const T* prev, T* out, T* __restrict__ absd, const SkCtl* ctl) {
    if (ctl->done) return;
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const int b = blockIdx.y;
    const T* row = mat + ((size_t)b * R + r) * L;
    const T* ad = add + (size_t)b * L;
    T mx = MathT<T>::ninf();
    for (int l = lane; l < L; l += 64) {
        const T x = row[l] + ad[l];
        mx = x > mx ? x : mx;
    }
    mx = wave_max(mx);
    T s = (T)0;
    for (int l = lane; l < L; l += 64) s += MathT<T>::exp(row[l] + ad[l] - mx);
    s = wave_sum(s);
    if (lane == 0) {
        const T nv = logm[(size_t)b * R + r] - (mx + MathT<T>::log(s));
        if (absd) {
            const T d = nv - prev[(size_t)b * R + r];
            absd[(size_t)b * R + r] = d < (T)0 ? -d : d;
        }
        out[(size_t)b * R + r] = nv;
    }
}

// min over the batch of diff_b = sum |du| + sum |dv|, summed by the first 256 threads of the workgroup (4 waves, whatever its
// size) in double and compared in the tensor dtype, as the reference sums in that dtype.  Block-uniform call; every thread
// returns the minimum.  `ld` loads one entry (plainly, or coherently where other workgroups wrote it during this launch).
template <typename T, typename Load>
__device__ __forceinline__ double sk_min_diff(const T* __restrict__ adu, const T* __restrict__ adv, int nb, int N, int M, Load ld) {
    __shared__ double red[4];
    __shared__ double best;
    if (threadIdx.x == 0) best = INFINITY;
    __syncthreads();
    for (int b = 0; b < nb; ++b) {
        if (threadIdx.x < 256) {
            double s = 0.0;
            for (int i = threadIdx.x; i < N; i += 256) s += (double)ld(adu + (size_t)b * N + i);
            for (int i = threadIdx.x; i < M; i += 256) s += (double)ld(adv + (size_t)b * M + i);
            s = wave_sum(s);
            if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const T d = (T)((red[0] + red[1]) + (red[2] + red[3]));
            if ((double)d < best) best = (double)d;
        }
        __syncthreads();
    }
    return best;
}

// one block: done = (min_b diff_b < threshold); counts the iteration
template <typename T>
__global__ __launch_bounds__(256) void sk_check(const T* __restrict__ adu, const T* __restrict__ adv, int nb, int N, int M,
                                                double threshold, SkCtl* ctl) {
    if (ctl->done) return;
    const double best = sk_min_diff<T>(adu, adv, nb, N, M, [](const T* p) { return *p; });
    if (threadIdx.x == 0) {
        ctl->iters += 1;
        if (best < threshold) ctl->done = 1;
    }
}

// ---- register-resident rows (the persistent kernels): a wave owns rows wave_g + q * nwaves, q < RPW, of a matrix and keeps
// each as SK_EPL elements per lane (element lane + 64 k in slot k; -inf beyond the row or the matrix) for the whole solve
#define SK_EPL 16  // rows up to 1024

template <typename T, int RPW>
__device__ __forceinline__ void sk_reg_rows_load(T (&rows)[RPW][SK_EPL], const T* __restrict__ mat, int R, int L, int wave_g, int nwaves,
                                                 int lane) {
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
        const int r = wave_g + q * nwaves;
#pragma unroll
        for (int k = 0; k < SK_EPL; ++k) {
            const int l = lane + 64 * k;
            rows[q][k] = (r < R && l < L) ? mat[(size_t)r * L + l] : MathT<T>::ninf();
        }
    }
}

// LSE_l(row[l] + pot[l]) over l < L, in every lane of the wave (sk_pass's arithmetic per row)
template <typename T>
__device__ __forceinline__ T sk_reg_row_lse(const T (&row)[SK_EPL], const T* __restrict__ pot, int L, int lane) {
    T x[SK_EPL], mx = MathT<T>::ninf(), s = (T)0;
#pragma unroll
    for (int k = 0; k < SK_EPL; ++k) {
        const int l = lane + 64 * k;
        x[k] = l < L ? row[k] + pot[l] : MathT<T>::ninf();
        mx = x[k] > mx ? x[k] : mx;
    }
    mx = wave_max(mx);
#pragma unroll
    for (int k = 0; k < SK_EPL; ++k)
        if (lane + 64 * k < L) s += MathT<T>::exp(x[k] - mx);
    s = wave_sum(s);
    return mx + MathT<T>::log(s);
}

// one row of the plan, pi[l] = exp(u_i + v_l + Cr_il), from the row of Cr in registers; v(l) loads v_l
template <typename T, typename Load>
__device__ __forceinline__ void sk_reg_row_plan(T* __restrict__ pi_row, const T (&cr)[SK_EPL], T ui, int M, int lane, Load v) {
#pragma unroll
    for (int k = 0; k < SK_EPL; ++k) {
        const int l = lane + 64 * k;
        if (l < M) pi_row[l] = MathT<T>::exp(ui + v(l) + cr[k]);
    }
}

}  // namespace
