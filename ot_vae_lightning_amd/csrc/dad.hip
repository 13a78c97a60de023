// Discrete Auto Diffuser (reference model/discrete_auto_diffuser.py:56-95): the shifted soft-label cross-entropy of its training loss,
// one categorical draw of its sampling loop, and the row gather that decodes the sampled ids.
//
// soft CE.  ce[b] = sum_{t < T-1} ( -sum_k p[b][t+1][k] * log_softmax(l[b][t][:])[k] ).  The reference forms it from two sliced copies,
// two transposes, log_softmax, a product and a sum; here a row (b, t) is ONE pass over l[b][t][:] and p[b][t+1][:]: with the running
// maximum m, s = sum exp(l - m), a = sum p l and ps = sum p the row is ps * (m + log s) - a.  The shift is index arithmetic.  s, a, ps
// and the sum over t are accumulated in fp64 (the row is memory-bound: free), every reduction in a fixed order, no float atomics.
//
// Rows of up to SOFT_CE_WAVE_K entries are taken by one wave (four rows per workgroup), longer ones by a whole workgroup.
#include "common.h"
#include "dropout_hash.h"

#define SOFT_CE_WAVE_K 512

struct RowAcc {
    float m;        // running maximum
    double s;       // sum exp(l - m)
    double a, ps;   // sum p * l, sum p
};

__device__ __forceinline__ void row_acc_add(RowAcc& r, float l, float p) {
    if (l > r.m) {
        r.s = (r.m == -INFINITY ? 0.0 : r.s * (double)__expf(r.m - l)) + 1.0;
        r.m = l;
    } else if (r.m != -INFINITY) {
        r.s += (double)__expf(l - r.m);
    }
    r.a += (double)p * (double)l;
    r.ps += (double)p;
}

// reduction over the TPR threads that share a row (TPR = 64: the wave; 256: the four waves of the workgroup through LDS, wave order)
template <int TPR>
__device__ __forceinline__ void row_acc_reduce(RowAcc& r, double* s_red) {
    const float m = wave_max(r.m);
    r.s = wave_sum(r.m == -INFINITY ? 0.0 : r.s * exp((double)r.m - (double)m));
    r.a = wave_sum(r.a);
    r.ps = wave_sum(r.ps);
    r.m = m;
    if (TPR == 256) {
        const int w = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) {
            s_red[w * 4 + 0] = (double)r.m;
            s_red[w * 4 + 1] = r.s;
            s_red[w * 4 + 2] = r.a;
            s_red[w * 4 + 3] = r.ps;
        }
        __syncthreads();
        double mm = s_red[0];
        for (int i = 1; i < 4; ++i) mm = s_red[i * 4] > mm ? s_red[i * 4] : mm;
        double s = 0.0, a = 0.0, ps = 0.0;
        for (int i = 0; i < 4; ++i) {
            const double mi = s_red[i * 4];
            s += mi == -INFINITY ? 0.0 : s_red[i * 4 + 1] * exp(mi - mm);
            a += s_red[i * 4 + 2];
            ps += s_red[i * 4 + 3];
        }
        __syncthreads();   // s_red is written again by the next row
        r.m = (float)mm;
        r.s = s;
        r.a = a;
        r.ps = ps;
    }
}

template <int TPR, bool VEC>
__global__ __launch_bounds__(256) void soft_ce_rows_kernel(const float* __restrict__ logits, int64_t lsb, int64_t lst,
                                                           const float* __restrict__ probs, int64_t psb, int64_t pst, int B, int T, int K,
                                                           float* __restrict__ lse, float* __restrict__ psum, double* __restrict__ rowloss) {
    __shared__ double s_red[16];
    constexpr int RPB = 256 / TPR;
    const int lane = threadIdx.x % TPR, sub = threadIdx.x / TPR;
    const int64_t rows = (int64_t)B * (T - 1);
    // (block-uniform trip count: the TPR = 256 reduction holds barriers)
    for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < rows; r0 += (int64_t)gridDim.x * RPB) {
        const int64_t row = r0 + sub;
        if (RPB > 1 && row >= rows) continue;   // whole waves: no barrier on this path
        const int b = (int)(row / (T - 1)), t = (int)(row % (T - 1));
        const float* __restrict__ l = logits + b * lsb + t * lst;
        const float* __restrict__ p = probs + b * psb + (t + 1) * pst;
        RowAcc acc = {-INFINITY, 0.0, 0.0, 0.0};
        if (VEC) {
            for (int k = lane * 4; k < K; k += TPR * 4) {
                const f32x4 lv = *reinterpret_cast<const f32x4*>(l + k);
                const f32x4 pv = *reinterpret_cast<const f32x4*>(p + k);
                row_acc_add(acc, lv.x, pv.x);
                row_acc_add(acc, lv.y, pv.y);
                row_acc_add(acc, lv.z, pv.z);
                row_acc_add(acc, lv.w, pv.w);
            }
        } else {
            for (int k = lane; k < K; k += TPR) row_acc_add(acc, l[k], p[k]);
        }
        row_acc_reduce<TPR>(acc, s_red);
        if (lane == 0) {
            const double e = (double)acc.m + log(acc.s);
            lse[(int64_t)b * T + t] = (float)e;
            psum[(int64_t)b * T + t] = (float)acc.ps;
            rowloss[row] = acc.ps * e - acc.a;
            if (t == T - 2) {   // the last position predicts nothing: defined values in the saved rows
                lse[(int64_t)b * T + T - 1] = 0.f;
                psum[(int64_t)b * T + T - 1] = 0.f;
            }
        }
    }
}

__global__ __launch_bounds__(256) void soft_ce_sum_kernel(const double* __restrict__ rowloss, int B, int Tm1, float* __restrict__ loss) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    double s = 0.0;
    for (int t = 0; t < Tm1; ++t) s += rowloss[(int64_t)b * Tm1 + t];
    loss[b] = (float)s;
}

template <int TPR, bool VEC>
__global__ __launch_bounds__(256) void soft_ce_bwd_kernel(const float* __restrict__ logits, int64_t lsb, int64_t lst,
                                                          const float* __restrict__ probs, int64_t psb, int64_t pst,
                                                          const float* __restrict__ lse, const float* __restrict__ psum,
                                                          const float* __restrict__ g, int B, int T, int K, float* __restrict__ dlogits,
                                                          float* __restrict__ dprobs) {
    constexpr int RPB = 256 / TPR;
    const int lane = threadIdx.x % TPR, sub = threadIdx.x / TPR;
    const int64_t rows = (int64_t)B * (T - 1);
    for (int64_t row = (int64_t)blockIdx.x * RPB + sub; row < rows; row += (int64_t)gridDim.x * RPB) {
        const int b = (int)(row / (T - 1)), t = (int)(row % (T - 1));
        const float* __restrict__ l = logits + b * lsb + t * lst;
        const float* __restrict__ p = probs + b * psb + (t + 1) * pst;
        const float gb = g[b], e = lse[(int64_t)b * T + t], ps = psum[(int64_t)b * T + t];
        float* __restrict__ dl = dlogits ? dlogits + ((int64_t)b * T + t) * K : nullptr;
        float* __restrict__ dp = dprobs ? dprobs + ((int64_t)b * T + t + 1) * K : nullptr;
        // the structural zeros: nothing predicts token 0, the last position predicts nothing
        float* __restrict__ z0 = (dprobs && t == 0) ? dprobs + (int64_t)b * T * K : nullptr;
        float* __restrict__ z1 = (dlogits && t == T - 2) ? dlogits + ((int64_t)b * T + T - 1) * K : nullptr;
        if (VEC) {
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            for (int k = lane * 4; k < K; k += TPR * 4) {
                const f32x4 lv = *reinterpret_cast<const f32x4*>(l + k);
                if (dl) {
                    const f32x4 pv = *reinterpret_cast<const f32x4*>(p + k);
                    f32x4 o;
                    o.x = gb * (__expf(lv.x - e) * ps - pv.x);
                    o.y = gb * (__expf(lv.y - e) * ps - pv.y);
                    o.z = gb * (__expf(lv.z - e) * ps - pv.z);
                    o.w = gb * (__expf(lv.w - e) * ps - pv.w);
                    *reinterpret_cast<f32x4*>(dl + k) = o;
                }
                if (dp) {
                    f32x4 o;
                    o.x = -gb * (lv.x - e);
                    o.y = -gb * (lv.y - e);
                    o.z = -gb * (lv.z - e);
                    o.w = -gb * (lv.w - e);
                    *reinterpret_cast<f32x4*>(dp + k) = o;
                }
                if (z0) *reinterpret_cast<f32x4*>(z0 + k) = zero;
                if (z1) *reinterpret_cast<f32x4*>(z1 + k) = zero;
            }
        } else {
            for (int k = lane; k < K; k += TPR) {
                const float lv = l[k];
                if (dl) dl[k] = gb * (__expf(lv - e) * ps - p[k]);
                if (dp) dp[k] = -gb * (lv - e);
                if (z0) z0[k] = 0.f;
                if (z1) z1[k] = 0.f;
            }
        }
    }
}

static inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

static int soft_ce_check(const char* who, const void* logits, int64_t lsb, int64_t lst, const void* probs, int64_t psb, int64_t pst, int B,
                         int T, int K) {
    OTVAE_REQUIRE(logits && probs && B > 0, "%s: bad argument", who);
    if (T < 2 || K < 1) {
        otvae_set_error("%s: needs at least two tokens and one class (T = %d, K = %d)", who, T, K);
        return OTVAE_EUNSUPPORTED;
    }
    // rows are K contiguous values; the tensors are only read, so rows may overlap or repeat (a transposed or broadcast view)
    OTVAE_REQUIRE(lst >= 0 && pst >= 0 && lsb >= 0 && psb >= 0, "%s: negative strides (%lld, %lld) / (%lld, %lld)", who, (long long)lsb,
                  (long long)lst, (long long)psb, (long long)pst);
    return OTVAE_OK;
}

static inline bool soft_ce_vec(const void* logits, int64_t lsb, int64_t lst, const void* probs, int64_t psb, int64_t pst, int K) {
    return K % 4 == 0 && ((lsb | lst | psb | pst) & 3) == 0 && aligned16(logits) && aligned16(probs);
}

static inline int soft_ce_grid(int64_t rows, int rpb) {
    const int64_t b = (rows + rpb - 1) / rpb;
    return (int)(b < 8192 ? b : 8192);
}

extern "C" int64_t otvae_soft_ce_ws(int B, int T) { return (B > 0 && T > 1) ? (int64_t)B * (T - 1) * (int64_t)sizeof(double) : 0; }

extern "C" int otvae_soft_ce_fwd(const float* logits, int64_t logits_stride_b, int64_t logits_stride_t, const float* probs,
                                 int64_t probs_stride_b, int64_t probs_stride_t, int B, int T, int K, float* loss, float* lse, float* psum,
                                 void* ws, void* stream) {
    const int rc = soft_ce_check("otvae_soft_ce_fwd", logits, logits_stride_b, logits_stride_t, probs, probs_stride_b, probs_stride_t, B, T, K);
    if (rc != OTVAE_OK) return rc;
    OTVAE_REQUIRE(loss && lse && psum && ws && (((uintptr_t)ws) & 7) == 0, "otvae_soft_ce_fwd: outputs and an 8-byte aligned workspace are required");
    const hipStream_t st = (hipStream_t)stream;
    const int64_t rows = (int64_t)B * (T - 1);
    const bool vec = soft_ce_vec(logits, logits_stride_b, logits_stride_t, probs, probs_stride_b, probs_stride_t, K);
    double* rowloss = (double*)ws;
#define SOFT_CE_FWD(TPR, VEC)                                                                                                        \
    soft_ce_rows_kernel<TPR, VEC><<<soft_ce_grid(rows, 256 / TPR), 256, 0, st>>>(logits, logits_stride_b, logits_stride_t, probs,  \
                                                                                 probs_stride_b, probs_stride_t, B, T, K, lse, psum, rowloss)
    if (K <= SOFT_CE_WAVE_K) {
        if (vec) SOFT_CE_FWD(64, true); else SOFT_CE_FWD(64, false);
    } else {
        if (vec) SOFT_CE_FWD(256, true); else SOFT_CE_FWD(256, false);
    }
#undef SOFT_CE_FWD
    OTVAE_CHECK_LAUNCH("otvae_soft_ce_fwd");
    soft_ce_sum_kernel<<<cdiv(B, 256), 256, 0, st>>>(rowloss, B, T - 1, loss);
    OTVAE_CHECK_LAUNCH("otvae_soft_ce_fwd (sum)");
    return OTVAE_OK;
}

extern "C" int otvae_soft_ce_bwd(const float* logits, int64_t logits_stride_b, int64_t logits_stride_t, const float* probs,
                                 int64_t probs_stride_b, int64_t probs_stride_t, const float* lse, const float* psum, const float* gloss, int B,
                                 int T, int K, float* dlogits, float* dprobs, void* stream) {
    const int rc = soft_ce_check("otvae_soft_ce_bwd", logits, logits_stride_b, logits_stride_t, probs, probs_stride_b, probs_stride_t, B, T, K);
    if (rc != OTVAE_OK) return rc;
    OTVAE_REQUIRE(lse && psum && gloss, "otvae_soft_ce_bwd: lse, psum and gloss are required");
    if (!dlogits && !dprobs) return OTVAE_OK;
    const hipStream_t st = (hipStream_t)stream;
    const int64_t rows = (int64_t)B * (T - 1);
    const bool vec = soft_ce_vec(logits, logits_stride_b, logits_stride_t, probs, probs_stride_b, probs_stride_t, K) &&
                     (!dlogits || aligned16(dlogits)) && (!dprobs || aligned16(dprobs));
#define SOFT_CE_BWD(TPR, VEC)                                                                                                       \
    soft_ce_bwd_kernel<TPR, VEC><<<soft_ce_grid(rows, 256 / TPR), 256, 0, st>>>(logits, logits_stride_b, logits_stride_t, probs,   \
                                                                                probs_stride_b, probs_stride_t, lse, psum, gloss, B, T, K, \
                                                                                dlogits, dprobs)
    if (K <= SOFT_CE_WAVE_K) {
        if (vec) SOFT_CE_BWD(64, true); else SOFT_CE_BWD(64, false);
    } else {
        if (vec) SOFT_CE_BWD(256, true); else SOFT_CE_BWD(256, false);
    }
#undef SOFT_CE_BWD
    OTVAE_CHECK_LAUNCH("otvae_soft_ce_bwd");
    return OTVAE_OK;
}

// ---- one categorical draw per row: the inverse CDF of u under softmax(logits[b][pos][:]) ------------------------------------------
// Thread t owns the contiguous chunk [t * C, (t + 1) * C) of the row, C = ceil(K / 256): chunk sums in index order, the 256 chunk totals
// scanned in index order by one thread, then every thread walks its chunk again from its prefix and counts the entries whose cumulative
// sum is <= u * total.  The cumulative sums are non-decreasing, so the counts add up to the index.  exp and the scan are fp64.
__global__ __launch_bounds__(256) void categorical_sample_kernel(const float* __restrict__ logits, int64_t sb, int64_t pos_off, int K,
                                                                 const float* __restrict__ u, const int64_t* __restrict__ key, int B,
                                                                 int64_t* __restrict__ ids, int64_t ids_stride, int col) {
    __shared__ double s_sum[256];
    __shared__ double s_target;
    __shared__ float s_max[4];
    __shared__ int s_cnt[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* __restrict__ l = logits + b * sb + pos_off;
    float m = -INFINITY;
    for (int k = tid; k < K; k += 256) m = fmaxf(m, l[k]);
    m = wave_max(m);
    if ((tid & 63) == 0) s_max[tid >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
    const int C = (K + 255) / 256;
    const int k0 = tid * C < K ? tid * C : K, k1 = k0 + C < K ? k0 + C : K;
    double c = 0.0;
    for (int k = k0; k < k1; ++k) c += exp((double)l[k] - (double)m);
    s_sum[tid] = c;
    __syncthreads();
    if (tid == 0) {
        double run = 0.0;
        for (int i = 0; i < 256; ++i) {
            const double v = s_sum[i];
            s_sum[i] = run;   // exclusive prefix
            run += v;
        }
        double uu;
        if (u) {
            uu = (double)u[b];
        } else {   // 24 bits from the library's counter-based generator, centred in their cell: never 0 or 1
            const uint64_t ck = call_key(key, 0);
            const uint32_t h = mix32(row_hash(ck, (uint32_t)col * (uint32_t)B + (uint32_t)b));
            uu = ((double)(h >> 8) + 0.5) * (1.0 / 16777216.0);
        }
        s_target = uu * run;
    }
    __syncthreads();
    const double target = s_target;
    double run = s_sum[tid];
    int cnt = 0;
    for (int k = k0; k < k1; ++k) {
        run += exp((double)l[k] - (double)m);
        cnt += run <= target ? 1 : 0;
    }
    cnt = wave_sum(cnt);
    __syncthreads();
    if ((tid & 63) == 0) s_cnt[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) {
        const int idx = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        ids[b * ids_stride + col] = idx < K - 1 ? idx : K - 1;
    }
}

extern "C" int otvae_categorical_sample(const float* logits, int64_t stride_b, int64_t stride_t, int pos, int B, int K, const float* u,
                                        const int64_t* key, int64_t* ids, int64_t ids_stride, int T, int col, void* stream) {
    OTVAE_REQUIRE(logits && ids && B > 0 && (u || key), "otvae_categorical_sample: bad argument (uniforms or a generator key are required)");
    if (K < 1) {
        otvae_set_error("otvae_categorical_sample: needs at least one class (K = %d)", K);
        return OTVAE_EUNSUPPORTED;
    }
    OTVAE_REQUIRE(pos >= 0 && stride_t >= 0 && stride_b >= 0, "otvae_categorical_sample: position %d / strides (%lld, %lld) do not address a row "
                  "of %d logits", pos, (long long)stride_b, (long long)stride_t, K);
    OTVAE_REQUIRE(T >= 1 && col >= 0 && col < T && ids_stride >= T, "otvae_categorical_sample: column %d outside the [%d][%d] id matrix (row stride %lld)",
                  col, B, T, (long long)ids_stride);
    categorical_sample_kernel<<<B, 256, 0, (hipStream_t)stream>>>(logits, stride_b, (int64_t)pos * stride_t, K, u, key, B, ids,
                                                                                ids_stride, col);
    OTVAE_CHECK_LAUNCH("otvae_categorical_sample");
    return OTVAE_OK;
}

// ---- out[n][:] = codebook[ids[n]][:] ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void codebook_gather_kernel(const float* __restrict__ codebook, const int64_t* __restrict__ ids, int64_t N,
                                                              int K, int d, float* __restrict__ out) {
    const int64_t total = N * d;
    for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t n = i / d;
        const int j = (int)(i - n * d);
        const int64_t id = ids[n];
        // an id outside the codebook reads nothing: the row is NaN
        out[i] = (id >= 0 && id < K) ? codebook[id * d + j] : __int_as_float(0x7fc00000);
    }
}

extern "C" int otvae_codebook_gather(const float* codebook, const int64_t* ids, int64_t N, int K, int d, float* out, void* stream) {
    OTVAE_REQUIRE(codebook && ids && out && N > 0 && K > 0 && d > 0, "otvae_codebook_gather: bad argument");
    const int64_t blocks = (N * d + 255) / 256;
    codebook_gather_kernel<<<(int)(blocks < 4096 ? blocks : 4096), 256, 0, (hipStream_t)stream>>>(codebook, ids, N, K, d, out);
    OTVAE_CHECK_LAUNCH("otvae_codebook_gather");
    return OTVAE_OK;
}
