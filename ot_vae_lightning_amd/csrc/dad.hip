// Discrete Auto Diffuser (reference model/discrete_auto_diffuser.py:56-95): the shifted soft-label cross-entropy of its training loss,
// one categorical draw of its sampling loop -- plain, or under a temperature, top-k and top-p (nucleus) filtering --, and the row gather
// that decodes the sampled ids.
//
// soft CE.  ce[b] = sum_{t < T-1} ( -sum_k p[b][t+1][k] * log_softmax(l[b][t][:])[k] ).  The reference forms it from two sliced copies,
// two transposes, log_softmax, a product and a sum; here a row (b, t) is ONE pass over l[b][t][:] and p[b][t+1][:]: with the running
// maximum m, s = sum exp(l - m), a = sum p l and ps = sum p the row is ps * (m + log s) - a.  The shift is index arithmetic.  s, a, ps
// and the sum over t are accumulated in fp64 (the row is memory-bound: free), every reduction in a fixed order, no float atomics.
//
// Rows of up to SOFT_CE_WAVE_K entries are taken by one wave (four rows per workgroup), longer ones by a whole workgroup.
#include "common.h"
#include "dropout_hash.h"
#include "ordered_key.h"

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
//
// The filtered draw (otvae_filtered_sample) runs the same walk over other weights.  Entries are totally ordered by (logit descending,
// index ascending); as ONE unsigned number that order is the packed key (ord_f32(logit) << 32) | (0xFFFFFFFF - index), all keys of a row
// distinct.  SCALE: the weight is exp((l - m) / tau).  CUT: an entry takes part iff its packed key is >= `cut`, the key of the last entry
// the filters keep; the others weigh 0, and the clamp is to the last kept index instead of K - 1.
__device__ __forceinline__ unsigned long long packed_key(float l, int k) {
    return ((unsigned long long)ord_f32(l + 0.f) << 32) | (0xFFFFFFFFu - (unsigned)k);   // + 0.f: -0 and +0 tie
}

template <bool SCALE, bool CUT>
__device__ __forceinline__ double draw_weight(float l, int k, float m, double tau, unsigned long long cut) {
    if (CUT && packed_key(l, k) < cut) return 0.0;
    const double d = (double)l - (double)m;
    return exp(SCALE ? d / tau : d);
}

__device__ __forceinline__ float block_max_256(float m, float* s_max) {   // s_max: LDS, 4 entries; ends behind a block barrier
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = m;
    __syncthreads();
    return fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
}

// ids[b][col] = the inverse CDF of this row's uniform over the weights of l[0 .. K), m = the row's maximum.  Whole 256-thread block.
template <bool SCALE, bool CUT>
__device__ __forceinline__ void inverse_cdf_walk(const float* __restrict__ l, int K, float m, double tau, unsigned long long cut,
                                                 const float* __restrict__ u, const int64_t* __restrict__ key, int B, int b,
                                                 int64_t* __restrict__ ids, int64_t ids_stride, int col) {
    __shared__ double s_sum[256];
    __shared__ double s_target;
    __shared__ int s_cnt[4], s_last[4];
    const int tid = threadIdx.x;
    const int C = (K + 255) / 256;
    const int k0 = tid * C < K ? tid * C : K, k1 = k0 + C < K ? k0 + C : K;
    double c = 0.0;
    for (int k = k0; k < k1; ++k) c += draw_weight<SCALE, CUT>(l[k], k, m, tau, cut);
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
    int cnt = 0, last = CUT ? -1 : K - 1;
    for (int k = k0; k < k1; ++k) {
        const float lk = l[k];
        run += draw_weight<SCALE, CUT>(lk, k, m, tau, cut);
        cnt += run <= target ? 1 : 0;
        if (CUT && packed_key(lk, k) >= cut) last = k;
    }
    cnt = wave_sum(cnt);
    if (CUT) last = wave_max(last);
    __syncthreads();
    if ((tid & 63) == 0) {
        s_cnt[tid >> 6] = cnt;
        s_last[tid >> 6] = last;
    }
    __syncthreads();
    if (tid == 0) {
        const int idx = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        if (CUT) last = max(max(s_last[0], s_last[1]), max(s_last[2], s_last[3]));
        ids[b * ids_stride + col] = idx < last ? idx : last;
    }
}

__global__ __launch_bounds__(256) void categorical_sample_kernel(const float* __restrict__ logits, int64_t sb, int64_t pos_off, int K,
                                                                 const float* __restrict__ u, const int64_t* __restrict__ key, int B,
                                                                 int64_t* __restrict__ ids, int64_t ids_stride, int col) {
    __shared__ float s_max[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* __restrict__ l = logits + b * sb + pos_off;
    float m = -INFINITY;
    for (int k = tid; k < K; k += 256) m = fmaxf(m, l[k]);
    m = block_max_256(m, s_max);
    inverse_cdf_walk<false, false>(l, K, m, 1.0, 0ULL, u, key, B, b, ids, ids_stride, col);
}

// the same draw with weights exp((l - m) / temperature): what otvae_filtered_sample launches when neither top-k nor top-p takes effect
__global__ __launch_bounds__(256) void scaled_sample_kernel(const float* __restrict__ logits, int64_t sb, int64_t pos_off, int K,
                                                            const float* __restrict__ u, const int64_t* __restrict__ key, int B,
                                                            int64_t* __restrict__ ids, int64_t ids_stride, int col, float temperature,
                                                            int32_t* __restrict__ kept) {
    __shared__ float s_max[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* __restrict__ l = logits + b * sb + pos_off;
    float m = -INFINITY;
    for (int k = tid; k < K; k += 256) m = fmaxf(m, l[k]);
    m = block_max_256(m, s_max);
    if (tid == 0 && kept) kept[b] = K;
    inverse_cdf_walk<true, false>(l, K, m, (double)temperature, 0ULL, u, key, B, b, ids, ids_stride, col);
}

// ---- the filtered draw: temperature, then top-k, then top-p on the renormalised survivors ---------------------------------------------
// The row's packed keys go into LDS (8 P bytes, P = K rounded up to a power of two; the padding keys are 0, below every real key)
// and one descending bitonic network turns them into the order; steps of distance <= 64 stay inside a wave's own 128-key chunks
// (sliced_w2.hip).  The first kk = min(top_k, K) sorted entries survive top-k; their fp64 weights are summed in 256 contiguous chunks of
// the order, the chunk totals scanned by one thread, and entry j survives top-p iff (mass before j) / (mass of the kk) < top_p -- a prefix
// of r entries.  The key at rank r - 1 is the cut of the index-order walk above.  The chunk length is odd: consecutive lanes then read
// 64-bit words an odd number of words apart, which no two lanes of a 32-lane group map to one LDS bank.
#define FS_MAX_K 16384
#define FS_STATIC_LDS 4608   // the kernel's static LDS (scan scratch here and in the walk: 4176 bytes by the compiler's report), rounded up

__global__ __launch_bounds__(256) void filtered_sample_kernel(const float* __restrict__ logits, int64_t sb, int64_t pos_off, int K, int P,
                                                              const float* __restrict__ u, const int64_t* __restrict__ key, int B,
                                                              int64_t* __restrict__ ids, int64_t ids_stride, int col, float temperature,
                                                              int top_k, float top_p, int32_t* __restrict__ kept) {
    extern __shared__ __align__(16) unsigned long long fs_keys[];   // [P]
    __shared__ double s_part[256];
    __shared__ double s_total;
    __shared__ int s_cnt[4];
    __shared__ unsigned long long s_cut;
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* __restrict__ l = logits + b * sb + pos_off;
    const double tau = (double)temperature;
    for (int k = tid; k < P; k += 256) fs_keys[k] = k < K ? packed_key(l[k], k) : 0ULL;
    __syncthreads();
    const int half = P >> 1;
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < half; t += 256) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int hi = lo | j;
                const bool down = (lo & k) == 0;
                const unsigned long long a = fs_keys[lo], c = fs_keys[hi];
                const bool swap = (a < c) == down;   // both loads first, stores without a branch
                fs_keys[lo] = swap ? c : a;
                fs_keys[hi] = swap ? a : c;
            }
            const int jn = j > 1 ? j >> 1 : k;   // the next step's distance
            if (j > 64 || jn > 64) __syncthreads();
            else wave_lds_sync();
        }
    }
    __syncthreads();
    const float m = unord_f32((unsigned)(fs_keys[0] >> 32));   // the first of the order holds the row's maximum
    const int kk = top_k > 0 && top_k < K ? top_k : K;
    int r = kk;
    if (top_p < 1.f) {
        const int C = ((kk + 255) / 256) | 1;
        const int j0 = tid * C < kk ? tid * C : kk, j1 = j0 + C < kk ? j0 + C : kk;
        double c = 0.0;
        for (int j = j0; j < j1; ++j) c += exp(((double)unord_f32((unsigned)(fs_keys[j] >> 32)) - (double)m) / tau);
        s_part[tid] = c;
        __syncthreads();
        if (tid == 0) {
            double run = 0.0;
            for (int i = 0; i < 256; ++i) {
                const double v = s_part[i];
                s_part[i] = run;   // exclusive prefix
                run += v;
            }
            s_total = run;
        }
        __syncthreads();
        const double total = s_total, p = (double)top_p;
        double run = s_part[tid];
        int cnt = 0;
        for (int j = j0; j < j1; ++j) {
            cnt += run / total < p ? 1 : 0;
            run += exp(((double)unord_f32((unsigned)(fs_keys[j] >> 32)) - (double)m) / tau);
        }
        cnt = wave_sum(cnt);
        if ((tid & 63) == 0) s_cnt[tid >> 6] = cnt;
        __syncthreads();
        r = max(s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3], 1);   // the first entry is always kept
    }
    if (tid == 0) {
        s_cut = fs_keys[r - 1];
        if (kept) kept[b] = r;
    }
    __syncthreads();
    inverse_cdf_walk<true, true>(l, K, m, tau, s_cut, u, key, B, b, ids, ids_stride, col);
}

// temperature 0, or top_k = 1: the first entry of the order, i.e. the largest packed key of the row.  No limit on K.
__global__ __launch_bounds__(256) void greedy_sample_kernel(const float* __restrict__ logits, int64_t sb, int64_t pos_off, int K,
                                                            int64_t* __restrict__ ids, int64_t ids_stride, int col,
                                                            int32_t* __restrict__ kept) {
    __shared__ unsigned long long s_best[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* __restrict__ l = logits + b * sb + pos_off;
    unsigned long long best = 0ULL;
    for (int k = tid; k < K; k += 256) {
        const unsigned long long e = packed_key(l[k], k);
        best = e > best ? e : best;
    }
    best = wave_max(best);
    if ((tid & 63) == 0) s_best[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) best = s_best[w] > best ? s_best[w] : best;
        ids[b * ids_stride + col] = (int64_t)(0xFFFFFFFFu - (unsigned)best);
        if (kept) kept[b] = 1;
    }
}

static int sample_check(const char* who, const float* logits, int64_t stride_b, int64_t stride_t, int pos, int B, int K, const float* u,
                        const int64_t* key, const int64_t* ids, int64_t ids_stride, int T, int col) {
    OTVAE_REQUIRE(logits && ids && B > 0 && (u || key), "%s: bad argument (uniforms or a generator key are required)", who);
    if (K < 1) {
        otvae_set_error("%s: needs at least one class (K = %d)", who, K);
        return OTVAE_EUNSUPPORTED;
    }
    OTVAE_REQUIRE(pos >= 0 && stride_t >= 0 && stride_b >= 0, "%s: position %d / strides (%lld, %lld) do not address a row of %d logits", who,
                  pos, (long long)stride_b, (long long)stride_t, K);
    OTVAE_REQUIRE(T >= 1 && col >= 0 && col < T && ids_stride >= T, "%s: column %d outside the [%d][%d] id matrix (row stride %lld)", who, col, B,
                  T, (long long)ids_stride);
    return OTVAE_OK;
}

extern "C" int otvae_categorical_sample(const float* logits, int64_t stride_b, int64_t stride_t, int pos, int B, int K, const float* u,
                                        const int64_t* key, int64_t* ids, int64_t ids_stride, int T, int col, void* stream) {
    if (int rc = sample_check("otvae_categorical_sample", logits, stride_b, stride_t, pos, B, K, u, key, ids, ids_stride, T, col)) return rc;
    categorical_sample_kernel<<<B, 256, 0, (hipStream_t)stream>>>(logits, stride_b, (int64_t)pos * stride_t, K, u, key, B, ids,
                                                                                ids_stride, col);
    OTVAE_CHECK_LAUNCH("otvae_categorical_sample");
    return OTVAE_OK;
}

extern "C" int otvae_filtered_sample(const float* logits, int64_t stride_b, int64_t stride_t, int pos, int B, int K, const float* u,
                                     const int64_t* key, int64_t* ids, int64_t ids_stride, int T, int col, float temperature, int top_k,
                                     float top_p, int32_t* kept, void* stream) {
    const char* who = "otvae_filtered_sample";
    if (int rc = sample_check(who, logits, stride_b, stride_t, pos, B, K, u, key, ids, ids_stride, T, col)) return rc;
    OTVAE_REQUIRE(temperature >= 0.f && temperature <= 3.402823466e38f, "%s: temperature %g is not a finite number >= 0", who,
                  (double)temperature);
    OTVAE_REQUIRE(top_k >= 0, "%s: top_k = %d is negative (0 switches it off)", who, top_k);
    OTVAE_REQUIRE(top_p > 0.f && top_p <= 1.f, "%s: top_p = %g is outside (0, 1] (1 switches it off)", who, (double)top_p);
    const hipStream_t st = (hipStream_t)stream;
    const int64_t pos_off = (int64_t)pos * stride_t;
    if (temperature == 0.f || top_k == 1) {
        greedy_sample_kernel<<<B, 256, 0, st>>>(logits, stride_b, pos_off, K, ids, ids_stride, col, kept);
    } else if ((top_k == 0 || top_k >= K) && top_p == 1.f) {
        scaled_sample_kernel<<<B, 256, 0, st>>>(logits, stride_b, pos_off, K, u, key, B, ids, ids_stride, col, temperature, kept);
    } else {
        if (K > FS_MAX_K) {
            otvae_set_error("%s: top-k / top-p filtering sorts the row in LDS: K = %d is beyond the limit of %d", who, K, FS_MAX_K);
            return OTVAE_EUNSUPPORTED;
        }
        int P = 1;
        while (P < K) P <<= 1;
        const size_t lds = (size_t)P * sizeof(unsigned long long);
        // static LDS counted in: at P = 8192 the keys alone fill 64 KiB and the scan scratch comes on top
        if (int rc = otvae_lds_grant<&filtered_sample_kernel>(who, lds + FS_STATIC_LDS, (size_t)FS_MAX_K * 8 + FS_STATIC_LDS)) return rc;
        filtered_sample_kernel<<<B, 256, lds, st>>>(logits, stride_b, pos_off, K, P, u, key, B, ids, ids_stride, col, temperature, top_k,
                                                          top_p, kept);
    }
    OTVAE_CHECK_LAUNCH(who);
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
