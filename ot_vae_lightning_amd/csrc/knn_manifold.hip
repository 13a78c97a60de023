// k-nearest-neighbour manifold statistics on the device (metrics/prdc.py): improved precision / recall (Kynkaanniemi et al. 2019) and
// density / coverage (Naeem et al. 2020) from three blocks of pairwise squared distances.  fp32 features, fp64 arithmetic on the fp64
// matrix cores: d2(a, b) = max(0, (|a|^2 + |b|^2) - 2 <a, b>), <a, b> from the 128 x 128 tile of gram_tile.h (kid.hip's main loop),
// the norms from one fixed-order pass (km_norms_kernel).  The expression is symmetric in a and b and the tile hands the same products
// to the matrix cores in the same order whichever side a row is on, so d2(a, b) has the same bits in every block and in a call with
// the sets exchanged.  Every output is an order statistic, an integer count or a minimum of such values: no result depends on a
// summation order or on which workgroup ran first (no atomics, no waiting between workgroups, plain vector stores), and nothing of
// size n x n is ever in memory.
//
// otvae_knn_sq_radii -- r2[i] = the k-th smallest of { d2(x_i, x_j) : j != i } (self excluded by index: duplicates are neighbours at 0)
//   * grid (G, nt), nt = ceil(n / 128) row strips.  Workgroup (g, ti) walks the column tiles tj = g, g + G, ... of strip ti with the
//     shared main loop (a diagonal tile stages one panel) and keeps, per row, the k smallest values it has seen: an unordered list in
//     LDS (slot-major, 8 slots for k <= 8 -- the kernel then takes exactly 80 KiB and two workgroups share a CU -- or 16), touched by
//     ONE thread (thread t < 128 owns tile row t), with the list's largest value and its slot in registers.  After the main loop the
//     accumulators go through the panels' LDS half a tile at a time (128 rows x 64 columns, row stride 65 doubles: waves (0, h) and
//     (1, h) write column half h, masked to +inf where j == i or j >= n), and the row's thread scans its 64 values: one LDS read and one
//     compare per candidate; only the ~k ln(columns / k) values per row that beat the current k-th replace it (one LDS write, k
//     independent reads for the new largest).  The lists were first kept in the workspace itself: a wave pays an insertion whenever ANY
//     of its 64 rows inserts, and at global-memory latency that cost half the main loop.  At the end each list goes to
//     cand[g][i][0 .. k) of the workspace.
//   * G minimises ceil(nt G / 512) x ceil(nt / G) -- rounds of 512 resident workgroups (256 CUs x 2) times column tiles per
//     workgroup -- and is the smallest such value; G n <= 2^25 bounds the workspace.  A pure function of n.  A plain row strip gives 79
//     workgroups at n = 10000 and the even split "just enough workgroups" (G = 7: 553) runs 41 of them in a second round behind the
//     other 512, 45 % over the time of the tiles themselves (measured); the rule picks G = 79 there, one tile per
//     workgroup like kid.hip, 12.2 rounds.  Mid-sized sets walk: G = 12 at 23 or 24 strips, two column tiles per workgroup.
//   * km_merge_kernel (one thread per row) merges the G lists: the k smallest of a union do not depend on the order of merging.
//   * the symmetry of the block is NOT used: selecting along columns as well would need a second set of lists per workgroup.
// otvae_manifold_counts -- with d2_ij = d2(real_i, fake_j):
//     count_fake[j] = #{ i : d2_ij <= r2_real[i] },  hit_real[i] = any_j (d2_ij <= r2_fake[j]),  min_real[i] = min_j d2_ij
//   * grid (ntM, ntN): one 128 x 128 tile per workgroup, the epilogue in registers: counts summed down the columns (in-lane over the
//     16 rows a lane holds of a column, shuffles over the 4 lane groups), any / min along the rows (in-lane over 4 columns, shuffles
//     over 16 lanes), the two waves that share rows or columns combined through LDS.  Per-tile partials cnt[ti][j], hit[tj][i],
//     min[tj][i] go to the workspace; km_combine_kernel adds / ors / mins them (integers and minima: any order gives the same bits).
// Closed balls (<=) throughout.  Finite features are a precondition.
#include "gram_tile.h"

#define KM_MAX_K 16
#define KM_MAX_TILES 16384   // row strips per set: n <= 2^21 (grid.y, and int32 counts with room)
#define KM_SLD 65            // row stride (doubles) of the staged 128 x 64 half tile: 130 dwords = 2 mod 64 banks
#define KM_TARGET_WG 512     // 256 CUs x 2 resident workgroups
#define KM_MAX_LISTS ((int64_t)1 << 25)   // G n <= 2^25 candidate lists: the workspace stays below 4 GiB at k = 16

static_assert(GT_T * KM_SLD <= 2 * GT_T * GT_LD, "the staged half tile must fit the two panels");

static bool km_set_ok(int64_t n, int D, int k) {
    return k >= 1 && k <= KM_MAX_K && n > k && D >= 1 && D <= GT_MAX_D && cdiv(n, GT_T) <= KM_MAX_TILES && n <= ((int64_t)1 << 21);
}
// G: the split of a strip's nt column tiles that finishes first when nt G workgroups of ceil(nt / G) tiles each run KM_TARGET_WG at
// a time -- rounds x tiles per workgroup --, the smallest such G (fewest lists to merge), among those whose lists stay below
// KM_MAX_LISTS rows.  A pure function of n.
static int km_groups(int64_t n) {
    const int nt = cdiv(n, GT_T);
    const int cap = imax(1, imin(nt, (int)(KM_MAX_LISTS / n)));
    int best = 1;
    int64_t best_cost = INT64_MAX;
    for (int G = 1; G <= cap; ++G) {
        const int64_t cost = (int64_t)cdiv((int64_t)nt * G, KM_TARGET_WG) * cdiv(nt, G);
        if (cost < best_cost) {
            best_cost = cost;
            best = G;
        }
    }
    return best;
}

extern "C" int otvae_knn_groups(int64_t n) { return n >= 1 && n <= ((int64_t)1 << 21) ? km_groups(n) : -1; }

extern "C" int64_t otvae_knn_sq_radii_ws(int64_t n, int D, int k) {
    if (!km_set_ok(n, D, k)) return -1;
    return (n + (int64_t)km_groups(n) * n * k) * (int64_t)sizeof(double);
}

extern "C" int64_t otvae_manifold_counts_ws(int64_t n_real, int64_t n_fake, int D) {
    if (!km_set_ok(n_real, D, 1) || !km_set_ok(n_fake, D, 1)) return -1;
    const int64_t ntn = cdiv(n_real, GT_T), ntm = cdiv(n_fake, GT_T);
    return (n_real + n_fake + ntm * n_real) * (int64_t)sizeof(double) + (ntn * n_fake + ntm * n_real) * (int64_t)sizeof(int32_t);
}

__device__ __forceinline__ double km_inf() { return __longlong_as_double(0x7ff0000000000000LL); }

// one wave per row: |x_i|^2 in fp64, lane-strided fused multiply-adds and a butterfly -- one fixed order per row
__global__ __launch_bounds__(256) void km_norms_kernel(const float* __restrict__ x, int64_t n, int D, double* __restrict__ nrm) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const float* __restrict__ p = x + row * D;
    double s = 0.0;
    for (int d = threadIdx.x & 63; d < D; d += 64) {
        const double v = (double)p[d];
        s = fma(v, v, s);
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) nrm[row] = s;
}

// v replaces the largest of the k values L[0], L[stride], ... (at slot pos); thr / pos = the largest afterwards and its slot.  The k
// reads do not depend on one another.  A list that starts as k times +inf is "not full yet" with no further bookkeeping.
__device__ __forceinline__ void km_insert(double* L, int stride, int k, double v, double& thr, int& pos) {
    L[pos * stride] = v;
    double m = L[0];
    int at = 0;
#pragma unroll 4
    for (int s = 1; s < k; ++s) {
        const double u = L[s * stride];
        at = u > m ? s : at;
        m = u > m ? u : m;
    }
    thr = m;
    pos = at;
}

// grid (G, nt): header.  KCAP: list slots in LDS (8: k <= 8, the whole kernel stays at 80 KiB, two workgroups per CU; 16: one)
template <bool VEC, int KCAP>
__global__ __launch_bounds__(256, KCAP <= 8 ? 2 : 1) void km_select_kernel(const float* __restrict__ x, const double* __restrict__ nrm, int n, int D, int k,
                                                        int nt, double* __restrict__ cand) {
    __shared__ __attribute__((aligned(16))) double panels[2][GT_T][GT_LD];
    __shared__ int64_t row_a[GT_T], row_b[GT_T];
    __shared__ double na_s[GT_T], nb_s[GT_T];
    __shared__ double lists[KCAP][GT_T];               // slot-major: thread t's list is lists[.][t], no bank shared with a neighbour
    double (*d2s)[KM_SLD] = reinterpret_cast<double (*)[KM_SLD]>(&panels[0][0][0]);
    const int g = blockIdx.x, G = gridDim.x, ti = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l16 = lane & 15, lk = lane >> 4;
    const int wr = wave >> 1, wc = wave & 1;
    const int i0 = ti * GT_T;

    const int my_i = i0 + tid;                         // threads 0 .. 127: the row whose list this thread keeps
    const bool owner = tid < GT_T && my_i < n;
    double* L = &lists[0][tid & (GT_T - 1)];
    double thr = km_inf();
    int pos = 0;
    if (tid < GT_T) {
        for (int s = 0; s < k; ++s) L[s * GT_T] = km_inf();
        row_a[tid] = my_i < n ? (int64_t)my_i * D : -1;
        na_s[tid] = my_i < n ? nrm[my_i] : 0.0;
    }

    for (int tj = g; tj < nt; tj += G) {
        const int j0 = tj * GT_T;
        if (tid >= GT_T) {
            const int j = j0 + tid - GT_T;
            row_b[tid - GT_T] = j < n ? (int64_t)j * D : -1;
            nb_s[tid - GT_T] = j < n ? nrm[j] : 0.0;
        }
        __syncthreads();
        f64x4 acc[4][4];
        gram_tile_mma<VEC>(x, x, row_a, row_b, D, ti == tj, panels[0], panels[1], acc);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (wc == h) {
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int col = b * 16 + l16, j = j0 + h * 64 + col;
                    const double nb = nb_s[h * 64 + col];
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = wr * 64 + a * 16 + 4 * r + lk;
                            double v = (na_s[row] + nb) - 2.0 * acc[a][b][r];
                            v = v < 0.0 ? 0.0 : v;
                            d2s[row][col] = (j >= n || j == i0 + row) ? km_inf() : v;
                        }
                }
            }
            __syncthreads();
            if (owner) {
#pragma unroll 8
                for (int c = 0; c < 64; ++c) {
                    const double v = d2s[tid][c];
                    if (v < thr) km_insert(L, GT_T, k, v, thr, pos);
                }
            }
            __syncthreads();
        }
    }
    if (owner) {
        double* __restrict__ out = cand + ((size_t)g * n + my_i) * k;
        for (int s = 0; s < k; ++s) out[s] = L[s * GT_T];
    }
}

// one thread per row: the k smallest of the G lists (unordered, +inf where a workgroup saw fewer than k columns)
__global__ __launch_bounds__(64) void km_merge_kernel(const double* __restrict__ cand, int n, int k, int G, double* __restrict__ r2) {
    __shared__ double Ls[KM_MAX_K][64];
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    double* L = &Ls[0][threadIdx.x];
    for (int s = 0; s < k; ++s) L[s * 64] = km_inf();
    double thr = km_inf();
    int pos = 0;
    for (int g = 0; g < G; ++g) {
        const double* __restrict__ c = cand + ((size_t)g * n + i) * k;
        for (int s = 0; s < k; ++s) {
            const double v = c[s];
            if (v < thr) km_insert(L, 64, k, v, thr, pos);
        }
    }
    r2[i] = thr;
}

// grid (ntM, ntN): header
template <bool VEC>
__global__ __launch_bounds__(256, 2) void km_count_kernel(const float* __restrict__ real, const double* __restrict__ nrm_real,
                                                       const double* __restrict__ r2_real, int N, const float* __restrict__ fake,
                                                       const double* __restrict__ nrm_fake, const double* __restrict__ r2_fake, int M,
                                                       int D, int32_t* __restrict__ ws_cnt, int32_t* __restrict__ ws_hit,
                                                       double* __restrict__ ws_min) {
    __shared__ __attribute__((aligned(16))) double panels[2][GT_T][GT_LD];
    __shared__ int64_t row_a[GT_T], row_b[GT_T];
    __shared__ double na_s[GT_T], nb_s[GT_T], ra_s[GT_T], rb_s[GT_T];
    __shared__ double min_s[2][GT_T];
    __shared__ int32_t hit_s[2][GT_T], cnt_s[2][GT_T];
    const int tj = blockIdx.x, ti = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l16 = lane & 15, lk = lane >> 4;
    const int wr = wave >> 1, wc = wave & 1;
    const int i0 = ti * GT_T, j0 = tj * GT_T;

    if (tid < GT_T) {
        const int i = i0 + tid;
        row_a[tid] = i < N ? (int64_t)i * D : -1;
        na_s[tid] = i < N ? nrm_real[i] : km_inf();   // a row or column beyond the set: d2 = +inf, in no ball, under no minimum
        ra_s[tid] = i < N ? r2_real[i] : -1.0;
    } else {
        const int c = tid - GT_T, j = j0 + c;
        row_b[c] = j < M ? (int64_t)j * D : -1;
        nb_s[c] = j < M ? nrm_fake[j] : km_inf();
        rb_s[c] = j < M ? r2_fake[j] : -1.0;
    }
    __syncthreads();
    f64x4 acc[4][4];
    gram_tile_mma<VEC>(real, fake, row_a, row_b, D, false, panels[0], panels[1], acc);

    double nb[4], rb[4];
    int cnt[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int col = wc * 64 + b * 16 + l16;
        nb[b] = nb_s[col];
        rb[b] = rb_s[col];
        cnt[b] = 0;
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = wr * 64 + a * 16 + 4 * r + lk;
            const double na = na_s[row], ra = ra_s[row];
            int hit = 0;
            double mn = km_inf();
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                double v = (na + nb[b]) - 2.0 * acc[a][b][r];
                v = v < 0.0 ? 0.0 : v;
                cnt[b] += v <= ra ? 1 : 0;
                hit |= v <= rb[b] ? 1 : 0;
                mn = v < mn ? v : mn;
            }
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {
                hit |= __shfl_xor(hit, o, 64);
                const double w = __shfl_xor(mn, o, 64);
                mn = w < mn ? w : mn;
            }
            if (l16 == 0) {
                hit_s[wc][row] = hit;
                min_s[wc][row] = mn;
            }
        }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        int c = cnt[b];
        c += __shfl_xor(c, 16, 64);
        c += __shfl_xor(c, 32, 64);
        if (lk == 0) cnt_s[wr][wc * 64 + b * 16 + l16] = c;
    }
    __syncthreads();
    if (tid < GT_T) {
        const int i = i0 + tid;
        if (i < N) {
            ws_hit[(size_t)tj * N + i] = hit_s[0][tid] | hit_s[1][tid];
            const double p = min_s[0][tid], q = min_s[1][tid];
            ws_min[(size_t)tj * N + i] = q < p ? q : p;
        }
    } else {
        const int c = tid - GT_T, j = j0 + c;
        if (j < M) ws_cnt[(size_t)ti * M + j] = cnt_s[0][c] + cnt_s[1][c];
    }
}

// thread e < N: real row e (or / min over the column tiles); thread e >= N: fake row e - N (sum over the row tiles)
__global__ __launch_bounds__(256) void km_combine_kernel(const int32_t* __restrict__ ws_cnt, const int32_t* __restrict__ ws_hit,
                                                         const double* __restrict__ ws_min, int N, int M, int ntn, int ntm,
                                                         int32_t* __restrict__ count_fake, int32_t* __restrict__ hit_real,
                                                         double* __restrict__ min_real) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < N) {
        int hit = 0;
        double mn = km_inf();
        for (int t = 0; t < ntm; ++t) {
            hit |= ws_hit[(size_t)t * N + e];
            const double v = ws_min[(size_t)t * N + e];
            mn = v < mn ? v : mn;
        }
        hit_real[e] = hit;
        min_real[e] = mn;
    } else if (e < (int64_t)N + M) {
        const int64_t j = e - N;
        int c = 0;
        for (int t = 0; t < ntn; ++t) c += ws_cnt[(size_t)t * M + j];
        count_fake[j] = c;
    }
}

extern "C" int otvae_knn_sq_radii(const float* x, int64_t n, int D, int k, double* r2, void* ws, void* stream) {
    OTVAE_REQUIRE(x && r2 && ws, "otvae_knn_sq_radii: null pointer");
    OTVAE_REQUIRE(km_set_ok(n, D, k), "otvae_knn_sq_radii: need 1 <= k <= %d, k < n <= 2^21, 1 <= D <= %d (got n = %lld, D = %d, k = %d)",
                  KM_MAX_K, GT_MAX_D, (long long)n, D, k);
    hipStream_t st = (hipStream_t)stream;
    const int nt = cdiv(n, GT_T), G = km_groups(n);
    double* nrm = (double*)ws;
    double* cand = nrm + n;
    km_norms_kernel<<<cdiv(n, 4), 256, 0, st>>>(x, n, D, nrm);
    const dim3 grid(G, nt);
    const bool vec = D % 4 == 0 && ((uintptr_t)x & 15) == 0;
    if (k <= 8) {
        if (vec) km_select_kernel<true, 8><<<grid, 256, 0, st>>>(x, nrm, (int)n, D, k, nt, cand);
        else km_select_kernel<false, 8><<<grid, 256, 0, st>>>(x, nrm, (int)n, D, k, nt, cand);
    } else {
        if (vec) km_select_kernel<true, KM_MAX_K><<<grid, 256, 0, st>>>(x, nrm, (int)n, D, k, nt, cand);
        else km_select_kernel<false, KM_MAX_K><<<grid, 256, 0, st>>>(x, nrm, (int)n, D, k, nt, cand);
    }
    km_merge_kernel<<<cdiv(n, 64), 64, 0, st>>>(cand, (int)n, k, G, r2);
    OTVAE_CHECK_LAUNCH("otvae_knn_sq_radii");
    return OTVAE_OK;
}

extern "C" int otvae_manifold_counts(const float* real, const double* r2_real, int64_t n_real, const float* fake, const double* r2_fake,
                                     int64_t n_fake, int D, int32_t* count_fake, int32_t* hit_real, double* min_real, void* ws,
                                     void* stream) {
    OTVAE_REQUIRE(real && r2_real && fake && r2_fake && count_fake && hit_real && min_real && ws, "otvae_manifold_counts: null pointer");
    OTVAE_REQUIRE(km_set_ok(n_real, D, 1) && km_set_ok(n_fake, D, 1), "otvae_manifold_counts: need 2 <= rows <= 2^21 per side, 1 <= D <= %d "
                  "(got %lld and %lld rows, D = %d)", GT_MAX_D, (long long)n_real, (long long)n_fake, D);
    hipStream_t st = (hipStream_t)stream;
    const int N = (int)n_real, M = (int)n_fake, ntn = cdiv(N, GT_T), ntm = cdiv(M, GT_T);
    double* nrm_real = (double*)ws;
    double* nrm_fake = nrm_real + N;
    double* ws_min = nrm_fake + M;
    int32_t* ws_hit = (int32_t*)(ws_min + (size_t)ntm * N);
    int32_t* ws_cnt = ws_hit + (size_t)ntm * N;
    km_norms_kernel<<<cdiv(N, 4), 256, 0, st>>>(real, N, D, nrm_real);
    km_norms_kernel<<<cdiv(M, 4), 256, 0, st>>>(fake, M, D, nrm_fake);
    const dim3 grid(ntm, ntn);
    if (D % 4 == 0 && (((uintptr_t)real | (uintptr_t)fake) & 15) == 0)
        km_count_kernel<true><<<grid, 256, 0, st>>>(real, nrm_real, r2_real, N, fake, nrm_fake, r2_fake, M, D, ws_cnt, ws_hit, ws_min);
    else
        km_count_kernel<false><<<grid, 256, 0, st>>>(real, nrm_real, r2_real, N, fake, nrm_fake, r2_fake, M, D, ws_cnt, ws_hit, ws_min);
    km_combine_kernel<<<cdiv((int64_t)N + M, 256), 256, 0, st>>>(ws_cnt, ws_hit, ws_min, N, M, ntn, ntm, count_fake, hit_real, min_real);
    OTVAE_CHECK_LAUNCH("otvae_manifold_counts");
    return OTVAE_OK;
}
