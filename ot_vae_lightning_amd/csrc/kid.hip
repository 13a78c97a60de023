// Kernel Inception Distance on the device (metrics/kid.py): the unbiased polynomial-kernel MMD^2 of S random subsets in one entry, and
// the append-only feature store its metric keeps.  fp32 features, fp64 arithmetic on the fp64 matrix cores, every sum in a fixed
// order (no float atomics, no cross-workgroup waiting, plain vector stores): results are run-to-run identical, and every entry can
// be captured into a hipGraph.
//
// otvae_poly_mmd_subsets -- per subset s with x_i = real[idx_real[s][i]], y_j = fake[idx_fake[s][j]], k(a, b) = (gamma <a, b> + coef)^degree:
//   per_subset[s] = (sum_{i != j} k(x_i, x_j) + sum_{i != j} k(y_i, y_j)) / (m (m - 1)) - 2 sum_{i, j} k(x_i, y_j) / m^2
//   * grid (tile, subset).  Per subset the lower-triangular 128 x 128 tiles of XX and of YY (an off-diagonal tile counts twice, a
//     diagonal tile masks i == j) and all tiles of XY: 2 nt (nt + 1) / 2 + nt^2 workgroups with nt = ceil(m / 128).
//   * a workgroup of 4 waves; wave (wr, wc) owns the 64 x 64 quarter (wr, wc) of the tile as 4 x 4 v_mfma_f64_16x16x4_f64 accumulators
//     (operand / result layout as in metrics.hip: lane l supplies A[l % 16][l / 16] and B[l / 16][l % 16], register r of lane l holds
//     D[4 r + l / 16][l % 16]): 8 LDS reads feed 16 MFMAs.
//   * (this and the item above are gram_tile.h, which knn_manifold.hip shares) the features are walked in chunks of 32: both gathered 128 x 32 row panels (one on a diagonal tile) go through LDS once per
//     chunk, converted to fp64 while staged.  The gather is at the load: a thread reads real[idx[row]][k0 + k ...], 8 lanes one
//     128-byte row segment with 16-byte loads (D a multiple of 4, 16-byte aligned bases: 11 % faster at D = 2048 than the 4-byte
//     form, which remains for every other D, 32 lanes per segment); no [S][m][D] array ever exists.  LDS is row-major with a row stride of 34 doubles (68 dwords = 4 mod 64
//     banks: the 16 rows x 2 k a half-wave's ds_read_b64 touches fall into 64 distinct banks).  The next chunk's global loads are
//     issued before the current chunk's MFMAs.
//   * why 128 x 128 and not metrics.hip's 64 x 64: a 64 x 64 tile loads 16 KiB of panel per 0.26 MFLOP (16 FLOP / byte), which at the
//     fp64 matrix rate asks ~5 TB/s of the cache hierarchy for a working set (2 x 10000 x 2048 fp32 = 160 MB) that only the
//     Infinity Cache holds; 128 x 128 halves that demand, and its 128 accumulator registers still leave two workgroups per CU.
//   * the epilogue applies k by repeated multiplication, masks rows >= m (and i == j), and sums the tile in an order that does not
//     change when the tile is transposed: inside a 16 x 16 MFMA block every lane adds the transposed element to its own
//     (V + V^T, fetched by lane shuffles), the 8 x 8 block sums of the tile are added as diagonal + (b[p][q] + b[q][p]), and the second
//     launch adds the XY tiles as diagonal + (P[ti][tj] + P[tj][ti]).  Exchanging real and fake (with their index arrays) therefore
//     gives the same bits: XX and YY trade places, and XY becomes its transpose.  One fp64 partial per tile goes to ws.
//   * a second launch (one workgroup per subset) adds the subset's partials in index order into per_subset; a third (one workgroup)
//     forms stats = {mean (summed in double-double), population std (two passes about per_subset[0])}.
// otvae_feature_append -- rows to buf[count[0] ...], the offset read on the device; a single-thread launch then advances the counts.
#include "gram_tile.h"

#define PM_T GT_T           // output tile, LDS row stride and the widest features: the shared tile's (gram_tile.h)
#define PM_LD GT_LD
#define PM_MAX_D GT_MAX_D
#define PM_MAX_DEGREE 8
#define PM_MAX_S 65535

static bool pm_valid(int S, int m, int D) { return S >= 1 && m >= 2 && D >= 1; }
static bool pm_supported(int S, int m, int D) { return S <= PM_MAX_S && D <= PM_MAX_D && cdiv(m, PM_T) <= 16384; }
static int64_t pm_tiles(int m) {
    const int64_t nt = cdiv(m, PM_T);
    return nt * (nt + 1) + nt * nt;
}

extern "C" int64_t otvae_poly_mmd_ws(int S, int m, int D) {
    if (!pm_valid(S, m, D) || !pm_supported(S, m, D)) return -1;
    return (int64_t)S * pm_tiles(m) * (int64_t)sizeof(double);
}

__device__ __forceinline__ void pm_tile_of(int t, int& ti, int& tj) {
    ti = (int)((sqrtf(8.f * (float)t + 1.f) - 1.f) * 0.5f);
    while (ti * (ti + 1) / 2 > t) --ti;
    while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
    tj = t - ti * (ti + 1) / 2;
}

// the same value on every thread: per-wave butterfly, then the four wave sums in index order
__device__ __forceinline__ double pm_block_sum(double v, double* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// grid (tiles, S): tile t < ntri: XX, t < 2 ntri: YY (both lower-triangular), else XY (row-major over nt x nt)
template <bool VEC>
__global__ __launch_bounds__(256, 2) void pm_tile_kernel(const float* __restrict__ real, int64_t n_real, const float* __restrict__ fake,
                                                      int64_t n_fake, int D, const int32_t* __restrict__ idx_real,
                                                      const int32_t* __restrict__ idx_fake, int m, int nt, int degree, double gamma,
                                                      double coef, double* __restrict__ ws) {
    __shared__ __attribute__((aligned(16))) double as[PM_T][PM_LD], bs_[PM_T][PM_LD];
    __shared__ double blk[8][8];
    __shared__ int64_t row_a[PM_T], row_b[PM_T];   // element offset of the gathered row, -1: beyond the subset
    const int ntri = nt * (nt + 1) / 2;
    const int s = blockIdx.y;
    int t = blockIdx.x, kind = 0, ti, tj;
    if (t >= 2 * ntri) {
        kind = 2;
        t -= 2 * ntri;
        ti = t / nt;
        tj = t - ti * nt;
    } else {
        if (t >= ntri) {
            kind = 1;
            t -= ntri;
        }
        pm_tile_of(t, ti, tj);
    }
    const bool diag = kind != 2 && ti == tj;
    const float* __restrict__ pa = kind == 1 ? fake : real;
    const float* __restrict__ pb = kind == 0 ? real : fake;
    const int32_t* ia = kind == 1 ? idx_fake : idx_real;
    const int32_t* ib = kind == 0 ? idx_real : idx_fake;
    const int64_t na = kind == 1 ? n_fake : n_real, nb = kind == 0 ? n_real : n_fake;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l16 = lane & 15, lk = lane >> 4;
    const int wr = wave >> 1, wc = wave & 1;
    const int i0 = ti * PM_T, j0 = tj * PM_T;

    if (tid < PM_T) {
        const int i = i0 + tid;
        int64_t r = -1;
        if (i < m) {
            r = ia ? (int64_t)ia[(size_t)s * m + i] : (int64_t)i;
            r = r < 0 ? 0 : (r >= na ? na - 1 : r);
            r *= D;
        }
        row_a[tid] = r;
    } else {
        const int j = j0 + tid - PM_T;
        int64_t r = -1;
        if (j < m) {
            r = ib ? (int64_t)ib[(size_t)s * m + j] : (int64_t)j;
            r = r < 0 ? 0 : (r >= nb ? nb - 1 : r);
            r *= D;
        }
        row_b[tid - PM_T] = r;
    }
    __syncthreads();

    f64x4 acc[4][4];
    gram_tile_mma<VEC>(pa, pb, row_a, row_b, D, diag, as, bs_, acc);   // gram_tile.h: staging and the MFMA main loop

    // epilogue: k, masks, transposition-invariant sums (header)
    const int src_hi = (l16 & 3) * 16 + lk;   // lane holding the transposed element of register r: src_hi + 4 r, its register l16 / 4
    const int src_reg = l16 >> 2;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            double v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = i0 + wr * 64 + a * 16 + 4 * r + lk, j = j0 + wc * 64 + b * 16 + l16;
                const double g = fma(gamma, acc[a][b][r], coef);
                double k = g;
                for (int d = 1; d < degree; ++d) k *= g;
                v[r] = (i < m && j < m && !(diag && i == j)) ? k : 0.0;
            }
            double sum = 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double tr = 0.0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const double got = __shfl(v[q], src_hi + 4 * r, 64);
                    tr = src_reg == q ? got : tr;
                }
                sum += v[r] + tr;
            }
            sum = wave_sum(sum);
            if (lane == 0) blk[wr * 4 + a][wc * 4 + b] = sum;
        }
    __syncthreads();
    if (tid == 0) {
        double p = 0.0;
        for (int q = 0; q < 8; ++q) p += blk[q][q];
        for (int q = 1; q < 8; ++q)
            for (int r = 0; r < q; ++r) p += blk[q][r] + blk[r][q];
        // every element was added twice (V + V^T); an off-diagonal tile of the symmetric XX / YY stands for its mirror image as well
        ws[(size_t)s * gridDim.x + blockIdx.x] = (kind != 2 && !diag) ? p : 0.5 * p;
    }
}

// grid (S): the subset's tile partials in index order
__global__ __launch_bounds__(256) void pm_subset_kernel(const double* __restrict__ ws, int m, int nt, double* __restrict__ per_subset) {
    __shared__ double red[4];
    const int ntri = nt * (nt + 1) / 2;
    const int tiles = 2 * ntri + nt * nt;
    const double* w = ws + (size_t)blockIdx.x * tiles;
    double xx = 0.0, yy = 0.0, xy = 0.0;
    for (int t = threadIdx.x; t < ntri; t += 256) {
        xx += w[t];
        yy += w[ntri + t];
        int ti, tj;
        pm_tile_of(t, ti, tj);
        const double* c = w + 2 * ntri;
        xy += ti == tj ? c[ti * nt + ti] : c[ti * nt + tj] + c[tj * nt + ti];
    }
    xx = pm_block_sum(xx, red);
    yy = pm_block_sum(yy, red);
    xy = pm_block_sum(xy, red);
    if (threadIdx.x == 0) {
        const double dm = (double)m;
        per_subset[blockIdx.x] = (xx + yy) / (dm * (dm - 1.0)) - 2.0 * xy / (dm * dm);
    }
}

// s + e == a + b exactly (Knuth's TwoSum)
__device__ __forceinline__ void pm_two_sum(double a, double b, double& s, double& e) {
    s = a + b;
    const double bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}

// one workgroup: mean and population std of v[0 .. S - 1].  Unbiased estimates scatter around zero, so the mean may be small against
// its terms: it is summed in double-double (per thread, then the 256 pairs in index order by one thread).  The std is taken about the
// pivot v[0] in two passes: it stays accurate when it is small against the mean.
__global__ __launch_bounds__(256) void pm_stats_kernel(const double* __restrict__ v, int S, double* __restrict__ stats) {
    __shared__ double red[4];
    __shared__ double part_hi[256], part_lo[256];
    const double pivot = v[0];
    double d = 0.0, hi = 0.0, lo = 0.0;
    for (int s = threadIdx.x; s < S; s += 256) {
        double e;
        pm_two_sum(hi, v[s], hi, e);
        lo += e;
        d += v[s] - pivot;
    }
    part_hi[threadIdx.x] = hi;
    part_lo[threadIdx.x] = lo;
    const double dbar = pm_block_sum(d, red) / (double)S;   // (its barriers also publish part_hi / part_lo)
    if (threadIdx.x == 0) {
        double h = 0.0, l = 0.0;
        for (int i = 0; i < 256; ++i) {
            double e;
            pm_two_sum(h, part_hi[i], h, e);
            l += e + part_lo[i];
        }
        stats[0] = (h + l) / (double)S;
    }
    double q = 0.0;
    for (int s = threadIdx.x; s < S; s += 256) {
        const double e = (v[s] - pivot) - dbar;
        q = fma(e, e, q);
    }
    q = pm_block_sum(q, red);
    if (threadIdx.x == 0) stats[1] = sqrt(q / (double)S);
}

extern "C" int otvae_poly_mmd_subsets(const float* real, int64_t n_real, const float* fake, int64_t n_fake, int D, const int32_t* idx_real,
                                      const int32_t* idx_fake, int S, int m, int degree, double gamma, double coef, void* ws,
                                      double* per_subset, double* stats, void* stream) {
    OTVAE_REQUIRE(real && fake && ws && per_subset && stats, "otvae_poly_mmd_subsets: null pointer");
    OTVAE_REQUIRE((idx_real == nullptr) == (idx_fake == nullptr), "otvae_poly_mmd_subsets: idx_real and idx_fake come together");
    OTVAE_REQUIRE(pm_valid(S, m, D) && n_real >= m && n_fake >= m, "otvae_poly_mmd_subsets: need S >= 1, D >= 1, 2 <= m <= min(n_real, n_fake)"
                  " (got S = %d, D = %d, m = %d, n = %lld / %lld)", S, D, m, (long long)n_real, (long long)n_fake);
    OTVAE_REQUIRE(degree >= 1 && gamma == gamma && coef == coef, "otvae_poly_mmd_subsets: degree must be >= 1, gamma and coef numbers");
    if (!pm_supported(S, m, D) || degree > PM_MAX_DEGREE) {
        otvae_set_error("otvae_poly_mmd_subsets: S = %d, m = %d, D = %d, degree = %d is beyond the envelope (S <= %d, D <= %d, degree <= %d)",
                        S, m, D, degree, PM_MAX_S, PM_MAX_D, PM_MAX_DEGREE);
        return OTVAE_EUNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    const int nt = cdiv(m, PM_T);
    const dim3 grid((unsigned)pm_tiles(m), S);
    if (D % 4 == 0 && (((uintptr_t)real | (uintptr_t)fake) & 15) == 0)
        pm_tile_kernel<true><<<grid, 256, 0, st>>>(real, n_real, fake, n_fake, D, idx_real, idx_fake, m, nt, degree, gamma, coef, (double*)ws);
    else
        pm_tile_kernel<false><<<grid, 256, 0, st>>>(real, n_real, fake, n_fake, D, idx_real, idx_fake, m, nt, degree, gamma, coef, (double*)ws);
    pm_subset_kernel<<<S, 256, 0, st>>>((const double*)ws, m, nt, per_subset);
    pm_stats_kernel<<<1, 256, 0, st>>>(per_subset, S, stats);
    OTVAE_CHECK_LAUNCH("otvae_poly_mmd_subsets");
    return OTVAE_OK;
}

// ================================================================================================ feature store
// row b of the call goes to row count[0] + b of buf when that is below the capacity; count is only read here
template <typename TIN>
__global__ __launch_bounds__(256) void fa_copy_kernel(const TIN* __restrict__ f, int B, int D, float* __restrict__ buf, int64_t capacity,
                                                      const int64_t* __restrict__ count) {
    int64_t stored = count[0];
    stored = stored < 0 ? 0 : stored;
    int64_t rows = capacity - stored;
    rows = rows < 0 ? 0 : (rows > B ? B : rows);
    const int64_t n = rows * D;
    float* __restrict__ dst = buf + stored * D;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) dst[e] = (float)f[e];
}

__global__ void fa_count_kernel(int B, int64_t capacity, int64_t* __restrict__ count) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        int64_t stored = count[0];
        stored = stored < 0 ? 0 : stored;
        stored += B;
        count[0] = stored > capacity ? capacity : stored;
        count[1] += B;
    }
}

extern "C" int otvae_feature_append(int in_dtype, const void* feats, int B, int D, float* buf, int64_t capacity, int64_t* count,
                                    void* stream) {
    OTVAE_REQUIRE(feats && buf && count && B > 0 && D > 0 && capacity > 0, "otvae_feature_append: bad argument");
    OTVAE_REQUIRE(in_dtype == 0 || in_dtype == 1, "otvae_feature_append: in_dtype must be 0 (fp32) or 1 (fp64)");
    hipStream_t st = (hipStream_t)stream;
    const int blocks = imax(1, imin(2048, cdiv((int64_t)B * D, 256 * 4)));
    if (in_dtype == 0) fa_copy_kernel<float><<<blocks, 256, 0, st>>>((const float*)feats, B, D, buf, capacity, count);
    else fa_copy_kernel<double><<<blocks, 256, 0, st>>>((const double*)feats, B, D, buf, capacity, count);
    fa_count_kernel<<<1, 64, 0, st>>>(B, capacity, count);
    OTVAE_CHECK_LAUNCH("otvae_feature_append");
    return OTVAE_OK;
}
