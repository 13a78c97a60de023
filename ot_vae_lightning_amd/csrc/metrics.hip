// Validation metrics on the device (the package's metrics/ module):
//   * streaming feature moments (n, sum f, sum f f^T in fp64) of the Frechet distance -- the reference's
//     FrechetInceptionDistance._extract_features / update (metrics/fid.py:99-122) feeding mean_cov (ot/matrix_utils.py:145-158)
//   * sum of squared errors, element count and the target's running range of PeakSignalNoiseRatio
// Everything is reduced in a fixed order (no float atomics): results are run-to-run identical.  No host synchronisation, plain
// vector stores only: every entry can be captured into a hipGraph.
//
// otvae_moments_accum -- sum_xx += F^T F for F [B][D], D <= 2048 (feature widths 64 ... 2048; otvae_gauss_stats was written for latent
// widths and computes both triangles with scalar FMAs behind a ksplit * (D+1)^2 * 8 byte workspace):
//   * 64 x 64 output tiles, only those with tile_i >= tile_j; a workgroup of 4 waves, wave w owns rows 16 w .. 16 w + 15 of the tile as
//     4 v_mfma_f64_16x16x4_f64 accumulators (operand / result layout as gemm_f64_mfma_kernel, gaussian_ot.hip: lane l supplies
//     A[l % 16][l / 16] and B[l / 16][l % 16], register r of lane l holds D[4 r + l / 16][l % 16]);
//   * the batch is walked in chunks of 32 rows: both 32 x 64 feature panels go through LDS once per workgroup tile (one panel on a
//     diagonal tile), converted to fp64 while staged, k-major with a row stride of 80 doubles so that the two k-rows a ds_read_b64
//     lane group touches fall into disjoint bank halves; the next chunk's global loads are issued before the current chunk's MFMAs;
//   * sum f comes from the diagonal tiles as one more accumulator against a B operand of ones (same pipe, same order);
//   * the strict upper triangle is never computed: every element (i, j), i >= j, is stored to [i][j] and [j][i], so the state stays
//     bit-symmetric;
//   * wide features have enough tiles to fill the chip (528 at D = 2048) and each workgroup adds its tile into the state itself: no
//     workspace, one launch.  Narrow ones split the batch over up to MA_KSPLIT_MAX = 8 workgroups per tile, whose partial TILES
//     (lower triangle only) go to the workspace and are added in split order by a second, short launch.
//     Workspace: at most 8 * (nt (nt + 1) / 2 * 4096 + nt * 64) doubles with nt = ceil(D / 64) and only while nt (nt + 1) / 2 < 512,
//     i.e. at most (4 * D64^2 + 264 * D64) * 8 bytes (D64 = D rounded up to 64) whatever B is -- below 4.2 * D^2 * 8 from D = 1024
//     on; at D = 2048: none.
#include "common.h"

#define MA_T 64              // output tile
#define MA_KC 32             // batch rows per staged chunk
#define MA_LD 80             // LDS row stride (doubles): 80 * 2 dwords = 32 mod 64 banks
#define MA_KSPLIT_MAX 8
#define MA_MAX_D 2048
#define MA_FILL 512          // workgroups wanted before the batch is split no further

static int ma_ntiles(int D) {
    const int nt = cdiv(D, MA_T);
    return nt * (nt + 1) / 2;
}
static int ma_ksplit(int B, int D) {
    const int want = cdiv(MA_FILL, ma_ntiles(D));
    return imax(1, imin(imin(MA_KSPLIT_MAX, want), B / 128));
}

extern "C" int64_t otvae_moments_accum_ws(int B, int D) {
    if (B <= 0 || D <= 0 || D > MA_MAX_D) return -1;
    const int ks = ma_ksplit(B, D);
    if (ks == 1) return 0;
    return (int64_t)ks * ((int64_t)ma_ntiles(D) * MA_T * MA_T + (int64_t)cdiv(D, MA_T) * MA_T) * (int64_t)sizeof(double);
}

__device__ __forceinline__ void ma_tile_of(int t, int& ti, int& tj) {
    ti = (int)((sqrtf(8.f * (float)t + 1.f) - 1.f) * 0.5f);
    while (ti * (ti + 1) / 2 > t) --ti;
    while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
    tj = t - ti * (ti + 1) / 2;
}

// grid (ntiles, ksplit).  ksplit == 1: the state is updated in place; otherwise partial tiles go to ws[ks][ntiles][64][64] and the
// partial feature sums of the diagonal tiles to ws_sum[ks][nt][64].
template <typename TIN, bool DIRECT>
__global__ __launch_bounds__(256) void ma_tile_kernel(const TIN* __restrict__ f, int B, int D, int rows_per, double* __restrict__ n_obs,
                                                      double* __restrict__ sum_x, double* __restrict__ sum_xx, double* __restrict__ ws,
                                                      double* __restrict__ ws_sum) {
    __shared__ double as[MA_KC][MA_LD], bs_[MA_KC][MA_LD];
    int ti, tj;
    ma_tile_of(blockIdx.x, ti, tj);
    const bool diag = ti == tj;
    double (*bs)[MA_LD] = diag ? as : bs_;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l16 = lane & 15, lk = lane >> 4;
    const int i0 = ti * MA_T, j0 = tj * MA_T;
    const int r0 = blockIdx.y * rows_per, r1 = min(B, r0 + rows_per);
    // staging: thread (row = wave + 4 u, col = lane) of the 32 x 64 panel -- 256 contiguous bytes (fp32) per wave and row
    const int ci = i0 + lane, cj = j0 + lane;
    const bool ci_ok = ci < D, cj_ok = cj < D;

    f64x4 acc[4], accs = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};

    TIN ra[MA_KC / 4], rb[MA_KC / 4];
    auto fetch = [&](int r) {
#pragma unroll
        for (int u = 0; u < MA_KC / 4; ++u) {
            const int row = r + wave + 4 * u;
            const bool ok = row < r1;
            ra[u] = (ok && ci_ok) ? f[(size_t)row * D + ci] : (TIN)0;
            if (!diag) rb[u] = (ok && cj_ok) ? f[(size_t)row * D + cj] : (TIN)0;
        }
    };
    if (r0 < r1) fetch(r0);
    for (int r = r0; r < r1; r += MA_KC) {
#pragma unroll
        for (int u = 0; u < MA_KC / 4; ++u) {
            as[wave + 4 * u][lane] = (double)ra[u];
            if (!diag) bs_[wave + 4 * u][lane] = (double)rb[u];
        }
        __syncthreads();
        if (r + MA_KC < r1) fetch(r + MA_KC);  // in flight under the MFMAs below
#pragma unroll
        for (int ks = 0; ks < MA_KC / 4; ++ks) {
            const double av = as[ks * 4 + lk][wave * 16 + l16];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bs[ks * 4 + lk][t * 16 + l16], acc[t], 0, 0, 0);
            if (diag) accs = __builtin_amdgcn_mfma_f64_16x16x4f64(av, 1.0, accs, 0, 0, 0);
        }
        __syncthreads();
    }

    if (DIRECT) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = i0 + wave * 16 + 4 * r + lk, j = j0 + t * 16 + l16;
                if (i < D && j < D && (!diag || i >= j)) {
                    const double v = sum_xx[(size_t)i * D + j] + acc[t][r];
                    sum_xx[(size_t)i * D + j] = v;
                    if (i != j) sum_xx[(size_t)j * D + i] = v;
                }
            }
        if (diag && l16 == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = i0 + wave * 16 + 4 * r + lk;
                if (i < D) sum_x[i] += accs[r];
            }
        }
        if (blockIdx.x == 0 && tid == 0) n_obs[0] += (double)B;
    } else {
        double* wt = ws + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (MA_T * MA_T);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) wt[(wave * 16 + 4 * r + lk) * MA_T + t * 16 + l16] = acc[t][r];
        if (diag && l16 == 0) {
            const int nt = (D + MA_T - 1) / MA_T;
#pragma unroll
            for (int r = 0; r < 4; ++r) ws_sum[((size_t)blockIdx.y * nt + ti) * MA_T + wave * 16 + 4 * r + lk] = accs[r];
        }
    }
}

// grid (ntiles + 1): workgroup t < ntiles adds the ksplit partials of tile t, in split order, into both triangles of the state; the
// last workgroup does the same for sum f and adds B to the observation count.
__global__ __launch_bounds__(256) void ma_final_kernel(const double* __restrict__ ws, const double* __restrict__ ws_sum, int B, int D,
                                                       int ksplit, double* __restrict__ n_obs, double* __restrict__ sum_x,
                                                       double* __restrict__ sum_xx) {
    const int ntiles = gridDim.x - 1;
    if ((int)blockIdx.x == ntiles) {
        const int nt = (D + MA_T - 1) / MA_T;
        for (int i = threadIdx.x; i < D; i += 256) {
            double s = 0.0;
            for (int k = 0; k < ksplit; ++k) s += ws_sum[(size_t)k * nt * MA_T + i];
            sum_x[i] += s;
        }
        if (threadIdx.x == 0) n_obs[0] += (double)B;
        return;
    }
    int ti, tj;
    ma_tile_of(blockIdx.x, ti, tj);
    const size_t split = (size_t)ntiles * (MA_T * MA_T);
    const double* wt = ws + (size_t)blockIdx.x * (MA_T * MA_T);
    for (int e = threadIdx.x; e < MA_T * MA_T; e += 256) {
        const int i = ti * MA_T + (e >> 6), j = tj * MA_T + (e & 63);
        if (i >= D || j >= D || (ti == tj && i < j)) continue;
        double s = 0.0;
        for (int k = 0; k < ksplit; ++k) s += wt[k * split + e];
        const double v = sum_xx[(size_t)i * D + j] + s;
        sum_xx[(size_t)i * D + j] = v;
        if (i != j) sum_xx[(size_t)j * D + i] = v;
    }
}

template <typename TIN>
static void ma_launch(const TIN* f, int B, int D, double* n_obs, double* sum_x, double* sum_xx, double* ws, hipStream_t st) {
    const int ks = ma_ksplit(B, D), ntiles = ma_ntiles(D);
    const int rows_per = cdiv(cdiv(B, ks), MA_KC) * MA_KC;
    if (ks == 1) {
        ma_tile_kernel<TIN, true><<<dim3(ntiles, 1), 256, 0, st>>>(f, B, D, rows_per, n_obs, sum_x, sum_xx, nullptr, nullptr);
        return;
    }
    double* ws_sum = ws + (size_t)ks * ntiles * (MA_T * MA_T);
    ma_tile_kernel<TIN, false><<<dim3(ntiles, ks), 256, 0, st>>>(f, B, D, rows_per, n_obs, sum_x, sum_xx, ws, ws_sum);
    ma_final_kernel<<<ntiles + 1, 256, 0, st>>>(ws, ws_sum, B, D, ks, n_obs, sum_x, sum_xx);
}

extern "C" int otvae_moments_accum(int in_dtype, const void* feats, int B, int D, double* n_obs, double* sum_x, double* sum_xx,
                                   void* ws, void* stream) {
    OTVAE_REQUIRE(feats && n_obs && sum_x && sum_xx && B > 0 && D > 0, "otvae_moments_accum: bad argument");
    OTVAE_REQUIRE(in_dtype == 0 || in_dtype == 1, "otvae_moments_accum: in_dtype must be 0 (fp32) or 1 (fp64)");
    OTVAE_REQUIRE(D <= MA_MAX_D, "otvae_moments_accum: D = %d exceeds %d", D, MA_MAX_D);
    OTVAE_REQUIRE(ws || ma_ksplit(B, D) == 1, "otvae_moments_accum: workspace missing (otvae_moments_accum_ws)");
    if (in_dtype == 0) ma_launch<float>((const float*)feats, B, D, n_obs, sum_x, sum_xx, (double*)ws, (hipStream_t)stream);
    else ma_launch<double>((const double*)feats, B, D, n_obs, sum_x, sum_xx, (double*)ws, (hipStream_t)stream);
    OTVAE_CHECK_LAUNCH("otvae_moments_accum");
    return OTVAE_OK;
}

// ================================================================================================ PSNR
// state: [0] sum (p - t)^2, [1] element count, [2] min target, [3] max target, then 3 x SQ_PARTS doubles of scratch for the first
// stage's per-workgroup partials (contents unspecified between calls).  Stage one: SQ_PARTS-or-fewer workgroups (the count depends on
// numel alone) stride over both tensors; stage two: one workgroup folds the partials in index order into state[0..3].
#define SQ_PARTS 256
#define SQ_HEAD 4

extern "C" int otvae_sqerr_state_words(void) { return SQ_HEAD + 3 * SQ_PARTS; }

__device__ __forceinline__ void sq_block_reduce(double& s, double& mn, double& mx, double (*red)[4]) {
    s = wave_sum(s);
    mn = wave_min(mn);
    mx = wave_max(mx);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[0][w] = s;
        red[1][w] = mn;
        red[2][w] = mx;
    }
    __syncthreads();
    s = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    mn = fmin(fmin(red[1][0], red[1][1]), fmin(red[1][2], red[1][3]));
    mx = fmax(fmax(red[2][0], red[2][1]), fmax(red[2][2], red[2][3]));
}

template <typename TIN>
__global__ __launch_bounds__(256) void sq_partial_kernel(const TIN* __restrict__ p, const TIN* __restrict__ t, int64_t numel,
                                                         double* __restrict__ state) {
    __shared__ double red[3][4];
    double s = 0.0, mn = INFINITY, mx = -INFINITY;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < numel; e += (int64_t)gridDim.x * 256) {
        const double tv = (double)t[e];
        const double d = (double)p[e] - tv;
        s = fma(d, d, s);
        mn = tv < mn ? tv : mn;
        mx = tv > mx ? tv : mx;
    }
    sq_block_reduce(s, mn, mx, red);
    if (threadIdx.x == 0) {
        state[SQ_HEAD + blockIdx.x] = s;
        state[SQ_HEAD + SQ_PARTS + blockIdx.x] = mn;
        state[SQ_HEAD + 2 * SQ_PARTS + blockIdx.x] = mx;
    }
}

__global__ __launch_bounds__(256) void sq_final_kernel(int parts, int64_t numel, double* __restrict__ state) {
    __shared__ double red[3][4];
    const int b = threadIdx.x;
    double s = b < parts ? state[SQ_HEAD + b] : 0.0;
    double mn = b < parts ? state[SQ_HEAD + SQ_PARTS + b] : INFINITY;
    double mx = b < parts ? state[SQ_HEAD + 2 * SQ_PARTS + b] : -INFINITY;
    sq_block_reduce(s, mn, mx, red);
    if (b == 0) {
        state[0] += s;
        state[1] += (double)numel;
        state[2] = fmin(state[2], mn);
        state[3] = fmax(state[3], mx);
    }
}

extern "C" int otvae_sqerr_accum(int in_dtype, const void* preds, const void* target, int64_t numel, double* state, void* stream) {
    OTVAE_REQUIRE(preds && target && state && numel > 0, "otvae_sqerr_accum: bad argument");
    OTVAE_REQUIRE(in_dtype == 0 || in_dtype == 1, "otvae_sqerr_accum: in_dtype must be 0 (fp32) or 1 (fp64)");
    hipStream_t st = (hipStream_t)stream;
    const int parts = imax(1, imin(SQ_PARTS, cdiv(numel, 256 * 8)));
    if (in_dtype == 0) sq_partial_kernel<float><<<parts, 256, 0, st>>>((const float*)preds, (const float*)target, numel, state);
    else sq_partial_kernel<double><<<parts, 256, 0, st>>>((const double*)preds, (const double*)target, numel, state);
    sq_final_kernel<<<1, 256, 0, st>>>(parts, numel, state);
    OTVAE_CHECK_LAUNCH("otvae_sqerr_accum");
    return OTVAE_OK;
}
