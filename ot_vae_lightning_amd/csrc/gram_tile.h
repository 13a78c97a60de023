// The 128 x 128 fp64 Gram tile that kid.hip (kernel sums) and knn_manifold.hip (k-smallest selection, ball counts) share: staging of two
// 128 x 32 fp32 row panels through LDS as fp64 and the v_mfma_f64_16x16x4_f64 main loop over the feature chunks.  The callers differ
// only in which rows they name (row_a / row_b: element offsets, so a gather and a contiguous strip are the same code) and in the epilogue.
//   * a workgroup of 4 waves; wave (wr, wc) = (wave / 2, wave % 2) owns the 64 x 64 quarter (wr, wc) of the tile as 4 x 4 accumulators:
//     lane l supplies A[l % 16][l / 16] and B[l / 16][l % 16], register r of acc[a][b] in lane l holds the product of tile row
//     wr * 64 + a * 16 + 4 r + l / 16 and tile column wc * 64 + b * 16 + l % 16.  8 LDS reads feed 16 MFMAs.
//   * the features are walked in chunks of 32.  VEC (D a multiple of 4, 16-byte aligned bases): thread (row = tid / 8 + 32 u,
//     k = 4 (tid % 8)) loads 16 bytes, 8 lanes one 128-byte row segment; otherwise thread (row = tid / 32 + 8 u, k = tid % 32) loads 4.
//     Both forms hand the same values to the matrix cores in the same order: the bits do not depend on the form.
//   * LDS is row-major with a row stride of 34 doubles (68 dwords = 4 mod 64 banks: the 16 rows x 2 k a half-wave's ds_read_b64 touches
//     fall into 64 distinct banks).  The next chunk's global loads are issued before the current chunk's MFMAs.
//   * diag (block-uniform): both panels are the same rows; only `as` is staged and read for both operands.
#pragma once
#include "common.h"

#define GT_T 128             // output tile
#define GT_KC 32             // features per staged chunk
#define GT_LD 34             // LDS row stride (doubles)
#define GT_MAX_D 2048

// row_a / row_b [GT_T] (LDS, published by a barrier before the call): element offset of the row in pa / pb, -1: a row of zeros.
// Ends with a block barrier: `as` / `bs_` are free for the caller's epilogue.
template <bool VEC>
__device__ __forceinline__ void gram_tile_mma(const float* __restrict__ pa, const float* __restrict__ pb, const int64_t* row_a,
                                              const int64_t* row_b, int D, bool diag, double (*as)[GT_LD], double (*bs_)[GT_LD],
                                              f64x4 (&acc)[4][4]) {
    double (*bs)[GT_LD] = diag ? as : bs_;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l16 = lane & 15, lk = lane >> 4;
    const int wr = wave >> 1, wc = wave & 1;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = f64x4{0.0, 0.0, 0.0, 0.0};

    const int sk = VEC ? (tid & 7) * 4 : tid & 31, sr = VEC ? tid >> 3 : tid >> 5;
    float ra[GT_T / 8], rb[GT_T / 8];
    auto fetch = [&](int k0) {
        const bool k_ok = k0 + sk < D;
        if (VEC) {
#pragma unroll
            for (int u = 0; u < GT_T / 32; ++u) {
                const int64_t oa = row_a[sr + 32 * u];
                const f32x4 va = (k_ok && oa >= 0) ? *reinterpret_cast<const f32x4*>(pa + oa + k0 + sk) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int e = 0; e < 4; ++e) ra[4 * u + e] = va[e];
                if (!diag) {
                    const int64_t ob = row_b[sr + 32 * u];
                    const f32x4 vb = (k_ok && ob >= 0) ? *reinterpret_cast<const f32x4*>(pb + ob + k0 + sk) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int e = 0; e < 4; ++e) rb[4 * u + e] = vb[e];
                }
            }
        } else {
#pragma unroll
            for (int u = 0; u < GT_T / 8; ++u) {
                const int64_t oa = row_a[sr + 8 * u];
                ra[u] = (k_ok && oa >= 0) ? pa[oa + k0 + sk] : 0.f;
                if (!diag) {
                    const int64_t ob = row_b[sr + 8 * u];
                    rb[u] = (k_ok && ob >= 0) ? pb[ob + k0 + sk] : 0.f;
                }
            }
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < D; k0 += GT_KC) {
        if (VEC) {
#pragma unroll
            for (int u = 0; u < GT_T / 32; ++u)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    as[sr + 32 * u][sk + e] = (double)ra[4 * u + e];
                    if (!diag) bs_[sr + 32 * u][sk + e] = (double)rb[4 * u + e];
                }
        } else {
#pragma unroll
            for (int u = 0; u < GT_T / 8; ++u) {
                as[sr + 8 * u][sk] = (double)ra[u];
                if (!diag) bs_[sr + 8 * u][sk] = (double)rb[u];
            }
        }
        __syncthreads();
        if (k0 + GT_KC < D) fetch(k0 + GT_KC);   // in flight under the MFMAs below
#pragma unroll
        for (int ks = 0; ks < GT_KC / 4; ++ks) {
            double av[4], bv[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) av[a] = as[wr * 64 + a * 16 + l16][ks * 4 + lk];
#pragma unroll
            for (int b = 0; b < 4; ++b) bv[b] = bs[wc * 64 + b * 16 + l16][ks * 4 + lk];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], acc[a][b], 0, 0, 0);
        }
        __syncthreads();
    }
}
