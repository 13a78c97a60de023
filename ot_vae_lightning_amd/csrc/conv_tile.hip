// ConvLayer forward / data-gradient as an IMAGE-TILE convolution on the fp32 MFMA (v_mfma_f32_16x16x4_f32), gfx950.
//
// The implicit-GEMM kernels of conv.hip gather every (row, k) element of the A operand from global memory with its own
// bounds test and address arithmetic; at this model's layer sizes (8..64 channels, 16x16 .. 1x1 maps, batch ~1000) that
// is ~1000 vector instructions per 64-row tile for 24..144 MFMAs, and the launches are bound by VALU issue, not by
// MFMA, LDS or HBM.  Here a workgroup owns IPB whole images instead:
//   * the layer input of those images (x after BatchNorm-apply + ReLU, nearest-upsampled; or the output gradient for
//     the data-gradient pass) is staged ONCE into LDS as a zero-padded "virtual grid" V[img][vy][vx][c] -- contiguous,
//     coalesced float4 loads, one activation per element, no per-tap re-reads;
//   * every (output position, tap) operand is then V[pixbase(position) + tapoff(tap) + c]: the bounds tests disappear
//     (padding is stored as zeros), the address is one add, and the inner loop is ds_read + MFMA;
//   * the weights of a group of taps sit in LDS next to it ([k][16*NT] slab, conflict-free reads).
// MFMA operands are swapped (A = weights, B = activations) so that D[out-channel][position]: a lane ends up with 4
// consecutive output channels of ONE position = one 16-byte store (and 16-byte loads of bias / residual / x).
//
// Same arithmetic as conv.hip (reference networks/cnn.py:183-192 and its autograd backward): products accumulate in
// fp32 over k = (tap, channel) in the same tap-major order; BatchNorm / BatchNorm-backward partial sums in fp64 with the
// fixed lane -> wave -> block order; workspace layouts ([2][cpad][P]) identical to the implicit-GEMM kernels.
#include <type_traits>

#include "common.h"
#include "conv_tile.h"

#define TILE_WMAX 4096  // floats of one weight chunk in LDS (16 KiB)

__device__ __forceinline__ int tdiv(int k, float inv_d) { return (int)(((float)k + 0.5f) * inv_d); }  // exact for k < 2^22
__device__ __forceinline__ int imax_d(int a, int b) { return a > b ? a : b; }

// The body of one workgroup (statements in conv_tile_body.h, shared with the one-job kernel below).  (bx, by, bz) is its index in a
// grid of (gx, *, gz) workgroups: the job-local ("virtual") index in the two-job kernel below.  tsm: the dynamic LDS; bn_tab: 2 x 256 floats of LDS.
template <int MODE, int NT, int RBW>
__device__ __forceinline__ void conv_tile_body(const TilePlan& pl, const float* __restrict__ S,
                                               const float* __restrict__ scale, const float* __restrict__ shift,
                                               int relu, const float* __restrict__ Wg,
                                               // FWD epilogue
                                               const float* __restrict__ bias, const float* __restrict__ res,
                                               float* __restrict__ y,
                                               // DGRAD epilogue
                                               const float* __restrict__ xin, const float* __restrict__ mean,
                                               const float* __restrict__ invstd, float* __restrict__ gv,
                                               double* __restrict__ partial, const BnFold& fold, float* tsm,
                                               float (*bn_tab)[256], int bx, int by, int bz, int gx, int gz) {
#define TILE_BX bx
#define TILE_BY by
#define TILE_BZ bz
#define TILE_GX gx
#define TILE_GZ gz
#include "conv_tile_body.h"
#undef TILE_BX
#undef TILE_BY
#undef TILE_BZ
#undef TILE_GX
#undef TILE_GZ
}

template <int MODE, int NT, int RBW>
__global__ __launch_bounds__(256) void conv_tile_kernel(TilePlan pl, const float* __restrict__ S,
                                                        const float* __restrict__ scale, const float* __restrict__ shift,
                                                        int relu, const float* __restrict__ Wg,
                                                        const float* __restrict__ bias, const float* __restrict__ res,
                                                        float* __restrict__ y, const float* __restrict__ xin,
                                                        const float* __restrict__ mean, const float* __restrict__ invstd,
                                                        float* __restrict__ gv, double* __restrict__ partial, BnFold fold) {
    extern __shared__ __align__(16) float tsm[];
    __shared__ __align__(16) float bn_tab[2][256];
#define TILE_BX blockIdx.x
#define TILE_BY blockIdx.y
#define TILE_BZ blockIdx.z
#define TILE_GX gridDim.x
#define TILE_GZ gridDim.z
#include "conv_tile_body.h"
#undef TILE_BX
#undef TILE_BY
#undef TILE_BZ
#undef TILE_GX
#undef TILE_GZ
}

// Two independent jobs of the same MODE (the two branches of a ConvBlock head) in ONE launch: the grid is job 0's workgroups followed
// by job 1's, each workgroup runs its own job's body -- unchanged -- with its job-local index.  One instantiation per pair of bodies,
// so the registers are the larger body's and the dynamic LDS (set by the host) the larger job's.
// Two equal bodies are ONE body called with the job's arguments: t.j[job] is a uniform address into the kernel arguments, as in
// conv_jobs_body (two separate by-value arguments and a select between them made the compiler keep a private copy in scratch).  Two
// different bodies sit in the two arms of a branch.
struct TilePairArgs {
    TileJobArgs j[2];
    int block1;  // first workgroup of job 1
};

template <int MODE, int NT, int RBW>
__device__ __forceinline__ void conv_tile_job(const TileJobArgs& j, int lb, float* tsm, float (*bn_tab)[256]) {
    const int bx = lb % j.gx, r = lb / j.gx;
    conv_tile_body<MODE, NT, RBW>(j.pl, j.S, j.scale, j.shift, j.relu, j.Wg, j.bias, j.res, j.y, j.xin, j.mean, j.invstd, j.gv, j.partial,
                                  j.fold, tsm, bn_tab, bx, r % j.gy, r / j.gy, j.gx, j.gz);
}

template <int MODE, int NT0, int RBW0, int NT1, int RBW1>
__global__ __launch_bounds__(256) void conv_tile_kernel_pair(TilePairArgs t) {
    extern __shared__ __align__(16) float tsm[];
    __shared__ __align__(16) float bn_tab[2][256];
    const int job = (int)blockIdx.x >= t.block1 ? 1 : 0;
    const int lb = (int)blockIdx.x - (job ? t.block1 : 0);
    if constexpr (NT0 == NT1 && RBW0 == RBW1) {
        conv_tile_job<MODE, NT0, RBW0>(t.j[job], lb, tsm, bn_tab);
    } else if (job == 0) {
        conv_tile_job<MODE, NT0, RBW0>(t.j[0], lb, tsm, bn_tab);
    } else {
        conv_tile_job<MODE, NT1, RBW1>(t.j[1], lb, tsm, bn_tab);
    }
}

// ------------------------------------------------------------------------------------------------ host: planning
static bool tap_touches(int rows, int rstride, int d, int lim) {
    // exists r in [0, rows): 0 <= r*rstride + d < lim
    for (int r = 0; r < rows; ++r) {
        const int v = r * rstride + d;
        if (v >= 0 && v < lim) return true;
    }
    return false;
}

bool conv_tile_plan(const Geom& g, int mode, TilePlan& pl, dim3& grid, size_t& smem) {
    if ((g.Cs % 4) || (g.Cn % 4)) return false;
    if (getenv("OTVAE_NO_TILE")) return false;
    pl = {};
    int tdy[4][TILE_MAXT], tdx[4][TILE_MAXT];  // virtual-grid offsets of the kept taps (before cropping)
    const int Hu = g.Hs * g.up, Wu = g.Ws * g.up;
    pl.N = g.N;
    int nz = 1;
    if (mode == 0) {
        pl.srcH = g.Hs, pl.srcW = g.Ws, pl.CK = g.Cs, pl.NC = g.Cn;
        pl.Hv = Hu + 2 * g.pad, pl.Wv = Wu + 2 * g.pad;
        pl.voffy = pl.voffx = g.pad;
        pl.ush = g.up - 1;
        pl.limH = Hu, pl.limW = Wu;
        pl.rowsH = g.Ho, pl.rowsW = g.Wo, pl.rstride = g.stride;
        if ((g.Ho - 1) * g.stride + g.KH > pl.Hv || (g.Wo - 1) * g.stride + g.KW > pl.Wv) return false;
        TileTaps& tp = pl.taps[0];
        for (int kh = 0; kh < g.KH; ++kh)
            for (int kw = 0; kw < g.KW; ++kw) {
                if (!tap_touches(g.Ho, g.stride, kh - g.pad, Hu) || !tap_touches(g.Wo, g.stride, kw - g.pad, Wu)) continue;
                if (tp.n == TILE_MAXT) return false;
                tdy[0][tp.n] = kh, tdx[0][tp.n] = kw;
                tp.wrow[tp.n] = kh * g.KW + kw;
                ++tp.n;
            }
    } else {
        pl.srcH = g.Ho, pl.srcW = g.Wo, pl.CK = g.Cn, pl.NC = g.Cs;
        pl.ush = 0;
        pl.limH = g.Ho, pl.limW = g.Wo;
        pl.rstride = 1;
        if (g.stride == 1) {
            const int vy = g.KH - 1 - g.pad, vx = g.KW - 1 - g.pad;
            if (vy < 0 || vx < 0) return false;
            pl.voffy = vy, pl.voffx = vx;
            pl.Hv = Hu + g.KH - 1, pl.Wv = Wu + g.KW - 1;
            pl.rowsH = Hu, pl.rowsW = Wu;
            pl.childmode = g.up == 2 ? 1 : 0;
            TileTaps& tp = pl.taps[0];
            for (int kh = 0; kh < g.KH; ++kh)
                for (int kw = 0; kw < g.KW; ++kw) {
                    if (!tap_touches(Hu, 1, g.pad - kh, g.Ho) || !tap_touches(Wu, 1, g.pad - kw, g.Wo)) continue;
                    if (tp.n == TILE_MAXT) return false;
                    tdy[0][tp.n] = g.KH - 1 - kh, tdx[0][tp.n] = g.KW - 1 - kw;
                    tp.wrow[tp.n] = kh * g.KW + kw;
                    ++tp.n;
                }
        } else {  // stride 2 (up == 1): one launch slice (blockIdx.z) per input-parity class
            if (g.up != 1 || (g.Hs & 1) || (g.Ws & 1)) return false;
            nz = 4;
            pl.s2 = 1;
            pl.rowsH = g.Hs >> 1, pl.rowsW = g.Ws >> 1;
            // source offset of tap kh for parity py: d = (py + pad - kh) / 2 when that is even
            int dmin = 0, dmax = 0;
            for (int py = 0; py < 2; ++py)
                for (int kh = 0; kh < imax(g.KH, g.KW); ++kh) {
                    const int t = py + g.pad - kh;
                    if (t & 1) continue;
                    const int d = t / 2;  // exact (t even), also for negative t
                    dmin = imin(dmin, d);
                    dmax = imax(dmax, d);
                }
            pl.voffy = pl.voffx = -dmin;
            pl.Hv = pl.rowsH + dmax - dmin, pl.Wv = pl.rowsW + dmax - dmin;
            for (int cls = 0; cls < 4; ++cls) {
                const int py = cls >> 1, px = cls & 1;
                TileTaps& tp = pl.taps[cls];
                for (int kh = 0; kh < g.KH; ++kh) {
                    const int ty = py + g.pad - kh;
                    if (ty & 1) continue;
                    for (int kw = 0; kw < g.KW; ++kw) {
                        const int tx = px + g.pad - kw;
                        if (tx & 1) continue;
                        const int dy = ty / 2, dx = tx / 2;
                        if (!tap_touches(pl.rowsH, 1, dy, g.Ho) || !tap_touches(pl.rowsW, 1, dx, g.Wo)) continue;
                        if (tp.n == TILE_MAXT) return false;
                        tdy[cls][tp.n] = dy + pl.voffy, tdx[cls][tp.n] = dx + pl.voffx;
                        tp.wrow[tp.n] = kh * g.KW + kw;
                        ++tp.n;
                    }
                }
            }
        }
    }
    pl.rowsPI = pl.rowsH * pl.rowsW;
    pl.CKp = pl.CK + 4;
    {
        // crop the virtual grid to the bounding box the kept taps can reach (a 3x3 layer on a 1x1 map keeps only its
        // centre tap: the grid shrinks from 3x3 to 1x1)
        int ylo = 1 << 30, yhi = -1, xlo = 1 << 30, xhi = -1;
        for (int c = 0; c < 4; ++c)
            for (int t = 0; t < pl.taps[c].n; ++t) {
                ylo = imin(ylo, tdy[c][t]), yhi = imax(yhi, tdy[c][t] + (pl.rowsH - 1) * pl.rstride);
                xlo = imin(xlo, tdx[c][t]), xhi = imax(xhi, tdx[c][t] + (pl.rowsW - 1) * pl.rstride);
            }
        if (yhi < 0) return false;  // no tap at all
        pl.Hv = yhi - ylo + 1, pl.Wv = xhi - xlo + 1;
        pl.voffy -= ylo, pl.voffx -= xlo;
        for (int c = 0; c < 4; ++c)
            for (int t = 0; t < pl.taps[c].n; ++t) pl.taps[c].off[t] = ((tdy[c][t] - ylo) * pl.Wv + (tdx[c][t] - xlo)) * pl.CKp;
    }
    if (pl.rowsPI > 256) return false;
    if (pl.rowsPI < 64 && !getenv("OTVAE_TILE_ALL")) return false;  // deep layers: the K-pipelined implicit GEMM is faster
                                                                      // (measured again at the final state: 16 rows 3.17, 4 rows 3.34 vs 3.10 ms)
    if (pl.CK * 16 > TILE_WMAX) return false;  // one tap of weights must fit the chunk (CK <= 256)
    // images per block: 64 .. 256 rows, more rows per block only when that still leaves >= 512 blocks (measured: 384..512
    // is the flat optimum for the whole step, 1024 and 2048 are 1 % slower)
    const int per_img_floats = pl.Hv * pl.Wv * pl.CKp;
    const long total_rows = (long)g.N * pl.rowsPI;
    int target = 64;
    if (total_rows / 128 >= 512) target = 128;
    if (total_rows / 256 >= 512) target = 256;
    int ipb = imax(1, target / pl.rowsPI);
    const int lds_floats = (96 * 1024) / 4 - TILE_WMAX - 4 * 2 * 64 * 2;
    while (ipb > 1 && (long)ipb * per_img_floats > lds_floats) --ipb;
    if ((long)ipb * per_img_floats > lds_floats) return false;
    ipb = imin(ipb, g.N);
    pl.IPB = ipb;
    pl.vfloats = ipb * per_img_floats;
    const int rows_blk = ipb * pl.rowsPI;
    pl.rbw = cdiv(rows_blk, 64);
    if (pl.rbw == 3) pl.rbw = 4;
    if (pl.rbw > 4) return false;
    // column tiles per wave: as conv.hip (>= 512 blocks when possible)
    const int nnt = cdiv(pl.NC, 16);
    int nt = nnt >= 4 ? 4 : nnt;
    const long rb = (long)cdiv(g.N, ipb) * nz;
    while (nt > 1 && rb * cdiv(nnt, nt) < 512) --nt;
    if (pl.rbw * nt > 8) nt = imax(1, 8 / pl.rbw);  // accumulator registers
    while (nt > 1 && pl.CK * 16 * nt > TILE_WMAX) --nt;  // one tap of weights must fit the chunk
    pl.nt = nt;
    const int ny = cdiv(nnt, nt);
    pl.cpad = ny * 16 * nt;
    pl.tpc = imax(1, TILE_WMAX / (pl.CK * 16 * nt));
    grid = dim3(cdiv(g.N, ipb), ny, nz);
    smem = ((size_t)pl.vfloats + TILE_WMAX) * sizeof(float) + sizeof(double) * 4 * 2 * 16 * nt;
    return true;
}

template <int MODE>
static int tile_launch(const TilePlan& pl, dim3 grid, size_t smem, hipStream_t st, const float* S, const float* scale,
                       const float* shift, int relu, const float* Wg, const float* bias, const float* res, float* y,
                       const float* xin, const float* mean, const float* invstd, float* gv, double* partial,
                       const BnFold& fold = BnFold{}) {
    const char* who = MODE == 0 ? "otvae_conv_fwd(tile)" : "otvae_conv_bwd_data(tile)";
#define TL(N_, R_)                                                                                                    \
    do {                                                                                                              \
        if (int rc = otvae_lds_grant<&conv_tile_kernel<MODE, N_, R_>>(who, smem, 96 * 1024)) return rc;               \
        conv_tile_kernel<MODE, N_, R_><<<grid, 256, smem, st>>>(pl, S, scale, shift, relu, Wg, bias, res, y, xin, mean, \
                                                                invstd, gv, partial, fold);                           \
    } while (0)
#define TLR(N_)                                  \
    switch (pl.rbw) {                            \
        case 1: TL(N_, 1); break;                \
        case 2: TL(N_, 2); break;                \
        default: TL(N_, 4); break;               \
    }
    switch (pl.nt) {
        case 1: TLR(1); break;
        case 2: TLR(2); break;
        case 3:
            if (pl.rbw == 4) return -1;
            switch (pl.rbw) {
                case 1: TL(3, 1); break;
                default: TL(3, 2); break;
            }
            break;
        default:
            if (pl.rbw == 4) return -1;
            switch (pl.rbw) {
                case 1: TL(4, 1); break;
                default: TL(4, 2); break;
            }
            break;
    }
#undef TLR
#undef TL
    return 0;
}

// (NT0, RBW0, NT1, RBW1) of the two-job kernels: what conv_tile_plan gives the ConvBlock heads of the capacity-8 and capacity-16
// networks at 8x8 and 16x16 maps (two equal stride-2 branches; an up-sampling 3x3 with its 1x1 skip) for batches of 1 .. 4096 images.
// Any other pair runs as two launches.
#define TILE_PAIR_CASES_FWD(X) X(1, 1, 1, 1) X(1, 2, 1, 2) X(1, 4, 1, 4) X(2, 1, 2, 1) X(2, 2, 2, 2) X(2, 2, 2, 4) X(2, 4, 2, 4)
// (the data-gradient pair (2, 1) + (2, 1) is left out: its two-job kernel took 66 VGPRs for the one-job kernel's 64 and with them 6
// waves per SIMD for 7)
#define TILE_PAIR_CASES_DGRAD(X) \
    X(1, 1, 1, 1) X(1, 2, 1, 2) X(1, 4, 1, 4) X(2, 2, 2, 2) X(2, 4, 2, 4) X(3, 1, 3, 1) X(4, 1, 4, 1) X(4, 2, 4, 2)

template <int MODE>
static int tile_pair_launch(const TileJobArgs& a, const TileJobArgs& b, size_t smem, hipStream_t st) {
    const int nb0 = a.gx * a.gy * a.gz, nb1 = b.gx * b.gy * b.gz;
    if (smem > 96 * 1024) return -1;
    const TilePairArgs t = {{a, b}, nb0};
#define X(N0_, R0_, N1_, R1_)                                                                                         \
    if (a.pl.nt == N0_ && a.pl.rbw == R0_ && b.pl.nt == N1_ && b.pl.rbw == R1_) {                                     \
        if (int rc = otvae_lds_grant<&conv_tile_kernel_pair<MODE, N0_, R0_, N1_, R1_>>("otvae_conv_multi(pair)", smem, 96 * 1024)) \
            return rc;                                                                                                \
        conv_tile_kernel_pair<MODE, N0_, R0_, N1_, R1_><<<nb0 + nb1, 256, smem, st>>>(t);                             \
        return 0;                                                                                                     \
    }
    if constexpr (MODE == 0) {
        TILE_PAIR_CASES_FWD(X)
    } else {
        TILE_PAIR_CASES_DGRAD(X)
    }
#undef X
    return -1;
}

int conv_tile_pair(int mode, const TileJobArgs& a, const TileJobArgs& b, size_t smem, hipStream_t st) {
    return mode == 0 ? tile_pair_launch<0>(a, b, smem, st) : tile_pair_launch<1>(a, b, smem, st);
}

int conv_tile_fwd(const TilePlan& pl, dim3 grid, size_t smem, hipStream_t st, const float* x, const float* scale,
                  const float* shift, int relu, const float* wT, const float* bias, const float* res, float* y,
                  double* partial, const BnFold& fold) {
    return tile_launch<0>(pl, grid, smem, st, x, scale, shift, relu, wT, bias, res, y, nullptr, nullptr, nullptr, nullptr,
                          partial, fold);
}

int conv_tile_dgrad(const TilePlan& pl, dim3 grid, size_t smem, hipStream_t st, const float* gy, const float* wD,
                    const float* x, const float* scale, const float* shift, int relu, const float* mean,
                    const float* invstd, float* gv, double* partial) {
    return tile_launch<1>(pl, grid, smem, st, gy, scale, shift, relu, wD, nullptr, nullptr, nullptr, x, mean, invstd, gv,
                          partial);
}
