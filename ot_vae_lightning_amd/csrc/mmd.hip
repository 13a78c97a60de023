// Kernel two-sample (maximum mean discrepancy) loss between the latents of a minibatch and prior draws, and its gradient in the latents
// (MMDPrior; DESIGN.md "MMD prior").  Nothing of size N x M ever reaches global memory.
//
// Forward, main launch.  A workgroup (256 threads, 4 waves) owns a tile of 32 rows of A against a run of 32-row column tiles of B:
//   z-workgroups   A = z rows; B walks the combined column space [z tiles | y tiles] (the zz and the zy block in ONE accumulator: w is
//                  multiplied by the block's coefficient, -4 cz scale or +4 / (N M) scale, before it becomes an operand);
//   y-workgroups   A = y rows, B = y tiles: the yy block, k only.
// Per column tile:
//   1. the 32 rows of B are staged whole ([32][D rounded up to 16], zero padded) beside the resident A tile; row norms from the staged
//      bits (8 lanes per row, fixed exchange tree);
//   2. Gram: each wave one 16 x 16 tile of A B^T, v_mfma_f32_16x16x4_f32, a lane reads the operands of four steps as one 16-byte LDS
//      read along k (A and B see the same k order, so the products pair up); r = |a|^2 + |b|^2 - 2 a.b, clamped by a comparison that
//      lets NaN through;
//   3. k(r), w(r) per element (S reciprocals or exponentials); masks by INDEX: rows / columns past the end give 0, the diagonal of a
//      self block gives w = 0 and k = 0 (unbiased) or k(0) (biased).  k goes, per tile, into the thread's fp64 partial;
//   4. w (times the coefficient) is written in the MFMA C/D layout into a [32][36] LDS tile and read back as the A operand of
//      W[32 x 32] X[32 x D]: wave (wr, wc) owns output rows 16 wr .. and every second 16-column tile, accumulators in registers
//      (4 NT registers; NT = 1, 2, 4 for D <= 32, 64, 128 and 16 up to 512, tiles past D skipped); the k order of this product, 4 (lane >> 4) + (s & 3) + 16 (s >> 2), makes
//      the four-byte reads of X rows bank-conflict free (rows 4 apart are 16 banks apart at a row stride of 4 mod 32 words).
//   After the run: partial gradient tile = rowsum(w) . z_i - (W X)_i  ->  ws (one slot per column split), fp64 partials -> ws.
// Finishing launch: block 0 adds the fp64 partials in index order -> terms, loss (replicated); all blocks add the gradient slots in
// index order -> G.  No float atomic anywhere: two runs give the same bits.  Every word of ws that is read was written by the main launch.
// A row with an entry that is not finite has a norm that is not finite: 0 x norm is added to the partials, so the loss is NaN even when
// every pair it takes part in happens to be at distance +inf (k = 0).
//
// Backward: gz = gadd + (sum gout) G, element-wise, one launch.
#include "common.h"

#define MMD_MAX_D 512
#define MMD_MAX_SCALES 8
#define MMD_TILE 32          // rows of A and of B per tile
#define MMD_WLD 36           // words per row of the w tile
#define MMD_MAX_SPLITS 64    // column splits of a row tile (bounds the gradient workspace at 64 N D words)
#define MMD_TARGET_WGS 256   // z-workgroups aimed at (one per CU)

struct MmdFn {
    float c[MMD_MAX_SCALES];   // imq: C_k             rbf: 1 / C_k
    float a[MMD_MAX_SCALES];   // imq: unused          rbf: -log2(e) / C_k
    int S;
};

struct MmdPlan {
    int rtN, rtM;       // row tiles of z, of y
    int cN, cM;         // column tiles of z, of y
    int tps_z, ns_z;    // column tiles per z-workgroup, column splits (ns_z = ceil((cN + cM) / tps_z): none is empty)
    int tps_y, ns_y;    // the same for the yy block
    int nz, ny;         // workgroups: nz = rtN ns_z, then ny = rtM ns_y
    int ld;             // words per staged row: D rounded up to 32, + 4
    int dp;             // D rounded up to 16
};

static inline bool mmd_plan(int N, int M, int D, MmdPlan* p) {
    if (N < 1 || M < 1 || D < 1 || D > MMD_MAX_D) return false;
    if ((int64_t)N * D >= (int64_t)1 << 31 || (int64_t)M * D >= (int64_t)1 << 31) return false;
    p->rtN = p->cN = cdiv(N, MMD_TILE);
    p->rtM = p->cM = cdiv(M, MMD_TILE);
    const int cols = p->cN + p->cM;
    const int want = imax(1, imin(imin(cols, MMD_MAX_SPLITS), cdiv(MMD_TARGET_WGS, p->rtN)));
    p->tps_z = cdiv(cols, want);
    p->ns_z = cdiv(cols, p->tps_z);
    p->tps_y = imin(p->cM, 2 * p->tps_z);   // a yy tile costs half a z tile (no gradient product)
    p->ns_y = cdiv(p->cM, p->tps_y);
    const int64_t nz = (int64_t)p->rtN * p->ns_z, ny = (int64_t)p->rtM * p->ns_y;
    if (nz + ny >= (int64_t)1 << 31) return false;
    p->nz = (int)nz;
    p->ny = (int)ny;
    p->dp = (D + 15) & ~15;
    p->ld = ((D + 31) & ~31) + 4;
    return true;
}

static inline size_t mmd_lds_bytes(const MmdPlan& p) {
    return ((size_t)2 * MMD_TILE * p.ld + MMD_TILE * MMD_WLD + 4 * MMD_TILE) * sizeof(float);
}
static inline size_t mmd_kpart_bytes(const MmdPlan& p) {   // [nz + ny][2] fp64, rounded up to 16 bytes (it is)
    return ((size_t)p.nz + p.ny) * 2 * sizeof(double);
}

// k(r), w(r) of four distances at once: the scale loop is unrolled to its maximum behind wave-uniform tests, its constants sit in
// registers, and the four chains of reciprocals (or exponentials) are independent
template <bool IMQ>
__device__ __forceinline__ void mmd_kw4(const float (&fc)[MMD_MAX_SCALES], const float (&fa)[MMD_MAX_SCALES], int S, const float (&r)[4],
                                        float (&k)[4], float (&w)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) k[q] = w[q] = 0.f;
#pragma unroll
    for (int s = 0; s < MMD_MAX_SCALES; ++s) {
        if (s < S) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (IMQ) {
                    const float t = __builtin_amdgcn_rcpf(fc[s] + r[q]);
                    const float u = fc[s] * t;
                    k[q] += u;
                    w[q] = fmaf(u, t, w[q]);
                } else {
                    const float e = __builtin_amdgcn_exp2f(r[q] * fa[s]);
                    k[q] += e;
                    w[q] = fmaf(e, fc[s], w[q]);
                }
            }
        }
    }
}

// block-wide fp64 sum in a fixed order (lane tree, then the four waves in index order); every thread gets the total
__device__ __forceinline__ double mmd_block_sum(double v, double* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// 32 rows [row0, row0 + 32) of src[rows][D] -> dst[32][ld], columns [0, dp), zero past the rows and past D
__device__ __forceinline__ void mmd_stage(float* __restrict__ dst, const float* __restrict__ src, int rows, int row0, int D, int dp,
                                          int ld, bool vec) {
    if (vec) {
        const int q = dp >> 2;
        for (int idx = threadIdx.x; idx < MMD_TILE * q; idx += 256) {
            const int rr = idx / q, c = (idx - rr * q) << 2;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row0 + rr < rows && c < D) v = *reinterpret_cast<const float4*>(src + (size_t)(row0 + rr) * D + c);   // D % 4 == 0
            *reinterpret_cast<float4*>(dst + rr * ld + c) = v;
        }
    } else {
        for (int idx = threadIdx.x; idx < MMD_TILE * dp; idx += 256) {
            const int rr = idx / dp, c = idx - rr * dp;
            dst[rr * ld + c] = (row0 + rr < rows && c < D) ? src[(size_t)(row0 + rr) * D + c] : 0.f;
        }
    }
}

// |row|^2 of the 32 staged rows: thread t takes the words 4 (t & 7) + 32 q .. + 3 of row t >> 3; the total is valid in lanes with
// (t & 7) == 0, which store it.  Returns 0 x norm for a live row (NaN when the row is not finite), 0 otherwise.
__device__ __forceinline__ float mmd_norms(const float* __restrict__ tile, float* __restrict__ out, int dp, int ld, int live_rows) {
    const int rr = threadIdx.x >> 3, sub = threadIdx.x & 7;
    float s = 0.f;
    for (int c = sub * 4; c < dp; c += 32) {
        const float4 f = *reinterpret_cast<const float4*>(tile + rr * ld + c);
        s += (f.x * f.x + f.y * f.y) + (f.z * f.z + f.w * f.w);
    }
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    if (sub == 0) out[rr] = s;
    return (sub == 0 && rr < live_rows) ? s * 0.f : 0.f;
}

// column tile ct of a workgroup's run: z-workgroups walk [z tiles | y tiles], y-workgroups the y tiles
__device__ __forceinline__ void mmd_tile_of(bool zblock, int ct, int cN, const float* z, const float* y, int N, int M, const float*& B,
                                            int& NB, int& j0) {
    const bool second = zblock && ct >= cN;
    B = (zblock && !second) ? z : y;
    NB = (zblock && !second) ? N : M;
    j0 = (second ? ct - cN : ct) * MMD_TILE;
}

// float4 rows: column tile ct from global memory into NT registers per thread (a tile is 32 q4 <= 256 NT float4), zero past the end
template <int NT>
__device__ __forceinline__ void mmd_prefetch(float4 (&pf)[NT], bool zblock, int ct, int cN, const float* z, const float* y, int N, int M,
                                             int D, int q4) {
    const float* B;
    int NB, j0;
    mmd_tile_of(zblock, ct, cN, z, y, N, M, B, NB, j0);
#pragma unroll
    for (int u = 0; u < NT; ++u) {
        const int idx = threadIdx.x + 256 * u, rr = idx / q4, cc = (idx - rr * q4) << 2;
        pf[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (idx < MMD_TILE * q4 && j0 + rr < NB && cc < D) pf[u] = *reinterpret_cast<const float4*>(B + (size_t)(j0 + rr) * D + cc);
    }
}

template <int NT, bool IMQ>
__global__ void __launch_bounds__(256)
mmd_fwd_kernel(const float* __restrict__ z, const float* __restrict__ y, int N, int M, int D, MmdPlan p, MmdFn f, float czz, float czy,
               int biased, int vec, double* __restrict__ kpart, float* __restrict__ gpart) {
    extern __shared__ __align__(16) float mmd_smem[];
    __shared__ double red[4];
    const int ld = p.ld, dp = p.dp;
    float* As = mmd_smem;
    float* Bs = As + MMD_TILE * ld;
    float* Ws = Bs + MMD_TILE * ld;
    float* na = Ws + MMD_TILE * MMD_WLD;
    float* nb = na + MMD_TILE;
    float* rsw = nb + MMD_TILE;   // [2][32] row sums of w, one half per wj
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, g = lane >> 4, c = lane & 15;
    const int wi = wv >> 1, wj = wv & 1;   // Gram: this wave's 16 x 16 tile
    const int wr = wv & 1, wc = wv >> 1;   // gradient product: output rows 16 wr .., column tiles wc, wc + 2, ...

    const bool zblock = (int)blockIdx.x < p.nz;
    int rt, sp, c_lo, c_hi, NA;
    const float* A;
    if (zblock) {
        rt = blockIdx.x / p.ns_z;
        sp = blockIdx.x - rt * p.ns_z;
        c_lo = sp * p.tps_z;
        c_hi = min(c_lo + p.tps_z, p.cN + p.cM);
        A = z;
        NA = N;
    } else {
        const int b = blockIdx.x - p.nz;
        rt = b / p.ns_y;
        sp = b - rt * p.ns_y;
        c_lo = sp * p.tps_y;
        c_hi = min(c_lo + p.tps_y, p.cM);
        A = y;
        NA = M;
    }
    const int i0 = rt * MMD_TILE;
    const bool grad = zblock && gpart != nullptr;
    float fc[MMD_MAX_SCALES], fa[MMD_MAX_SCALES];
#pragma unroll
    for (int s = 0; s < MMD_MAX_SCALES; ++s) {
        fc[s] = f.c[s];
        fa[s] = f.a[s];
    }

    mmd_stage(As, A, NA, i0, D, dp, ld, vec != 0);
    __syncthreads();
    double k0 = 0.0, k1 = 0.0;   // z-workgroup: sums of k over the zz / zy tiles; y-workgroup: yy / unused
    k0 += (double)mmd_norms(As, na, dp, ld, NA - i0);

    f32x4 gacc[NT];
#pragma unroll
    for (int u = 0; u < NT; ++u) gacc[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float rs[4] = {0.f, 0.f, 0.f, 0.f};   // row sums of w over this lane's columns, rows 16 wi + 4 g + r

    // float4 rows: the next column tile travels from global memory into registers while this one is worked on (a tile is
    // 32 dp / 4 <= 256 NT float4, so NT per thread)
    const int q4 = dp >> 2;
    const int cN = p.cN;
    float4 pf[NT];
    if (vec && c_lo < c_hi) mmd_prefetch<NT>(pf, zblock, c_lo, cN, z, y, N, M, D, q4);

    for (int ct = c_lo; ct < c_hi; ++ct) {
        const bool second = zblock && ct >= cN;        // the zy block
        const bool self = !second;                      // zz or yy: B is A's own array
        const float* B;
        int NB, j0;
        mmd_tile_of(zblock, ct, cN, z, y, N, M, B, NB, j0);
        const float coef = second ? czy : czz;

        __syncthreads();   // the previous tile's readers of Bs, nb and Ws are done
        if (vec) {
#pragma unroll
            for (int u = 0; u < NT; ++u) {
                const int idx = t + 256 * u, rr = idx / q4, cc = (idx - rr * q4) << 2;
                if (idx < MMD_TILE * q4) *reinterpret_cast<float4*>(Bs + rr * ld + cc) = pf[u];
            }
        } else {
            mmd_stage(Bs, B, NB, j0, D, dp, ld, false);
        }
        __syncthreads();
        if (vec && ct + 1 < c_hi) mmd_prefetch<NT>(pf, zblock, ct + 1, cN, z, y, N, M, D, q4);
        k0 += (double)mmd_norms(Bs, nb, dp, ld, NB - j0);

        // Gram tile of this wave; two accumulators take alternate steps
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        const float* ap = As + (wi * 16 + c) * ld + 4 * g;
        const float* bp = Bs + (wj * 16 + c) * ld + 4 * g;
        float4 av = *reinterpret_cast<const float4*>(ap), bv = *reinterpret_cast<const float4*>(bp);
        for (int kk = 0; kk < dp; kk += 16) {
            const int kn = kk + 16 < dp ? kk + 16 : kk;   // the next step's operands are read before this step's products
            const float4 an = *reinterpret_cast<const float4*>(ap + kn), bn = *reinterpret_cast<const float4*>(bp + kn);
            acc0 = mfma16(av.x, bv.x, acc0);
            acc1 = mfma16(av.y, bv.y, acc1);
            acc0 = mfma16(av.z, bv.z, acc0);
            acc1 = mfma16(av.w, bv.w, acc1);
            av = an;
            bv = bn;
        }
        __syncthreads();   // nb is complete

        float kt = 0.f;
        const int lj = wj * 16 + c, gj = j0 + lj;
        const float nbj = nb[lj];
        float rr[4], kv[4], wvv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int li = wi * 16 + g * 4 + r;
            float v = na[li] + nbj - 2.f * (acc0[r] + acc1[r]);
            v = v < 0.f ? 0.f : v;   // NaN fails the comparison and stays
            rr[r] = (self && i0 + li == gj) ? 0.f : v;
        }
        mmd_kw4<IMQ>(fc, fa, f.S, rr, kv, wvv);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int li = wi * 16 + g * 4 + r, gi = i0 + li;
            const bool valid = gi < NA && gj < NB;
            const bool diag = self && gi == gj;
            kt += (valid && !(diag && !biased)) ? kv[r] : 0.f;
            if (grad) {
                const float wm = (valid && !diag) ? wvv[r] * coef : 0.f;
                Ws[li * MMD_WLD + lj] = wm;
                rs[r] += wm;
            }
        }
        if (second) k1 += (double)kt;
        else k0 += (double)kt;

        if (grad) {
            __syncthreads();   // the w tile is complete
            const float4 w0 = *reinterpret_cast<const float4*>(Ws + (wr * 16 + c) * MMD_WLD + 4 * g);
            const float4 w1 = *reinterpret_cast<const float4*>(Ws + (wr * 16 + c) * MMD_WLD + 16 + 4 * g);
#pragma unroll 1
            for (int h = 0; h < 2; ++h) {   // the two halves of k one after the other: 4 NT operand loads in flight, not 8 NT
                const float4 wh = h ? w1 : w0;
                const float aw[4] = {wh.x, wh.y, wh.z, wh.w};
                const float* bh = Bs + (4 * g + 16 * h) * ld + c + wc * 16;
                if (dp == 32 * NT) {   // every accumulator tile is live: straight-line loads and products
#pragma unroll
                    for (int s = 0; s < 4; ++s)
#pragma unroll
                        for (int u = 0; u < NT; ++u) gacc[u] = mfma16(aw[s], bh[s * ld + 32 * u], gacc[u]);
                } else {
#pragma unroll
                    for (int s = 0; s < 4; ++s)
#pragma unroll
                        for (int u = 0; u < NT; ++u)
                            if ((wc + 2 * u) * 16 < dp) gacc[u] = mfma16(aw[s], bh[s * ld + 32 * u], gacc[u]);   // wave-uniform
                }
            }
        }
    }

    if (grad) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float v = rs[r];
            v += __shfl_xor(v, 1, 64);
            v += __shfl_xor(v, 2, 64);
            v += __shfl_xor(v, 4, 64);
            v += __shfl_xor(v, 8, 64);
            if (c == 0) rsw[wj * MMD_TILE + wi * 16 + g * 4 + r] = v;
        }
        __syncthreads();
        float* out = gpart + (size_t)sp * N * D;
#pragma unroll
        for (int u = 0; u < NT; ++u) {
            const int d = (wc + 2 * u) * 16 + c;
            if (d < D) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int li = wr * 16 + g * 4 + r, gi = i0 + li;
                    if (gi < N) out[(size_t)gi * D + d] = (rsw[li] + rsw[MMD_TILE + li]) * As[li * ld + d] - gacc[u][r];
                }
            }
        }
    }
    k0 = mmd_block_sum(k0, red);
    k1 = mmd_block_sum(k1, red);
    if (t == 0) {
        kpart[(size_t)blockIdx.x * 2] = k0;
        kpart[(size_t)blockIdx.x * 2 + 1] = k1;
    }
}

// block 0: terms = normalised sums of the partials in index order, loss[0 .. rep) = scale (Ezz + Eyy - 2 Ezy);
// every block: G[e] = gpart[0][e] + gpart[1][e] + ... in index order (G == NULL: one block, no gradient)
__global__ void __launch_bounds__(256)
mmd_finish_kernel(const double* __restrict__ kpart, int nz, int ny, double izz, double iyy, double izy, double scale, int rep,
                  float* __restrict__ loss, float* __restrict__ terms, const float* __restrict__ gpart, int ns, size_t nd,
                  float* __restrict__ G) {
    __shared__ double red[4];
    if (G) {
        for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < nd; e += (size_t)gridDim.x * 256) {
            float a = gpart[e];
            for (int s = 1; s < ns; ++s) a += gpart[(size_t)s * nd + e];
            G[e] = a;
        }
    }
    if (blockIdx.x != 0) return;
    double a = 0.0, b = 0.0, cyy = 0.0;
    for (int i = threadIdx.x; i < nz; i += 256) {
        a += kpart[(size_t)i * 2];
        b += kpart[(size_t)i * 2 + 1];
    }
    for (int i = threadIdx.x; i < ny; i += 256) cyy += kpart[((size_t)nz + i) * 2];
    const double ezz = izz * mmd_block_sum(a, red), ezy = izy * mmd_block_sum(b, red), eyy = iyy * mmd_block_sum(cyy, red);
    const float v = (float)(scale * (ezz + eyy - 2.0 * ezy));
    if (threadIdx.x == 0) {
        terms[0] = (float)ezz;
        terms[1] = (float)eyy;
        terms[2] = (float)ezy;
    }
    for (int q = threadIdx.x; q < rep; q += 256) loss[q] = v;
}

// gz[e] = gadd[e] + (sum_b gout[b]) G[e]: every wave sums gout itself (lanes take every 64th, fixed exchange tree)
__global__ void __launch_bounds__(256)
mmd_bwd_kernel(const float* __restrict__ gout, int ng, const float* __restrict__ gadd, const float* __restrict__ G, size_t nd,
               float* __restrict__ gz) {
    float gs = 0.f;
    for (int q = threadIdx.x & 63; q < ng; q += 64) gs += gout[q];
    gs = wave_sum(gs);
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < nd; e += (size_t)gridDim.x * 256) {
        const float v = __fmul_rn(gs, G[e]);   // rounded on its own: gadd is ADDED to the same bits, never fused in
        gz[e] = gadd ? gadd[e] + v : v;
    }
}

extern "C" int64_t otvae_mmd_ws(int N, int M, int D) {
    MmdPlan p;
    if (!mmd_plan(N, M, D, &p)) return -1;
    return (int64_t)mmd_kpart_bytes(p) + (int64_t)p.ns_z * N * D * (int64_t)sizeof(float);
}

template <int NT, bool IMQ>
static int mmd_launch(const float* z, const float* y, int N, int M, int D, const MmdPlan& p, const MmdFn& f, float czz, float czy,
                      int biased, int vec, double* kpart, float* gpart, hipStream_t st) {
    const size_t lds = mmd_lds_bytes(p);
    // the kernel also has 32 bytes of static LDS: ask for what the widest D needs, not all 160 KiB
    const size_t most = ((size_t)2 * MMD_TILE * (MMD_MAX_D + 4) + MMD_TILE * MMD_WLD + 4 * MMD_TILE) * sizeof(float);
    if (int rc = otvae_lds_grant<&mmd_fwd_kernel<NT, IMQ>>("otvae_mmd_fwd", lds, most)) return rc;
    mmd_fwd_kernel<NT, IMQ><<<dim3(p.nz + p.ny), 256, lds, st>>>(z, y, N, M, D, p, f, czz, czy, biased, vec, kpart, gpart);
    OTVAE_CHECK_LAUNCH("otvae_mmd_fwd(tiles)");
    return OTVAE_OK;
}

extern "C" int otvae_mmd_fwd(const float* z, const float* y, int N, int M, int D, int kernel, const double* scales, int nscales,
                             double sigma2, int unbiased, double scale, int loss_rep, void* ws, float* loss, float* terms, float* G,
                             void* stream) {
    OTVAE_REQUIRE(z && y && scales && ws && loss && terms, "otvae_mmd_fwd: NULL argument");
    OTVAE_REQUIRE(N > 0 && M > 0 && D > 0 && loss_rep > 0, "otvae_mmd_fwd: bad sizes (N %d, M %d, D %d, loss_rep %d)", N, M, D, loss_rep);
    OTVAE_REQUIRE(kernel == 0 || kernel == 1, "otvae_mmd_fwd: kernel must be 0 (imq) or 1 (rbf), got %d", kernel);
    OTVAE_REQUIRE(nscales >= 1 && nscales <= MMD_MAX_SCALES, "otvae_mmd_fwd: 1 .. %d scales, got %d", MMD_MAX_SCALES, nscales);
    OTVAE_REQUIRE(sigma2 > 0.0, "otvae_mmd_fwd: sigma2 must be positive");
    OTVAE_REQUIRE(!unbiased || (N >= 2 && M >= 2), "otvae_mmd_fwd: the unbiased estimator needs N, M >= 2 (got %d, %d)", N, M);
    OTVAE_REQUIRE((uintptr_t)ws % 16 == 0, "otvae_mmd_fwd: the workspace must be 16-byte aligned");
    MmdPlan p;
    if (!mmd_plan(N, M, D, &p)) {
        otvae_set_error("otvae_mmd_fwd: D = %d, N = %d, M = %d is beyond 1 <= D <= %d with N D, M D < 2^31", D, N, M, MMD_MAX_D);
        return OTVAE_EUNSUPPORTED;
    }
    MmdFn f = {};
    f.S = nscales;
    for (int k = 0; k < nscales; ++k) {
        OTVAE_REQUIRE(scales[k] > 0.0, "otvae_mmd_fwd: scale %d is not positive", k);
        const double Ck = 2.0 * (double)D * sigma2 * scales[k];
        if (kernel == 0) {
            f.c[k] = (float)Ck;
        } else {
            f.c[k] = (float)(1.0 / Ck);
            f.a[k] = (float)(-1.4426950408889634 / Ck);
        }
    }
    const double dn = (double)N, dm = (double)M;
    const double izz = unbiased ? 1.0 / (dn * (dn - 1.0)) : 1.0 / (dn * dn);
    const double iyy = unbiased ? 1.0 / (dm * (dm - 1.0)) : 1.0 / (dm * dm);
    const double izy = 1.0 / (dn * dm);
    const float czz = (float)(-4.0 * scale * izz), czy = (float)(4.0 * scale * izy);
    const int vec = D % 4 == 0 && (uintptr_t)z % 16 == 0 && (uintptr_t)y % 16 == 0;
    double* kpart = (double*)ws;
    float* gpart = G ? (float*)((char*)ws + mmd_kpart_bytes(p)) : nullptr;
    hipStream_t st = (hipStream_t)stream;
    int rc;
#define MMD_GO(NT_) \
    rc = kernel == 0 ? mmd_launch<NT_, true>(z, y, N, M, D, p, f, czz, czy, !unbiased, vec, kpart, gpart, st) \
                     : mmd_launch<NT_, false>(z, y, N, M, D, p, f, czz, czy, !unbiased, vec, kpart, gpart, st)
    if (D <= 32) MMD_GO(1);
    else if (D <= 64) MMD_GO(2);
    else if (D <= 128) MMD_GO(4);
    else MMD_GO(16);   // (an 8-tile instantiation for D <= 256 compiled to more registers than this one: not built)
#undef MMD_GO
    if (rc != OTVAE_OK) return rc;
    const size_t nd = (size_t)N * D;
    const int fin = G ? imin(cdiv((int64_t)nd, 256), 2048) : 1;
    mmd_finish_kernel<<<fin, 256, 0, st>>>(kpart, p.nz, p.ny, izz, iyy, izy, scale, loss_rep, loss, terms, gpart, p.ns_z, nd, G);
    OTVAE_CHECK_LAUNCH("otvae_mmd_fwd(finish)");
    return OTVAE_OK;
}

extern "C" int otvae_mmd_bwd(const float* gout, int ng, const float* gadd, const float* G, int N, int D, float* gz, void* stream) {
    OTVAE_REQUIRE(gout && G && gz, "otvae_mmd_bwd: NULL argument");
    OTVAE_REQUIRE(ng > 0 && N > 0 && D > 0 && (int64_t)N * D < (int64_t)1 << 31, "otvae_mmd_bwd: bad sizes (ng %d, N %d, D %d)", ng, N, D);
    const size_t nd = (size_t)N * D;
    mmd_bwd_kernel<<<imin(cdiv((int64_t)nd, 256), 1024), 256, 0, (hipStream_t)stream>>>(gout, ng, gadd, G, nd, gz);
    OTVAE_CHECK_LAUNCH("otvae_mmd_bwd");
    return OTVAE_OK;
}
