// Sinkhorn divergence between a minibatch of latents z[N][D] and prior draws y[M][D] (Genevay, Peyre, Cuturi 2018), the debiased form
// of the minibatch-OT prior's loss:
//
//   S(z, y) = W(z, y) - W(z, z) / 2 - W(y, y) / 2,   W(p, q) = <C_pq, pi_pq>,   C_pq,ij = |p_i - q_j|^2
//
// with the three entropic plans taken at ONE absolute epsilon (all three costs are divided by cmax = max C_zy) and after the SAME number
// of iterations, so that the bias terms cancel and S(z, z) = 0.  Four stages:
//   cost      one launch, one workgroup per tile: every cross tile (arithmetic and tile maxima of sqdist_mfma_kernel / sqdist_kernel,
//             sinkhorn.hip) and the upper-triangle tiles of both self blocks, mirrored at the store
//   solve     sinkhorn_impl through otvae_sk_solve_uniform, all three problems on the cross block's tile maxima
//   read-out  <C, pi> of the three problems in ot_cost_partial's order (fp64), the plans the gradient needs copied out of the solver's
//             batch on the way; then the signed combination, replicated N times
//   gradient  one launch: [pi_zy | -(pi_zz + pi_zz^T) / 2] [y ; z] and the row sums of that operand
#include "sinkhorn_rows.h"
#include "sinkhorn_solve.h"

#define SD_MAX_ROWS 32768  // N, M: every matrix stays below 2^31 entries, every tile count fits an int
#define SD_PARTS 256       // fp64 partial sums per problem (COST_PARTS of sinkhorn.hip: the cross term has to come out bit-identical)

// ------------------------------------------------------------------------------------------------ cost tiles
// workgroup `idx` of the cost launch -> its tile: kind 0 = cross (tn x tm tiles, row major), 1 = z against z, 2 = y against y (the
// tiles bi <= bj of a t x t grid, row after row)
__device__ __forceinline__ void sd_tile(int idx, int tn, int tm, int& kind, int& bi, int& bj) {
    kind = 0;
    if (idx < tn * tm) {
        bi = idx / tm;
        bj = idx - bi * tm;
        return;
    }
    idx -= tn * tm;
    int t = tn;
    kind = 1;
    if (idx >= tn * (tn + 1) / 2) {
        idx -= tn * (tn + 1) / 2;
        t = tm;
        kind = 2;
    }
    bi = 0;
    while (idx >= t - bi) {
        idx -= t - bi;
        ++bi;
    }
    bj = bi + idx;
}
static int sd_tiles(int tn, int tm) { return tn * tm + tn * (tn + 1) / 2 + tm * (tm + 1) / 2; }

// Plain form (fp64): 16 x 16 tiles, the loop of sqdist_kernel.  pmax[rep][tn * tm]: the cross tile's maximum, once per problem of
// the solve.
template <typename T>
__global__ __launch_bounds__(256) void sd_cost_kernel(const T* __restrict__ z, const T* __restrict__ yv, int N, int M, int D, T* __restrict__ Czy,
                                                      T* __restrict__ Czz, T* __restrict__ Cyy, T* __restrict__ pmax, int rep) {
    __shared__ T xs[16][33], ys[16][33];
    __shared__ T s_mx[4];
    const int tn = (N + 15) / 16, tm = (M + 15) / 16;
    int kind, bi, bj;
    sd_tile(blockIdx.x, tn, tm, kind, bi, bj);
    const T* xb = kind == 2 ? yv : z;
    const T* yb = kind == 1 ? z : yv;
    const int R = kind == 2 ? M : N, S = kind == 1 ? N : M;  // rows of the tile's two sides
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int i = bi * 16 + ty, j = bj * 16 + tx;
    T dot = 0, xx = 0, yy = 0;
    for (int d0 = 0; d0 < D; d0 += 32) {
        for (int e = threadIdx.x; e < 16 * 32; e += 256) {
            const int r = e >> 5, d = e & 31;
            const int gi = bi * 16 + r, gj = bj * 16 + r;
            xs[r][d] = (gi < R && d0 + d < D) ? xb[(size_t)gi * D + d0 + d] : (T)0;
            ys[r][d] = (gj < S && d0 + d < D) ? yb[(size_t)gj * D + d0 + d] : (T)0;
        }
        __syncthreads();
#pragma unroll 8
        for (int d = 0; d < 32; ++d) {
            const T a = xs[ty][d], c = ys[tx][d];
            dot += a * c;
            xx += a * a;
            yy += c * c;
        }
        __syncthreads();
    }
    const T val = xx + yy - (T)2 * dot;
    if (kind) {  // a self block: the entries above the diagonal, each stored on both sides of it; the diagonal is zero
        T* Cm = kind == 1 ? Czz : Cyy;
        if (i < R && j < R) {
            if (i < j) {
                Cm[(size_t)i * R + j] = val;
                Cm[(size_t)j * R + i] = val;
            } else if (i == j) {
                Cm[(size_t)i * R + i] = (T)0;
            }
        }
        return;
    }
    if (i < N && j < M) Czy[(size_t)i * M + j] = val;
    T mx = wave_max((i < N && j < M) ? val : MathT<T>::ninf());
    if ((threadIdx.x & 63) == 0) s_mx[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        const T m01 = s_mx[0] > s_mx[1] ? s_mx[0] : s_mx[1], m23 = s_mx[2] > s_mx[3] ? s_mx[2] : s_mx[3];
        for (int b = 0; b < rep; ++b) pmax[(size_t)b * tn * tm + bi * tm + bj] = m01 > m23 ? m01 : m23;
    }
}

// fp32 on the matrix cores: the tile loop of sqdist_mfma_kernel (64 x 64 tile, 4 waves of 2 x 2 MFMA 16x16x4 tiles, K = D in chunks of
// 32 through LDS, norms from the staged rows), copied so that the cross block has that kernel's bits; what differs is where the two
// 64-row slabs come from and the store.
#define SD_KC 32
#define SD_LD 36  // floats per LDS row: 16-byte aligned rows, 4 banks apart
__global__ __launch_bounds__(256) void sd_cost_mfma_kernel(const float* __restrict__ z, const float* __restrict__ yv, int N, int M, int D,
                                                           float* __restrict__ Czy, float* __restrict__ Czz, float* __restrict__ Cyy,
                                                           float* __restrict__ pmax, int rep) {
    __shared__ __align__(16) float xs[64 * SD_LD], ys[64 * SD_LD];
    __shared__ float nx[64], ny[64], s_mx[4];
    const int tn = (N + 63) / 64, tm = (M + 63) / 64;
    int kind, bi, bj;
    sd_tile(blockIdx.x, tn, tm, kind, bi, bj);
    const float* xb = kind == 2 ? yv : z;
    const float* yb = kind == 1 ? z : yv;
    const int R = kind == 2 ? M : N, S = kind == 1 ? N : M;
    const int i0 = bi * 64, j0 = bj * 64;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, wi = w >> 1, wj = w & 1;
    const bool vec = (D & 3) == 0;
    f32x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[a][c] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float nrm = 0.f;  // thread t: half (t & 1) of row (t >> 1) of the 128 staged rows (0..63 of x, 64..127 of y)
    auto load4 = [&](const float* base, int row, int rows, int d) -> float4 {
        if (row >= rows) return make_float4(0.f, 0.f, 0.f, 0.f);
        const float* p = base + (size_t)row * D + d;
        if (vec && d + 3 < D) return *reinterpret_cast<const float4*>(p);
        return make_float4(d < D ? p[0] : 0.f, d + 1 < D ? p[1] : 0.f, d + 2 < D ? p[2] : 0.f, d + 3 < D ? p[3] : 0.f);
    };
    const int sr = t >> 3, sc = (t & 7) * 4;  // staging: rows sr, sr + 32; 4 floats at column sc
    float4 px[2], py[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        px[u] = load4(xb, i0 + sr + 32 * u, R, sc);
        py[u] = load4(yb, j0 + sr + 32 * u, S, sc);
    }
    for (int d0 = 0; d0 < D; d0 += SD_KC) {
        __syncthreads();  // the previous chunk's readers are done
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            *reinterpret_cast<float4*>(&xs[(sr + 32 * u) * SD_LD + sc]) = px[u];
            *reinterpret_cast<float4*>(&ys[(sr + 32 * u) * SD_LD + sc]) = py[u];
        }
        __syncthreads();
        if (d0 + SD_KC < D) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                px[u] = load4(xb, i0 + sr + 32 * u, R, d0 + SD_KC + sc);
                py[u] = load4(yb, j0 + sr + 32 * u, S, d0 + SD_KC + sc);
            }
        }
        {
            const int rr = t >> 1;
            const float* src = (rr < 64 ? xs + rr * SD_LD : ys + (rr - 64) * SD_LD) + (t & 1) * 16;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 f = *reinterpret_cast<const float4*>(src + 4 * q);
                nrm += (f.x * f.x + f.y * f.y) + (f.z * f.z + f.w * f.w);
            }
        }
#pragma unroll
        for (int kk = 0; kk < SD_KC; kk += 16) {
            float4 av[2], bv[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                av[a] = *reinterpret_cast<const float4*>(&xs[(wi * 32 + a * 16 + (lane & 15)) * SD_LD + kk + 4 * (lane >> 4)]);
                bv[a] = *reinterpret_cast<const float4*>(&ys[(wj * 32 + a * 16 + (lane & 15)) * SD_LD + kk + 4 * (lane >> 4)]);
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    acc[a][c] = mfma16(av[a].x, bv[c].x, acc[a][c]);
                    acc[a][c] = mfma16(av[a].y, bv[c].y, acc[a][c]);
                    acc[a][c] = mfma16(av[a].z, bv[c].z, acc[a][c]);
                    acc[a][c] = mfma16(av[a].w, bv[c].w, acc[a][c]);
                }
        }
    }
    nrm += __shfl_xor(nrm, 1, 64);
    if ((t & 1) == 0) {
        if ((t >> 1) < 64) nx[t >> 1] = nrm;
        else ny[(t >> 1) - 64] = nrm;
    }
    __syncthreads();
    if (kind) {
        // a self block: a lane's 4 accumulator entries are 4 consecutive rows li of one column lj, i.e. 16 contiguous bytes of row lj
        // of the mirrored tile.  Off the diagonal tile every entry lies above the diagonal; on it, the entries with i < j are the ones
        // that count (stored on both sides), and the diagonal is zero.
        float* Cm = kind == 1 ? Czz : Cyy;
        const bool vecr = (R & 3) == 0 && ((uintptr_t)Cm & 15) == 0;  // (the blocks lie back to back: C_yy starts N M + N N floats in)
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int li = wi * 32 + a * 16 + (lane >> 4) * 4, lj = wj * 32 + c * 16 + (lane & 15);
                const int gi = i0 + li, gj = j0 + lj;
                float val[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) val[r] = nx[li + r] + ny[lj] - 2.f * acc[a][c][r];
                if (gj >= R) continue;
                if (bi != bj && vecr && gi + 3 < R) {
                    *reinterpret_cast<float4*>(&Cm[(size_t)gj * R + gi]) = make_float4(val[0], val[1], val[2], val[3]);
#pragma unroll
                    for (int r = 0; r < 4; ++r) Cm[(size_t)(gi + r) * R + gj] = val[r];
                    continue;
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (gi + r >= R) continue;
                    if (gi + r < gj) {
                        Cm[(size_t)(gi + r) * R + gj] = val[r];
                        Cm[(size_t)gj * R + gi + r] = val[r];
                    } else if (gi + r == gj) {
                        Cm[(size_t)gj * R + gj] = 0.f;
                    }
                }
            }
        return;
    }
    float mx = -INFINITY;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int li = wi * 32 + a * 16 + (lane >> 4) * 4 + r, lj = wj * 32 + c * 16 + (lane & 15);
                const float val = nx[li] + ny[lj] - 2.f * acc[a][c][r];
                if (i0 + li < N && j0 + lj < M) {
                    Czy[(size_t)(i0 + li) * M + j0 + lj] = val;
                    mx = val > mx ? val : mx;
                }
            }
    mx = wave_max(mx);
    if (lane == 0) s_mx[w] = mx;
    __syncthreads();
    if (t == 0) {
        const float m = fmaxf(fmaxf(s_mx[0], s_mx[1]), fmaxf(s_mx[2], s_mx[3]));
        for (int b = 0; b < rep; ++b) pmax[(size_t)b * tn * tm + bi * tm + bj] = m;
    }
}

// ------------------------------------------------------------------------------------------------ read-out
template <typename T>
struct SdProblems {   // the three problems, in the order cross, z-z, y-y
    const T* C[3];
    const T* pi[3];
    T* out[3];        // where the plan goes for the gradient (NULL: nowhere)
    size_t total[3];
};
__device__ __forceinline__ bool sd_starved(const int32_t* __restrict__ iters, int n) {
    bool bad = false;
    for (int q = 0; q < n; ++q) bad |= iters[q] < 0;
    return bad;
}

// ws[b][p] = the p-th partial of <C_b, pi_b>: ot_cost_partial's sum (sinkhorn.hip), problem b on min(256, cdiv(total_b, 1024)) blocks.
// The plans the gradient reads leave the solver's batch here; all NaN if any of the solves was starved.
template <typename T>
__global__ __launch_bounds__(256) void sd_cost_partial(SdProblems<T> p, const int32_t* __restrict__ iters, int n_iters,
                                                       double* __restrict__ ws) {
    __shared__ double red[4];
    const int b = blockIdx.y;
    const size_t total = p.total[b];
    const size_t parts = total < (size_t)SD_PARTS * 1024 ? (total + 1023) / 1024 : SD_PARTS;
    if (blockIdx.x >= parts) return;
    const T* __restrict__ Cm = p.C[b];
    const T* __restrict__ pi = p.pi[b];
    T* __restrict__ out = p.out[b];
    const bool bad = sd_starved(iters, n_iters);
    double s = 0.0;
    for (size_t e = blockIdx.x * (size_t)256 + threadIdx.x; e < total; e += parts * 256) {
        const T q = pi[e];
        s += (double)Cm[e] * (double)q;
        if (out) out[e] = bad ? (T)NAN : q;
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) ws[(size_t)b * SD_PARTS + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// terms[b] = the partials of problem b added in index order (ot_cost_final's sum); loss[i] = scale (terms[0] - terms[1] / 2 -
// terms[2] / 2) for i < N; iters_out = the iteration count, -1 (and NaN everywhere) if a solve was starved
template <typename T>
__global__ __launch_bounds__(256) void sd_final(const double* __restrict__ ws, size_t t0, size_t t1, size_t t2, double scale, int N,
                                                const int32_t* __restrict__ iters, int n_iters, T* __restrict__ loss,
                                                double* __restrict__ terms, int32_t* __restrict__ iters_out) {
    __shared__ double s_t[3];
    if (threadIdx.x < 3) {
        const size_t total = threadIdx.x == 0 ? t0 : threadIdx.x == 1 ? t1 : t2;
        const int parts = (int)(total < (size_t)SD_PARTS * 1024 ? (total + 1023) / 1024 : SD_PARTS);
        double s = 0.0;
        for (int q = 0; q < parts; ++q) s += ws[(size_t)threadIdx.x * SD_PARTS + q];
        s_t[threadIdx.x] = sd_starved(iters, n_iters) ? (double)NAN : s;
    }
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x < 3) terms[threadIdx.x] = s_t[threadIdx.x];
    if (blockIdx.x == 0 && threadIdx.x == 3) *iters_out = sd_starved(iters, n_iters) ? -1 : iters[0];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < N) loss[i] = (T)(scale * (s_t[0] - 0.5 * s_t[1] - 0.5 * s_t[2]));
}

extern "C" int64_t otvae_sinkhorn_div_ws(int dtype, int N, int M) {
    if (N <= 0 || M <= 0 || N > SD_MAX_ROWS || M > SD_MAX_ROWS || dtype < 0 || dtype > 1) return -1;
    const size_t es = dtype ? 8 : 4;
    const int L = N > M ? N : M;
    const int64_t solver = otvae_sinkhorn_ws(dtype, N == M ? 3 : 1, L, L);
    if (solver < 0) return -1;
    const size_t mats = align256(((size_t)N * M + (size_t)N * N + (size_t)M * M) * es);
    // tile maxima x 3, partial sums, iteration counts, C x 3, pi x 3, u x 3, v x 3, the solver's own
    return (int64_t)(align256((size_t)3 * otvae_sqdist_max_parts(dtype, N, M) * es) + align256(3 * SD_PARTS * sizeof(double)) + 256 +
                     2 * mats + 2 * align256((size_t)3 * L * es)) + solver;
}

template <typename T>
static int sd_fwd(const T* z, const T* y, int N, int M, int D, double reg, int max_iter, double loss_scale, bool batched, void* ws, T* loss,
                  double* terms, T* pi_zy, T* pi_zz, int32_t* iters, hipStream_t st) {
    constexpr int dtype = sizeof(T) == 8;
    const int tile = dtype ? 16 : 64, tn = cdiv(N, tile), tm = cdiv(M, tile), P = tn * tm, L = N > M ? N : M;
    const size_t szy = (size_t)N * M, szz = (size_t)N * N, syy = (size_t)M * M;
    char* w = (char*)ws;
    T* pmax = (T*)w;
    w += align256((size_t)3 * P * sizeof(T));
    double* cws = (double*)w;
    w += align256(3 * SD_PARTS * sizeof(double));
    int32_t* its = (int32_t*)w;
    w += 256;
    T* Cm = (T*)w;  // C_zy | C_zz | C_yy, back to back: [3][N][N] when N == M
    w += align256((szy + szz + syy) * sizeof(T));
    T* pi = (T*)w;  // the plans, likewise
    w += align256((szy + szz + syy) * sizeof(T));
    T* u = (T*)w;
    w += align256((size_t)3 * L * sizeof(T));
    T* v = (T*)w;
    w += align256((size_t)3 * L * sizeof(T));
    const int nb = batched ? 3 : 1;
    if constexpr (dtype == 0)
        sd_cost_mfma_kernel<<<sd_tiles(tn, tm), 256, 0, st>>>(z, y, N, M, D, Cm, Cm + szy, Cm + szy + szz, pmax, nb);
    else
        sd_cost_kernel<T><<<sd_tiles(tn, tm), 256, 0, st>>>(z, y, N, M, D, Cm, Cm + szy, Cm + szy + szz, pmax, nb);
    OTVAE_CHECK_LAUNCH("otvae_sinkhorn_div_fwd(cost matrices)");
    // The three solves share one stream, always: the persistent solver's residency guard counts only its own launch, and two spinning
    // solves that together exceed the device would each run out their bounded wait.
    if (batched) {
        if (const int rc = otvae_sk_solve_uniform(dtype, Cm, 3, N, N, reg, max_iter, pmax, P, w, pi, u, v, its, st)) return rc;
    } else {
        const size_t off[3] = {0, szy, szy + szz};
        const int rows[3] = {N, N, M}, cols[3] = {M, N, M};
        for (int b = 0; b < 3; ++b)
            if (const int rc = otvae_sk_solve_uniform(dtype, Cm + off[b], 1, rows[b], cols[b], reg, max_iter, pmax, P, w, pi + off[b], u, v,
                                                      its + b, st))
                return rc;
    }
    SdProblems<T> p;
    p.C[0] = Cm, p.C[1] = Cm + szy, p.C[2] = Cm + szy + szz;
    p.pi[0] = pi, p.pi[1] = pi + szy, p.pi[2] = pi + szy + szz;
    p.out[0] = pi_zy, p.out[1] = pi_zz, p.out[2] = nullptr;
    p.total[0] = szy, p.total[1] = szz, p.total[2] = syy;
    const size_t most = szy > szz ? (szy > syy ? szy : syy) : (szz > syy ? szz : syy);
    sd_cost_partial<T><<<dim3(imin(SD_PARTS, cdiv(most, 1024)), 3), 256, 0, st>>>(p, its, batched ? 1 : 3, cws);
    sd_final<T><<<cdiv(N, 256), 256, 0, st>>>(cws, szy, szz, syy, loss_scale, N, its, batched ? 1 : 3, loss, terms, iters);
    OTVAE_CHECK_LAUNCH("otvae_sinkhorn_div_fwd(read-out)");
    return OTVAE_OK;
}

extern "C" int otvae_sinkhorn_div_fwd(int dtype, const void* z, const void* y, int N, int M, int D, double reg, int max_iter,
                                      double loss_scale, int batched, void* ws, void* loss, double* terms, void* pi_zy, void* pi_zz,
                                      int32_t* iters, void* stream) {
    OTVAE_REQUIRE(z && y && ws && loss && terms && pi_zy && pi_zz && iters, "otvae_sinkhorn_div_fwd: NULL argument");
    OTVAE_REQUIRE(dtype == 0 || dtype == 1, "otvae_sinkhorn_div_fwd: dtype must be 0 (fp32) or 1 (fp64)");
    OTVAE_REQUIRE(N > 0 && M > 0 && D > 0 && max_iter >= 0 && reg > 0.0, "otvae_sinkhorn_div_fwd: bad sizes");
    OTVAE_REQUIRE(batched >= -1 && batched <= 1 && (batched != 1 || N == M), "otvae_sinkhorn_div_fwd: one batch of three needs N == M");
    if (N > SD_MAX_ROWS || M > SD_MAX_ROWS) {
        otvae_set_error("otvae_sinkhorn_div_fwd: built for N, M <= %d, got N = %d, M = %d", SD_MAX_ROWS, N, M);
        return OTVAE_EUNSUPPORTED;
    }
    OTVAE_REQUIRE(dtype == 1 || ((uintptr_t)z % 16 == 0 && (uintptr_t)y % 16 == 0), "otvae_sinkhorn_div_fwd: fp32 inputs must be 16-byte aligned");
    const bool batch = batched < 0 ? N == M : batched == 1;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == 0)
        return sd_fwd<float>((const float*)z, (const float*)y, N, M, D, reg, max_iter, loss_scale, batch, ws, (float*)loss, terms,
                             (float*)pi_zy, (float*)pi_zz, iters, st);
    return sd_fwd<double>((const double*)z, (const double*)y, N, M, D, reg, max_iter, loss_scale, batch, ws, (double*)loss, terms,
                          (double*)pi_zy, (double*)pi_zz, iters, st);
}

// ------------------------------------------------------------------------------------------------ gradient
// gz_i = gadd_i + 2 s (z_i rs_i - sum_k A_ik B_k),  A = [pi_zy | -(pi_zz + pi_zz^T) / 2]  (N x (M + N)),  B = [y ; z],  rs_i = sum_k A_ik
//
// Plain form (fp64): ot_cost_grad_kernel's 32 x 32 tiles walked over both halves of K; in the second half the tile of pi_zz^T is read
// as rows of pi_zz and turned in LDS.
template <typename T>
__global__ __launch_bounds__(256) void sd_grad_kernel(const T* __restrict__ z, const T* __restrict__ y, const T* __restrict__ pzy,
                                                      const T* __restrict__ pzz, const T* __restrict__ g, int ng, T scale,
                                                      const T* __restrict__ gadd, int N, int M, int D, T* __restrict__ gz) {
    __shared__ T ps[32][33], ys[32][33], pt[32][33];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int i0 = blockIdx.y * 32, d0 = blockIdx.x * 32;
    T acc[2][2] = {{(T)0, (T)0}, {(T)0, (T)0}}, rs[2] = {(T)0, (T)0};
    for (int half = 0; half < 2; ++half) {
        const int K = half ? N : M;
        const T* __restrict__ pm = half ? pzz : pzy;
        const T* __restrict__ bm = half ? z : y;
        for (int j0 = 0; j0 < K; j0 += 32) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int e = threadIdx.x + 256 * u, r = e >> 5, c = e & 31;
                ps[r][c] = (i0 + r < N && j0 + c < K) ? pm[(size_t)(i0 + r) * K + j0 + c] : (T)0;          // [i][j]
                ys[r][c] = (j0 + r < K && d0 + c < D) ? bm[(size_t)(j0 + r) * D + d0 + c] : (T)0;          // [j][d]
                if (half) pt[r][c] = (j0 + r < N && i0 + c < N) ? pzz[(size_t)(j0 + r) * N + i0 + c] : (T)0;  // [j][i]
            }
            __syncthreads();
            if (half) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {  // every thread turns the entries it staged itself
                    const int e = threadIdx.x + 256 * u, r = e >> 5, c = e & 31;
                    ps[r][c] = (T)-0.5 * (ps[r][c] + pt[c][r]);
                }
                __syncthreads();
            }
#pragma unroll 8
            for (int j = 0; j < 32; ++j) {
                const T p0 = ps[ty][j], p1 = ps[ty + 16][j], y0 = ys[j][tx], y1 = ys[j][tx + 16];
                rs[0] += p0;
                rs[1] += p1;
                acc[0][0] += p0 * y0;
                acc[0][1] += p0 * y1;
                acc[1][0] += p1 * y0;
                acc[1][1] += p1 * y1;
            }
            __syncthreads();
        }
    }
    T gs = (T)0;  // the upstream gradient of every replica of the loss, summed in index order by every thread alike
    for (int q = 0; q < ng; ++q) gs += g[q];
    const T two_g = (T)2 * scale * gs;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int i = i0 + ty + 16 * a, d = d0 + tx + 16 * c;
            if (i < N && d < D) {
                const T val = two_g * (rs[a] * z[(size_t)i * D + d] - acc[a][c]);
                gz[(size_t)i * D + d] = gadd ? gadd[(size_t)i * D + d] + val : val;
            }
        }
}

// fp32 on the matrix cores, after ot_cost_grad_mfma_kernel (sinkhorn.hip): a workgroup owns one 16 x 16 tile of gz, its 4 waves split
// each half of K into 4 contiguous ranges and accumulate one MFMA 16x16x4 tile each, A and B straight from global memory (L2
// resident), the 4 partial tiles combined through LDS in wave order.  In the second half the A operand also needs pi_zz[k][i], 16 rows
// i of 64 columns k per step: the wave reads them as 64-byte pieces of 64 ROWS of pi_zz (4 lanes per row, 16-byte loads) into a
// [k][i] tile in LDS and takes its operands from there.
#define SD_TLD 20  // floats per row of that tile: 16-byte aligned rows
__global__ __launch_bounds__(256) void sd_grad_mfma_kernel(const float* __restrict__ z, const float* __restrict__ y,
                                                           const float* __restrict__ pzy, const float* __restrict__ pzz,
                                                           const float* __restrict__ g, int ng, float scale, const float* __restrict__ gadd,
                                                           int N, int M, int D, float* __restrict__ gz) {
    __shared__ float part[3][5][64];
    __shared__ __align__(16) float tt[4][64 * SD_TLD];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int i0 = blockIdx.y * 16, d0 = blockIdx.x * 16;
    const int row = i0 + (lane & 15), col = d0 + (lane & 15), kq = 4 * (lane >> 4);
    const bool row_ok = row < N, col_ok = col < D;
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
    float rs = 0.f;
    // 4 consecutive k of this lane's row of `pm` (K columns), zero beyond k_hi
    auto loadA = [&](const float* __restrict__ pm, int K, int kk, int k_hi) -> float4 {
        if (!row_ok || kk >= k_hi) return make_float4(0.f, 0.f, 0.f, 0.f);
        const float* prow = pm + (size_t)row * K;
        if ((K & 3) == 0 && kk + 3 < k_hi) return *reinterpret_cast<const float4*>(prow + kk);
        return make_float4(prow[kk], kk + 1 < k_hi ? prow[kk + 1] : 0.f, kk + 2 < k_hi ? prow[kk + 2] : 0.f,
                           kk + 3 < k_hi ? prow[kk + 3] : 0.f);
    };
    auto loadB = [&](const float* __restrict__ bm, int kk, int k_hi) -> float {
        return (col_ok && kk < k_hi) ? bm[(size_t)kk * D + col] : 0.f;
    };
    {   // first half: A = pi_zy, B = y, K = M
        const int span = ((M + 63) / 64) * 16;  // k per wave, a multiple of 16
        const int k_lo = w * span, k_hi = min(M, k_lo + span);
        for (int k = k_lo; k < k_hi; k += 64) {
            float4 av[4];
            float bv[4][4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                av[u] = loadA(pzy, M, k + 16 * u + kq, k_hi);
#pragma unroll
                for (int s_ = 0; s_ < 4; ++s_) bv[u][s_] = loadB(y, k + 16 * u + kq + s_, k_hi);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                rs += (av[u].x + av[u].y) + (av[u].z + av[u].w);
                acc = mfma16(av[u].x, bv[u][0], acc);
                acc = mfma16(av[u].y, bv[u][1], acc);
                acc = mfma16(av[u].z, bv[u][2], acc);
                acc = mfma16(av[u].w, bv[u][3], acc);
            }
        }
    }
    {   // second half: A = -(pi_zz + pi_zz^T) / 2, B = z, K = N.  Every wave makes the same number of rounds (the barriers).
        const int span = ((N + 63) / 64) * 16;
        const int k_lo = w * span, k_hi = min(N, k_lo + span);
        const bool vecn = (N & 3) == 0;
        float* tw = tt[w];
        const int tr = lane >> 2, tc = (lane & 3) * 4;  // staging: row 16 u + tr of the round's 64, 4 floats at column tc
        for (int k = k_lo; k < k_lo + span; k += 64) {
            float4 av[4], cv[4];
            float bv[4][4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int kr = k + 16 * u + tr, ic = i0 + tc;
                float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
                if (kr < k_hi) {
                    const float* p = pzz + (size_t)kr * N + ic;
                    if (vecn && ic + 3 < N) q = *reinterpret_cast<const float4*>(p);
                    else q = make_float4(ic < N ? p[0] : 0.f, ic + 1 < N ? p[1] : 0.f, ic + 2 < N ? p[2] : 0.f, ic + 3 < N ? p[3] : 0.f);
                }
                cv[u] = q;
                av[u] = loadA(pzz, N, k + 16 * u + kq, k_hi);
#pragma unroll
                for (int s_ = 0; s_ < 4; ++s_) bv[u][s_] = loadB(z, k + 16 * u + kq + s_, k_hi);
            }
            __syncthreads();  // the previous round's readers are done with the tile
#pragma unroll
            for (int u = 0; u < 4; ++u) *reinterpret_cast<float4*>(&tw[(16 * u + tr) * SD_TLD + tc]) = cv[u];
            __syncthreads();
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float* tcol = tw + (16 * u + kq) * SD_TLD + (lane & 15);  // pi_zz[k + 16 u + kq + s][row]
                const float a0 = -0.5f * (av[u].x + tcol[0]), a1 = -0.5f * (av[u].y + tcol[SD_TLD]);
                const float a2 = -0.5f * (av[u].z + tcol[2 * SD_TLD]), a3 = -0.5f * (av[u].w + tcol[3 * SD_TLD]);
                rs += (a0 + a1) + (a2 + a3);
                acc = mfma16(a0, bv[u][0], acc);
                acc = mfma16(a1, bv[u][1], acc);
                acc = mfma16(a2, bv[u][2], acc);
                acc = mfma16(a3, bv[u][3], acc);
            }
        }
    }
    rs += __shfl_xor(rs, 16, 64);
    rs += __shfl_xor(rs, 32, 64);  // every lane: this wave's share of the row sum of row (lane & 15)
    if (w > 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) part[w - 1][r][lane] = acc[r];
        part[w - 1][4][lane] = rs;
    }
    __syncthreads();
    if (w != 0) return;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] += part[q][r][lane];
        rs += part[q][4][lane];
    }
    float gs = 0.f;  // sum of the upstream gradients of the loss replicas: lanes take every 64th, fixed shuffle tree
    for (int q = lane; q < ng; q += 64) gs += g[q];
    gs = wave_sum(gs);
    const float two_g = 2.f * scale * gs;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int li = (lane >> 4) * 4 + r;
        const float rsi = __shfl(rs, li, 64);
        const int i = i0 + li;
        if (i < N && col_ok) {
            const size_t e = (size_t)i * D + col;
            const float v = two_g * (rsi * z[e] - acc[r]);
            gz[e] = gadd ? gadd[e] + v : v;
        }
    }
}

extern "C" int otvae_sinkhorn_div_grad(int dtype, const void* z, const void* y, const void* pi_zy, const void* pi_zz, const void* g, int ng,
                                       double scale, const void* gadd, int N, int M, int D, void* gz, void* stream) {
    OTVAE_REQUIRE(z && y && pi_zy && pi_zz && g && gz && ng > 0 && N > 0 && M > 0 && D > 0, "otvae_sinkhorn_div_grad: bad argument");
    OTVAE_REQUIRE(dtype == 0 || dtype == 1, "otvae_sinkhorn_div_grad: dtype must be 0 or 1");
    OTVAE_REQUIRE(dtype == 1 || ((uintptr_t)pi_zy % 16 == 0 && (uintptr_t)pi_zz % 16 == 0),
                  "otvae_sinkhorn_div_grad: fp32 plans must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (dtype == 0)
        sd_grad_mfma_kernel<<<dim3(cdiv(D, 16), cdiv(N, 16)), 256, 0, st>>>((const float*)z, (const float*)y, (const float*)pi_zy,
                                                                            (const float*)pi_zz, (const float*)g, ng, (float)scale,
                                                                            (const float*)gadd, N, M, D, (float*)gz);
    else
        sd_grad_kernel<double><<<dim3(cdiv(D, 32), cdiv(N, 32)), 256, 0, st>>>((const double*)z, (const double*)y, (const double*)pi_zy,
                                                                               (const double*)pi_zz, (const double*)g, ng, scale,
                                                                               (const double*)gadd, N, M, D, (double*)gz);
    OTVAE_CHECK_LAUNCH("otvae_sinkhorn_div_grad");
    return OTVAE_OK;
}
