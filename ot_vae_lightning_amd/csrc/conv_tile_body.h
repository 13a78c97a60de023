// The statements of the image-tile kernel (conv_tile.hip), included TWICE: into conv_tile_kernel, where TILE_BX / TILE_BY / TILE_BZ and
// TILE_GX / TILE_GZ are blockIdx and gridDim, and into conv_tile_body, the device function the two-job kernel calls with a job-local
// block index.  One text, but the one-job kernel is compiled as kernel code and not as an inlined call, so that it keeps the registers
// it had (as an inlined function some instantiations moved: profiles/r06_pair_launch_ab.txt).  In scope: template arguments MODE, NT,
// RBW; pl, S, scale, shift, relu, Wg, bias, res, y, xin, mean, invstd, gv, partial, fold; tsm (the dynamic LDS) and bn_tab (2 x 256
// floats of LDS).  No include guard, on purpose.
    constexpr int BN = 16 * NT;
    // forward: the BatchNorm affine of the input in LDS (CK <= 256 here) -- folded from the statistic slots by every block, or copied
    // from the arrays a finalize launch left (common.h: bn_tab_fill)
    const float* sc_p = nullptr;
    const float* sh_p = nullptr;
    if constexpr (MODE == 0) {
        if (scale != nullptr || fold.slots != nullptr) {
            bn_tab_fill(fold, scale, shift, pl.CK, bn_tab[0], bn_tab[1], (TILE_BX | TILE_BY | TILE_BZ) == 0);
            sc_p = bn_tab[0];
            sh_p = bn_tab[1];
        }
    }
    float* V = tsm;                                   // [IPB][Hv][Wv][CKp]
    float* Wl = tsm + pl.vfloats;                     // [tpc*CK][BN]
    double* red = reinterpret_cast<double*>(Wl + TILE_WMAX);  // [4 waves][2][BN]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int cls = TILE_BZ;
    const TileTaps& tp = pl.taps[cls];
    const int CK = pl.CK, CKp = pl.CKp, NC = pl.NC;
    const int n0 = TILE_BY * BN;
    const int img0 = TILE_BX * pl.IPB;
    const int nimg = min(pl.IPB, pl.N - img0);

    // ---- stage the virtual grid of this block's images (zeros in the padding ring and past the last image)
    {
        const int ck4 = CK >> 2;
        const float inv_ck4 = 1.0f / (float)ck4, inv_wv = 1.0f / (float)pl.Wv, inv_hv = 1.0f / (float)pl.Hv;
        const int total = pl.IPB * pl.Hv * pl.Wv * ck4;
        for (int e0 = tid; e0 < total; e0 += 256 * 4) {
            float4 v[4];
            int dst[4], cc[4];
            bool ok[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int e = e0 + 256 * u;
                const int pix = tdiv(e, inv_ck4);
                const int c4 = e - pix * ck4;
                const int t1 = tdiv(pix, inv_wv);
                const int vx = pix - t1 * pl.Wv;
                const int img = tdiv(t1, inv_hv);
                const int vy = t1 - img * pl.Hv;
                const int uy = vy - pl.voffy, ux = vx - pl.voffx;
                ok[u] = e < total && img < nimg && (unsigned)uy < (unsigned)pl.limH && (unsigned)ux < (unsigned)pl.limW;
                dst[u] = e < total ? pix * CKp + c4 * 4 : -1;
                cc[u] = c4 * 4;
                const size_t off = ok[u] ? ((size_t)((unsigned)(img0 + img) * pl.srcH + (uy >> pl.ush)) * pl.srcW + (ux >> pl.ush)) * CK + c4 * 4 : 0;
                v[u] = *reinterpret_cast<const float4*>(S + off);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (dst[u] < 0) continue;
                float4 a = v[u];
                if (MODE == 0) {
                    if (sc_p != nullptr) {
                        const float4 sc = *reinterpret_cast<const float4*>(sc_p + cc[u]);
                        const float4 sh = *reinterpret_cast<const float4*>(sh_p + cc[u]);
                        a.x = fmaf(a.x, sc.x, sh.x);
                        a.y = fmaf(a.y, sc.y, sh.y);
                        a.z = fmaf(a.z, sc.z, sh.z);
                        a.w = fmaf(a.w, sc.w, sh.w);
                    }
                    if (relu) {
                        a.x = fmaxf(a.x, 0.f);
                        a.y = fmaxf(a.y, 0.f);
                        a.z = fmaxf(a.z, 0.f);
                        a.w = fmaxf(a.w, 0.f);
                    }
                }
                if (!ok[u]) a = make_float4(0.f, 0.f, 0.f, 0.f);  // padding is zero AFTER the activation
                *reinterpret_cast<float4*>(V + dst[u]) = a;
            }
        }
    }

    // ---- this wave's row blocks: lane (r16) <-> one output position of each
    const int rows_blk = pl.IPB * pl.rowsPI;
    // integer divisions by launch constants go through one float multiply (exact: tdiv), not the ~25-instruction
    // udiv expansion; they sit in per-row-block code that would otherwise out-weigh the MFMAs of a small layer
    const float inv_rpi = 1.0f / (float)pl.rowsPI, inv_rw = 1.0f / (float)pl.rowsW;
    const float inv_ws = 1.0f / (float)imax_d(pl.rowsW >> 1, 1);
    int pixbase[RBW];  // float offset of the position's virtual-grid origin
    int rloc[RBW];     // row within the block, or -1
#pragma unroll
    for (int i = 0; i < RBW; ++i) {
        const int rb = wave + 4 * i;
        const int rl = rb * 16 + r16;
        int pb = 0;
        int ok = -1;
        if (rl < rows_blk) {
            const int img = tdiv(rl, inv_rpi);
            const int r = rl - img * pl.rowsPI;
            int ry, rx;
            if (pl.childmode) {
                const int parent = r >> 2, child = r & 3;
                const int ws = pl.rowsW >> 1;
                const int sy = tdiv(parent, inv_ws), sx = parent - sy * ws;
                ry = 2 * sy + (child >> 1);
                rx = 2 * sx + (child & 1);
            } else {
                ry = tdiv(r, inv_rw);
                rx = r - ry * pl.rowsW;
            }
            pb = ((img * pl.Hv + ry * pl.rstride) * pl.Wv + rx * pl.rstride) * CKp;
            if (img < nimg) ok = rl;
        }
        pixbase[i] = pb + kq;
        rloc[i] = ok;
    }

    f32x4 acc[RBW][NT];
#pragma unroll
    for (int i = 0; i < RBW; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // ---- weight chunks: groups of `tpc` taps x all CK channels, [k][BN] in LDS; next chunk prefetched into registers
    const int tpc = pl.tpc;
    const int nchunk = (tp.n + tpc - 1) / tpc;
    constexpr int NWV = TILE_WMAX / 4 / 256;  // float4 slots per thread per chunk
    float4 wreg[NWV];
    const float inv_ck = 1.0f / (float)CK;
    auto wload = [&](int ch) {
        const int t0 = ch * tpc;
        const int rows = min(tpc, tp.n - t0) * CK;
#pragma unroll
        for (int u = 0; u < NWV; ++u) {
            const int e = tid + 256 * u;
            const int row = e / (BN / 4), c4 = e - row * (BN / 4);
            const bool ok = row < rows && n0 + c4 * 4 < NC;
            const int tl = ok ? tdiv(row, inv_ck) : 0;
            const int c = row - tl * CK;
            const size_t off = ok ? ((size_t)tp.wrow[t0 + tl] * CK + c) * NC + n0 + c4 * 4 : 0;
            const float4 v = *reinterpret_cast<const float4*>(Wg + off);
            wreg[u] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto wstore = [&]() {
#pragma unroll
        for (int u = 0; u < NWV; ++u) {
            const int e = tid + 256 * u;
            if (e < tpc * CK * (BN / 4)) *reinterpret_cast<float4*>(Wl + e * 4) = wreg[u];
        }
    };
    wload(0);
    wstore();
    __syncthreads();
    for (int ch = 0; ch < nchunk; ++ch) {
        if (ch + 1 < nchunk) wload(ch + 1);
        const int t0 = ch * tpc;
        const int tcount = min(tpc, tp.n - t0);
        for (int tl = 0; tl < tcount; ++tl) {
            const int toff = tp.off[t0 + tl];
            const float* wr = Wl + (size_t)(tl * CK + kq) * BN + r16;
            // KS k-steps (4 channels each) per trip: all LDS reads of the trip are issued before its MFMAs, so one
            // lgkmcnt wait covers KS*(NT+RBW) reads instead of one wait per MFMA group (the loop is latency-bound at
            // one wave per SIMD otherwise).  Accumulation order over k is unchanged.
            auto ksteps = [&](int c0, auto ks_tag) {
                constexpr int KS = decltype(ks_tag)::value;
                float w[KS][NT], a[KS][RBW];
#pragma unroll
                for (int s = 0; s < KS; ++s) {
#pragma unroll
                    for (int j = 0; j < NT; ++j) w[s][j] = wr[(c0 + 4 * s) * BN + j * 16];
#pragma unroll
                    for (int i = 0; i < RBW; ++i) a[s][i] = V[pixbase[i] + toff + c0 + 4 * s];
                }
#pragma unroll
                for (int s = 0; s < KS; ++s)
#pragma unroll
                    for (int i = 0; i < RBW; ++i)
#pragma unroll
                        for (int j = 0; j < NT; ++j) acc[i][j] = mfma16(w[s][j], a[s][i], acc[i][j]);
            };
            int c0 = 0;
            for (; c0 + 16 <= CK; c0 += 16) ksteps(c0, std::integral_constant<int, 4>{});
            for (; c0 + 8 <= CK; c0 += 8) ksteps(c0, std::integral_constant<int, 2>{});
            for (; c0 < CK; c0 += 4) ksteps(c0, std::integral_constant<int, 1>{});
        }
        if (ch + 1 < nchunk) {
            __syncthreads();
            wstore();
            __syncthreads();
        }
    }

    // ---- epilogue: lane = position r16 of the row block, channels n0 + 16 j + 4 kq .. + 3
    double s1[NT][4], s2[NT][4];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) s1[j][r] = s2[j][r] = 0.0;
    const bool want_sums = (MODE == 0) ? (partial != nullptr) : (mean != nullptr);

#pragma unroll
    for (int i = 0; i < RBW; ++i) {
        const int rl = rloc[i];
        // position decode (again; cheap, once per row block)
        int img = 0, r = 0;
        if (rl >= 0) {
            img = tdiv(rl, inv_rpi);
            r = rl - img * pl.rowsPI;
        }
        const unsigned gimg = img0 + img;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int ch = n0 + j * 16 + kq * 4;
            const bool chok = ch < NC;
            float4 val = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
            if (MODE == 0) {
                if (rl >= 0 && chok) {
                    const size_t o = ((size_t)gimg * pl.rowsPI + r) * NC + ch;
                    if (bias) {
                        const float4 b = *reinterpret_cast<const float4*>(bias + ch);
                        val.x += b.x, val.y += b.y, val.z += b.z, val.w += b.w;
                    }
                    if (res) {
                        const float4 q = *reinterpret_cast<const float4*>(res + o);
                        val.x += q.x, val.y += q.y, val.z += q.z, val.w += q.w;
                    }
                    *reinterpret_cast<float4*>(y + o) = val;
                    if (partial) {
                        s1[j][0] += (double)val.x, s2[j][0] += (double)val.x * (double)val.x;
                        s1[j][1] += (double)val.y, s2[j][1] += (double)val.y * (double)val.y;
                        s1[j][2] += (double)val.z, s2[j][2] += (double)val.z * (double)val.z;
                        s1[j][3] += (double)val.w, s2[j][3] += (double)val.w * (double)val.w;
                    }
                }
            } else {
                bool writer = rl >= 0 && chok;
                size_t o = 0;
                if (pl.childmode) {
                    // the 4 children of one source pixel are 4 consecutive lanes: fixed-order quad sum
                    float4 t;
                    t.x = val.x + __shfl_xor(val.x, 1, 64), t.y = val.y + __shfl_xor(val.y, 1, 64);
                    t.z = val.z + __shfl_xor(val.z, 1, 64), t.w = val.w + __shfl_xor(val.w, 1, 64);
                    val.x = t.x + __shfl_xor(t.x, 2, 64), val.y = t.y + __shfl_xor(t.y, 2, 64);
                    val.z = t.z + __shfl_xor(t.z, 2, 64), val.w = t.w + __shfl_xor(t.w, 2, 64);
                    writer = writer && ((r16 & 3) == 0);
                    o = ((size_t)gimg * (pl.rowsPI >> 2) + (r >> 2)) * NC + ch;
                } else if (pl.s2) {
                    const int ry = tdiv(r, inv_rw), rx = r - ry * pl.rowsW;
                    const int py = cls >> 1, px = cls & 1;
                    o = (((size_t)gimg * (2 * pl.rowsH) + 2 * ry + py) * (2 * pl.rowsW) + 2 * rx + px) * NC + ch;
                } else {
                    o = ((size_t)gimg * pl.rowsPI + r) * NC + ch;
                }
                if (writer) {
                    float4 xv = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (relu || mean) xv = *reinterpret_cast<const float4*>(xin + o);
                    if (relu) {
                        float4 a = xv;
                        if (scale) {
                            const float4 sc = *reinterpret_cast<const float4*>(scale + ch);
                            const float4 sh = *reinterpret_cast<const float4*>(shift + ch);
                            a.x = fmaf(a.x, sc.x, sh.x), a.y = fmaf(a.y, sc.y, sh.y);
                            a.z = fmaf(a.z, sc.z, sh.z), a.w = fmaf(a.w, sc.w, sh.w);
                        }
                        val.x = a.x > 0.f ? val.x : 0.f;
                        val.y = a.y > 0.f ? val.y : 0.f;
                        val.z = a.z > 0.f ? val.z : 0.f;
                        val.w = a.w > 0.f ? val.w : 0.f;
                    }
                    *reinterpret_cast<float4*>(gv + o) = val;
                    if (mean) {
                        const float4 mu = *reinterpret_cast<const float4*>(mean + ch);
                        const float4 is = *reinterpret_cast<const float4*>(invstd + ch);
                        s1[j][0] += (double)val.x, s2[j][0] += (double)val.x * (double)((xv.x - mu.x) * is.x);
                        s1[j][1] += (double)val.y, s2[j][1] += (double)val.y * (double)((xv.y - mu.y) * is.y);
                        s1[j][2] += (double)val.z, s2[j][2] += (double)val.z * (double)((xv.z - mu.z) * is.z);
                        s1[j][3] += (double)val.w, s2[j][3] += (double)val.w * (double)((xv.w - mu.w) * is.w);
                    }
                }
            }
        }
    }

    if (want_sums) {
        // fixed order: the 16 position lanes of each kq group (xor tree), then the 4 waves through LDS
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double a = s1[j][r], b = s2[j][r];
                a += __shfl_xor(a, 1, 64), b += __shfl_xor(b, 1, 64);
                a += __shfl_xor(a, 2, 64), b += __shfl_xor(b, 2, 64);
                a += __shfl_xor(a, 4, 64), b += __shfl_xor(b, 4, 64);
                a += __shfl_xor(a, 8, 64), b += __shfl_xor(b, 8, 64);
                if (r16 == 0) {
                    red[(wave * 2 + 0) * BN + j * 16 + kq * 4 + r] = a;
                    red[(wave * 2 + 1) * BN + j * 16 + kq * 4 + r] = b;
                }
            }
        __syncthreads();
        if (tid < 2 * BN) {
            const int which = tid / BN, cc = tid % BN;
            const double t = (red[(0 * 2 + which) * BN + cc] + red[(1 * 2 + which) * BN + cc]) +
                             (red[(2 * 2 + which) * BN + cc] + red[(3 * 2 + which) * BN + cc]);
            // the job-local block index: partials and statistic slots land where the one-job launch puts them
            const unsigned p = (unsigned)TILE_BZ * TILE_GX + TILE_BX;
            const unsigned Ptot = (unsigned)TILE_GX * TILE_GZ;
            if (n0 + cc < pl.cpad) bn_stat_out(partial, which, pl.cpad, n0 + cc, Ptot, p, t);  // [2][cpad][P], or the statistic slots
        }
    }
