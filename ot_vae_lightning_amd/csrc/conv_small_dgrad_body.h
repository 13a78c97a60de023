// The statements of the direct data-gradient kernel (conv_small.hip), included TWICE: into conv_small_dgrad_kernel, where SMALL_VB /
// SMALL_NB are blockIdx.x / gridDim.x, and into conv_small_dgrad_body, the device function the two-job kernel calls with a job-local
// block index and block count.  One text, but the one-job kernel is compiled as kernel code and not as an inlined call: as an inlined
// function several instantiations of the RGB layers lost their registers (16 -> 3 3x3 up-2: 223 -> 256 + 18 AGPR, 2 -> 1 waves per
// SIMD; profiles/r06_pair_launch_ab.txt).  In scope: template arguments CS, CN, KSU; g, gy, wD, x, scale, shift, relu, mean, invstd,
// gv, partial, CsPad; the LDS arrays w_s[SMALL_MAXW] (wD[t][co][c]) and red[4][2][SMALL_MAXC].  No include guard, on purpose.
    constexpr int CSM = CS ? CS : SMALL_MAXC, CNM = CN ? CN : SMALL_MAXC;
    const int Cs = CS ? CS : g.Cs, Cn = CN ? CN : g.Cn;
    const int T = g.KH * g.KW;
    for (int i = threadIdx.x; i < T * Cs * Cn; i += 256) w_s[i] = wD[i];
    __syncthreads();
    float sc[CSM], sh[CSM], mu[CSM], is[CSM];
#pragma unroll
    for (int c = 0; c < CSM; ++c) {
        const bool in = CS || c < Cs;
        sc[c] = (scale && in) ? scale[c] : 1.f;
        sh[c] = (scale && in) ? shift[c] : 0.f;
        mu[c] = (mean && in) ? mean[c] : 0.f;
        is[c] = (mean && in) ? invstd[c] : 0.f;
    }
    const unsigned P = (unsigned)g.N * g.Hs * g.Ws;
    const float inv_ws = 1.0f / (float)g.Ws, inv_hs = 1.0f / (float)g.Hs;
    const bool small = P < (1u << 22);
    const int nchild = g.up * g.up;
    const int smask = g.stride - 1, sshift = g.stride - 1;
    double s1[CSM], s2[CSM];
#pragma unroll
    for (int c = 0; c < CSM; ++c) s1[c] = s2[c] = 0.0;
    for (unsigned p = SMALL_VB * 256 + threadIdx.x; p < P; p += SMALL_NB * 256) {
        const unsigned t0 = sdiv(p, g.Ws, inv_ws, small);
        const int sx = p - t0 * g.Ws;
        const int n = sdiv(t0, g.Hs, inv_hs, small);
        const int sy = t0 - (unsigned)n * g.Hs;
        float acc[CSM];
#pragma unroll
        for (int c = 0; c < CSM; ++c) acc[c] = 0.f;
        if constexpr (KSU > 0 && CS > 0 && CN > 0) {
            constexpr int KS = KSU >> 4, STRIDE = (KSU >> 2) & 3, UP = KSU & 3;
            constexpr int NT1 = (KS + STRIDE - 1) / STRIDE;  // taps of one parity class per dimension
            constexpr int NL = UP * UP * NT1 * NT1;
            constexpr int GS = (NL * CN <= 32) ? NL : NT1 * NT1;  // everything at once, or one child at a time
#pragma unroll 1  // a real loop over the children: unrolled, the address arithmetic of all NL taps is live at once
            for (int l0 = 0; l0 < NL; l0 += GS) {
                SMALL_REREAD_LDS();
                float gg[GS][CN];
                int tap[GS];  // kh * KS + kw, or -1 when the tap does not reach an output position
#pragma unroll
                for (int i = 0; i < GS; ++i) {
                    const int l = l0 + i;
                    const int ch = l / (NT1 * NT1), a = (l / NT1) % NT1, b = l % NT1;
                    const int iy = sy * UP + ch / UP, ix = sx * UP + ch % UP;
                    const int kh = ((iy + g.pad) & (STRIDE - 1)) + a * STRIDE, kw = ((ix + g.pad) & (STRIDE - 1)) + b * STRIDE;
                    const int ty = iy + g.pad - kh, tx = ix + g.pad - kw;
                    const int oy = ty >> (STRIDE - 1), ox = tx >> (STRIDE - 1);
                    const bool ok = kh < KS && kw < KS && ty >= 0 && tx >= 0 && oy < g.Ho && ox < g.Wo;
                    tap[i] = ok ? kh * KS + kw : -1;
                    const int cy = min(max(oy, 0), g.Ho - 1), cx = min(max(ox, 0), g.Wo - 1);
                    load_chan<CN>(gy + ((size_t)((unsigned)n * g.Ho + cy) * g.Wo + cx) * CN, gg[i], CN);
                }
#pragma unroll
                for (int i = 0; i < GS; ++i) {
                    const float* wp = w_s + max(tap[i], 0) * CN * CS;
#pragma unroll
                    for (int co = 0; co < CN; ++co) {
                        const float gval = __int_as_float(__float_as_int(gg[i][co]) & ~(tap[i] >> 31));
#pragma unroll
                        for (int c = 0; c < CS; ++c) acc[c] = fmaf(gval, wp[co * CS + c], acc[c]);
                    }
                }
            }
        } else
        for (int ch = 0; ch < nchild; ++ch) {
            const int iy = sy * g.up + (ch >> 1), ix = sx * g.up + (ch & 1);
            // stride 2: only the taps of this position's parity class contribute; start there and step by the stride
            for (int kh = (iy + g.pad) & smask; kh < g.KH; kh += g.stride) {
                const int ty = iy + g.pad - kh;
                if (ty < 0) break;  // kh only grows
                const int oy = ty >> sshift;
                if (oy >= g.Ho) continue;
                for (int kw = (ix + g.pad) & smask; kw < g.KW; kw += g.stride) {
                    const int tx = ix + g.pad - kw;
                    if (tx < 0) break;
                    const int ox = tx >> sshift;
                    if (ox >= g.Wo) continue;
                    float gg[CNM];
                    load_chan<CN>(gy + ((size_t)((unsigned)n * g.Ho + oy) * g.Wo + ox) * Cn, gg, Cn);
                    const float* wp = w_s + (kh * g.KW + kw) * Cn * Cs;
#pragma unroll
                    for (int co = 0; co < CNM; ++co) {
                        if (CN || co < Cn) {
#pragma unroll
                            for (int c = 0; c < CSM; ++c)
                                if (CS || c < Cs) acc[c] = fmaf(gg[co], wp[co * Cs + c], acc[c]);
                        }
                    }
                }
            }
        }
        const size_t o = (size_t)p * Cs;
        float xv[CSM];
        if (relu || mean) load_chan<CS>(x + o, xv, Cs);
#pragma unroll
        for (int c = 0; c < CSM; ++c) {
            if (CS || c < Cs) {
                float val = acc[c];
                if (relu) {
                    const float v = scale ? fmaf(xv[c], sc[c], sh[c]) : xv[c];
                    val = v > 0.f ? val : 0.f;
                }
                acc[c] = val;
                if (mean) {
                    s1[c] += (double)val;
                    s2[c] += (double)val * (double)((xv[c] - mu[c]) * is[c]);
                }
            }
        }
        store_chan<CS>(gv + o, acc, Cs);
    }
    if (mean) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
        for (int c = 0; c < CSM; ++c) {
            const double a = wave_sum(s1[c]), b = wave_sum(s2[c]);
            if (lane == 0) {
                red[wave][0][c] = a;
                red[wave][1][c] = b;
            }
        }
        __syncthreads();
        if (threadIdx.x < 2 * SMALL_MAXC) {
            const int which = threadIdx.x / SMALL_MAXC, c = threadIdx.x % SMALL_MAXC;
            if (c < Cs) {
                const double t = (red[0][which][c] + red[1][which][c]) + (red[2][which][c] + red[3][which][c]);
                bn_stat_out(partial, which, CsPad, c, SMALL_NB, SMALL_VB, t);
            }
        }
    }
