// The statements of the direct forward kernel (conv_small.hip), included TWICE: into conv_small_fwd_kernel, where SMALL_VB / SMALL_NB
// are blockIdx.x / gridDim.x, and into conv_small_fwd_body, the device function the two-job kernel calls with a job-local block index
// and block count (see conv_small_dgrad_body.h for why).  In scope: template arguments CS, CN, KS; g, x, scale, shift, relu, wT, bias,
// res, y, partial, CnPad, fold; the LDS arrays w_s[SMALL_MAXW] ([tap][c][CNM], row padded to CNM when CN is generic),
// redf[4][2][SMALL_MAXC], sc_s / sh_s / b_s[SMALL_MAXC].  No include guard, on purpose.
    constexpr int CSM = CS ? CS : SMALL_MAXC, CNM = CN ? CN : SMALL_MAXC;
    const int Cs = CS ? CS : g.Cs, Cn = CN ? CN : g.Cn;
    const int T = g.KH * g.KW;
    for (int i = threadIdx.x; i < T * Cs * Cn; i += 256) w_s[i] = wT[i];
    if (threadIdx.x < SMALL_MAXC) {
        const int c = threadIdx.x;
        sc_s[c] = (scale && c < Cs) ? scale[c] : 1.f;
        sh_s[c] = (scale && c < Cs) ? shift[c] : 0.f;
        b_s[c] = (bias && c < Cn) ? bias[c] : 0.f;
    }
    __syncthreads();
    if (fold.slots) bn_fold_prologue(fold, Cs, sc_s, sh_s, SMALL_VB == 0);  // the BatchNorm of x folded in (common.h); ends with a barrier
    const bool affine = scale != nullptr || fold.slots != nullptr;
    float sc[CSM], sh[CSM];
#pragma unroll
    for (int c = 0; c < CSM; ++c) {
        sc[c] = sc_s[c];
        sh[c] = sh_s[c];
    }
    const int Hu = g.Hs * g.up, Wu = g.Ws * g.up, ush = g.up - 1;
    const unsigned M = (unsigned)g.N * g.Ho * g.Wo;
    const float inv_wo = 1.0f / (float)g.Wo, inv_ho = 1.0f / (float)g.Ho;
    const bool small = M < (1u << 22);
    double s1[CNM], s2[CNM];
#pragma unroll
    for (int j = 0; j < CNM; ++j) s1[j] = s2[j] = 0.0;
    for (unsigned m = SMALL_VB * 256 + threadIdx.x; m < M; m += SMALL_NB * 256) {
        const unsigned t0 = sdiv(m, g.Wo, inv_wo, small);
        const int ox = m - t0 * g.Wo;
        const int n = sdiv(t0, g.Ho, inv_ho, small);
        const int oy = t0 - (unsigned)n * g.Ho;
        float acc[CNM];
#pragma unroll
        for (int j = 0; j < CNM; ++j) acc[j] = b_s[j];
        if constexpr (KS > 0 && CS > 0 && CN > 0) {
            // taps in groups whose loads (<= 32 registers) are in flight together; the clobber keeps a group's loads from
            // drifting above the previous group's arithmetic (and the weights in LDS, see SMALL_REREAD_LDS)
            constexpr int GS = (KS * KS * CS <= 32) ? KS * KS : KS;  // all taps at once, or one kernel row at a time
#pragma unroll
            for (int t0g = 0; t0g < KS * KS; t0g += GS) {
                SMALL_REREAD_LDS();
                float xv[GS][CS];
                int ok[GS];  // all-ones / zero bit mask: applied with an AND (a select here becomes a branch per channel)
#pragma unroll
                for (int i = 0; i < GS; ++i) {
                    const int t = t0g + i;
                    const int iy = oy * g.stride + t / KS - g.pad, ix = ox * g.stride + t % KS - g.pad;
                    ok[i] = ((unsigned)iy < (unsigned)Hu && (unsigned)ix < (unsigned)Wu) ? -1 : 0;
                    const int cy = min(max(iy, 0), Hu - 1) >> ush, cx = min(max(ix, 0), Wu - 1) >> ush;
                    load_chan<CS>(x + ((size_t)((unsigned)n * g.Hs + cy) * g.Ws + cx) * CS, xv[i], CS);
                }
#pragma unroll
                for (int i = 0; i < GS; ++i) {
                    const float* wp = w_s + (t0g + i) * CS * CN;
#pragma unroll
                    for (int c = 0; c < CS; ++c) {
                        const float a = __int_as_float(__float_as_int(act1(xv[i][c], sc[c], sh[c], affine, relu)) & ok[i]);
#pragma unroll
                        for (int j = 0; j < CN; ++j) acc[j] = fmaf(a, wp[c * CN + j], acc[j]);
                    }
                }
            }
        } else {
            for (int kh = 0; kh < g.KH; ++kh) {
                const int iy = oy * g.stride + kh - g.pad;
                if ((unsigned)iy >= (unsigned)Hu) continue;
                for (int kw = 0; kw < g.KW; ++kw) {
                    const int ix = ox * g.stride + kw - g.pad;
                    if ((unsigned)ix >= (unsigned)Wu) continue;
                    float xv[CSM];
                    load_chan<CS>(x + ((size_t)((unsigned)n * g.Hs + (iy >> ush)) * g.Ws + (ix >> ush)) * Cs, xv, Cs);
                    const float* wp = w_s + (kh * g.KW + kw) * Cs * Cn;
#pragma unroll
                    for (int c = 0; c < CSM; ++c) {
                        if (CS || c < Cs) {
                            const float a = act1(xv[c], sc[c], sh[c], affine, relu);
#pragma unroll
                            for (int j = 0; j < CNM; ++j)
                                if (CN || j < Cn) acc[j] = fmaf(a, wp[c * Cn + j], acc[j]);
                        }
                    }
                }
            }
        }
        if (res) {
            float rv[CNM];
            load_chan<CN>(res + (size_t)m * Cn, rv, Cn);
#pragma unroll
            for (int j = 0; j < CNM; ++j) acc[j] += rv[j];
        }
        store_chan<CN>(y + (size_t)m * Cn, acc, Cn);
        if (partial) {
#pragma unroll
            for (int j = 0; j < CNM; ++j) {
                s1[j] += (double)acc[j];
                s2[j] += (double)acc[j] * (double)acc[j];
            }
        }
    }
    if (partial) {  // per-channel sums of the output = the next layer's BatchNorm statistics
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
        for (int j = 0; j < CNM; ++j) {
            const double a = wave_sum(s1[j]), b = wave_sum(s2[j]);
            if (lane == 0) {
                redf[wave][0][j] = a;
                redf[wave][1][j] = b;
            }
        }
        __syncthreads();
        if (threadIdx.x < 2 * SMALL_MAXC) {
            const int which = threadIdx.x / SMALL_MAXC, c = threadIdx.x % SMALL_MAXC;
            if (c < Cn)
                bn_stat_out(partial, which, CnPad, c, SMALL_NB, SMALL_VB,
                            (redf[0][which][c] + redf[1][which][c]) + (redf[2][which][c] + redf[3][which][c]));
        }
    }
