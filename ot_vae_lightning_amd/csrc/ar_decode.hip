// Incremental (key/value-cached) decoding of the causal AutoRegressive transformer (networks/vit.py): one NEW token per batch row.
//
// otvae_ar_embed_step: out[b][:] = LayerNorm(vocab[ids[b]][:] + positions[pos][:])   -- the step's input, one wave per row.
// otvae_ar_layer_step: one post-norm nn.TransformerEncoderLayer (ReLU, eval mode, causal) for the token at position `pos` of every row,
// as ONE launch:
//     qkv = x W_in + b_in;  kcache[b][h][pos][:] = k;  vcache[b][h][pos][:] = v
//     a   = softmax(q . kcache[b][h][0..pos][:]^T / sqrt(C)) . vcache[b][h][0..pos][:]          (per head, a single query)
//     x1  = LayerNorm1(x + a W_out + b_out);   y = LayerNorm2(x1 + relu(x1 W_1 + b_1) W_2 + b_2)
//
// A workgroup (8 waves) owns ARD_ROWS = 16 batch rows = the M of v_mfma_f32_16x16x4_f32: the four weight matrices are read once per 16
// rows, straight from global memory as the MFMA's B operand (lane l reads W[k0 + l / 16][n0 + l % 16]: 64-byte runs), the A operand comes
// from LDS.  LDS holds xs [16][D + 4] (x, then the pre-norm sums, then x1, then the second pre-norm sums) and buf [16][3 D + 4] (q | k | v;
// the attention output of a head overwrites its q; afterwards the feed-forward's hidden activations in chunks of 3 D columns, linear2's
// [16][D] accumulators staying in registers across the chunks): 16 * (4 D + 8) * 4 bytes, 131,584 at D = 512 of the 160 KiB of a CU.  The
// + 4 padding puts the 16 rows x 4 k of an A-operand read on 64 different banks when D % 64 == 0.
//
// Attention: a wave takes one (row, head) pair at a time and streams over the cache in chunks of 64 positions: lane t of the chunk forms
// the score of position t (q from LDS, the key row from the cache; position `pos` itself from LDS: nothing this launch wrote to global
// memory is read back), the running maximum / sum are updated (online soft-max) and the weighted sum over the value rows is accumulated
// with the lanes on the head's columns (for C < 64 the 64 / C lane groups take different positions and are added at the end in a fixed
// order).  No score matrix, no atomics: the result is bit-reproducible.
//
// Envelope (OTVAE_EUNSUPPORTED outside): 16 <= D <= 512 with D % 16 == 0, head width C = D / H with C % 4 == 0, 1 <= F <= 4 D,
// Tmax <= ARD_MAX_T.  B is arbitrary (the last tile is partial), 0 <= pos < Tmax.
#include "common.h"

#define ARD_ROWS 16
#define ARD_WAVES 8
#define ARD_THREADS (ARD_WAVES * 64)
#define ARD_PAD 4
#define ARD_MAX_D 512
#define ARD_MAX_T 4096
#define ARD_NT 4   // 16-column tiles a wave has in flight in one pass over K

// acc[u] += A[16][K] . W[krow0 .. krow0 + K)[16 columns of tile t_u], t_u = tile0 + u * ARD_WAVES, the tile's first column col0 + 16 t_u.
// A: LDS, row stride lda.  W: global, [Ktot][N] row-major; rows >= Ktot, columns >= N and tiles >= ntiles contribute 0.
__device__ __forceinline__ void ard_gemm(const float* A, int lda, int K, const float* __restrict__ W, int N, int krow0, int Ktot, int col0,
                                         int tile0, int ntiles, f32x4 (&acc)[ARD_NT]) {
    const int lane = threadIdx.x & 63, r = lane & 15, kq = lane >> 4;
    int col[ARD_NT];
    bool ok[ARD_NT];
#pragma unroll
    for (int u = 0; u < ARD_NT; ++u) {
        const int t = tile0 + u * ARD_WAVES;
        col[u] = col0 + t * 16 + r;
        ok[u] = t < ntiles && col[u] < N;
    }
    const float* a = A + r * lda + kq;
    for (int k0 = 0; k0 < K; k0 += 16) {   // K % 16 == 0: four MFMA k-steps = 4 * ARD_NT weight loads in flight
        float av[4], bv[4][ARD_NT];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            av[s] = a[k0 + 4 * s];
            const int kr = krow0 + k0 + 4 * s + kq;
            const bool kok = kr < Ktot;
            const float* __restrict__ w = W + (int64_t)kr * N;
#pragma unroll
            for (int u = 0; u < ARD_NT; ++u) bv[s][u] = (kok && ok[u]) ? w[col[u]] : 0.f;
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int u = 0; u < ARD_NT; ++u) acc[u] = mfma16(av[s], bv[s][u], acc[u]);
    }
}

// rows 2 * wave, 2 * wave + 1 of xs: biased-variance LayerNorm, written back in place (y == NULL) or to y[row0 + r][:] for rows < B
__device__ __forceinline__ void ard_layernorm(float* xs, int ldx, int D, const float* __restrict__ g, const float* __restrict__ be, float eps,
                                              float* __restrict__ y, int row0, int B) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = wave * (ARD_ROWS / ARD_WAVES); r < (wave + 1) * (ARD_ROWS / ARD_WAVES); ++r) {
        float v[ARD_MAX_D / 64];
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < ARD_MAX_D / 64; ++j) {
            const int c = lane + 64 * j;
            v[j] = c < D ? xs[r * ldx + c] : 0.f;
            s += v[j];
        }
        const float mean = wave_sum(s) / (float)D;
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < ARD_MAX_D / 64; ++j) {
            const int c = lane + 64 * j;
            const float d = c < D ? v[j] - mean : 0.f;
            q += d * d;
        }
        const float rstd = 1.f / sqrtf(wave_sum(q) / (float)D + eps);
#pragma unroll
        for (int j = 0; j < ARD_MAX_D / 64; ++j) {
            const int c = lane + 64 * j;
            if (c < D) {
                const float o = (v[j] - mean) * rstd * g[c] + be[c];
                if (!y) xs[r * ldx + c] = o;
                else if (row0 + r < B) y[(int64_t)(row0 + r) * D + c] = o;
            }
        }
    }
}

__global__ __launch_bounds__(ARD_THREADS) void ar_layer_step_kernel(
    const float* __restrict__ x, int B, int D, int H, int F, int pos, int Tmax, const float* __restrict__ w_in, const float* __restrict__ b_in,
    const float* __restrict__ w_out, const float* __restrict__ b_out, const float* __restrict__ g1, const float* __restrict__ be1, float eps1,
    const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2,
    const float* __restrict__ g2, const float* __restrict__ be2, float eps2, float* __restrict__ kc, float* __restrict__ vc,
    float* __restrict__ y) {
    extern __shared__ __align__(16) float ard_sm[];
    const int ldx = D + ARD_PAD, ldb = 3 * D + ARD_PAD;
    float* xs = ard_sm;
    float* buf = ard_sm + ARD_ROWS * ldx;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int erow = (lane >> 4) * 4, ecol = lane & 15;   // element e of an accumulator: row erow + e, column ecol of its tile
    const int row0 = blockIdx.x * ARD_ROWS, C = D / H;

    for (int i = tid; i < ARD_ROWS * D; i += ARD_THREADS) {
        const int r = i / D, c = i - r * D;
        xs[r * ldx + c] = row0 + r < B ? x[(int64_t)(row0 + r) * D + c] : 0.f;
    }
    __syncthreads();

    // ---- q | k | v = x W_in + b_in -> buf
    {
        const int nt = 3 * D / 16;
        for (int t0 = wave; t0 < nt; t0 += ARD_WAVES * ARD_NT) {
            f32x4 acc[ARD_NT] = {};
            ard_gemm(xs, ldx, D, w_in, 3 * D, 0, D, 0, t0, nt, acc);
#pragma unroll
            for (int u = 0; u < ARD_NT; ++u) {
                const int t = t0 + u * ARD_WAVES;
                if (t < nt) {
                    const int col = t * 16 + ecol;
                    const float bias = b_in[col];
#pragma unroll
                    for (int e = 0; e < 4; ++e) buf[(erow + e) * ldb + col] = acc[u][e] + bias;
                }
            }
        }
    }
    __syncthreads();

    // ---- append this token's key / value rows to the caches
    for (int i = tid; i < ARD_ROWS * D; i += ARD_THREADS) {
        const int r = i / D, c = i - r * D;
        if (row0 + r < B) {
            const int h = c / C, cc = c - h * C;
            const int64_t at = (((int64_t)(row0 + r) * H + h) * Tmax + pos) * C + cc;
            kc[at] = buf[r * ldb + D + c];
            vc[at] = buf[r * ldb + 2 * D + c];
        }
    }

    // ---- single-query attention, one (row, head) pair per wave at a time; the output overwrites the pair's q
    {
        int lg = 6;                      // Cp = min(64, next power of two >= C) lanes span the head's columns
        while (lg > 2 && (1 << (lg - 1)) >= C) --lg;
        const int Cp = 1 << lg, TG = 64 >> lg;
        const int cl = lane & (Cp - 1), tg = lane >> lg;
        const float scale = 1.f / sqrtf((float)C);
        for (int p = wave; p < ARD_ROWS * H; p += ARD_WAVES) {
            const int r = p / H, h = p - r * H;
            if (row0 + r >= B) continue;   // wave-uniform
            float* q = buf + r * ldb + h * C;
            const float* kn = q + D;
            const float* vn = q + 2 * D;
            const int64_t base = ((int64_t)(row0 + r) * H + h) * Tmax * C;
            const float* __restrict__ kg = kc + base;
            const float* __restrict__ vg = vc + base;
            float m = -INFINITY, l = 0.f;
            float acc[ARD_MAX_D / 64] = {};
            for (int t0 = 0; t0 <= pos; t0 += 64) {
                const int t = t0 + lane;
                float s = -INFINITY;
                if (t < pos) {
                    const float* __restrict__ kr = kg + (int64_t)t * C;
                    float d = 0.f;
                    for (int c = 0; c < C; c += 4) {
                        const f32x4 kv = *reinterpret_cast<const f32x4*>(kr + c);
                        d += q[c] * kv.x + q[c + 1] * kv.y + q[c + 2] * kv.z + q[c + 3] * kv.w;
                    }
                    s = d * scale;
                } else if (t == pos) {
                    float d = 0.f;
                    for (int c = 0; c < C; c += 4) d += q[c] * kn[c] + q[c + 1] * kn[c + 1] + q[c + 2] * kn[c + 2] + q[c + 3] * kn[c + 3];
                    s = d * scale;
                }
                const float mn = fmaxf(m, wave_max(s));          // finite: the chunk holds at least one position <= pos
                const float corr = __expf(m - mn);               // 0 on the first chunk (m = -inf)
                const float pr = t <= pos ? __expf(s - mn) : 0.f;
                l = l * corr + wave_sum(pr);
                m = mn;
#pragma unroll
                for (int j = 0; j < ARD_MAX_D / 64; ++j) acc[j] *= corr;
                const int n = pos + 1 - t0 < 64 ? pos + 1 - t0 : 64;
                for (int i = 0; i * TG < n; ++i) {
                    const int tt = i * TG + tg;                  // < 64
                    const float pv = __shfl(pr, tt, 64);
                    if (tt < n) {
                        const int ta = t0 + tt;
#pragma unroll
                        for (int j = 0; j < ARD_MAX_D / 64; ++j) {
                            const int c = cl + 64 * j;
                            if (c < C) acc[j] += pv * (ta == pos ? vn[c] : vg[(int64_t)ta * C + c]);
                        }
                    }
                }
            }
            for (int o = Cp; o < 64; o <<= 1) acc[0] += __shfl_xor(acc[0], o, 64);   // the lane groups of a narrow head, fixed order
            const float inv = 1.f / l;
            if (tg == 0) {
#pragma unroll
                for (int j = 0; j < ARD_MAX_D / 64; ++j) {
                    const int c = cl + 64 * j;
                    if (c < C) q[c] = acc[j] * inv;
                }
            }
        }
    }
    __syncthreads();

    // ---- xs = x + a W_out + b_out, then LayerNorm1 in place
    {
        const int nt = D / 16;   // <= ARD_WAVES * ARD_NT
        f32x4 acc[ARD_NT] = {};
        ard_gemm(buf, ldb, D, w_out, D, 0, D, 0, wave, nt, acc);
#pragma unroll
        for (int u = 0; u < ARD_NT; ++u) {
            const int t = wave + u * ARD_WAVES;
            if (t < nt) {
                const int col = t * 16 + ecol;
                const float bias = b_out[col];
#pragma unroll
                for (int e = 0; e < 4; ++e) xs[(erow + e) * ldx + col] += acc[u][e] + bias;
            }
        }
    }
    __syncthreads();
    ard_layernorm(xs, ldx, D, g1, be1, eps1, nullptr, row0, B);
    __syncthreads();

    // ---- feed-forward: hidden columns in chunks of 3 D through buf, linear2's accumulators in registers across the chunks
    {
        const int Fp = (F + 15) & ~15, FC = 3 * D, nt2 = D / 16;
        f32x4 acc2[ARD_NT] = {};
        for (int f0 = 0; f0 < Fp; f0 += FC) {
            const int fc = Fp - f0 < FC ? Fp - f0 : FC, nt1 = fc / 16;
            for (int t0 = wave; t0 < nt1; t0 += ARD_WAVES * ARD_NT) {
                f32x4 acc[ARD_NT] = {};
                ard_gemm(xs, ldx, D, w1, F, 0, D, f0, t0, nt1, acc);
#pragma unroll
                for (int u = 0; u < ARD_NT; ++u) {
                    const int t = t0 + u * ARD_WAVES;
                    if (t < nt1) {
                        const int lc = t * 16 + ecol, col = f0 + lc;
                        const float bias = col < F ? b1[col] : 0.f;
#pragma unroll
                        for (int e = 0; e < 4; ++e) buf[(erow + e) * ldb + lc] = col < F ? fmaxf(acc[u][e] + bias, 0.f) : 0.f;
                    }
                }
            }
            __syncthreads();
            ard_gemm(buf, ldb, fc, w2, D, f0, F, 0, wave, nt2, acc2);
            __syncthreads();
        }
#pragma unroll
        for (int u = 0; u < ARD_NT; ++u) {
            const int t = wave + u * ARD_WAVES;
            if (t < nt2) {
                const int col = t * 16 + ecol;
                const float bias = b2[col];
#pragma unroll
                for (int e = 0; e < 4; ++e) xs[(erow + e) * ldx + col] += acc2[u][e] + bias;
            }
        }
    }
    __syncthreads();
    ard_layernorm(xs, ldx, D, g2, be2, eps2, y, row0, B);
}

extern "C" int otvae_ar_layer_step(const float* x, int B, int D, int H, int F, int pos, int Tmax, const float* w_in, const float* b_in,
                                   const float* w_out, const float* b_out, const float* ln1_g, const float* ln1_b, float eps1,
                                   const float* w1, const float* b1, const float* w2, const float* b2, const float* ln2_g,
                                   const float* ln2_b, float eps2, float* kcache, float* vcache, float* y, void* stream) {
    OTVAE_REQUIRE(x && w_in && b_in && w_out && b_out && ln1_g && ln1_b && w1 && b1 && w2 && b2 && ln2_g && ln2_b && kcache && vcache && y,
                  "otvae_ar_layer_step: null pointer");
    OTVAE_REQUIRE(B > 0 && D > 0 && H > 0 && F > 0 && Tmax > 0, "otvae_ar_layer_step: bad sizes (B = %d, D = %d, H = %d, F = %d, Tmax = %d)", B, D,
                  H, F, Tmax);
    OTVAE_REQUIRE(D % H == 0, "otvae_ar_layer_step: D = %d is not a multiple of H = %d", D, H);
    OTVAE_REQUIRE(pos >= 0 && pos < Tmax, "otvae_ar_layer_step: position %d outside a cache of %d", pos, Tmax);
    OTVAE_REQUIRE(eps1 > 0.f && eps2 > 0.f, "otvae_ar_layer_step: LayerNorm eps must be positive");
    OTVAE_REQUIRE(((((uintptr_t)kcache) | ((uintptr_t)vcache)) & 15) == 0, "otvae_ar_layer_step: the caches must be 16-byte aligned");
    const int C = D / H;
    if (D < 16 || D > ARD_MAX_D || D % 16 != 0 || C % 4 != 0 || F > 4 * D || Tmax > ARD_MAX_T) {
        otvae_set_error("otvae_ar_layer_step: D = %d, head width %d, F = %d, Tmax = %d is outside the envelope (16 <= D <= %d, D %% 16 == 0, "
                        "head width %% 4 == 0, F <= 4 D, Tmax <= %d)", D, C, F, Tmax, ARD_MAX_D, ARD_MAX_T);
        return OTVAE_EUNSUPPORTED;
    }
    const size_t lds = (size_t)ARD_ROWS * (4 * D + 2 * ARD_PAD) * sizeof(float);
    if (int rc = otvae_lds_grant<&ar_layer_step_kernel>("otvae_ar_layer_step", lds,
                                                        (size_t)ARD_ROWS * (4 * ARD_MAX_D + 2 * ARD_PAD) * sizeof(float)))
        return rc;
    ar_layer_step_kernel<<<cdiv(B, ARD_ROWS), ARD_THREADS, lds, (hipStream_t)stream>>>(x, B, D, H, F, pos, Tmax, w_in, b_in, w_out, b_out, ln1_g,
                                                                                        ln1_b, eps1, w1, b1, w2, b2, ln2_g, ln2_b, eps2, kcache,
                                                                                        vcache, y);
    OTVAE_CHECK_LAUNCH("otvae_ar_layer_step");
    return OTVAE_OK;
}

// ---- out[b][:] = LayerNorm(vocab[ids[b * ids_stride]][:] + positions[pos][:]); an id outside [0, V) yields a NaN row ------------------
__global__ __launch_bounds__(256) void ar_embed_step_kernel(const int64_t* __restrict__ ids, int64_t ids_stride, int pos, int B, int D, int V,
                                                            const float* __restrict__ vocab, const float* __restrict__ positions,
                                                            const float* __restrict__ g, const float* __restrict__ be, float eps,
                                                            float* __restrict__ out) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;   // whole waves; no barrier below
    const int64_t id = ids[b * ids_stride];
    const bool idok = id >= 0 && id < V;
    const float* __restrict__ pr = positions + (int64_t)pos * D;
    float s = 0.f;
    for (int c = lane; c < D; c += 64) s += idok ? vocab[id * D + c] + pr[c] : 0.f;
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
    for (int c = lane; c < D; c += 64) {
        const float d = idok ? vocab[id * D + c] + pr[c] - mean : 0.f;
        q += d * d;
    }
    const float rstd = 1.f / sqrtf(wave_sum(q) / (float)D + eps);
    for (int c = lane; c < D; c += 64)
        out[(int64_t)b * D + c] = idok ? (vocab[id * D + c] + pr[c] - mean) * rstd * g[c] + be[c] : __int_as_float(0x7fc00000);
}

extern "C" int otvae_ar_embed_step(const int64_t* ids, int64_t ids_stride, int pos, int B, int D, int V, int P, const float* vocab,
                                   const float* positions, const float* ln_g, const float* ln_b, float eps, float* out, void* stream) {
    OTVAE_REQUIRE(ids && vocab && positions && ln_g && ln_b && out, "otvae_ar_embed_step: null pointer");
    OTVAE_REQUIRE(B > 0 && D > 0 && V > 0 && P > 0 && ids_stride >= 0 && eps > 0.f, "otvae_ar_embed_step: bad sizes (B = %d, D = %d, V = %d, P = %d)",
                  B, D, V, P);
    OTVAE_REQUIRE(pos >= 0 && pos < P, "otvae_ar_embed_step: position %d outside the %d learned positions", pos, P);
    ar_embed_step_kernel<<<cdiv(B, 4), 256, 0, (hipStream_t)stream>>>(ids, ids_stride, pos, B, D, V, vocab, positions, ln_g, ln_b, eps, out);
    OTVAE_CHECK_LAUNCH("otvae_ar_embed_step");
    return OTVAE_OK;
}
