/*
 * otvae.h -- C ABI of libotvae_hip.so, the MI355X (gfx950) implementation of the training-step hot path of
 * theoad/ot-vae-lightning.  Plain pointers and sizes only (no torch / HIP types): `stream` is a hipStream_t
 * passed as void* (NULL = default stream).  All pointers are DEVICE pointers unless stated otherwise.
 *
 * Conventions
 *   - Activations are fp32 NHWC ([N][H][W][C] contiguous).  Conv weights are HWIO ([KH][KW][Cin][Cout]); the
 *     Python side keeps the reference's logical OIHW shape on a tensor whose strides give this memory order.
 *   - Every function only enqueues work on `stream`: no allocation, no host synchronisation, no global state, so
 *     all of them can be captured into a hipGraph.  Workspaces are supplied by the caller.
 *   - Return value: OTVAE_OK or a negative OTVAE_E* code (bad shape/argument -> nothing was launched).
 *   - There is no CPU implementation behind this ABI.
 *
 * Each entry point cites the reference code (paths under ot_vae_lightning/) whose arithmetic it replaces.
 */
#ifndef OTVAE_H
#define OTVAE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OTVAE_OK 0
#define OTVAE_EINVAL (-1)       /* bad argument / shape */
#define OTVAE_EUNSUPPORTED (-2) /* valid but not implemented for this size */
#define OTVAE_ELAUNCH (-3)      /* hipLaunch / runtime error */

int otvae_abi_version(void);           /* bumps when a signature changes */
const char* otvae_last_error(void);    /* host string describing the last non-OK return of this thread */
int otvae_device_info(int* n_cu, int* wave_size, char* arch, int arch_len); /* host query helper */
/* A HIP stream of the library's own on the calling thread's current device (hipStreamNonBlocking), for hosts whose framework hands out
 * streams from a small round-robin pool (torch: 32 per device -- the 33rd "new" stream is the first one again, and two lanes of one
 * captured step end up on one queue).  The Python mirror recycles the streams it creates and never destroys them. */
int otvae_stream_create(void** stream);
int otvae_stream_destroy(void* stream);

/* Geometry of one ConvLayer (networks/cnn.py:48-154,183-192): input [N][Hs][Ws][Cs] --(nearest x`up`)-->
 * conv KHxKW / stride / pad --> [N][Ho][Wo][Cn].  `up` is 1 or 2; up==2 requires stride==1.  pad >= 0 and Ho, Wo > 0:
 * a negative padding or an empty output is OTVAE_EINVAL. */
typedef struct {
    int32_t N, Hs, Ws, Cs;
    int32_t up;
    int32_t Ho, Wo, Cn;
    int32_t KH, KW, stride, pad;
} otvae_conv_geom;

/* ---- BatchNorm2d, training mode (networks/cnn.py:122,184) ------------------------------------------------- */
/* per-channel partial sums of x[M][C]: partial[2][C][P] (double, P fastest), P = otvae_bn_stats_nparts(M, C). */
int otvae_bn_stats_nparts(int64_t M, int C);
int otvae_bn_stats(const float* x, int64_t M, int C, double* partial, void* stream);
/* mean/invstd from the partials; for each of `n_bn` BatchNorm modules sharing this input (a ConvBlock's
 * block[0] and skip normalise the same tensor) writes scale = gamma*invstd, shift = beta - mean*scale and updates
 * running_mean/var (momentum, unbiased var) and num_batches_tracked.  Arrays of n_bn device pointers are HOST
 * arrays. running pointers may be NULL (no update).  `ld` = row stride of the partials (C for otvae_bn_stats, CnPad when
 * they come from the producing conv's epilogue, see otvae_conv_fwd). */
int otvae_bn_finalize(const double* partial, int P, int ld, int64_t M, int C, float eps, float momentum,
                      float* mean, float* invstd, int n_bn,
                      const float* const* gamma, const float* const* beta,
                      float* const* running_mean, float* const* running_var, int64_t* const* num_batches_tracked,
                      float* const* scale, float* const* shift, void* stream);

/* ---- ConvLayer.forward: y = conv(up(relu?(x*scale+shift))) + bias (+ residual) ---------------------------- */
/* scale/shift NULL -> no normalisation; relu applies after the affine; bias/residual NULL -> absent.
 * residual has y's shape (ConvBlock `out + skip(x)`, networks/cnn.py:334). wT is the HWIO weight. */
/* stat_partial (nullable): fp64 [2][CnPad][P] per-block partial sums (sum y, sum y^2) per output channel, written by
 * the epilogue so that the NEXT layer's BatchNorm needs no separate pass over y; P, CnPad from _stats_ws. */
int otvae_conv_fwd_stats_ws(const otvae_conv_geom* g, int* P, int* CnPad);
int otvae_conv_fwd(const otvae_conv_geom* g, const float* x, const float* scale, const float* shift, int relu,
                   const float* wT, const float* bias, const float* residual, float* y, double* stat_partial,
                   void* stream);

/* HWIO [T][Cs][Cn] -> [T][Cn][Cs] (the dgrad operand layout) */
int otvae_weight_transpose(const float* wT, float* wD, int T, int Cs, int Cn, void* stream);
/* the same for every conv weight of a model in one launch: device table[n_layers][5] of int64
 * {src element offset (from src_base), dst element offset (from dst_base), T, Cs, Cn}; max_elems = largest T*Cs*Cn */
int otvae_weight_transpose_batched(const float* src_base, float* dst_base, const int64_t* table, int n_layers,
                                   int64_t max_elems, void* stream);

/* ---- ConvLayer backward ------------------------------------------------------------------------------------ */
/* Data gradient.  gv[N][Hs][Ws][Cs] = d loss / d (x*scale+shift) i.e. the gradient entering BatchNorm's output
 * (after the nearest-upsample sum and the ReLU mask recomputed from x).  With mean/invstd != NULL also writes
 * the per-block fp64 partial sums bn_partial[2][CsPad][P] of (gv, gv*xhat) that BatchNorm backward needs;
 * P and CsPad from otvae_conv_bwd_data_ws. */
int otvae_conv_bwd_data_ws(const otvae_conv_geom* g, int* P, int* CsPad);
int otvae_conv_bwd_data(const otvae_conv_geom* g, const float* gy, const float* wD,
                        const float* x, const float* scale, const float* shift, int relu,
                        const float* mean, const float* invstd,
                        float* gv, double* bn_partial, void* stream);
/* BatchNorm backward for up to two branches that normalise the same x (block[0] and skip):
 * finalize: reduces the partials, writes dgamma/dbeta of each branch and the coefficient vectors coef[(2+nb)][C]
 * apply:    dx = sum_b coef[2+b][c]*gv_b - coef[0][c]*x - coef[1][c]   (elementwise, M*C elements) */
int otvae_bn_bwd_finalize(int nb, const double* const* bn_partial, const int* P, int CsPad, int64_t M, int C,
                          const float* mean, const float* invstd, const float* const* gamma,
                          float* const* dgamma, float* const* dbeta, float* coef, void* stream);
int otvae_bn_bwd_apply(int nb, const float* const* gv, const float* x, const float* coef, int64_t M, int C,
                       float* dx, void* stream);

/* Weight (+bias) gradient.  Workspace partial[P][K+hasb][Cn] floats with K = KH*KW*Cs; P from _ws.
 * gw is written in HWIO order, gb[Cn] if has_bias. */
int otvae_conv_bwd_weight_ws(const otvae_conv_geom* g, int has_bias, int* P);
int otvae_conv_bwd_weight(const otvae_conv_geom* g, const float* x, const float* scale, const float* shift, int relu,
                          const float* gy, int has_bias, float* partial, float* gw, float* gb, int defer_reduce,
                          void* stream);
/* With defer_reduce != 0 only the partials are written; the caller later reduces any number of layers in one launch
 * (host arrays of n entries; K = KH*KW*Cs, Kp = K + has_bias, P from otvae_conv_bwd_weight_ws).
 * Taps that touch the image for no output position (8 of the 9 taps of a 3x3 layer on a 1x1 map, 12 of the 16 of a
 * 4x4 stride-2 layer from 2x2 to 1x1) have an exactly zero gradient: otvae_conv_dead_taps returns them (bit kh*KW+kw).
 * With defer_reduce == OTVAE_DEFER_SPARSE the weight-gradient kernels may leave the partial rows of those taps
 * unwritten; the caller must then pass the layer's Cs and mask to otvae_wgrad_reduce_batched, which writes zeros there
 * without reading the partials (Cs and dead may both be NULL: every row is read). */
#define OTVAE_DEFER_DENSE 1
#define OTVAE_DEFER_SPARSE 2
int otvae_conv_dead_taps(const otvae_conv_geom* g, uint32_t* mask);
int otvae_wgrad_reduce_batched(int n, const float* const* partial, const int* P, const int* K, const int* Kp,
                               const int* Cn, float* const* gw, float* const* gb, const int* Cs, const uint32_t* dead,
                               void* stream);
/* The same with a destination window per layer (otvae_conv_job.ldgw / gw_col0; both arrays NULL, or ldgw[j] == 0: dense): gw[j] is
 * the whole [K][ldgw[j]] gradient, the partials are those of the Cn[j]-wide layer; columns outside the window are written as exact
 * zeros by the same launch.  A windowed entry has no bias row (Kp[j] == K[j]).  Sums are formed exactly as for the dense layer. */
int otvae_wgrad_reduce_batched_win(int n, const float* const* partial, const int* P, const int* K, const int* Kp,
                                   const int* Cn, float* const* gw, float* const* gb, const int* Cs, const uint32_t* dead,
                                   const int* ldgw, const int* gw_col0, void* stream);

/* ---- several independent ConvLayer kernels in ONE launch ----------------------------------------------------
 * The two branches of a ConvBlock (block[0] and skip read the same x, networks/cnn.py:311-335) in the forward pass,
 * and the weight- and data-gradient of every branch in the backward pass, are independent of each other; at the
 * layer sizes of this model each one alone fills a fraction of the 256 CUs.  otvae_conv_multi gives exactly the
 * results of otvae_conv_fwd / otvae_conv_bwd_data / otvae_conv_bwd_weight called once per job (same kernels bodies,
 * same fixed-order reductions, same workspace layouts), but packs the MFMA-path jobs into one launch whose workgroups
 * are divided among the jobs; jobs on another path (image-tile kernels, tiny channel counts) are launched one by one or two by
 * two (otvae_conv_multi_launches below).  No job may read
 * what another job of the same call writes.  `jobs` is a HOST array. */
#define OTVAE_JOB_FWD 0
#define OTVAE_JOB_BWD_DATA 1
#define OTVAE_JOB_BWD_WEIGHT 2
/* ---- BatchNorm statistic SLOTS (round 4): cross-block sums without a finalize launch, bit-reproducible --------------------------------
 * Instead of P per-block partials a producer may add its per-channel sums into `nslots` (a power of two <= 64: the caller's choice, the
 * same number for the producer and the consumer of a buffer; atomics on one address are performed one after the other, ~0.1 us each,
 * so nslots should grow with the producer's block count) accumulators of int64 fixed-point limbs with integer atomics (associative:
 * the totals do not depend on arrival order); layout and arithmetic in csrc/common.h.  `slots` buffers hold
 * otvae_bn_slots_words(ld, nslots) int64 words, are 16-byte
 * aligned and must be ZERO before the producer runs.  A consumer kernel that is handed an otvae_bn_fold
 * turns the sums into (scale, shift) in its own prologue -- every block for itself -- and its first block leaves mean / invstd / scale /
 * shift in global memory for the backward pass and advances the running buffers: what otvae_bn_finalize did in a launch of its own
 * (reference: nn.BatchNorm2d in training mode, networks/cnn.py:122,184).  otvae_bn_finalize_slots is the stand-alone form. */
typedef struct otvae_bn_fold {
    const void* slots;            /* NULL: no fold */
    int32_t ld;                   /* channel stride of the slots (>= channels) */
    int32_t nslots;               /* slots in use (power of two <= 64): what the producer of `slots` was given */
    int64_t count;                /* elements per channel: N * H * W of the normalised tensor */
    float eps, momentum;
    const float* gamma;
    const float* beta;
    float* running_mean;          /* nullable (with running_var, num_batches_tracked) */
    float* running_var;
    int64_t* num_batches_tracked;
    float* mean_out;              /* nullable pair: the branch that publishes the statistics the branches share */
    float* invstd_out;
    float* scale_out;             /* this branch's affine, for the backward pass */
    float* shift_out;
} otvae_bn_fold;
int64_t otvae_bn_slots_words(int ld, int nslots);
int otvae_bn_stats_slots(const float* x, int64_t M, int C, void* slots, int ld, int nslots, void* stream);
int otvae_bn_finalize_slots(int n_bn, const otvae_bn_fold* folds, int C, void* stream);
/* The BatchNorm backward pair (otvae_bn_bwd_finalize + otvae_bn_bwd_apply below) as ONE launch, for sums (sum gv, sum gv * xhat) that a
 * data-gradient job left in slots (otvae_conv_job.bn_slots, otvae_attn_stage_bwd_slots): the finalize arithmetic runs in the launch's
 * prologue, its first block writes dgamma / dbeta.  dx == NULL: parameter gradients only (gv / x may then be NULL).  training == 0:
 * eval-mode BatchNorm (a fixed affine: no batch-statistics terms in dx).  C <= 1024. */
int otvae_bn_bwd_apply_slots(int nb, const float* const* gv, const float* x, const void* const* slots, const int* nslots, int ld,
                             int64_t M, int C, const float* mean, const float* invstd, const float* const* gamma,
                             float* const* dgamma, float* const* dbeta, int training, float* dx, void* stream);

typedef struct otvae_conv_job {
    int32_t kind;               /* OTVAE_JOB_* */
    int32_t relu;               /* ReLU after the (optional) affine of the layer INPUT x */
    int32_t has_bias;           /* BWD_WEIGHT */
    int32_t defer_reduce;       /* BWD_WEIGHT: 0, OTVAE_DEFER_DENSE or OTVAE_DEFER_SPARSE */
    otvae_conv_geom geom;
    const float* x;             /* layer input [N][Hs][Ws][Cs] (BWD_DATA: only for the ReLU mask / BatchNorm sums) */
    const float* scale;         /* BatchNorm scale/shift of x, or NULL */
    const float* shift;
    const float* w;             /* FWD: HWIO weight; BWD_DATA: dgrad-layout weight (otvae_weight_transpose) */
    const float* bias;          /* FWD */
    const float* residual;      /* FWD */
    float* y;                   /* FWD */
    double* stat_partial;       /* FWD (nullable) */
    const float* gy;            /* BWD_DATA / BWD_WEIGHT: gradient of the layer output */
    const float* mean;          /* BWD_DATA (nullable, with invstd and bn_partial) */
    const float* invstd;
    float* gv;                  /* BWD_DATA */
    double* bn_partial;
    float* wpartial;            /* BWD_WEIGHT workspace */
    float* gw;                  /* BWD_WEIGHT */
    float* gb;
    void* stat_slots;           /* FWD (nullable, instead of stat_partial): statistic slots of the OUTPUT, channel stride = the ld of otvae_conv_fwd_stats_ws */
    void* bn_slots;             /* BWD_DATA (nullable, instead of bn_partial): statistic slots of the BatchNorm-backward sums, channel stride = the CsPad of otvae_conv_bwd_data_ws */
    int32_t stat_nslots;        /* slots in use in stat_slots / bn_slots (power of two <= 64) */
    int32_t bn_nslots;
    otvae_bn_fold fold;         /* FWD (fold.slots nullable): the BatchNorm of the INPUT x folded into this launch; scale / shift are then ignored */
    /* ---- a COLUMN WINDOW of a wider weight (all three 0: the dense layer).  geom.Cn is the width of the window. */
    int32_t ldw;                /* FWD: row pitch (floats) of the HWIO weight `w` points INTO, >= Cn; `w` is the window's first column.
                                 * BWD_DATA: the window's rows of the dgrad-layout weight are contiguous, so ldw is 0 or Cs.
                                 * A job with ldw != 0 always runs as a one-job implicit-GEMM launch (never direct / image-tile / packed). */
    int32_t ldgw;               /* BWD_WEIGHT: row pitch (floats) of `gw` (the WHOLE gradient, >= gw_col0 + Cn); has_bias must be 0; P from otvae_conv_window_ws.  The */
    int32_t gw_col0;            /* reduction writes the window's columns [gw_col0, gw_col0 + Cn) and exact zeros into every other column */
} otvae_conv_job;
int otvae_conv_multi(int n, const otvae_conv_job* jobs, void* stream);
/* The workspace queries for the jobs of a layer over a column window of a weight with `ld` output channels (geom.Cn = the window):
 * statistics rows / padded Cn of the forward job and BatchNorm-backward rows / padded Cs of the data-gradient job with ldw != 0 (planned
 * on the implicit GEMM whatever the dense layer of the same geometry takes), and the split-K partials of the weight-gradient job with
 * ldgw = ld: it splits the pixels as the wide layer's job does, so the window of the gradient is bit for bit what that job computes. */
int otvae_conv_window_ws(const otvae_conv_geom* g, int ld, int* P_fwd, int* CnPad, int* P_bwd, int* CsPad, int* P_wgrad);
/* Introspection for measurement (bench.py's per-kernel roofline): what the calling thread's last otvae_conv_multi did --
 * bit i of packed_mask: job i ran inside one packed conv_jobs_kernel launch; uniform_tap: that launch's template flavour
 * (1 = conv_jobs_kernel<true>), -1 if nothing was packed. */
int otvae_conv_multi_last(unsigned* packed_mask, int* uniform_tap);
/* The number of kernel launches the calling thread's last otvae_conv_multi made (immediate weight-gradient reductions included).
 * Two forward or two data-gradient jobs of the image-tile kernels, or of the direct kernels for tiny channel counts, share ONE launch
 * when a two-job kernel exists for them (the heads of the ConvBlocks at 8x8 and larger maps); OTVAE_PAIR_LAUNCH=0 in the environment
 * launches them one by one.  Results are the same bits either way. */
int otvae_conv_multi_launches(int* n);
/* Host query, launches nothing: the (tile, tap) visits of the implicit-GEMM launch that serves the forward pass (mode 0) or the data
 * gradient (mode 1) of a layer -- `launch_rule`: every 64-row tile walks each tap some row of the launch can use (the rule before
 * the per-tile list, and of OTVAE_GEMM_LIVE_TAPS=0); `per_tile`: rows position-major, a tile walks the taps one of ITS rows can use.
 * Both counts are equal for a layer on the scalar path (a channel count not a multiple of 4).  The counts assume 16-byte aligned
 * tensors: a launch given a misaligned x / gy, weight, scale or shift pointer takes the scalar path whatever its channel counts.  Returns OTVAE_EUNSUPPORTED when the
 * image-tile or direct kernels take the layer (not served by the implicit GEMM). */
int otvae_conv_gemm_chunks(const otvae_conv_geom* g, int mode, int64_t* launch_rule, int64_t* per_tile);

/* ---- QKVAttention (networks/nets_utils.py:63-82) ---------------------------------------------------------- */
/* qkv [N][T][3*H*C] (channel = which*H*C + h*C + c) -> out [N][T][H*C]; lse [N][H][T] saved for backward.
 * aux (nullable; honoured for head widths C <= 2, ignored otherwise): [N][H][T][C*C] per-query covariance of values and
 * keys under the attention weights, D[c'][c] = sum_s p_s (v_s[c'] - out[c']) k_s[c].  Passing the same buffer to
 * otvae_attn_bwd lets it form dq[c] = sum_c' gout[c'] D[c'][c] without a pass over the keys; with aux == NULL it
 * recomputes the pairs. */
int otvae_attn_fwd(const float* qkv, int N, int T, int H, int C, float* out, float* lse, float* aux, void* stream);
int otvae_attn_bwd(const float* qkv, const float* out, const float* lse, const float* gout, const float* aux,
                   int N, int T, int H, int C, float* gqkv, void* stream);
/* The same kernels with an explicit score scale: scores = scale * q.k (otvae_attn_fwd / _bwd use 1/C, the product of the
 * two C^-1/2 factors of QKVAttention; torch.nn.MultiheadAttention inside the reference's ViT, networks/vit.py:169-172,
 * uses 1/sqrt(C)). */
int otvae_attn_fwd_scaled(const float* qkv, int N, int T, int H, int C, float scale, float* out, float* lse, float* aux,
                          void* stream);
int otvae_attn_bwd_scaled(const float* qkv, const float* out, const float* lse, const float* gout, const float* aux, int N,
                          int T, int H, int C, float scale, float* gqkv, void* stream);

/* The whole AttentionBlock forward (networks/cnn.py:212-240: proj_out(attention(qkv(BN(x)))) [+ the ConvBlock's skip, cnn.py:331-335])
 * as ONE launch: a workgroup owns whole images, forms q / k / v of its tokens from the normalised input (scale / shift [H*C] = the
 * BatchNorm affine in front of the bias-free 1x1 qkv convolution, both NULL without one; wqkv [H*C][3*H*C], wproj [H*C][H*C] in the
 * HWIO order of otvae_conv_fwd), runs the attention of otvae_attn_fwd_scaled and applies the bias-free 1x1 output projection,
 * the residual sum (nullable) and the per-channel partial sums of y for the next BatchNorm (stat_partial [2][H*C][rows], nullable;
 * rows from otvae_attn_stage_plan).  qkv [N][T][3*H*C] (nullable: only a three-launch backward pass reads it), out [N][T][H*C] (the attention output), lse and aux are written as by the
 * three separate launches: the backward pass is theirs.  otvae_attn_stage_plan returns OTVAE_EUNSUPPORTED (no error text) for
 * shapes the fused kernel does not take (T == 1, T % 4 != 0, a width that is not a power of two <= 32, heads that do not fit one
 * workgroup): the caller then issues the three launches. */
int otvae_attn_stage_plan(int N, int T, int H, int C, int need_aux, int* stat_rows);
int otvae_attn_stage_fwd(const float* x, const float* scale, const float* shift, const float* wqkv, const float* wproj,
                         const float* residual, int N, int T, int H, int C, float qk_scale, float* qkv, float* out, float* lse,
                         float* aux, float* y, double* stat_partial, void* stream);
/* The same launch with the BatchNorm in front of the qkv convolution FOLDED IN (fold->slots != NULL: scale / shift are ignored, see
 * otvae_bn_fold) and / or the output's statistics into statistic slots (stat_slots, channel stride H * C) instead of stat_partial. */
int otvae_attn_stage_fwd_fold(const float* x, const otvae_bn_fold* fold, const float* scale, const float* shift, const float* wqkv,
                              const float* wproj, const float* residual, int N, int T, int H, int C, float qk_scale, float* qkv,
                              float* out, float* lse, float* aux, float* y, double* stat_partial, void* stat_slots, int stat_nslots,
                              void* stream);

/* The AttentionBlock's backward pass as ONE launch on what otvae_attn_stage_fwd wrote (qkv, out, lse, aux): the attention output's
 * gradient is formed from gy [N][T][H*C] (gout = gy . wproj^T), the attention backward of otvae_attn_bwd_scaled writes gqkv
 * [N][T][3*H*C] (read afterwards by the qkv weight-gradient job), and gv [N][T][H*C] = gqkv . wqkv^T, the gradient of the qkv
 * convolution's normalised input, leaves with the BatchNorm-backward partial sums bn_partial [2][H*C][rows] (sum gv, sum gv * xhat per
 * channel, xhat = (x - mean) * invstd: what otvae_conv_bwd_data emits for otvae_bn_bwd_finalize; mean / invstd / x / bn_partial all
 * NULL without a BatchNorm).  qkv == NULL (otvae_attn_stage_fwd was given qkv == NULL and wrote none: 12 of the 28 bytes per value it
 * moves at the small maps): q / k / v are formed again from x through scale / shift, the forward kernel's arithmetic.  rows from
 * otvae_attn_stage_bwd_plan, which returns OTVAE_EUNSUPPORTED for shapes the kernel does not
 * take (the caller then issues the three launches). */
int otvae_attn_stage_bwd_plan(int N, int T, int H, int C, int* bn_rows);
int otvae_attn_stage_bwd(const float* gy, const float* wproj, const float* wqkv, const float* x, const float* mean,
                         const float* invstd, const float* scale, const float* shift, const float* qkv, const float* out,
                         const float* lse, const float* aux, int N, int T, int H, int C, float qk_scale, float* gqkv, float* gv,
                         double* bn_partial, void* stream);
/* The same launch with the BatchNorm-backward sums into statistic slots (channel stride H * C; consumed by otvae_bn_bwd_apply_slots). */
int otvae_attn_stage_bwd_slots(const float* gy, const float* wproj, const float* wqkv, const float* x, const float* mean,
                               const float* invstd, const float* scale, const float* shift, const float* qkv, const float* out,
                               const float* lse, const float* aux, int N, int T, int H, int C, float qk_scale, float* gqkv, float* gv,
                               void* bn_slots, int bn_nslots, void* stream);

/* Element-wise dropout with the same counter-based masks (keep(row, col) of a [rows][D] tensor, D % 4 == 0), optionally
 * fused with the ReLU in front of it: y = keep ? act(x)/(1-p) : 0.  relu != 0: the dropout(relu(linear1(x))) of a training-
 * mode nn.TransformerEncoderLayer; relu == 0: PositionalEmbedding's embedding dropout (networks/vit.py:54-58).  The backward
 * recomputes the mask from used[0] and reads x for the ReLU gate. */
int otvae_dropout_fwd(const float* x, int64_t rows, int D, int relu, float p, const int64_t* key, int stream_id, float* y,
                      int64_t* used, void* stream);
int otvae_dropout_bwd(const float* x, const float* gy, int64_t rows, int D, int relu, float p, const int64_t* used, float* gx,
                      void* stream);
/* keep[row*cols + col] = 1 iff the hashed dropout of the call that left `used` keeps (row, col); uint8 [rows][cols].
 * row / col are what the producing kernel hashes: attention (slice*Tq + query, key token); LayerNorm and token
 * dropout (row, column); dropout2d (n, c).  Test and debugging aid. */
int otvae_dropout_keep_mask(int64_t rows, int cols, float p, const int64_t* used, uint8_t* keep, void* stream);

/* Self-attention with dropout on the attention probabilities: nn.MultiheadAttention(dropout=p) in training mode, which is
 * how the reference's ViT builds every layer (networks/vit.py:157-172 hand `dropout` to nn.TransformerEncoderLayer;
 * configs/vae/vit.yaml trains with 0.1).  P = softmax(scale * q k^T), out = (P o keep / (1-p)) v, keep ~ Bernoulli(1-p).
 * The T x T mask is never stored: keep[t][s] is a counter-based hash of (call key, slice, t, s) that the backward pass
 * recomputes.  key: device int64[2] {seed, call counter} -- device memory, so that a captured hipGraph draws a fresh mask
 * on every replay once the host bumps the counter with a captured add; stream_id (0..4094) tells call sites apart.  The
 * forward writes the call key it derived to used[0] (device int64[1]); the backward reads it from there.
 * causal != 0 restricts the softmax of token t to tokens s <= t (the ViT's `causal_mask`, networks/vit.py:215-217); p may
 * then be 0.  lse is the natural log of the UN-dropped row sums.  T <= 256 and T*(2C+3) <= 16384; C in {1,2,4,8,16,32}. */
int otvae_attn_dropout_fwd(const float* qkv, int N, int T, int H, int C, float scale, float p, int causal, const int64_t* key,
                           int stream_id, float* out, float* lse, int64_t* used, void* stream);
int otvae_attn_dropout_bwd(const float* qkv, const float* out, const float* lse, const float* gout, int N, int T, int H,
                           int C, float scale, float p, int causal, const int64_t* used, float* gqkv, void* stream);
/* Cross-attention: nn.MultiheadAttention(query, memory, memory) inside the nn.TransformerDecoderLayer of the ViT's
 * `preprocess_depth` variant (networks/vit.py:171-181, 240-244): Tq queries of one token set against Tk keys / values of another,
 * scores = scale * q.k, the same dropout on the probabilities as above (p may be 0: key / used may then be NULL).  q, k and v
 * are addressed as ptr[n * img_stride + t * row_stride + h * C + c] (strides in floats), so thirds of one in-projected
 * tensor or three separate tensors both fit; out [N][Tq][H*C], lse [N][H][Tq]; the backward writes gq / gk / gv through their
 * own strides and touches nothing else.  max(Tq, Tk) <= 256 and max(Tq, Tk)*(2C+3) <= 16384; C in {1,2,4,8,16,32}. */
int otvae_attn_cross_fwd(const float* q, int64_t q_img_stride, int q_row_stride, const float* k, const float* v,
                         int64_t kv_img_stride, int kv_row_stride, int N, int Tq, int Tk, int H, int C, float scale, float p,
                         const int64_t* key, int stream_id, float* out, float* lse, int64_t* used, void* stream);
int otvae_attn_cross_bwd(const float* q, int64_t q_img_stride, int q_row_stride, const float* k, const float* v,
                         int64_t kv_img_stride, int kv_row_stride, const float* out, const float* lse, const float* gout, int N,
                         int Tq, int Tk, int H, int C, float scale, float p, const int64_t* used, float* gq,
                         int64_t gq_img_stride, int gq_row_stride, float* gk, float* gv, int64_t gkv_img_stride,
                         int gkv_row_stride, void* stream);

/* ---- LayerNorm over the last dimension (the token streams of the ViT: networks/vit.py:38,54 and the two norms of each
 * nn.TransformerEncoderLayer, :169-172; torch.nn.functional.layer_norm arithmetic) ---------------------------------------
 * y[m][:] = (s - mean(s)) * rstd(s) * gamma + beta with s = x[m][:] + res[m][:] (res nullable: the "x + sublayer(x)" of the
 * post-norm block summed in; s is written to sum_out [M][D], which otvae_layernorm_bwd takes as xs; without a residual
 * sum_out may be NULL and xs = x).  mean / rstd [M] are saved for backward.  D <= 2048.
 * key != NULL: the "x + dropout(sublayer(x))" of a training-mode nn.TransformerEncoderLayer (networks/vit.py:157-172 with
 * dropout > 0) folded into the same kernels: s = res + x o keep / (1-p), 0 <= p < 1.  keep(row, col) is the counter-based hash of
 * otvae_attn_dropout_* (key = device int64[2] {seed, call counter}, stream_id 0..4094 per call site, the forward leaves its call
 * key in used[0]); nothing but s is stored; res, sum_out and used are then required.  key == NULL: p must be 0, used may be NULL.
 * Backward: gx [M][D] = dL/ds, dgamma / dbeta [D]; ws: otvae_layernorm_bwd_ws(M, D) floats.  used == NULL (p = 0, gx_dropped NULL):
 * gx is the gradient of both x and res.  used = the forward's: gx is the residual's gradient and gx_dropped = gx o keep / (1-p)
 * the sublayer output's. */
int otvae_layernorm_fwd(const float* x, const float* res, const float* gamma, const float* beta, int M, int D, float eps,
                        float p, const int64_t* key, int stream_id, float* sum_out, float* y, float* mean, float* rstd,
                        int64_t* used, void* stream);
int otvae_layernorm_bwd_ws(int M, int D);
int otvae_layernorm_bwd(const float* xs, const float* gy, const float* gamma, const float* mean, const float* rstd, int M, int D,
                        float p, const int64_t* used, float* gx, float* gx_dropped, float* dgamma, float* dbeta, float* ws,
                        void* stream);

/* ---- GaussianPrior / ConditionalGaussianPrior (prior/gaussian.py:58-96, prior/conditional_gaussian.py:44-93) + Prior.forward
 * scaling (prior/base.py:74-78): re-parametrisation z = mu + eps sd and loss[B] = coeff * KL(q || p) in one pass, explicit backward.
 * h [B][S][2D]: within each of the S slices the first D entries are the means, the next D the log-variances (channels-last maps:
 * S = H*W positions; torch.chunk on another dimension: S = the sizes in front of it); eps, z [B][S*D].
 * prior_mean, prior_log_std [B][S*D] (rows of the class embeddings gathered by label): p = N(prior_mean, exp(prior_log_std)^2) per
 * sample; both NULL: p = N(0, I).  The backward also returns the gradients of the gathered rows (each nullable).
 * mode bit 0: empirical_kl -- the Monte-Carlo estimate sum log q(z) - log p(z) at the drawn z instead of the closed form;
 * bit 1: fixed_var -- q = N(h, s) with s = 1, or temp[b] + 1e-8 when a per-sample temperature temp[B] is given (`time` of encode;
 * NULL otherwise, and never with a conditional prior); h is then [B][S][D] (no log-variance half).  gz, gloss: nullable. */
int otvae_gaussian_prior_fwd(const float* h, const float* eps, const float* temp, const float* prior_mean,
                             const float* prior_log_std, int B, int S, int D, float coeff, int mode, float* z, float* loss,
                             void* stream);
int otvae_gaussian_prior_bwd(const float* h, const float* eps, const float* temp, const float* prior_mean,
                             const float* prior_log_std, const float* gz, const float* gloss, int B, int S, int D, float coeff,
                             int mode, float* gh, float* g_prior_mean, float* g_prior_log_std, void* stream);

/* ---- VAE.nelbo reduction (model/vae.py:158-176) ----------------------------------------------------------- */
/* out[3] = {total, recon, prior}: recon = mean((pred-target)^2) over numel entries, prior = mean(prior_loss[0..B))/chw.
 * B = the number of entries of prior_loss: one per latent the prior saw = expansion * batch (model/vae.py:165-169,
 * utils/__init__.py:154-175), independent of numel.  ws: double[otvae_nelbo_ws()] scratch. */
int otvae_nelbo_ws(void);
int otvae_nelbo_fwd(const float* pred, const float* target, int64_t numel, const float* prior_loss, int B,
                    float chw, double* ws, float* out, void* stream);
/* gout[3] = upstream gradient of out: gpred = (gout[0]+gout[1]) * 2*(pred-target)/numel ;
 * gprior[B] = (gout[0]+gout[2])/(B*chw).  gout NULL = {1,0,0}. */
int otvae_nelbo_bwd(const float* pred, const float* target, int64_t numel, int B, float chw,
                    const float* gout, float* gpred, float* gprior, void* stream);

/* ---- ConvLayer activations other than ReLU, and equalized_lr (networks/cnn.py:114-118,128-147,186-188) -----------
 * kind: 0 identity, 1 ReLU, 2 LeakyReLU(0.2), 3 SELU, 4 GELU (erf form), 5 SiLU.  x, out, ga, gv: [M][C] channels-last.
 * The fused convolution kernels carry ReLU only; these run unfused around them (csrc/activation.hip). */
/* out = act(x * scale[c] + shift[c]); scale == shift == NULL: out = act(x) */
int otvae_bn_act_fwd(const float* x, const float* scale, const float* shift, int kind, int64_t M, int C, float* out,
                     void* stream);
/* blocks (= partial sums per channel) otvae_bn_act_bwd uses for M rows */
int otvae_bn_act_bwd_parts(int64_t M);
/* gv = ga * act'(x * scale + shift).  With mean / invstd (training-mode BatchNorm in front of the activation) also the
 * BatchNorm-backward sums per block, partial[2][C][P] (fp64) = {sum gv, sum gv * (x - mean) * invstd}: the layout
 * otvae_bn_bwd_finalize reads (its CsPad = C). */
int otvae_bn_act_bwd(const float* ga, const float* x, const float* scale, const float* shift, const float* mean,
                     const float* invstd, int kind, int64_t M, int C, float* gv, double* partial, void* stream);
/* dst[i] = alpha * src[i], n contiguous floats (weight * conv_scale * lr_mult, bias * lr_mult and their gradients) */
int otvae_scale_f32(const float* src, float alpha, int64_t n, float* dst, void* stream);

/* ---- grouped / dilated ConvLayer (networks/cnn.py:66-67,103-104: nn.Conv2d(in, out, k, stride, padding, dilation, groups)).
 * The layer's weight w [Cout][Cin / groups][KH][KW] (contiguous, as nn.Conv2d stores it) is expanded into the dense weight of the
 * convolution entry points, dense [(KH-1) dil + 1][(KW-1) dil + 1][Cin][Cout] (HWIO memory): zeros between groups and in the holes
 * of the dilation.  _bwd gathers the dense weight's gradient back onto w's layout.  The expanded kernel may span at most 7 x 7. */
int otvae_weight_expand_fwd(const float* w, int Cout, int Cin, int groups, int KH, int KW, int dilation, float* dense, void* stream);
int otvae_weight_expand_bwd(const float* gdense, int Cout, int Cin, int groups, int KH, int KW, int dilation, float* gw, void* stream);

/* ---- GroupNorm / InstanceNorm2d in front of a ConvLayer's activation (networks/cnn.py:121-125: nn.GroupNorm(div_sqrt(C // groups), C),
 * nn.InstanceNorm2d(C) = G == C without gamma / beta).  x, out, ga, dx [N][HW][C] channels-last; statistics per (sample, group) over
 * the group's C / G channels and all HW positions (biased variance, eps inside the root); kind: the activation codes above. */
/* out = act(xhat * gamma + beta) (gamma == beta == NULL: act(xhat)); mean, rstd [N][G] are kept for the backward */
int otvae_group_norm_act_fwd(const float* x, const float* gamma, const float* beta, int N, int HW, int C, int G, float eps, int kind,
                             float* out, float* mean, float* rstd, void* stream);
/* dx of the same chain from ga = dL/d out; with gamma also the per-sample parameter partials pgamma, pbeta [N][C]
 * (d gamma = otvae_colsum_f32(pgamma), d beta likewise) */
int otvae_group_norm_act_bwd(const float* ga, const float* x, const float* gamma, const float* beta, const float* mean,
                             const float* rstd, int N, int HW, int C, int G, int kind, float* dx, float* pgamma, float* pbeta,
                             void* stream);
/* dst[c] = sum_r src[r][c] in fixed order, src [R][C] */
int otvae_colsum_f32(const float* src, int R, int C, float* dst, void* stream);
/* Backward pass of an embedding lookup (nn.Embedding: the ViT's class token, networks/vit.py:167,203; the class rows of
 * ConditionalGaussianPrior, prior/conditional_gaussian.py:76-77): gw[k][:] = sum of g[b][:] over the b with idx[b] == k, in
 * increasing b.  g [B][d], idx [B] int64, gw [K][d] (every row written). */
int otvae_embedding_bwd(const float* g, const int64_t* idx, int B, int K, int d, float* gw, void* stream);

/* ---- FiLM conditioning (`additional_embed`) and Dropout2d of ConvLayer (networks/cnn.py:112-118,160-192); x, out, g [N][HW][C] ------- */
/* out = x * scale[n][c] + bias[n][c] (scale / bias [N][C]: the two Linear projections of the activated embedding) */
int otvae_film_fwd(const float* x, const float* scale, const float* bias, int N, int HW, int C, float* out, void* stream);
/* gx = g * scale; gscale[n][c] = sum_hw g x; gbias[n][c] = sum_hw g */
int otvae_film_bwd(const float* g, const float* x, const float* scale, int N, int HW, int C, float* gx, float* gscale, float* gbias,
                   void* stream);
/* FiLM and the layer's activation in one pass each way (csrc/film_act.hip): out = act(x * scale[n][c] + bias[n][c]), act_kind as in
 * otvae_bn_act_fwd (0: none); the same bits as otvae_film_fwd followed by otvae_bn_act_fwd.  N <= 65535, HW * C < 2^31. */
int otvae_film_act_fwd(const float* x, const float* scale, const float* bias, int N, int HW, int C, int act_kind, float* out,
                       void* stream);
/* v = x * scale + bias; ga = g * act'(v); gx = ga * scale; gscale[n][c] = sum_hw ga x; gbias[n][c] = sum_hw ga (fp64 sums in a fixed
 * order: bit-reproducible).  gscale / gbias NULL together: only gx.  ws: otvae_film_act_bwd_ws bytes, 8-byte aligned (NULL when that
 * is 0 or gscale is NULL): fp64 partials of the row chunks a small batch is cut into. */
int64_t otvae_film_act_bwd_ws(int N, int HW, int C);
int otvae_film_act_bwd(const float* g, const float* x, const float* scale, const float* bias, int N, int HW, int C, int act_kind,
                       float* gx, float* gscale, float* gbias, void* ws, void* stream);
/* Gaussian Fourier features of GaussianFourierProjection (networks/nets_utils.py:51-52): out[n] = [sin(p), cos(p)] [N][2 * half],
 * p = ((t[n] * w[j]) * 2) * pi in fp32 in that order; t [N], w [half] */
int otvae_fourier_features(const float* t, const float* w, int N, int half, float* out, void* stream);
/* nn.Dropout2d(p): y = keep(n, c) ? x / (1 - p) : 0 with keep = hash(call key, n, c); key = device int64[2] {seed, call counter},
 * used[0] <- the call key (the backward recomputes the mask from it; no mask tensor) */
int otvae_dropout2d_fwd(const float* x, int N, int HW, int C, float p, const int64_t* key, int stream_id, float* y, int64_t* used,
                        void* stream);
int otvae_dropout2d_bwd(const float* gy, int N, int HW, int C, float p, const int64_t* used, float* gx, void* stream);

/* ---- GaussianModel(update_with_autograd=True): log-density under N(mean, L L^T) / N(mean, diag(sigma^2))
 * (ot/distribution_models/gaussian_model.py:52-55,76-93,125-128; torch.distributions.MultivariateNormal(scale_tril=) /
 * Independent(Normal) in the reference).  fp64, x / y / qg [nb][B][D], mean [nb][D], L [nb][D][D] lower triangular with a
 * positive diagonal (diag != 0: sigma [nb][D]), D <= 128. */
/* y = L^-1 (x - mean); lp[nb][B] = -|y|^2 / 2 - sum_i log L_ii - D/2 log(2 pi) */
int otvae_mvn_logprob_fwd(const double* x, const double* mean, const double* L, int nb, int B, int D, int diag, double* y,
                          double* lp, void* stream);
/* qg_b = g_b L^-T y_b (diag: g_b y_b / sigma): d mean = sum_b qg_b, d x_b = -qg_b,
 * d L = tril(sum_b qg_b y_b^T) - (sum_b g_b) diag(1 / L_ii), formed by the caller with otvae_gemm_f64 */
int otvae_mvn_logprob_bwd(const double* g, const double* y, const double* L, int nb, int B, int D, int diag, double* qg,
                          void* stream);

/* ---- Adam (model/vae.py:148-151; torch.optim.Adam defaults) over one flat buffer --------------------------- */
/* dst[i][0..n[i]) = src[i][0..n[i]) for `count` contiguous fp32 ranges in one launch per 32 (pointer tables on the HOST, passed to the
 * kernel by value): the gradients autograd left in p.grad (embeddings, learned tokens) into their slots of the flat gradient buffer
 * that otvae_adam_step reads -- what the reference's optimizer finds in p.grad (model/vae.py:148-151). */
int otvae_copy_batched(int count, const float* const* src, float* const* dst, const int64_t* n, void* stream);

/* The start of a step as ONE launch: *step += 1 (device int32, the 1-based count of the update this step ends in), the step guard's
 * backup (n > 0: state[n], every running buffer of the model as one flat fp32 range, is copied to backup; a refused step copies it
 * back) and the zeroing of `zero_words` int64 words (the BatchNorm statistic slots the step's kernels add into; 16-byte aligned, an
 * even count, may be 0).  otvae_zero_words: the zeroing alone. */
int otvae_step_begin(int32_t* step, const float* state, float* backup, int64_t n, void* zero, int64_t zero_words, void* stream);
/* hyper (device): float[4] = {lr, beta1, beta2, eps}; step: the counter otvae_step_begin incremented.  g is multiplied by
 * grad_scale first (1/world_size for data-parallel means), or by grad_scale_dev[0] when given (what otvae_grad_clip_coef leaves).
 * Guarded update (guard != NULL; watch_loss and state need it): what makes a bad step survivable inside a captured training step (the
 * reference leans on Lightning's loop to stop on a NaN loss, configs/ddp.yaml:1-5; a hipGraph replay has no host in the loop).  The
 * update is applied only when every watched device scalar is finite: watch_loss[0] (the step's loss; a starved Sinkhorn solve poisons it
 * with NaN; nullable), and grad_scale_dev[0..1] = {scale, |g|} when given (with max_norm <= 0 otvae_grad_clip_coef only reports the
 * norm).  A skipped step leaves p, m, v unchanged, takes *step back by one, restores state[n_state] from backup (a NaN that reaches a
 * BatchNorm does not stay one -- the next ReLU maps the NaN-normalised tensor to zeros -- so later layers would fold finite but
 * meaningless batch statistics into their running buffers; n_state 0: no such buffers), and counts itself: guard[0] += 1, guard[1] =
 * the step number that was skipped (device int32[2]).
 * ema_shadow (nullable): the parameter moving average of the reference's `ema_decay` option (model/base.py:99,153-190; kept there by
 * the third-party torch_ema package, requirements.txt:10, unpinned): ema_shadow[n] -= (1 - d) (ema_shadow - p_new), d = min(ema_decay,
 * (1 + t) / (10 + t)) with t the device step counter (one update per accepted optimizer step), in the optimizer's own pass.  A refused
 * step leaves the shadow alone. */
int otvae_adam_step(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper, int32_t* step,
                    float grad_scale, const float* grad_scale_dev, const float* watch_loss, int32_t* guard, float* state,
                    const float* backup, int64_t n_state, float* ema_shadow, double ema_decay, void* stream);
/* The same moving-average update alone, with the caller's effective decay (a stock optimizer stepped by the reference's own loop) */
int otvae_ema_update(float* shadow, const float* p, int64_t n, double decay, void* stream);
int otvae_zero_words(void* zero, int64_t zero_words, void* stream);

/* ---- global-norm gradient clipping (configs/ddp.yaml:4 `gradient_clip_val: 1.0`, applied by Lightning through
 * torch.nn.utils.clip_grad_norm_) over the flat gradient buffer -------------------------------------------------- */
/* g[n] holds the gradient SUM over ranks, grad_scale = 1/world_size.  norm = |g * grad_scale|_2 (fp64 accumulation);
 * out[0] = grad_scale * min(1, max_norm / (norm + 1e-6)) = the scale otvae_adam_step applies to g (grad_scale_dev); out[1] = norm.
 * max_norm <= 0: no clipping (out[0] = grad_scale).  ws: otvae_grad_clip_ws() doubles. */
int otvae_grad_clip_ws(void);
int otvae_grad_clip_coef(const float* g, int64_t n, float grad_scale, float max_norm, double* ws, float* out,
                         void* stream);

/* ---- generic convolution: any stride, square footprints up to 32 x 32 (the fallback behind the tuned kernels, which take strides 1 / 2
 * and footprints up to 7 x 7): what `ConvLayer(down_sample=s)` makes for s >= 4 -- a (2 s) x (2 s) kernel with stride s, e.g. the
 * 8 x 8 / stride 4 layers of CNN(scaling_factor=4) (networks/cnn.py:98-101,605-621).  Plain direct convolutions (no BatchNorm / activation
 * fusion, geom->up must be 1), NHWC activations, HWIO weights, fp32, deterministic. ---- */
int otvae_conv_generic_fwd(const otvae_conv_geom* geom, const float* x, const float* w_hwio, const float* bias, float* y, void* stream);
int otvae_conv_generic_bwd_data(const otvae_conv_geom* geom, const float* gy, const float* w_hwio, float* gx, void* stream);
int64_t otvae_conv_generic_bwd_weight_ws(const otvae_conv_geom* geom, int has_bias); /* floats */
int otvae_conv_generic_bwd_weight(const otvae_conv_geom* geom, const float* x, const float* gy, int has_bias, float* ws,
                                  float* gw_hwio, float* gb, void* stream);

/* ---- standard-normal draws (prior/gaussian.py:93 `q.rsample()`, the prior samples of the minibatch-OT prior) ---------- */
/* out[n] ~ N(0, 1) from a counter-based hash of (key[0] = seed, key[1] = call counter, stream_id, element index): the
 * values do not depend on the launch shape.  key = device int64[3] {seed, counter, 0}; advance != 0: the call's last
 * workgroup increments the counter, so a captured step draws fresh noise on every replay without host work. */
int otvae_normal_fill(float* out, int64_t n, int64_t* key, int stream_id, int advance, void* stream);

/* ---- sinkhorn_log (ot/w2_utils.py:276-319) ---------------------------------------------------------------- */
/* a[nb][N], b[nb][M], C[nb][N][M] -> pi[nb][N][M] (may alias no input), u[nb][N], v[nb][M] potentials.
 * dtype: 0 = fp32, 1 = fp64.  ws: bytes from otvae_sinkhorn_ws.  Stops all problems at the first iteration where
 * min over the batch of (|du|_1+|dv|_1) < threshold, evaluated on the device (no host sync); threshold <= 0
 * runs exactly max_iter iterations.  iters_done (device int32, may be NULL).
 * Every route below gives the same bits.  otvae_sinkhorn_route tells which one a problem takes, from its shape alone (it neither
 * queries the device nor reads the environment; `tracked` = threshold > 0; -1 for a bad argument):
 *   OTVAE_SK_ROUTE_LAUNCHES (0)      one launch per half-iteration: N or M > 1024, more than 4096 (fp32) / 1024 (fp64) rows, where
 *                                    rows = nb * max(N, M); also every problem when OTVAE_SK_MULTILAUNCH is set in the environment
 *   OTVAE_SK_ROUTE_BARRIER | rpw     all iterations in one launch of cdiv(rows, 8 rpw) <= 128 workgroups of 512 threads, a wave keeping
 *                                    rpw rows of each matrix in registers (1 up to 1024 rows, 2 up to 2048, 4 up to 4096), the
 *                                    potentials exchanged through a counter barrier: fp64, and fp32 when tracked
 *   OTVAE_SK_ROUTE_FLAGS | rpw       the same with every potential entry travelling as one {epoch, value} word and no barrier:
 *                                    fp32 with a fixed iteration count
 * The workgroups of a one-launch solve wait for each other, so the solve checks at run time that the device holds them all at
 * once and takes the launches if not.  That guard cannot bind here for the shapes above: they need at most 128 workgroups, the
 * MI355X has 256 CUs, and every CU holds at least one 512-thread workgroup of these kernels (their launch bound keeps the registers
 * within one CU's file, and the potential takes <= 16 KiB of LDS). */
#define OTVAE_SK_ROUTE_LAUNCHES 0
#define OTVAE_SK_ROUTE_BARRIER 0x10
#define OTVAE_SK_ROUTE_FLAGS 0x20
int otvae_sinkhorn_route(int dtype, int nb, int N, int M, int tracked);
int64_t otvae_sinkhorn_ws(int dtype, int nb, int N, int M);
int otvae_sinkhorn_log(int dtype, const void* a, const void* b, const void* C, int nb, int N, int M,
                       double reg, int max_iter, double threshold, void* ws,
                       void* pi, void* u, void* v, int32_t* iters_done, void* stream);
/* The reference's sinkhorn_log is plain torch arithmetic: autograd differentiates it through every iteration with respect to
 * a, b and C (ot/w2_utils.py:301-319).  These two entry points are that derivative.  otvae_sinkhorn_log_tape: the same solve (one
 * launch per half-iteration, the kernels of otvae_sinkhorn_log's launch route: identical bits and stopping rule) that also keeps what the reverse sweep needs in `tape`
 * (otvae_sinkhorn_tape_bytes: Cr, Cr^T, log marginals, the potentials of every iteration, the iteration count).
 * otvae_sinkhorn_log_bwd: gpi[nb][N][M] = dL/dpi -> gC[nb][N][M], ga[nb][N], gb[nb][M] (each may be NULL; ga / gb need a / b),
 * ws: otvae_sinkhorn_bwd_ws bytes.  The iteration count the forward stopped at is read on the device (no host sync). */
int64_t otvae_sinkhorn_tape_bytes(int dtype, int nb, int N, int M, int max_iter);
int64_t otvae_sinkhorn_bwd_ws(int dtype, int nb, int N, int M, int max_iter);
int otvae_sinkhorn_log_tape(int dtype, const void* a, const void* b, const void* C, int nb, int N, int M, double reg,
                            int max_iter, double threshold, void* tape, void* pi, void* u, void* v, int32_t* iters_done,
                            void* stream);
int otvae_sinkhorn_log_bwd(int dtype, const void* gpi, const void* pi, const void* a, const void* b, int nb, int N, int M,
                           double reg, int max_iter, void* tape, void* ws, void* gC, void* ga, void* gb, void* stream);
/* The same solve on C / max(C) per problem, the `cost_matrix / max_per_mat` of batch_ot_gmm (ot/w2_utils.py:265-266), without
 * a pass that finds the maximum or divides: pmax[nb][P] are partial maxima of each problem's C (otvae_sqdist_max leaves them),
 * reduced inside the solver's first kernel; cmax[nb] (may be NULL) receives the maxima.  a / b may be NULL in both entry points:
 * uniform marginals 1/N, 1/M.
 * A persistent solve whose bounded wait ran out (OTVAE_SK_SPIN_LIMIT polls, default 2^22) fills pi, u, v with NaN and reports
 * iters_done = -1: a starved solve cannot pass for a result. */
int otvae_sinkhorn_log_normalized(int dtype, const void* a, const void* b, const void* C, const void* pmax, int P, int nb,
                                  int N, int M, double reg, int max_iter, double threshold, void* ws, void* pi, void* u, void* v,
                                  void* cmax, int32_t* iters_done, void* stream);
/* The minibatch-OT prior's forward (configs[2]/[3]: BASELINE.json; the arithmetic of ot/w2_utils.py:265-269 on
 * C_ij = |z_i - y_j|^2 with uniform marginals) in one call: C[N][M], pi[N][M], u[N], v[M], cost[1] = sum C * pi, cmax[1]
 * (may be NULL).  z[N][D], y[M][D].  cost[cost_rep] = loss_scale * sum C * pi, the same value cost_rep times (the Prior
 * contract returns one loss entry per sample, prior/base.py:74-78; loss_scale = loss_coeff x annealing).
 * ws: otvae_sinkhorn_prior_ws bytes. */
int64_t otvae_sinkhorn_prior_ws(int dtype, int N, int M);
int otvae_sinkhorn_prior_fwd(int dtype, const void* z, const void* y, int N, int M, int D, double reg, int max_iter,
                             double threshold, double loss_scale, int cost_rep, void* ws, void* C, void* pi, void* u, void* v,
                             void* cost, void* cmax, int32_t* iters_done, void* stream);
/* cost[nb] = sum_ij C*pi (fp64 accumulate, fixed order), out dtype = dtype; ws: double[nb*256] */
int otvae_ot_cost(int dtype, const void* C, const void* pi, int nb, int N, int M, double* ws, void* cost, void* stream);
/* pairwise squared euclidean cost C[nb][N][M] = |x_i - y_j|^2, x[nb][N][D], y[nb][M][D] */
int otvae_sqdist(int dtype, const void* x, const void* y, int nb, int N, int M, int D, void* C, void* stream);
/* the same, also leaving the maximum of every output tile in pmax[nb][otvae_sqdist_max_parts(dtype, N, M)] */
int otvae_sqdist_max_parts(int dtype, int N, int M);
int otvae_sqdist_max(int dtype, const void* x, const void* y, int nb, int N, int M, int D, void* C, void* pmax, void* stream);
/* Gradient of scale * sum_ij C_ij pi_ij with respect to z for C_ij = |z_i - y_j|^2 and a fixed plan (the minibatch OT prior's
 * backward, SinkhornPrior): gz[i][d] = 2 scale (sum_q g[q]) sum_j pi_ij (z_id - y_jd); z [N][D], y [M][D], pi [N][M]; g[ng] =
 * the upstream gradients of the ng replicas of the cost that the forward handed out (device memory); gadd[N][D] (may be
 * NULL) is added to the result (the gradient reaching z through its other consumer, the decoder).  fp32 runs on the
 * matrix cores (16 x 16 x 4 MFMA tiles, fixed summation order). */
int otvae_ot_cost_grad(int dtype, const void* z, const void* y, const void* pi, const void* g, int ng, double scale,
                       const void* gadd, int N, int M, int D, void* gz, void* stream);

/* ---- Sinkhorn divergence between latents and prior draws (SinkhornDivergencePrior; Genevay, Peyre, Cuturi 2018) -------- */
/* z[N][D], y[M][D], dtype 0 = fp32 / 1 = fp64, N, M, D >= 1, N and M may differ.
 *   S(z, y) = W(z, y) - W(z, z) / 2 - W(y, y) / 2,   W(p, q) = sum_ij C_pq,ij pi_pq,ij,   C_pq,ij = |p_i - q_j|^2
 * cmax = max C_zy; the three plans are the entropic plans of C_zy / cmax, C_zz / cmax, C_yy / cmax with uniform marginals after exactly
 * max_iter iterations of sinkhorn_log (v, then u) with the same reg: one absolute epsilon = reg cmax for all three, the same iteration
 * count for all three (no threshold), so that the bias terms cancel and S(z, z) = 0.
 * One cost launch leaves all three matrices: the cross block with the arithmetic and the tile maxima of otvae_sqdist_max (fp32: 64 x 64
 * tiles on the 16 x 16 x 4 MFMA path), the self blocks from their upper-triangle tiles mirrored at the store: bitwise symmetric, exact
 * zero diagonal.  The solve is otvae_sinkhorn_log_normalized's, every problem on the cross block's maxima: with N == M one batch of
 * three, otherwise three consecutive solves on the stream (otvae_sinkhorn_route tells the route of each).  batched: -1 = that rule,
 * 0 = three consecutive solves whatever the shape, 1 = one batch of three (N == M only); the bits do not depend on it.
 *   terms[3] (fp64) = W(z, y), W(z, z), W(y, y), unscaled, each summed in fp64 in the fixed order of otvae_ot_cost;
 *   loss[i] = loss_scale (terms[0] - terms[1] / 2 - terms[2] / 2) for every i < N (one entry per sample, prior/base.py:74-78);
 *   pi_zy[N][M], pi_zz[N][N]: the plans the gradient needs (fp32: 16-byte aligned);
 *   iters[1] = max_iter, or -1 if a one-launch solve was starved: then loss, terms and both plans are NaN.
 * A latent or draw that is not finite makes the loss NaN.  6 launches batched (cost, init, solve, finish, read-out x 2), 12 otherwise (one-launch solves).
 * ws: otvae_sinkhorn_div_ws bytes (-1: N or M beyond 32768 or a bad argument).
 * otvae_sinkhorn_div_grad, the envelope gradient (plans held constant, nothing for y), one launch, no atomics, no workspace:
 *   gz[i][d] = (gadd ? gadd[i][d] : 0) + s (2 sum_j pi_zy,ij (z_id - y_jd) - sum_j (pi_zz,ij + pi_zz,ji) (z_id - z_jd)),
 *   s = scale sum_q g[q], g[ng] the upstream gradients of the loss replicas (device memory), gadd[N][D] the gradient reaching z
 *   through its other consumer.  fp32: the K-concatenated product [pi_zy | -(pi_zz + pi_zz^T) / 2] [y ; z] on the matrix cores, the
 *   transposed operand read through LDS, fixed summation order. */
int64_t otvae_sinkhorn_div_ws(int dtype, int N, int M);
int otvae_sinkhorn_div_fwd(int dtype, const void* z, const void* y, int N, int M, int D, double reg, int max_iter, double loss_scale,
                           int batched, void* ws, void* loss, double* terms, void* pi_zy, void* pi_zz, int32_t* iters, void* stream);
int otvae_sinkhorn_div_grad(int dtype, const void* z, const void* y, const void* pi_zy, const void* pi_zz, const void* g, int ng,
                            double scale, const void* gadd, int N, int M, int D, void* gz, void* stream);

/* ---- sliced Wasserstein-2 between latents and prior draws (SlicedWassersteinPrior; SURVEY F3: no reference class) ------- */
/* z[N][D], y[N][D], dirs[L][D] (raw direction draws), all fp32.  theta_l = dirs_l / |dirs_l| (written to theta[L][D]); p = z theta^T,
 * q = y theta^T; every column of p (with its row indices) and of q is sorted in LDS by a bitonic network padded with +inf to the next
 * power of two, ties by the smaller original row.  resid[l][i] = p_l,i - q_l,(rank_l(i)) in ORIGINAL row order;
 * loss[loss_rep] = scale / (L N) sum_l sum_i resid[l][i]^2, the same value loss_rep times (prior/base.py:74-78).  One workgroup per
 * projection leaves an fp64 partial in ws (otvae_sliced_w2_ws bytes, 8-byte aligned); a one-block second launch sums them in index order:
 * the loss is bit-reproducible and no float atomic is used.  A projection that is not finite makes the loss NaN.
 * Envelope: 1 <= N <= 4096, D >= 1, L >= 1; beyond it OTVAE_EUNSUPPORTED (otvae_sliced_w2_ws: -1). */
int64_t otvae_sliced_w2_ws(int N, int L);
int otvae_sliced_w2_fwd(const float* z, const float* y, const float* dirs, int N, int D, int L, double scale, int loss_rep, void* ws,
                        float* theta, float* resid, float* loss, void* stream);
/* gz[i][d] = (gadd ? gadd[i][d] : 0) + (sum_b gout[b]) scale 2 / (L N) sum_l resid[l][i] theta[l][d]; gout[N] are the upstream gradients
 * of the loss replicas, gadd[N][D] (may be NULL) the gradient reaching z through its other consumer.  One launch, fixed summation order. */
int otvae_sliced_w2_bwd(const float* gout, const float* gadd, const float* resid, const float* theta, int N, int D, int L,
                        double scale, float* gz, void* stream);

/* ---- kernel two-sample (MMD) loss between latents and prior draws (MMDPrior; SURVEY F3: no reference class) ------------- */
/* z[N][D], y[M][D], fp32.  r(a, b) = |a - b|^2 (Gram form on the fp32 matrix cores, clamped below at 0, NaN passes the clamp),
 * C_k = 2 D sigma2 scales[k], k = 0 .. nscales - 1 <= 8 (scales: HOST array, read at launch time);
 *   kernel 0 (imq): k(r) = sum_k C_k / (C_k + r),   w(r) = -k'(r) = sum_k C_k / (C_k + r)^2
 *   kernel 1 (rbf): k(r) = sum_k exp(-r / C_k),     w(r) = sum_k exp(-r / C_k) / C_k
 *   Ezz = cz sum_{i != j} k(r(z_i, z_j)), Eyy = cy sum_{i != j} k(r(y_i, y_j)), Ezy = 1 / (N M) sum_{i, j} k(r(z_i, y_j)),
 *   cz = 1 / (N (N - 1)), cy = 1 / (M (M - 1)) (unbiased != 0; needs N, M >= 2) or 1 / N^2, 1 / M^2 with the diagonal k(0) in the sums
 *   (unbiased == 0).  The diagonal is identified by INDEX: two different rows holding the same vector are a pair.
 *   loss[loss_rep] = scale (Ezz + Eyy - 2 Ezy), the same value loss_rep times; terms[3] = (Ezz, Eyy, Ezy), unscaled;
 *   G[N][D] (may be NULL: then the gradient product is skipped) = scale d MMD2 / d z,
 *   d MMD2 / d z_i = -4 cz sum_{j != i} w(r(z_i, z_j)) (z_i - z_j) + 4 / (N M) sum_j w(r(z_i, y_j)) (z_i - y_j).
 * One main launch (a workgroup takes a 32-row tile against a run of 32-row column tiles: Gram tile, k and w, w re-laid through LDS
 * into the A operand of a second product with the staged column rows) and a finishing launch that adds the fp64 partial sums of k
 * and the partial gradient tiles of the column splits in index order: bit-reproducible, no float atomic, nothing of size N x M in
 * memory.  ws: otvae_mmd_ws bytes, 16-byte aligned, written before it is read.  A latent or draw that is not finite makes the loss NaN.
 * Envelope: 1 <= D <= 512, N D and M D below 2^31; beyond it OTVAE_EUNSUPPORTED (otvae_mmd_ws: -1). */
int64_t otvae_mmd_ws(int N, int M, int D);
int otvae_mmd_fwd(const float* z, const float* y, int N, int M, int D, int kernel, const double* scales, int nscales, double sigma2,
                  int unbiased, double scale, int loss_rep, void* ws, float* loss, float* terms, float* G, void* stream);
/* gz[i][d] = (gadd ? gadd[i][d] : 0) + (sum_b gout[b]) G[i][d]; gout[ng] are the upstream gradients of the loss replicas, gadd[N][D]
 * (may be NULL) the gradient reaching z through its other consumer.  One launch; the product is rounded before the single fp32 add. */
int otvae_mmd_bwd(const float* gout, int ng, const float* gadd, const float* G, int N, int D, float* gz, void* stream);

/* ---- Gaussian W2 with empirical covariance as a loss term (GaussianW2Prior; BASELINE north_star) ------------ */
/* Forward tail of L = w2_gaussian(mean_cov(_stats(z)), N(mut, covt)) (ot/w2_utils.py:40-80, ot/matrix_utils.py:145-158,
 * gaussian_model.py:144-157): lam[D], vt[D][D] = eigenvalues / eigenvector rows of M = covt^1/2 cov covt^1/2 (otvae_eigh_fn,
 * fn 3).  mut == NULL: zero mean; covt == NULL: identity (then M = cov and the make_pd shift of the 'spd' validation,
 * w2_utils.py:661-669, is applied to cov and its spectrum alike).  loss[rep] = scale * L (fp32, the same value rep times: one
 * entry per sample, prior/base.py:74-78);  q[D][D] = diag(lam^-1/4) vt, so that M^-1/2 = q^T q. */
int otvae_w2_prior_tail(const double* mu, const double* mut, const double* cov, const double* covt, const double* lam,
                        const double* vt, int D, double scale, int rep, float* loss, double* q, void* stream);
/* Backward: gz[i][:] = gadd[i][:] + (2 scale sum(g) / B) [ (mu - mut) + (z_i - mu) - W (z_i - mu) ], W[D][D] = covt^1/2 M^-1/2
 * covt^1/2 (symmetric) -- the closed form of the reference's autograd through eigh-based sqrtm.  z, gadd (may be NULL), gz:
 * [B][D] fp32 (dtype 0) or fp64 (1); g[ng] fp32 upstream gradients of the loss replicas. */
int otvae_w2_prior_bwd(int dtype, const void* z, int B, int D, const double* mu, const double* mut, const double* W,
                       const float* g, int ng, double scale, const void* gadd, void* gz, void* stream);

/* ---- GaussianModel statistics (ot/distribution_models/gaussian_model.py:99-108,144-157) ------------------- */
/* samples [nb][B][D] (in_dtype 0=fp32,1=fp64) -> fp64 sum_x[nb][D], sum_xx[nb][D][D] (diag: [nb][D]),
 * accumulated into the running buffers:  run = decay<0 ? run + new : run*decay + new*(1-decay)
 * (utils/__init__.py:204-206); n_obs[nb] likewise with new = B.  With accumulate==0 the raw batch statistics are
 * written instead (the all-reduce path reduces them before the EMA). */
int64_t otvae_gauss_stats_ws(int nb, int B, int D, int diag); /* bytes */
int otvae_gauss_stats(int in_dtype, const void* samples, int nb, int B, int D, int diag, int accumulate,
                      double decay, double* ws, double* n_obs, double* sum_x, double* sum_xx, void* stream);
/* mean_cov (ot/matrix_utils.py:145-158): mean = sum/n, cov = sum_xx/n - mean mean^T */
int otvae_mean_cov(const double* n_obs, const double* sum_x, const double* sum_xx, int nb, int D, int diag,
                   double* mean, double* cov, void* stream);

/* ---- validation metrics (csrc/metrics.hip) ---------------------------------------------------------------- */
/* Streaming feature moments of the Frechet distance: what FrechetInceptionDistance._extract_features / update keep per side
 * (metrics/fid.py:99-122: features.sum(0), features.T @ features, the observation count) and mean_cov (ot/matrix_utils.py:145-158)
 * consumes.  feats [B][D] (in_dtype 0 = fp32, 1 = fp64), 1 <= B, 1 <= D <= 2048; ADDS B to n_obs[1], sum_b f_b to sum_x[D] and
 * sum_b f_b f_b^T to sum_xx[D][D] (all fp64) in place on the fp64 matrix cores.  Only the lower triangle is computed; every element is
 * stored to [i][j] and [j][i], so a state that starts symmetric stays bit-symmetric.  Fixed reduction order, no atomics.
 * ws: otvae_moments_accum_ws(B, D) bytes (may be NULL when that is 0) -- at most (4 * D64^2 + 264 * D64) * 8 bytes with D64 = D
 * rounded up to a multiple of 64, whatever B is: below 4.2 * D^2 * 8 from D = 1024 on, and 0 from D = 1985 on (wide features are
 * not split over the batch). */
int64_t otvae_moments_accum_ws(int B, int D); /* bytes; -1: bad argument */
int otvae_moments_accum(int in_dtype, const void* feats, int B, int D, double* n_obs, double* sum_x, double* sum_xx, void* ws,
                        void* stream);
/* PeakSignalNoiseRatio's accumulation in one pass over both tensors (in_dtype as above, numel elements each): state[0] += sum (p - t)^2
 * (differences and sum in fp64), state[1] += numel, state[2] = min(state[2], min target), state[3] = max(state[3], max target).
 * state: otvae_sqerr_state_words() doubles -- the four above followed by scratch of the two-stage fixed-order reduction.  A fresh
 * state is {0, 0, +inf, -inf, ...}. */
int otvae_sqerr_state_words(void);
int otvae_sqerr_accum(int in_dtype, const void* preds, const void* target, int64_t numel, double* state, void* stream);
/* StructuralSimilarityIndexMeasure's accumulation (csrc/ssim.hip): preds / target [B][C][H][W] NCHW-contiguous (in_dtype as above) are
 * each read once.  With E[.] the mean under the separable window wh[kh] x ww[kw] (HOST arrays of weights summing to 1 per axis; they
 * are rounded to fp32 once and travel in the kernel's argument block) at the (H - kh + 1) (W - kw + 1) positions per plane whose
 * window lies inside the image:
 *   mu_p = E[p], mu_t = E[t], s_pp = E[p^2] - mu_p^2, s_tt = E[t^2] - mu_t^2, s_pt = E[p t] - mu_p mu_t,
 *   ssim = (2 mu_p mu_t + c1) (2 s_pt + c2) / ((mu_p^2 + mu_t^2 + c1) (s_pp + s_tt + c2)),  c1 = (k1 R)^2, c2 = (k2 R)^2,
 * the second moments formed about one pixel of the workgroup's tile (they are shift-invariant; E[x^2] - mu^2 of the raw values cancels
 * on narrow-range images), the map evaluated in fp64.  ssim_b is the mean of the map over C and all positions of image b; it depends
 * on image b alone, bit for bit, whatever B is (range_mode 2 excepted: R is the batch's).  per_image (nullable) [B] receives ssim_b;
 * state[0] += sum_b ssim_b, state[1] += B.  Fixed reduction order, no atomics, no host read: one launch over the images and a
 * one-workgroup fold of its partials (range_mode 2: one more launch over the images in front, for R).
 * range_mode 0: R = range_hi - range_lo, inputs as they are (pass range_lo = 0, range_hi = R); 1: inputs are clamped to
 * [range_lo, range_hi] at the load, R = range_hi - range_lo; 2: R = max(max p - min p, max t - min t) over this call's tensors, found
 * on the device by a launch of its own (range_lo / range_hi are ignored).
 * state: otvae_ssim_state_words() doubles -- {sum ssim_b, image count, two unused words} followed by the range pass's per-workgroup
 * minima / maxima (contents unspecified between calls).  A fresh state is all zeros.
 * ws: otvae_ssim_ws(B, C, H, W, kh, kw) bytes -- one double per (image, channel, 16 x 32 tile of positions); the tile and partial
 * layout depend on C, H, W, kh, kw alone.
 * OTVAE_EINVAL: null pointers, non-positive sizes, even windows, H < kh or W < kw, range_hi <= range_lo in modes 0 / 1, k1 / k2 < 0.
 * OTVAE_EUNSUPPORTED (otvae_ssim_ws: -1, as for every refused argument): more than 31 taps on an axis, 2^31 or more tiles or plane
 * elements. */
int otvae_ssim_state_words(void);
int64_t otvae_ssim_ws(int B, int C, int H, int W, int kh, int kw); /* bytes; -1: refused arguments */
int otvae_ssim_accum(int in_dtype, const void* preds, const void* target, int B, int C, int H, int W, int kh, int kw, const double* wh,
                     const double* ww, double k1, double k2, int range_mode, double range_lo, double range_hi, double* per_image,
                     double* state, void* ws, void* stream);
/* The gradient of otvae_ssim_accum's per-image values (csrc/ssim_grad.hip; losses.py's SSIMLoss): with an upstream cotangent g[b]
 * (DEVICE array, fp64) on ssim_b and n = C (H - kh + 1) (W - kw + 1),
 *   grad_preds[q] = alpha(q) + 2 p_q beta(q) + t_q gamma(q),   alpha, beta, gamma = W^T[(g_b / n) a], W^T[(g_b / n) b], W^T[(g_b / n) c],
 *   a = 2 mu_t (A2 - A1) / (B1 B2) - 2 mu_p S / B1 + 2 mu_p S / B2,  b = -S / B2,  c = 2 A1 / (B1 B2)
 * (A1 = 2 mu_p mu_t + c1, A2 = 2 s_pt + c2, B1 = mu_p^2 + mu_t^2 + c1, B2 = s_pp + s_tt + c2, S = A1 A2 / (B1 B2)); W^T is the adjoint
 * of the valid window filter, separable like it.  The kernel evaluates this about a pixel of the workgroup's tile, as the forward does
 * (fp32 differences staged, the coefficients in fp64 from the fp32 moments), so alpha and 2 p beta do not cancel on narrow-range
 * images.  The gradient for target is the same call with preds and target exchanged (S is symmetric).
 * grad_preds [B][C][H][W] in in_dtype: EVERY element is written, nothing need be zeroed.  One launch, fixed summation order, no atomics,
 * no host read; image b's gradient depends on image b and g[b] alone, bit for bit.
 * range_mode 0 and 1 as in otvae_ssim_accum; in mode 1 the gradient is 0 where preds lies strictly outside [range_lo, range_hi]
 * (torch.clamp's rule: equality passes the gradient).
 * ws: otvae_ssim_grad_ws(B, C, H, W, kh, kw) bytes -- 0 at present: each workgroup recomputes the moments under its 16 x 32 tile of
 * pixels in LDS (44 KiB for the 11 x 11 window); ws may then be NULL.
 * OTVAE_EINVAL: as otvae_ssim_accum, and range_mode 2 (R from the batch depends on the data; a loss needs a fixed scale).
 * OTVAE_EUNSUPPORTED (otvae_ssim_grad_ws: -1, as for every refused argument): more than 15 taps on an axis (sigma > 2.0 for a Gaussian
 * window: the tile with its 2 (k - 1) halo no longer fits 64 KiB of LDS), 2^31 or more tiles or plane elements. */
int64_t otvae_ssim_grad_ws(int B, int C, int H, int W, int kh, int kw); /* bytes; -1: refused arguments */
int otvae_ssim_grad(int in_dtype, const void* preds, const void* target, int B, int C, int H, int W, int kh, int kw, const double* wh,
                    const double* ww, double k1, double k2, int range_mode, double range_lo, double range_hi, const double* g,
                    void* grad_preds, void* ws, void* stream);
/* MultiScaleStructuralSimilarityIndexMeasure's accumulation (csrc/ssim.hip; metrics/ms_ssim.py): otvae_ssim_accum's map, window,
 * in_dtype, range_mode and state layout, over S scales.  With p_0 = preds, t_0 = target and scale s on [B][C][H >> s][W >> s],
 *   cs   = (2 s_pt + c2) / (s_pp + s_tt + c2),   ssim = (2 mu_p mu_t + c1) / (mu_p^2 + mu_t^2 + c1) * cs    at every valid position,
 *   v_s[b] = the mean over C and all positions of cs for s < S - 1, of ssim for s = S - 1,
 *   p_{s+1} = the 2 x 2, stride-2 average of p_s (a trailing odd row / column dropped; always of the UNCLAMPED values), t likewise,
 *   msssim_b = prod_s f(v_s[b])^betas[s],   f = identity (normalize 0; a negative v_s gives NaN), relu (1) or (v + 1) / 2 (2).
 * One launch per scale: it reads the scale's pair once, leaves {sum cs, sum ssim} per workgroup in ws and writes the next scale's pair
 * into the pyramids (each pooled element exactly once, in in_dtype); then a one-workgroup fold over all scales in a fixed order.
 * range_mode 1 clamps each scale's images at the load; range_mode 2 takes R per scale from that scale's two images (one more launch
 * per scale).  per_image (nullable) [B] receives msssim_b; w (nullable) [S][B] receives w_s[b] = d msssim_b / d v_s[b] =
 * betas[s] msssim_b f'(v_s) / f(v_s), and 0 where f(v_s[b]) = 0 under normalize 1 / 2: a dead image passes no gradient.  (A deliberate
 * rule: the composed formula meets 0 * inf there, which autograd turns into NaN or into 0 depending on how the derivative of relu is
 * written.)  state[0] += sum_b msssim_b, state[1] += B.  No atomics, no host read; msssim_b, w_.[b] and image b's
 * pooled images depend on image b alone, bit for bit, whatever B is (range_mode 2 excepted).
 * betas: HOST array [S].  state: otvae_ms_ssim_state_words() doubles, laid out as otvae_ssim_accum's; a fresh state is all zeros.
 * pyr_preds / pyr_target: otvae_ms_ssim_pyramid(in_dtype, B, C, H, W, S) bytes each -- scales 1 .. S - 1 of the image, one after the
 * other; written here, read by otvae_ms_ssim_grad (both may be NULL when S = 1).
 * ws: otvae_ms_ssim_ws(B, C, H, W, kh, kw, S) bytes -- two doubles per (scale, image, channel, 16 x 32 tile of positions).
 * OTVAE_EINVAL: as otvae_ssim_accum, S < 1, normalize outside 0 .. 2, and a scale smaller than the window: H >> (S - 1) < kh or
 * W >> (S - 1) < kw.  OTVAE_EUNSUPPORTED (the size queries: -1, as for every refused argument): S > 8, more than 31 taps on an axis,
 * 2^31 or more tiles or plane elements. */
int otvae_ms_ssim_state_words(void);
int64_t otvae_ms_ssim_pyramid(int in_dtype, int B, int C, int H, int W, int S);   /* bytes per image tensor; -1: refused arguments */
int64_t otvae_ms_ssim_ws(int B, int C, int H, int W, int kh, int kw, int S);      /* bytes; -1: refused arguments */
int otvae_ms_ssim_accum(int in_dtype, const void* preds, const void* target, int B, int C, int H, int W, int kh, int kw,
                        const double* wh, const double* ww, double k1, double k2, int range_mode, double range_lo, double range_hi,
                        int S, const double* betas, int normalize, double* per_image, double* w, void* pyr_preds, void* pyr_target,
                        double* state, void* ws, void* stream);
/* The gradient of otvae_ms_ssim_accum's per-image values (csrc/ssim_grad.hip; losses.py's MSSSIMLoss): with an upstream cotangent g[b]
 * (DEVICE array, fp64) on msssim_b, the weights w [S][B] and the pyramids that call left, and n_s = C (H_s - kh + 1) (W_s - kw + 1),
 *   d/dp_s[q] = own_s(q) + 1/4 d/dp_{s+1}[q >> 1]   (no second term at the last scale, nor under a dropped odd row / column),
 *   own_s(q) = alpha(q) + 2 p_q beta(q) + t_q gamma(q),   alpha, beta, gamma = W^T[(g_b w_s[b] / n_s) (a, b, c)]
 * in otvae_ssim_grad's notation; a, b, c are the ones documented there at the last scale and, for the cs scales s < S - 1,
 *   a = 2 (cs mu_p - mu_t) / B2,  b = -cs / B2,  c = 2 / B2      (the same formula with A1 = B1 = 1).
 * One launch per scale from the coarsest to the finest, each built like otvae_ssim_grad's and evaluated about a pixel of the tile.
 * grad_preds [B][C][H][W] in in_dtype: EVERY element is written, nothing need be zeroed; fixed summation order, no atomics, no host
 * read; image b's gradient depends on image b, g[b] and w_.[b] alone, bit for bit.  range_mode 0 and 1 only; in mode 1 the OWN term of
 * a scale is 0 where that scale's preds pixel lies strictly outside [range_lo, range_hi]; the coarser scales' gradient always passes
 * (the pooling took the unclamped values).  The gradient for target is the same call with preds / target and the two pyramids
 * exchanged (every term is symmetric).
 * ws: otvae_ms_ssim_grad_ws(in_dtype, B, C, H, W, kh, kw, S) bytes -- the gradients of scales 1 .. S - 1, alternating between two
 * buffers (0 bytes at S = 1; ws may then be NULL).
 * OTVAE_EINVAL: as otvae_ms_ssim_accum, and range_mode 2.  OTVAE_EUNSUPPORTED (otvae_ms_ssim_grad_ws: -1): S > 8, more than 15 taps
 * on an axis, 2^31 or more tiles or plane elements. */
int64_t otvae_ms_ssim_grad_ws(int in_dtype, int B, int C, int H, int W, int kh, int kw, int S); /* bytes; -1: refused arguments */
int otvae_ms_ssim_grad(int in_dtype, const void* preds, const void* target, const void* pyr_preds, const void* pyr_target, int B, int C,
                       int H, int W, int kh, int kw, const double* wh, const double* ww, double k1, double k2, int range_mode,
                       double range_lo, double range_hi, int S, const double* g, const double* w, void* grad_preds, void* ws,
                       void* stream);
/* Kernel Inception Distance (csrc/kid.hip; metrics/kid.py): the unbiased polynomial-kernel MMD^2 of S subsets of m rows each, in one
 * entry.  real [n_real][D], fake [n_fake][D] fp32 row-major; idx_real / idx_fake [S][m] (device, int32; both NULL: every subset is
 * rows 0 .. m - 1).  For subset s, x_i = real[idx_real[s][i]], y_j = fake[idx_fake[s][j]], k(a, b) = (gamma <a, b> + coef)^degree:
 *   per_subset[s] = (sum_{i != j} k(x_i, x_j) + sum_{i != j} k(y_i, y_j)) / (m (m - 1)) - 2 sum_{i, j} k(x_i, y_j) / m^2
 *   stats = {mean_s per_subset[s], population std (divide by S) of per_subset}
 * (torchmetrics' poly_kernel / maximum_mean_discrepancy).  gamma is the number to use: the caller resolves "default" to 1 / D.
 * Features are converted to fp64 while staged, products and the D-long sums run on the fp64 matrix cores, k is evaluated in fp64 by
 * repeated multiplication; all sums are fp64 in a fixed order (no atomics, no host read), so results are bit-identical from run to
 * run, and exchanging (real, idx_real) with (fake, idx_fake) gives the same bits.  The rows of a subset are gathered at the load: no
 * [S][m][D] or [m][m] array exists in memory.  An index outside [0, n) is clamped into it.
 * ws: otvae_poly_mmd_ws(S, m, D) bytes -- one double per (subset, 128 x 128 tile): S * (nt (nt + 1) + nt^2) * 8 with nt = ceil(m / 128).
 * OTVAE_EINVAL: null pointers (only one index array included), S < 1, D < 1, m < 2, m > min(n_real, n_fake), degree < 1, NaN gamma / coef.
 * OTVAE_EUNSUPPORTED (otvae_poly_mmd_ws: -1, as for every refused argument): D > 2048, S > 65535, degree > 8, m > 2^21. */
int64_t otvae_poly_mmd_ws(int S, int m, int D); /* bytes; -1: refused arguments */
int otvae_poly_mmd_subsets(const float* real, int64_t n_real, const float* fake, int64_t n_fake, int D, const int32_t* idx_real,
                           const int32_t* idx_fake, int S, int m, int degree, double gamma, double coef, void* ws, double* per_subset,
                           double* stats, void* stream);
/* The feature store of the metric: the B rows of feats [B][D] (in_dtype 0 = fp32, 1 = fp64: ROUNDED to fp32 here) are copied to
 * buf[count[0] ...] of buf [capacity][D] fp32; rows that would land at or beyond capacity are not stored.  count (device, int64 [2]:
 * rows stored, rows seen) is read on the device -- a captured call appends at the right place on every replay -- and advanced by a
 * single-thread launch behind the copy: stored = min(stored + B, capacity), seen += B. */
int otvae_feature_append(int in_dtype, const void* feats, int B, int D, float* buf, int64_t capacity, int64_t* count, void* stream);
/* k-nearest-neighbour manifold statistics (csrc/knn_manifold.hip; metrics/prdc.py): the pieces of improved precision / recall and of
 * density / coverage.  Features fp32 row-major, distances d2(a, b) = max(0, (|a|^2 + |b|^2) - 2 <a, b>) in fp64 on the fp64 matrix
 * cores (the tile of otvae_poly_mmd_subsets), the same bits for a pair in every call and whichever side a row is on.  Outputs are
 * order statistics, integer counts and minima: bit-identical from run to run.  Balls are closed (<=).  Finite features are a
 * precondition; nothing of size n x n is in memory.
 * otvae_knn_sq_radii: r2[i] = the k-th smallest of { d2(x_i, x_j) : j != i } -- self is excluded by INDEX: a duplicate row is a neighbour
 *   at distance 0.  x [n][D], r2 [n] fp64.  The nt = ceil(n / 128) column tiles of a 128-row strip are split over otvae_knn_groups(n)
 *   workgroups (the smallest G <= min(nt, 2^25 / n) that minimises ceil(nt G / 512) ceil(nt / G): rounds of resident workgroups times
 *   tiles per workgroup), each leaving its k candidates per row in ws; a second launch merges them.
 *   ws: otvae_knn_sq_radii_ws(n, D, k) bytes = 8 (n + groups n k).
 * otvae_manifold_counts: with d2_ij = d2(real_i, fake_j): count_fake[j] = #{ i : d2_ij <= r2_real[i] } (int32 [n_fake]),
 *   hit_real[i] = 1 if some j has d2_ij <= r2_fake[j], else 0 (int32 [n_real]), min_real[i] = min_j d2_ij (fp64 [n_real]).  Per-tile
 *   partials in ws, combined by a second launch.  ws: otvae_manifold_counts_ws(n_real, n_fake, D) bytes.
 * OTVAE_EINVAL, nothing launched (the _ws queries and otvae_knn_groups: -1): null pointers, k outside 1 .. 16, n <= k (counts: n < 2),
 * D outside 1 .. 2048, n > 2^21. */
int otvae_knn_groups(int64_t n);
int64_t otvae_knn_sq_radii_ws(int64_t n, int D, int k); /* bytes; -1: refused arguments */
int64_t otvae_manifold_counts_ws(int64_t n_real, int64_t n_fake, int D); /* bytes; -1: refused arguments */
int otvae_knn_sq_radii(const float* x, int64_t n, int D, int k, double* r2, void* ws, void* stream);
int otvae_manifold_counts(const float* real, const double* r2_real, int64_t n_real, const float* fake, const double* r2_fake,
                          int64_t n_fake, int D, int32_t* count_fake, int32_t* hit_real, double* min_real, void* ws, void* stream);

/* ---- symmetric eigen-decomposition based matrix functions (ot/matrix_utils.py:37-109) --------------------- */
/* A[nb][D][D] fp64 symmetric (lower triangle is read, like eigh(UPLO='L')).  fn: 0 = none (eigvals only),
 * 1 = sqrtm, 2 = invsqrtm: out[nb][D][D] = V f(lambda) V^T; 3 = eigenvectors: out[nb][k][:] is the unit eigenvector of
 * eigvals[nb][k] (so that callers form several functions of one matrix from a single decomposition).  eigvals[nb][D]
 * are not sorted.  D <= 128: one workgroup per matrix in LDS; 128 < D <= 2048: block Jacobi.
 * ws: bytes from otvae_eigh_ws. */
int64_t otvae_eigh_ws(int nb, int D);
int64_t otvae_eigh_onesided_ws(int nb, int D); /* part of otvae_eigh_ws for D <= 128: the one-sided solver's share */
int64_t otvae_eigh_block_onesided_ws(int nb, int D); /* part of otvae_eigh_ws for 128 < D <= 1024 */
int otvae_eigh_fn(const double* A, int nb, int D, int fn, double* out, double* eigvals, void* ws, void* stream);
/* otvae_eigh_fn started from an orthonormal basis the caller already has (Vinit[nb][D][D], row k = vector k; e.g. the eigenvectors
 * of the previous training step's latent covariance, prior/gaussian_w2.py): the iteration begins with the nearly orthogonal columns
 * A v_k and needs 2-4 sweeps instead of ~9; the result is the same decomposition.  A must be symmetric in both triangles; g0:
 * scratch of nb*D*D doubles.  warm (nullable): device int read by the kernels, 0 = "Vinit holds nothing yet" (run cold): lets a
 * captured step decide per replay.  Vinit == NULL, D > 128: the cold solver. */
int otvae_eigh_fn_warm(const double* A, const double* Vinit, const int* warm, int nb, int D, int fn, double* out, double* eigvals,
                       void* ws, double* g0, void* stream);
/* make_psd (ot/matrix_utils.py:123-142) without host sync: shift_b = (any_b lambda_min_b <= thr ? 1 : 0) *
 * (|min(lambda_min_b,0)| + (strict ? 1e-8 : 0)), A_b += shift_b * I.  cond_any: 1 = apply only if some matrix of
 * the batch fails the test (w2_utils.py:667-669), 0 = always (gaussian_model.py:204-214). */
int otvae_make_psd(double* A, const double* eigvals, int nb, int D, int strict, int cond_any, void* stream);
/* Lower Cholesky factor L[nb][D][D] of A[nb][D][D] (fp64, lower triangle read): the factor torch.distributions.MultivariateNormal
 * samples with (the reference's stochastic apply_transport, ot/w2_utils.py:521-525).  info[nb] (may be NULL): 0, or 1 + the index
 * of the first non-positive pivot (then L holds NaN from that column on).  L must not alias A. */
int otvae_cholesky(const double* A, int nb, int D, double* L, int* info, void* stream);
/* C[nb][m][n] = alpha * op(A) op(B) + beta*C, fp64, row-major; transX: 0 = N, 1 = T. bcast flags: operand has
 * batch stride 0 */
int otvae_gemm_f64(int transA, int transB, int nb, int m, int n, int k, double alpha, const double* A, int a_bcast,
                   const double* B, int b_bcast, double beta, double* C, void* stream);
/* the same in fp32: the small weighted sums of the mixture / codebook models (weights @ atoms, probs^T @ samples:
 * ot/distribution_models/base.py:241-251, codebook_model.py:145-148, ot/transport/discrete_transport.py:70-76) */
int otvae_gemm_f32(int transA, int transB, int nb, int m, int n, int k, float alpha, const float* A, int a_bcast,
                   const float* B, int b_bcast, float beta, float* C, void* stream);
/* y[rows][K] = softmax_k(scale * x) and its backward gx = scale * y o (gy - sum_k y gy): the assignment distributions
 * softmax(energy / temperature) (base.py:216-224) and F.gumbel_softmax (:234-235); dtype 0 = fp32, 1 = fp64 */
int otvae_softmax_rows(int dtype, const void* x, int64_t rows, int K, double scale, void* y, void* stream);
int otvae_softmax_rows_bwd(int dtype, const void* y, const void* gy, int64_t rows, int K, double scale, void* gx, void* stream);
/* out[rows] = log sum_k exp(x[r][k]) (torch.logsumexp over the last dimension: the mixture log-density read-out of
 * GaussianMixtureModel, gaussian_model.py:129-132 on a MixtureSameFamily) and its backward gx[r][k] = g[r] exp(x[r][k] - lse[r]) */
int otvae_lse_rows(int dtype, const void* x, int64_t rows, int K, void* out, void* stream);
int otvae_lse_rows_bwd(int dtype, const void* x, const void* lse, const void* g, int64_t rows, int K, void* gx, void* stream);
/* w2_gaussian tail (ot/w2_utils.py:78-80): out[nb] = |ms-mt|^2 + tr(cs + ct - 2*sqrt_mix) */
int otvae_w2_tail(const double* ms, const double* mt, const double* cs, const double* ct, const double* sqrt_mix,
                  int nb, int D, double* out, void* stream);
/* w2_gaussian (ot/w2_utils.py:40-80) and the non-stochastic full-matrix operator of eq. 17 (compute_transport_operators ->
 * _compute_transport_full_mat, :756-769) of the same nb pairs of Gaussians in one call, from the spectra of the two covariances
 * (lam_x[nb][D], vt_x[nb][D][D] with row k = eigenvector k, as otvae_eigh_fn(fn = 3) returns them), including the reference's
 * 'spd' argument validation (:661-669: with make_pd a strictly positive shift |min(lambda_min, 0)| + 1e-8 on a side whose batch
 * holds a matrix that is not positive definite).  w2[nb], T[nb][D][D] = (1 - pg_star) Cs^-1/2 (Cs^1/2 Ct Cs^1/2)^1/2 Cs^-1/2 + pg_star I.
 * No host synchronisation inside: flags[3] (device ints) = {a source covariance is not positive definite, a target covariance is
 * not, Ct^1/2 Cs Ct^1/2 is not symmetric} for the caller to turn into the reference's ValueErrors.  ws: otvae_w2_transport_ws(nb, D)
 * bytes; eigh_ws: otvae_eigh_ws(2 * nb, D) bytes. */
int64_t otvae_w2_transport_ws(int nb, int D);
int otvae_w2_transport(const double* ms, const double* mt, const double* cs, const double* ct, const double* lam_s, const double* vt_s,
                       const double* lam_t, const double* vt_t, int nb, int D, double pg_star, int make_pd, void* ws, void* eigh_ws,
                       double* w2, double* T, int* flags, void* stream);
/* apply_transport (ot/w2_utils.py:517-520): y[nb][B][D] = T[nb] (x - ms) + mt ; x dtype 0/1, y same dtype */
int otvae_apply_transport(int dtype, const void* x, const double* ms, const double* mt, const double* T,
                          int nb, int B, int D, void* y, void* stream);

/* ---- CodebookModel.energy/assign 'argmax'/predict (ot/distribution_models/codebook_model.py:150-160,
 *      base.py:216-233): x[nb][B][d], codebook[nb][K][d] -> idx[nb][B] (int64), enc[nb][B][d] = codebook[idx].
 *      idx is always in [0, K): a sample with a NaN weight (NaN component, or any NaN atom) gets 0, the reference's
 *      argmax(softmax(.)) of a row that the NaN has made all NaN. */
int otvae_codebook_assign(const float* x, const float* codebook, int nb, int B, int K, int d, float temperature,
                          int64_t* idx, float* enc, void* stream);
/* The assignment distribution itself (base.py:216-224): probs[nb][B][K] = softmax_k(energy/temperature), and
 * (nullable) entropy[nb][B] = -sum_k p log p, which the CodebookPrior 'kl' loss uses (prior/codebook.py:81-82). */
int otvae_codebook_probs(const float* x, const float* codebook, int nb, int B, int K, int d, float temperature,
                         float* probs, float* entropy, void* stream);
/* its backward with respect to the samples (the reference's codebook is a frozen parameter unless update_with_autograd,
 * codebook_model.py:84-86): gprobs[nb][B][K] / gentropy[nb][B] are the upstream gradients (either may be NULL), probs the
 * forward's output; gx[nb][B][d].  K <= 4096. */
int otvae_codebook_probs_bwd(const float* x, const float* codebook, const float* probs, const float* gprobs,
                             const float* gentropy, int nb, int B, int K, int d, float temperature, float* gx, void* stream);

/* The same with the gradient of the atoms too: CodebookModel(update_with_autograd=True) trains its codebook as a parameter
 * (reference ot/distribution_models/codebook_model.py:89 `requires_grad=self.update_with_autograd`; energies :158-160 under
 * torch.autograd).  coef_ws: [nb][B][K] floats of workspace; gc: [nb][K][d], summed over the samples in a fixed order. */
int otvae_codebook_probs_bwd_atoms(const float* x, const float* codebook, const float* probs, const float* gprobs,
                                   const float* gentropy, int nb, int B, int K, int d, float temperature, float* gx,
                                   float* coef_ws, float* gc, void* stream);

/* CodebookModel.energy for the metrics besides the hot path's euclidean p = 2 (ot/distribution_models/codebook_model.py:155-168):
 * metric 0: 1 / (cdist_p(x, c) + 1e-8) for any p > 0; metric 1 ('cosine'): |x . c| / ((sum |x|^p)(sum |c|^p) + 1e-8)^(1/p).
 * E [nb][B][K], raw (MixtureMixin.assign applies topk and the temperature afterwards, base.py:216-224).  _bwd: gx [nb][B][d] and /
 * or gc [nb][K][d] (NULL = not wanted) from gE, summed in a fixed order. */
int otvae_codebook_energy(const float* x, const float* codebook, int nb, int B, int K, int d, int metric, float p, float* E,
                          void* stream);
int otvae_codebook_energy_bwd(const float* x, const float* codebook, const float* gE, int nb, int B, int K, int d, int metric,
                              float p, float* gx, float* gc, void* stream);
/* k-means sufficient statistics for one-hot ('argmax') assignments (MixtureMixin.kmean_iteration, base.py:241-252):
 * counts[nb][K] = number of samples per atom, sums[nb][K][d] = their sum, members added in increasing sample order. */
int otvae_codebook_kmeans(const float* x, const int64_t* idx, int nb, int B, int K, int d, float* counts, float* sums,
                          void* stream);

/* ---- Gaussian mixture (diagonal covariances): GaussianMixtureModel.energy, gassian_mixture_model.py:91-99 ------------
 * energy[nb][B][K] = log N(x_b; mean_k, diag var_k) + log w_k for x [nb][B][d], mean / var [nb][K][d], logw [nb][K];
 * dtype 0 = fp32, 1 = fp64 (all tensors).  The assignment (softmax / argmax over K) and the weighted sufficient
 * statistics that follow are [B][K]-sized library reductions on the caller's side. */
int otvae_gmm_diag_energy(int dtype, const void* x, const void* mean, const void* var, const void* logw, int nb, int B, int K,
                          int d, void* energy, void* stream);

/* ---- Discrete Auto Diffuser (model/discrete_auto_diffuser.py) ------------------------------------------------------------------------ */
/* DAD.prior_loss's cross-entropy (discrete_auto_diffuser.py:63-72: two sliced copies, two transposes, F.cross_entropy with soft labels,
 * sum over the tokens) in one pass: loss[b] = sum_{t < T-1} ( -sum_k probs[b][t+1][k] * log_softmax(logits[b][t][:])[k] ), the
 * one-token shift done by index arithmetic.  logits / probs: fp32 [B][T][K] addressed as base + b * stride_b + t * stride_t + k (strides in
 * elements, rows of K contiguous values; read only, so a transposed or broadcast view is taken in place).  Also written, for the backward pass: lse[B][T] (log-sum-exp of row (b, t)) and psum[B][T]
 * (sum_k probs[b][t+1][k]); their column T-1 is 0.  ws: otvae_soft_ce_ws(B, T) bytes, 8-byte aligned.  Fixed reduction orders, the sums
 * in fp64.  T < 2 or K < 1: OTVAE_EUNSUPPORTED. */
int64_t otvae_soft_ce_ws(int B, int T);
int otvae_soft_ce_fwd(const float* logits, int64_t logits_stride_b, int64_t logits_stride_t, const float* probs,
                      int64_t probs_stride_b, int64_t probs_stride_t, int B, int T, int K, float* loss, float* lse, float* psum,
                      void* ws, void* stream);
/* Its backward pass (what autograd derives from discrete_auto_diffuser.py:63-72), gloss [B]: dlogits[b][t][k] = gloss[b] *
 * (exp(logits[b][t][k] - lse[b][t]) * psum[b][t] - probs[b][t+1][k]) for t < T-1 and exactly 0 in row T-1; dprobs[b][t+1][k] =
 * -gloss[b] * (logits[b][t][k] - lse[b][t]) and exactly 0 in row 0.  dlogits / dprobs: contiguous [B][T][K], either may be NULL. */
int otvae_soft_ce_bwd(const float* logits, int64_t logits_stride_b, int64_t logits_stride_t, const float* probs,
                      int64_t probs_stride_b, int64_t probs_stride_t, const float* lse, const float* psum, const float* gloss, int B,
                      int T, int K, float* dlogits, float* dprobs, void* stream);
/* One step of DAD.sample's loop (discrete_auto_diffuser.py:88-89: Categorical(logits[:, i].softmax(-1)).sample()):
 * ids[b][col] = the number of k whose cumulative sum of exp(logits[b][pos][0..k] - max) is <= u[b] * total, clamped to K-1 -- the inverse
 * CDF of u[b] under softmax(logits[b][pos][:]), exp and the scan in fp64 in index order.  logits: fp32, row (b, pos) at base + b * stride_b +
 * pos * stride_t; u [B] in [0, 1), or NULL: drawn from the library's counter-based generator, key = device int64[2] {seed, call counter}
 * (the draw depends on (key, col, b) only; the caller advances the counter).  ids: int64 [B][T] with row stride ids_stride. */
int otvae_categorical_sample(const float* logits, int64_t stride_b, int64_t stride_t, int pos, int B, int K, const float* u,
                             const int64_t* key, int64_t* ids, int64_t ids_stride, int T, int col, void* stream);
/* The same step (discrete_auto_diffuser.py:88-89, which the reference can only draw unfiltered) under a temperature, top-k and top-p
 * (nucleus) filtering, applied in that order; otvae_categorical_sample's parameters, then:
 *   temperature >= 0: weights w_k = exp((logits[k] - max) / temperature) in fp64; 0 decodes greedily;
 *   top_k (0 = off): the first min(top_k, K) entries of the order (logit descending, index ascending: ties fall to the lower index) survive;
 *   top_p in (0, 1] (1 = off): a survivor is kept iff the mass of the survivors before it in the order, over the survivors' total, is < top_p
 *     (the smallest prefix whose mass reaches top_p; the first entry is always kept);
 *   kept [B] (nullable): the number of kept entries per row.
 * ids[b][col] = the inverse CDF of u[b] over the kept entries walked in index order, dropped entries weighing 0: the number of entries whose
 * cumulative kept mass is <= u[b] * (kept total), clamped to the last kept index -- always a kept index.  temperature = 1 with both filters
 * off gives otvae_categorical_sample's ids bit for bit, for the same u and for the same key.  temperature = 0 and top_k = 1 give the first
 * entry of the order.  -inf logits weigh 0; rows holding NaN or nothing but -inf are outside the contract.  A kept entry of weight 0 (a -inf
 * logit inside the top_k, or an exp that underflows) is never drawn: u = 0 yields the first kept entry of positive weight.  One launch, no
 * host read.
 * OTVAE_EINVAL: temperature < 0 or not finite, top_k < 0, top_p outside (0, 1].  A row is sorted in LDS when top-k or top-p takes effect:
 * OTVAE_EUNSUPPORTED then for K > 16384 (8 bytes per entry of K rounded up to a power of two); temperature alone and greedy decoding
 * take any K. */
int otvae_filtered_sample(const float* logits, int64_t stride_b, int64_t stride_t, int pos, int B, int K, const float* u,
                          const int64_t* key, int64_t* ids, int64_t ids_stride, int T, int col, float temperature, int top_k,
                          float top_p, int32_t* kept, void* stream);
/* The decode of sampled ids (discrete_auto_diffuser.py:92-93: one_hot(ids) @ codebook, B*T*K*d multiply-adds for a row gather):
 * out[n][:] = codebook[ids[n]][:], codebook [K][d], ids [N] int64; an id outside [0, K) yields a NaN row. */
int otvae_codebook_gather(const float* codebook, const int64_t* ids, int64_t N, int K, int d, float* out, void* stream);

/* ---- key/value-cached decoding of the causal AutoRegressive transformer (networks/vit.py:249-260), one new token per row ------------- */
/* One post-norm nn.TransformerEncoderLayer (ReLU, eval mode, causal mask) for the token at position pos of each of B rows, as ONE launch:
 *   qkv = x w_in + b_in (nn.MultiheadAttention's q | k | v split, heads contiguous);  kcache[b][h][pos][:] = k, vcache[b][h][pos][:] = v;
 *   a = softmax(q . kcache[b][h][0..pos][:]^T / sqrt(C)) . vcache[b][h][0..pos][:];  x1 = LayerNorm1(x + a w_out + b_out);
 *   y = LayerNorm2(x1 + relu(x1 w1 + b1) w2 + b2).
 * x, y: [B][D] (y may not alias x).  Weights on [in][out] memory: w_in [D][3D], w_out [D][D], w1 [D][F], w2 [F][D].  LayerNorms: biased
 * variance, eps1 / eps2.  kcache / vcache: fp32 [B][H][Tmax][C], C = D / H, 16-byte aligned; rows 0 .. pos-1 are read, row pos is written,
 * nothing beyond pos is touched.  No atomics: bit-reproducible.
 * OTVAE_EINVAL: null pointers, pos >= Tmax, D % H != 0.  OTVAE_EUNSUPPORTED outside the envelope 16 <= D <= 512 with D % 16 == 0,
 * C % 4 == 0, F <= 4 D, Tmax <= 4096 (the layer's activations of 16 rows stay in LDS: 64 (4 D + 8) bytes). */
int otvae_ar_layer_step(const float* x, int B, int D, int H, int F, int pos, int Tmax, const float* w_in, const float* b_in,
                        const float* w_out, const float* b_out, const float* ln1_g, const float* ln1_b, float eps1, const float* w1,
                        const float* b1, const float* w2, const float* b2, const float* ln2_g, const float* ln2_b, float eps2,
                        float* kcache, float* vcache, float* y, void* stream);
/* The step's input (networks/vit.py:249-260 with PositionalEmbedding, vit.py:33-58, restricted to one position):
 * out[b][:] = LayerNorm(vocab[ids[b * ids_stride]][:] + positions[pos][:]), vocab [V][D], positions [P][D], out [B][D]; an id outside
 * [0, V) yields a NaN row.  ids_stride in elements: a column of an int64 [B][T] matrix is taken in place. */
int otvae_ar_embed_step(const int64_t* ids, int64_t ids_stride, int pos, int B, int D, int V, int P, const float* vocab,
                        const float* positions, const float* ln_g, const float* ln_b, float eps, float* out, void* stream);

/* ---- image transforms around the model ------------------------------------------------------------------------------------------------ */
/* torchvision.transforms.functional.gaussian_blur, the degradation of the reference's latent-transport experiments
 * (tests/test_latent_transport.py:35, tests/test_conditional_vit_vae.py:91-95: GaussianBlur(5, sigma=(1.5, 1.5))): every channel of
 * x [N][C][H][W] is reflect-padded by (kx / 2, ky / 2) without edge repeat (F.pad(mode="reflect")) and correlated with the window
 * wy[ky] x wx[kx].  wx / wy are HOST arrays (they travel in the kernel's argument block): the caller evaluates torchvision's
 * _get_gaussian_kernel1d in fp32.  channels_last = 0: x and y are NCHW-contiguous; 1: both are NHWC memory (the package's layout); the
 * output has the layout of the input, no converted or padded copy is made.  One launch, no atomics; a plane's result does not depend
 * on N or on its place in the batch; kx = ky = 1 with weight 1 returns the input's bits.
 * OTVAE_EINVAL: null pointers, even or non-positive kernel sizes.  OTVAE_EUNSUPPORTED outside the envelope: kx, ky <= 31,
 * kx / 2 < W and ky / 2 < H (what reflect padding itself requires), N * C * H * W < 2^31. */
int otvae_gaussian_blur_fwd(const float* x, int N, int C, int H, int W, int channels_last, int kx, int ky, const float* wx,
                            const float* wy, float* y, void* stream);
/* Its adjoint (what autograd derives from F.pad(mode="reflect") + F.conv2d): per axis, with p = k / 2 and gy extended by zeros,
 * G(m) = sum_t w[t] gy[m + p - t] and gx[i] = G(i) + [1 <= i <= p] G(-i) + [H-1-p <= i <= H-2] G(2 (H-1) - i).  A gather in a fixed
 * order, no atomics.  Arguments and envelope as the forward entry. */
int otvae_gaussian_blur_bwd(const float* gy, int N, int C, int H, int W, int channels_last, int kx, int ky, const float* wx,
                            const float* wy, float* gx, void* stream);
/* Collage.list_to_collage (utils/collage.py:112-121: torch.cat(images, -1).clamp(0, 1), torchvision's make_grid(nrow=1, padding=2,
 * pad_value=0)) without the concatenated temporary: the first n samples of L <= 16 maps [B][C][H][W_l] side by side, clamped to [0, 1],
 * a single channel repeated three times (C' = 3 if C == 1 else C); sample k at row k (H + 2) + 2, column 2 of a zero-bordered
 * [n (H + 2) + 2][sum W_l + 4] grid, or for n == 1 the bare [H][sum W_l] image, as make_grid returns it.
 * maps: HOST array of L device pointers; strides: HOST int64 [L][4], the (sample, channel, row, pixel) strides of each map in elements
 * (any layout is read in place); widths: HOST int [L].  as_uint8 = 0: out is fp32 [C'][OH][OW], what the loggers take; 1: out is
 * uint8 [OH][OW][C'] = trunc(clamp(v * 255 + 0.5, 0, 255)), torchvision.utils.save_image's quantisation. */
int otvae_collage(const float* const* maps, const int64_t* strides, const int* widths, int L, int n, int C, int H, int as_uint8,
                  void* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OTVAE_H */
