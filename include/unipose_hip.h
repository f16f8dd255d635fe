/*
 * unipose_hip.h — C ABI of libunipose_hip.so: hand-written gfx950 (MI355X, CDNA4) kernels for the
 * UniPose / UniPose-LSTM forward+backward hot path.
 *
 * The reference (bmartacho/UniPose) has NO native / FFI layer: its arithmetic is PyTorch ATen ops
 * reached from Python nn.Modules.  Each entry point below therefore cites the
 * reference call site(s) whose ATen op it replaces (paths relative to the reference tree).  The
 * Python binding a maintainer adds is the ctypes table in unipose_amd/_C.py.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (fp32 unless stated), borrowed for the call, never freed;
 *   - activations are NHWC ("pixel-major"): element (n,h,w,c) of a tensor with pixel stride `ld`
 *     lives at ((n*H + h)*W + w)*ld + c; ld >= C lets a producer write into a channel slice of a
 *     wider buffer (this is how torch.cat is eliminated: wasp.py:84, decoder.py:51);
 *   - channel counts seen by the convolution kernels are padded to a multiple of 4 (`Cp`), pad
 *     channels hold zeros; pixel strides and base pointers are multiples of 4 floats (16 B);
 *   - `stream` is a hipStream_t (as void*); all work is enqueued asynchronously on it;
 *   - return value: 0 on success, negative up_status on failure; up_last_error() gives the text.
 *     No C++ exception crosses this boundary.
 *   - host-side global state: the per-thread error string; the development knobs of up_conv_tune (and the UP_* environment
 *     variables read at load time), which select kernels process-wide; per-stream K-split scratch (up_stream_release) and
 *     per-geometry device tables (tap-sort permutations, weight-gradient rectangles) allocated on first use and kept.
 */
#ifndef UNIPOSE_HIP_H
#define UNIPOSE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    UP_OK = 0,
    UP_ERR_INVALID = -1,     /* bad argument (shape, alignment, null pointer) */
    UP_ERR_UNSUPPORTED = -2, /* configuration this library does not implement */
    UP_ERR_LAUNCH = -3,      /* HIP launch / runtime error */
    UP_ERR_WORKSPACE = -4    /* caller-provided workspace too small */
} up_status;

const char* up_last_error(void);
int up_abi_version(void);   /* 10; the revision that added the up_clip_* layout kernels and the up_unipose_lstm_* video entry
                               points kept it at 10: the additions are purely additive */

/* Geometry of one 2-D convolution (nn.Conv2d as used at resnet.py:10-16,61,80-84,104-109;
 * wasp.py:9,52,59-60; decoder.py:17,22,26,30; model/uniposeLSTM.py:12-14,30-38,85-89).
 * Any stride >= 1, dil >= 1, pad >= 0 and rectangular filters are accepted as long as P, Q follow from them and the
 * output is not empty: a filter extent dil * (R - 1) + 1 (or the S one) larger than the padded input H + 2 * pad
 * (W + 2 * pad) has no output pixel: every launching entry (up_pack_weights, up_conv2d_fwd*, up_conv2d_bwd_data*,
 * up_conv2d_bwd_weight*) refuses it with UP_ERR_INVALID; the informational queries either do not validate the
 * descriptor (up_conv_stats_tiles*) or answer 0 / UP_ERR_INVALID for it. */
typedef struct {
    int32_t N, H, W;      /* input batch / height / width                                   */
    int32_t C, Cp;        /* real input channels, padded input channels (Cp%4==0, Cp>=C)    */
    int32_t ldx;          /* input pixel stride in floats (>= Cp, %4==0)                     */
    int32_t K;            /* output channels                                                 */
    int32_t R, S;         /* kernel height / width                                           */
    int32_t stride, pad, dil;
    int32_t P, Q;         /* output height / width                                           */
    int32_t ldy;          /* output pixel stride in floats (>= K)                            */
    int32_t Kp;           /* padded output channels for the dgrad weight image (Kp%4==0)     */
} up_conv_desc;

/* Fused epilogue of the forward convolution (all optional, applied in this order):
 *   v = acc;  if(scale) v = v*scale[k] + shift[k];   (folded eval-mode BatchNorm, K7)
 *   if(bias) v += bias[k];  if(residual) v += residual[pixel*ldr + k];  if(relu) v = max(v,0)
 * `stats` != NULL asks for per-(row-tile, channel) Welford partials {count, mean, M2} of the RAW
 * accumulator (train-mode BatchNorm statistics, K7).  A call that passes `stats` TOGETHER with scale, bias, residual or relu
 * is refused with UP_ERR_INVALID and launches nothing (the statistics are not "taken before" such an epilogue: the
 * combination does not exist).  In bf16 storage the partials come from the fp32 accumulators, not from the rounded y.
 * Also refused with UP_ERR_INVALID before any launch: scale without shift; a residual with ldr < K; `fold` without `stats`
 * (or without gamma / beta / its four outputs, or with only one of the running statistics); UP_MATH_BF16S_F32OUT with a
 * residual or with stats.  Of every output pixel only lanes [0, K) are written (in bf16 storage at most up to the next
 * multiple of 32): the lanes behind them, up to ldy, keep what they held. */
/* ABI 10: BatchNorm finalize FOLDED into the launch that writes `stats`.  Every workgroup takes a ticket after publishing its
 * partial row; the last arriver merges the partials in a fixed order (deterministic; the same bits as up_bn_finalize on the same
 * stats) and writes mean / invstd / scale / shift (+ the running-statistics update) — no up_bn_finalize launch on the critical
 * path.  `folded` is set by the call: 1 = done by the launch, 0 = the caller runs up_bn_finalize (row groups, fold switched off
 * with up_conv_tune("bn_fold", 0), scratch exhausted).  Scratch (tickets + level-1 rows, ~8 MB) is per stream, like the K-split's. */
typedef struct {
    float eps, momentum;
    float* running_mean;   /* optional pair, updated in place */
    float* running_var;
    const float* gamma;
    const float* beta;
    float* mean;           /* out [K] */
    float* invstd;
    float* scale;
    float* shift;
    int32_t folded;        /* out */
} up_bn_fold;
typedef struct {
    const float* scale;
    const float* shift;
    const float* bias;
    const float* residual;
    int32_t ldr;
    int32_t relu;
    float* stats;         /* [up_conv_stats_tiles(desc)][K][3] or NULL */
    up_bn_fold* fold;     /* optional (ABI 10, needs stats): see above */
} up_conv_epilogue;

/* Re-lay an OIHW fp32 weight (PyTorch layout) for the implicit-GEMM kernels:
 *   w_fwd  [K][R*S][Cp]  (forward, B operand rows = output channel, k-contiguous)
 *   w_dgrad[C ][R*S][Kp] (data-gradient: rows = input channel)           — either may be NULL.
 * The data-gradient image is opaque: for stride-2, dilation-1 convolutions it holds four parity-class sub-images
 * (same total size); only up_conv2d_bwd_data with the SAME descriptor may read it. */
int up_pack_weights(const up_conv_desc* d, const float* w_oihw, float* w_fwd, float* w_dgrad, void* stream);
/* The same for many parameters in ONE launch (every weight changes once per optimizer step): `jobs` is a table in
 * DEVICE memory; w_fwd / w_dgrad may be NULL per job. */
typedef struct {
    const float* w;        /* OIHW */
    float* w_fwd;
    float* w_dgrad;
    int32_t K, C, Cp, Kp, taps;
    int32_t geometry;      /* stride | R << 4 | S << 10 | pad << 16 | dilation << 24: selects the data-gradient image layout
                              (stride-2 convolutions use a parity-class-major one, like up_pack_weights does) */
} up_pack_job;
int up_pack_weights_batched(const up_pack_job* jobs_device, int njobs, void* stream);

/* Forward convolution, implicit GEMM on v_mfma_f32_32x32x2_f32 (replaces aten::convolution, K1-K6,K17). */
int up_conv2d_fwd(const up_conv_desc* d, const float* x, const float* w_fwd, float* y,
                  const up_conv_epilogue* ep, void* stream);
int up_conv_stats_tiles(const up_conv_desc* d);   /* row tiles the fp32 forward kernel will use */
int up_conv_stats_tiles_math(const up_conv_desc* d, int math);   /* ... the forward kernel of arithmetic `math` (up_math) */
/* Load balance: when the tile count leaves a short tail (tiles % CUs small), the forward / data-gradient launch splits
 * each tail tile along K into this many parts (1 = no split), one per CU, and merges them in a fixed order through a
 * per-stream scratch the library allocates on first use (one 128x128 fp32 partial per CU: 16 MB + flags).  UP_TAIL_SPLIT=0 disables it.  Informational. */
int up_conv_split_parts(const up_conv_desc* d);
/* Frees the per-stream scratch of a stream the caller retires (no launch or captured graph of that stream may run afterwards);
 * a stream that never ran a split launch has none: no-op. */
int up_stream_release(void* stream);
/* ABI 10, experiment support: a HIP stream whose kernels run only on the compute units named by `mask` (bit i of `words` 32-bit
 * words = logical CU i; hipExtStreamCreateWithCUMask) — the weight-gradient side stream on a fixed share of the chip
 * (UNIPOSE_SIDE_CUS, profiles/r06_experiments.txt) — and a probe that reports where the workgroups of a stream run:
 * out[blocks][2] = (XCC id, CU | SH << 4 | SE << 5 of HW_ID), device memory. */
int up_stream_create_cu_mask(const uint32_t* mask, int words, void** stream);
int up_stream_destroy(void* stream);
int up_probe_placement(int blocks, int* out_device, void* stream);
/* Development knobs (A/B runs inside one process; each also has an environment variable read at load time).  Twelve keys + five of round 6
 * (round 4 removed the ones whose question is settled: short_k, short_k_mult, db_min_k, wgrad_per_cu, tap_skip, lds_swz and
 * the bf16 forms that lost in round 3):
 * "tiny_k" (UP_TINY_K, round 5: fp32 reductions of at most this length always take 64x64 tiles; default 128),
 * "tile_want" (UP_TILE_WANT; "tile_want_bf16" for the plain-bf16 kernels) workgroups a launch should at least have when the tile
 * size is chosen, "tail_split" (UP_TAIL_SPLIT), "split_per_cu" (UP_SPLIT_PER_CU: launches with fewer tiles than CUs split every tile
 * along K up to this many workgroups per CU), "tap_sort" (UP_TAP_SORT: GEMM rows ordered by their set of live filter taps so that
 * the tile-level tap skipping becomes near exact), "wgrad_rect" (UP_WGRAD_RECT, see up_conv_wgrad_visits).
 * bf16 storage: "glds" (UP_GLDS: direct-to-LDS kernels of bf16s_glds.h, default 1; 0 = the register-staged kernels), "bn_rows"
 * (row-strided BatchNorm kernels).  Round 6, the 8-wave (32 TM) x 256 tiles of bf16s_big.h: "glds_big" (UP_GLDS_BIG, default 1: launches
 * with N % 256 == 0, 64-aligned channels and a reduction of at least "big_min_k" (UP_BIG_MIN_K, 1024) run on igemm_big_kernel),
 * "big_stages" (UP_BIG_STAGES: LDS stages of the 160-row tiles, 3 | 2), "big_rows" (UP_BIG_ROWS: 0 = rows per tile by the fill
 * rule, else only 160 / 192 / 256), "big_dgrad" (UP_BIG_DGRAD: 0 keeps data gradients on igemm_glds_kernel); "stem7" (UP_STEM7, default 0:
 * the 7x7 stride-2 first convolution on stem7_kernel of stem_f32.h — equal bits, faster alone, not faster inside the step).  fp32 (round 4): "glds32" (UP_GLDS32: forward / data gradient on f32_glds.h, default 1),
 * "glds32_epi" (LDS-transposed 16-byte-store epilogue, 1), "glds32_wgrad" (weight gradient on f32_glds.h, 1).  "cu_count" (tests: pretend the chip has this many CUs when planning
 * splits; 0 = the real count).
 * These knobs and the UP_* environment variables they mirror are PROCESS-GLOBAL host state (kernel selection of every later
 * launch on every stream), like the library's per-stream K-split scratch and per-geometry tables; see the note at the top.
 * Change them only between steps: workspace sizes and the BatchNorm partial-row count follow the tile choice. */
int up_conv_tune(const char* key, int value);
/* Diagnostics: fp32 forward / data-gradient launches since load, by kernel family ("big": bf16-storage launches on igemm_big_kernel) — "igemm" (register-staged igemm_kernel),
 * "glds32" (f32_glds.h), "glds32_epi1" (of those, with the LDS-transposed epilogue), "glds32_bnred" (with the fused
 * BatchNorm-backward reduction), "wgrad_glds32" / "wgrad_glds32_st1" (fp32 weight-gradient launches on the direct-to-LDS kernel /
 * of those, the one-stage form), "wgrad_rect" (weight-gradient launches of any family that ran with a live-rectangle table),
 * "wgrad_st1" (register-staged fp32 weight-gradient launches on the one-stage form); two names are not counts but describe the most
 * recent weight-gradient launch: "wgrad_splits" (its pixel splits) and "wgrad_variant" (its index for up_profile_variant_name: kernel
 * family and tile pair, also where nothing is profiled; -1 before the first launch); -1 for an unknown name.  Tests use it to prove which kernel a case ran on. */
long long up_conv_counter(const char* name);
/* Analysis (host only, no launch): share of (row tile, filter tap) pairs the K loop of the forward (data_gradient = 0) or
 * data-gradient launch of `d` visits with its rows in image order and in tap-sorted order ("tap_sort" knob), and the share
 * of (pixel, tap) pairs that touch the image at all (`live`: what a perfect skip would visit).  Aligned fast path only. */
int up_conv_tap_visits(const up_conv_desc* d, int data_gradient, double* image_order, double* tap_sorted, double* live);
/* The same for the weight gradient with the "wgrad_rect" knob (UP_WGRAD_RECT, default off until measured): each column
 * tile of the weight-gradient GEMM reduces over the bounding rectangle of the output pixels on which its filter taps read
 * real input (instead of all N*P*Q pixels); *rect_fraction = share of (pixel, column tile) pairs still visited. */
int up_conv_wgrad_visits(const up_conv_desc* d, double* rect_fraction);

/* Data gradient: dx[N,H,W,ldx(:Cp)] from dy[N,P,Q,ldy(:K)] (replaces convolution_backward, input half).
 * Writes all Cp channels of every input pixel (pad channels get 0).  `add` (optional, [N,H,W,ld_add]) is a second
 * gradient of the same input — the identity branch of a residual block, resnet.py:36-40 — summed in the epilogue
 * instead of by a separate add kernel. */
int up_conv2d_bwd_data(const up_conv_desc* d, const float* dy, const float* w_dgrad, float* dx,
                       const float* add, int ld_add, void* stream);
/* Extended data-gradient epilogue (round 4; fp32 and bf16 storage).  Two things a residual network's backward otherwise pays
 * separate full-tensor passes for (resnet.py:25-42):
 *  - `bn`: dx is dz of the layer z = relu(bn(y) (+ res)) that produced this convolution's input (bn1 -> relu -> conv2,
 *    bn2 -> relu -> conv3, a block's output -> the next identity block's conv1): the launch also reduces that layer's two
 *    BatchNorm-backward sums per row tile — partial[tile][c] = {sum g, invstd[c] * sum g * (y - mean[c])}, g = dz * [z > 0] —
 *    so the layer's backward (up_bn_bwd_prereduced_t) needs no reduction pass (native_batch_norm_backward's first read of dz, y);
 *  - `add_relu_bits`: the addend (the skip-connection gradient, resnet.py:36-40) is the UNMASKED dz of the block's last layer
 *    and its ReLU mask is applied here (bit row * C + c of that layer's sign bits), so that layer's backward need not write
 *    dz * [z > 0] as a tensor of its own (threshold_backward's output).
 * up_conv2d_bwd_data_tiles_math(d, math) = rows of `partial`, and > 0 exactly when the launch of `d` runs on a kernel that
 * supports the two extras (math = UP_MATH_F32 or UP_MATH_BF16S); with 0 use the plain entry points (add only).
 * Both sums are taken on the STORED dx (in bf16 storage: after the rounding to bf16, also where an addend joined in fp32), like a
 * separate reduction pass that reads dx back.  Refused before any launch: add_relu_bits without add, dgamma without dbeta (or the
 * reverse), bn->C != d->C or bn->ld < d->C (UP_ERR_INVALID); a slot or add_relu_bits where up_conv2d_bwd_data_tiles_math is 0
 * (stride 2, Kp % 32 != 0, more than 32 taps), groups > 1 with UP_MATH_BF16S or where up_conv2d_bwd_data_tiles_grouped is 0
 * (UP_ERR_UNSUPPORTED).  With bn_fold switched off, or groups > 1 and gsum == NULL, dgamma / dbeta / gsum are not written. */
/* Row groups (ABI 8): `groups` equal batches stacked along N that must keep separate BatchNorm statistics (the frames of the video
 * model's batched trunk).  Every group is tiled on its own, so no row tile straddles two groups and stats is
 * [groups][up_conv_stats_tiles_grouped(d, groups)][K][3] — the layout up_bn_finalize_groups merges; no extra pass over y
 * (up_bn_batch_stats_t) is needed.  fp32 only, direct-to-LDS kernel with the LDS-transposed epilogue: up_conv_stats_tiles_grouped
 * returns 0 and up_conv2d_fwd_grouped UP_ERR_UNSUPPORTED (nothing launched) otherwise. */
/* ABI 10 (row groups): the statistics pass and the finalize as one launch where the fold applies (else the two launches);
 * and the grouped backward whose sums the data gradient already merged (up_bn_reduce_slot.gsum, folded = 1): the apply pass alone. */
int up_bn_stats_groups_t(const void* y, int ldy, int64_t rows_per_group, int C, int groups, int dtype, float* stats, float eps,
                         float momentum, float* running_mean, float* running_var, const float* gamma, const float* beta, float* coef,
                         void* stream);
int up_bn_bwd_groups_finalized_t(const void* dz, int lddz, const uint32_t* relu_bits, const void* y, int ldy, const float* gamma,
                                 const float* coef, int relu, void* dy, int lddy, void* dres, int lddres, const float* gsum,
                                 int64_t rows_per_group, int C, int groups, int dtype, void* stream);
int up_bn_bwd_groups_prereduced_ok(int64_t rows_per_group, int C, int groups, int ld);
int up_bn_bwd_groups_prereduced_t(const void* dz, int lddz, const uint32_t* relu_bits, const void* y, int ldy, const float* gamma,
                                  const float* coef, int relu, void* dy, int lddy, void* dres, int lddres, float* dgamma, float* dbeta,
                                  float* workspace, size_t workspace_bytes, const float* partial, int tiles, int64_t rows_per_group,
                                  int C, int groups, int dtype, void* stream);
int up_conv_stats_tiles_grouped(const up_conv_desc* d, int groups);
int up_conv2d_fwd_grouped(const up_conv_desc* d, const float* x, const float* w_fwd, float* y, float* stats, int groups, void* stream);

typedef struct {
    const void* y;             /* raw convolution output of the producing layer, [rows][ld] (element type of dx)  */
    const uint32_t* relu_bits; /* sign bits of z (bit row * C + c), NULL when the layer has no ReLU               */
    const float* mean;         /* [C] batch (or running) mean / 1 / sqrt(var + eps) of that BatchNorm              */
    const float* invstd;
    float* partial;            /* out: [up_conv2d_bwd_data_tiles_math(d, math)][C][2]                               */
    int32_t ld, C;             /* pixel stride of y; channels (== d->C of this convolution)                        */
    int32_t group_stride;      /* row groups (ABI 8): floats between two groups' mean / invstd vectors, else 0     */
    float* dgamma;             /* ABI 10, optional pair: the launch also FINISHES the reduction (last-arriver ticket, see      */
    float* dbeta;              /* up_bn_fold): [C] sums over all rows; then up_bn_bwd_finalized_t runs the apply pass alone   */
    float* gsum;               /* row groups (ep->groups > 1): [groups][dgamma | dbeta][C], every group's own sums (its data     */
                               /* gradient needs them: up_bn_bwd_groups_finalized_t); NULL: a grouped launch does not fold        */
    int32_t folded;            /* out: 1 = dgamma / dbeta (/ gsum) are final; 0 = call up_bn_bwd_(groups_)prereduced_t on `partial` */
} up_bn_reduce_slot;
typedef struct {
    const void* add;               /* second gradient of the same input (element type of dx), or NULL              */
    const uint32_t* add_relu_bits; /* optional ReLU mask of the addend, see above                                   */
    up_bn_reduce_slot* bn;         /* optional fused BatchNorm-backward reduction                                   */
    int32_t ld_add;
    int32_t groups;                /* row groups (ABI 8; 0 / 1: none): the N images are `groups` equal batches, every one tiled
                                      on its own; bn->partial is then [groups][up_conv2d_bwd_data_tiles_grouped][C][2] and
                                      bn->mean / invstd are per group (group_stride).  fp32 only.                       */
} up_dgrad_epilogue;
int up_conv2d_bwd_data_tiles_grouped(const up_conv_desc* d, int groups);   /* tiles per group, 0: not supported */
int up_conv2d_bwd_data_tiles(const up_conv_desc* d);                 /* = ..._tiles_math(d, UP_MATH_F32) */
int up_conv2d_bwd_data_tiles_math(const up_conv_desc* d, int math);
/* w_dgrad: the fp32 data-gradient image of up_pack_weights (math = UP_MATH_F32) or the bf16 `hi` plane of
 * up_pack_weights_bf16 (UP_MATH_BF16S: dy, dx, add and bn->y are bf16). */
int up_conv2d_bwd_data_ex(const up_conv_desc* d, const void* dy, const void* w_dgrad, void* dx, const up_dgrad_epilogue* ep,
                          int math, void* stream);

/* bf16-operand variants of the forward / data-gradient convolution (v_mfma_f32_32x32x16_bf16, fp32 accumulate,
 * fp32 activations in HBM).  math = UP_MATH_BF16X3: every operand is carried as hi = bf16(x), lo = bf16(x - hi)
 * and a*b ~= ah*bh + ah*bl + al*bh (fp32-equivalent, relative error 2^-16 per product);  UP_MATH_BF16: plain bf16
 * operands (BASELINE config 5 arithmetic).  Weights come as bf16 planes made by up_pack_weights_bf16 in the
 * [rows][R*S][padded channels] order of up_pack_weights.  Requires the padded reduction channel count (Cp forward,
 * Kp backward) to be a multiple of 32; otherwise UP_ERR_UNSUPPORTED (use the fp32 entry points). */
typedef enum { UP_MATH_F32 = 0, UP_MATH_BF16X3 = 1, UP_MATH_BF16 = 2, UP_MATH_BF16S = 3, UP_MATH_BF16S_F32OUT = 4 } up_math;
int up_pack_weights_bf16(const up_conv_desc* d, const float* w_oihw, uint16_t* fwd_hi, uint16_t* fwd_lo,
                         uint16_t* dgrad_hi, uint16_t* dgrad_lo, void* stream);
/* The same for many parameters in ONE launch (ABI 9; like up_pack_weights_batched: an optimizer step changes every weight, and
 * 2 x 115 separate 5-us launches per step cost more than the packing itself).  `jobs` is a table in DEVICE memory; the
 * fwd / dgrad plane pairs may be NULL per job, and so may the lo plane of a pair alone (only UP_MATH_BF16X3 reads lo planes). */
typedef struct {
    const float* w;        /* OIHW */
    uint16_t* fwd_hi;
    uint16_t* fwd_lo;
    uint16_t* dgrad_hi;
    uint16_t* dgrad_lo;
    int32_t K, C, Cp, Kp, taps, reserved;
} up_pack_job_bf16;
int up_pack_weights_bf16_batched(const up_pack_job_bf16* jobs_device, int njobs, void* stream);
int up_conv2d_fwd_bf16(const up_conv_desc* d, const float* x, const uint16_t* w_hi, const uint16_t* w_lo, float* y,
                       const up_conv_epilogue* ep, int math, void* stream);
int up_conv2d_bwd_data_bf16(const up_conv_desc* d, const float* dy, const uint16_t* w_hi, const uint16_t* w_lo,
                            float* dx, const float* add, int ld_add, int math, void* stream);

/* Weight gradient into PyTorch OIHW layout (replaces convolution_backward, weight half); `dbias`
 * (K floats) may be NULL.  Split-K partial slabs live in the caller-provided workspace. */
size_t up_conv2d_bwd_weight_workspace(const up_conv_desc* d);
int up_conv2d_bwd_weight(const up_conv_desc* d, const float* x, const float* dy, float* dw_oihw,
                         float* dbias, void* workspace, size_t workspace_bytes, void* stream);
/* The same on v_mfma_f32_32x32x16_bf16 (BASELINE configs[4] arithmetic: operands rounded to bf16 while they are staged,
 * fp32 accumulation, fp32 split-K slabs and result; same workspace).  Falls back to the fp32 kernel for tensors of more
 * than 2^31 elements. */
int up_conv2d_bwd_weight_bf16(const up_conv_desc* d, const float* x, const float* dy, float* dw_oihw,
                              float* dbias, void* workspace, size_t workspace_bytes, void* stream);

/* ---- bf16 STORAGE (BASELINE configs[4]: "bf16, 736x736, batch 16/GPU") -------------------------------------------------
 * Activations and activation gradients live in HBM as bf16 (raw 16-bit patterns, NHWC, channel counts and pixel strides
 * multiples of 8 = 16-byte channel groups; convolution outputs are padded to multiples of 32 channels so that every
 * reduction is a whole number of 32-wide K slices); all arithmetic is fp32 (BatchNorm statistics, accumulators) or
 * bf16 MFMA with fp32 accumulation; weights, weight gradients, BatchNorm parameters and the optimizer stay fp32.
 *   - convolutions: up_conv2d_fwd_bf16 / up_conv2d_bwd_data_bf16 with math = UP_MATH_BF16S — x / y / residual / add are
 *     then bf16 tensors passed through the same pointer arguments; up_conv2d_bwd_weight_bf16s below.  up_conv2d_fwd_bf16 also
 *     takes math = UP_MATH_BF16S_F32OUT: bf16 x, fp32 y (no residual / statistics) — the network's LAST convolution
 *     (decoder.py:30), so that the heat-maps and the bilinear up-sampling behind them (model/unipose.py:31-32) are not
 *     rounded to 8-bit mantissas;
 *   - every streaming operator has a `_t` twin taking the element type of its activation tensors (UP_DT_F32 / UP_DT_BF16);
 *     the fp32 entry points above are the `_t` forms with UP_DT_F32.  The max-pool takes two types: it is where the
 *     network leaves the fp32 stem (fp32 in, bf16 out; its backward bf16 in, fp32 out). */
enum { UP_DT_F32 = 0, UP_DT_BF16 = 1 };
int up_conv2d_bwd_weight_bf16s(const up_conv_desc* d, const void* x_bf16, const void* dy_bf16, float* dw_oihw,
                               float* dbias, void* workspace, size_t workspace_bytes, void* stream);

/* The three weight-gradient entry points above behind one signature, plus accumulation: `math` = UP_MATH_F32 (fp32 tensors,
 * fp32 MFMA), UP_MATH_BF16 (fp32 tensors, bf16 operands) or UP_MATH_BF16S (bf16 tensors); accumulate != 0 ADDS the result to
 * dw_oihw / dbias instead of overwriting them (dw += sum of the split-K slabs, in one rounding step like a separate add).
 * A weight that is used several times per backward pass — every weight of the video model, once per frame
 * (uniposeLSTM.py:116-133) — is then summed by the reduce pass itself: no extra buffer, no add kernel per use. */
int up_conv2d_bwd_weight_acc(const up_conv_desc* d, const void* x, const void* dy, float* dw_oihw, float* dbias,
                             void* workspace, size_t workspace_bytes, int math, int accumulate, void* stream);

/* ---- BatchNorm (nn.BatchNorm2d, K7; every bnX site, e.g. resnet.py:11,14,16; wasp.py:11,53,61) ---- */
/* eval: scale = g/sqrt(rv+eps), shift = b - rm*scale */
int up_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean,
                      const float* running_var, float eps, int C, float* scale, float* shift, void* stream);
/* train: merge the conv epilogue partials -> batch mean / invstd, update running stats in place
 * (momentum, unbiased variance), emit scale/shift for up_bn_apply and mean/invstd for backward. */
int up_bn_finalize(const float* stats, int tiles, int C, float eps, float momentum,
                   float* running_mean, float* running_var,
                   const float* gamma, const float* beta,
                   float* mean, float* invstd, float* scale, float* shift, void* stream);
/* z = relu?(y*scale[c] + shift[c] (+ residual)).  relu_bits (optional, (rows*C + 31)/32 words): dense bit array,
 * bit row*C + c = (z > 0) — the backward passes read it instead of z (1/32 of the bytes). */
int up_bn_apply(const float* y, int ldy, const float* scale, const float* shift,
                const float* residual, int ldr, int relu, float* z, int ldz, uint32_t* relu_bits,
                int64_t rows, int C, void* stream);
/* backward of z = relu?(bn(y) (+res)):  g = dz * (z>0 if relu);  dgamma = sum g*xhat, dbeta = sum g,
 * dy = gamma*invstd*(g - dbeta/M - xhat*dgamma/M)  (train)   or   gamma*invstd*g (eval: use_batch_stats=0);
 * dres (optional) = g.  The ReLU mask comes from relu_bits when given (z may then be NULL), else from z. */
int up_bn_bwd(const float* dz, int lddz, const float* z, int ldz, const uint32_t* relu_bits,
              const float* y, int ldy,
              const float* gamma, const float* mean, const float* invstd, int relu, int use_batch_stats,
              float* dy, int lddy, float* dres, int lddres, float* dgamma, float* dbeta,
              float* workspace, size_t workspace_bytes, int64_t rows, int C, void* stream);
size_t up_bn_bwd_workspace(int64_t rows, int C);
int up_bn_apply_t(const void* y, int ldy, const float* scale, const float* shift, const void* residual, int ldr,
                  int relu, void* z, int ldz, uint32_t* relu_bits, int64_t rows, int C, int dtype, void* stream);
/* The same pass in the CENTRED form ATen evaluates (native_batch_norm: (x - mean) * invstd * weight + bias):
 * z = relu?((y - mean[c]) * scale[c] + beta[c] (+ residual)), scale = gamma * invstd from up_bn_finalize, beta = the BatchNorm bias.
 * y * scale + (beta - mean * scale) rounds the product mean * scale: an absolute error of 2^-24 |mean| * scale on z, i.e. a relative
 * |mean| / std ulps — 364 ulps for the reference's BatchNorm behind the global-average-pool branch (wasp.py:53: four samples per
 * channel at B = 4), enough to flip ReLU decisions the reference does not flip: the WASP gradients of G14 moved from 2.7x to within
 * the reference's own fp32-vs-fp64 distance with this form.  ABI version 6. */
int up_bn_apply_centered_t(const void* y, int ldy, const float* mean, const float* scale, const float* beta, const void* residual,
                           int ldr, int relu, void* z, int ldz, uint32_t* relu_bits, int64_t rows, int C, int dtype, void* stream);
int up_bn_bwd_t(const void* dz, int lddz, const void* z, int ldz, const uint32_t* relu_bits, const void* y, int ldy,
                const float* gamma, const float* mean, const float* invstd, int relu, int use_batch_stats,
                void* dy, int lddy, void* dres, int lddres, float* dgamma, float* dbeta,
                float* workspace, size_t workspace_bytes, int64_t rows, int C, int dtype, void* stream);
/* ... and with running sums over several calls: acc_dgamma[c] += this call's dgamma[c] (likewise dbeta), for a BatchNorm that
 * runs once per frame of the video unroll (uniposeLSTM.py:116-133); dgamma / dbeta still receive this call's sums. */
int up_bn_bwd_acc_t(const void* dz, int lddz, const void* z, int ldz, const uint32_t* relu_bits, const void* y, int ldy,
                const float* gamma, const float* mean, const float* invstd, int relu, int use_batch_stats,
                void* dy, int lddy, void* dres, int lddres, float* dgamma, float* dbeta, float* acc_dgamma, float* acc_dbeta,
                float* workspace, size_t workspace_bytes, int64_t rows, int C, int dtype, void* stream);
/* BatchNorm backward whose reduction pass ran inside the data-gradient launch that produced dz (up_conv2d_bwd_data_ex):
 * `partial` = that launch's [chunks][C][2] sums; finalize + apply only. */
int up_bn_bwd_prereduced_t(const void* dz, int lddz, const uint32_t* relu_bits, const void* y, int ldy, const float* gamma,
                           const float* mean, const float* invstd, int relu, int use_batch_stats, void* dy, int lddy, void* dres,
                           int lddres, float* dgamma, float* dbeta, float* acc_dgamma, float* acc_dbeta, float* partial, int chunks,
                           int64_t rows, int C, int dtype, void* stream);
/* ABI 10: ... and when that launch also carried the merge (up_bn_reduce_slot.dgamma / dbeta, folded = 1): dgamma / dbeta are
 * final, the apply pass alone (bn_bwd_apply of native_batch_norm_backward). */
int up_bn_bwd_finalized_t(const void* dz, int lddz, const uint32_t* relu_bits, const void* y, int ldy, const float* gamma,
                          const float* mean, const float* invstd, int relu, int use_batch_stats, void* dy, int lddy, void* dres,
                          int lddres, const float* dgamma, const float* dbeta, int64_t rows, int C, int dtype, void* stream);

/* ---- grouped BatchNorm: one tensor holds `groups` row groups of equal size (the T frames of a clip batch, frame-major), each
 * normalised with ITS OWN batch statistics — what `groups` separate module calls do in the reference's video loop
 * (uniposeLSTM.py:116-133 runs the trunk once per frame), while every convolution sees one T-times larger batch.
 *   up_bn_batch_stats_t      partial (count, mean, M2) per (group, 256-row chunk, channel): stats[groups][tiles][C][3]
 *   up_bn_finalize_groups    coef[groups][4][C] = mean, invstd, scale, shift; running statistics updated group by group
 *   up_bn_apply_groups_t     z = relu((y - mean_g) * scale_g + beta (+ res)) per group (beta = NULL: y * scale_g + shift_g), relu_bits
 *                            as in up_bn_apply
 *   up_bn_bwd_groups_t       data gradient per group from that group's sums; dgamma / dbeta = sums over all groups */
/* Statistics of SMALL batches (<= 4096 rows per group), float64 two-pass, one tile per group: stats[groups][1][C][3] for
 * up_bn_finalize (tiles = 1) / up_bn_finalize_groups.  The host side uses it below 256 rows per channel — the BatchNorm behind the
 * global-average-pool branch (wasp.py:53), B rows — where the mean must be the correctly rounded one (see the kernel). */
int up_bn_exact_stats_t(const void* y, int ldy, int64_t rows_per_group, int C, int groups, int dtype, float* stats, void* stream);
int up_bn_batch_stats_tiles(int64_t rows_per_group);
int up_bn_batch_stats_t(const void* y, int ldy, int64_t rows_per_group, int C, int groups, int dtype, float* stats, void* stream);
int up_bn_finalize_groups(const float* stats, int tiles, int C, int groups, int64_t rows_per_group, float eps, float momentum,
                          float* running_mean, float* running_var, const float* gamma, const float* beta, float* coef,
                          void* stream);
int up_bn_apply_groups_t(const void* y, int ldy, const float* coef, const float* beta, const void* res, int ldr, int relu, void* z,
                         int ldz, uint32_t* relu_bits, int64_t rows_per_group, int C, int groups, int dtype, void* stream);
size_t up_bn_bwd_groups_workspace(int64_t rows_per_group, int C, int groups);
int up_bn_bwd_groups_t(const void* dz, int lddz, const uint32_t* relu_bits, const void* y, int ldy, const float* gamma,
                       const float* coef, int relu, void* dy, int lddy, void* dres, int lddres, float* dgamma, float* dbeta,
                       float* workspace, size_t workspace_bytes, int64_t rows_per_group, int C, int groups, int dtype,
                       void* stream);

/* ---- pointwise / data movement ---- */
int up_relu_bwd(const float* dz, const float* z, float* dx, int64_t n, void* stream);              /* K8 */
int up_copy2d(const float* src, int lds, float* dst, int ldd, int64_t rows, int C, void* stream);   /* K13 */
int up_add2d(const float* a, int lda, const float* b, int ldb, float* dst, int ldd, int64_t rows, int C, void* stream);
int up_nchw_to_nhwc(const float* x, float* y, int N, int C, int H, int W, int ldy, void* stream);   /* boundary */
int up_nhwc_to_nchw(const float* x, int ldx, float* y, int N, int C, int H, int W, void* stream);
/* nn.MaxPool2d(3,2,1) (resnet.py:65, decoder.py:33): idx (uint8, 0..8 = window tap of the first max). */
int up_maxpool3s2_fwd(const float* x, int ldx, float* y, int ldy, uint8_t* idx,
                      int N, int H, int W, int C, int P, int Q, void* stream);
int up_maxpool3s2_bwd(const float* dy, int lddy, const uint8_t* idx, float* dx, int lddx,
                      int N, int H, int W, int C, int P, int Q, void* stream);
/* F.interpolate(mode='bilinear', align_corners=True) (wasp.py:83, decoder.py:49, model/unipose.py:32) */
int up_bilinear_fwd(const float* x, int ldx, float* y, int ldy, int N, int H, int W, int C, int P, int Q, void* stream);
int up_bilinear_bwd(const float* dy, int lddy, float* dx, int lddx, int N, int H, int W, int C, int P, int Q, void* stream);
/* nn.AdaptiveAvgPool2d(1) (wasp.py:51) */
int up_gap_fwd(const float* x, int ldx, float* y, int N, int HW, int C, void* stream);
int up_gap_bwd(const float* dy, float* dx, int lddx, int N, int HW, int C, void* stream);
/* nn.AvgPool2d(9,8,1) on the 1-channel centre map (model/uniposeLSTM.py:75,114); NCHW(1ch) in,
 * writes channel `coff` of an NHWC buffer with pixel stride ldy */
int up_avgpool9s8_fwd(const float* x, float* y, int ldy, int coff, int N, int H, int W, int P, int Q, void* stream);
/* Clip layout (ABI 10 additions, the video plan below): a clip is batch-major, (B, T, ...); the trunk and the head of the video
 * network run frame-major, on T * B images, image f = t * B + b.  Data movement only (the pooling is avgpool9s8's arithmetic):
 *   up_clip_nchw_to_nhwc    x (B, T, C, H, W) -> y frame-major (T * B, H, W, ldy), pad channels C <= c < ldy zero
 *   up_clip_avgpool9s8_fwd  AvgPool2d(9,8,1) of the (B, T, 1, H, W) centre maps into channel coff of the frame-major
 *                           (T * B, P, Q, ldy) buffer
 *   up_clip_nhwc_to_nchw    x frame-major (T * B, H, W, ldx) -> y (B, T, C, H, W)
 * ldy / ldx % 4 == 0 and a 16-byte aligned NHWC pointer. */
int up_clip_nchw_to_nhwc(const float* x, float* y, int B, int T, int C, int H, int W, int ldy, void* stream);
int up_clip_avgpool9s8_fwd(const float* x, float* y, int ldy, int coff, int B, int T, int H, int W, int P, int Q, void* stream);
int up_clip_nhwc_to_nchw(const float* x, int ldx, float* y, int B, int T, int C, int H, int W, void* stream);
/* The clip kernels of the video plan's evaluation entries (ABI 10 additions).  Each is its non-clip / non-mirrored neighbour with
 * the frame-major order (and the mirror) folded in, equal bits to the composition:
 *   up_clip_nchw_to_nhwc_flip    y[f, h, w, c] = x[b, t, c, h, W-1-w] for f = t * B + b, pad channels zero: up_clip_nchw_to_nhwc of
 *                                the mirrored clip.
 *   up_clip_avgpool9s8_flip_fwd  up_clip_avgpool9s8_fwd of the mirrored centre maps, read in place.  The window of output column q is
 *                                that of the MIRRORED map (the padding sits on one side, so it is not the mirror of the window of
 *                                column Q-1-q), summed over ascending columns of the mirrored map, the same divisor: equal bits to
 *                                pooling cm.flip(-1).  Only channel coff is written.
 *   up_clip_heatmap_decode       up_heatmap_decode for T * B frame-major images: image f = t * B + b is read at hm + f * stride_b,
 *                                its J results go to row b * T + t of idx (B,T,J) (may be NULL), preds_xy (B,T,J,2), maxvals (B,T,J).
 *                                The same arithmetic, LDS staging and NaN / tie rules; T == 1 is up_heatmap_decode.
 *   up_clip_final_preds          up_final_preds with the same reordering; inv (B,T,2,3) float64 batch-major, one crop per frame (may
 *                                be NULL, like coords_xy).
 * UP_ERR_INVALID (nothing launched): a null pointer, a size or a stride <= 0, P, Q not the pooled size, an offset beyond int32, and
 * what the neighbours refuse. */
int up_clip_nchw_to_nhwc_flip(const float* x, float* y, int B, int T, int C, int H, int W, int ldy, void* stream);
int up_clip_avgpool9s8_flip_fwd(const float* x, float* y, int ldy, int coff, int B, int T, int H, int W, int P, int Q, void* stream);
/* (up_clip_heatmap_decode / up_clip_final_preds are declared with their neighbours below) */
/* The _strided forms of the clip kernels that write frame-major images (ABI 10 additions; the one-pass flip test of the video plan
 * below; up_clip_crop_to_nhwc_strided, up_clip_center_pool_strided and up_clip_center_pool_flip_strided are declared with their
 * neighbours).  Each is its neighbour with two more arguments: the output is frames of frame_images >= B images, and the image
 * written for sample (b, t) is t * frame_images + first + b instead of t * B + b; images a launch does not address, and the lanes the
 * neighbour leaves alone, are not touched.  frame_images = B, first = 0 is the neighbour itself (which keeps its own launch); two
 * launches with frame_images = 2 B, first = 0 and first = B fill the two halves of every frame of one tensor.  One device function
 * per pair, so the bits of an image are the neighbour's.  The crop's y_nhwc and y_flip_nhwc keep separate pointers and share
 * frame_images / first: one launch, the source read once.
 * UP_ERR_INVALID (nothing launched): first < 0, frame_images < first + B, T * frame_images beyond the int32 range, and what the
 * neighbour refuses (up_clip_avgpool9s8_fwd_strided: what up_clip_avgpool9s8_flip_fwd refuses). */
int up_clip_nchw_to_nhwc_strided(const float* x, float* y, int B, int T, int C, int H, int W, int ldy, int frame_images, int first,
                                 void* stream);
int up_clip_nchw_to_nhwc_flip_strided(const float* x, float* y, int B, int T, int C, int H, int W, int ldy, int frame_images, int first,
                                      void* stream);
int up_clip_avgpool9s8_fwd_strided(const float* x, float* y, int ldy, int coff, int B, int T, int H, int W, int P, int Q,
                                   int frame_images, int first, void* stream);
int up_clip_avgpool9s8_flip_fwd_strided(const float* x, float* y, int ldy, int coff, int B, int T, int H, int W, int P, int Q,
                                        int frame_images, int first, void* stream);
/* nn.Dropout (wasp.py:63, decoder.py:25,29): keep-mask from a counter hash of (seed, element index)
 * or, when ext_mask != NULL, from the caller (float 0/1) — the injectable-RNG hook used for parity.
 * UP_ERR_INVALID (nothing written): a null x / y / mask, n <= 0, p < 0 or p >= 1, an unknown dtype. */
int up_dropout_fwd(const float* x, float* y, uint8_t* mask, const float* ext_mask, int64_t n,
                   float p, uint64_t seed, void* stream);
int up_dropout_bwd(const float* dy, const uint8_t* mask, float* dx, int64_t n, float p, void* stream);
/* `_t` twins of the data-movement operators (see "bf16 STORAGE" above) */
int up_nchw_to_nhwc_t(const float* x, void* y, int N, int C, int H, int W, int ldy, int dt_out, void* stream);
int up_nhwc_to_nchw_t(const void* x, int ldx, float* y, int N, int C, int H, int W, int dt_in, void* stream);
int up_maxpool3s2_fwd_t(const void* x, int ldx, void* y, int ldy, uint8_t* idx, int N, int H, int W, int C, int P, int Q,
                        int dt_in, int dt_out, void* stream);
int up_maxpool3s2_bwd_t(const void* dy, int lddy, const uint8_t* idx, void* dx, int lddx, int N, int H, int W, int C, int P,
                        int Q, int dt_in, int dt_out, void* stream);
int up_bilinear_fwd_t(const void* x, int ldx, void* y, int ldy, int N, int H, int W, int C, int P, int Q, int dtype,
                      void* stream);
int up_bilinear_bwd_t(const void* dy, int lddy, void* dx, int lddx, int N, int H, int W, int C, int P, int Q, int dtype,
                      void* stream);
int up_gap_fwd_t(const void* x, int ldx, void* y, int N, int HW, int C, int dtype, void* stream);
int up_gap_bwd_t(const void* dy, void* dx, int lddx, int N, int HW, int C, int dtype, void* stream);
int up_dropout_fwd_t(const void* x, void* y, uint8_t* mask, const float* ext_mask, int64_t n, float p, uint64_t seed,
                     int dtype, void* stream);
/* ABI 10: ... with a step counter in DEVICE memory mixed into the seed (seed + *step_device * 0x9E3779B97F4A7C15): a captured
 * training step (hipGraph, unipose_amd.graph.GraphedTrainStep) replays the launch with unchanged arguments, its masks still
 * differ from step to step.  step_device = NULL: up_dropout_fwd_t. */
int up_dropout_fwd_step_t(const void* x, void* y, uint8_t* mask, const float* ext_mask, int64_t n, float p, uint64_t seed,
                          const uint64_t* step_device, int dtype, void* stream);
int up_dropout_bwd_t(const void* dy, const uint8_t* mask, void* dx, int64_t n, float p, int dtype, void* stream);
/* nn.MSELoss() mean reduction (unipose.py:70,117): loss[0] = mean((y-t)^2); bwd: dy = 2(y-t)/n * dloss[0] */
int up_mse_fwd(const float* y, const float* t, float* loss, float* workspace, int64_t n, void* stream);
int up_mse_bwd(const float* y, const float* t, const float* dloss, float* dy, int64_t n, void* stream);
size_t up_mse_workspace(int64_t n);

/* ---- ConvLSTM gate math (model/uniposeLSTM.py:16-24, 40-64).  `gates` is the fused gate
 * pre-activation tensor [rows][ldg] laid out g|i|o(|f), each Cg wide, produced by ONE convolution
 * over cat(x,h) with the gate weights stacked along K.  Row strides: gates and dgates [rows][ldg]; cprev [rows][ldc];
 * cell, hide, dcell, dhide AND dcprev [rows][ldo] (dcprev is laid out like cell, not like cprev).  Only the lanes
 * c < Cg of cell / hide / dcprev and c < 3 * Cg (4 * Cg) of dgates are written. ---- */
int up_lstm0_fwd(const float* gates, int ldg, float* cell, float* hide, int ldo, int64_t rows, int Cg, void* stream);
int up_lstm0_bwd(const float* gates, int ldg, const float* dcell, const float* dhide, int ldo,
                 float* dgates, int64_t rows, int Cg, void* stream);
int up_lstm_fwd(const float* gates, int ldg, const float* cprev, int ldc, float* cell, float* hide, int ldo,
                int64_t rows, int Cg, void* stream);
int up_lstm_bwd(const float* gates, int ldg, const float* cprev, int ldc, const float* cell,
                const float* dcell, const float* dhide, int ldo,
                float* dgates, float* dcprev, int64_t rows, int Cg, void* stream);

/* ---- ConvLSTM state of many independent streams in one batch (no reference counterpart) ----
 * A POOL holds the recurrent state of `slots` streams: record s starts at pool + s * slot_stride floats and is
 * hide (rows_per_sample, ldo) then cell (rows_per_sample, ldo), fp32, rows_per_sample = h * w, ldo = rup4(K+2); slot_stride >=
 * 2 * rows_per_sample * ldo (the plans round the record up to 256 bytes).  Every offset is computed in 64 bits.
 * A call works on B samples of rows_per_sample consecutive rows each and takes a per-call table on the HOST, read before the call
 * returns and passed to the kernel by value: slot_host[b] the record of sample b, or -1 for an idle lane; first_host[b] != 0 for a
 * sample that starts (or restarts).  A first and an idle sample are both computed as a first frame (LSTM_0); nothing of the pool is
 * read for them and nothing is written for an idle one.
 * UP_ERR_INVALID (nothing launched, nothing written): B outside 1 .. UP_SERVE_CAP, slots < 1, a slot outside -1 .. slots-1, the same
 * slot >= 0 twice, a null pointer, a size <= 0, a stride smaller than the rows it strides.
 *   up_lstm_state_gather  writes all ldo lanes dst[row * ldd + coff .. + ldo) of every row: the pool's hide row of slot[b] for a
 *                         continuing sample, +0.0f for a first or idle one.  No other lane of dst is touched.
 *   up_lstm_serve_fwd     one element per (row, lane < ldo).  Lanes < Cg: a first or idle sample evaluates up_lstm0_fwd's formula
 *                         on gates0 [rows][ldg0] (g|i|o), a continuing one up_lstm_fwd's on gates [rows][ldg] (g|i|o|f) with the
 *                         previous cell read in place from its record; the result goes to cell / hide [rows][ldo] (lanes < Cg
 *                         only, as up_lstm_fwd) and, for slot >= 0, into the record, by the thread that read it.  Lanes Cg .. ldo-1
 *                         are written as +0.0f into the record only, so a fresh pool may be uninitialised memory and the next gather
 *                         copies whole padded rows.  gates0 may be NULL when no sample is first or idle, gates when none
 *                         continues; a NULL one that a sample needs is UP_ERR_INVALID.
 * Each sample's rows equal, bit for bit, up_lstm0_fwd resp. up_lstm_fwd on those rows (the same device functions). */
enum { UP_SERVE_CAP = 64 };
int up_lstm_state_gather(const float* pool, int64_t slot_stride, int slots, const int32_t* slot_host, const int32_t* first_host, int B,
                         int64_t rows_per_sample, int ldo, float* dst, int ldd, int coff, void* stream);
int up_lstm_serve_fwd(const float* gates0, int ldg0, const float* gates, int ldg, float* pool, int64_t slot_stride, int slots,
                      const int32_t* slot_host, const int32_t* first_host, float* cell, float* hide, int ldo, int B,
                      int64_t rows_per_sample, int Cg, void* stream);

/* ---- heat-map argmax (utils/evaluate.py:32-54 get_max_preds; utils/utils.py:94-106) ----
 * hm: NCHW fp32 (B,J,H,W) as returned by the model.  One wavefront per (b,j): first-max flat index
 * (lowest index wins ties), preds = (idx % W, idx / W) zeroed where max <= 0.  idx may be NULL. */
int up_heatmap_argmax(const float* hm, int B, int J, int H, int W,
                      int32_t* idx, float* preds_xy, float* maxvals, void* stream);

/* ---- heat-map decode: up-sampling + argmax without the up-sampled maps (ABI 10 addition) ----
 * The outputs of up_heatmap_argmax for B x J maps of H x W AS IF they had been up-sampled to P x Q by up_bilinear_fwd first
 * (the reference's full-resolution mode, model/unipose.py:31-32, followed by get_max_preds): idx = p * Q + q on the P x Q grid
 * (may be NULL), preds_xy (B,J,2) zeroed where max <= 0, maxvals (B,J); NaN wins, the lowest flat index wins ties.  Every fine
 * value is computed with the arithmetic of up_bilinear_fwd, so the result equals the composition bit for bit; P == H and
 * Q == W reads the maps as they are (= up_heatmap_argmax).  The fine grid is never written: one workgroup per map, the coarse
 * map in LDS where it fits (up to 12288 values), else read through L2.
 * A map is addressed by three element strides, value (b, j, pixel i) at hm[b * stride_b + j * stride_j + i * stride_p]:
 *   NHWC as a convolution leaves it (ld physical channels): stride_b = H * W * ld, stride_j = 1, stride_p = ld;
 *   NCHW as the models and the video entries return it:     stride_b = J * H * W,  stride_j = H * W, stride_p = 1.
 * UP_ERR_INVALID (nothing launched): null hm / preds_xy / maxvals, a size or a stride <= 0, P < H or Q < W (down-sampling is
 * not a reference use), P * Q or the offset of the last element beyond the int32 range. */
int up_heatmap_decode(const float* hm, int64_t stride_b, int64_t stride_j, int64_t stride_p, int B, int J, int H, int W,
                      int P, int Q, int32_t* idx, float* preds_xy, float* maxvals, void* stream);
/* ... of T * B frame-major images into batch-major results (see the clip kernels above) */
int up_clip_heatmap_decode(const float* hm, int64_t stride_b, int64_t stride_j, int64_t stride_p, int B, int T, int J, int H, int W,
                           int P, int Q, int32_t* idx, float* preds_xy, float* maxvals, void* stream);

/* ---- the evaluation protocol around the forward: flip test and final_preds (ABI 10 additions) ----
 * What published PCKh numbers of this family of networks add to get_max_preds (utils/extra_utils, vendored from pytorch-pose):
 * the flip test (transforms.py:22-43 flip_back, :70-76 fliplr), the quarter-pixel refinement (evaluation.py:75-88 final_preds)
 * and the way back to the source image (transforms.py:79-125 get_transform / transform / transform_preds).
 *
 * up_nchw_to_nhwc_flip: up_nchw_to_nhwc with the mirror folded in, y[n,h,w,c] = x[n,c,h,W-1-w]; pad channels C <= c < ldy are
 * written as zeros exactly as there.  Equal bits to up_nchw_to_nhwc of the mirrored tensor; the same refusals.
 *
 * up_flip_merge: out[b,j,y,x] = 0.5f * (a[b,j,y,x] + f[b,perm[j],y,W-1-x]) — one float32 add, one multiply by 0.5, each rounded
 * once.  The MEAN, where pytorch-pose's drivers take the sum: the argmax is the same and the values stay heat-maps.  a and f
 * share three element strides, out has its own, each addressing a map as up_heatmap_decode's do (NHWC as a convolution leaves
 * it, pad channels never read or written, or NCHW).  perm_host: J int32 on the HOST, checked here and passed to the kernel by
 * value (256 bytes); it need not be an involution.  out may be a when the strides are equal; out must not overlap f.
 * UP_ERR_INVALID (nothing launched): a null pointer, a size or a stride <= 0, a perm entry outside 0..J-1, out == f (mirrored
 * reads cross threads), out == a with other strides, the offset of the last element beyond int32.  UP_ERR_UNSUPPORTED: J > 256.
 *
 * up_final_preds: one wavefront per map, like up_heatmap_argmax.  Per map (b, j):
 *   1. i = the first-max flat index (lowest index wins ties, a NaN wins); maxvals[b,j] = the maximum;
 *   2. x = i % W + 1, y = i / W + 1 as float32, both 0 unless max > 0 (a NaN maximum masks to 0 as maxval.gt(0) does);
 *   3. px = (int)x, py = (int)y; if 1 < px < res0 and 1 < py < res1 and px < W and py < H (the last two hold wherever the
 *      reference does not raise IndexError and keep every read inside the map):
 *      x += 0.25f * sgn(hm[py-1][px] - hm[py-1][px-2]), y += 0.25f * sgn(hm[py][px-1] - hm[py-2][px-1]), sgn(p - q) computed as
 *      (p > q) - (p < q): the sign of the float32 difference for finite values, and defined for infinities;
 *   4. x += 0.5f, y += 0.5f: coords_xy (B,J,2), may be NULL;
 *   5. inv (device, (B,2,3) float64 row-major: the first two rows of np.linalg.inv(get_transform(center, scale, res))):
 *      p0 = (double)x - 1, p1 = (double)y - 1, v_i = (inv[b][i][0] * p0 + inv[b][i][1] * p1) + inv[b][i][2], every product and
 *      sum rounded on its own (no FMA), preds_xy[b,j,i] = (float)((long long)v_i + 1): truncation towards zero like astype(int).
 *      |v_i| >= 2^31 is outside the contract: the launch stays safe, the value is unspecified.  inv == NULL: preds = coords.
 * res0 bounds x and res1 bounds y: the reference's own order in final_preds, and the OPPOSITE of get_transform, where res[1]
 * scales x — so on non-square maps the reference only works with res = [W, H].  Kept as it is.
 * Strides as in up_heatmap_decode.  UP_ERR_INVALID (nothing launched): null hm / preds_xy / maxvals, a size, a stride or a res
 * <= 0, H * W or the offset of the last element beyond int32. */
int up_nchw_to_nhwc_flip(const float* x, float* y, int N, int C, int H, int W, int ldy, void* stream);
int up_flip_merge(const float* a, const float* f, int64_t in_stride_b, int64_t in_stride_j, int64_t in_stride_p, int B, int J,
                  int H, int W, const int32_t* perm_host, float* out, int64_t out_stride_b, int64_t out_stride_j,
                  int64_t out_stride_p, void* stream);
/* up_clip_flip_merge (ABI 10 addition): up_flip_merge over T * B images behind a two-level batch index.  Image (t, b) of a and of f
 * (its own pointer, the same strides) is read at t * in_stride_t + b * in_stride_b, out is written at t * out_stride_t + b *
 * out_stride_b; the arithmetic (one add, one multiply by 0.5, each rounded once), the perm rule, the NaN / inf behaviour and the
 * device function are up_flip_merge's.  With in_stride_t = 2 B * image, in_stride_b = image, f = a + B * image it merges the two
 * halves of every frame of a (T * 2 B) tensor into a compact frame-major (T * B) one in one launch; with in_stride_t = B *
 * in_stride_b and out_stride_t = B * out_stride_b it is up_flip_merge of T * B images.
 * UP_ERR_INVALID / UP_ERR_UNSUPPORTED (nothing launched): as up_flip_merge, with T and the two frame strides among the sizes and
 * strides, and the offset of the last element of the last frame within int32. */
int up_clip_flip_merge(const float* a, const float* f, int64_t in_stride_t, int64_t in_stride_b, int64_t in_stride_j,
                       int64_t in_stride_p, int B, int T, int J, int H, int W, const int32_t* perm_host, float* out, int64_t out_stride_t,
                       int64_t out_stride_b, int64_t out_stride_j, int64_t out_stride_p, void* stream);
int up_final_preds(const float* hm, int64_t stride_b, int64_t stride_j, int64_t stride_p, int B, int J, int H, int W, int res0,
                   int res1, const double* inv, float* preds_xy, float* coords_xy, float* maxvals, void* stream);
int up_clip_final_preds(const float* hm, int64_t stride_b, int64_t stride_j, int64_t stride_p, int B, int T, int J, int H, int W,
                        int res0, int res1, const double* inv, float* preds_xy, float* coords_xy, float* maxvals, void* stream);

/* ---- training targets and input normalisation (the step BEFORE the path) ----
 * up_make_heatmaps: lsp_lspet_data.py:224-236 / mpii_data.py:165-175.  kpt_xy (B,K,2) float64 pixel coordinates of the
 * input image; joint k of sample b is centred at int(coordinate) / stride on the H x W map; values
 * exp(-D2 / 2 / sigma^2) computed in float64 (utils/utils.py:200-203), clipped to <= 1, < 0.0099 -> 0, stored float32;
 * out (B,K+1,H,W): channel 0 = 1 - max over the joint channels, channel k+1 = joint k.
 * up_make_gaussian_maps: one such map per centre (the centre maps, lsp_lspet_data.py:238-242; centres as given).
 * up_normalize_image: (pixel - mean) / std and HWC -> CHW (Mytransforms.py:10-41 with mean 128, std 256). */
int up_make_heatmaps(const double* kpt_xy, int B, int K, int H, int W, double stride, double sigma, float* out,
                     void* stream);
int up_make_gaussian_maps(const double* center_xy, int N, int H, int W, double sigma, float* out, void* stream);
int up_normalize_image(const float* img_hwc, int B, int H, int W, int C, float mean, float stdv, float* out_chw,
                       void* stream);

/* ---- training targets of the optional box head (ABI 10 addition; SURVEY 8f N2 + N4) ----
 * The five maps the reference's loaders build with getBoundingBox (utils/lsp_lspet_data.py:71-113, returned as the sixth item of
 * every sample, :247-249; the same function with a guard in utils/bbc_data.py:23-72), for a whole batch in one launch.
 * kpt_xy (B,K,2) float64 pixel coordinates as for up_make_heatmaps; height, width: the image size the loader passes (img.shape);
 * out (B,5,h,w) float32, dense, h = int(height / stride), w = int(width / stride); map order centre, top-left, bottom-left,
 * top-right, bottom-right — the order up_persons_decode reads from box_ch0.  Per sample, statement by statement in float64 with
 * int() truncating towards zero (negative values included), the reference's quirks kept:
 *   a joint counts when kpt[1] >= 0 OR kpt[0] >= 0;  x collects kpt[1], y collects kpt[0] of the counted joints;
 *   x_min = int(max(min(x), 0)), x_max = int(min(max(x), width)), y_min = int(max(min(y), 0)), y_max = int(min(max(y), height))
 *     (x holds the second coordinate and is still bounded by `width`; x_max and y_max may be negative);
 *   centre = ((x_min + x_max) / 2, (y_min + y_max) / 2);
 *   cell(v, n) = int(min(int(v / stride), n / stride - 1)); the five pairs (cell(y, height), cell(x, width)) of the centre,
 *     (y_min, x_min), (y_min, x_max), (y_max, x_min), (y_max, x_max) — n / stride - 1 is not rounded first (100 / 3 - 1 = 32.33);
 *   map i is the Gaussian of up_make_heatmaps (float64 exp(-D2 / 2 / sigma^2), clipped to <= 1, < 0.0099 -> 0, stored float32)
 *     centred at COLUMN = the first entry of pair i (from y) and ROW = the second (from x).  The reference hard-codes sigma 3.
 * A sample without a counted joint gets the maps of bbc_data.py:32-36 (the box 0, 0, 0, 0: five Gaussians at pixel (0, 0)) and
 * status[b] = UP_BOX_NO_VISIBLE_JOINT — where the LSP form raises ValueError (min of an empty list), which is the caller's
 * business; every other sample gets UP_BOX_OK.  status (B) int32 may be NULL.  A sample never affects another.
 * Contract: finite coordinates with |coordinate| <= 1e9 (non-finite values are outside it); any K >= 1.  One thread per output
 * pixel walks the K joints of its sample.
 * UP_ERR_INVALID (nothing launched): null kpt_xy / out, B, K, height or width <= 0, stride or sigma <= 0, h or w < 1,
 * B * 5 * h * w beyond the int32 range. */
enum { UP_BOX_OK = 0, UP_BOX_NO_VISIBLE_JOINT = 1 };
int up_make_box_maps(const double* kpt_xy, int B, int K, int height, int width, double stride, double sigma, float* out,
                     int32_t* status, void* stream);

/* ---- augmentation of a training batch: one affine resample per image (ABI 10 addition) ----
 * What the reference's loaders do to the pixels with Mytransforms.RandomResized, RandomRotate, RandomCrop / SinglePersonCrop and
 * RandomHorizontalFlip (utils/Mytransforms.py, composed in utils/utils.py:231-345) followed by to_tensor + normalize, as ONE bilinear
 * resample under a per-sample affine map (unipose_amd/augment.py composes the four steps; three OpenCV resamples in the reference).
 * src_hwc (B,Hs,Ws,C) dense, src_type UP_PIX_U8 (uint8) or UP_PIX_F32 (float32), C = 1 .. 4;  out_chw (B,C,Ho,Wo) float32, dense.
 * valid_hw (B,2) int32 on the device or NULL: the (height, width) of sample b that holds pixels, for images of different sizes
 *   padded into one buffer; cut to 0 .. Hs / 0 .. Ws; NULL = Hs x Ws.  What lies beyond it is never read.
 * inv (B / frames_per_map, 6) float64 on the device: image b uses map b / frames_per_map (the T frames of a clip share one), which
 *   takes the OUTPUT pixel (column u, row v) to the source position  sx = i0*u + i1*v + i2,  sy = i3*u + i4*v + i5.
 * Per output pixel, for every channel:
 *   sx = fma(i0, u, fma(i1, v, i2)), sy likewise, in float64;  x0 = floor(sx), y0 = floor(sy);
 *   fx = (float)(sx - x0), fy = (float)(sy - y0)  (the float64 difference rounded once);
 *   the taps (y0, x0), (y0, x0+1), (y0+1, x0), (y0+1, x0+1): a tap with 0 <= x < valid width and 0 <= y < valid height is the
 *     pixel converted to float32, any other tap is `border` and is not loaded — a constant border that blends, as
 *     cv2.warpAffine(borderValue=...) does.  Unless -1 <= x0 <= width-1 and -1 <= y0 <= height-1, decided in float64 (so also for
 *     NaN, infinities and coordinates such as 1e12 that no integer holds), all four taps are border;
 *   in float32, each line one rounding:  top = fmaf(fx, v01 - v00, v00);  bot = fmaf(fx, v11 - v10, v10);
 *     val = fmaf(fy, bot - top, top);  out = (val - mean) / stdv  — the float32 division of up_normalize_image, so an identity map
 *     (and any integer translation or mirror: fx = fy = 0) reproduces up_normalize_image bit for bit.
 * The reference uses border = mean = 128, stdv = 256.  One thread per output pixel covers the C channels; consecutive threads
 * store consecutive u; 64-bit indexing; no LDS; a grid of at most 2^21 threads walks larger outputs in further trips.
 * UP_ERR_INVALID (nothing launched): null src_hwc / inv / out_chw, an unknown src_type, B, Hs, Ws, Ho or Wo <= 0, C outside 1 .. 4,
 * frames_per_map < 1 or not a divisor of B, stdv <= 0 (or NaN). */
enum { UP_PIX_U8 = 0, UP_PIX_F32 = 1 };
int up_augment_image(const void* src_hwc, int src_type, int B, int Hs, int Ws, int C, const int32_t* valid_hw, const double* inv,
                     int frames_per_map, float border, float mean, float stdv, float* out_chw, int Ho, int Wo, void* stream);

/* ---- the crop in front of the network: source frames to the trunk's NHWC input (ABI 10 addition) ----
 * How a camera frame and a person's centre / scale become the input of the network (the geometry of transforms.py:79-116
 * get_transform, made by unipose_amd/protocol.py crop_maps; the reference's own crop, transforms.py:128-179, copies an integer window
 * and resizes it with scipy.misc.imresize, which SciPy has removed: its pixels cannot be reproduced, the pixel contract is this
 * project's).  up_augment_image's resample, written once as the trunk's NHWC input and, from the same thread, as the mirrored input
 * of the flip test; nothing is staged in NCHW.
 * src_hwc (F,Hs,Ws,C) dense, src_type UP_PIX_U8 or UP_PIX_F32, C = 1 .. 4.
 * frame_of (B) int32 on the device or NULL: sample b reads frame frame_of[b], so several persons share one frame; NULL: sample b
 *   reads frame b, and F must equal B.  Device data, never trusted: an index outside 0 .. F-1 makes every tap of that sample
 *   `border` and nothing is loaded for it.
 * valid_hw (F,2) int32 on the device or NULL: PER SOURCE FRAME, the (height, width) of frame f that holds pixels, cut to 0 .. Hs /
 *   0 .. Ws as in up_augment_image; what lies beyond it is never read.
 * inv (B,6) float64 on the device: one map per sample, with the meaning of up_augment_image's inv.
 * Per output pixel (u, v) and channel c < C: exactly the arithmetic stated for up_augment_image above (float64 coordinates with fma,
 * the float64 decision whether any tap can be valid, the three fmaf blends, the float32 division (val - mean) / stdv) — one device
 * function serves both kernels.  y_nhwc[b,v,u,c] and y_flip_nhwc[b,v,Wo-1-u,c] receive the same value, computed once; the pad
 * channels C <= c < ldy are written as zeros, as up_nchw_to_nhwc writes them.  Either output may be NULL, not both.
 * Contract: y_nhwc has equal bits to up_nchw_to_nhwc(up_augment_image(src[frame_of], valid_hw[frame_of], ...)), y_flip_nhwc to
 * up_nchw_to_nhwc_flip of the same.
 * One thread per output pixel, consecutive threads consecutive u; a pixel's ldy channels leave as 16-byte stores (with ldy = 4 a
 * wavefront writes 1 KiB of consecutive pixels per instruction, in either direction); 64-bit indexing; no LDS; a grid of at most
 * 2^21 threads walks larger outputs in further trips.
 * UP_ERR_INVALID (nothing launched): null src_hwc / inv, both outputs NULL, y_nhwc == y_flip_nhwc, an unknown src_type, F, B, Hs,
 * Ws, Ho or Wo <= 0, C outside 1 .. 4, ldy < C or ldy % 4 != 0, an output that is not 16-byte aligned, frame_of == NULL with
 * F != B, stdv <= 0 (or NaN). */
int up_crop_to_nhwc(const void* src_hwc, int src_type, int F, int Hs, int Ws, int C, const int32_t* frame_of, const int32_t* valid_hw,
                    const double* inv, int B, float border, float mean, float stdv, float* y_nhwc, float* y_flip_nhwc, int Ho, int Wo,
                    int ldy, void* stream);
/* The clip form (ABI 10 addition; the video plan from source frames below): B x T samples, sample (b, t) with frame_of (B,T) (or
 * NULL: F must equal B * T and sample (b, t) reads frame b * T + t), valid_hw (F,2) per source frame and inv (B,T,6) on the
 * caller's side batch-major; the outputs y_nhwc and y_flip_nhwc (T * B, Ho, Wo, ldy) FRAME-major, as the video plan keeps a clip.
 * Contract: image t * B + b of y_nhwc has equal bits to sample b * T + t of up_crop_to_nhwc called with B * T samples and the same
 * (flattened) arguments, y_flip_nhwc to its y_flip_nhwc; T = 1 is up_crop_to_nhwc itself.  The same kernel with the reordering
 * folded in (one device function holds the resample): one thread per output pixel, 16-byte stores, pad channels zero, an index of
 * frame_of outside 0 .. F-1 makes the sample all border and loads nothing, at most 2^21 threads per grid, 64-bit indexing.
 * UP_ERR_INVALID (nothing launched): T <= 0, frame_of == NULL with F != B * T, and what up_crop_to_nhwc refuses. */
int up_clip_crop_to_nhwc(const void* src_hwc, int src_type, int F, int Hs, int Ws, int C, const int32_t* frame_of,
                         const int32_t* valid_hw, const double* inv, int B, int T, float border, float mean, float stdv, float* y_nhwc,
                         float* y_flip_nhwc, int Ho, int Wo, int ldy, void* stream);
/* ... into frames of frame_images images (the _strided forms above): image t * frame_images + first + b of y_nhwc and of y_flip_nhwc */
int up_clip_crop_to_nhwc_strided(const void* src_hwc, int src_type, int F, int Hs, int Ws, int C, const int32_t* frame_of,
                                 const int32_t* valid_hw, const double* inv, int B, int T, float border, float mean, float stdv,
                                 float* y_nhwc, float* y_flip_nhwc, int Ho, int Wo, int ldy, int frame_images, int first, void* stream);

/* ---- the pooled centre map straight from the centre (ABI 10 additions) ----
 * What the video network does with a centre map is AvgPool2d(9,8,1) down to the heat-maps' grid (uniposeLSTM.py:75,114): these
 * write the pooled map from the centre coordinates, the (N,1,H,W) maps never exist.
 * center_xy (N,2) resp. (B,T,2) float64 on the device, (column, row) in pixels of the H x W map; sigma as up_make_gaussian_maps.
 * Output: channel coff of y (N, P, Q, ldy) resp. frame-major (T * B, P, Q, ldy) from the batch-major centres; no other channel of y is
 * touched.  P = (H - 7) / 8 + 1, Q = (W - 7) / 8 + 1.
 * Contract: equal bits to up_avgpool9s8_fwd / up_clip_avgpool9s8_fwd / up_clip_avgpool9s8_flip_fwd of
 * up_make_gaussian_maps(center_xy, N, H, W, sigma).  Every tap is up_make_gaussian_maps' value (float64 exp(-d2 / 2 / sigma / sigma),
 * clipped to <= 1, < 0.0099 -> 0, rounded to float32) and the window, the divisor and the order of the sum are the pooling's: rows
 * ascending, within a row ascending columns of the plane that is pooled, one float32 add per tap, one float32 division at the end.
 * _flip: the plane is the mirrored map m[r][w] = g[r][W-1-w]; its tap at column w is the Gaussian about (cx, cy) evaluated at column
 * W-1-w — NOT a Gaussian about W-1-cx, whose subtraction rounds differently.
 * A tap with d2 > 9.4 sigma^2 is taken as the 0 it is without evaluating exp (the cut lies at d2 = 2 sigma^2 ln(1 / 0.0099) =
 * 9.2304 sigma^2).  A NaN centre propagates NaN, an infinite one gives 0, as in the two-call form.
 * One thread per pooled pixel, consecutive threads consecutive q; no LDS, no atomics.
 * UP_ERR_INVALID (nothing launched): a null pointer, a size <= 0, sigma <= 0 (or NaN), coff outside 0 .. ldy-1, P, Q not the pooled
 * size or <= 0, H * W beyond the int32 range. */
int up_center_pool(const double* center_xy, double sigma, float* y, int ldy, int coff, int N, int H, int W, int P, int Q, void* stream);
int up_clip_center_pool(const double* center_xy, double sigma, float* y, int ldy, int coff, int B, int T, int H, int W, int P, int Q,
                        void* stream);
int up_clip_center_pool_flip(const double* center_xy, double sigma, float* y, int ldy, int coff, int B, int T, int H, int W, int P, int Q,
                             void* stream);
/* ... into frames of frame_images images (the _strided forms above): channel coff of image t * frame_images + first + b */
int up_clip_center_pool_strided(const double* center_xy, double sigma, float* y, int ldy, int coff, int B, int T, int H, int W, int P,
                                int Q, int frame_images, int first, void* stream);
int up_clip_center_pool_flip_strided(const double* center_xy, double sigma, float* y, int ldy, int coff, int B, int T, int H, int W, int P,
                                     int Q, int frame_images, int first, void* stream);

/* ---- PCK / PCKh evaluation (utils/evaluate.py:5-29 calc_dists / dist_acc, :58-172 accuracy) ----
 * From the joint coordinates of the predicted and the target heat-maps (two up_heatmap_argmax calls), entirely on
 * the device: per joint the fraction of counted samples (both target coordinates > 1) whose normalised distance is
 * below 0.5 (acc), thr_pck * torso (pck) and thr_pckh * head (pckh); entry 0 of each is replaced by the mean over
 * the joints with any counted sample; visible[j] = 1 for those joints, *cnt = their number.  Head and torso sizes
 * come from the target joints of sample 0, as in the reference.  Arithmetic types follow the reference under
 * NumPy >= 2 (float32 thresholds, float64 distances).  x is divided by H / 10 and y by W / 10, the reference's own order.
 * Nothing is launched or written on UP_ERR_UNSUPPORTED (J outside 1..256: one workgroup, one thread per joint) and on
 * UP_ERR_INVALID (a null pointer, B / H / W <= 0, an unknown dataset id, fewer joint channels than the dataset's head / torso
 * formulas touch: LSP 15, COCO 14, Penn_Action 9, NTID 5, PoseTrack 14, BBC 8, MPII 11).  With no counted sample at all
 * *cnt = 0, every result is 0 and entry 0 is not replaced. */
enum { UP_DS_LSP = 0, UP_DS_COCO = 1, UP_DS_PENN_ACTION = 2, UP_DS_NTID = 3, UP_DS_POSETRACK = 4, UP_DS_BBC = 5,
       UP_DS_MPII = 6 };
int up_pck_accuracy(const float* pred_xy, const float* target_xy, int B, int J, int H, int W, int dataset,
                    double thr_pck, double thr_pckh, double* acc, double* pck, double* pckh, double* visible,
                    int32_t* cnt, void* stream);

/* ---- multi-person decode of the optional box head (utils/uniPose.py:14-200 uniPose_kpts) ----
 * up_peak_mask: mask[e] = 1 where maps[e] > 0 and >= each in-bounds neighbour of its 3x3 neighbourhood — the peaks the
 * reference extracts with scipy's maximum_filter / binary_erosion on the centre and the four corner maps; maps is
 * (nmaps,H,W) fp32, mask (nmaps,H,W) bytes.
 * up_box_argmax: maps (C,H,W) of ONE sample; boxes (P,4) int32 = row0,row1,col0,col1 (half-open, non-empty, inside the
 * map: the caller checks, as numpy would raise); for every person and channel ch0..ch0+nch-1 the position of the first
 * maximum inside the box, relative to the box, row-major: out_hw (P,nch,2) int32 = (row, col). */
int up_peak_mask(const float* maps, int nmaps, int H, int W, uint8_t* mask, void* stream);
int up_box_argmax(const float* maps, int C, int H, int W, const int32_t* boxes, int P, int ch0, int nch,
                  int32_t* out_hw, void* stream);

/* ---- multi-person decode of a whole batch in one launch (ABI 10 addition) ----
 * For every sample b what the reference's uniPose_kpts gives on maps[b:b+1], with nothing crossing to the host: one workgroup per
 * sample lists the peaks (the rule of up_peak_mask) of the five box maps box_ch0 .. box_ch0+4 = centre, top-left, bottom-left,
 * top-right, bottom-right in row-major order, walks the n centre peaks, and arg-maxes the joint channels joint_ch0 ..
 * joint_ch0+njoints-1 inside every person's box (the order of up_box_argmax: NaN wins, the first maximum in the box's row-major
 * order wins ties, a box of -inf only gives its first pixel).  The five maps are staged in LDS where 5 * H * W <= 12288 values,
 * read through L2 otherwise.  The maps are addressed by three element strides exactly like up_heatmap_decode's (NHWC as a
 * convolution leaves it, pad channels never read, or NCHW); C is the number of logical channels.
 *   count[b]  = n, the number of centre peaks, always.
 *   status[b] = UP_PERSONS_OVERFLOW when n > max_persons (nothing else is written for the sample); otherwise the first failure
 *               of the reference's walk idx = 0 .. n-1, at each idx in its order: tl[idx] exists, br[idx] exists, the box rows
 *               tl.row .. br.row, columns tl.col .. br.col (half-open) is non-empty, bl[idx] exists, tr[idx] exists — a missing
 *               entry is UP_PERSONS_MISSING_CORNER (the reference's IndexError), an empty box UP_PERSONS_EMPTY_BOX (its
 *               ValueError); the kpts rows of such a sample are unspecified.  A corner map with more than max_persons peaks is
 *               no overflow: only its first n entries are ever used.  NaN in the five box maps is outside the contract.
 *   kpts (B, max_persons, njoints + 5, 2) int32 = (x, y): with UP_PERSONS_OK person p < n gets the njoints joints, then centre,
 *               tl, bl, tr, br.  Rows of persons >= n are not written.  A failing sample does not affect the others.
 * max_persons bounds the LDS lists: 1 .. UP_PERSONS_CAP.
 * UP_ERR_INVALID (nothing launched): a null pointer, a size or a stride <= 0, max_persons outside 1 .. UP_PERSONS_CAP, box_ch0 < 0
 * or box_ch0 + 5 > C, joint_ch0 < 0, njoints < 1 or joint_ch0 + njoints > C, the offset of the last element or the size of kpts
 * beyond the int32 range. */
enum { UP_PERSONS_OK = 0, UP_PERSONS_MISSING_CORNER = 1, UP_PERSONS_EMPTY_BOX = 2, UP_PERSONS_OVERFLOW = 3 };
enum { UP_PERSONS_CAP = 512 };
int up_persons_decode(const float* maps, int64_t stride_b, int64_t stride_j, int64_t stride_p, int B, int C, int H, int W,
                      int box_ch0, int joint_ch0, int njoints, int max_persons, int32_t* count, int32_t* status, int32_t* kpts,
                      void* stream);

/* ---- whole-graph inference entry (ABI 9) ----------------------------------------------------------------------------
 * The UniPose image network (model/unipose.py:8-38: ResNet-101 + WASP + decoder) with every BatchNorm folded into its
 * convolution, as ONE call on one stream — what the reference's validation / test loops issue as `heat = model(input)`
 * (unipose.py:150-160).  The plan owns the packed weight images and biases (device memory); activations live in a
 * caller-provided workspace of up_unipose_plan_workspace() bytes (256-byte aligned), reused between calls.
 *   up_unipose_plan_create(&cfg, &plan);
 *   for i in [0, up_unipose_plan_num_convs): set_conv(plan, i, folded weight of <name>.weight, <name>.bias or NULL, stream)
 *   up_unipose_forward(plan, input NCHW (batch, 3, H, W), heat-maps NCHW (batch, out_channels, ceil(H/8), ceil(W/8)), workspace, bytes, stream)
 * Convolution names are the reference's state_dict prefixes ("backbone.layer3.11.conv2", "wasp.aspp2.atrous_conv",
 * "decoder.last_conv.8"); a parameter that is applied twice (wasp.conv2, wasp.py:72-80) appears twice, setting it once suffices.
 * Launches and descriptors are those of the drop-in module's folded inference forward: equal bits.  Training has no
 * whole-graph entry (it runs through autograd).
 * Three more programs run over the same weights and the same workspace (up_unipose_plan_workspace() covers the largest of the
 * four; the full-resolution one needs a (batch, H, W, out_channels rounded up to 4) fp32 tensor more than the trunk):
 *   up_unipose_forward_upsampled  the module's forward at stride != 8 (model/unipose.py:31-32): the heat-maps up-sampled to the
 *                                 input size (up_bilinear_fwd), written NCHW (batch, out_channels, H, W).  Equal bits again.
 *   up_unipose_keypoints          the trunk, then up_heatmap_decode straight from the NHWC output of decoder.last_conv.8: no layout
 *                                 pass, no up-sampled tensor.  out_h x out_w is the heat-map size ceil(H/8) x ceil(W/8) (what
 *                                 up_heatmap_argmax gives on up_unipose_forward's result) or the input size H x W (... on
 *                                 up_unipose_forward_upsampled's); any other size is UP_ERR_INVALID.  idx (may be NULL), preds_xy,
 *                                 maxvals: (batch, out_channels[, 2]); with the box head all out_channels are decoded, the
 *                                 caller slices.
 *   up_unipose_persons            for a plan with the box head: the trunk, then up_persons_decode straight from the NHWC output of
 *                                 decoder.last_conv.8, on the heat-maps' own grid (the one the reference decodes on): count, status
 *                                 (batch), kpts (batch, max_persons, njoints + 5, 2) as documented there.  Channel arguments
 *                                 outside out_channels, max_persons outside 1 .. UP_PERSONS_CAP or a null pointer are
 *                                 UP_ERR_INVALID before anything is launched.
 * The evaluation protocol (flip test, final_preds; see up_flip_merge / up_final_preds) has three programs more.  They need a
 * larger workspace, up_unipose_plan_flip_workspace() bytes, because the flip test keeps the first pass's heat-maps while the
 * trunk runs again; up_unipose_plan_workspace() is what it was.  All work on the heat-maps' own grid ceil(H/8) x ceil(W/8).
 *   up_unipose_flip_forward       the trunk on x and on the mirrored x (up_nchw_to_nhwc_flip) over the same activations — every
 *                                 convolution launch is the one up_unipose_forward makes — then up_flip_merge with perm_host
 *                                 (out_channels int32 on the host) into heat_nchw (batch, out_channels, ceil(H/8), ceil(W/8)):
 *                                 equal bits to merging up_unipose_forward of x and of the mirrored x.
 *   up_unipose_final_preds        the same, merged in place, then up_final_preds straight from the NHWC maps: preds_xy, coords_xy
 *                                 (may be NULL), maxvals (batch, out_channels[, 2]); inv (device, (batch,2,3) float64) may be NULL.
 *                                 perm_host == NULL: one pass, no flip test (up_unipose_plan_workspace() bytes suffice).
 * A perm entry outside 0 .. out_channels-1, res <= 0, a null pointer, unset weights or a too-small workspace are refused before
 * anything is launched.  up_unipose_plan_program_workspace(plan, k): the need of program k alone, in the order of this comment
 * (0 forward, 1 upsampled, 2 keypoints, 3 persons, 4 flip_forward, 5 final_preds with and 6 without the flip test), 0 for any
 * other k: up_unipose_plan_workspace() is the largest of 0..3, up_unipose_plan_flip_workspace() of 4..6.
 * From source frames: two entries put up_crop_to_nhwc (C = 3, B = batch, Ho x Wo = H x W, ldy = 4) in front of these programs, in
 * place of their layout pass — in the flip test ONE launch fills the input and the mirrored input, and the source is read once per
 * person.  src_hwc .. stdv are up_crop_to_nhwc's arguments (crop_inv its inv); every convolution launch is the one the
 * corresponding program above makes, so with equal crop bits the results are equal bit for bit.
 *   up_unipose_frame_heatmaps     heat_nchw (batch, out_channels, ceil(H/8), ceil(W/8)): up_unipose_forward's result, or with
 *                                 perm_host != NULL up_unipose_flip_forward's, of the cropped input.
 *   up_unipose_frame_final_preds  up_unipose_final_preds of the cropped input; perm_host == NULL: no flip test.  inv, res0, res1:
 *                                 the way back as there (protocol.inverse_maps on the heat-map grid), independent of crop_inv.
 * Refused before anything is launched: what up_crop_to_nhwc refuses, and what the entries above refuse.  The mirrored input stays
 * alive through the first trunk, so the flip forms need more than up_unipose_plan_flip_workspace(): the need of each is
 * up_unipose_plan_program_workspace(plan, UP_PROGRAM_FROM_FRAMES + k), k = 0, 4, 5, 6 naming the program it otherwise equals (0 for
 * any other k); neither up_unipose_plan_workspace() nor up_unipose_plan_flip_workspace() changes.
 * Storage: up_unipose_plan_create_t(cfg, dtype, &plan) with dtype = UP_DT_F32 (what up_unipose_plan_create makes) or UP_DT_BF16;
 * any other dtype is UP_ERR_INVALID, *plan stays untouched and nothing is allocated.  up_unipose_plan_dtype() reads it back.  A
 * UP_DT_BF16 plan runs every program above in bf16 STORAGE: the launches of the folded module under the bf16-storage arithmetic
 * (UP_MATH_BF16S).  The input pass (layout or crop) and backbone.conv1 stay fp32 (4 input channels are no multiple of 32), the
 * stem's max-pool writes bf16 (up_maxpool3s2_fwd_t), every later convolution is up_conv2d_fwd_bf16(UP_MATH_BF16S) on bf16 tensors
 * whose channels are padded to multiples of 32 (pad lanes zeroed by the program in every call), the pooling, resize and concat
 * passes are the `_t` forms, and decoder.last_conv.8 is the UP_MATH_BF16S_F32OUT launch: the endings read fp32 NHWC maps of
 * out_channels rounded up to 32 lanes.  The plan keeps bf16 weight images (the hi plane of up_pack_weights_bf16; fp32 for the
 * stem) and fp32 biases.  Nothing changes at the boundary: fp32 input or source frames, fp32 results, folded fp32 OIHW weights
 * through up_unipose_plan_set_conv, the same refusals.  The workspace figures are the plan's own (smaller than the fp32 plan's).
 * The flip test in ONE pass: up_unipose_plan_create_ex(cfg, dtype, flags, &plan) with flags = 0 (what _create_t makes) or
 * UP_PLAN_FLIP_ONE_PASS; any other bit is UP_ERR_INVALID, *plan stays untouched and nothing is allocated.  up_unipose_plan_flags()
 * reads it back.  A flagged plan builds the programs with the flip test (4, 5, UP_PROGRAM_FROM_FRAMES + 4 and + 5) as one trunk
 * over 2 * batch images, images 0 .. batch-1 the input and batch .. 2 batch-1 the mirrored input, the two layout passes (or the one
 * crop launch) writing the halves of one tensor, and up_flip_merge reading the halves of the trunk's output.  The entries, their
 * arguments and refusals are the same.  Its results equal, bit for bit, up_flip_merge of the two halves of up_unipose_forward of a
 * plan of batch 2 * batch on cat(x, mirror(x)) — NOT the two-pass form's, wherever a convolution picks its kernel by the number of
 * rows.  up_unipose_plan_flip_workspace() and up_unipose_plan_program_workspace(plan, k) report those programs' own need, about that
 * of a forward at batch 2 * batch (the from-frames forms keep no extra tensor); every other program, up_unipose_plan_workspace()
 * and the weights are what they are without the flag. */
enum { UP_PROGRAM_FROM_FRAMES = 256 };
enum { UP_PLAN_FLIP_ONE_PASS = 1 };     /* flags of up_unipose_plan_create_ex / up_unipose_lstm_plan_create_ex */
typedef struct up_unipose_plan up_unipose_plan;
typedef struct {
    int32_t batch, height, width;   /* input (batch, 3, height, width) */
    int32_t output_stride;          /* 16 or 8 (resnet.py:49-58) */
    int32_t out_channels;           /* channels of decoder.last_conv.8: num_classes + 1 (+ 5 for the multi-person box head) */
} up_unipose_config;
int up_unipose_plan_create(const up_unipose_config* cfg, up_unipose_plan** plan);     /* = ..._create_t(cfg, UP_DT_F32, plan) */
int up_unipose_plan_create_t(const up_unipose_config* cfg, int dtype, up_unipose_plan** plan);
int up_unipose_plan_dtype(const up_unipose_plan* plan);      /* UP_DT_F32 / UP_DT_BF16; UP_ERR_INVALID for NULL */
int up_unipose_plan_create_ex(const up_unipose_config* cfg, int dtype, int flags, up_unipose_plan** plan);   /* _create_t: flags = 0 */
int up_unipose_plan_flags(const up_unipose_plan* plan);      /* 0 / UP_PLAN_FLIP_ONE_PASS; UP_ERR_INVALID for NULL */
void up_unipose_plan_destroy(up_unipose_plan* plan);
int up_unipose_plan_num_convs(const up_unipose_plan* plan);
const char* up_unipose_plan_conv_name(const up_unipose_plan* plan, int i);
int up_unipose_plan_conv_shape(const up_unipose_plan* plan, int i, int32_t* oihw /* [4] */, int32_t* has_bias);
int up_unipose_plan_set_conv(up_unipose_plan* plan, int i, const float* w_oihw, const float* bias, void* stream);
size_t up_unipose_plan_workspace(const up_unipose_plan* plan);
int up_unipose_forward(up_unipose_plan* plan, const float* x_nchw, float* heat_nchw, void* workspace, size_t workspace_bytes,
                       void* stream);
int up_unipose_forward_upsampled(up_unipose_plan* plan, const float* x_nchw, float* heat_nchw, void* workspace,
                                 size_t workspace_bytes, void* stream);
int up_unipose_keypoints(up_unipose_plan* plan, const float* x_nchw, int out_h, int out_w, int32_t* idx, float* preds_xy,
                         float* maxvals, void* workspace, size_t workspace_bytes, void* stream);
int up_unipose_persons(up_unipose_plan* plan, const float* x_nchw, int box_ch0, int joint_ch0, int njoints, int max_persons,
                       int32_t* count, int32_t* status, int32_t* kpts, void* workspace, size_t workspace_bytes, void* stream);
size_t up_unipose_plan_flip_workspace(const up_unipose_plan* plan);
size_t up_unipose_plan_program_workspace(const up_unipose_plan* plan, int program);
int up_unipose_flip_forward(up_unipose_plan* plan, const float* x_nchw, const int32_t* perm_host, float* heat_nchw, void* workspace,
                            size_t workspace_bytes, void* stream);
int up_unipose_final_preds(up_unipose_plan* plan, const float* x_nchw, const int32_t* perm_host, const double* inv, int res0,
                           int res1, float* preds_xy, float* coords_xy, float* maxvals, void* workspace, size_t workspace_bytes,
                           void* stream);
int up_unipose_frame_heatmaps(up_unipose_plan* plan, const void* src_hwc, int src_type, int F, int Hs, int Ws, const int32_t* frame_of,
                              const int32_t* valid_hw, const double* crop_inv, float border, float mean, float stdv,
                              const int32_t* perm_host, float* heat_nchw, void* workspace, size_t workspace_bytes, void* stream);
int up_unipose_frame_final_preds(up_unipose_plan* plan, const void* src_hwc, int src_type, int F, int Hs, int Ws,
                                 const int32_t* frame_of, const int32_t* valid_hw, const double* crop_inv, float border, float mean,
                                 float stdv, const int32_t* perm_host, const double* inv, int res0, int res1, float* preds_xy,
                                 float* coords_xy, float* maxvals, void* workspace, size_t workspace_bytes, void* stream);

/* ---- whole-clip and per-frame inference entry of UniPose-LSTM (ABI 10 additions) ----------------------------------------
 * The video network (model/uniposeLSTM.py:67-138: the image trunk with the video WASP, ConvLSTM, five-convolution head) with
 * every BatchNorm folded, like up_unipose_forward above: the plan owns the packed weights, activations and the recurrent state
 * between frames live in a caller-provided workspace of up_unipose_lstm_plan_workspace() bytes (256-byte aligned).  Two forms:
 *   up_unipose_lstm_step  one frame, what the reference's loop issues as `heat, cell, hide = model(x, cm, j, heat, hide, cell)`
 *                         (uniposeLSTM.py:124-128): x (B, 3, H, W), centre map (B, 1, H, W), the caller's state prev_hide /
 *                         prev_cell (B, K+2, h, w) NCHW, both NULL for the first frame (LSTM_0); writes heat (B, K+1, h, w) and
 *                         the new cell / hide (B, K+2, h, w).  Launches of the drop-in module's per-frame path.
 *   up_unipose_lstm_clip  the whole clip of config.frames frames: x (B, T, 3, H, W), centre maps (B, T, 1, H, W) -> heat
 *                         (B, T, K+1, h, w) and the cell / hide of the LAST frame (either may be NULL).  The trunk once on the T * B
 *                         frames, the recurrence frame by frame with the state kept in the workspace, the head once on the T * B
 *                         hidden states: the launches of the module's whole-clip unroll (batch_frames).
 * h = ceil(H / 8) must equal the pooled centre map's (H - 7) / 8 + 1, i.e. H % 8 (and W % 8) in {0, 7}: create refuses the rest.
 * Convolution names are the reference's state_dict prefixes: the trunk's (wasp.conv2 twice; the video WASP's
 * wasp.global_avg_pool.1 has no bias), lstm_0.conv_{g,i,o}_lstm, lstm.conv_{g,i,o,f}{x,h}_lstm and conv1 .. conv5.  The plan
 * stacks the gate weights itself once all parts of a cell are set; a forward call while any is unset fails ("never set").
 * Both forms return heat-maps, on the h x w grid only (the reference's video model stores `stride` and never up-samples).
 *
 * The evaluation entries run the same convolution launches over the same weight store and read the NHWC output of conv5 directly;
 * the plan keeps a clip frame-major inside, results are batch-major (B, T, ...):
 *   up_unipose_lstm_clip_keypoints    the clip program up to conv5, then up_clip_heatmap_decode: idx (B,T,K+1) (may be NULL),
 *                                     preds_xy (B,T,K+1,2), maxvals (B,T,K+1) on the out_h x out_w grid, which is h x w or the
 *                                     input's H x W (anything else: UP_ERR_INVALID); cell_last / hide_last as up_unipose_lstm_clip
 *                                     (may be NULL).  No NCHW heat tensor is written.
 *   up_unipose_lstm_clip_flip         the flip test, this project's extension (the reference's video drivers run none): the whole clip
 *                                     program on the clip and again on the mirrored clip (up_clip_nchw_to_nhwc_flip; the mirrored centre
 *                                     maps pooled from the mirrored side, up_clip_avgpool9s8_flip_fwd), each pass with its own
 *                                     recurrent state, every convolution launch one that up_unipose_lstm_clip makes; the first pass's
 *                                     heat-maps stay alive through the second; then up_flip_merge in place with perm_host (K+1 int32 on
 *                                     the host) and up_clip_nhwc_to_nchw into heat (B, T, K+1, h, w).  Equal bits to merging
 *                                     up_unipose_lstm_clip of the clip and of the mirrored clip frame by frame.  No state is
 *                                     returned: there are two.
 *   up_unipose_lstm_clip_final_preds  the same merged in place, then up_clip_final_preds: preds_xy, coords_xy (may be NULL)
 *                                     (B,T,K+1,2), maxvals (B,T,K+1); inv (device, (B,T,2,3) float64, one crop per frame) may be NULL.
 *                                     perm_host == NULL: one pass, no flip test.
 *   up_unipose_lstm_stream_keypoints  one frame in, joints out, for a caller that feeds a camera: the step program with hide and cell
 *                                     kept in `state`, a caller-owned, opaque, 256-byte aligned device buffer of
 *                                     up_unipose_lstm_plan_state_bytes() bytes (the plan's own NHWC (B, h, w, rup4(K+2)), twice), then
 *                                     up_heatmap_decode on the out_h x out_w grid: idx (B,K+1) (may be NULL), preds_xy (B,K+1,2),
 *                                     maxvals (B,K+1); heat_nchw (B, K+1, h, w) may be NULL.  first != 0: LSTM_0, nothing is read from
 *                                     `state`, the new state is written into it; first == 0: the state is copied into the program's
 *                                     tensors and overwritten with the new one at the end.  Whole padded rows are copied, so the pad
 *                                     channels stay the zeros the plan wrote.  Several streams may share one plan (and workspace,
 *                                     calls in stream order), each with its own buffer.  A NULL or misaligned state: UP_ERR_INVALID.
 * Workspaces: up_unipose_lstm_plan_program_workspace(plan, k) is the need of program k alone, in the order 0 step-first, 1 step-next,
 * 2 clip, 3 clip_keypoints, 4 clip_flip, 5 clip_final_preds with and 6 without the flip test, 7 stream-first, 8 stream-next, 0 for any
 * other k.  up_unipose_lstm_plan_workspace() is the largest of 0..3 and 6..8 (step and clip ask for exactly that, as before),
 * up_unipose_lstm_plan_flip_workspace() of 4 and 5; an evaluation entry asks for its own program's need.  Unset weights, a too-small
 * workspace, a perm entry outside 0..K, res <= 0 and a null required pointer are refused before anything is launched.
 *
 * From source frames (ABI 10 additions): three entries put the crop and up_center_pool in front of these programs, in place of their
 * layout pass and of the pooling of full-resolution centre maps.  src_hwc .. stdv are up_clip_crop_to_nhwc's arguments with
 * B = batch, T = frames (C = 3, Ho x Wo = H x W, ldy = 4; crop_inv (B,T,6) its inv), for the stream up_crop_to_nhwc's with
 * crop_inv (B,6); center_xy (B,T,2) resp. (B,2) float64 on the device and sigma are up_clip_center_pool's resp. up_center_pool's:
 * the centre in pixels of the H x W network input.  In the flip test ONE crop launch fills the input and the mirrored input, and
 * the mirrored pass pools its centre map from the same coordinates with up_clip_center_pool_flip.  Every convolution launch is one
 * the corresponding program above makes, so the results equal, bit for bit, those of the entry above called with the crop
 * (up_augment_image) and up_make_gaussian_maps(center_xy) as x and centre maps.
 *   up_unipose_lstm_clip_frame_heatmaps       perm_host == NULL: up_unipose_lstm_clip, cell_last / hide_last optional as there;
 *                                             perm_host != NULL: up_unipose_lstm_clip_flip, and a non-NULL cell_last or hide_last is
 *                                             refused (there are two states).
 *   up_unipose_lstm_clip_frame_final_preds    up_unipose_lstm_clip_final_preds; inv (B,T,2,3) or NULL, res0, res1: the way back as
 *                                             there, independent of crop_inv.
 *   up_unipose_lstm_stream_frame_final_preds  one camera frame in, joints in frame pixels out: up_crop_to_nhwc with B samples,
 *                                             up_center_pool, the step program with the state in `state` exactly as
 *                                             up_unipose_lstm_stream_keypoints keeps it (`first` as there), then up_final_preds straight
 *                                             from the NHWC output of conv5: preds_xy, coords_xy (may be NULL) (B,K+1,2), maxvals (B,K+1);
 *                                             inv (B,2,3) or NULL; heat_nchw (B,K+1,h,w) may be NULL.  No flip test inside a stream.
 * Refused before anything is launched: what the crop and the centre-pool kernels refuse, and what the entries above refuse (a NULL
 * or misaligned state included); the outputs are then untouched.  Workspace: each asks for
 * up_unipose_lstm_plan_program_workspace(plan, UP_PROGRAM_FROM_FRAMES + k), k = 2, 4, 5, 6, 7, 8 naming the program it otherwise
 * equals (0 for any other k; the flip forms keep the mirrored input alive through the first pass); neither
 * up_unipose_lstm_plan_workspace() nor up_unipose_lstm_plan_flip_workspace() changes.
 * Storage: up_unipose_lstm_plan_create_t(cfg, dtype, &plan) with dtype = UP_DT_F32 (what up_unipose_lstm_plan_create makes) or
 * UP_DT_BF16; any other dtype is UP_ERR_INVALID, *plan stays untouched and nothing is allocated.  up_unipose_lstm_plan_dtype() reads
 * it back.  A UP_DT_BF16 plan runs every program above with the launches of the folded module under the bf16-storage arithmetic:
 * the trunk as the image plan's (fp32 input pass and stem, bf16 tensors and weight images behind it, decoder.last_conv.8 the
 * UP_MATH_BF16S_F32OUT launch).  Everything behind the trunk stays fp32 TENSORS, because the 15 / 16-channel state lies outside the
 * 32-lane granularity of the bf16 kernels: the hand-over tensor of rup4(K+2) lanes (zeroed in every call, the K+1 real lanes of the
 * trunk's 32-lane maps copied in, the pooled centre map in lane K+1), cells, hides, the gate kernels, the head and every ending.  The
 * convolutions of those tensors pick their arithmetic by their physical input width: Cp % 32 == 0 runs
 * up_conv2d_fwd_bf16(UP_MATH_BF16) — fp32 in and out, bf16 operands, the weight's hi plane — (conv2 .. conv5, and the stacked gate
 * convolution where 2 * rup4(K+2) is a multiple of 32, e.g. K = 13), anything else up_conv2d_fwd (lstm_0, conv1, the gate
 * convolution at K = 15).  The stacked gate weights are stacked in fp32 and rounded once.  Nothing changes at the boundary: the same
 * arguments, fp32 state (up_unipose_lstm_plan_state_bytes() is equal for both storages), the same refusals; the workspace figures
 * are the plan's own (smaller than the fp32 plan's).
 * The flip test in ONE pass: up_unipose_lstm_plan_create_ex(cfg, dtype, flags, &plan) with flags = 0 (what _create_t makes) or
 * UP_PLAN_FLIP_ONE_PASS; any other bit is UP_ERR_INVALID, *plan stays untouched and nothing is allocated.
 * up_unipose_lstm_plan_flags() reads it back.  A flagged plan builds programs 4, 5, UP_PROGRAM_FROM_FRAMES + 4 and + 5 as ONE pass over
 * frames of 2 B images: frame-major image t * 2 B + b is the plain sample, t * 2 B + B + b its mirror (the _strided layout, pooling,
 * crop and centre-pool entries write the halves), the gate convolution of frame t runs on 2 B contiguous rows, so each half keeps its
 * own state, the head runs once on T * 2 B hidden states, and up_clip_flip_merge merges the halves of conv5's output into a compact
 * frame-major tensor the endings read as before.  Entries, arguments and refusals are the same (no state is returned).  The results
 * equal, bit for bit, up_flip_merge, frame by frame, of the two batch halves of up_unipose_lstm_clip of a plan of batch 2 B on
 * cat(x, mirror(x)), cat(center, mirror(center)) — not the two-pass form's wherever a convolution picks its kernel by the number of
 * rows.  up_unipose_lstm_plan_flip_workspace() and ..._program_workspace(plan, k) report those programs' own need (about a clip at
 * batch 2 B); every other program, up_unipose_lstm_plan_workspace() and up_unipose_lstm_plan_state_bytes() are unchanged. */
typedef struct up_unipose_lstm_plan up_unipose_lstm_plan;
typedef struct {
    int32_t batch, frames, height, width;   /* clip (batch, frames, 3, height, width); frames = 1 if only the step form is used */
    int32_t output_stride;                  /* 16 or 8 */
    int32_t num_classes;                    /* K: heat-maps K+1, recurrent state K+2 channels */
} up_unipose_lstm_config;
int up_unipose_lstm_plan_create(const up_unipose_lstm_config* cfg, up_unipose_lstm_plan** plan);   /* = ..._create_t(cfg, UP_DT_F32, plan) */
int up_unipose_lstm_plan_create_t(const up_unipose_lstm_config* cfg, int dtype, up_unipose_lstm_plan** plan);
int up_unipose_lstm_plan_dtype(const up_unipose_lstm_plan* plan);      /* UP_DT_F32 / UP_DT_BF16; UP_ERR_INVALID for NULL */
int up_unipose_lstm_plan_create_ex(const up_unipose_lstm_config* cfg, int dtype, int flags, up_unipose_lstm_plan** plan);
int up_unipose_lstm_plan_flags(const up_unipose_lstm_plan* plan);      /* 0 / UP_PLAN_FLIP_ONE_PASS; UP_ERR_INVALID for NULL */
void up_unipose_lstm_plan_destroy(up_unipose_lstm_plan* plan);
int up_unipose_lstm_plan_num_convs(const up_unipose_lstm_plan* plan);
const char* up_unipose_lstm_plan_conv_name(const up_unipose_lstm_plan* plan, int i);
int up_unipose_lstm_plan_conv_shape(const up_unipose_lstm_plan* plan, int i, int32_t* oihw /* [4] */, int32_t* has_bias);
int up_unipose_lstm_plan_set_conv(up_unipose_lstm_plan* plan, int i, const float* w_oihw, const float* bias, void* stream);
size_t up_unipose_lstm_plan_workspace(const up_unipose_lstm_plan* plan);
int up_unipose_lstm_step(up_unipose_lstm_plan* plan, const float* x_nchw, const float* center_nchw, const float* prev_hide,
                         const float* prev_cell, float* heat_nchw, float* cell_nchw, float* hide_nchw, void* workspace,
                         size_t workspace_bytes, void* stream);
int up_unipose_lstm_clip(up_unipose_lstm_plan* plan, const float* x, const float* center, float* heat, float* cell_last,
                         float* hide_last, void* workspace, size_t workspace_bytes, void* stream);
size_t up_unipose_lstm_plan_flip_workspace(const up_unipose_lstm_plan* plan);
size_t up_unipose_lstm_plan_program_workspace(const up_unipose_lstm_plan* plan, int program);
size_t up_unipose_lstm_plan_state_bytes(const up_unipose_lstm_plan* plan);
int up_unipose_lstm_clip_keypoints(up_unipose_lstm_plan* plan, const float* x, const float* center, int out_h, int out_w, int32_t* idx,
                                   float* preds_xy, float* maxvals, float* cell_last, float* hide_last, void* workspace,
                                   size_t workspace_bytes, void* stream);
int up_unipose_lstm_clip_flip(up_unipose_lstm_plan* plan, const float* x, const float* center, const int32_t* perm_host, float* heat,
                              void* workspace, size_t workspace_bytes, void* stream);
int up_unipose_lstm_clip_final_preds(up_unipose_lstm_plan* plan, const float* x, const float* center, const int32_t* perm_host,
                                     const double* inv, int res0, int res1, float* preds_xy, float* coords_xy, float* maxvals,
                                     void* workspace, size_t workspace_bytes, void* stream);
int up_unipose_lstm_stream_keypoints(up_unipose_lstm_plan* plan, const float* x_nchw, const float* center_nchw, void* state, int first,
                                     int out_h, int out_w, int32_t* idx, float* preds_xy, float* maxvals, float* heat_nchw,
                                     void* workspace, size_t workspace_bytes, void* stream);
int up_unipose_lstm_clip_frame_heatmaps(up_unipose_lstm_plan* plan, const void* src_hwc, int src_type, int F, int Hs, int Ws,
                                        const int32_t* frame_of, const int32_t* valid_hw, const double* crop_inv, float border,
                                        float mean, float stdv, const double* center_xy, double sigma, const int32_t* perm_host,
                                        float* heat, float* cell_last, float* hide_last, void* workspace, size_t workspace_bytes,
                                        void* stream);
int up_unipose_lstm_clip_frame_final_preds(up_unipose_lstm_plan* plan, const void* src_hwc, int src_type, int F, int Hs, int Ws,
                                           const int32_t* frame_of, const int32_t* valid_hw, const double* crop_inv, float border,
                                           float mean, float stdv, const double* center_xy, double sigma, const int32_t* perm_host,
                                           const double* inv, int res0, int res1, float* preds_xy, float* coords_xy, float* maxvals,
                                           void* workspace, size_t workspace_bytes, void* stream);
int up_unipose_lstm_stream_frame_final_preds(up_unipose_lstm_plan* plan, const void* src_hwc, int src_type, int F, int Hs, int Ws,
                                             const int32_t* frame_of, const int32_t* valid_hw, const double* crop_inv, float border,
                                             float mean, float stdv, const double* center_xy, double sigma, void* state, int first,
                                             const double* inv, int res0, int res1, float* preds_xy, float* coords_xy, float* maxvals,
                                             float* heat_nchw, void* workspace, size_t workspace_bytes, void* stream);

/* Many independent streams in ONE call (ABI 10 additions).  The stream entries above take one `first` flag and one state buffer for
 * the whole batch, so their B samples must start together and never restart.  The two entries below are those entries for a batch
 * whose samples are in different phases: the state lives in a caller-owned POOL of `slots` per-stream records (layout and tables:
 * up_lstm_state_gather / up_lstm_serve_fwd above; here rows_per_sample = h * w, ldo = rup4(K+2), the record stride rounded up to 256
 * bytes; the pool is up_unipose_lstm_plan_pool_bytes(plan, slots) bytes, 256-byte aligned, and may start as uninitialised memory),
 * and each call names, per sample b of the plan's batch, slot_host[b] (the record of its stream, or -1 for an idle lane) and
 * first_host[b] (!= 0: the stream starts or restarts with this frame).  Both tables are host memory, read before the call returns.
 *   up_unipose_lstm_serve_keypoints          up_unipose_lstm_stream_keypoints: x_nchw, center_nchw, the grid and the outputs as there.
 *   up_unipose_lstm_serve_frame_final_preds  up_unipose_lstm_stream_frame_final_preds: the crop, centre and way-back arguments as there.
 * THE RESULT, by definition: lane b of a call (its preds_xy / maxvals / idx / coords_xy / heat_nchw rows) equals, bit for bit, lane b
 * of this plan's own stream entry at the same batch on the same inputs — called with first != 0 for a first or idle lane; for a
 * continuing lane with first == 0 and a state buffer that holds that stream's state in lane b (the other lanes anything finite, e.g.
 * zeros).  The record of slot_host[b] >= 0 after the call equals lane b of the state buffer after that stream call: hide rows, then
 * cell rows, the pad lanes +0.0f.  Records of slots the table does not name keep every byte; for an idle lane nothing is written.
 * It is lane b, not any lane: a convolution's tail-tile K-split makes a row's summation order depend on its position in the batch, so
 * the same stream served in another lane may differ in the last bits (as it does between two batch sizes).
 * The launches: the trunk, hand-over and centre pooling of the stream programs, then BOTH gate convolutions at the plan's batch (the
 * lstm_0 one skipped when no sample is first or idle; the copy of z, the gather and the lstm one skipped when none continues), one
 * up_lstm_state_gather straight into the gate convolution's input, one up_lstm_serve_fwd, the head and the ending.  No flip test
 * inside a stream; UP_PLAN_FLIP_ONE_PASS changes nothing here.  Both storages.
 * Workspace: up_unipose_lstm_plan_program_workspace(plan, UP_PROGRAM_SERVE + 0) for _serve_keypoints, + 1 for
 * _serve_frame_final_preds (0 for any other k); no other figure of the plan changes.
 * Refused before anything is launched, outputs and pool untouched: a plan of batch > UP_SERVE_CAP (UP_ERR_UNSUPPORTED, from these
 * entries only), a NULL or misaligned pool, slots < 1, a slot outside -1 .. slots-1, the same slot >= 0 twice, NULL tables, and
 * everything the stream entry refuses (unset weights, a too-small workspace: UP_ERR_WORKSPACE). */
enum { UP_PROGRAM_SERVE = 512 };
size_t up_unipose_lstm_plan_pool_bytes(const up_unipose_lstm_plan* plan, int slots);   /* 0 for NULL or slots < 1 */
int up_unipose_lstm_serve_keypoints(up_unipose_lstm_plan* plan, const float* x_nchw, const float* center_nchw, void* pool, int slots,
                                    const int32_t* slot_host, const int32_t* first_host, int out_h, int out_w, int32_t* idx,
                                    float* preds_xy, float* maxvals, float* heat_nchw, void* workspace, size_t workspace_bytes,
                                    void* stream);
int up_unipose_lstm_serve_frame_final_preds(up_unipose_lstm_plan* plan, const void* src_hwc, int src_type, int F, int Hs, int Ws,
                                            const int32_t* frame_of, const int32_t* valid_hw, const double* crop_inv, float border,
                                            float mean, float stdv, const double* center_xy, double sigma, void* pool, int slots,
                                            const int32_t* slot_host, const int32_t* first_host, const double* inv, int res0, int res1,
                                            float* preds_xy, float* coords_xy, float* maxvals, float* heat_nchw, void* workspace,
                                            size_t workspace_bytes, void* stream);

/* ---- measurement hooks (bench.py roofline leg; no reference counterpart) ----
 * Between begin/end every MFMA convolution launch is bracketed by two hipEvents on its stream;
 * end() returns per kernel variant {launches, total ms, total algorithmic FLOP}. */
int up_profile_variants(void);
const char* up_profile_variant_name(int i);
int up_profile_begin(void);
int up_profile_enable(int on);   /* pause / resume recording between begin and end (sampled profiling) */
int up_profile_end(double* out, int variants);
/* per variant: FLOP of the collection up_profile_end just closed with dilated launches charged for their live (pixel, tap) pairs only */
int up_profile_live_flops(double* out, int variants);

#ifdef __cplusplus
}
#endif
#endif /* UNIPOSE_HIP_H */
