/*
 * pafuse_hip.h - C ABI of the MI355X (gfx950) implementation of the PAFUSE hot path:
 * the D3DP DDIM denoising loop over three per-body-part MixSTE spatio-temporal transformers.
 *
 * Every entry point takes plain device pointers, sizes and a HIP stream (as void*); no torch types.
 * All tensors are dense row-major fp32 in device memory unless stated; "t" vectors are int64.
 * Return value: 0 on success, a negative PAFUSE_E_* code otherwise (pafuse_last_error() has the text).
 * Nothing here allocates, synchronises or touches the default stream: launches go to `stream` only, scratch
 * comes from the caller's workspace, so every call can be captured into a hipGraph.
 *
 * Reference interface each entry point replaces (paths relative to valeoai/PAFUSE):
 *   pafuse_linear            torch.nn.Linear (+ nn.GELU) as used in common/mixste.py:30-43,54,57
 *   pafuse_layernorm         torch.nn.LayerNorm as used in common/mixste.py:96,101,203-204,208
 *   pafuse_attention         Attention.forward between qkv and proj, common/mixste.py:65-79
 *   pafuse_block_forward     Block.forward, common/mixste.py:113-116
 *   pafuse_attention_backward, pafuse_linear_weight_grad   the backward of the two above as torch autograd derives it
 *                            (unit entries of the training step's kernels; with pafuse_layernorm_backward,
 *                            pafuse_linear_input_grad, pafuse_linear_train, pafuse_gelu_backward; the first and last
 *                            layers: pafuse_train_head_grad, pafuse_train_patch_grad, pafuse_train_group_sum,
 *                            pafuse_train_sinusoid)
 *   pafuse_time_embed        MixSTE2.time_mlp, common/mixste.py:127-139,179-184
 *   pafuse_mixste2_forward   MixSTE2.forward (is_train=False), common/mixste.py:278-298
 *   pafuse_d3dp_sample       D3DP.ddim_sample_flip / ddim_sample, common/diffusionpose.py:227-316
 *                            (with model_predictions[_fliping] :174-225, pred_parts/split_data :163-172,328-335)
 *   pafuse_embed             the input stage of model_predictions_fliping + split_data + the first lines of
 *                            MixSTE2.STE_forward: common/diffusionpose.py:193-198,328-335, common/mixste.py:227-235
 *   pafuse_embed_unit        the same stage in each output form the loop launches (folded LayerNorm, images, row windows)
 *   pafuse_ddim_finalize     the output stage of a DDIM step: part concat + un-flip + TTA mean + clamp
 *                            (common/diffusionpose.py:165-171,211-218), epsilon in fp64 (:157-161,222-223), update (:302-312)
 *   pafuse_hypothesis_errors the per-joint part of evaluate()'s aggregation, main_h3wb.py:327-362
 *   pafuse_hypothesis_partials / _combine  the same from per-shard partial reductions (sharded or chunked P)
 *   pafuse_pose_partials / _combine  the P-Agg / J-Agg aggregates as poses, from shards or chunks of P (no ground truth)
 *   pafuse_pose_partials_fit the same state without a trajectory: the root of every hypothesis fitted from the detections
 *   pafuse_pose_path         J-Agg coherent in time: per joint a path through the hypotheses of a clip (Viterbi along the frames)
 *   pafuse_frames_path       the same path along a whole VIDEO: the candidates of a frame are the hypotheses of all windows covering it
 *   pafuse_spread_partials / _combine  the spread of the hypotheses beside the P-Agg mean: per-joint covariance and std
 *   pafuse_pose_windows_fold / pafuse_spread_windows_fold / pafuse_frames_finish  those states of overlapping windows
 *                            pooled into one pose (and spread) per video frame
 *   pafuse_frames_root_fit / pafuse_trajectory_smooth  the camera-space root of that per-frame pose, fitted from the
 *                            detections, and a confidence-weighted local-linear filter along the frames
 *   pafuse_detections_repair missing 2-D detections filled along the frames by that filter, per joint, a hand or face joint
 *                            relative to the joint it hangs on - the input side, before lifting
 *   pafuse_detections_screen observed detections screened in front of it: outliers against a leave-one-out local line rejected
 *                            by a robust per-joint scale, left/right swaps exchanged back
 *   pafuse_tracks_links / _path / _gather  in front of both: the K unordered candidate detections of every frame (all of
 *                            frame["predictions"], of which in_the_wild/h3wb_diffusion.py:65 takes entry 0) linked along the
 *                            frames into per-person videos
 *   pafuse_frames_focal_sums / pafuse_focal_solve  the focal length that fit needs, estimated from the same pose and
 *                            detections: one value per video, with the fraction of the signal it explains
 *   pafuse_foot_contacts / pafuse_ground_sums / pafuse_ground_solve / pafuse_frames_to_world  behind that fit: which way is
 *                            up - the ground plane through the foot points that do not move, and the poses in world space
 *                            (in place of the demo camera's fixed rotation, in_the_wild/h3wb_diffusion.py)
 *   pafuse_frame_errors / pafuse_frame_errors_reduce  that per-frame pose and root scored against ground truth: position,
 *                            velocity (mean_velocity_error, common/loss.py:488-497), acceleration, root and part-based errors
 *   pafuse_procrustes_errors the Protocol #2 part of it (ft2d.p2), main_h3wb.py:381-395, common/loss.py:251-458
 *   pafuse_procrustes_partials / _combine  Protocol #2 from per-shard partial states (sharded or chunked P)
 *   pafuse_mixste2_train_*   MixSTE2.forward (is_train=True) + autograd backward, common/mixste.py:215-225,260-298
 *   pafuse_d3dp_qsample      D3DP.prepare_diffusion_concat / q_sample, common/diffusionpose.py:319-326,358-374
 */
#ifndef PAFUSE_HIP_H
#define PAFUSE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PAFUSE_OK 0
#define PAFUSE_E_ARG (-1)       /* null pointer / bad size */
#define PAFUSE_E_SHAPE (-2)     /* a width this build has no kernel for */
#define PAFUSE_E_WORKSPACE (-3) /* workspace too small */
#define PAFUSE_E_HIP (-4)       /* a HIP launch failed */
#define PAFUSE_E_RANGE (-5)     /* pafuse_d3dp_check_range: a denoiser output was not finite ('f16x2': an activation left the fp16 range) */

#define PAFUSE_MAX_DEPTH 16
#define PAFUSE_MAX_PARTS 4

/* Parameters of one transformer block; names follow the reference state dict
 * ({STE,TTE}blocks.<i>.{norm1,attn.qkv,attn.proj,norm2,mlp.fc1,mlp.fc2}.{weight,bias}). Linear weights are
 * [out,in] row-major exactly as torch stores them - nothing is re-packed. */
typedef struct pafuse_block_weights {
    const float *norm1_w, *norm1_b; /* [C] */
    const float *qkv_w, *qkv_b;     /* [3C,C], [3C] */
    const float *proj_w, *proj_b;   /* [C,C], [C] */
    const float *norm2_w, *norm2_b; /* [C] */
    const float *fc1_w, *fc1_b;     /* [H,C], [H]   (H = mlp hidden width, 2C by default) */
    const float *fc2_w, *fc2_b;     /* [C,H], [C] */
    /* split-precision modes only (pafuse_mixste2_weights.operand_bf16 == 2 or 3): the pre-split images of the four linear
     * weights, made by pafuse_split_weights from the fp32 tensors above with layout 2 (qkv, fc1), 1 (proj, fc2) -
     * mode 3: with PAFUSE_SPLIT_F16X2 - (a cache - remake after a weight changes); NULL otherwise */
    const void *qkv_ws, *proj_ws, *fc1_ws, *fc2_ws;
    /* split-precision modes, optional: LayerNorm folded into the GEMM that consumes it (qkv_lt and fc1_lt set, in every block
     * of a denoiser, or neither).  With them set, qkv_ws / fc1_ws must be the images of W (.) g - the weight scaled along its
     * input axis by norm1 / norm2's weight g - and
     *   qkv_lt[n] = sum_k beta_k W_nk + b_n     (norm1 -> qkv; fc1_lt likewise with norm2)
     * formed in fp64 and rounded once.  The whole-row kernels then store the residual stream CENTRED on its row mean
     * (x - mean(x): every reader of the stream is a LayerNorm or the residual add that feeds one, and LayerNorm does not see
     * a row's mean) and emit the row's (mean, rstd) instead of the normalised row; qkv / fc1 read the centred row and apply
     * rstd acc + lt in their epilogue: the same function as LN(x) W^T + b (common/mixste.py:113-116) with one [M,C] store
     * and one normalise pass less per whole-row launch, and nothing that cancels on rows whose mean is large against their
     * spread.  qkv_ls / fc1_ls (sum_k g_k W_nk: round 3's uncentred form) are not read any more; leave them NULL.
     * pafuse_block_forward ignores the fold (it is handed a normalised-input-free block). */
    const float *qkv_ls, *qkv_lt, *fc1_ls, *fc1_lt;
    /* split-precision mode, optional: the qkv projection and the attention of a block in ONE kernel (fqa_kernel: one
     * workgroup = whole sequences x one head; q, k, v never reach memory).  qkv_hs is the layout-2 image of the HEAD-MAJOR
     * qkv weight: for head h = 0 .. heads-1 the d rows of q_h, then zero rows up to DP, then k_h and v_h likewise
     * (DP = 32 for head dim d <= 32, else 48; [heads * 3 * DP, C] in all) - of W (.) g when the LayerNorm is folded;
     * qkv_hb [heads * 3 * DP] is the bias (folded: qkv_lt) in that row order (qkv_hl: round 3's uncentred term, not read - leave it NULL), zeros in the
     * padding.  Used when set and the sequence length has a fused form (L <= 48; in f16x2 mode L <= 80 at head dim <= 32:
     * the 68 joints of the face); otherwise, and for
     * pafuse_block_forward, the block runs qkv GEMM + attention from qkv_ws.  Same arithmetic per product and the same
     * attention as the two kernels. */
    const void *qkv_hs;
    const float *qkv_hb, *qkv_hl;
    /* f16x2 mode with the LayerNorm folded, optional: fc1 -> GELU -> fc2 (+ residual, + the LayerNorms behind it) of a block in
     * ONE kernel (hmlp_kernel: the hidden activations [M, 2C] stay in registers, common/mixste.py:37-43,115).  fc2_hp is the
     * PAFUSE_SPLIT_F16X2 image of fc2.weight with its columns (hidden units) re-ordered inside every group of 16:
     *   column 16 b + 8 h + i of the image = column 16 b + 8 (i >> 2) + 4 h + (i & 3) of the weight   (h = 0, 1; i = 0 .. 7)
     * - the order in which the first layer's accumulators hold a token's hidden units.  Used when set, the channel width is
     * 224 / 256 / 384, the hidden width 2C and the residual stream is kept as its H image only (keep_f32_residual == 0);
     * otherwise the block runs the two launches from fc1_ws / fc2_ws.  Same products, same K order between 16-deep steps. */
    const void *fc2_hp;
} pafuse_block_weights;

/* One MixSTE2 (common/mixste.py:141-210): F frames, J joints of this part, C channels, `depth` spatial +
 * `depth` temporal blocks, `heads` heads (C % heads == 0), mlp hidden = 2C unless mlp_hidden says otherwise. */
typedef struct pafuse_mixste2_weights {
    int32_t frames, joints, channels, depth, heads, in_chans; /* in_chans must be 5 (2-D + 3-D) */
    int32_t operand_bf16; /* matrix-product mode of the linear layers (LayerNorm, softmax and the attention arithmetic are fp32 in
                             every mode, and so is everything in memory except the operand images of modes 3 and 4;
                             pafuse_amd.D3DP's default is 2):
                             0: fp32-input matrix cores (v_mfma_f32_32x32x2_f32): a k-ordered fp32 FMA chain.
                             2: split precision "bf16x3": every fp32 operand is the exact sum of three bf16 slices,
                                products keep the six terms above 2^-24 relative on the bf16 matrix cores with fp32
                                accumulation - fp32-equivalent results (closer to exact arithmetic than the FMA
                                chain) at 2.7x the matrix rate.  Inference entry points need the *_ws weight images;
                                the training entry points do not (weights change every step: each pass makes the images
                                of its weights itself, in one launch) and run every GEMM of the step this way.
                             3: split precision "f16x2" (inference only): activations as two fp16 slices, weights as two
                                stored + one derived (PAFUSE_SPLIT_F16X2 images in *_ws), three products per k on the fp16
                                matrix cores - fp32-equivalent results at 5.3x the fp32 matrix rate.
                             4: split precision "bf16x3" on the image pipeline (round 5, inference only, opt-in: it measures
                                85 hypotheses/s against mode 2's 100): the arithmetic of mode 2 - every operand the exact sum of three bf16 slices,
                                the six products above 2^-24 relative, fp32 accumulation - with both GEMM operands as pre-split
                                "X images" (PAFUSE_SPLIT_X images in *_ws / qkv_hs; activations split once by their producer),
                                qkv + attention fused in every block (qkv_hs, qkv_hb required), and - with the LayerNorm
                                folded - the residual stream kept only as the X image of x - mean(row): exactly that fp32 row.
                                Widths 224 / 256 / 384, sequence lengths <= 80 (head dim <= 32) / <= 32 (head dim <= 48).
                             1: opt-in reduced precision - operands rounded to ONE bf16 (RNE), fp32 accumulate
                                (BASELINE configs[1]; inference only) */
    int32_t mlp_hidden;   /* MixSTE2(mlp_ratio=...): hidden width int(C * mlp_ratio) of every block's MLP, a multiple of 32,
                             at most 3C; 0 = 2C (PAFUSE: mlp_ratio = 2, common/diffusionpose.py:146).  Inference only. */
    float qk_scale;       /* MixSTE2(qk_scale=...): attention logit scale; 0 = head_dim^-0.5 (common/mixste.py:52).
                             Inference only.  (qkv_bias=False: point qkv_b at zeros.) */
    int32_t keep_f32_residual; /* operand_bf16 == 3 with the LayerNorm folded: 0 (default) keeps the residual stream between the
                             blocks in memory ONLY as its H image - of x - mean(row): every reader of the stream is a LayerNorm or
                             the residual add that feeds one, so a row's mean never reaches the output and is not carried - as
                             hi + 2^-11 lo (22-23 significant bits); the whole-row kernels read it as the residual and write it
                             back in place (a quarter of their HBM traffic less); 1 also keeps the fp32 rows and adds those. */
    const float *patch_w, *patch_b;                           /* Spatial_patch_to_embedding [C,5], [C] */
    const float *pos_spatial;                                 /* Spatial_pos_embed [J,C] */
    const float *pos_temporal;                                /* Temporal_pos_embed [F,C] */
    const float *tm1_w, *tm1_b, *tm3_w, *tm3_b;               /* time_mlp.1 [2C,C],[2C]; time_mlp.3 [C,2C],[C] */
    const float *freqs;                                       /* [C/2] sinusoid frequencies (mixste.py:134-136) */
    const float *snorm_w, *snorm_b, *tnorm_w, *tnorm_b;       /* Spatial_norm, Temporal_norm (eps 1e-6) */
    const float *hnorm_w, *hnorm_b;                           /* head.0 LayerNorm (eps 1e-5) */
    const float *head_w, *head_b;                             /* head.1 [3,C], [3] */
    pafuse_block_weights ste[PAFUSE_MAX_DEPTH];
    pafuse_block_weights tte[PAFUSE_MAX_DEPTH];
} pafuse_mixste2_weights;

/* Everything D3DP's sampler needs besides the tensors (common/diffusionpose.py:59-155). */
typedef struct pafuse_d3dp_config {
    int32_t num_parts;                 /* 3: body, face, hands (iteration order = concat order) */
    int32_t num_kps;                   /* 134 */
    int32_t frames;                    /* 27 */
    int32_t flip;                      /* 1: ddim_sample_flip, 0: ddim_sample */
    double scale;                      /* args.ft2d.scale (a Python float in the reference: the clamp bound is
                                          (float)(1.1 * scale) formed in fp64, multiplier / divisor are (float)scale,
                                          exactly as torch demotes Python scalars against fp32 tensors) */
    pafuse_mixste2_weights part[PAFUSE_MAX_PARTS];
    const int32_t *part_joints[PAFUSE_MAX_PARTS]; /* device: joint indices of each part (split_data) */
    const int32_t *joint_part;         /* device [num_kps]: part id of every joint */
    const int32_t *joint_local;        /* device [num_kps]: index of the joint inside its part */
    const int32_t *flip_perm;          /* device [num_kps]: flipped[j] = orig[perm[j]] (diffusionpose.py:197-198) */
    int32_t part_by_part_launches;     /* launch-schedule option of the single-stream bf16x3 schedule (no aux streams): 0 (default) runs
                                          the same layer of the independent body-part denoisers in ONE grid (grouped_*_kernel), 1 launches
                                          every layer part by part.  A tile's arithmetic does not depend on the grid it runs in, so both
                                          give the same bits (tests/test_hip_fullsize.py); it exists for that test and for A/B timing.
                                          Per call: the library keeps no process-wide schedule state and reads no environment variable. */
} pafuse_d3dp_config;

/* Per-step scalars of the loop, computed by the host exactly as the reference does in fp64
 * (common/diffusionpose.py:157-161, 302-306). */
typedef struct pafuse_ddim_step {
    int64_t time;                /* timestep fed to the denoisers */
    int32_t last;                /* 1 when time_next < 0: img = x_start, no update */
    double sqrt_recip_acp;       /* sqrt_recip_alphas_cumprod[time] */
    double sqrt_recipm1_acp;     /* sqrt_recipm1_alphas_cumprod[time] */
    double sqrt_alpha_next, c, sigma;
} pafuse_ddim_step;

const char *pafuse_version(void);
const char *pafuse_last_error(void);
/* Layout version of the structs above (bumped whenever a field is added, moved or removed: this header has no size fields).
 * A caller built against another header gets shifted pointers, not an error - compare with PAFUSE_ABI_VERSION at load time
 * (pafuse_amd/_lib.py does; tests/cabi/linear_smoke.c shows the C side). */
#define PAFUSE_ABI_VERSION 8
int pafuse_abi_version(void);

/* out[M,N] = act(A[M,K] @ W[N,K]^T + bias), act: 0 none, 1 exact-erf GELU; +2: bf16 operands (see operand_bf16).
 * K,N multiples of 32. */
int pafuse_linear(const float *A, const float *W, const float *bias, float *out, int64_t M, int32_t N, int32_t K,
                  int32_t act, void *stream);

/* Split-precision weight image: W [N,K] fp32 (K % 32 == 0) -> `out`, pafuse_split_weights_bytes(N, K) = 6*N*K bytes
 * ([K/c][N][6c B] with c = 32 or 16: per row and K chunk, sub-blocks of 8 k x 3 bf16 slices, laid out as the kernels'
 * LDS image).  `layout` names the layer the image is for - it decides c and the rotation of the sub-blocks inside a row:
 *   0  pafuse_linear_split without PAFUSE_LINEAR_QKV_IMAGE: the 32x32x16-MFMA plain kernel (mlp.fc1 until ABI 5)
 *   1  attn.proj, mlp.fc2: the whole-row kernels (c = 16 at the widths that have an LDS-DMA tile)
 *   2  attn.qkv, mlp.fc1: the 16x16x32-MFMA kernels (pafuse_block_weights.qkv_ws and - since ABI 6 - fc1_ws must be made with layout 2)
 * pafuse_linear_split is pafuse_linear on such an image (act: 0 none, 1 GELU, + PAFUSE_LINEAR_QKV_IMAGE when the image
 * has layout 2): the unit entry of the split-precision products, which replace the same nn.Linear call sites
 * (common/mixste.py:38-42,65,80). */
#define PAFUSE_LINEAR_QKV_IMAGE 2
size_t pafuse_split_weights_bytes(int64_t N, int64_t K);
/* the bytes pafuse_split_weights writes for `layout` (the layout bits + PAFUSE_SPLIT_F16X2 / PAFUSE_SPLIT_X): 6 N K for the
 * bf16x3 images, 4 N K + 256 for the f16x2 H image; pafuse_split_weights_bytes (6 N K) is large enough for every layout */
size_t pafuse_split_image_bytes(int64_t N, int64_t K, int32_t layout);
int pafuse_split_weights(const float *W, int32_t N, int32_t K, int32_t layout, void *out, void *stream);
int pafuse_linear_split(const float *A, const void *Wsplit, const float *bias, float *out, int64_t M, int32_t N,
                        int32_t K, int32_t act, void *stream);

/* Second split-precision scheme, "f16x2" (operand_bf16 == 3, round 4): THREE fp16 MFMA products per fp32-equivalent product.
 * Both GEMM operands are "H images": rows of 4 K bytes, per sub-block of 8 k the 16 bytes of the first fp16 slice, then the
 * 16 of the second - [rows][K/8][hi 8 x f16 | lo 8 x f16]:
 *   activation a   hi = f16(a), lo = f16((a - hi) * 2^11); written in this form by the kernel that PRODUCES the tensor
 *                  (whole-row epilogues, attention, the fc1 epilogue, the embedding) - same bytes as fp32, split once;
 *   weight W       pafuse_split_weights(W, N, K, PAFUSE_SPLIT_F16X2, out, stream): the image of Ws = 2^k W (the tensor's
 *                  largest |Ws| in [2^14, 2^15)): w0 = f16(Ws), w1 = f16(Ws - w0); 4 N K bytes + a 256-byte tail whose
 *                  first float is 2^-k (a buffer of pafuse_split_weights_bytes(N, K) bytes is large enough); every layer
 *                  uses this one geometry, whatever the value of the layout bits.
 * Kept per product: hi w0 + hi w1 + lo (w0 2^-11), fp32 accumulate, the accumulator times 2^-k in the epilogue; dropped
 * terms and slice roundings ~ 2^-22 relative.  fp32-equivalent: the same bounds against exact arithmetic as bf16x3 hold
 * (tests/test_hip_parity.py).  Activations must stay below 65504 in magnitude (beyond it hi is inf and the affected outputs
 * are inf / NaN, never silently wrong).  Inference only; channel widths 224 / 256 / 384, plain-layer widths that are
 * multiples of 128 or 224.
 * pafuse_hsplit_rows: X [R,K] fp32 -> its activation H image (4 R K bytes).  pafuse_linear_h: nn.Linear on H images
 * (act: 0 none, 1 GELU): fp32 `out` [M,N], or - when out_h is given - the H image of the output instead (either may be
 * NULL, not both).  N a multiple of 128 or 224, K of 32.  Replaces the same nn.Linear call sites (common/mixste.py:38-42,65,80). */
#define PAFUSE_SPLIT_F16X2 4

/* The bf16x3 scheme on the image pipeline (operand_bf16 == 4, round 5): the products of mode 2, both operands as "X images" -
 * rows of 6 K bytes (K % 32 == 0), per chunk of 32 k the 32 bf16 of slice 0, then of slice 1, then of slice 2:
 * [rows][K/32][3][32 x bf16].  x = s0 + s1 + s2 exactly (s0 = bf16(x), s1 = bf16(x - s0), s2 = bf16(x - s0 - s1), RNE, the
 * subtractions exact), so an X image IS the fp32 tensor, bit for bit; no scaling, no range limit beyond fp32's, inf / NaN stay
 * inf / NaN (in every slice).
 *   weight W      pafuse_split_weights(W, N, K, PAFUSE_SPLIT_X, out, stream): 6 N K bytes = pafuse_split_weights_bytes(N, K);
 *                 one geometry for every layer, whatever the value of the layout bits;
 *   activation    written in this form by the kernel that PRODUCES the tensor; pafuse_xsplit_rows: X [R,K] fp32 -> its X image
 *                 (unit tests, pafuse_block_forward).
 * pafuse_linear_x: nn.Linear on X images (act: 0 none, 1 GELU): fp32 `out` [M,N], or - when out_x is given - the X image of the
 * output instead.  N a multiple of 128, 224 or 96, K of 32.  Replaces the same nn.Linear call sites (common/mixste.py:38-42,65,80). */
#define PAFUSE_SPLIT_X 8
int pafuse_xsplit_rows(const float *X, int64_t R, int32_t K, void *out, void *stream);
int pafuse_linear_x(const void *Ax, const void *Wx, const float *bias, float *out, void *out_x, int64_t M, int32_t N, int32_t K,
                    int32_t act, void *stream);

int pafuse_hsplit_rows(const float *X, int64_t R, int32_t K, void *out, void *stream);
int pafuse_linear_h(const void *Ah, const void *Wh, const float *bias, float *out, void *out_h, int64_t M, int32_t N, int32_t K,
                    int32_t act, void *stream);

/* qkv projection + attention of whole sequences in ONE kernel on operand images - the unit entry of hfqa_kernel (scheme
 * PAFUSE_SPLIT_F16X2: H images) and xfqa_kernel (PAFUSE_SPLIT_X: X images); common/mixste.py:65-79:
 *   (q | k | v)[m] = rstd_m * (x[m] W^T) + b   (rstd_m = stats[2 m + 1], stats NULL: 1 - with stats the image is the CENTRED row and
 *   W is W (.) g, b = W beta + b: the folded LayerNorm);   o[sequence, head] = softmax(q k^T * scale) v
 * x_img: the image of x [M,C]; qkv_hs / qkv_hb: the head-major weight image [heads * 3 * DP, C] and bias of
 * pafuse_block_weights.qkv_hs / qkv_hb; o_img: the image of o [M,C] (rows no sequence touches are left alone).  Sequence map as
 * pafuse_attention; qk_scale 0 = head_dim^-0.5.  Shapes with a fused form only (sequence length <= 80 at head dim <= 32, <= 32
 * at head dim <= 48; PAFUSE_SPLIT_X at head dim > 32: an even number of heads). */
int pafuse_qkv_attention_image(int32_t scheme, const void *x_img, const float *stats, const void *qkv_hs, const float *qkv_hb,
                               void *o_img, int64_t M, int64_t nseq, int32_t L, int32_t C, int32_t heads, int64_t group,
                               int64_t group_stride, int64_t seq_stride, int64_t tok_stride, float qk_scale, void *stream);

/* The MLP of a block on H images in one kernel (the unit entry of hmlp_kernel; common/mixste.py:37-43,115 with norm2 folded):
 *   y = xc + GELU(rstd * (xc W1^T) + bias1) W2^T + bias2,   xc = the rows of `xh` (the CENTRED image of the residual stream),
 *   rstd = stats_in[2 m + 1] (NULL: 1);  out_xh = the H image of y - mean(y),  stats_out[m] = (mean(y), 1 / sqrt(var(y) + eps)).
 * W1h: the PAFUSE_SPLIT_F16X2 image of fc1.weight [2C, C] (of W1 (.) g for a folded LayerNorm, bias1 = W1 beta + b1);
 * W2hp: the image of fc2.weight [C, 2C] in the column order of pafuse_block_weights.fc2_hp.  C = 224, 256 or 384.
 * out_xh may be xh itself (a workgroup owns its rows). */
int pafuse_mlp_h(const void *xh, const float *stats_in, const void *W1h, const float *bias1, const void *W2hp, const float *bias2,
                 void *out_xh, float *stats_out, int64_t M, int32_t C, float eps, void *stream);

/* The whole-row layers (attn.proj, mlp.fc2 with the residual add and the LayerNorm chain behind them, common/mixste.py:41,80,
 * 114-115,243,250,257) as unit entry points: the kernels pafuse_mixste2_forward / pafuse_d3dp_sample launch for them, picked by
 * the same dispatch.  Per row m of [M, N] (N = the channel width, the whole row):
 *   y  = A[m] W^T + bias + resid[m]                  (training: y = resid[m] + rowscale[seq(m)] (A[m] W^T + bias), out_pre = y)
 *   z  = post_w ? LN(y; post_w, post_b, post_eps) : y ;   z += pos[(m / posJ) % posF] if pos ;   out_x = z
 *   next_w set:  ln_stats NULL: n = LN(z; next) -> out_n, and with head_w: out_head[m] = n head_w^T + head_b  (head_w [3,N])
 *                ln_stats set (the LayerNorm folded into its consumer): ln_stats[m] = (mean(z), rstd(z)), out_x = z - mean(z)
 *                (the stored mean: the row and its statistics agree), no out_n
 * Every output pointer may be NULL (not written).  out_x may be resid itself (a workgroup owns its rows).
 * operand_bf16 as pafuse_mixste2_weights.operand_bf16:
 *   0, 1: W fp32.   2: Wsplit = the layout-1 image of W (pafuse_split_weights(W, N, K, 1, ..)).
 *   3, 4 (inference): A_img = the H / X image of A; Wsplit = the PAFUSE_SPLIT_F16X2 / PAFUSE_SPLIT_X image of W; the residual is
 *         fp32 `resid` or - resid_img - the (centred) image of it; out_x_img / out_n_img: the images of out_x / n (may alias
 *         resid_img).  Widths 224 / 256 / 384.
 *   training (EPI_ROWLN_TRAIN; modes 0 and 2, W always - shapes without a split tile run the fp32 kernels): rowscale [nseq] or
 *         NULL (= 1), seq(m) = rs_temporal ? (m / rs_FJ) rs_J + m % rs_J : m / rs_J; out_pre [M,N] or NULL.
 * Refused (PAFUSE_E_ARG): head without next, ln_stats without next or with the head, out_n with ln_stats, pos with posJ or
 * posF <= 0, a missing operand or image, training in modes 1, 3, 4 or in a group, n outside 1 .. 4; (PAFUSE_E_SHAPE): a width
 * without a whole-row kernel, K not a positive multiple of 32.  M == 0: nothing is launched.
 * pafuse_linear_rowln_group: n independent layers; shared_grid != 0 runs them in ONE grid where the grouped kernel has variants
 * for all of them (mode 2, widths 384 / 256 / 224 at M >= 4096 - the library's single-stream schedule), else one launch each. */
typedef struct pafuse_rowln_args {
    int64_t M;
    int32_t N, K;
    int32_t operand_bf16;
    int32_t training;
    const float *A;                 /* [M,K] (modes 0 - 2) */
    const float *W;                 /* [N,K] (modes 0, 1, training) */
    const void *Wsplit;             /* modes 2 - 4: the weight image */
    const float *bias;              /* [N] */
    const float *resid;             /* [M,N] */
    float *out_x, *out_n;           /* [M,N] */
    const float *post_w, *post_b;   /* [N] */
    float post_eps;
    const float *pos;               /* [posF, N] */
    int32_t posJ, posF;
    const float *next_w, *next_b;   /* [N] */
    float next_eps;
    const float *head_w, *head_b;   /* [3,N], [3] */
    float *out_head;                /* [M,3] */
    float *ln_stats;                /* [M,2] */
    const void *A_img;              /* modes 3, 4: [M,K] image */
    const void *resid_img;          /* modes 3, 4: [M,N] image of the (centred) residual, instead of resid */
    void *out_x_img, *out_n_img;    /* modes 3, 4: [M,N] images */
    const float *rowscale;          /* training */
    int32_t rs_temporal, rs_J, rs_FJ;
    float *out_pre;                 /* training: [M,N] */
} pafuse_rowln_args;
int pafuse_linear_rowln(const pafuse_rowln_args *a, void *stream);
int pafuse_linear_rowln_group(const pafuse_rowln_args *a, int32_t n, int32_t shared_grid, void *stream);

/* out[M,C] = LayerNorm(x[M,C]) * w + b  (biased variance, eps inside the sqrt). */
int pafuse_layernorm(const float *x, const float *w, const float *b, float *out, int64_t M, int32_t C, float eps,
                     void *stream);

/* o[M,C] = softmax(q k^T * d^-1/2) v per (sequence, head) on qkv[M,3C] laid out [.., 3, heads, d].
 * Sequence s (0..nseq) holds rows  (s / inner) * inner * L * tstride_outer ... described by:
 *   row(s, t) = (s / group) * group_stride + (s % group) * seq_stride + t * tok_stride
 * spatial: group=1, group_stride=L, seq_stride=0, tok_stride=1; temporal: group=J, group_stride=F*J,
 * seq_stride=1, tok_stride=J. */
int pafuse_attention(const float *qkv, float *o, int64_t nseq, int32_t L, int32_t C, int32_t heads, int64_t group,
                     int64_t group_stride, int64_t seq_stride, int64_t tok_stride, void *stream);

/* Unit entry points of the training step's backward kernels (round 5; the step itself is pafuse_mixste2_train_backward).
 * pafuse_attention_backward: dqkv[M,3C] from qkv[M,3C] and dO[M,C] - what autograd derives from common/mixste.py:66-79
 * (S = q k^T d^-1/2, P = softmax(S), O = P v:  dV = P^T dO, dP = dO V^T, dS = P (dP - rowsum(P dP)), dQ = dS K d^-1/2,
 * dK = dS^T Q d^-1/2), sequence map as pafuse_attention.  Rows no sequence touches are left alone.
 * pafuse_linear_weight_grad: dW[N,K] += dY[M,N]^T X[M,K] and, with db, db[N] += column sums of dY - the weight and bias
 * gradient of nn.Linear (common/mixste.py:30-43,54,57) as the training step forms them: operand_bf16 0 = fp32 matrix cores,
 * 2 = split (bf16x3) products on the large tiles where a PAFUSE width divides; partial sums in a fixed order (bit-reproducible).
 * workspace: pafuse_linear_weight_grad_bytes() bytes. */
int pafuse_attention_backward(const float *qkv, const float *d_o, float *dqkv, int64_t nseq, int32_t L, int32_t C, int32_t heads,
                              int64_t group, int64_t group_stride, int64_t seq_stride, int64_t tok_stride, void *stream);
size_t pafuse_linear_weight_grad_bytes(void);
int pafuse_linear_weight_grad(const float *dY, const float *X, float *dW, float *db, int64_t M, int32_t N, int32_t K,
                              int32_t operand_bf16, void *workspace, size_t workspace_bytes, void *stream);

/* More unit entry points of the training step: each calls the host function the step calls (train_host.inc).
 * pafuse_layernorm_backward (ln_backward): with xh = (x - mean) rstd, g = dy w:
 *   dx = add + rstd (g - mean(g) - xh mean(g xh))  (add NULL: 0; add may be dx itself, as the step's norm1 call passes it),
 *   out_scaled = drop[seq(m)] dx (drop NULL: 1; seq(m) = temporal ? (m / FJ) J + m % J : m / J),
 *   dw += sum_m dy xh, db += sum_m dy, dbranch += sum_m out_scaled (NULL: not formed; needs out_scaled).
 *   C % 4 == 0 and C <= 384: the half-wave kernel (16-byte accesses: dy, x, w, add, dx, out_scaled 16-byte aligned), else the
 *   one-wave-per-row kernel (C <= 768).
 * pafuse_linear_input_grad (input_grad): dX[M,K] = dY[M,N] W[N,K], times gelu'(dact_u[M,K]) when dact_u is given (the dX GEMM
 *   of mlp.fc2).  operand_bf16 0: W transposed, fp32 products; 2: split products on the M16 image of W^T where the step runs
 *   them (M >= 128), made by split_weights_transposed_kernel (image_source 0) or by the one-launch batch kernel the step uses
 *   (image_source 1).  dact_u: K % 64 == 0 unless the split route is taken.
 * pafuse_linear_train (plain_linear): u[M,N] = A[M,K] W[N,K]^T + bias, h = gelu(u) from the same epilogue (h NULL: not
 *   formed; h: N % 64 == 0 unless the split route is taken) - mlp.fc1 of the training forward, and the time MLP (M < 128).
 * pafuse_gelu_backward (gelu_bwd): du[M,N] = dh gelu'(u) (du may be dh), db[N] += column sums of du.  N % 4 == 0.
 * workspace: pafuse_train_unit_bytes(M, N, K) bytes, 16-byte aligned (layernorm_backward: N = C, K = 0; gelu_backward: K = 0).
 * Refused before any launch: a NULL operand, M < 0, a misaligned vector operand, a width outside the kernels' range, a mode
 * other than 0 / 2, a too-small workspace, dbranch without out_scaled, drop with J or FJ <= 0.  M == 0: nothing is launched. */
typedef struct pafuse_lnb_args {
    const float *dy, *x, *w;  /* [M,C], [M,C], [C] */
    float eps;
    const float *add;         /* [M,C] or NULL; may be dx */
    float *dx;                /* [M,C] */
    const float *drop;        /* [nseq] or NULL */
    int32_t temporal, J, FJ;  /* the sequence map of drop */
    float *out_scaled;        /* [M,C] or NULL */
    float *dw, *db, *dbranch; /* [C], added into; dbranch may be NULL */
    int64_t M;
    int32_t C;
} pafuse_lnb_args;
size_t pafuse_train_unit_bytes(int64_t M, int32_t N, int32_t K);
int pafuse_layernorm_backward(const pafuse_lnb_args *a, void *workspace, size_t workspace_bytes, void *stream);
int pafuse_linear_input_grad(const float *dY, const float *W, const float *dact_u, float *dX, int64_t M, int32_t N, int32_t K,
                             int32_t operand_bf16, int32_t image_source, void *workspace, size_t workspace_bytes, void *stream);
int pafuse_linear_train(const float *A, const float *W, const float *bias, float *u, float *h, int64_t M, int32_t N, int32_t K,
                        int32_t operand_bf16, void *workspace, size_t workspace_bytes, void *stream);
int pafuse_gelu_backward(const float *u, const float *dh, float *du, float *db, int64_t M, int32_t N, void *workspace,
                         size_t workspace_bytes, void *stream);

/* Unit entry points of the gradients at the rim of the training step - the output head, the patch embedding, the position and
 * time embeddings - and of the sinusoid in front of the time MLP: each calls the host function the step calls (train_host.inc).
 * Gradient outputs are ADDED INTO (as the step accumulates into its gradient struct), except dhn and dtemb, which are OVERWRITTEN.
 * pafuse_train_head_grad (head_grad): out = hn head_w^T + head_b with dout [M,3], hn [M,C], head_w [3,C]:
 *   d_head_w [3,C] += dout^T hn,  d_head_b [3] += column sums of dout,  dhn [M,C] = dout head_w.
 * pafuse_train_patch_grad (concat_inputs, patch_grad): x0 = (x2d | x3d) patch_w^T + patch_b + pos_spatial[j] + temb[b] with
 *   x2d [B,F,J,2], x3d [B,F,J,3], g = d x0 [B,F,J,C]:  d_patch_w [C,5] += g^T (x2d | x3d),  d_patch_b [C] += column sums of g,
 *   d_pos_spatial [J,C] += sums of g over (b, f),  dtemb [B,C] = sums of g over (f, j).
 * pafuse_train_group_sum (group_sum): out [G,C] = (accumulate 1: out +) sums of x [B,F,J,C] over the rows of each group -
 *   mode 0: per joint (G = J, Spatial_pos_embed), 1: per frame (G = F, Temporal_pos_embed), 2: per sample (G = B, time embedding).
 * pafuse_train_sinusoid (sinusoid): out [B,C] = [sin(a) | cos(a)], a = (float)t[b] * freqs[k] in fp32, freqs [C/2]
 *   (common/mixste.py:132-138); C even.
 * workspace: the entry's own ..._bytes query (0 for arguments the entry refuses).  Partial sums are joined in a fixed order
 * (bit-reproducible).  Refused before any launch: a NULL operand, a negative size, a mode outside 0 .. 2, an accumulate flag
 * other than 0 / 1, C < 1 (sinusoid: odd C), a too-small workspace.  No rows (M, or one of B, F, J, = 0): nothing is launched. */
size_t pafuse_train_head_grad_bytes(int64_t M, int32_t C);
int pafuse_train_head_grad(const float *dout, const float *hn, const float *head_w, float *d_head_w, float *d_head_b, float *dhn,
                           int64_t M, int32_t C, void *workspace, size_t workspace_bytes, void *stream);
size_t pafuse_train_patch_grad_bytes(int32_t B, int32_t F, int32_t J, int32_t C);
int pafuse_train_patch_grad(const float *x2d, const float *x3d, const float *g, float *d_patch_w, float *d_patch_b,
                            float *d_pos_spatial, float *dtemb, int32_t B, int32_t F, int32_t J, int32_t C, void *workspace,
                            size_t workspace_bytes, void *stream);
size_t pafuse_train_group_sum_bytes(int32_t mode, int32_t B, int32_t F, int32_t J, int32_t C);
int pafuse_train_group_sum(const float *x, float *out, int32_t mode, int32_t accumulate, int32_t B, int32_t F, int32_t J, int32_t C,
                           void *workspace, size_t workspace_bytes, void *stream);
int pafuse_train_sinusoid(const int64_t *t, const float *freqs, float *out, int32_t B, int32_t C, void *stream);

/* x[S*L,C] <- Block(x) in place for S contiguous sequences of L tokens (Block.forward, eps 1e-6).  operand_bf16: the
 * matrix-product mode of the four linear layers (as pafuse_mixste2_weights.operand_bf16; 2, 3 and 4 need the *_ws images of
 * their scheme, 4 also qkv_hs / qkv_hb). */
size_t pafuse_block_workspace_bytes(int64_t rows, int32_t C); /* 0 if a size is < 1 */
int pafuse_block_forward(const pafuse_block_weights *w, float *x, int64_t S, int32_t L, int32_t C, int32_t heads,
                         int32_t operand_bf16, void *workspace, size_t workspace_bytes, void *stream);

/* temb[B,C] = time_mlp(t[B]);  hid_scratch: [B,2C] floats of device scratch */
int pafuse_time_embed(const pafuse_mixste2_weights *w, const int64_t *t, int32_t B, float *temb, float *hid_scratch,
                      void *stream);

/* 1 when the inference kernels of matrix-product mode `mode` (pafuse_mixste2_weights.operand_bf16) exist for a denoiser of
 * channel width C, MLP hidden width `hidden` (0 = 2C), `heads` heads and sequences of `joints` / `frames` tokens, else 0 -
 * callers pick mode 4 where it is supported and mode 2 elsewhere (the single-model variant, width 288). */
int pafuse_mode_supported(int32_t mode, int32_t C, int32_t hidden, int32_t heads, int32_t joints, int32_t frames);

/* How many of the 2 * depth blocks of `w` will run qkv + attention as the one fused kernel (pafuse_block_weights.qkv_hs
 * set and the block's sequence length / head dim have a fused form); negative = an error code.  Callers and tests use
 * it to know which path a configuration takes. */
int pafuse_mixste2_fused_blocks(const pafuse_mixste2_weights *w);

/* MixSTE2.forward, eval: x2d[B,F,J,2], x3d[B,P,F,J,3], t[B] -> out[B,P,F,J,3]. */
size_t pafuse_mixste2_workspace_bytes(const pafuse_mixste2_weights *w, int32_t B, int32_t P); /* 0 if w is NULL or a size is < 1 */
int pafuse_mixste2_forward(const pafuse_mixste2_weights *w, const float *x2d, const float *x3d, const int64_t *t,
                           int32_t B, int32_t P, float *out, void *workspace, size_t workspace_bytes, void *stream);

/* The whole DDIM loop for B clips x P hypotheses and `nsteps` sampling steps.
 *   x2d, x2d_flip [B,F,J,2] (x2d_flip ignored when cfg->flip == 0)
 *   noise [n_draws,B,P,F,J,3]: draw 0 is the initial img, draw k the randn_like of the k-th update
 *         (n_draws >= 1 + number of steps with last == 0)
 *   out   [B,nsteps,P,F,J,3]: x_start of every step (torch.stack(preds_all, dim=1))
 * `aux_streams` (may be NULL / n_aux 0): extra HIP streams; a step's work is cut into (part, hypothesis-group) lanes,
 * one stream each, groups = (n_aux + 1) / parts (>= 1): 2 aux streams = the three parts side by side (fastest
 * measured; more lanes cost more in small launches than they gain in overlap).  Events are created and destroyed
 * inside the call only when aux streams are given.  The library must be built without packed-fp32 VALU instructions
 * for this (as __graft_entry__.build() does, -DPAFUSE_NO_PACKED_F32): beside v_mfma_f32_32x32x16_bf16 waves of another
 * queue a v_pk_*_f32 with a high-register src1 select returns wrong lanes on MI355X
 * (profiles/r03_bf16_mfma_concurrency.md).  A build without that flag ignores the aux streams when any part runs a
 * bf16-MFMA mode (operand_bf16 != 0) and pafuse_d3dp_lanes returns 1. */
size_t pafuse_d3dp_workspace_bytes(const pafuse_d3dp_config *cfg, int32_t B, int32_t P); /* 0 if cfg is NULL or a size is < 1 */
int pafuse_d3dp_sample(const pafuse_d3dp_config *cfg, const pafuse_ddim_step *steps, int32_t nsteps,
                       const float *x2d, const float *x2d_flip, const float *noise, int32_t n_draws, int32_t B,
                       int32_t P, float *out, void *workspace, size_t workspace_bytes, void *stream,
                       void *const *aux_streams, int32_t n_aux);

/* pafuse_d3dp_sample with the loop's noise drawn inside its own kernels from "noise stream v1"  instead
 * of read from a [n_draws,B,P,F,J,3] stack: draw k (0 = the initial img, k >= 1 = the update after step k - 1) of global clip b,
 * global hypothesis p, frame f, joint j is
 *   (r0..r3) = Philox4x32-10(counter (f*J + j, p, b, k), key (seed, call));   u(r) = (r + 0.5) * 2^-32
 *   x = sqrt(-2 ln u(r0)) cos(2 pi u(r1)),  y = sqrt(-2 ln u(r0)) sin(2 pi u(r1)),  z = sqrt(-2 ln u(r2)) cos(2 pi u(r3))
 * evaluated in fp64 and rounded once to fp32 (host statement: pafuse_amd/noise.py).  key4_dev: four uint32 IN DEVICE MEMORY,
 * {seed, call, b0, p0}, read by the kernels when they run - b0 / p0 are the global indices of this call's first clip / first
 * hypothesis, so a call on clips [b0, b0 + B) and hypotheses [p0, p0 + P) returns that slice of the full call, and a captured
 * graph is replayed with other words after a 16-byte copy.  Everything else as pafuse_d3dp_sample (same workspace, same lanes);
 * the arithmetic that consumes the normals is the same, so the result equals pafuse_d3dp_sample on the pafuse_noise_fill
 * tensors of the same key, bit for bit. */
int pafuse_d3dp_sample_seeded(const pafuse_d3dp_config *cfg, const pafuse_ddim_step *steps, int32_t nsteps,
                              const float *x2d, const float *x2d_flip, const uint32_t *key4_dev, int32_t B, int32_t P,
                              float *out, void *workspace, size_t workspace_bytes, void *stream,
                              void *const *aux_streams, int32_t n_aux);

/* Draw `draw` of noise stream v1 for B clips x P hypotheses of F frames x J joints as a tensor: out [B,P,F,J,3].
 * key4_dev as above (device memory). */
int pafuse_noise_fill(const uint32_t *key4_dev, int32_t draw, int32_t B, int32_t P, int32_t F, int32_t J, float *out,
                      void *stream);

/* Loud failure through the loop.  pafuse_d3dp_sample keeps one int32 in its workspace (byte offset pafuse_d3dp_range_flag_offset,
 * zeroed at the start of every call) that the output stage of every step sets when a denoiser prediction is not finite.  The
 * values themselves flow on as NaN - the clamps of the loop keep a NaN a NaN, exactly as torch.clamp does
 * (common/diffusionpose.py:193,216-217) - so an 'f32' / 'bf16x3' run returns what the reference returns.  In 'f16x2' a non-finite
 * prediction is how an activation beyond the fp16 range shows (|a| >= 65504: its high slice is inf): callers of that mode ask
 * pafuse_d3dp_check_range after the call - the ONE entry point of this library that synchronises (`stream`) - and get
 * PAFUSE_E_RANGE; pafuse_amd.D3DP raises.  (Inside a stream capture, read the word yourself after the replay.) */
size_t pafuse_d3dp_range_flag_offset(const pafuse_d3dp_config *cfg, int32_t B, int32_t P);
int pafuse_d3dp_check_range(const pafuse_d3dp_config *cfg, int32_t B, int32_t P, const void *workspace, void *stream);

/* Number of distinct HIP streams pafuse_d3dp_sample will launch on when handed `n_aux` aux streams (the caller's
 * stream + the first (result - 1) aux streams).  A caller that forks its aux streams into a stream capture must fork
 * exactly those: the library joins the streams it used, an extra forked stream would leave the capture unjoined. */
int pafuse_d3dp_lanes(const pafuse_d3dp_config *cfg, int32_t B, int32_t P, int32_t n_aux);

/* ---- the two index-carrying stages of a DDIM step as unit entry points (SURVEY.md 8b "finer ops") ---------------
 * pafuse_embed: input stage of one body part.  For every row (fl, b, p, f, j) of the part's token matrix
 * (fl < nflip; row = (((fl*B + b)*P + p)*F + f)*J + j):
 *   jj = joints ? joints[j] : j                      split_data's gather            diffusionpose.py:328-335
 *   v3 = x3d[b, p, f, fl ? perm[jj] : jj, :]         L/R swap of the flipped copy   diffusionpose.py:197-198
 *   if do_clamp: v3 = clamp(v3, +-1.1*scale) / scale                                diffusionpose.py:193-194
 *   if fl: v3.x = -v3.x                                                             diffusionpose.py:196
 *   v2 = (fl ? x2d_flip : x2d)[b, f, jj, :]          2-D input broadcast over P     mixste.py:228-229
 *   x[row]  = patch_w [v2, v3] + patch_b + pos_spatial[j] + temb[b]                 mixste.py:230-235
 *   xn[row] = LayerNorm(x[row]; norm_w, norm_b, norm_eps)                           (norm1 of the first block)
 * x3d [B,P,F,J3,3], x2d/x2d_flip [B,F,J3,2], joints int32 [J] (values < J3; NULL = identity, needs J3 == J),
 * perm int32 [J3] (needed when nflip == 2), patch_w [C,5], patch_b [C], pos_spatial [J,C], temb [B,C],
 * x / xn [nflip*B*P*F*J, C].  C % 4 == 0, C <= 384.  The index tables live on the device and are trusted. */
int pafuse_embed(const float *x3d, const float *x2d, const float *x2d_flip, const int32_t *joints, const int32_t *perm,
                 const float *patch_w, const float *patch_b, const float *pos_spatial, const float *temb,
                 const float *norm_w, const float *norm_b, float norm_eps, int32_t B, int32_t P, int32_t F, int32_t J,
                 int32_t J3, int32_t C, int32_t nflip, int32_t do_clamp, double scale, float *x, float *xn, void *stream);

/* pafuse_embed_unit: the same stage in every output form the sampling loop launches it in, for the rows [row0, row0 + nrows)
 * of the token matrix - through the one host function that maps (product mode, folded LayerNorm, H-residual-only) to the
 * kernel's outputs for pafuse_d3dp_sample, pafuse_mixste2_forward and pafuse_embed alike.  Operands as pafuse_embed; further:
 *   operand_bf16     as pafuse_mixste2_weights.operand_bf16.  3 / 4: the normalised (or centred) row is written as its H / X
 *                    image into `image` ([M,C] rows of 4 C / 6 C bytes) and xn is not written
 *   ln_folded        (modes 2 - 4) the LayerNorm is left to the qkv GEMM: stats[2 i] = (mean, rstd) of row row0 + i, no xn;
 *                    mode 2: x holds the CENTRED rows x - mean; modes 3 / 4: the image is that of the centred row, x stays plain
 *   h_residual_only  (modes 3 / 4, folded) the fp32 rows are not kept: x is not written (and may be NULL)
 * x, xn and image are indexed by the ABSOLUTE row (buffers of all M = nflip B P F J rows), stats by the LOCAL row (nrows pairs).
 * Refused before any launch: PAFUSE_E_ARG for what pafuse_embed refuses, a mode outside 0 .. 4, ln_folded in modes 0 / 1,
 * h_residual_only outside (modes 3 / 4, folded), a window that is empty or not inside [0, M), an output the form writes that
 * is NULL; PAFUSE_E_SHAPE for an H image at C % 8 != 0 or an X image at C % 32 != 0. */
typedef struct pafuse_embed_args {
    const float *x3d, *x2d, *x2d_flip;
    const int32_t *joints, *perm;
    const float *patch_w, *patch_b, *pos_spatial, *temb, *norm_w, *norm_b;
    float norm_eps;
    int32_t B, P, F, J, J3, C, nflip, do_clamp;
    double scale;
    int32_t operand_bf16, ln_folded, h_residual_only;
    float *x, *xn;                  /* [M,C] */
    void *image;                    /* modes 3, 4: [M,C] image */
    float *stats;                   /* ln_folded: [nrows,2] */
    int64_t row0, nrows;
} pafuse_embed_args;
int pafuse_embed_unit(const pafuse_embed_args *a, void *stream);

/* pafuse_ddim_finalize: output stage of DDIM step `step` of T.  pred[i] = part i's denoiser output
 * [nflip*B*P*F*part_joints[i], 3] (host array of `num_parts` device pointers; flipped half second).  Per (b,p,f,j):
 *   x0 = pred[joint_part[j]][.., joint_local[j], :]                       torch.cat(dim=-2)   diffusionpose.py:171
 *   if flip: u = flipped prediction of joint flip_perm[j], u.x = -u.x ; x0 = (x0 + u) / 2     :211-215
 *   x0 = clamp(x0 * scale, +-1.1*scale) -> out[b, step, p, f, j, :]                            :216-218, :298
 *   last step: img = x0.  Otherwise eps = (sqrt_recip_acp*img - x0) / sqrt_recipm1_acp in fp64 (:157-161) and
 *   img = x0*sqrt_alpha_next + c*eps + sigma*noise (:308-312; scalar demotion as torch does it per sampler).
 * img [B,P,F,J,3] in/out, noise [B,P,F,J,3] (may be NULL on the last step), out [B,T,P,F,J,3];
 * joint_part / joint_local / flip_perm int32 [J] on the device (trusted). */
int pafuse_ddim_finalize(const float *const *pred, const int32_t *part_joints, int32_t num_parts,
                         const int32_t *joint_part, const int32_t *joint_local, const int32_t *flip_perm, float *img,
                         const float *noise, float *out, int32_t B, int32_t P, int32_t F, int32_t J, int32_t T,
                         int32_t step, int32_t flip, double scale, const pafuse_ddim_step *st, void *stream);

/* Hypothesis aggregation on the gathered predictions - the caller-side step of main_h3wb.py:327-362
 * (wb_pose_from_parts common/utils.py:113-126, project_to_2d common/camera.py:30-60, the per-joint parts of
 * mpjpe_diffusion* common/loss.py:36-168).  pred [B,T,P,F,J,3] and gt [B,F,J,3] are part-centred; x2d [B,F,J,2];
 * traj [B,F,3]; cam [9]; conn/pbroot int32 [J] (connection joint / part root of every joint).
 * Outputs: e3, epb [B,T,P,F,J] (per-hypothesis whole-body / part-re-centred errors), jbest, pagg, jagg,
 * paggpb [B,T,F,J].  The means over (b,f,j) and the P-Best argmin are left to the caller (a few tiny reductions). */
int pafuse_hypothesis_errors(const float *pred, const float *gt, const float *x2d, const float *traj, const float *cam,
                             const int32_t *conn, const int32_t *pbroot, int32_t B, int32_t T, int32_t P, int32_t F,
                             int32_t J, float *e3, float *epb, float *jbest, float *pagg, float *jagg, float *paggpb,
                             void *stream);

/* The same aggregation from per-shard partial reductions (Protocol #1 only): a shard holds hypotheses
 * [h0, h0 + P_r) of the P - the hypotheses of one rank, or one chunk of them on a single device - and is reduced to a
 * state whose size does not depend on P, so that evaluation never holds (or gathers) the whole [B,T,P,F,J,3] tensor.
 * pred [B,T,P_r,F,J,3] is the LOCAL tensor; the other operands are those of pafuse_hypothesis_errors, plus
 * part int32 [J], the part number 0 .. num_parts-1 of every joint.
 * State, one flat 8-byte aligned buffer of pafuse_hypothesis_partials_bytes bytes, n = B*T*F*J:
 *   double sum[n][3]    sum over the local h, in h order, of the whole-body joint (the P-Agg mean pose; a part root's sum
 *                       is the sum of that joint of the same frame)
 *   float  jbest[n]     minimum over the local h of e3                                   (+inf when P_r == 0)
 *   float  e2[n], sel3[n]; int32 idx[n]   the J-Agg candidate: smallest reprojection error, its e3, its GLOBAL
 *                       hypothesis index h0 + h; first minimum wins; (+inf, 0, -1) where no e2 of the shard is finite
 *   double hsum[P_r][T][1 + num_parts]    per local hypothesis and step: sum over (b, f, j) of e3, then of epb over the
 *                       joints of each part (their sum over the parts is the whole-pose epb sum), fp64, fixed order
 * Everything that depends on P_r is at the end: a ragged shard is a prefix of a buffer sized for the largest one, so W
 * ranks exchange their states with one all-gather of equal-sized buffers.  Two kernels, no atomics, bit-reproducible;
 * the per-hypothesis sums are independent of how the P hypotheses are cut into shards.  workspace:
 * pafuse_hypothesis_partials_workspace_bytes bytes of scratch, 8-byte aligned (the workgroups' shares of hsum).
 * B == 0 or P_r == 0: no kernel runs, the state is the neutral one.  Refused: a null operand, negative sizes or h0
 * (PAFUSE_E_ARG), num_parts outside 1 .. PAFUSE_MAX_PARTS (PAFUSE_E_SHAPE), a small workspace (PAFUSE_E_WORKSPACE). */
size_t pafuse_hypothesis_partials_bytes(int32_t B, int32_t T, int32_t P_r, int32_t F, int32_t J, int32_t num_parts);
size_t pafuse_hypothesis_partials_workspace_bytes(int32_t B, int32_t T, int32_t P_r, int32_t F, int32_t J,
                                                  int32_t num_parts);
int pafuse_hypothesis_partials(const float *pred, const float *gt, const float *x2d, const float *traj, const float *cam,
                               const int32_t *conn, const int32_t *pbroot, const int32_t *part, int32_t num_parts,
                               int32_t B, int32_t T, int32_t P_r, int32_t F, int32_t J, int32_t h0, void *state,
                               size_t state_bytes, void *workspace, size_t workspace_bytes, void *stream);

/* Combines W such states, `stride_bytes` apart (rank-major, as an all-gather leaves them) and in ascending-h0 order.
 * Only the first 40*n bytes of each are read (the per-hypothesis tail is not combined: concatenate it).  Writes
 *   merged (may be NULL): the 40*n-byte head of the state of the union - sums added in shard order, minimum of the
 *           minima, the candidate with the smallest e2 and, among equal ones, the lowest global index.  It may be
 *           the first operand itself (a running state accumulating chunk after chunk), but then without the maps;
 *   jbest, pagg, jagg, paggpb [B,T,F,J] (all four or none): what pafuse_hypothesis_errors writes.  jbest and jagg are
 *           bit-equal to it; pagg / paggpb use the fp64 sums divided by P_total (that kernel sums in fp32). */
int pafuse_hypothesis_combine(const void *states, int32_t W, size_t stride_bytes, const float *gt, const int32_t *conn,
                              const int32_t *pbroot, int32_t B, int32_t T, int32_t F, int32_t J, int32_t P_total,
                              void *merged, float *jbest, float *pagg, float *jagg, float *paggpb, void *stream);

/* The aggregates as poses, from the same shards: P-Agg (the mean over the hypotheses of the whole-body pose) and J-Agg
 * (per joint, the whole-body joint of the hypothesis whose 2-D reprojection is closest to the input).  No ground truth.
 * pred [B,T,P_r,F,J,3] holds the part-centred hypotheses [h0, h0 + P_r) of the run; x2d [B,F,J,2], traj [B,F,3], cam [9],
 * conn int32 [J] as above.  x2d, traj and cam all NULL: mean-only (in the wild there is no camera and no trajectory) -
 * the reprojection is skipped and every candidate stays neutral.
 * State, one flat 8-byte aligned buffer of pafuse_pose_partials_bytes = 44*n rounded up to 8 bytes, n = B*T*F*J:
 *   double sum[n][3]    sum over the local h, in h order, of the whole-body joint (one fp32 add of the connection joint,
 *                       joint 0 pinned at 0)
 *   float  e2[n]; int32 idx[n]; float sel[n][3]   the J-Agg candidate: smallest reprojection error (the fp32 expression of
 *                       pafuse_hypothesis_errors, so the index is the one every evaluation entry picks), its GLOBAL
 *                       hypothesis index h0 + h, its whole-body joint; first minimum wins; (+inf, -1, NaN NaN NaN) where
 *                       no e2 of the shard is finite
 * Nothing depends on P_r: W ranks exchange their states with one all-gather.  One kernel, no workspace, no atomics,
 * bit-reproducible.  B == 0 or P_r == 0: no kernel runs, the state is the neutral one (zero sums, no candidate).
 * Refused (PAFUSE_E_ARG): a null operand, negative sizes or h0, some but not all of x2d / traj / cam, a short state. */
size_t pafuse_pose_partials_bytes(int32_t B, int32_t T, int32_t F, int32_t J);
int pafuse_pose_partials(const float *pred, const float *x2d, const float *traj, const float *cam, const int32_t *conn,
                         int32_t B, int32_t T, int32_t P_r, int32_t F, int32_t J, int32_t h0, void *state,
                         size_t state_bytes, void *stream);

/* The same state WITHOUT a trajectory (J-Agg in the wild): the root position t of every (hypothesis, frame) is fitted
 * on the device from the detections and the intrinsics, and takes the place of traj in the reprojection error.
 * x2d [B,F,J,2] screen-normalised detections, conf [B,F,J] their weights (NULL: every weight 1), cam [9].
 * The fit, fp64 per (b,t,h,f) over the whole-body joints w_j (fx, fy, cx, cy = cam[0:4]; the distortion terms cam[4:9]
 * take no part in it - they do in the error):
 *   a = (u - cx)/fx, b = (v - cy)/fy, rx = a*wz - wx, ry = b*wz - wy
 *   W, Sa, Sb, Sq = sum c*(1, a, b, a^2 + b^2);  Srx, Sry, Sm = sum c*(rx, ry, a*rx + b*ry)
 *   den = Sq - (Sa^2 + Sb^2)/W;  tz = (-Sm + (Sa*Srx + Sb*Sry)/W)/den;  tx = (Srx + Sa*tz)/W;  ty = (Sry + Sb*tz)/W
 * A weight that is not > 0 (0, negative, NaN) takes its joint out of every sum and out of the pick: its candidate
 * stays (+inf, -1, NaN NaN NaN) whatever its coordinates hold.  No fit - fewer than two weighted joints, den not finite
 * and > 0, t not finite in fp32 - offers no candidate; the sums still take the hypothesis.  The order of every sum over
 * j is fixed (pafuse_amd/rootfit.py states it and the same operations in numpy), so the result is bit-reproducible and
 * does not depend on how P is cut.  A per-frame fit with a KNOWN focal length: no temporal smoothing, no focal estimate.
 * tfit (NULL: not wanted) [B,T,P_r,F,3] fp32: the fitted root of every local hypothesis, NaN where there is no fit.
 * One kernel, no workspace, no atomics.  B == 0 or P_r == 0: no kernel runs, the state is the neutral one.
 * Refused (PAFUSE_E_ARG): a null pred / x2d / cam / conn, negative sizes or h0, a short or misaligned state. */
int pafuse_pose_partials_fit(const float *pred, const float *x2d, const float *conf /* [B,F,J] or NULL = all 1 */,
                             const float *cam, const int32_t *conn, int32_t B, int32_t T, int32_t P_r, int32_t F,
                             int32_t J, int32_t h0, void *state, size_t state_bytes,
                             float *tfit /* [B,T,P_r,F,3] or NULL */, void *stream);

/* Combines W such states, `stride_bytes` apart and in ascending-h0 order: sums added in shard order, the candidate with
 * the smallest e2 and, among equal ones, the lowest global index.  Writes any of (NULL: not wanted, at least one):
 *   merged    the state of the union; of the operands it may only lie over the FIRST (a running state over chunks)
 *   mean      [B,T,F,J,3] fp32 = sum / P_total, divided in fp64 and rounded once
 *   pick      [B,T,F,J,3] fp32 the J-Agg pose (NaN where no state holds a candidate)
 *   pick_idx  [B,T,F,J] int32 its hypothesis (-1 where none) */
int pafuse_pose_combine(const void *states, int32_t W, size_t stride_bytes, int32_t B, int32_t T, int32_t F, int32_t J,
                        int32_t P_total, void *merged, float *mean, float *pick, int32_t *pick_idx, void *stream);

/* J-Agg COHERENT IN TIME.  The pick above takes every frame on its own; this one chooses, per line (b, t, j), a path h(f)
 * through ALL P hypotheses of a clip that minimises
 *   sum_f u_f(h(f)) + weight * sum_f |off_f(h(f)) - off_f-1(h(f-1))|
 * by a Viterbi recursion along the frames (pafuse_amd/posepath.py states it operation for operation; fp64, contraction
 * off, correctly rounded sqrt; after every frame the frame's minimum is subtracted from the running costs and added to the
 * total).  w = the whole-body joint; off = (double)w - (double)mean (mean NULL: absolute).  A hypothesis is AVAILABLE at a
 * frame if its offset is finite; a frame is OBSERVED if conf > 0 (NULL: always) and an available hypothesis has a finite
 * e2 - the fp32 reprojection error of pafuse_pose_partials, under `root`: the shared trajectory [B,F,3], or
 * (root_per_hypothesis != 0) [B,T,P,F,3], as pafuse_pose_partials_fit writes to tfit.  u is e2 at an observed frame (+inf
 * where it is not finite) and 0 for every available hypothesis at an unobserved one: the joint crosses a gap by smoothness
 * alone.  Ties go to the lower hypothesis at every step.  weight == 0: the pick of pafuse_pose_combine wherever that has one.
 * weight has the unit of normalised screen length per metre; fx / Z is the weight at which a jump costs what it projects to.
 *   pick     [B,T,F,J,3] the chosen hypothesis's whole-body joint     pick_idx [B,T,F,J] int32 its index
 *   pick_e2  [B,T,F,J] (NULL: not wanted) its e2, +inf at an unobserved frame
 *   cost     [B,T,J] double (NULL: not wanted) the cost of the path
 * A line with a frame at which no hypothesis is available, or without an observed frame, has no path: -1, NaN, +inf and a
 * NaN cost at all its frames.  Per clip only: nothing crosses a clip seam.  Not a smoother of the pose values: every joint
 * returned is some hypothesis's joint.
 * workspace: pafuse_pose_path_workspace_bytes bytes, 8-byte aligned (one back-pointer byte per line, frame and hypothesis:
 * 1/12 of pred).  One kernel, one wave per line, no atomics, bit-reproducible.  B == 0 launches nothing.
 * Refused before any HIP call: a null required operand, negative sizes, a short or misaligned workspace, a weight that is
 * negative or not finite (PAFUSE_E_ARG); P > 256 or F > 256 (PAFUSE_E_SHAPE). */
size_t pafuse_pose_path_workspace_bytes(int32_t B, int32_t T, int32_t P, int32_t F, int32_t J);
int pafuse_pose_path(const float *pred /* [B,T,P,F,J,3] */, const float *x2d /* [B,F,J,2] */,
                     const float *root /* [B,F,3] or [B,T,P,F,3] */, int32_t root_per_hypothesis, const float *cam /* [9] */,
                     const float *conf /* [B,F,J] or NULL */, const int32_t *conn /* [J] */,
                     const float *mean /* [B,T,F,J,3] or NULL */, double weight, int32_t B, int32_t T, int32_t P, int32_t F,
                     int32_t J, float *pick, int32_t *pick_idx, float *pick_e2, double *cost, void *workspace,
                     size_t workspace_bytes, void *stream);

/* THE PATH OF A WHOLE VIDEO.  pafuse_pose_path stops at the clip: every F frames the path starts again from nothing, and
 * pooled windows (stride < F) cannot be combined with it.  Here the recursion runs along the N frames of the video, and the
 * candidates at video frame n are the pairs (window, hypothesis) of ALL windows that cover n - window w covers the frames
 * [starts[w], starts[w] + valid[w]), its local frame f = n - starts[w].  pafuse_amd/posepath.py frames_path states it: the
 * statement of pafuse_pose_path on the dense [W*P, N] form in which a window that does not cover a frame is unavailable
 * there; the arithmetic (fp64, contraction off, correctly rounded sqrt, the frame's minimum subtracted after every frame),
 * availability, observation and the unary cost u are those of pafuse_pose_path, with
 *   off = (double)w - (double)mean[t,n,j]   mean [T,N,J,3] as pafuse_frames_finish writes it (NULL: absolute offsets)
 *   e2 under root [N,3] (one trajectory of the video) or (root_per_hypothesis != 0) [W,T,P,F,3] (tfit of the windows)
 *   x2d [N,J,2] and conf [N,J] (NULL: all observed) per VIDEO frame
 * Ties go to the lower (window, hypothesis) at every step - the order of pafuse_pose_windows_fold -, so weight == 0 is the
 * pick, index and window of pafuse_frames_finish wherever that has one.
 * The windows must be the whole video: starts strictly ascending, starts[0] == 0, starts[w] + valid[w] not descending,
 * no gap (starts[w+1] <= starts[w] + valid[w]), the last window ending at N, valid in 1 .. F - everything
 * pafuse_amd.windows.window_starts produces, the shifted last window and the one padded window of a short video included.
 * starts / valid are passed twice, device and host copies, as pafuse_pose_windows_fold takes them: the checks read the
 * host copy, the kernel the device copy, and the call neither copies nor synchronises.
 *   pick     [T,N,J,3] the chosen hypothesis's whole-body joint
 *   pick_idx [T,N,J] int32 its hypothesis      pick_win [T,N,J] int32 its window (the index within this call)
 *   pick_e2  [T,N,J] (NULL: not wanted) its e2, +inf at an unobserved frame
 *   cost     [T,J] double (NULL: not wanted) the cost of the path
 * A LINE DIES WHOLE: one frame at which no candidate is available, or no observed frame at all, and the line (t, j) has no
 * path at ANY frame of the video: -1, -1, NaN, +inf and a NaN cost.  Segments that restart are not built.  Not a smoother
 * of the pose values: every joint returned is some hypothesis's joint.
 * workspace: pafuse_frames_path_workspace_bytes bytes, 8-byte aligned: one back-pointer byte per (line, frame, slot),
 * [T*J, N, K] rounded up to 8, K = P * the largest number of windows that cover one frame; it grows with the length of the
 * video, as pred does.  The function returns 0 for whatever the call would refuse.  One kernel, one wave per line (t, j), no
 * atomics, bit-reproducible.  N has no limit of its own.
 * Refused before any HIP call: a null required operand, sizes < 1 (W == 0 too: a video has at least one window), windows
 * that break a rule above, a weight that is negative or not finite, a short or misaligned workspace (PAFUSE_E_ARG);
 * K > 256 (PAFUSE_E_SHAPE). */
size_t pafuse_frames_path_workspace_bytes(int32_t N, int32_t T, int32_t J, int32_t P, int32_t W,
                                          const int32_t *starts_host, const int32_t *valid_host);
int pafuse_frames_path(const float *pred /* [W,T,P,F,J,3] */, const float *x2d /* [N,J,2] */,
                       const float *root /* [N,3] or [W,T,P,F,3] */, int32_t root_per_hypothesis,
                       const float *cam /* [9] */, const float *conf /* [N,J] or NULL */, const int32_t *conn /* [J] */,
                       const float *mean /* [T,N,J,3] or NULL */, double weight,
                       int32_t W, int32_t T, int32_t P, int32_t F, int32_t J, int32_t N,
                       const int32_t *starts, const int32_t *valid, const int32_t *starts_host, const int32_t *valid_host,
                       float *pick /* [T,N,J,3] */, int32_t *pick_idx, int32_t *pick_win /* [T,N,J] */,
                       float *pick_e2 /* [T,N,J] or NULL */, double *cost /* [T,J] or NULL */,
                       void *workspace, size_t workspace_bytes, void *stream);

/* The spread of the hypotheses beside the mean pose, from the same shards: first and second moments of the whole-body
 * joint per (b,t,f,j).  pred [B,T,P_r,F,J,3] holds the part-centred hypotheses [h0, h0 + P_r) of the run, conn int32 [J].
 * State, one flat 8-byte aligned buffer of pafuse_spread_partials_bytes = (9*n + 1)*8 bytes, n = B*T*F*J, all doubles:
 *   double sum[n][3]   sum over the local h, in h order, of the whole-body joint: the sum of a pose state, bit for bit
 *   double m2[n][6]    centred second moments sum_h (w_h - mean)(w_h - mean)^T in the order xx, xy, xz, yy, yz, zz, updated
 *                      per hypothesis by Welford's rule (d = w - sum_prev/k_prev; sum += w; m2 += d (x) (w - sum/k))
 *   double count       P_r
 * All state arithmetic is fp64, floating-point contraction off.  Nothing depends on P_r: W ranks exchange their states
 * with one all-gather of double rows.  One kernel, no workspace, no atomics, bit-reproducible.  B == 0: the state is
 * empty (0 bytes).  P_r == 0: no kernel runs, the state is the neutral one (all zeros, count 0).  h0 is checked only.
 * Refused (PAFUSE_E_ARG): a null pred or conn with work to do, negative sizes or h0, a short or misaligned state, a grid
 * out of range. */
size_t pafuse_spread_partials_bytes(int32_t B, int32_t T, int32_t F, int32_t J);
int pafuse_spread_partials(const float *pred, const int32_t *conn, int32_t B, int32_t T, int32_t P_r, int32_t F, int32_t J,
                           int32_t h0, void *state, size_t state_bytes, void *stream);

/* Combines W such states, `stride_bytes` apart and in ascending-h0 order, by Chan's pairwise rule in fp64, left to right:
 * delta = sum_B/n_B - sum_A/n_A, m2 = m2_A + m2_B + delta (x) delta * n_A n_B / (n_A + n_B), sum = sum_A + sum_B; a state
 * with count 0 is skipped.  Writes any of (NULL: not wanted, at least one):
 *   merged   the state of the union; of the operands it may only lie over the FIRST (a running state over chunks)
 *   mean     [B,T,F,J,3] fp32 = sum / count
 *   cov      [B,T,F,J,6] fp32 = m2 / count, the POPULATION covariance (one hypothesis: 0, not NaN), order as m2
 *   std_dev  [B,T,F,J]   fp32 = sqrt((m2_xx + m2_yy + m2_zz) / count): the RMS distance of the hypotheses from the mean joint
 * each divided in fp64 and rounded once.  Total count 0: NaN.  A non-finite hypothesis makes the three outputs of its
 * element NaN and touches no other element.
 * Refused (PAFUSE_E_ARG): null states, negative sizes, W < 1, a stride smaller than the state, misalignment, a merged
 * state over an operand other than the first, no output, a grid out of range. */
int pafuse_spread_combine(const void *states, int32_t W, size_t stride_bytes, int32_t B, int32_t T, int32_t F, int32_t J,
                          void *merged, float *mean, float *cov, float *std_dev, void *stream);

/* Overlapping windows pooled into one state per video FRAME.  A video of N frames is cut into windows of F frames; window
 * b of a batch starts at frame starts[b] and its first valid[b] frames are real (a video shorter than F is one padded
 * window; the padding is never folded).  The batch's hypotheses have been reduced to ONE pose state [B,T,F,J] - what
 * pafuse_pose_partials, pafuse_pose_partials_fit or the `merged` output of pafuse_pose_combine writes for the union of
 * P_total hypotheses - and / or one spread state; the folds below merge row (b,t,f,j) into frame row (t, starts[b] + f, j).
 * Frame pose state, one flat 8-byte aligned buffer of pafuse_frame_pose_state_bytes = 48*r + 4*N rounded up to 8 bytes,
 * r = T*N*J rows in (t,n,j) order:
 *   double sum[r][3]; float e2[r]; int32 idx[r]; int32 win[r]; float sel[r][3]   as in a pose state; win: the GLOBAL window
 *                       index of the candidate
 *   int32 count[N]      the hypotheses folded into frame n
 * Frame spread state, pafuse_frame_spread_state_bytes = (9*r + N)*8 bytes:  double sum[r][3]; double m2[r][6]; double count[N].
 * The *_init entries write the neutral states: zero sums and counts, candidate (+inf, -1, -1, NaN NaN NaN); zero moments. */
size_t pafuse_frame_pose_state_bytes(int32_t N, int32_t T, int32_t J);
size_t pafuse_frame_spread_state_bytes(int32_t N, int32_t T, int32_t J);
int pafuse_frame_pose_state_init(void *frame_state, size_t frame_bytes, int32_t N, int32_t T, int32_t J, void *stream);
int pafuse_frame_spread_state_init(void *frame_state, size_t frame_bytes, int32_t N, int32_t T, int32_t J, void *stream);

/* Folds the pose state of B windows into the frame state.  For every (n,t,j) the windows of the batch that cover frame n
 * are visited in ascending order: sum += state.sum (one fp64 add per component and window), count[n] += P_total, and the
 * candidate is replaced only if state.e2 < e2 (strict: among equal errors the lowest window keeps it, and within it the
 * lowest hypothesis); idx takes the state's global hypothesis index, win takes w0 + b (w0: the global index of the
 * batch's first window).  A gather - one thread per (n,t,j) of the frame range the batch touches; no atomics, no
 * workspace; frames outside that range (and frames in a gap between two windows) are not touched.  A frame's windows
 * arrive in ascending order whether they come in one batch or in several, so the result does not depend on the batching,
 * provided the batches come in ascending window order.
 * starts / valid are passed TWICE: device int32 [B], which the kernel reads, and host int32 [B] with the same values, which
 * this entry checks (the call neither copies nor synchronises, so it can be captured).  Should the two differ, the kernel
 * still reads inside the batch state and writes inside the frames the host copy names.
 * Refused (PAFUSE_E_ARG): a null operand, N, T, F, J < 1 or B, w0, P_total < 0, a window reaching past N or starting below
 * 0, valid outside 1 .. F, starts not strictly ascending, a short or misaligned state.  B == 0 launches nothing. */
int pafuse_pose_windows_fold(void *frame_state, size_t frame_bytes, int32_t N, const void *state, size_t state_bytes,
                             int32_t B, int32_t T, int32_t F, int32_t J, const int32_t *starts, const int32_t *valid,
                             const int32_t *starts_host, const int32_t *valid_host, int32_t w0, int32_t P_total,
                             void *stream);

/* The same fold for a spread state (pafuse_spread_partials, or the `merged` output of pafuse_spread_combine): every
 * covering window is merged into the frame by Chan's rule, the operations of pafuse_spread_combine in its order, fp64,
 * contraction off; count[n] += the state's count per window.  A state with count 0 folds nothing.  Two kernels (the
 * counts are written behind the fold, whose every thread reads them).  Operands and refusals as above. */
int pafuse_spread_windows_fold(void *frame_state, size_t frame_bytes, int32_t N, const void *state, size_t state_bytes,
                               int32_t B, int32_t T, int32_t F, int32_t J, const int32_t *starts, const int32_t *valid,
                               const int32_t *starts_host, const int32_t *valid_host, void *stream);

/* Writes any of (NULL: not wanted, at least one), from a frame pose state (frame_state; NULL when nothing of it is asked):
 *   mean      [T,N,J,3] fp32 = sum / count[n], divided in fp64 and rounded once (count 0: NaN)
 *   pick      [T,N,J,3] fp32, pick_idx [T,N,J] int32, pick_win [T,N,J] int32   the J-Agg pose, its hypothesis and its window
 *                       (NaN, -1, -1 where no window offered a candidate)
 * and from a frame spread state (frame_spread; NULL when nothing of it is asked), by the arithmetic of pafuse_spread_combine:
 *   std_dev   [T,N,J] fp32,  cov [T,N,J,6] fp32   (count 0 or a non-finite hypothesis: NaN)
 * Refused (PAFUSE_E_ARG): negative sizes, no output, an output without its state, misalignment, a grid out of range. */
int pafuse_frames_finish(const void *frame_state, const void *frame_spread, int32_t N, int32_t T, int32_t J, float *mean,
                         float *pick, int32_t *pick_idx, int32_t *pick_win, float *std_dev, float *cov, void *stream);

/* The camera-space root of the finished per-frame pose: one fit per (t, frame) on the pose that is returned (the pooled
 * mean or the pick of pafuse_frames_finish, or any [T,N,J,3] array), by the algebra of pafuse_pose_partials_fit, operation
 * for operation (fp64, contraction off, the same fixed order of every sum over j; pafuse_amd/trajectory.py states it).
 * x2d [N,J,2] screen-normalised detections and conf [N,J] their weights are shared by the T steps; cam[0:4] = fx fy cx cy.
 * Besides a weight that is not > 0, a joint any component of whose pose is not finite drops out of every sum (a frame no
 * window covered, a pick without a candidate), so W, Sa, Sb, Sq are per (t, n).  No fit - fewer than two joints in the
 * sums, den not finite and > 0, t not finite in fp32 - is NaN in traj.
 *   traj  [T,N,3]  the root, metres, camera space; camera-space pose = pose + traj (broadcast over j)
 *   wsum  [T,N]    (NULL: not wanted) W rounded to fp32: the weight the frame's fit rests on; 0 where there is no fit
 *   resid [T,N]    (NULL: not wanted) sqrt(R / W), R = sum c*(ex^2 + ey^2), ex = (tx - a*tz) - rx, ey = (ty - b*tz) - ry with
 *                  t before its rounding: the weighted algebraic residual in metres (a wrong focal length shows here);
 *                  NaN where there is no fit
 * One kernel, one wave per (t, n), no workspace, no atomics, bit-reproducible.
 * Refused (PAFUSE_E_ARG) before any HIP call: a null pose / x2d / cam / traj, T, N or J < 1. */
int pafuse_frames_root_fit(const float *pose /* [T,N,J,3] whole-body, root-relative */,
                           const float *x2d /* [N,J,2] */, const float *conf /* [N,J] or NULL = all 1 */,
                           const float *cam /* [>=4]: fx fy cx cy */, int32_t T, int32_t N, int32_t J,
                           float *traj /* [T,N,3], NaN = no fit */, float *wsum /* [T,N] or NULL */,
                           float *resid /* [T,N] or NULL */, void *stream);

/* A confidence-weighted local-linear filter along the frames of a trajectory.  For every (t, n) the frames
 * m = max(0, n - r) .. min(N - 1, n + r) are walked in ascending order, d = m - n, all in fp64 with contraction off:
 *   g = (1 - d*d/(r+1)^2)^2 (the biweight taper), omega = g * weight[t,m]; a frame takes part only if its weight is > 0
 *   (NULL: 1) and the three components of traj[t,m] are finite
 *   S0, S1, S2 = sum omega*(1, d, d*d);  per component Q0, Q1 = sum omega*(y, d*y);  D = S0*S2 - S1*S1
 *   two frames or more and D finite and > 0:  (S2*Q0 - S1*Q1)/D, the local line's value at d = 0
 *   else S0 > 0:  Q0/S0;   else NaN
 * rounded once to fp32.  A line, not a mean: constant velocity comes through without lag or end-shrinkage; a frame
 * without a fit is filled from its neighbours.  A fixed-radius linear smoother, not a tracker.
 * One kernel, one thread per (t, n).  Refused (PAFUSE_E_ARG) before any HIP call: a null traj or out, T or N < 1, radius
 * outside 1 .. 64, out == traj. */
int pafuse_trajectory_smooth(const float *traj /* [T,N,3] */, const float *weight /* [T,N] or NULL */, int32_t T, int32_t N,
                             int32_t radius /* 1..64 */, float *out /* [T,N,3], may not alias traj */, void *stream);

/* Missing 2-D detections repaired along the frames before lifting, per joint (pafuse_amd/detections.py states the arithmetic;
 * DESIGN.md section 6j).  observed(n, j): conf[n,j] > threshold and both coordinates of x2d[n,j] finite (a NaN confidence is
 * not observed).  An observed joint is copied: the same bits, status 0.  A missing one is filled by the filter of
 * pafuse_trajectory_smooth over the frames m = max(0, n - r) .. min(N - 1, n + r) in which joint j is observed, omega =
 * g * conf[m,j]: the local line's value at d = 0 (two frames or more, D finite and > 0: status 1, filled), else Q0/S0 (S0 > 0:
 * status 2, held), else status 3, unfilled.  The value is rounded once to fp32; one that is not finite in fp32 is status 3.
 * Status 3 keeps the input's bits: no input gets worse and no NaN is created.
 * The level rule.  anchor [J] names the joint a joint hangs on (a finger on its wrist), < 0 for none.  Joint j is LEVEL 1 iff
 * 0 <= anchor[j] < J and anchor[anchor[j]] < 0; every other joint is LEVEL 0 - anchor[j] < 0, out of range, anchored on
 * itself or on an anchored joint, and every joint of a NULL table.  anchor[anchor[j]] is read only for an in-range anchor[j],
 * so no table causes a read out of bounds; this entry does NOT refuse a table the rule demotes (the Python layers do).
 * Level 0 filters y = x2d[m,j].  Level 1, a = anchor[j], filters y = x2d[m,j] - out[m,a] over the frames in which also
 * status[m,a] != 3 and writes out[n,a] + line, and only if status[n,a] != 3 (otherwise status 3): a hand lost for a few
 * frames moves with its wrist.
 *   out      [N,J,2]  the repaired detections
 *   conf_out [N,J]    (NULL: not wanted) conf where status is 0, 0 elsewhere: a filled joint carries no measurement
 *   status   [N,J]    0 observed, 1 filled, 2 held, 3 unfilled
 * Two launches of one kernel on the stream (level 0, then level 1; one with a NULL table), one thread per (n, j); level 1
 * reads out / status of level-0 joints and writes level-1 joints, which is why out may not alias x2d and status is required.
 * No workspace, no atomics, no host synchronisation, bit-reproducible.
 * Refused (PAFUSE_E_ARG) before any HIP call: a null x2d / conf / out / status, N or J < 1, radius outside 1 .. 64, a threshold
 * that is not finite or < 0, out == x2d, conf_out == conf, a grid out of range. */
int pafuse_detections_repair(const float *x2d /* [N,J,2] */, const float *conf /* [N,J] */,
                             const int32_t *anchor /* [J] device, or NULL */, int32_t N, int32_t J, int32_t radius /* 1..64 */,
                             float threshold /* >= 0 */, float *out /* [N,J,2], may not alias x2d */,
                             float *conf_out /* [N,J] or NULL, may not alias conf */, uint8_t *status /* [N,J] */, void *stream);

/* OBSERVED 2-D detections screened in front of that repair: outliers rejected, left/right swaps undone, per joint along the
 * frames (pafuse_amd/detscreen.py states the arithmetic, operation for operation).  observed(n, j) is the
 * repair's rule.  All in fp64 with contraction off, rounded once where a value is stored.
 * The partner rule.  mirror [J] names every joint's mirror joint.  Joint j has the partner q = mirror[j] iff 0 <= q < J, q != j
 * and mirror[q] == j; mirror[q] is read only for an in-range q, so no table causes a read out of bounds; a NULL table has no
 * pairs; this entry does NOT refuse a table whose entries the rule drops (the Python layers do).
 * Residual of (n, j) against an accepted set acc: the filter of pafuse_trajectory_smooth, omega = g * conf[m,j], over the frames
 * m = max(0, n - r) .. min(N - 1, n + r), m != n, with acc[m,j] - leave one out.  The fit exists iff that filter finds a line
 * (two frames or more, D finite and > 0) and >= support frames took part; e = float(sqrt(dx*dx + dy*dy)) from the line's
 * value at d = 0; NaN where (n, j) is not observed or has no fit.
 * acc_0 = observed; for p = 1 .. passes: acc_p = fit ? double(e_p) <= tau_j : acc_{p-1}, e_p against acc_{p-1} (a Jacobi
 * update; every observed frame is re-tested in every pass, which re-admits the neighbours of a gross outlier).
 * tau_j = double(gate) * max(1.4826 * double(med_j), double(floor)), med_j the exact lower median of the values of e_1[:, j]
 * that are not NaN (rank (c - 1) / 2 of c, +inf last; 0 without a value), found by a radix select on the bit patterns.
 * One more evaluation against acc_passes gives e_self and, for a pair both observed at n, e_cross(n, j): the partner's
 * detection against j's line.  The pair's frame is swapped iff both are observed, one of them is not accepted, and for both
 * joints double(e_cross) <= tau and e_cross < e_self.
 *   out      [N,J,2]  the partner's detection where swapped, else the input's bits
 *   conf_out [N,J]    the partner's confidence where swapped, 0 where rejected, else the input's bits
 *   status   [N,J]    0 accepted, 1 rejected, 2 swapped, 3 not observed (every bit kept)
 *   resid    [N,J]    (NULL: not wanted) e_self, NaN where there is none
 *   scale    [J]      (NULL: not wanted) float(tau_j)
 *   workspace         pafuse_detections_screen_workspace_bytes(N, J) bytes (0 for a size < 1), 8-byte aligned
 * passes + 3 launches on the stream: one thread per (n, j), but the scales, one wave per joint.  No atomics, no host
 * synchronisation, bit-reproducible.  gate 4, floor 0.005, passes 3 and support 3 are defaults, not tuned values.
 * Refused (PAFUSE_E_ARG) before any HIP call: a null x2d / conf / out / conf_out / status, N or J < 1, radius outside 1 .. 64,
 * passes outside 1 .. 8, support outside 2 .. 129, a gate or floor that is not finite and > 0, a threshold that is not finite
 * or < 0, out == x2d, conf_out == conf, a null, short or misaligned workspace, a grid out of range. */
size_t pafuse_detections_screen_workspace_bytes(int32_t N, int32_t J);
int pafuse_detections_screen(const float *x2d /* [N,J,2] */, const float *conf /* [N,J] */,
                             const int32_t *mirror /* [J] device, or NULL */, int32_t N, int32_t J, int32_t radius /* 1..64 */,
                             int32_t passes /* 1..8 */, int32_t support /* 2..129 */, float threshold /* >= 0 */,
                             float gate /* > 0 */, float floor /* > 0 */, float *out /* [N,J,2], may not alias x2d */,
                             float *conf_out /* [N,J], may not alias conf */, uint8_t *status /* [N,J] */,
                             float *resid /* [N,J] or NULL */, float *scale /* [J] or NULL */, void *workspace,
                             size_t workspace_bytes, void *stream);

/* PEOPLE FOLLOWED THROUGH A VIDEO: x2d [N,K,J,2] and conf [N,K,J], K candidate detections per frame in no stable order (an
 * all-zero slot is "nobody"), become M per-person rows assign [M,N] and, gathered, M one-person videos for everything above
 * (pafuse_amd/tracks.py states the arithmetic, operation for operation).  fp64, contraction off, sums
 * over the joints in the order of pafuse_frames_root_fit.
 * Nodes.  A joint is observed by the repair's rule; size(n,k) = sqrt((xmax - xmin) * (ymax - ymin)) over the observed joints;
 * the candidate is present iff >= support joints are observed and size is finite and > 0 (size is NaN where it is absent).
 * Links.  a = (n - g, ka), b = (n, kb), g = 1 .. G, both present with >= support common observed joints: w = min(conf_a,
 * conf_b), d = sum(w * sqrt(dx*dx + dy*dy)) / sum(w), cost = d / (0.5 * (size_a + size_b));
 * gain[n][g-1][ka][kb] = (gate - cost) - skip * (g - 1) iff cost <= gate, else -inf.
 * Path.  Per round, in ascending n: S[n,b] = max(0.0, max over g ascending, a ascending of S[n-g,a] + gain[n][g-1][a][b]) under
 * strict > for a node that is present and not used, -inf for every other; the track ends at the first maximum of S in
 * (n, b) order, its nodes come from the back-pointers and are marked used; a round whose path has fewer than min_frames
 * nodes ends the extraction: it and all later rounds are -1 everywhere, score NaN, 0 frames.  With a seed only the seed
 * starts a path and the frames before it are not walked (M must be 1); the half before the seed is the caller's second call
 * on the frame-reversed video.
 *   workspace  pafuse_tracks_workspace_bytes(N, K, J, G) bytes (0 for a size out of range), 8-byte aligned, laid out as
 *              gain [N,G,K,K] fp64 | size [N,K] fp64 | back-pointers [N,K,2] bytes | used flags [N,K] bytes.
 *              THE GAIN TABLE GROWS AS N*G*K*K*8 BYTES: 41 MB at N = 5 000, G = 4, K = 16; 1.3 GB at K = 64, G = 8.  Pass the
 *              largest number of people in any frame as K, not 64.
 *   pafuse_tracks_links   two launches (one wave per candidate, one wave per (n, g, kb)): writes size and every element of gain
 *   pafuse_tracks_path    one launch of ONE wave, the M rounds inside it; gain / size NULL: those pafuse_tracks_links left in
 *                         the workspace, else tables from anywhere (8-byte aligned); uses the back-pointers and used flags
 *   pafuse_tracks_gather  out [M,N,J,2], conf_out [M,N,J]: the bits of candidate assign[m][n]; zeros with confidence 0 where it
 *                         is -1 (or outside [0, K)) - the detector's own "not found", which pafuse_detections_repair fills
 * No atomics, no host synchronisation, bit-reproducible.  gate 0.5, skip 0.05, max_gap 4, support 5 and min_frames 5 are
 * defaults, not tuned values.
 * Refused (PAFUSE_E_ARG) before any HIP call: a null x2d / conf / assign / score / frames / out / conf_out, N or J < 1, K outside
 * 1 .. 64, G outside 1 .. 8, M outside 1 .. 64, support outside 1 .. 65535, min_frames < 1, a gate that is not finite and > 0, a
 * skip or threshold that is not finite or < 0, a seed outside [0,N) x [0,K) (no seed: -1, -1) or with M != 1, a null, short or
 * misaligned workspace, a misaligned gain or size, a grid out of range. */
size_t pafuse_tracks_workspace_bytes(int32_t N, int32_t K /* 1..64 */, int32_t J, int32_t G /* 1..8 */);
int pafuse_tracks_links(const float *x2d /* [N,K,J,2] */, const float *conf /* [N,K,J] */, int32_t N, int32_t K, int32_t J,
                        int32_t G, int32_t support, float threshold /* >= 0 */, double gate /* > 0 */, double skip /* >= 0 */,
                        void *workspace, size_t workspace_bytes, void *stream);
int pafuse_tracks_path(const double *gain /* [N,G,K,K] or NULL */, const double *size /* [N,K] or NULL */, int32_t N, int32_t K,
                       int32_t G, int32_t M /* 1..64 */, int32_t min_frames, int32_t seed_n, int32_t seed_k,
                       int32_t *assign /* [M,N] */, double *score /* [M] */, int32_t *frames /* [M] */, void *workspace,
                       size_t workspace_bytes, void *stream);
int pafuse_tracks_gather(const float *x2d /* [N,K,J,2] */, const float *conf /* [N,K,J] */, const int32_t *assign /* [M,N] */,
                         int32_t N, int32_t K, int32_t J, int32_t M, float *out /* [M,N,J,2] */, float *conf_out /* [M,N,J] */,
                         void *stream);

/* The per-frame pose smoothed along the frames, every frame weighted by the inverse of its hypothesis covariance
 * (pafuse_amd/posesmooth.py states the arithmetic, operation for operation).  A fixed-radius
 * local-linear filter per joint: frame m enters with the MATRIX weight W = (Sigma + floor^2*I)^-1, Sigma the covariance of
 * its hypotheses (pafuse_frames_finish's cov: xx xy xz yy yz zz) - it is trusted in each direction as far as its hypotheses
 * agree in that direction and otherwise carried by its neighbours' line.  All in fp64 with contraction off.
 * Row (t, m, j): the cofactors and determinant of Sigma + floor^2*I; the row takes part iff the three components of its pose are
 * finite, the determinant is finite and the three leading minors are > 0 (a NaN in cov removes the row, as does an indefinite
 * covariance); W = cofactors / det.
 * Output (t, n, j): over m = max(0, n - r) .. min(N - 1, n + r) ascending, d = m - n, g the taper of pafuse_trajectory_smooth:
 *   A0, A1, A2 = sum g*W*(1, d, d*d);   b0, b1 = sum g*W*y*(1, d)
 *   two rows or more and the 6x6 system [[A2, A1], [A1, A0]] [slope; value] = [b1; b0] factors by LDL^T (no square root, no
 *   pivot search) with six pivots finite and > 0 and a finite value:  value, the local line at d = 0   (code 1)
 *   else a row or more and A0 value = b0 factors the same way:  value, the weighted mean             (code 2)
 *   else NaN                                                                                          (code 3)
 * rounded once to fp32; a value that is not finite in fp32 is code 3, NaN.  With equal covariances W cancels and the result
 * is pafuse_trajectory_smooth's filter per joint: constant velocity passes without lag or end-shrinkage.  The matrix weights act
 * only where the covariance VARIES along the frames.  No motion model, no covariance of the result, no bone-length constraint.
 *   cov   [T,N,J,6] or NULL: all zeros - every frame weighs the same in every direction
 *   floor metres, finite and > 0: a regulariser that keeps a zero covariance (one hypothesis, or identical ones) solvable, not
 *         a tuned value
 *   out   [T,N,J,3], may not alias pose;   code uint8 [T,N,J] or NULL
 *   workspace  pafuse_pose_smooth_workspace_bytes(T, N, J) = 48 bytes per (t, n, j), 8-byte aligned, the caller's: the first of
 *              the two kernels stores W of every row there once, the second walks it (forming W again at every visit instead
 *              needs no workspace, gives the same bits and measured 1.2 times slower)
 * Two kernels on the stream, one thread per row and one per (t, n, j); no atomics, no host synchronisation, bit-reproducible.
 * Refused (PAFUSE_E_ARG) before any HIP call: a null pose or out, T, N or J < 1, radius outside 1 .. 64, a floor that is not
 * finite and > 0, out == pose, a workspace that is null, too small or not 8-byte aligned, a grid out of range. */
size_t pafuse_pose_smooth_workspace_bytes(int32_t T, int32_t N, int32_t J); /* 0 if a size is < 1 */
int pafuse_pose_smooth(const float *pose /* [T,N,J,3] */, const float *cov /* [T,N,J,6] or NULL */, int32_t T, int32_t N,
                       int32_t J, int32_t radius /* 1..64 */, float floor /* metres, > 0 */,
                       float *out /* [T,N,J,3], may not alias pose */, uint8_t *code /* [T,N,J] or NULL */,
                       void *workspace, size_t workspace_bytes, void *stream);

/* Bone lengths held constant along a video (pafuse_amd/bones.py states the arithmetic of both entries, operation for
 * operation).  All in fp64 with contraction off, rounded once to fp32.
 *   pose   [T,N,J,3] the per-frame pose, N the frames of the video (NaN: none)
 *   cov    [T,N,J,6] the covariance of its hypotheses (pafuse_frames_finish's cov: xx xy xz yy yz zz), or NULL: all zeros, bit
 *          for bit.  A joint's EFFECTIVE covariance is cov + floor^2*I; it is USABLE under the three leading-minor tests of
 *          pafuse_pose_smooth (a NaN anywhere, or an indefinite matrix, is not)
 *   parent int32 [J]: the joint that joint j's bone hangs on; an entry outside 0 .. j-1 is READ AS -1, no bone - a parent index
 *          is smaller than its child's, so no table can make a walk run on (the Python layers refuse such a table)
 *   floor  metres, finite and > 0: a regulariser that keeps a zero covariance usable, not a tuned value
 *
 * pafuse_bone_lengths - one length per bone and step from the whole video.  Bone j (parent p), frame n: d = x_j - x_p, l = |d|,
 * u = d/l, v = u'E_j u + u'E_p u.  The frame takes part iff the six pose values are finite, l is finite and > 0, both
 * covariances are usable and v is finite and > 0; its weight is w = 1/v: a frame is trusted as far as its hypotheses agree
 * ALONG the bone.  S0 = sum w, S1 = sum w*l, S2 = sum (w*l)*l in the order of the per-frame wave kernels (lane i adds frames
 * i, i + 64, ... ascending, then the butterfly), L = S1/S0, dev = sqrt(max(S2/S0 - L*L, 0)).
 *   mirror int32 [J] or NULL: the left/right partner of joint j or -1.  Bone j and bone m = mirror[j] (in range, != j, itself a
 *          bone) POOL their frames - every lane runs on from the lower-indexed bone's frames into the higher's - so partners
 *          that name each other get the same bits
 *   length [T,J]: L, NaN where j has no bone or no frame takes part;   dev [T,J] or NULL: the weighted standard deviation of the
 *          INPUT's bone length, the known diagnostic;   frames int32 [T,J] or NULL: the frames that took part (both bones')
 * One kernel, one wave per (t, j); no atomics, bit-reproducible.
 *
 * pafuse_bone_project - every frame (t, n), on its own, moved onto the lengths length[t, :] by the least Mahalanobis distance.
 * A joint without a bone (a chain top, such as the root) is PINNED: its E counts as 0 and it never moves.  Bone j is ACTIVE in
 * a frame iff it has a parent, length[t,j] is finite and > 0, both ends are finite and both covariances usable.
 * `iterations` Jacobi sweeps from y = pose.  Phase A, per active bone: d = y_j - y_p, l, u; g_c = E_j u, g_p = E_p u,
 * s = u'g_c + u'g_p (the bone skips the sweep unless l and s are finite and > 0); lam = (l - L)/s, a_j = g_c*lam, b_j = g_p*lam -
 * the exact minimiser of dc'E_c^-1 dc + dp'E_p^-1 dp under the linearised constraint.  Phase B, per joint that is not pinned:
 * n_j = [own bone active] + its active child bones (fixed per frame); y_j += (-a_j + sum of b_k over the children k
 * ascending)/n_j - the averaging keeps Jacobi stable at a wrist with six bones.  snap = 1: afterwards every joint whose bone is
 * active walks up while the bone is active and adds, leaf to root, (y_c - y_p)*(L_c/l_c) (the unscaled difference where l_c is
 * not finite or not > 0) to the y of the joint the walk ends at: the lengths become exact up to the fp32 rounding.
 *   length [T,J] fp32: an INPUT - pafuse_bone_lengths' or the caller's own (a calibration, another video), symmetric or not
 *   out    [T,N,J,3], may not alias pose.  A joint with n_j = 0 keeps the input's bits; no NaN is created; iterations = 0 with
 *          snap = 0 returns the input, bit for bit
 *   code   uint8 [T,N,J] or NULL: 1 the joint is part of an active bone; 0 untouched; 3 untouched although a bone was asked of
 *          it (its own bone or a child's has a length) - a pose that is not finite or an unusable covariance made it impossible
 *   resid  [T,N,2] or NULL: (before, after) the largest |l - L| over the frame's active bones in metres, before on pose, after
 *          ON THE FP32 VALUES RETURNED; NaN: no active bone.  Jacobi converges slowly: `after` without snap shows an unconverged
 *          frame, `before` stays visible behind the snap
 * One kernel, one wave per (t, n), the frame in LDS; no atomics, no workspace, bit-reproducible.
 * Both refuse (PAFUSE_E_ARG) before any HIP call: a null pose, parent, length (or out), T, N or J < 1, J > 256, iterations
 * outside 0 .. 64, snap not 0 or 1, a floor that is not finite and > 0, out == pose, a grid out of range. */
int pafuse_bone_lengths(const float *pose /* [T,N,J,3] */, const float *cov /* [T,N,J,6] or NULL */,
                        const int32_t *parent /* [J] */, const int32_t *mirror /* [J] or NULL */,
                        int32_t T, int32_t N, int32_t J, float floor,
                        float *length /* [T,J] */, float *dev /* [T,J] or NULL */, int32_t *frames /* [T,J] or NULL */, void *stream);
int pafuse_bone_project(const float *pose, const float *cov /* or NULL */, const int32_t *parent,
                        const float *length /* [T,J] */, int32_t T, int32_t N, int32_t J,
                        int32_t iterations /* 0..64 */, int32_t snap /* 0|1 */, float floor,
                        float *out /* [T,N,J,3], may not alias pose */, uint8_t *code /* or NULL */,
                        float *resid /* [T,N,2] or NULL */, void *stream);

/* The focal length of the video's camera from the finished per-frame pose and its detections, part one: the sums per
 * (t, frame) (pafuse_amd/focal.py states the arithmetic).  Operands as pafuse_frames_root_fit, except
 * that of cam only cx, cy = cam[2:4] and the pixel aspect rho = cam[1]/cam[0] are read: cam and cam with fx, fy doubled give
 * the same bits.  With p = u - cx, q = (v - cy)/rho, hx = p*Z, hy = q*Z the pinhole is linear in (1/f; tx, ty, tz/f):
 * X + tx = hx/f + (tz/f)*p, Y + ty = hy/f + (tz/f)*q.  The per-frame directions e_x, e_y and (p, q) are projected out of
 * g = (X, Y) and h = (hx, hy) with the weights c, from thirteen sums over the joints that take part (weight > 0 and a finite
 * pose), fp64, contraction off, every sum in the fixed order of pafuse_frames_root_fit:
 *   K = <h_perp,h_perp>   H = <h_perp,g_perp>   G = <g_perp,g_perp>
 * A frame takes part if at least 4 joints are in the sums, den = Spp - (Sp*Sp + Sq*Sq)/W is finite and > 0 and K, H, G are
 * finite.
 *   state double [T,N,4]   (K, H, G, 1.0) per (t, n); (0, 0, 0, 0) for a frame that takes no part.  States of several videos
 *                          of one camera concatenate along N.
 * One kernel, one wave per (t, n), no workspace, no atomics, bit-reproducible.
 * Refused (PAFUSE_E_ARG) before any HIP call: a null pose / x2d / cam / state, T, N or J < 1, a state that is not 8-byte
 * aligned. */
int pafuse_frames_focal_sums(const float *pose /* [T,N,J,3] whole-body, root-relative */,
                             const float *x2d /* [N,J,2] */, const float *conf /* [N,J] or NULL = all 1 */,
                             const float *cam /* [>=4]: fx fy cx cy */, int32_t T, int32_t N, int32_t J,
                             double *state /* [T,N,4] */, void *stream);

/* Part two: the estimate per t.  K, H, G and the frame count are summed over n as pafuse_frame_errors_reduce sums (lane l
 * adds frames l, l + 64, ... in ascending order, then v += v[lane ^ o] for o = 32 .. 1).  There is an estimate if the count
 * is >= 1, K > 0 and H > 0 - h regressed ON g, the direction that survives pose noise:
 *   focal   [T] fp32   K/H rounded once, in the units of the detections (screen-normalised: pixels = focal * width / 2); NaN
 *                      without an estimate
 *   r2      [T] fp32   (NULL: not wanted) (H*H)/(G*K) rounded once: the fraction of the perspective signal the line explains;
 *                      NaN without an estimate
 *   frames  [T] int32  (NULL: not wanted) the frames that took part
 *   cam_out [T,cam_len] fp32  (NULL: not wanted) (focal, rho*(K/H) in fp64 rounded once, cam[2], ..., cam[cam_len-1]): the
 *                      intrinsics to hand to pafuse_frames_root_fit.  NaN in the first two slots without an estimate, so
 *                      that a video without one gives a NaN trajectory and not a guessed one.
 * The estimate inherits a depth-scale error of the pose one for one, and a single frame or a distant person carries little
 * signal: r2 and frames are what tells.  One kernel, one wave per t, bit-reproducible.
 * Refused (PAFUSE_E_ARG) before any HIP call: a null state / cam / focal, T or N < 1, cam_len outside 4 .. 9, a state that is
 * not 8-byte aligned. */
int pafuse_focal_solve(const double *state /* [T,N,4] */, int32_t T, int32_t N, const float *cam /* [cam_len] */,
                       int32_t cam_len /* 4..9 */, float *focal /* [T] */, float *r2 /* [T] or NULL */,
                       int32_t *frames /* [T] or NULL */, float *cam_out /* [T,cam_len] or NULL */, void *stream);

/* Which way is up: the ground plane of a video from its foot contacts, and the poses in world space (pafuse_amd/ground.py
 * states every operation and its order).  A foot that is not moving is on the ground, and the ground
 * is the plane through those points.  fp64, contraction off, every output rounded once; four kernels, no workspace, no
 * atomics, bit-reproducible.  The chain is foot_contacts, `passes` times (ground_sums, ground_solve), frames_to_world on one
 * stream: a later pass reads the plane and scale of the one before ON THE DEVICE.  speed 0.015 m/frame, gate 2.5, floor
 * 0.005 m, spread 0.03 m, radius 3 and 3 passes are the defaults of the Python layer: defaults, not tuned values.
 *
 * pafuse_foot_contacts: for every (t, n, k) the camera-space point pose[t,m,points[k]] + traj[t,m] goes through the
 * local-linear filter of pafuse_trajectory_smooth (weight 1; a frame takes part if its six values are finite).  Only a line
 * through at least 3 frames counts:
 *   foot       [T,N,K,3] fp32  the line's value at the frame; NaN without such a line
 *   foot_speed [T,N,K]   fp32  (NULL: not wanted) v = |the line's slope|, metres per frame; NaN without
 *   contact    [T,N,K]   fp32  (1 - (v/speed)^2)^2 for v < speed, else 0; 0 without
 * Refused (PAFUSE_E_ARG) before any HIP call: a null pose / traj / points / foot / contact, T, N or J < 1, K outside 1 .. 16,
 * radius outside 1 .. 64, a speed that is not finite and > 0, a grid out of range.  points[k] lies in [0, J) (the caller's
 * promise: it is device memory; a point outside reads nothing and gives NaN, NaN, 0). */
int pafuse_foot_contacts(const float *pose /* [T,N,J,3] root-relative */, const float *traj /* [T,N,3]; NaN: no root */,
                         const int32_t *points /* [K] */, int32_t T, int32_t N, int32_t J, int32_t K /* 1..16 */,
                         int32_t radius /* 1..64 */, double speed /* metres per frame */, float *foot /* [T,N,K,3] */,
                         float *foot_speed /* [T,N,K] or NULL */, float *contact /* [T,N,K] */, void *stream);

/* The sums of every (t, n) over its K points in ascending order.  A point takes part if contact > 0 and its foot and the
 * frame's root are finite; its weight is omega = contact * rho: rho = 1 without a plane (plane and scale NULL: the first
 * pass), else (1 - z*z)^2 for |z| < 1 and 0 beyond, z = (n.p - d)/(gate * scale[t]) with (n, d) = plane[t] (a NaN plane: 0).
 *   state double [T,N,14]  omega; omega*p (3); (omega*p_a)*p_b (xx xy xz yy yz zz, about the camera origin); omega*(root - p)
 *                          (3); the number of points with omega > 0.  A frame whose every weight is 0: exactly 14 zeros.
 *                          States of several videos of one scene concatenate along N.
 * Refused (PAFUSE_E_ARG) before any HIP call: a null foot / contact / traj / state, plane without scale or the reverse, T or
 * N < 1, K outside 1 .. 16, a gate that is not finite and > 0, a state / plane / scale that is not 8-byte aligned. */
int pafuse_ground_sums(const float *foot /* [T,N,K,3] */, const float *contact /* [T,N,K] */, const float *traj /* [T,N,3] */,
                       const double *plane /* [T,4] or NULL */, const double *scale /* [T]; NULL iff plane is */,
                       int32_t T, int32_t N, int32_t K, double gate, double *state /* [T,N,14] */, void *stream);

/* The plane per t.  The slots are summed over n as pafuse_focal_solve sums; mu = S/W, C = M/W - mu mu^T; the eigen
 * decomposition of C is a cyclic Jacobi of 8 fixed sweeps (+ - * / sqrt only), sorted ascending.  With u = sum omega*(root - p):
 *   code 1 plane  lambda1 >= spread^2 and lambda1 >= 9*max(lambda0, floor^2): n = the eigenvector of lambda0
 *   code 2 line   else lambda2 >= spread^2: the contacts lie on a line a; n = normalize(u - (u.a) a)   (a person standing)
 *   code 3 body   else W > 0 and |u| > 0: n = normalize(u)
 *   code 0 none   NaN in every floating-point output, never a guess
 * n is signed so that n.u >= 0 (the root is above the feet), d = n.mu, rms = sqrt(n.C n), sigma = max(floor, rms).
 *   plane double [T,4] (n, d) and scale double [T] (sigma): what the next pafuse_ground_sums and pafuse_frames_to_world read
 *   up [T,3], camera_height [T] (= -d), rms [T], eig [T,3] fp32, points [T] int32, code [T] uint8: each may be NULL
 * One wave per t.  Refused (PAFUSE_E_ARG) before any HIP call: a null state / plane / scale, T or N < 1, a floor or spread
 * that is not finite and > 0, a state / plane / scale that is not 8-byte aligned. */
int pafuse_ground_solve(const double *state /* [T,N,14] */, int32_t T, int32_t N, double floor /* metres */,
                        double spread /* metres */, double *plane /* [T,4] */, double *scale /* [T] */, float *up,
                        float *camera_height, float *rms, float *eig, int32_t *points, uint8_t *code, void *stream);

/* Camera space to world space per t from plane[t]: z = n, x = normalize(e - (e.n) n) with e = (1,0,0), the camera's right
 * ((0,0,1) if |n_x| > 0.99), y = z cross x; p = pose + traj -> (x.p, y.p, n.p - d): the third component of a joint is its
 * height above the ground.  NaN in gives NaN out, a NaN plane (code 0) gives NaN.
 *   pose_world [T,N,J,3] fp32;  traj_world [T,N,3] fp32 (NULL: not wanted) the root traj[t,n] likewise
 * Refused (PAFUSE_E_ARG) before any HIP call: a null pose / traj / plane / pose_world, T, N or J < 1, a plane that is not
 * 8-byte aligned, a grid out of range. */
int pafuse_frames_to_world(const float *pose /* [T,N,J,3] */, const float *traj /* [T,N,3] */, const double *plane /* [T,4] */,
                           int32_t T, int32_t N, int32_t J, float *pose_world /* [T,N,J,3] */,
                           float *traj_world /* [T,N,3] or NULL */, void *stream);

/* Frame-level errors of the per-frame pose against ground truth (pafuse_amd/framemetrics.py states the arithmetic):
 * pose [T,N,J,3] and gt [N,J,3] whole-body and root-relative, traj [T,N,3] / gt_root [N,3] the camera-space root (both or
 * neither).  Every fp32 input is converted to double once; everything after that is fp64 with contraction off:
 * d[n,j] = pose[t,n,j] - gt[n,j], r[n] = traj[t,n] - gt_root[n], |v| = sqrt((v0*v0 + v1*v1) + v2*v2).  A joint takes part in
 * a frame only if the three components of its pose and of its gt are finite.  K = 6 + num_parts slots per (t, n), each
 * the sum of a term over the joints that take part, and their number:
 *   0 mpjpe      |d[n,j]|
 *   1 mpjve      |d[n,j] - d[n-1,j]|                            n >= 1, the joint in both frames (mean_velocity_error, common/loss.py:488)
 *   2 accel      |(d[n+1,j] - d[n,j]) - (d[n,j] - d[n-1,j])|    1 <= n <= N-2, the joint in all three frames
 *   3 root       |r[n]|              one term, count 1          traj given; traj[t,n] and gt_root[n] finite
 *   4 root_vel   |r[n] - r[n-1]|     one term                   traj given, n >= 1, both frames
 *   5 abs_mpjpe  |d[n,j] + r[n]|                                traj given: the camera-space error
 *   6+i          |d[n,j] - d[n,pbroot[j]]| over the joints with part[j] == i whose part root takes part too (the part
 *                re-centred error of pafuse_hypothesis_errors)
 * A slot that is not defined for a frame or has no participant holds 0.0 and 0.  Every sum over j in the fixed order of
 * pafuse_frames_root_fit.  A metric is sum of sums / sum of counts (metres, metres/frame, metres/frame^2).
 *   err double [T,N,K], cnt int32 [T,N,K]
 * One kernel, one wave per (t, n), no workspace, no atomics, bit-reproducible.
 * Refused before any HIP call: a null pose / gt / pbroot / part / err / cnt, traj without gt_root or the reverse, T, N or
 * J < 1 (PAFUSE_E_ARG); num_parts outside 1 .. PAFUSE_MAX_PARTS (PAFUSE_E_SHAPE). */
int pafuse_frame_errors(const float *pose /* [T,N,J,3] */, const float *gt /* [N,J,3] */,
                        const float *traj /* [T,N,3] or NULL */, const float *gt_root /* [N,3]; NULL iff traj is */,
                        const int32_t *pbroot /* [J] root joint of every joint's part */,
                        const int32_t *part /* [J] part of every joint, 0 .. num_parts-1 */, int32_t num_parts, int32_t T,
                        int32_t N, int32_t J, double *err /* [T,N,6+num_parts] */, int32_t *cnt /* [T,N,6+num_parts] */,
                        void *stream);

/* The sums of those maps over the frames: sums double [T,K] and counts int64 [T,K] from err [T,N,K] and cnt [T,N,K].
 * One wave per (t, k): lane l adds frames l, l + 64, ... in ascending order, then v += v[lane ^ o] for o = 32 .. 1.
 * Bit-reproducible, independent of any launch shape.
 * Refused before any HIP call: a null pointer, T or N < 1 (PAFUSE_E_ARG); K outside 7 .. 6 + PAFUSE_MAX_PARTS
 * (PAFUSE_E_SHAPE). */
int pafuse_frame_errors_reduce(const double *err, const int32_t *cnt, int32_t T, int32_t N, int32_t K, double *sums,
                               int64_t *counts, void *stream);

/* Protocol #2 (P-MPJPE) on the same operands - common/loss.py:251-458 as main_h3wb.py:381-395 calls it: every
 * whole-body hypothesis pose (and, per (b,t,f), the mean over h of them) aligned to its whole-body target by the
 * reference's similarity transform (scale, rotation with the reflection fix, translation), in fp64.
 * Outputs: jbest [B,T,F,J] per-joint minimum over h of the aligned error (NaN if any is NaN, like np.min);
 * pbest_sums double [B,T,P,F] sum over j of the aligned errors of every pose; pagg [B,T,F,J] aligned error of the
 * mean pose; jagg [B,T,F,J] aligned error of the hypothesis pafuse_hypothesis_errors picks for J-Agg (smallest 2-D
 * reprojection error of the unaligned pose, first minimum wins; 0 where no reprojection error is finite);
 * pick int32 [B,T,F,J] (may be NULL) that hypothesis (-1 where none).  J <= 256.  Deterministic, no atomics. */
int pafuse_procrustes_errors(const float *pred, const float *gt, const float *x2d, const float *traj, const float *cam,
                             const int32_t *conn, int32_t B, int32_t T, int32_t P, int32_t F, int32_t J, float *jbest,
                             double *pbest_sums, float *pagg, float *jagg, int32_t *pick, void *stream);

/* Protocol #2 from per-shard partial states (opt-in: harness.evaluate_sequence(p2_gather="partials")).  Per (b,t,f) every
 * hypothesis is aligned on its own, so a shard [h0, h0 + P_r) reduces to a state whose head does not depend on P.
 * pred [B,T,P_r,F,J,3] is the LOCAL tensor; the other operands are those of pafuse_procrustes_errors.  J <= 256.
 * State, one flat 8-byte aligned buffer of pafuse_procrustes_partials_bytes = 16*n + 8*T*P_r bytes, n = B*T*F*J:
 *   float  jbest[n]     minimum over the local h of the aligned per-joint error, NaN-sticky (+inf when P_r == 0)
 *   float  e2[n], sel[n]; int32 idx[n]   the J-Agg candidate: smallest reprojection error (the fp32 expression of
 *                       pafuse_hypothesis_errors), that hypothesis's aligned error, its GLOBAL index h0 + h; first minimum
 *                       wins; (+inf, 0, -1) where no e2 of the shard is finite
 *   double psum[P_r][T] per local hypothesis and step: sum over (b, f) of the per-pose sums over j of the aligned errors
 *                       (pbest_sums of pafuse_procrustes_errors reduced in one fixed order: the same bits however P is cut)
 * The tail is at the end: a ragged shard is a prefix of a buffer sized for the largest one.  The state holds no sums for
 * the P-Agg mean pose - pafuse_procrustes_combine borrows them.  workspace: pafuse_procrustes_partials_workspace_bytes bytes,
 * 8-byte aligned (the per-pose sums [B,T,P_r,F]).  Two kernels, no atomics, bit-reproducible.  B == 0 or P_r == 0: no
 * kernel runs, the state is the neutral one.  Refused: a null operand, negative sizes or h0, a short state (PAFUSE_E_ARG),
 * J > 256 (PAFUSE_E_SHAPE), a small workspace (PAFUSE_E_WORKSPACE). */
size_t pafuse_procrustes_partials_bytes(int32_t B, int32_t T, int32_t P_r, int32_t F, int32_t J);
size_t pafuse_procrustes_partials_workspace_bytes(int32_t B, int32_t T, int32_t P_r, int32_t F, int32_t J);
int pafuse_procrustes_partials(const float *pred, const float *gt, const float *x2d, const float *traj, const float *cam,
                               const int32_t *conn, int32_t B, int32_t T, int32_t P_r, int32_t F, int32_t J, int32_t h0,
                               void *state, size_t state_bytes, void *workspace, size_t workspace_bytes, void *stream);

/* Combines W such states, `stride_bytes` apart and in ascending-h0 order; only the first 16*n bytes of each are read
 * (concatenate the psum tails).  Per joint: the NaN-sticky minimum of the minima; the candidate with the smallest e2 and,
 * among equal ones, the lowest global index.  sums (NULL unless pagg is wanted): W arrays double[n][3], `sums_stride_bytes`
 * apart - the heads of the Protocol #1 states (pafuse_hypothesis_partials) or pose states (pafuse_pose_partials) of the
 * same shards, which both begin with the fp64 sum over h of the whole-body joint.  They are added in shard order, divided
 * by P_total in fp64, and that mean pose is aligned once against the target gt [B,F,J,3] (conn int32 [J]).
 * Writes any of (NULL: not wanted, at least one):
 *   merged  the 16*n-byte head of the union's state; of the operands it may only lie over the FIRST state
 *   jbest, pagg, jagg [B,T,F,J] fp32, pick [B,T,F,J] int32: what pafuse_procrustes_errors writes for all hypotheses.
 *           jbest, jagg and pick are bit-equal to it; pagg sums the mean pose per shard first (fp64 roundings apart).
 *           jagg is 0 and pick is -1 where no state holds a candidate.
 * Refused: null operands, negative sizes, W < 1, P_total < 1, pagg without sums, close or misaligned states
 * (PAFUSE_E_ARG), J > 256 (PAFUSE_E_SHAPE). */
int pafuse_procrustes_combine(const void *states, int32_t W, size_t stride_bytes, const void *sums,
                              size_t sums_stride_bytes, const float *gt, const int32_t *conn, int32_t B, int32_t T,
                              int32_t F, int32_t J, int32_t P_total, void *merged, float *jbest, float *pagg, float *jagg,
                              int32_t *pick, void *stream);

/* Replays the GEMM launches of one flip-TTA denoiser pass (all three parts) back to back on `stream`, for
 * bench.py's per-kernel roofline measurement: returns the number of launches, adds their algorithmic FLOPs to
 * *flops.  Uses (and overwrites) the workspace like pafuse_d3dp_sample does. */
int pafuse_d3dp_replay_gemms(const pafuse_d3dp_config *cfg, int32_t B, int32_t P, void *workspace,
                             size_t workspace_bytes, void *stream, double *flops);
/* The same for a subset of the four linear layers of every block: layer_mask bits 1 = qkv, 2 = proj, 4 = fc1 (+GELU),
 * 8 = fc2 (15 = pafuse_d3dp_replay_gemms).  bench.py times each layer kind alone for the per-kernel roofline lines. */
int pafuse_d3dp_replay_layers(const pafuse_d3dp_config *cfg, int32_t B, int32_t P, void *workspace,
                              size_t workspace_bytes, void *stream, int32_t layer_mask, double *flops);

/* ---- Training: MixSTE2 in train mode and its backward -------------------------------------------
 * Replaces MixSTE2.forward with is_train=True (common/mixste.py:215-225,260-298: no hypothesis axis, DropPath on
 * both residual branches of every Block :113-116) and what autograd derives from it.
 *   x2d [B,F,J,2], x3d [B,F,J,3] (the noised target), t [B] -> out [B,F,J,3]
 *   drop_path: NULL (no DropPath) or float [2*depth][2][B*max(F,J)] - for block k in execution order (STE0, TTE0,
 *              STE1, ...) and branch (0 attention, 1 MLP) the factor mask/keep_prob of every sequence (spatial
 *              blocks: B*F sequences (b,f); temporal blocks: B*J sequences (b,j)), as timm's DropPath draws it.
 *   saved:     pafuse_mixste2_train_bytes(w, B) bytes; the forward leaves the activations the backward needs there.
 * Backward: dout [B,F,J,3] -> ADDS the gradient of every parameter into the buffer the like-named pointer of `grads`
 * addresses (same struct as the weights; `freqs` and the dimensions are ignored).  All row reductions are two-stage
 * in a fixed order: bit-reproducible, no atomics.  `side_stream` (may be NULL): a second HIP stream the weight-gradient
 * GEMMs run on next to the input-gradient chain (forked and joined with events inside the call; results identical).
 * w->operand_bf16: 0 = every GEMM on the fp32 matrix cores; 2 = split-precision products in the GEMMs of the step
 * (qkv, fc1, the whole-row proj / fc2, every dX and dW; fp32-equivalent, gradients within the same bounds); 1 is refused.
 * B is bounded by the reduction partials of the time embedding's gradient, 32 B C floats of 18.9 M: B <= 1536 at C = 384
 * (PAFUSE_E_SHAPE above that, from both calls, before any launch). */
size_t pafuse_mixste2_train_bytes(const pafuse_mixste2_weights *w, int32_t B);
int pafuse_mixste2_train_forward(const pafuse_mixste2_weights *w, const float *x2d, const float *x3d, const int64_t *t,
                                 int32_t B, const float *drop_path, float *out, void *saved, size_t saved_bytes,
                                 void *stream);
int pafuse_mixste2_train_backward(const pafuse_mixste2_weights *w, const pafuse_mixste2_weights *grads,
                                  const float *dout, int32_t B, const float *drop_path, void *saved, size_t saved_bytes,
                                  void *stream, void *side_stream);

/* D3DP.prepare_diffusion_concat + q_sample (common/diffusionpose.py:319-326,358-374) for B samples of per_sample
 * floats: out = clamp(sqrt_acp[t_b] * (x0*scale) + sqrt_1m_acp[t_b] * noise, +-1.1 scale) / scale, in fp64 as the
 * reference's fp64 buffers force, cast to fp32. */
int pafuse_d3dp_qsample(const float *x0, const float *noise, const int64_t *t, const double *sqrt_alphas_cumprod,
                        const double *sqrt_one_minus_alphas_cumprod, double scale, float *out, int32_t B,
                        int64_t per_sample, void *stream);

/* Training draws of noise stream v1 (host statement: pafuse_amd/noise.py reference_train_draws and
 * reference_droppath).  Philox4x32-10 under the key (seed, call), call = the model's training forward passes; g = the GLOBAL
 * index of a clip; counter word 3 takes three values reserved at the top of its range (the sampling loop's word 3 is its
 * draw number, an int32 counted up from 0: at most 2^31 - 1):
 *   noise of (f, j)    counter (f*J + j, 0, g, 0xFFFFFFFF)   the three normals of the stream, as pafuse_noise_fill draws them
 *   timestep of g      counter (0, 0, g, 0xFFFFFFFE)         t = (uint64(r0) * num_timesteps) >> 32
 *   DropPath           counter (s, (denoiser << 16) | (k << 1) | branch, g, 0xFFFFFFFD)   keep iff (r0 + 0.5) 2^-32 < keep[k]
 * key4_dev: four uint32 IN DEVICE MEMORY, {seed, call, first, stride}: local clip i of the call is global clip
 * g = first + i * stride.  The library reads the words on the device and never synchronises, so it cannot check them: the
 * CALLER must make sure that stride >= 1 and first + (B - 1) * stride < 2^32 (pafuse_amd.ops.train_key does).
 *
 * pafuse_d3dp_qsample_seeded: pafuse_d3dp_qsample on B clips of F x J joints with (t, noise) drawn inside the kernel; the
 * arithmetic that consumes them is the same, so `out` equals pafuse_d3dp_qsample fed t_out and noise_out, bit for bit.
 * sqrt_alphas_cumprod / sqrt_one_minus_alphas_cumprod: num_timesteps doubles each.  t_out [B] int64; noise_out [B,F,J,3]
 * or NULL (the normals are then never stored). */
int pafuse_d3dp_qsample_seeded(const float *x0, const uint32_t *key4_dev, const double *sqrt_alphas_cumprod,
                               const double *sqrt_one_minus_alphas_cumprod, double scale, int32_t num_timesteps,
                               float *out, int64_t *t_out, float *noise_out, int32_t B, int32_t F, int32_t J,
                               void *stream);

/* The drop_path table of pafuse_mixste2_train_forward for one denoiser, float [2*depth][2][B*max(F,J)], in one launch.  Block k
 * in execution order (even: spatial, sequences (b, f), L_k = F; odd: temporal, sequences (b, j), L_k = J), branch 0 attention /
 * 1 MLP: column i * L_k + s holds factor[k] if the draw of sequence s of local clip i keeps the branch, else 0; the columns
 * beyond B * L_k hold 1.  keep [2*depth] doubles (1 - rate of block k) and factor [2*depth] floats (1 / keep as the caller's
 * framework rounds it) in device memory: the kernel compares and selects.  denoiser < 2^16 (the part's index: the parts draw
 * independently), depth <= 2^14, out_floats = the floats `out` holds (PAFUSE_E_ARG if fewer than the table's). */
int pafuse_train_droppath_fill(const uint32_t *key4_dev, int32_t denoiser, int32_t depth, int32_t F, int32_t J, int32_t B,
                               const double *keep, const float *factor, float *out, int64_t out_floats, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PAFUSE_HIP_H */
