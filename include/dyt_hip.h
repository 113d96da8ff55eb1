/*
 * dyt_hip.h -- C ABI of libdyt_hip.so: the MI355X (gfx950) implementation of the
 * Dynamic-Tuning ViT-B/16 fine-tune hot path.
 *
 * The reference (NUS-HPC-AI-Lab/Dynamic-Tuning) has no FFI: its hot path sits behind a
 * Python nn.Module API.  This header is therefore the boundary a
 * maintainer binds with ctypes from the reference's module files; every entry point cites
 * the reference interface it replaces (paths relative to the reference root).
 * INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - every function returns 0 (DYT_OK) or a negative error code; no exceptions cross the
 *     ABI; dyt_last_error() returns a thread-local message for the last failure;
 *   - all tensor arguments are DEVICE pointers owned by the caller (torch allocates them);
 *     the library never frees them and never synchronises the host with the device;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it;
 *   - the library owns (hipMalloc) only its private copies of the frozen weights and its
 *     activation workspace, both sized at dyt_ctx_create();
 *   - one context per process / device; thread-compatible, not thread-safe.
 */
#ifndef DYT_HIP_H
#define DYT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DYT_OK 0
#define DYT_ERR_ARG (-1)     /* bad argument / unsupported shape */
#define DYT_ERR_HIP (-2)     /* a HIP runtime call failed */
#define DYT_ERR_STATE (-3)   /* call order violated (e.g. backward without a saved forward) */

/* arithmetic mode of the dense contractions (dyt_config::precision).  The library is built twice from the same sources:
 * libdyt_hip.so (16-bit operand type bfloat16) and libdyt_hip_f16.so (-DDYT_FP16: IEEE half; dyt_operand_type() tells which).
 * Together with DYT_OPT_F32_SPLIT16 (below) that gives the eight host-side precision names of dynamic-tuning_amd/runtime.py:
 *   "fp32"     either library, DYT_PREC_FP32                      exact fp32 on the matrix cores (v_mfma_f32_32x32x2_f32)
 *   "bf16"     libdyt_hip.so,     DYT_PREC_BF16                   bf16 MFMA operands, fp32 accumulate / residual stream / statistics
 *   "fp16"     libdyt_hip_f16.so, DYT_PREC_BF16 (its 16-bit mode) IEEE-half operands, gradient operands x 2^12 (the default)
 *   "fp16x3"   libdyt_hip_f16.so, DYT_PREC_FP32 + SPLIT16 = 1     every frozen-weight product as three half products, fp32 data flow
 *   "fp16x3f"  ... SPLIT16 = 2                                    the same forward, gradient products hi * hi (fp32-width backward)
 *   "fp16x3h"  ... SPLIT16 = 3                                    the same forward, backward pass on 16-bit operands (fp16 mode's kernels)
 *   "fp16x3q"  ... SPLIT16 = 5                                    as 3 with qkv / proj as hi * hi + two fp8 correction products
 *   "fp16f8"   ... SPLIT16 = 4                                    as 3 with every forward GEMM in that fp8-correction form
 * In the two 16-bit modes LayerNorm-2 is folded into the fc1 GEMM (per-row statistics from the proj epilogue, gamma / beta folded into
 * the frozen fc1 weight copy, normalisation in the fc1 epilogue: DESIGN.md section 5).  DYT_LN_FOLD=0 in the environment when
 * dyt_create runs keeps it a separate kernel (LayerNorm in fp32, then rounded: the order of the reference's autocast). */
#define DYT_PREC_FP32 0 /* exact: fp32 operands, fp32 accumulate -- the parity mode */
#define DYT_PREC_BF16 1 /* fast: 16-bit MFMA operands (bfloat16 or IEEE half by build), fp32 accumulate, fp32 residual stream */

/* dyt_forward flags */
#define DYT_F_TRAINING 1       /* model.train(): Gumbel noise + adapter dropout (dynamic_adapter.py:29-42,127) */
#define DYT_F_COMPLETE 2       /* forward(x, complete_model=True): mask not applied (vision_transformer_IN21K.py:161) */
#define DYT_F_SAVE 4           /* keep activations of this pass in `slot` for dyt_backward */
#define DYT_F_MASKED_DENSE 8   /* student pass computes the MLP for every token and multiplies by the
                                  mask, exactly as the reference trains (vision_transformer_IN21K.py:159-162), so
                                  the gate of a DROPPED token still receives <dL/dx', mlp(x)>; its backward is
                                  compacted all the same (rows of mask * dL/dx' of dropped tokens are exactly zero):
                                  the reference's gradients at 133.5 instead of 139.6 GFLOP / image.
                                  Default is the compacted MLP of models/model_speed_test.py:274-310, forward too */
#define DYT_F_ACCUM_GRAD 32    /* dyt_step_fwd_bwd: add to grad_flat instead of overwriting it -- gradient accumulation over
                                  accum_iter micro-batches (engine_finetune.py:43-46,66-76; fold 1/accum_iter into dyt_adamw's grad_scale) */
#define DYT_F_DEVICE_SEED 64   /* the Philox seed is read from the context's device-side seed word (dyt_seed) instead of the
                                  `seed` argument, and dyt_step_fwd_bwd advances that word by one when it is done: a step
                                  captured into a hipGraph then draws fresh Gumbel noise / dropout masks at every replay */
#define DYT_F_TOKENS_IN 128    /* dyt_forward: `images` is the residual stream [B,197,768] itself (no patch embedding) -- stand-alone
                                * Block.forward on a token tensor, as block_flops_dict.py:36-46 calls it; forward only */
#define DYT_F_TOKENS_OUT 256   /* dyt_forward: `logits` receives the block stack's output tokens [B,197,768] (no final norm / head) */
#define DYT_F_GATE_ALWAYS 16   /* also evaluate the token dispatcher in a COMPLETE pass (the reference does,
                                  and discards it, :150-152) so token_select/token_logits are returned */
#define DYT_F_IMAGES_U8 512    /* dyt_forward, dyt_step_fwd_bwd: `images` is a `const uint8_t*` batch [B,3,224,224] of raw 0..255 pixels, 16-byte
                                  aligned.  The patch embedding normalises it in its load: ((float)u / 255.0f - mean[c]) / std[c], three
                                  correctly rounded fp32 operations -- torchvision's ToTensor() + Normalize(mean, std) -- with the
                                  context's statistics (dyt_set_input_norm; ImageNet until it is called).  From the embedding GEMM's
                                  operand onwards the pass is bit for bit the float pass on that normalised image, in every precision
                                  mode.  Both passes of dyt_step_fwd_bwd read the bytes.  Not with DYT_F_TOKENS_IN (DYT_ERR_ARG). */
#define DYT_F_IMAGES_NHWC 1024 /* with DYT_F_IMAGES_U8 only (else DYT_ERR_ARG): the byte batch is channels-last, [B,224,224,3] -- what
                                  image decoders produce */

/* parameter ids (frozen unless marked T = trainable); `layer` is the block index, or 0 */
enum dyt_param {
    DYT_P_CLS = 0,      /* cls_token [1,1,768] */
    DYT_P_POS,          /* pos_embed [1,197,768] */
    DYT_P_PE_W,         /* patch_embed.proj.weight [768,3,16,16] */
    DYT_P_PE_B,         /* patch_embed.proj.bias [768] */
    DYT_P_LN1_W, DYT_P_LN1_B,     /* blocks.i.norm1 */
    DYT_P_QKV_W, DYT_P_QKV_B,     /* blocks.i.attn.qkv [2304,768] */
    DYT_P_PROJ_W, DYT_P_PROJ_B,   /* blocks.i.attn.proj [768,768] */
    DYT_P_LN2_W, DYT_P_LN2_B,     /* blocks.i.norm2 */
    DYT_P_FC1_W, DYT_P_FC1_B,     /* blocks.i.mlp.fc1 [3072,768] */
    DYT_P_FC2_W, DYT_P_FC2_B,     /* blocks.i.mlp.fc2 [768,3072] */
    DYT_P_NORM_W, DYT_P_NORM_B,   /* norm */
    DYT_P_AD_DOWN_W, DYT_P_AD_DOWN_B, /* T blocks.i.adaptmlp.down_proj [r,768] */
    DYT_P_AD_UP_W, DYT_P_AD_UP_B,     /* T blocks.i.adaptmlp.up_proj [768,r] */
    DYT_P_GATE_W, DYT_P_GATE_B,       /* T blocks.i.mlp_token_select.mlp_head [1,768] */
    DYT_P_HEAD_W, DYT_P_HEAD_B,       /* T head [C,768] */
    /* video model only (cfg.frames > 1): the attentive pooling head, all trainable (missing from the
     * ViT checkpoint) -- video_models/video_vision_transformer_IN21K.py:27-110,407-410 */
    DYT_P_POOL_QUERY,                     /* T query_token [1,1,768] */
    DYT_P_POOL_NQ_W, DYT_P_POOL_NQ_B,     /* T attentive_blocks.norm_q */
    DYT_P_POOL_NK_W, DYT_P_POOL_NK_B,     /* T attentive_blocks.norm_k */
    DYT_P_POOL_NV_W, DYT_P_POOL_NV_B,     /* T attentive_blocks.norm_v */
    DYT_P_POOL_Q_W, DYT_P_POOL_K_W, DYT_P_POOL_V_W,   /* T attentive_blocks.cross_attn.{q,k,v}.weight [768,768] */
    DYT_P_POOL_Q_BIAS, DYT_P_POOL_V_BIAS,             /* T attentive_blocks.cross_attn.{q_bias,v_bias} [768] */
    DYT_P_POOL_PROJ_W, DYT_P_POOL_PROJ_B,             /* T attentive_blocks.cross_attn.proj [768,768] */
    DYT_P_AD_SCALE,     /* T blocks.i.adaptmlp.scale [1] -- only with tuning_config.ffn_adapter_scalar == "learnable_scalar" (DYT_OPT_LEARNABLE_SCALE) */
    DYT_P_AD_LN_W, DYT_P_AD_LN_B,   /* T blocks.i.adaptmlp.adapter_layer_norm_before.{weight,bias} [768] -- only with dyt_config::adapter_ln != 0 */
    DYT_P_FC_NORM_W, DYT_P_FC_NORM_B,   /* T fc_norm.{weight,bias} [768] -- only with DYT_CREATE_FC_NORM / DYT_CREATE_AVG_POOL (ABI v5) */
    DYT_P_COUNT
};

/* Replaces the constructor arguments of vit_base_patch16_224_in21k(num_classes, tuning_config,
 * select_config) -- models/vision_transformer_IN21K.py:199-323,414-421.  Fixed by the factory:
 * patch 16, dim 768, depth 12, heads 12, mlp_ratio 4, qkv_bias, LayerNorm eps 1e-6. */
typedef struct dyt_config {
    int32_t num_classes;     /* head width C */
    int32_t ffn_num;         /* adapter bottleneck r (tuning_config.ffn_num), 1..64 */
    int32_t depth;           /* 12 */
    int32_t precision;       /* DYT_PREC_* */
    int32_t max_batch;       /* images per call the workspace is sized for */
    int32_t slots;           /* saved-activation slots (2: student + teacher pass) */
    float adapter_scale;     /* tuning_config.ffn_adapter_scalar (0.1 main_image.py:192, 1.0 main_vtab.py:185) */
    float adapter_dropout;   /* 0.1, vision_transformer_IN21K.py:133 */
    float tau;               /* 5, dynamic_adapter.py:59 */
    float threshold;         /* 0.5, dynamic_adapter.py:59 */
    int32_t frames;          /* 0/1: image model.  t > 1: video model (video_models/video_vision_transformer_IN21K.py:
                                435-483) -- `images`/`batch` of every call are the b*t frames of b clips, clip-major
                                ("b c t h w -> (b t) c h w"), batch % t == 0; logits / targets have b = batch/t rows;
                                the cls-pooling head is replaced by the attentive pooling head over the t*197
                                final-norm tokens of a clip (one query, 12 heads) */
    int32_t adapter_ln;      /* tuning_config.ffn_adapter_layernorm_option (models/dynamic_adapter.py:88,95-98,121-122,132-133): 0 = "none" (every
                                shipped script), 1 = "in": the adapter reads LayerNorm(u) (its own trainable nn.LayerNorm(768), eps 1e-5), 2 = "out":
                                the scaled adapter output goes through that LayerNorm before it joins the residual stream.  Adds the two
                                [768] tensors DYT_P_AD_LN_W / _B per block to the flat trainable layout.  Generic row kernels (no fusion, no
                                cls-only tail); image model only.  (ABI v2: the field was appended in round 6.) */
    int32_t inference_only;  /* 0: the training layout (every pass kind, two slots of saved activations, the backward's transients and weight
                                images).  1: a context for eval forwards alone -- ONE set of per-block buffers shared by all `depth` blocks, one
                                slot (every slot index runs in it), two residual streams used in turn, the forward's transients, and none of the
                                transposed / fragment-order weight images only the gradient GEMMs read.  Results are bit-identical to the same
                                eval forward in a training-layout context.  dyt_forward with DYT_F_SAVE, dyt_backward, dyt_step_fwd_bwd,
                                dyt_allreduce_grads, dyt_clip_grad_norm, dyt_set_soft_targets, dyt_set_drop_path(_scales) with a non-zero
                                argument, dyt_mlp_gathered_bwd and the saved-pass accessors (dyt_debug_dispatch / _dact / _drop_path) return
                                DYT_ERR_ARG (the text names inference_only) before anything is enqueued.  dyt_adamw* take no context: their
                                caller refuses (runtime.DyTEngine).
                                (ABI v3: appended last.) */
} dyt_config;

typedef struct dyt_ctx dyt_ctx;

const char* dyt_last_error(void);
int dyt_version(void);
/* the 16-bit operand type DYT_PREC_BF16 selects in THIS build of the library: 0 bfloat16 (libdyt_hip.so), 1 IEEE half
 * (libdyt_hip_f16.so, same sources compiled with -DDYT_FP16; the reference's own autocast dtype, engine_finetune.py:47) */
int dyt_operand_type(void);

int dyt_ctx_create(const dyt_config* cfg, dyt_ctx** out);
/* dyt_ctx_create with creation flags (ABI v4); dyt_ctx_create(cfg, out) is dyt_ctx_create_ex(cfg, 0, out).  Unknown bits: DYT_ERR_ARG.
 *   DYT_CREATE_WIDE_HEAD  the classification head (final LayerNorm of the cls rows + Linear(768, num_classes), forward and backward)
 *                         runs as exact-fp32 MFMA GEMMs (csrc/head_wide.hip) and num_classes may be 1 ... 65 536 -- the
 *                         ImageNet-21K classifier has 21 843 rows -- instead of the row kernels' 1 ... 1024.  An explicit form, not a
 *                         lifted limit: the wide kernels sum in another order (the head's dx over class slices of 1024 added in
 *                         ascending order), so their results differ from the row kernels' in the last bits and the row-kernel head
 *                         stays the bit-pinned default.  Below 1025 classes both forms run on the same weights.  fp32 arithmetic in
 *                         every precision mode, no atomics: bit-reproducible run to run.  Image model only (frames > 1: DYT_ERR_ARG);
 *                         valid together with dyt_config::inference_only.  Adds [ceil(C/1024)][max_batch][768] floats per slot to
 *                         the training layout. */
#define DYT_CREATE_WIDE_HEAD 1u
/* The reference's global_pool / fc_norm constructor arguments (models/vision_transformer_IN21K.py:205,216,259-261,314-317; forward_head
 * :375-380).  ABI v5.  With neither bit set every offset, launch and result bit is what it was.
 *   DYT_CREATE_FC_NORM    the head's LayerNorm (eps 1e-6, the arithmetic of the final norm on the cls rows) is the reference's `fc_norm`
 *                         (:316, applied at :378) and the final `norm` is an identity (:314).  Its weight and bias are TRAINABLE -- the
 *                         ViT-B/16 IN21K checkpoint has no fc_norm.*, so the freeze rule of main_image.py:250-256 leaves them on -- and
 *                         live in the caller's flat buffer as DYT_P_FC_NORM_W / DYT_P_FC_NORM_B: two [768] tensors directly behind
 *                         head.bias, inside part 0 of dyt_grad_part (final when the head's backward is, before any block's).
 *                         dyt_trainable_offset serves the two ids in such a context only; dyt_set_frozen(DYT_P_NORM_W / _B) returns
 *                         DYT_ERR_ARG there (the text names the flag).  The head backward additionally leaves dy = dlogits W_head
 *                         ([max_batch][768] per slot, training layout, counted by dyt_ctx_bytes) and one kernel adds
 *                         d_gamma[c] += sum_b dy[b][c] xhat[b][c], d_beta[c] += sum_b dy[b][c] in ascending image order, xhat recomputed
 *                         from the saved (mean, rstd) and the LayerNorm's input row.
 *   DYT_CREATE_AVG_POOL   global_pool='avg' (:377): the row fed to that LayerNorm is the mean of the 196 patch-token rows of the last
 *                         block's output, cls row excluded, instead of the cls row.  Goes with DYT_CREATE_FC_NORM (the reference's default
 *                         for 'avg', :261) and switches the cls-only tail off (DYT_OPT_CLS_TAIL stays 0: every patch token of the last
 *                         block reaches the head).  Per output channel the 196 rows are summed as 7 runs of 28 consecutive rows, each run
 *                         a chain in ascending token order, the run sums added in ascending order, the result divided by 196.  The
 *                         backward writes the whole gradient stream once: cls rows exactly 0, every patch row dpooled / 196.
 *                         Adds [max_batch][768] floats per slot.  The bit is given TOGETHER with DYT_CREATE_FC_NORM (6u): on its own it
 *                         would be the reference's ('avg', fc_norm=False) -- LayerNorm over all 197 rows in front of the mean, with the
 *                         frozen norm -- which has no HIP path and returns DYT_ERR_ARG (the text names create_flags and both bits).
 *                         runtime.DyTEngine(avg_pool=True) and the models' global_pool='avg' set both.
 * Both are image-model flags (frames > 1: DYT_ERR_ARG) and combine with DYT_CREATE_WIDE_HEAD, dyt_config::inference_only,
 * dyt_config::adapter_ln and every precision mode; the head stays fp32, without atomics, bit-reproducible. */
#define DYT_CREATE_AVG_POOL 2u
#define DYT_CREATE_FC_NORM 4u
int dyt_ctx_create_ex(const dyt_config* cfg, uint32_t create_flags, dyt_ctx** out);
int dyt_ctx_destroy(dyt_ctx* ctx);
/* bytes of device memory the context holds (weights + workspace) */
int dyt_ctx_bytes(const dyt_ctx* ctx, int64_t* bytes);

/* Scheduling options (results are identical either way; both default to on):
 *   DYT_OPT_STREAM_OVERLAP  0: everything on the caller's stream.  1 (default): dyt_step_fwd_bwd runs the student and the
 *                           teacher pass on two streams (fork/join with events on the caller's stream).  2: additionally
 *                           the adapter branch of every block on its own stream, 3: only that -- both measured SLOWER
 *                           than 1 whenever the branch streams really get their own hardware queues (26.1 vs 31.5 /
 *                           30.0 ms per step at B=128 with a hardware queue per stream; the serial step is 29.5 ms), kept for
 *                           measurement only.  4: the two FORWARD passes overlap, the teacher's backward starts after the
 *                           student's -- like 0 a bit-reproducible schedule, 29.0 instead of 26.1 ms
 *   DYT_OPT_CLS_TAIL        last block: evaluate MLP + adapter (forward and backward) for the cls rows
 *                           only -- only x[:,0] reaches forward_head (vision_transformer_IN21K.py:375-380)
 *   DYT_OPT_SHARE_BLOCK0    dyt_step_fwd_bwd: the teacher pass reuses the student pass's patch embedding and
 *                           block-0 attention branch (same images, frozen weights, nothing random before it) */
#define DYT_OPT_STREAM_OVERLAP 1
#define DYT_OPT_CLS_TAIL 2
#define DYT_OPT_SHARE_BLOCK0 3
/*   DYT_OPT_COUNT_FLOPS_TOKENS  value n in 1..197 (0 = off): the FLOP-probe variant of the reference,
 *                           Block.forward_count_flops (vision_transformer_IN21K.py:167-185, driven by
 *                           block_flops_dict.get_block_flops :33-55 through `count_flops` / `token_select_num`): every
 *                           block runs its MLP on the FIRST n tokens of each image (cls + the first n-1 patch tokens)
 *                           whatever the gate decides; token_select reports that forced pattern.  This one DOES change
 *                           results. */
#define DYT_OPT_COUNT_FLOPS_TOKENS 4
/*   DYT_OPT_GRAD_SCALE_LOG2     value k in 0..24: the gradient is multiplied by 2^k wherever the library holds it in its 16-bit
 *                               operand type (g_at, dZ, dA2, dqkv ...) and divided again where it returns to fp32 -- a fixed loss
 *                               scale that never leaves the library (what the reference's GradScaler does for its fp16 autocast,
 *                               misc.py:252-272).  Default: 0 in libdyt_hip.so (bf16 has fp32's exponent range), 12 in
 *                               libdyt_hip_f16.so.  Returned gradients are unscaled either way. */
#define DYT_OPT_GRAD_SCALE_LOG2 5
/*   DYT_OPT_FC2_CAT             1 (default): in the 16-bit modes the adapter's up-projection is computed as the leading
 *                           k-tile of the fc2 contraction (x_out = u + [d_act | h][s Wup | W2]^T + b: one pass over the
 *                           fp32 residual stream instead of two, no up-projection launch) in every compacted or
 *                           complete pass (training student pass: the gate gradient is corrected for the adapter term).  0: always two launches (reference op
 *                           order, models/vision_transformer_IN21K.py:157-163).  fp32 mode: ignored (always two launches). */
#define DYT_OPT_FC2_CAT 6
/*   DYT_OPT_ATTN_BWD_FUSED      1 (default): 16-bit modes run the attention backward of a head (dQ and dK/dV) in ONE persistent
 *                           kernel (q, dO, o read once; delta never leaves the chip); 0: two kernels (bit-identical results);
 *                           2: the fused kernel with the per-wave k / v / o rows prefetched a head ahead.  PROCESS-wide. */
#define DYT_OPT_ATTN_BWD_FUSED 7
/*   DYT_OPT_F32_SPLIT16         fp32 mode only, default 0.  1: every GEMM against a FROZEN weight runs on the 16-bit matrix cores as
 *                           three products hi*hi + hi*lo + lo*hi (both fp32 operands split into two 16-bit parts, one contraction
 *                           over the K-concatenated parts, fp32 accumulate, the fp32 epilogues): the per-GEMM error of the exact
 *                           fp32 MFMA kernel (1-2e-6 of max|C| with IEEE-half parts) at ~2.7x its speed; the attention forward and
 *                           backward likewise (DYT_SPLIT_ATTN=0 keeps the exact-fp32 attention kernels).  LayerNorm, adapter-sized
 *                           GEMMs and every row kernel stay exact fp32.  Host-side precision name: "fp16x3".
 *                           2 ("fp16x3f"): the forward pass as in 1 -- logits, token-keep decisions, losses and saved activations
 *                           are those of value 1 bit for bit -- while every GRADIENT product takes the hi*hi term alone (the
 *                           frozen-weight dgrad GEMMs contract dY_hi * W_hi; the attention backward's dP / dQ / dK / dV likewise, its
 *                           score recomputation keeps three products): gradients within 7e-4 relative L2 of the fp32 oracle
 *                           (value 1: 1.5e-4; the bar of the exact mode's test: 2e-3) at 0.81x the step time of value 1.
 *                           3 ("fp16x3h"): the forward as in 1 bit for bit, with what the backward pass reads saved in the 16-bit
 *                           operand type next to / instead of the fp32 tensors (q / k / v as hi + lo planes from the QKV epilogue, the
 *                           attention output, u, gelu'(z), the MLP output and the adapter bottleneck from their producers; ReLU /
 *                           dropout / gate masks are the exact forward's), and the BACKWARD pass on the 16-bit mode's data flow and
 *                           kernels (gradient operands x 2^12): gradients within 1.4e-3 of the oracle over five seeds, 0.85x the
 *                           step time of value 2.
 *                           4 ("fp16f8"): as 3, every forward GEMM as hi * hi on the f16 matrix cores + the two correction products
 *                           hi * lo + lo * hi on the fp8 (e4m3) ones (v_mfma_scale_f32_16x16x128_f8f6f4, twice the f16 rate per k: a
 *                           2K- instead of a 3K-equivalent contraction; operand images [hi16 | e4m3 hi | e4m3 lo 2^12], weights with a
 *                           per-matrix power of two, descaled by the MFMA's E8M0 scale operand): per GEMM 2e-5 of max|C| (three-part
 *                           1-2e-6, plain half 4e-4), logits ~5e-5, gate logits ~5e-5 from the fp32 reference -- inside the 1e-3 logit
 *                           bar, but token-keep decisions within ~1e-5 of the threshold can differ.
 *                           5 ("fp16x3q"): as 3 with only the attention branch's GEMMs (qkv, proj) in the form of 4, the MLP's
 *                           three-part: gate logits ~1e-5 (0 differing decisions over five seeds at B=16 and at B=128).  A complete_model
 *                           (teacher) pass takes the form of 4 for its MLP as well and the hi * hi product alone in its attention
 *                           forward -- its gate output is discarded, so no token-keep decision depends on it, only its logits
 *                           (<= 1e-4 from the reference at B=16, 2.7e-4 from the fp32 mode at B=128, instead of 7e-6).
 *                           Values >= 1 allocate a second arena (the [hi | lo] weight images, split-operand scratch, the 16-bit
 *                           tensors of 3..5) the first time they are set; plain fp32 contexts do not carry it. */
#define DYT_OPT_F32_SPLIT16 8
/*   DYT_OPT_ATTN_V2             bit mask, default 3 (environment DYT_ATTN_V2 overrides the default).  16-bit modes: bit 0 = the round-5
 *                           attention FORWARD kernel (csrc/attention_v2.hip: K / V / Q as swizzled LDS images filled by LDS-DMA from a loader
 *                           wave, V^T fragments by ds_read_b64_tr_b16 from the row-major image, online softmax per 32-key tile), bit 1 = the
 *                           round-5 BACKWARD kernel (four DMA images, every transposed operand a transposed read of the same image, row
 *                           statistics by the loader wave, results stored as whole rows from inside the next tile loop).  0: the round 1-4
 *                           kernels of csrc/attention_16.hip (DYT_OPT_ATTN_BWD_FUSED then selects among those).  Same arithmetic contract;
 *                           different summation order, so results agree to rounding, not bit for bit.  PROCESS-wide. */
#define DYT_OPT_ATTN_V2 9
/*   DYT_OPT_GEMM_SPLITK         default 1 (environment DYT_SPLITK overrides the default).  16-bit kernels: the K = 3072 GEMMs of the cls-only
 *                           last block (DYT_OPT_CLS_TAIL; M = batch rows: fc2 forward with the adapter pair, fc1 dgrad) run split over
 *                           256-wide k slices on ~300 workgroups + one reduce launch that applies the epilogue, instead of 6 tiles of
 *                           128x128 (csrc/gemm_skinny.h).  Slices are summed in a fixed order: deterministic; agrees with the tile kernels to
 *                           fp32 rounding of the k sums, not bit for bit.  PROCESS-wide. */
#define DYT_OPT_GEMM_SPLITK 10
/*   DYT_OPT_LEARNABLE_SCALE     default 0.  1: tuning_config.ffn_adapter_scalar == "learnable_scalar" (models/dynamic_adapter.py:101-102, 138: the
 *                           adapter output is multiplied by a trainable nn.Parameter(torch.ones(1)) per block instead of a constant).  The
 *                           parameter is DYT_P_AD_SCALE of the flat buffer (one word per block, behind the gate bias; set it like any
 *                           trainable tensor), dyt_config.adapter_scale is ignored.  The per-step adapter copies carry the scale
 *                           (W' = s W_up, b' = s b_up), so every kernel runs as with scale 1; the backward leaves dL/dW', dL/db' in a
 *                           scratch buffer and one small kernel applies the chain rule: dW_up = s dW', db_up = s db',
 *                           ds = <dW', W_up> + <db', b_up>.  The scale words belong to the caller's flat buffer and are whatever it holds:
 *                           write the reference's initial value 1.0 (models/dynamic_adapter.py:102) before the first pass -- a zeroed
 *                           buffer means s = 0, i.e. adapters off and no up-projection gradient.  Must be set before the first forward
 *                           pass of the context; changing it afterwards returns DYT_ERR_STATE. */
#define DYT_OPT_LEARNABLE_SCALE 11
int dyt_ctx_set_option(dyt_ctx* ctx, int option, int value);
/* the process-wide options (DYT_OPT_ATTN_BWD_FUSED, DYT_OPT_ATTN_V2, DYT_OPT_GEMM_SPLITK) without a context: unit entries such as dyt_attention() see them too */
int dyt_set_global_option(int option, int value);

/* Stochastic depth -- timm's DropPath as the reference's blocks use it (models/vision_transformer_IN21K.py:121,131 construct it with
 * dpr[l] = linspace(0, drop_path_rate, depth)[l], :285; :148 x + drop_path1(attn(norm1 x)), :159 drop_path2(mlp(norm2 x));
 * main_image.py:118,213 --drop_path).  In every TRAINING forward pass (DYT_F_TRAINING) block l > 0 multiplies the attention branch and
 * the MLP branch of image b by two independent factors: 1 / keep_l with probability keep_l = 1 - rate * l / (depth - 1), else 0
 * (scale_by_keep); evaluation passes and rate 0 (the default, what every reference script runs) do nothing.  The factors ride in the
 * residual epilogues of the proj and fc2 GEMMs; the backward pass scales the two branch gradients by the same factors.  Each pass
 * (student, complete_model) draws its own, from the call's Philox seed (sub-stream 0x10000 + 2 l + branch of the slot).
 * With a rate > 0 the 16-bit modes run the adapter's up-projection as its own launch again (DYT_OPT_FC2_CAT has no scaled form). */
int dyt_set_drop_path(dyt_ctx* ctx, float rate);
/* Tests / reproducibility across frameworks: the factors of the next training passes of `slot` are read from `scales` (device,
 * [2][depth][batch of the call]: [0] attention branch, [1] MLP branch; row 0 = block 0 is ignored, it is never dropped) instead of being
 * drawn; the pointer is kept, not copied; null restores the library's own draws. */
int dyt_set_drop_path_scales(dyt_ctx* ctx, int slot, const float* scales);

/* Byte images (DYT_F_IMAGES_U8).  Added without an ABI version change (the version stays 5): a caller discovers the two entries by
 * their symbols, like dyt_adamw_segments.
 * dyt_set_input_norm: the per-channel mean / std of the passes enqueued from now on (the reference's Normalize(mean, std); its
 * --inception switch is 0.5 / 0.5).  Until it is called a context holds the ImageNet statistics (0.485, 0.456, 0.406) /
 * (0.229, 0.224, 0.225).  `mean` and `std` are HOST arrays read during the call; the context keeps host values that travel in the
 * kernels' arguments, so nothing is launched and a step in flight is not disturbed.  A captured step keeps the values it was
 * captured with.  DYT_ERR_ARG: a non-finite mean, a std component that is not finite and > 0. */
int dyt_set_input_norm(dyt_ctx* ctx, const float mean[3], const float std[3]);
/* The same three operations to a plain fp32 image batch, without a context: src uint8 [batch,3,224,224] (nhwc != 0: [batch,224,224,3]),
 * dst fp32 [batch,3,224,224], both device pointers, 16-byte aligned; mean / std host arrays.  For whatever has to see float images
 * before the library does (a mixup_fn), and the reference point of the byte path: dyt_forward on bytes equals dyt_forward on this
 * image bit for bit.  One launch on `stream`, no synchronisation.  DYT_ERR_ARG as above, for a misaligned pointer and for batch < 1. */
int dyt_normalize_u8(const uint8_t* src, float* dst, int batch, int nhwc, const float mean[3], const float std[3], void* stream);

/* Copy one FROZEN parameter (fp32, reference state_dict layout) into the context; the library
 * keeps its own copies in the layouts/dtypes its kernels want (incl. transposes for dgrad).
 * Replaces load_state_dict(...) for the frozen keys -- main_image.py:245. */
int dyt_set_frozen(dyt_ctx* ctx, int param, int layer, const float* src, void* stream);

/* The 74 trainable tensors live in ONE flat fp32 buffer owned by the caller (so one AdamW
 * launch and one all-reduce cover them).  Offsets in elements. -- main_image.py:250-256,285 */
int dyt_trainable_numel(const dyt_ctx* ctx, int64_t* numel);
int dyt_trainable_offset(const dyt_ctx* ctx, int param, int layer, int64_t* offset, int64_t* numel);

/* VisionTransformer.forward(x, complete_model) -- models/vision_transformer_IN21K.py:343-385,
 * Block.forward :144-165, TokenSelect.forward / _gumbel_sigmoid dynamic_adapter.py:25-77,
 * Adapter.forward :120-140.
 *   images        [B,3,224,224] fp32, already normalised; with DYT_F_IMAGES_U8 a uint8 batch (see the flag)
 *   trainable     flat trainable buffer (dyt_trainable_offset layout)
 *   g1, g2        [depth,B,196] fp32 Gumbel draws to inject (parity tests), or NULL: logistic noise
 *                 from the on-device Philox stream (seed, slot) -- same distribution as g1-g2
 *   keep_mask     [depth,B*197,r] uint8 adapter-dropout keep mask to inject, or NULL: Philox
 *   logits        [B,C] out
 *   token_select  [B,depth,196] out fp32 {0,1} (may be NULL)
 *   token_logits  [B,depth,196] out fp32       (may be NULL)
 */
int dyt_forward(dyt_ctx* ctx, int slot, const float* images, int batch, int flags,
                const float* trainable, const float* g1, const float* g2,
                const uint8_t* keep_mask, uint64_t seed,
                float* logits, float* token_select, float* token_logits, void* stream);

/* Backward of one saved pass: what loss.backward() does through the module
 * (engine_finetune.py:74-76 via misc.py:258-259).  Gradients of the trainable tensors are
 * ACCUMULATED into grad_flat (same layout as `trainable`).
 *   dlogits        [B,C]
 *   dtoken_select  [B,depth,196] or NULL  (gradient w.r.t. the straight-through mask)
 *   dtok_uniform   device float[3] or NULL: {uniform, extra for dropped, extra for kept} gradient per
 *                  mask element, as produced by dyt_loss (used when dtoken_select is NULL)
 *   dtoken_logits  [B,depth,196] or NULL
 */
int dyt_backward(dyt_ctx* ctx, int slot, const float* dlogits, const float* dtoken_select,
                 const float* dtok_uniform, const float* dtoken_logits, float* grad_flat, void* stream);

/* Token-level training: the backbone under a head and a loss of the caller's own (a dense-prediction head over the reference backbone's
 * out_indices, dense_tasks/Segmentation/backbone/segmentation_vision_transformer_IN21K.py:526-560).  Image model (frames = 1) only.
 *
 * dyt_forward_taps: dyt_forward with DYT_F_TOKENS_OUT and without DYT_F_TOKENS_IN (`tokens` [B,197,768] takes the place of `logits`:
 * the last block's output, no final norm), which also writes taps[i] -- an array of `depth` DEVICE pointers in HOST memory, each NULL or an
 * fp32 [B,197,768] buffer -- := the residual stream behind block i, un-normalised, on `stream`: bit for bit the pass's own snapshot
 * xs[i + 1]; no other output bit of the pass depends on `taps` (NULL: none).  Inference-only contexts serve it too.  With DYT_F_SAVE
 * the slot holds a TOKEN-LEVEL pass: every row of the last block is saved, dyt_backward_tokens is its backward, dyt_backward refuses it
 * (as dyt_backward_tokens refuses a slot saved by dyt_forward without DYT_F_TOKENS_OUT).
 *
 * dyt_backward_tokens: gradients of the adapters, gates, adapter LayerNorms and learnable scales ACCUMULATED into grad_flat exactly as
 * dyt_backward does; the ranges of head.*, fc_norm.* (and the frozen norm.*) are left as they are.
 *   dtokens        [B,197,768] fp32 or NULL: gradient of LN_final(tokens) (contexts with DYT_CREATE_FC_NORM, whose final norm is an
 *                  identity: of the tokens themselves)
 *   dtaps          NULL or an array of `depth` device pointers in host memory, each NULL or the fp32 [B,197,768] gradient of taps[i]
 *   dtoken_select / dtok_uniform / dtoken_logits   as dyt_backward
 * All adds happen in the library: the top of the stream is LNbwd_final(dtokens) + dtaps[depth-1]; dtaps[i], i < depth-1, is added in fp32
 * inside block i+1's LayerNorm-1 backward, in front of every store and rounding of that row.
 * DYT_ERR_ARG / DYT_ERR_STATE with a text, before anything is enqueued: every gradient input NULL, frames > 1, an inference-only context,
 * a slot that does not hold a token-level pass.  Not part of dyt_step_fwd_bwd, so there is no captured-graph form of this route. */
int dyt_forward_taps(dyt_ctx* ctx, int slot, const float* images, int batch, int flags, const float* trainable,
                     const float* gumbel_g1, const float* gumbel_g2, const uint8_t* keep_mask, uint64_t seed,
                     float* tokens, float* const* taps, float* token_select, float* token_logits, void* stream);
int dyt_backward_tokens(dyt_ctx* ctx, int slot, const float* dtokens, const float* const* dtaps, const float* dtoken_select,
                        const float* dtok_uniform, const float* dtoken_logits, float* grad_flat, void* stream);

/* Loss of the fine-tune step and its gradient w.r.t. both logits -- engine_finetune.py:52-63 and
 * AdaLoss.forward models/losses.py:48-84:
 *   loss = CE(s,y) + ratio*((mean(mask)-target)^2 + w_min*sum(clamp(t_min-mask,0))) + CE(t,y)
 *          + KL(log_softmax s || log_softmax t.detach(), batchmean)
 * The mask statistics are taken from the token counts saved by the student pass in `slot_student`.
 *   out_losses  device float[8]: loss, base_loss, token_loss(scaled), teacher_loss, distillation_loss,
 *               mean keep ratio, kept tokens, 0
 *   dtok        device float[3] (see dyt_backward)
 */
int dyt_loss(dyt_ctx* ctx, int slot_student, const float* logits_s, const float* logits_t,
             const int64_t* targets, int batch, float token_target_ratio, float token_loss_ratio,
             float token_minimal, float token_minimal_weight,
             float* dlogits_s, float* dlogits_t, float* out_losses, float* dtok, void* stream);

/* Mixup / soft labels (reference engine_finetune.py:44-45,60-62: `samples, targets = mixup_fn(samples, targets)` hands class-probability
 * targets [rows, num_classes] to nn.CrossEntropyLoss for the student and the teacher pass alike): the loss evaluations that follow -- dyt_loss,
 * dyt_step_fwd_bwd -- read `targets` (device fp32; the pointer is kept, not copied; rows = the logits' rows) instead of their integer labels,
 * which are then ignored: CE = -sum_c t_c log p_c, d logits = p sum_c t_c - t.  NULL restores the integer labels. */
int dyt_set_soft_targets(dyt_ctx* ctx, const float* targets, int rows);

/* On-device Mixup / CutMix (timm's Mixup, mode='batch', restated in csrc/mix.h), fused into the patch-embedding load.  Added without an ABI
 * version change (the version stays 5) and without a flag: the three entries are discovered by their symbols, and "mix on" is context state
 * like the soft targets.
 * The draw lives in DEVICE memory: params_dev points to 16 words, 16-byte aligned, laid out as csrc/mix.h's MixParams --
 *   int32 mode (0 identity, 1 mixup, 2 cutmix); float lam, 1 - lam; int32 yl, yh, xl, xh (cutmix: rows [yl,yh) x columns [xl,xh) come from
 *   the partner); float on, off (target row: off everywhere, on at the label); int32 smooth_on, float keep, add (the criterion's own label
 *   smoothing on top: t * keep + add); 4 reserved words
 * -- and is read by the kernels when they RUN, never copied into their arguments: a captured step replayed after the block was overwritten
 * mixes with the new draw.  Image n of a batch pairs with image count-1-n (video: the same frame of the mirrored clip).
 * dyt_set_mix: while params_dev is set, every pass of this context that takes images (dyt_forward, dyt_step_fwd_bwd; uint8 or fp32) mixes
 * them where the embedding operand is produced -- bit for bit the float path on dyt_mix_images' output -- and dyt_step_fwd_bwd computes its
 * loss against the class-probability rows dyt_mix_targets would write from its integer labels (context-owned buffer of max_batch x
 * num_classes floats, allocated by the first call: make that call outside a stream capture).  The pointer is kept, not copied; NULL turns
 * mix off, and the passes launch exactly the kernels they launched before.  `frames` must be the context's.  Refused with a text, before
 * anything is enqueued: an inference_only context, an odd number of images / clips (by the pass), mix together with dyt_set_soft_targets
 * (DYT_ERR_STATE). */
int dyt_set_mix(dyt_ctx* ctx, const void* params_dev, int frames);
/* The mixed images as a plain fp32 batch, without a context: src fp32 [count,3,224,224] (src_kind 0), uint8 [count,3,224,224] (1) or uint8
 * [count,224,224,3] (2) -> dst fp32 [count,3,224,224]; bytes are normalised with mean / std (host arrays, as dyt_normalize_u8; unused and
 * may be NULL for src_kind 0) before they are mixed.  count = clips * frames, an even number of clips.  One launch on `stream`. */
int dyt_mix_images(const void* src, float* dst, int count, int frames, int src_kind, const float mean[3], const float std[3], const void* params_dev, void* stream);
/* The class-probability rows of a draw: labels int64 [rows] -> out fp32 [rows, num_classes] (16-byte aligned),
 * out[r] = lam t(labels[r]) + (1 - lam) t(labels[rows-1-r]), three fp32 roundings, then the criterion's smoothing if the block asks for it.
 * rows even, 1 <= num_classes <= 65 536.  One launch on `stream`. */
int dyt_mix_targets(const int64_t* labels, float* out, int rows, int num_classes, const void* params_dev, void* stream);

/* On-device Random Erasing (the "erase a normalised batch" RandomErasing of timm / SlowFast, restated in csrc/erase.h), fused into the
 * patch-embedding load.  Added like the mix entries: no ABI version change, no flag, discovered by symbol; "erase on" is context state.
 * The draw lives in DEVICE memory: table_dev points to 32-bit words, 16-byte aligned --
 *   16 header words: mode (0 off, 1 const = 0.0f, 2 rand = one N(0,1) colour per image, box and channel, 3 pixel = one N(0,1) value per
 *   pixel and channel), frames, cube (!= 0: one row per clip, shared by its frames), units (rows in use), the 64-bit noise seed as two
 *   words, 10 reserved words;
 *   then one row of 20 words per unit: the box count n (0..4), four boxes (top, h, left, w), 3 unused words
 * -- and is read by the kernels when they RUN: a captured step replayed after the table was overwritten erases with the new draw.  Nothing
 * in the table is used as an index: the row is chosen from the image number, n is clamped, boxes are only compared against.  A later box
 * overwrites an earlier one.  The noise is Philox4x32-10 keyed by (seed, image, channel, row, column) through Box-Muller (csrc/erase.h).
 * dyt_set_erase: while table_dev is set, every TRAINING pass of this context that takes images (dyt_forward with DYT_F_TRAINING,
 * dyt_step_fwd_bwd; uint8 or fp32) erases them where the embedding operand is produced, BEFORE the mix of dyt_set_mix (the partner's
 * erased pixels are what is blended in) -- bit for bit the float path on dyt_erase_images' output.  Forwards without DYT_F_TRAINING never
 * erase.  units_capacity = the rows the allocation behind table_dev holds; the pointer is kept, not copied; NULL turns erasing off, and the
 * passes launch exactly the kernels they launched before.  Refused with a text, before anything is enqueued: an inference_only context, a
 * misaligned pointer, `frames` other than the context's, units_capacity < 1, and (by the pass) a batch of more images than units_capacity. */
int dyt_set_erase(dyt_ctx* ctx, const void* table_dev, int units_capacity, int frames);
/* The erased images as a plain fp32 batch, without a context: src as in dyt_mix_images -> dst fp32 [count,3,224,224].  The table must hold
 * a row for every image (count rows at least).  mix_params_dev: NULL, or a MixParams block -- the erased batch is then mixed with its
 * erased mirror (count an even number of clips).  One launch on `stream`. */
int dyt_erase_images(const void* src, float* dst, int count, int frames, int src_kind, const float mean[3], const float std[3], const void* table_dev, const void* mix_params_dev, void* stream);

/* Device RandomResizedCrop + horizontal flip / Resize + CenterCrop from byte sources (csrc/resample.h, csrc/resample.hip): Pillow's bicubic
 * Image.resize for 8-bit images restated bit for bit -- fp64 coefficients quantised to 22 bits, an int32 horizontal pass that rounds to
 * uint8, an int32 vertical pass on those bytes -- applied to a crop box that acts as the image (crop, then resize).  Three context-free
 * entries, added without an ABI version change (the version stays 5) and discovered by their symbols; the same bits from both libraries.
 * src uint8 [batch, src_h, src_w, 3] (channels-last, padded to one shape) -> dst uint8 [batch, 224, 224, 3], the layout
 * DYT_F_IMAGES_U8 | DYT_F_IMAGES_NHWC reads.  The draw lives in DEVICE memory: table_dev points to 32-bit words, 16-byte aligned --
 *   16 header words: filter (3 = bicubic; any other value: every image is written as zeros), units (rows in use), 14 reserved words;
 *   then one row of 12 words per image: src_h, src_w (the image's valid extent inside the padded shape), top, left, box_h, box_w (the crop
 *   box), full_h, full_w (the size the box is resized to), off_y, off_x (the 224 x 224 window inside it), flags (bit 0: mirror the output
 *   columns), one unused word
 * -- and is read by the kernels when they RUN: a captured graph replayed after the table was overwritten resamples with the new draw.
 * A row is valid when the box lies inside the valid extent, the extent inside [src_h, src_w], 1 <= box, 224 <= full, the window inside
 * full, and box <= 2.5 full per axis (at most 11 taps).  Nothing of a row is used as an index before that check (64-bit comparisons); an
 * image whose row fails it, or that has no row (image number >= units), is written as ZEROS.  capacity = the rows the allocation behind
 * table_dev holds.  scratch_dev: dyt_resample_scratch_bytes(batch) bytes at least, 16-byte aligned (the coefficient tables: 23 296 bytes
 * per image).  Two launches on `stream`.  Refused with a text, before anything is enqueued: null or misaligned pointers, batch < 1,
 * batch > capacity, a scratch buffer that is too small, a source side < 1 or above 4096. */
int dyt_resample_u8(const uint8_t* src, int batch, int src_h, int src_w, uint8_t* dst, const void* table_dev, int capacity, void* scratch_dev, int64_t scratch_bytes, void* stream);
int64_t dyt_resample_scratch_bytes(int batch);
/* Debug / test entry: the coefficient tables of table row `row` as the kernels compute them -> out_dev int32 [2][13][224] (16-byte aligned):
 * axis 0 = output rows, 1 = output columns; per axis the first tap (relative to the box), the tap count and 11 coefficients of each of
 * the 224 window positions.  An invalid row gives zeros.  One launch on `stream`. */
int dyt_resample_coeffs(const void* table_dev, int capacity, int row, int src_h, int src_w, int32_t* out_dev, void* stream);

/* The same crop / resize at ANY downscale (csrc/resample_wide.h, csrc/resample_wide.hip): the table, the filter, the rounding and the
 * layouts of dyt_resample_u8, without its bound of box <= 2.5 full.  A row is valid under every other condition of dyt_resample_u8; a box
 * side is at most 4096 and full at least 224, so a window position takes at most 75 taps.  Three context-free entries, added without an
 * ABI version change (the version stays 5) and discovered by their symbols; the same bits from both libraries, and for every row
 * dyt_resample_u8 takes, its bits.
 * dyt_resample_wide_u8: scratch_dev holds dyt_resample_wide_scratch_bytes(batch, src_h) bytes at least, 16-byte aligned: the coefficient
 * tables (137 984 bytes per image), then the horizontally resampled source rows, uint8 [batch][src_h][672].  Three launches on `stream`
 * whose grids depend on (batch, src_h, src_w) alone: coefficients, a horizontal pass over the source rows the window's vertical taps need
 * (each filtered once), a vertical pass over the intermediate.  An invalid row is written as ZEROS.  The padding of the source never
 * reaches an output.  Refused with a text, before anything is enqueued: what dyt_resample_u8 refuses. */
int dyt_resample_wide_u8(const uint8_t* src, int batch, int src_h, int src_w, uint8_t* dst, const void* table_dev, int capacity, void* scratch_dev, int64_t scratch_bytes, void* stream);
int64_t dyt_resample_wide_scratch_bytes(int batch, int src_h);
/* Debug / test entry: dyt_resample_coeffs of the wide route -> out_dev int32 [2][77][224] (16-byte aligned): per axis the first tap, the tap
 * count and 75 coefficients of each of the 224 window positions.  An invalid row gives zeros.  One launch on `stream`. */
int dyt_resample_wide_coeffs(const void* table_dev, int capacity, int row, int src_h, int src_w, int32_t* out_dev, void* stream);

/* Device clip pipeline from byte clips (csrc/resample_clip.h, csrc/resample_clip.hip): short-side scale jitter + random crop, random resized
 * crop, uniform one- / three-view crops and the mirror of the video loaders, as ONE two-tap resample of normalised frames --
 * torch.nn.functional.interpolate(x, size, mode='bilinear', align_corners=False) restated bit for bit: per axis scale = (float)box / (float)full,
 * real = max(fmaf(scale, d + 0.5f, -0.5f), 0), taps (int)real and the next one clamped to the box, weights l1 = clamp(real - i0, 0, 1),
 * l0 = 1 - l1; per value fmaf(l0, v0, l1 * v1), columns first, then rows; v = ((float)byte / 255.0f - mean[c]) / std[c].  No antialiasing,
 * nothing rounded to bytes.  Two context-free entries, added without an ABI version change (the version stays 5) and discovered by their
 * symbols; the same bits from both libraries.
 * dyt_resample_clip_f32: src uint8 [batch, frames, src_h, src_w, 3] (16-byte aligned; clips padded to one shape) -> dst fp32
 * [units, frames, 3, 224, 224] (16-byte aligned).  table_dev is the table of dyt_resample_u8 with header word 0 (filter) = 2 ("float
 * bilinear"; with any other value every unit is written as zeros) and the rows' 12th word = src, the index of the source clip the row
 * reads: output unit r is written from table row r, one row serves all frames of its clip, and several rows (spatial views) may share a
 * source clip.  A row is valid when the extent lies inside [src_h, src_w], the box inside the extent, 1 <= box, 224 <= full <= 2^23 (so
 * that d + 0.5f is exact), the window inside full and 0 <= src < batch; there is no 2.5x bound.  Nothing of a row is used as an index
 * before that check (64-bit comparisons); a unit whose row fails it, or that has no row (unit >= the header's units), is written as
 * ZEROS.  The table is read when the kernel RUNS.  One launch on `stream`.  Refused with a text, before anything is enqueued: null or
 * misaligned pointers, batch / frames / units < 1, frames or units above 65535, units > capacity, a source side < 1 or above 4096, a
 * non-finite mean, a non-finite or zero std. */
int dyt_resample_clip_f32(const uint8_t* src, int batch, int frames, int src_h, int src_w, float* dst, int units, const void* table_dev, int capacity, const float mean[3], const float std[3], void* stream);
/* Debug / test entry: the taps and weights of table row `row` as the kernel computes them -> out_dev int32 [2][4][224] (16-byte aligned):
 * axis 0 = output rows, 1 = output columns; per axis i0, i1 (relative to the box) and the bit patterns of l0, l1 of each of the 224
 * window positions.  An invalid row gives zeros (the row's src word is not checked here: no source is read).  One launch on `stream`. */
int dyt_resample_clip_coeffs(const void* table_dev, int capacity, int row, int src_h, int src_w, int32_t* out_dev, void* stream);

/* RandAugment on the device for byte clips and images (csrc/randaug.h, csrc/randaug.hip): the reference's video_datasets/rand_augment.py
 * -- Pillow's 8-bit arithmetic behind it -- restated byte for byte as twelve operations: Identity, Invert, Solarize, SolarizeAdd, Posterize,
 * AutoContrast, Equalize (3 x 256 tables), Brightness, Color, Contrast (Image.blend against a degenerate value, fp32), Sharpness (blend
 * against ImageFilter.SMOOTH) and Affine (Image.transform with a fill colour, bilinear or bicubic, fp64).  Two context-free entries, added
 * without an ABI version change (the version stays 5) and discovered by their symbols; the same bytes from both libraries.
 * dyt_randaug_u8: src uint8 [units, frames, src_h, src_w, 3] (clips padded to one shape; an image batch is frames = 1) -> dst of the same
 * shape; work is a third buffer of that shape and stats int32 [units * frames * 1024] (all 16-byte aligned, all distinct).  table_dev:
 * 16 header words (magic 0x31475541, units, layers) and 20-word rows [layers][capacity], one per (layer, unit): op, the unit's valid h and
 * w, an integer argument, filter (2 bilinear, 3 bicubic), fill (r | g << 8 | b << 16), an fp32 factor, the buffers the row reads and writes
 * (source | destination << 8; 0 src, 1 dst, 2 work) and six fp64 coefficients.  All frames of a unit share its rows.  Layers run one after
 * another on `stream`; layer 0 reads src, pixel-local operations may work in place, Sharpness and Affine write the buffer they do not read,
 * the last layer writes dst.  Bytes outside a unit's valid h x w arrive in dst unchanged.  launch_mask (HOST memory, one word per layer, or
 * null = everything): bits 0..3 = some unit of the layer runs a table / blend / Sharpness / Affine operation, bit 4 = some unit needs the
 * frame histograms (AutoContrast, Equalize, Contrast); only what is named is launched.  Nothing of a row is used before it is checked; a unit
 * with an invalid row in any layer, a buffer sequence that does not link, or no row is written as ZEROS.  The table is read when the kernels
 * RUN.  Refused with a text, before anything is enqueued: null or misaligned pointers, src == dst (or work equal to either), units / frames /
 * layers < 1, layers > 8, units * frames > 65535, units > capacity, a side < 1 or above 4096. */
int dyt_randaug_u8(const uint8_t* src, int units, int frames, int src_h, int src_w, uint8_t* dst, uint8_t* work, int32_t* stats, const void* table_dev, int capacity, int layers, const uint32_t* launch_mask, void* stream);
/* Debug / test entry: the 3 x 256 table (table operations; the identity otherwise) and the Contrast constant that (unit, frame, layer)
 * uses when `src` is that layer's input -> out_dev int32 [769] (16-byte aligned).  An invalid unit gives zeros.  Overwrites stats. */
int dyt_randaug_table(const uint8_t* src, int units, int frames, int src_h, int src_w, int32_t* stats, const void* table_dev, int capacity, int layers, int unit, int frame, int layer, int32_t* out_dev, void* stream);

/* Streaming evaluation statistics (csrc/eval_stats.h, csrc/eval_stats.hip): a batch of logits, labels and token masks is folded into a
 * fixed-size device-resident state, so that an evaluation loop keeps no per-sample tensor.  Two context-free entries, added without an ABI
 * version change (the version stays 5) and discovered by their symbols; pure fp32 / integer, the same bits from both libraries.
 * The state is ADDITIVE -- every entry accumulates, the caller zeroes it, ranks merge with a SUM all-reduce:
 *   counts     int64 [DYT_EVAL_OFF_KEEP + layers * (tokens + 1)]:
 *                [0, 8)   head: rows counted, rows ignored, rows holding a NaN, mask rows (images) counted, 4 spare words
 *                [8, 24)  rank histogram: bin r < 15 = exactly r classes rank ahead of the label, bin 15 = 15 or more
 *                [24, ..) keep histogram [layers][tokens + 1]: (image, layer) pairs by their number of non-zero mask entries
 *   per_class  int64 [2 * classes] or NULL: per-class totals, then per-class top-1 hits
 *   loss_sum   double [1]: sum of the row losses
 * Rows: logits fp32 [rows, ld] (ld >= classes elements between rows; any 4-byte aligned base -- 16-byte loads are used for the part of each row
 * that allows them), labels int64 [rows].  A label outside [0, classes) makes the row IGNORED: counted as such, excluded from everything
 * else, row_rank -1, row_loss 0.  A row holding a NaN is counted (rows, NaN word, last rank bin, its class total), is no hit at any k
 * (row_rank = classes) and stays out of loss_sum (row_loss 0).  Otherwise rank = #{j : x_j > x_t} + #{j < t : x_j == x_t} and
 * row_loss = -((x_t - max) - log(sum_j exp(x_j - max))).  row_rank int32 [rows] and row_loss fp32 [rows] are written for every row.
 * Two launches on `stream`: the row kernel (each logit read once), then ONE workgroup that folds the row results (loss in double in a
 * fixed order, integer adds elsewhere): the state is bit-reproducible run to run.
 * Masks: token_select fp32 [images, layers, tokens]; one launch.
 * DYT_ERR_ARG with a text, before anything is enqueued: a null pointer (per_class excepted), rows / images outside 1 ... 2^20, classes outside
 * 1 ... 65 536, ld < classes, layers outside 1 ... 64, tokens outside 1 ... 1024, counts / labels / loss_sum / per_class not 8-byte aligned. */
#define DYT_EVAL_HEAD_WORDS 8
#define DYT_EVAL_ROWS 0
#define DYT_EVAL_IGNORED 1
#define DYT_EVAL_NAN_ROWS 2
#define DYT_EVAL_MASK_ROWS 3
#define DYT_EVAL_RANK_BINS 16
#define DYT_EVAL_OFF_RANK 8
#define DYT_EVAL_OFF_KEEP 24
int dyt_eval_rows(const float* logits, int64_t ld, const int64_t* labels, int rows, int classes, int64_t* counts, int64_t* per_class, double* loss_sum, int32_t* row_rank, float* row_loss, void* stream);
int dyt_eval_keep(const float* token_select, int images, int layers, int tokens, int64_t* counts, void* stream);

/* torch.optim.AdamW over the flat trainable buffer -- main_image.py:285; the gradient is first
 * multiplied by grad_scale (1/world_size after a SUM all-reduce).  `step` is 1-based. */
int dyt_adamw(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t numel,
              int step, float lr, float beta1, float beta2, float eps, float weight_decay,
              float grad_scale, void* stream);

/* The same update guarded like the reference's NativeScaler / GradScaler.step (misc.py:256-272; the reference trains under fp16 autocast):
 * when grad holds an inf or NaN -- a 16-bit operand overflowed somewhere in the step -- parameters and moments are left untouched and
 * the skip is counted, without a host round trip.  state = device int32[4], zero-initialised and owned by the caller's optimizer:
 * {updates applied, updates skipped, non-finite flag of this call, reserved}; the bias corrections use state[0] + 1 as the step. */
int dyt_adamw_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t numel, int32_t* state,
                      float lr, float beta1, float beta2, float eps, float weight_decay, float grad_scale, void* stream);

/* The same update for torch.optim.AdamW with several param_groups (the reference's util/lr_decay.py recipe: no weight decay on 1-D tensors,
 * layer-wise lr): ONE launch over the flat buffer, lr and weight_decay taken per segment.  Segment k covers elements
 * [segments[k-1].end, segments[k].end), the first starts at 0.  `segments` is a HOST array that is read during the call and never
 * afterwards (the table travels in the kernel's arguments), so the caller may overwrite it as soon as the call returns; no host sync.
 *   state != NULL   the guarded semantics above over the WHOLE buffer (an inf / NaN anywhere in grad leaves every segment untouched and
 *                   is counted in state[1]; the bias corrections use state[0] + 1); `step` is ignored
 *   state == NULL   the unguarded semantics with the 1-based `step`
 * Every element sees the arithmetic of the one-group entries bit for bit.  DYT_ERR_ARG (with an error text, before anything is
 * enqueued): num_segments outside 1 ... DYT_ADAMW_MAX_SEGMENTS, ends that do not increase strictly, a last end other than numel.
 * Added without an ABI version change (the version stays 5): a caller discovers this entry by its symbol (dlsym / hasattr). */
#define DYT_ADAMW_MAX_SEGMENTS 128
typedef struct { int64_t end; float lr; float weight_decay; } dyt_adamw_segment;   /* elements [previous end, end) */
int dyt_adamw_segments(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t numel,
                       int32_t* state, int step, const dyt_adamw_segment* segments, int num_segments,
                       float beta1, float beta2, float eps, float grad_scale, void* stream);

/* Model EMA (timm's ModelEmaV2) over a flat fp32 buffer, in place and context-free:
 *   ema[i] = fl( fl(decay * ema[i]) + fl(one_minus_decay * param[i]) )
 * -- `ema_v.copy_(decay * ema_v + (1. - decay) * model_v)` as torch evaluates it on fp32 tensors: three fp32 roundings, no fused
 * multiply-add, denormals kept.  The caller forms 1. - decay in double and rounds both scalars to float once.  One launch on `stream`,
 * no atomics, no host sync; 16-byte accesses where both pointers allow them, scalar accesses for unaligned slices and the tail, the
 * same bits either way.  numel == 0 is a successful no-op.  DYT_ERR_ARG (with an error text, before anything is enqueued): a null
 * pointer with numel > 0, numel < 0, a pointer that is not 4-byte aligned, decay or one_minus_decay non-finite or outside [0, 1].
 * The AdamW entries above are not involved: the update is a launch of its own behind them.
 * Added without an ABI version change (the version stays 5): a caller discovers this entry by its symbol, like dyt_adamw_segments. */
int dyt_ema_update(float* ema, const float* param, int64_t numel, float decay, float one_minus_decay, void* stream);

/* One whole fine-tune step body (engine_finetune.py:47-79 without the host syncs): student +
 * teacher forward, loss, one backward over both passes into grad_flat (zeroed first).  The caller
 * all-reduces grad_flat (DDP, main_image.py:280-282) and then calls dyt_adamw. */
int dyt_step_fwd_bwd(dyt_ctx* ctx, const float* images, const int64_t* targets, int batch,
                     int flags, const float* trainable,
                     const float* g1, const float* g2, const uint8_t* keep_mask, uint64_t seed,
                     float token_target_ratio, float token_loss_ratio,
                     float token_minimal, float token_minimal_weight,
                     float* grad_flat, float* out_losses, float* logits_s, float* logits_t,
                     float* token_select, void* stream);

/* Set the device-side seed word used by DYT_F_DEVICE_SEED passes (one tiny launch on `stream`). */
int dyt_seed(dyt_ctx* ctx, uint64_t seed, void* stream);

/* Chunked all-reduce (what DDP's bucketed hooks do inside loss.backward(), misc.py:258-259 / main_image.py:280-282):
 * the backward pass runs block 11 -> 0, so part 0 of the flat gradient = the head and blocks >= depth/2 (a contiguous
 * tail of the buffer) is final while the frozen-backbone backward of the lower blocks is still running.
 *   dyt_grad_part(ctx, part, &offset, &numel)   part 0: early (upper) range, part 1: the rest
 *   dyt_stream_wait_grads(ctx, 0, comm_stream)  makes comm_stream wait (device-side) until part 0 of the last
 *                                               dyt_step_fwd_bwd is complete, so its all-reduce overlaps the rest of
 *                                               the backward; the step's own stream owns the whole buffer once
 *                                               dyt_step_fwd_bwd's work is done, as before. */
int dyt_grad_part(const dyt_ctx* ctx, int part, int64_t* offset, int64_t* numel);
int dyt_stream_wait_grads(dyt_ctx* ctx, int part, void* stream);

/* The gradient all-reduce itself, on RCCL (replaces DistributedDataParallel's bucket all-reduce, main_image.py:280-282; the
 * collective call sites of SURVEY.md section 2.3): SUM of grad_flat over the ranks of `rccl_comm` (an ncclComm_t the binder created
 * with ncclCommInitRank; one process per GPU).  With a `comm_stream` different from `stream`, part 0 is reduced on comm_stream as soon
 * as the last dyt_step_fwd_bwd has it final (overlapping the backward of the lower blocks), part 1 on `stream`, and `stream` owns the
 * whole buffer afterwards; comm_stream = NULL: one all-reduce on `stream`.  The 1/world factor is the caller's (dyt_adamw's
 * grad_scale).  RCCL is bound at load time from the host process (no link-time dependency): DYT_ERR_STATE when it is absent. */
int dyt_allreduce_grads(dyt_ctx* ctx, void* rccl_comm, float* grad_flat, void* comm_stream, void* stream);

/* torch.nn.utils.clip_grad_norm_ over the flat gradient (engine_finetune.py:74 -> misc.py:262-266, --clip_grad):
 * norm_out[0] (device, may be NULL) = || pre_scale * grad ||_2 ; grad *= min(1, max_norm / (norm + 1e-6)).
 * pre_scale is the factor AdamW will apply (1/world after a SUM all-reduce, 1/accum_iter). */
int dyt_clip_grad_norm(dyt_ctx* ctx, float* grad, int64_t numel, float max_norm, float pre_scale, float* norm_out, void* stream);

/* Test hook: the token dispatcher's index arrays of a pass still held in `slot` (compacted student pass), block `layer`:
 *   row_src[K] compact row -> token row (ascending = nonzero() of model_speed_test.py:300), dst_of[B*197] token row ->
 *   compact row or -1, counts[B] kept tokens per image incl. cls, total[1] = K.  Device-to-device copies on `stream`;
 *   any pointer may be NULL. */
int dyt_debug_dispatch(dyt_ctx* ctx, int slot, int layer, int32_t* row_src, int32_t* dst_of, int32_t* counts, int32_t* total,
                       void* stream);
/* Test accessor: the adapter bottleneck relu(down(u)) (x dropout scale) a saved pass holds for `layer`, as fp32 [rows, 64] (64 = the
 * padded rank); *rows_out = B*197, or B when the last block ran in the cls-only tail form.  out: device memory for B*197*64 floats. */
int dyt_debug_dact(dyt_ctx* ctx, int slot, int layer, float* out, int* rows_out, void* stream);
/* tests: the stochastic-depth factors [2][depth][batch] the last pass of `slot` ran with (drawn or injected); DYT_ERR_STATE when it ran without */
int dyt_debug_drop_path(dyt_ctx* ctx, int slot, float* out, void* stream);

/* ---- sub-module entry points: they allocate scratch and synchronise; not for the hot loop ---- */
/* Adapter.forward (models/dynamic_adapter.py:120-140, layernorm option "none"): out[M,768] = [residual +] scale *
 * (dropout_p(relu(x down_w^T + down_b)) up_w^T + up_b).  down_w [r,768], up_w [768,r] (nn.Linear layouts), r <= 64; residual may be
 * NULL (add_residual=False); drop_p > 0: keep_mask [M,r] (uint8) if given, else Philox(seed). */
int dyt_adapter_fwd(const float* x, const float* down_w, const float* down_b, const float* up_w, const float* up_b,
                    const float* residual, float* out, int M, int r, float scale, float drop_p, const uint8_t* keep_mask,
                    uint64_t seed, int precision, void* stream);
/* its backward for dout [M,768] with the same draws: dx [M,768] (may be NULL); the parameter gradients are ACCUMULATED */
int dyt_adapter_bwd(const float* x, const float* down_w, const float* down_b, const float* up_w, const float* dout, float* dx,
                    float* d_down_w, float* d_down_b, float* d_up_w, float* d_up_b, int M, int r, float scale, float drop_p,
                    const uint8_t* keep_mask, uint64_t seed, int precision, void* stream);
/* The wide head (DYT_CREATE_WIDE_HEAD) without a context, exactly the launches the context path runs: logits [B,C] = LN(cls_x) head_w^T
 * + head_b (final LayerNorm norm_w / norm_b, eps 1e-6; cls_x [B,768] the un-normalised cls rows).  With dlogits [B,C] also its
 * backward: dx [B,768] = the gradient w.r.t. cls_x (may be NULL), d_head_w [C,768] / d_head_b [C] ACCUMULATED (each may be NULL).
 * dlogits NULL: forward only, no gradient is touched.  C = 1 ... 65 536. */
int dyt_head_wide(const float* cls_x, const float* norm_w, const float* norm_b, const float* head_w, const float* head_b,
                  float* logits, const float* dlogits, float* dx, float* d_head_w, float* d_head_b, int batch, int C, void* stream);
/* The pooled head (DYT_CREATE_AVG_POOL / DYT_CREATE_FC_NORM, optionally DYT_CREATE_WIDE_HEAD in create_flags) without a context, exactly
 * the launches the context path runs (reference forward_head, models/vision_transformer_IN21K.py:375-380): logits [B,C] =
 * fc_norm(row_b) head_w^T + head_b, row_b = mean of the 196 patch rows of x_tokens [B,197,768] (AVG_POOL | FC_NORM) or its cls row (FC_NORM alone).
 * With dlogits [B,C] also the backward: dx_tokens [B,197,768] is OVERWRITTEN with the gradient w.r.t. x_tokens (AVG_POOL: cls rows 0,
 * patch rows dpooled / 196; FC_NORM alone: the cls rows, zero elsewhere); d_fc_norm_w / d_fc_norm_b [768], d_head_w [C,768], d_head_b [C]
 * are ACCUMULATED (+=) and may each be NULL.  dlogits NULL: forward only.  C = 1 ... 1024, with DYT_CREATE_WIDE_HEAD 1 ... 65 536.
 * Unit-test entry: allocates its scratch and synchronises. */
int dyt_pool_head(const float* x_tokens, const float* fc_norm_w, const float* fc_norm_b, const float* head_w, const float* head_b,
                  float* logits, const float* dlogits, float* dx_tokens, float* d_fc_norm_w, float* d_fc_norm_b,
                  float* d_head_w, float* d_head_b, int batch, int C, uint32_t create_flags, void* stream);
/* the token-gathered MLP of block `layer` (frozen weights of the context; models/model_speed_test.py:297-305): for the tokens with a
 * non-zero mask, x[t] += fc2(gelu(fc1(LN2(u[t])))); u, x fp32 [batch*197,768] (x in place), mask [batch*197]; total_out[1] (device,
 * may be NULL) = number of gathered tokens */
int dyt_mlp_gathered_fwd(dyt_ctx* ctx, int layer, const float* u, const float* mask, float* x, int batch, int32_t* total_out,
                         void* stream);
/* Its backward (dyt_mlp_gathered_bwd): for dy = the gradient w.r.t. x above, du [B*197,768] += the gradient that reaches u
 * through the gathered MLP of block `layer` -- LN2 backward of fc1^T (gelu'(z) * (fc2^T dy)) scattered back to the kept tokens, nothing
 * for the dropped ones (the residual path du += dy is the caller's; frozen weights: no weight gradients).  Autograd of
 * models/model_speed_test.py:297-305.  Unit-test entry: recomputes the forward, allocates scratch and synchronises. */
int dyt_mlp_gathered_bwd(dyt_ctx* ctx, int layer, const float* u, const float* mask, const float* dy, float* du, int batch, void* stream);

/* ---- the backward row kernels alone (csrc/block_bwd.hip, csrc/ln.hip), for tests/test_gpu_row_bwd.py.  Each entry checks its arguments (DYT_ERR_ARG with
 * a text, before anything is enqueued), launches the product's own kernel through the launcher csrc/backward.hip calls, and synchronises.
 * Added without an ABI version change (the version stays 5), discovered by their symbols like dyt_adamw_segments.
 * `precision` is DYT_PREC_FP32 or DYT_PREC_BF16; at 1 every `void*` operand is of the library's 16-bit type (bfloat16 in libdyt_hip.so,
 * IEEE half in libdyt_hip_f16.so), at 0 it is fp32.  gs (> 0) is the factor the 16-bit gradient operands carry (fp16 mode: 2^12, else
 * 1); the launchers of the first three entries ignore it at precision 0.  `stats` is [rows] (mean, rstd) pairs, i.e. 2 * rows floats.
 * Buffer sizes are the caller's business: nothing here can check them. */
/* bwd_prep_kernel (BwdPrepArgs): g_at[t] = AT(gs g[t]); r = dst_of ? dst_of[t] : t; for r >= 0: dH[r] = AT(gs row_mask[t] g[t]) and
 * dmask[t] = <g[t], h[r]>; dmask[t] = 0 where r < 0 or h is NULL.  g [M,768] fp32; h, dst_of, row_mask, g_at, dH, dmask may each be
 * NULL (not all three outputs). */
int dyt_unit_bwd_prep(const float* g, const void* h, const int32_t* dst_of, const float* row_mask, void* g_at, void* dH, float* dmask,
                      int M, float gs, int precision, void* stream);
/* ln_bwd_kernel (launch_ln_bwd): d = LNbwd(dy[row] / gs; x[row], stats[row], w) + (base[row] | base_at[row] / gs | 0), written as
 * dx[row] (fp32), g_at[row] = AT(gs d), out3[row] = d * s3 as the [rows][2*768] hi | lo split operand (precision 0 only; out3_hi_only:
 * the hi half alone), and dmask_next[row] = <d, h_next[r]> with r = dst_of_next ? dst_of_next[row] : row (0 where r < 0 or h_next is
 * NULL).  dx may alias base.  base_at: precision 1 only, not together with base.  At least one of dx / g_at / out3. */
int dyt_unit_ln_bwd(const void* dy, const float* x, const float* stats, const float* w, const float* base, const void* base_at, float* dx,
                    int rows, void* g_at, const void* h_next, const int32_t* dst_of_next, float* dmask_next, float gs, void* out3,
                    float s3, int out3_hi_only, int precision, void* stream);
/* the tapped instantiations of the same kernel (dyt_backward_tokens): d as above + tap[row], tap fp32 [rows][768], not NULL; added in
 * fp32 behind base / base_at and in front of every output */
int dyt_unit_ln_bwd_tap(const void* dy, const float* x, const float* stats, const float* w, const float* base, const void* base_at, float* dx,
                        int rows, void* g_at, const void* h_next, const int32_t* dst_of_next, float* dmask_next, float gs, void* out3,
                        float s3, int out3_hi_only, const float* tap, int precision, void* stream);
/* ln_param_grad_kernel + ln_param_reduce_kernel (launch_ln_param_grad; scratch allocated inside): out[0:768] += sum_t (dy[t] / gs) xhat[t],
 * out[768:1536] += sum_t dy[t] / gs, xhat = (x - mean) rstd from `stats`. */
int dyt_unit_ln_param_grad(const void* dy, const float* x, const float* stats, float* out, int rows, float gs, int precision, void* stream);
/* tok_bwd_kernel (launch_tok_bwd) and, with gate_w set, the deferred reduction of its partials (queue_tok_reduce + flush_reductions:
 * reduce_partials_batch_kernel) into d_gate[769] (+=: 768 weight gradients, then the bias gradient).  The struct mirrors TokBwdArgs of
 * csrc/kernels.h field for field (its `partial` scratch is allocated inside, inv_gs is 1 / gs); every pointer may be NULL unless
 * named below.  Per token t = b * 197 + n, with r = the token's compact row (g_cls: b for n == 0, else none; dst_of ? dst_of[t] : t):
 *   du'  = (g_cls ? (n == 0 ? g_cls[b] : 0) : du_in_at ? du_in_at[t] / gs : du[t]) + dad[t] / gs
 *          + (r >= 0 ? branch_scale[b] LNbwd(dA2[r]; u[t], stats2[t], ln2_w) / gs : 0) + (n >= 1 && gate_w ? dlogit gate_w : 0)
 *   dlogit = (branch_scale[b] (dmask[t] - [maskf[t] != 0] <cat_dact[t], cat_ddz[t]> cat_ddz_scale *cat_ddz_dscale) + ext)
 *            soft[t] (1 - soft[t]) (/ tau when training) + dtoken_logits[b * out_stride + n - 1]
 *   ext  = dtoken_select ? dtoken_select[b * out_stride + n - 1] : dtok ? dtok[0] + (maskf[t] != 0 ? dtok[2] : dtok[1]) : 0
 *   d_gate[0:768] += sum_t dlogit u[t], d_gate[768] += sum_t dlogit            (patch tokens only)
 * du' goes to du (fp32, in place), du_at = AT(gs du') and du3 = du' du3_scale as the split operand -- only when write_du.
 * DYT_ERR_ARG: M not a positive multiple of 197; write_du with du == NULL and du_at == NULL, or without any incoming gradient; du3 at
 * precision 1; du_in_at at precision 0; gs != 1 at precision 0; u NULL with dA2 or gate_w; dA2 (with write_du) without stats2 / ln2_w;
 * gate_w without soft / d_gate, with training and tau <= 0, with dtok or cat_dact but no maskf, with cat_dact xor cat_ddz. */
typedef struct {
    float* du; const void* dA2; const int32_t* dst_of; const float* u; const float* stats2; const float* ln2_w;
    const float* gate_w; const float* soft; const float* maskf; const float* dmask;
    const float* dtoken_select; const float* dtoken_logits; const float* dtok;
    void* du_at; const void* dad; const float* g_cls;
    const void* cat_dact; const void* cat_ddz; const float* cat_ddz_dscale;
    void* du3; const float* branch_scale; const void* du_in_at;
    int32_t out_stride, training, M, write_du, du3_hi_only;
    float tau, gs, cat_scale, cat_ddz_scale, du3_scale;
} dyt_unit_tok_bwd_args;
int dyt_unit_tok_bwd(const dyt_unit_tok_bwd_args* args, float* d_gate, int precision, void* stream);

/* ---- the forward row kernels alone (csrc/dispatch.hip, csrc/ln.hip, csrc/embed.hip), for tests/test_gpu_row_fwd.py: the token dispatcher,
 * the LayerNorm family around it, the folded form's weight side and the embedding prologue.  As above: each entry checks its arguments
 * (DYT_ERR_ARG with a text, before anything is enqueued), calls the launcher csrc/forward.hip or csrc/ctx.hip calls, and synchronises; no
 * arithmetic of its own.  Added without an ABI version change (the version stays 5), discovered by their symbols.  `precision` and the
 * `void*` operands as above; `stats` is (mean, rstd) pairs, 2 floats per row.  Buffer sizes are the caller's business. */
/* gate_logits_kernel + gate_select_kernel (launch_gate).  The struct mirrors GateArgs of csrc/kernels.h field for field.  Per patch token
 * t = b * 197 + n (n >= 1): l = <u[t], w> + b[0]; z = l (eval), (l + g1[b * 196 + n - 1] - g2[...]) / tau (training with g1), or
 * (l + log(x) - log1p(-x)) / tau with x = u01(word 0 of Philox4x32-10(key = seed_dev ? *seed_dev : seed, counter = (t, subseq)))
 * (training without g1); soft[t] = 1 / (1 + exp(-z)); keep = force_first > 0 ? n < force_first : soft[t] > threshold; maskf[t] = keep;
 * out_select[b * out_stride + n - 1] = keep and out_logits[...] = l when given.  cls (n = 0): soft = maskf = 1, kept, no out_* entry.
 * keep_local[b * 197 + 0 .. counts[b])] = the kept n of image b, ascending.
 * DYT_ERR_ARG: NULL u / w / b / soft / maskf / keep_local / counts; batch < 1; g1 without g2 or the reverse; training with tau <= 0;
 * out_select / out_logits with out_stride < 196; force_first outside 0..197. */
typedef struct {
    const float* u; const float* w; const float* b; const float* g1; const float* g2; const uint64_t* seed_dev;
    float* soft; float* maskf; float* out_select; float* out_logits; int32_t* keep_local; int32_t* counts;
    uint64_t seed, subseq;
    int32_t batch, training, out_stride, force_first;
    float tau, threshold;
} dyt_unit_gate_args;
int dyt_unit_gate(const dyt_unit_gate_args* args, void* stream);
/* gather_index_kernel (launch_gather_index): from keep_local / counts / maskf as dyt_unit_gate leaves them, row_src[0:total[0]] = the kept
 * token rows ascending, dst_of[t] = the compact row of token t or -1, total[0] = the kept tokens, total[1] = batch * 197 - total[0]
 * (written with or without drop_src), and, when drop_src is given, drop_src[0:total[1]] = the dropped token rows ascending. */
int dyt_unit_gather_index(const int32_t* keep_local, const int32_t* counts, int32_t* total, const float* maskf, int32_t* row_src,
                          int32_t* dst_of, int batch, int32_t* drop_src, void* stream);
/* ln_gather_kernel (launch_ln_gather): the same index arrays (total[1] only with drop_src) and out[dst] = LN(u[src]; w, b, eps 1e-6) for
 * the kept rows, stats[src] = (mean, rstd).  out3 (precision 0 only; replaces out): the rows as the [rows][2*768] hi | lo split operand,
 * out3_f8: as [hi16 768 | e4m3(hi) 768 bytes | e4m3(lo 2^12) 768 bytes]. */
int dyt_unit_ln_gather(const float* u, const float* w, const float* b, const int32_t* keep_local, const int32_t* counts, int32_t* total,
                       const float* maskf, void* out, float* stats, int32_t* row_src, int32_t* dst_of, int batch, void* out3, int out3_f8,
                       int32_t* drop_src, int precision, void* stream);
/* ln_fwd_kernel (launch_ln_fwd): out[row] = LN(x[row]; w, b, eps 1e-6), stats[row] = (mean, rstd) when stats is given; out3 / out3_f8 as
 * above (precision 0 only, DYT_ERR_ARG at precision 1; out is then not written and may be NULL). */
int dyt_unit_ln_fwd(const float* x, const float* w, const float* b, void* out, float* stats, int rows, void* out3, int out3_f8, int precision,
                    void* stream);
/* adapter_ln_fwd_kernel (launch_adapter_ln_fwd): out[row] = LN(x[row]; w, b, eps 1e-5) (+ resid[row]), of the 16-bit operand type when
 * out_at_precision is 1, else fp32; stats and resid may be NULL. */
int dyt_unit_adapter_ln_fwd(const float* x, const float* w, const float* b, void* out, float* stats, const float* resid, int rows,
                            int out_at_precision, void* stream);
/* ln_cls_kernel (launch_ln_cls): out[b] = LN(u[b * 197]; w, b, eps 1e-6) ([batch, 768]), stats[b * 197] = (mean, rstd) (the other entries
 * of the [batch * 197] array are not written), u_cls[b] = the operand-type copy of u[b * 197] when given. */
int dyt_unit_ln_cls(const float* u, const float* w, const float* b, void* out, float* stats, void* u_cls, int batch, int precision, void* stream);
/* ln_fold_w_kernel (launch_ln_fold_w without the fragment-order twin): Wf[n] = AT(gamma W[n]) ([N, 768], 16-bit), cs[n] = the sum of the
 * ROUNDED Wf[n], bf[n] = bias[n] + <W[n], beta>.  Precision 0 is the launcher's refusal (DYT_ERR_ARG). */
int dyt_unit_ln_fold_w(const float* W, const float* gamma, const float* beta, const float* bias, void* Wf, float* cs, float* bf, int N,
                       int precision, void* stream);
/* image_load_kernel (launch_image_load, fp32 source to the operand; images [batch, 3, 224, 224] fp32 -> patches [batch * 196, 768] with column c * 256 + i * 16 + j) when images
 * and patches are given, and cls_rows_kernel (launch_cls_rows; x0[b * 197] = cls + pos, x0 [batch * 197, 768] fp32) when cls, pos and x0 are. */
int dyt_unit_embed(const float* images, void* patches, const float* cls, const float* pos, float* x0, int batch, int precision, void* stream);
/* pad_convert_kernel: dst [dst_rows, dst_cols] = src [rows, cols] (launch_pad_convert), or its transpose when `transpose`
 * (launch_transpose_convert), rounded to the operand type, zero outside the source. */
int dyt_unit_pad_convert(const float* src, void* dst, int rows, int cols, int dst_rows, int dst_cols, int transpose, int precision, void* stream);

/* ---- the attention kernels alone (csrc/attention.hip and the family units csrc/attention_{16,exact,split,v2}.hip), for tests/test_gpu_unit_attention.py.  The structs mirror
 * AttnFwdArgs / AttnBwdArgs of csrc/kernels.h field for field (bool as int32); unset pointers are NULL.  The entries check the struct
 * pointer, `precision` and batch >= 1, call launch_attn_fwd / launch_attn_bwd, return the launcher's error (every refusal of
 * csrc/attn_route.h and of the launchers arrives as DYT_ERR_ARG with a text, before anything is enqueued) and synchronise: no arithmetic,
 * no kernel, no layout conversion of their own.  The kernel is the one attn_fwd_route() / attn_bwd_route() pick from the fields and the
 * process-wide DYT_OPT_F32_SPLIT16 / DYT_OPT_ATTN_BWD_FUSED / DYT_OPT_ATTN_V2 (dyt_set_global_option).  Added without an ABI version change.
 * q / k / v [batch*12][197][64] of the operand type (fp32 at precision 0), q already times 1/8; the planar form takes the 16-bit hi / lo
 * planes in the same layout.  out / o16 [batch*197][768], out3 [batch*197][SPLIT_A*768] 16-bit words, lse [batch*12][197] fp32 (natural log). */
typedef struct {
    const void* q; const void* k; const void* v;
    const void* q_hi; const void* k_hi; const void* v_hi; const void* q_lo; const void* k_lo; const void* v_lo;
    void* out; void* out3; void* q16; void* k16; void* v16; void* o16; float* lse;
    int32_t planar, out3_f8, lse_optional, split16, parts, batch;
} dyt_unit_attn_fwd_args;
int dyt_unit_attn_fwd(const dyt_unit_attn_fwd_args* args, int precision, void* stream);
/* out [batch*197][out_ld] (out_ld 0 = 768), dout [batch*197][768], delta [batch*12][197] fp32 scratch (= rowsum(dout * out) where the route
 * writes it), dqkv [batch*197][2304] = (dq / 8 | dk | dv), dqkv3 = dqkv * s3 as the [batch*197][3*2304] split operand (precision 0). */
typedef struct {
    const void* q; const void* k; const void* v; const void* out; const void* dout; const float* lse;
    float* delta; void* dqkv; void* dqkv3;
    int32_t out_ld, out_hi_only, split16, grad_parts, q_tiles, batch;
    float s3;
} dyt_unit_attn_bwd_args;
int dyt_unit_attn_bwd(const dyt_unit_attn_bwd_args* args, int precision, void* stream);

/* ---- the weight-gradient and partial-reduction kernels alone (csrc/wgrad.hip), for tests/test_gpu_unit_wgrad.py.  As above: each entry checks
 * its arguments (DYT_ERR_ARG with a text, before anything is enqueued), calls the launcher csrc/backward.hip / csrc/step.hip call, and
 * synchronises; no arithmetic and no kernel of its own.  Added without an ABI version change, discovered by their symbols.
 * dyt_unit_wgrad_args is WgradArgs of csrc/kernels.h field for field (bool as int32); the caller owns every buffer, `partial` (the number of
 * floats dyt_wgrad_scratch_floats(M) returns, one buffer per product) included.  Per product, with X [M,768] and Y [M,64] of the operand type (fp32 at
 * precision 0) and a = alpha_dev ? *alpha_dev : 1:
 *   out_w[c * sc + j * sj] += alpha a sum_m X[m][c] Y[m][j]  (c < 768, j < r; columns j >= r of Y are read and have no effect)
 *   out_xsum[c] += alpha_x a sum_m X[m][c]   (when given)        out_ysum[j] += alpha_y a sum_m Y[m][j], j < r   (when given)
 * half_products (precision 0 only): X x_scale and Y y_scale (powers of two) are rounded to the library's 16-bit type as they are loaded,
 * the products run on the 16-bit matrix cores and alpha / (x_scale y_scale), alpha_x / x_scale, alpha_y / y_scale undo the scales.
 * pair = 1: consecutive products go two by two through one launch_wgrad(P, w, 2, ...) (same M and r, different `partial`), else one by one.
 * defer = 1: every reduction is queued into ONE ReduceQueue together with the n_tok token reductions (queue_tok_reduce:
 * out[i] += sum_p partial[p * 769 + i], i < 769, p < nparts) and flush_reductions runs once at the end (wgrad_reduce_batch_kernel,
 * reduce_partials_batch_kernel); defer = 0: wgrad_reduce_kernel behind each launch, n_tok must be 0.
 * DYT_ERR_ARG, nothing launched: prods NULL; n_prod outside 1..32 (ReduceQueue::MAX_WG); n_tok outside 0..16 (MAX_TOK) or non-zero without
 * defer or with toks NULL; an odd n_prod with pair; a precision outside {0, 1}; per product NULL X / Y / partial / out_w, r outside 1..64,
 * M < 1, half_products at precision 1, x_scale or y_scale not positive; per token reduction NULL partial / out or nparts < 1.  The
 * launcher's own refusals (a pair with different M or r or one `partial`; mixed product forms in a pair; mixed ranks in a queue) come back
 * as its error, before the refused product's kernel is enqueued; products accepted before it have run, their reductions have not. */
typedef struct {
    const void* X; const void* Y; int32_t M, r; float* partial;
    float* out_w; int32_t sc, sj; float alpha;
    float* out_xsum; float alpha_x; float* out_ysum; float alpha_y;
    int32_t half_products; float x_scale, y_scale; const float* alpha_dev;
} dyt_unit_wgrad_args;
typedef struct { const float* partial; int32_t nparts; float* out; } dyt_unit_tok_reduce_args;
int dyt_unit_wgrad(const dyt_unit_wgrad_args* prods, int n_prod, int pair, int defer, const dyt_unit_tok_reduce_args* toks, int n_tok,
                   int precision, void* stream);
/* reduce_partials_kernel (launch_reduce_partials): out[i] += alpha sum_p partial[p * stride + i], i < n, p < nparts.
 * DYT_ERR_ARG: NULL partial / out, nparts < 1, n < 1, stride < 0. */
int dyt_unit_reduce_partials(const float* partial, int nparts, int stride, float* out, int n, float alpha, void* stream);

/* One nn.Linear (c = a w^T + bias; a [M,K], w [N,K], bias [N] or NULL, c [M,N], fp32 device pointers) through the split forms of the
 * fp32 mode: form 3 = every product as three IEEE-half products (hi*hi + hi*lo + lo*hi), form 8 = hi*hi on the f16 matrix cores plus
 * the two correction products on the fp8 (e4m3) matrix cores ("fp16f8").  K % 128 == 0, N % 128 == 0.  Unit-test entry: allocates
 * scratch and synchronises.  Reference op: nn.Linear of models/vision_transformer_IN21K.py:56,73 and timm Mlp (:124-129). */
int dyt_linear_split(const float* a, const float* w, const float* bias, float* c, int M, int N, int K, int form, void* stream);

/* ---- single-kernel entry points (unit tests; also the building blocks of the sub-module API) ---- */
/* nn.LayerNorm(768, eps=1e-6) forward; out fp32 */
int dyt_layernorm(const float* x, const float* w, const float* b, float* out, int rows, void* stream);
/* C[M,N] = A[M,K] @ W[N,K]^T + bias  (nn.Linear); precision selects the kernel family */
int dyt_linear(const float* a, const float* w, const float* bias, float* c, int M, int N, int K,
               int precision, void* stream);
/* scaled_dot_product_attention over [B,12,197,64] from a fused qkv [B*197,2304] (Attention.forward
 * vision_transformer_IN21K.py:54-72): out [B*197,768]; if dout != NULL also returns dqkv */
int dyt_attention(const float* qkv, float* out, const float* dout, float* dqkv, int batch,
                  int precision, void* stream);
/* TokenSelect.forward + index compaction for one block: u [B*197,768], w[768], b[1];
 * outputs mask [B,196], logits [B,196], keep_idx int32 [B*197] (flat kept rows, ascending),
 * counts int32 [B] (kept per image incl. cls), total int32[1] */
int dyt_gate_compact(const float* u, const float* w, const float* b, const float* g1, const float* g2,
                     int batch, int training, float tau, float threshold,
                     float* mask, float* logits, int32_t* keep_idx, int32_t* counts, int32_t* total,
                     void* stream);

/* ---- measurement hooks (bench.py, tools/gemm_bench.py) ---- */
/* C[M,N] (bf16) = A[M,K] (bf16) @ W[N,K]^T (bf16), fp32 accumulate; `variant` selects a kernel build
 * (0 / 10 / 70: the 128x128, 256x256 and pre-shuffled-weight kernels, 30: the product dispatch, 9 / 19 / 79: with phase timers) */
int dyt_gemm_bf16_raw(const void* a, const void* w, void* c, int M, int N, int K, int variant, void* stream);
/* C[M,N] (fp32) = A[M,K] (fp32) @ W[N,K]^T (fp32) on the exact-fp32 MFMA kernel of the parity mode (csrc/gemm_f32_mfma.h);
 * N % 64 == 0, K % 64 == 0; no synchronisation.  variant 0: plain store; 1: the adapter up-projection epilogue (residual read
 * from c + M*N, c = resid + 0.1 * acc); 2: accumulate (c += acc) */
int dyt_gemm_f32_raw(const float* a, const float* w, float* c, int M, int N, int K, int variant, void* stream);
/* the adapter weight-gradient kernel alone: out_w[c*r + j] += sum_m X[m][c] Y[m][j] (X [M,768], Y [M,64], fp32 or bf16 by
 * `precision`), out_xsum[c] += sum_m X[m][c], out_ysum[j] += sum_m Y[m][j]; `partial` = dyt_wgrad_scratch_floats(M) floats */
int64_t dyt_wgrad_scratch_floats(int M);
int dyt_wgrad_raw(const void* X, const void* Y, int M, int r, int precision, float* partial, float* out_w, float* out_xsum,
                  float* out_ysum, void* stream);
/* measurement hooks of tools/probes/determinism_*.py: with DYT_DBG_CKSUM=1 in the environment every backward
 * launch is followed by an integer checksum of its output; read back per pass (slot 0 student, 1 teacher) with its label; one
 * launch's output can be kept whole (DYT_DBG_DUMP="<slot>:<label>") and copied out.  No effect unless the variables are set. */
int dyt_debug_checksums(int slot, uint64_t* out, int max_n, int* n_out);
const char* dyt_debug_checksum_label(int slot, int i);
int64_t dyt_debug_dump_read(void* dst_device, int64_t max_bytes);
/* phase timers of the instrumented GEMM variants: cycles {prologue, main loop, epilogue} summed over
 * workgroups and the workgroup count; synchronises; optionally resets */
int dyt_debug_counters(uint64_t* out4, int reset);
/* bracket every kernel launch with hipEvents on `stream` and accumulate per category */
int dyt_profile_enable(dyt_ctx* ctx, int on);
/* categories: 0 gemm (big MFMA GEMMs), 1 attention, 2 everything else.  Returns accumulated
 * milliseconds, launches and algorithmic FLOPs since the last call, then resets.  Synchronises.
 * category 3: `launches` = bf16 GEMM KERNEL launches since dyt_profile_enable(ctx, 1) (one GEMM of category 0 may be
 * two kernel launches with different tiles); ms / flops are 0; no reset, no synchronisation. */
int dyt_profile_read(dyt_ctx* ctx, int category, double* ms, int64_t* launches, double* flops);

#ifdef __cplusplus
}
#endif
#endif /* DYT_HIP_H */
