// libdyt_hip.so: context, whole-model forward / backward orchestration and the C ABI
// declared in include/dyt_hip.h.  Host side only enqueues kernels on the caller's stream: no
// host<->device synchronisation, no allocation after dyt_ctx_create, kept-token counts stay on
// the device (GEMM grids are sized for the dense case and tiles beyond the device-side row count
// exit immediately), so a step is graph-capturable.
//
// Mirrors (paths relative to the reference root):
//   VisionTransformer.forward_features/forward_head  models/vision_transformer_IN21K.py:343-385
//   Block.forward                                    models/vision_transformer_IN21K.py:144-165
//   compacted MLP                                    models/model_speed_test.py:274-310
//   step body                                        engine_finetune.py:47-79
//
// This header is private to the ctx / forward / backward / step / debug / unit_abi units (not installed): the context, the
// orchestration macros and the functions that cross those units.
#pragma once
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/dyt_hip.h"
#include "kernels.h"

using namespace dyt;

// ------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------
struct LayerW {  // frozen, library-owned
    float *ln1_w, *ln1_b, *qkv_b, *proj_b, *ln2_w, *ln2_b, *fc1_b, *fc2_b;
    void *qkv_w, *qkv_wT, *proj_w, *proj_wT, *fc1_w, *fc1_wT, *fc2_w, *fc2_wT;
    void *qkv_wp = nullptr, *fc1_wp = nullptr, *fc2_wTp = nullptr;   // bf16 mode: MFMA-fragment-order twins (gemm_bpre.h)
    void *proj_wp = nullptr, *proj_wTp = nullptr, *qkv_wTp = nullptr, *fc1_wTp = nullptr;
    // fp32 mode: [N, 2K] 16-bit [hi | lo] images of the eight matrices (DYT_OPT_F32_SPLIT16, launch_split3_w)
    void *qkv_w3 = nullptr, *qkv_wT3 = nullptr, *proj_w3 = nullptr, *proj_wT3 = nullptr, *fc1_w3 = nullptr, *fc1_wT3 = nullptr, *fc2_w3 = nullptr, *fc2_wT3 = nullptr;
    // fp32 mode with a 16-bit backward ("fp16x3h", dyt_ctx::bwd16): the transposed matrices the dgrad GEMMs multiply by, in the 16-bit
    // operand type, plain [in,out] and in MFMA fragment order (what the 16-bit mode keeps as *_wT / *_wTp)
    void *fc1_w3b = nullptr, *fc2_w3b = nullptr, *qkv_w3b = nullptr, *proj_w3b = nullptr;   // second image of a class whose two passes take different forms (student three-part, teacher fp8-correction)
    int* w_exp = nullptr;   // "fp16f8": device words with the exponents of the four forward images (qkv, proj, fc1, fc2), launch_split_w_f8
    void *qkv_wT16 = nullptr, *qkv_wTp16 = nullptr, *proj_wT16 = nullptr, *proj_wTp16 = nullptr, *fc1_wT16 = nullptr, *fc1_wTp16 = nullptr,
         *fc2_wT16 = nullptr, *fc2_wTp16 = nullptr;
    // 16-bit modes, LayerNorm-2 folded into fc1 (dyt_ctx::ln_fold): AT(gamma W1) plain + in fragment order, its column sums, b1 + W1 beta
    void *fc1_wf = nullptr, *fc1_wfp = nullptr; float *fc1_cs = nullptr, *fc1_bf = nullptr, *fc1_w32 = nullptr;   // (w32: the fp32 source, so that gamma W is rounded once)
};
struct LayerS {  // saved activations of one pass
    float2 *st1, *st2;
    void *q, *k, *v, *attn_o, *u_at, *z, *d_act;
    float *lse, *u, *soft, *maskf;
    void* h;
    int *keep_local, *offsets, *total, *row_src, *dst_of;
    float2* ln_part = nullptr;    // dyt_ctx::ln_fold: the proj epilogue's per-row LayerNorm partials of u ([M][LN_PARTS])
    float2* st_a = nullptr;       // dyt_ctx::ad_ln: (mean, rstd) of the adapter's LayerNorm input, [M]
    float* up32 = nullptr;        // dyt_ctx::ad_ln == 2: the LayerNorm's input s (d_act W_up^T + b_up), fp32 [M,768] (its backward needs x_hat)
    bool h_has_adapter = false;   // h = mlp(x) + s up(d_act) + s b_up (fc2 carried the up-projection, DYT_OPT_FC2_CAT)
    // dyt_ctx::bwd16: what the backward pass reads, in the 16-bit operand type (written by the exact forward next to / instead of
    // the fp32 tensors above: q16 / k16 / v16 / o16 by the split attention kernel, u16 by the proj epilogue, z16 = gelu'(z) by the
    // fc1 epilogue, dact16 by the down-projection epilogue, h16 by the fc2 epilogue)
    void* ao3 = nullptr;   // bwd16: the attention output as the proj GEMM's split operand image, kept per layer: its hi plane (row stride SPLIT_A * 768) IS the 16-bit output the backward reads (no separate o16 write: 14 of the forward kernel's 125 us)
    void *q16 = nullptr, *k16 = nullptr, *v16 = nullptr, *o16 = nullptr, *u16 = nullptr, *z16 = nullptr, *dact16 = nullptr, *h16 = nullptr;
};
struct Transients {  // scratch of one pass (per slot, so two passes can run on two streams)
    void *xn, *h1, *g_at, *dZ, *ddz, *du_at, *dO, *dqkv, *dA2, *dxn, *dad;
    float* sk_ws = nullptr;   // inference-only contexts: the split-K workspace of the cls-only last block's fc2 (a training context lends it T.dZ)
    void* dact_s = nullptr;   // 16-bit modes: adapter_scale * d_act, the A2 operand of the fc2 + up-projection contraction
    void* dact3 = nullptr;    // 16-bit-backward split modes: the same as a [M][hi 64 | lo 64] image (three-part up-projection, alone or as the fc2 GEMM's leading tiles)
    void* a3 = nullptr;   // fp32 mode: [M, 3 * 3072] 16-bit scratch for the split A operand of a GEMM
    void* g3 = nullptr;   // [M, 3*768]: the gradient stream as a split operand, written by ln_bwd (next block's GELU' dgrad) and tok_bwd (proj dgrad); attention output in the forward pass
    void *xn3 = nullptr, *h3 = nullptr, *dqkv3 = nullptr;   // dqkv3: [M, 3*2304] from the attention backward   // ... and the split operands producers write directly: LN output [M, 3*768], fc1 output / dZ [M, 3*3072]
    float *g, *delta, *dmask, *tok_partial, *wg_partial, *wg_partial2;
    void *qlo = nullptr, *klo = nullptr, *vlo = nullptr;   // dyt_ctx::bwd16: lo planes of q / k / v (the hi planes are LayerS::q16 / k16 / v16), QKV epilogue -> split attention forward
    int* drop_src = nullptr;        // dyt_ctx::ln_fold: token rows of the DROPPED tokens of the block in flight (gather_index -> their up-projection launch)
    float2* st_compact = nullptr;   // dyt_ctx::ln_fold: scratch for LN2's (mean, rstd) in logical-row order (GemmArgs::ln_scratch)
    void* dad16 = nullptr;   // dyt_ctx::bwd16: the adapter dgrad as a 16-bit [M,768] operand of tok_bwd (T.dad of the 16-bit modes)
    // dyt_ctx::ad_ln: fp32-sized [M,768] scratch each -- xa: LayerNorm_a(u) in the operand type of the pass that reads it ("in"; recomputed by the backward);
    // dup: the gradient behind the adapter's LayerNorm ("out") / the fp32 adapter dgrad of an fp32 backward ("in"); ln_part: parameter-gradient partials
    float *xa = nullptr, *dup = nullptr, *aln_part = nullptr;
};
struct PoolS {  // video pooling head: saved activations of one pass (pool.hip)
    float *xf = nullptr, *P = nullptr, *o = nullptr, *y = nullptr, *qn = nullptr, *qhat = nullptr, *qs = nullptr, *st_q = nullptr;
    float *dq_part = nullptr, *gq = nullptr, *dqn = nullptr, *dy = nullptr, *dO = nullptr;
    float2 *st_f = nullptr, *st_kv = nullptr;
    void *xk = nullptr, *xv = nullptr, *Kp = nullptr, *Vp = nullptr;
    void *dKt = nullptr, *xkt = nullptr, *dVt = nullptr, *xvt = nullptr;   // [768, Mpad] token-transposed operands of the k / v weight gradients
    hipStream_t wstream = nullptr; hipEvent_t ev_wf = nullptr, ev_wj = nullptr; bool wpending = false;   // weight-gradient side stream
};
struct Slot {
    Transients T;
    PoolS pool;
    hipStream_t branch = nullptr;        // side stream for the adapter branch of this pass
    float* u0_own = nullptr; void* u0_at_own = nullptr;  // block-0 buffers (slot 1 may alias slot 0's, see step)
    hipEvent_t ev_f = nullptr, ev_j = nullptr;
    bool no_branch = false;              // this pass runs without its adapter side stream (see dyt_step_fwd_bwd)
    std::vector<LayerS> L;
    std::vector<float*> wg_part, wg_part2, tok_part;   // per-layer partial buffers: their reductions are batched (ReduceQueue)
    std::vector<float*> xs;  // depth+1 residual-stream snapshots
    int* counts = nullptr;   // [depth*B]
    void* ucls_at = nullptr; // last block: AT(u[cls rows]) [B,768] (adapter-down operand, kept for its wgrad)
    void* ucls16 = nullptr;  // dyt_ctx::bwd16: its 16-bit copy
    void* u0_16_own = nullptr;   // block-0 u16 of this slot (slot 1 may alias slot 0's, like u0_own)
    float2* part0_own = nullptr; // block-0 LayerNorm partials of this slot (idem)
    float* gcls = nullptr;   // last block backward: gradient at the cls rows [B,768]
    float* cls_n = nullptr;
    float2* head_stats = nullptr;
    float* pooled = nullptr;      // dyt_ctx::avg_pool: [max_batch][768] the head's input rows (avg_pool_fwd)
    float* head_dy = nullptr;     // dyt_ctx::fc_norm, training layout: [max_batch][768] dlogits @ W_head, the gradient behind fc_norm (its parameter gradients)
    float* head_part = nullptr;   // dyt_ctx::wide_head, training layout: [ceil(C/1024)][max_batch][768] class-slice partial sums of the head's dx (per slot: the two passes' backward run on two streams)
    int batch = 0, flags = 0;
    bool valid = false;
    bool tokens = false;     // the saved pass is token-level (DYT_F_TOKENS_OUT): every row of the last block is saved, no head ran -- dyt_backward_tokens' slot, not dyt_backward's
    bool saved16 = false;    // the saved pass holds the 16-bit tensors of a 16-bit backward (dyt_ctx::bwd16)
    const float* trainable = nullptr;  // flat trainable buffer the saved pass was computed with
    // stochastic depth (dyt_set_drop_path): the per-image branch factors [2][depth][batch] of this slot's passes -- drawn by the library
    // into dp_own at every training forward, or the caller's (dp_inject, dyt_set_drop_path_scales); dp = what the SAVED pass used (null: none)
    float* dp_own = nullptr; const float* dp_inject = nullptr; const float* dp = nullptr;
    float* gscr = nullptr;   // DYT_OPT_LEARNABLE_SCALE: [depth * layer_stride] the backward's up-projection gradients before the chain rule through the scale
};
// dyt_backward_tokens: the gradient enters at the tokens and the taps instead of at the logits
struct TokenGrads { const float* dtokens = nullptr; const float* const* dtaps = nullptr; };
struct ProfRec { int cat; double flops; hipEvent_t a, b; const int* m_dev; int M; };

struct dyt_ctx {
    dyt_config cfg;
    // dyt_config::inference_only: one aliased LayerS, one slot, two residual streams, forward transients and forward weight images only
    // (layout / layout_aux); every entry point that needs more refuses (refuse_inference)
    bool inf = false;
    // DYT_CREATE_WIDE_HEAD (dyt_ctx_create_ex): the head runs on the MFMA kernels of head_wide.hip (num_classes up to 65 536) instead of the row
    // kernels of step_tail.hip (up to 1024, the bit-pinned default); image model only
    bool wide_head = false;
    // DYT_CREATE_FC_NORM: the head's LayerNorm is the reference's fc_norm -- gamma / beta are trainable words of the caller's flat buffer
    // (off_fnw / off_fnb, directly behind head.bias) and the frozen norm_w / norm_b are not used; DYT_CREATE_AVG_POOL (given with DYT_CREATE_FC_NORM only): the row
    // that LayerNorm reads is the mean of the 196 patch rows of the last block's output (Slot::pooled) instead of the cls row; no cls-only tail
    bool fc_norm = false, avg_pool = false;
    int64_t off_fnw = 0, off_fnb = 0;
    int prec;
    size_t at;  // bytes per activation element
    char* arena = nullptr;
    size_t arena_size = 0, arena_used = 0;
    // second arena, allocated when DYT_OPT_F32_SPLIT16 is first switched on: everything only the split forms of the fp32 mode use
    // (the [hi | lo] weight images, the split operand scratch, the 16-bit tensors of a 16-bit backward) -- a plain fp32 context
    // does not carry it
    char* aux_arena = nullptr;
    size_t aux_size = 0;
    bool aux_bwd16 = false;     // the aux arena holds the bwd16 buffers
    int f8_mask_complete = 0;   // ... of a complete_model (teacher) pass: no token-keep decision depends on it (its gate output is discarded), only its logits -- "fp16x3q": 15 + 32 (32 = its attention forward as the hi * hi product alone)
    int f8_mask = 0;            // classes of forward GEMMs in that form: 1 qkv, 2 proj, 4 fc1, 8 fc2, 16 patch embedding ("fp16f8" = 31, "fp16x3q" = 3)
    bool f8 = false;            // "fp16f8": forward GEMMs as hi * hi on the f16 matrix cores + the two correction products on the fp8 ones (DYT_OPT_F32_SPLIT16 = 4; implies bwd16)
    int* pe_w_exp = nullptr; unsigned* f8_scratch = nullptr;
    bool bwd16 = false;         // "fp16x3h": the fp16x3 forward, the backward on the 16-bit mode's operands and kernels (DYT_OPT_F32_SPLIT16 = 3)
    void *ad_up_wT16 = nullptr, *ad_down_wT16 = nullptr, *ad_scratch16 = nullptr;   // bwd16: per-step 16-bit copies of the adapter matrices the dgrads read
    void* ad_up_w3 = nullptr;   // bwd16: [depth][768][hi 64 | lo 64] image of the (fp32) up-projection copies: the three-part up-projection's weight operand
    // frozen
    float *cls, *pos, *pe_b, *norm_w, *norm_b;
    void* pe_w;
    std::vector<LayerW> W;
    // per-step AT copies of the adapters (all layers contiguous)
    void *ad_down_w, *ad_down_wT, *ad_up_w, *ad_up_wT;
    float* ad_down_b;
    bool split_attn = true;     // ... and the attention forward too (attn_fwd_split_kernel; DYT_SPLIT_ATTN=0: exact fp32 MFMA kernel)
    float split_gs = 4096.0f;   // ... their gradient operands are multiplied by this power of two before the split
    int split_bwd_parts = 3;    // ... products of the GRADIENT GEMMs' contraction (3 full, 1 = dY_hi * W_hi: "fp16x3f")
    int split_bwd_attn_parts = 3;   // ... and of the split attention backward's dP / dQ / dK / dV products (3 or 1; the score recomputation keeps three)
    const float* soft_targets = nullptr; int soft_batch = 0;   // dyt_set_soft_targets: class-probability targets of the next loss evaluations
    // dyt_set_mix: while mix_params (a DEVICE block the kernels read at run time) is set, forward_impl launches the mixing image load and
    // dyt_step_fwd_bwd writes the class-probability rows into mix_soft ([max_batch][num_classes], allocated by the first dyt_set_mix) for its loss
    const MixParams* mix_params = nullptr; int mix_frames = 1; float* mix_soft = nullptr; size_t mix_soft_bytes = 0;
    // dyt_set_erase: while erase_table (a DEVICE table the kernels read at run time, csrc/erase.h) is set, the TRAINING passes of forward_impl
    // launch the erasing image load (which also mixes when mix_params is set); erase_capacity = the rows the table's allocation holds
    const void* erase_table = nullptr; int erase_capacity = 0; int erase_frames = 1;
    bool split16 = false;       // fp32 mode: frozen-weight GEMMs as three 16-bit MFMA products (DYT_OPT_F32_SPLIT16)
    void* pe_w3 = nullptr;
    // 16-bit modes: LayerNorm-2 is not a kernel -- the proj epilogue emits per-row partial statistics of u, fc1 contracts the 16-bit copy
    // of u with gamma-folded weights and normalises in its epilogue (GemmArgs::ln_part).  -0.3 ms of a 26.8 ms step; vs the
    // oracle at B=16 as accurate as the kernel form (logits 1.6e-3 vs 1.8e-3).  Environment DYT_LN_FOLD=0 when the context is created:
    // the ln_fwd / ln_gather kernels (the reference's autocast order: LayerNorm in fp32, then round)
    bool ln_fold = true;
    bool fc2_cat = true;        // 16-bit modes: adapter up-projection rides on the fc2 GEMM where no separate h is needed
    // trainable flat layout
    int64_t layer_stride, off_dw, off_db, off_uw, off_ub, off_gw, off_gb, off_hw, off_hb, n_train;
    // video model (frames > 1): attentive pooling head, trainable
    int frames = 1;
    int64_t off_pquery = 0, off_pnq_w = 0, off_pnq_b = 0, off_pnk_w = 0, off_pnk_b = 0, off_pnv_w = 0, off_pnv_b = 0,
            off_pq_w = 0, off_pk_w = 0, off_pv_w = 0, off_pq_bias = 0, off_pv_bias = 0, off_pproj_w = 0, off_pproj_b = 0;
    void *pk_w = nullptr, *pk_wT = nullptr, *pv_w = nullptr, *pv_wT = nullptr;   // per-step AT copies of k / v weights
    std::vector<Slot> slots;
    float *dl_s, *dl_t, *dtok, *logits_s, *logits_t, *losses, *grad2, *loss_part;
    int* cls_rows = nullptr;   // [max_batch] token row of each image's cls token (b*197)
    uint64_t* seed_dev = nullptr;   // device-side Philox seed word (DYT_F_DEVICE_SEED: captured graphs draw fresh noise per replay)
    float* clip_scratch = nullptr;  // [256] partial sums of dyt_clip_grad_norm
    // gradient availability for a chunked all-reduce (dyt_stream_wait_grads): layers >= grad_split and the head are final
    hipEvent_t ev_half_s = nullptr, ev_half_t = nullptr, ev_upper = nullptr, ev_comm = nullptr;
    hipStream_t aux = nullptr;       // sums the upper part of the two passes' gradient buffers while the backward goes on
    bool upper_recorded = false;
    float gs = 1.0f;           // factor the gradient carries wherever it is held in the 16-bit operand type (fp16 build: 2^12, a
                               // fixed loss scale confined to the library: fp32 streams and every returned gradient are unscaled)
    bool cls_tail = true;      // last block: MLP/adapter on the cls rows only (only they reach the head)
    // second stream: the student and the teacher pass of a step are independent and run concurrently
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_b0 = nullptr;
    bool overlap = true;                 // any stream overlap
    bool ov_pass = true, ov_branch = false;  // student / teacher passes on two streams; adapter branch on its own stream
    bool ov_bwd_serial = false;          // the teacher's backward starts after the student's (bit-reproducible schedule)
    bool share_block0 = true;  // step: the teacher pass reuses the student's embedding + block-0 attention branch
    bool learn_scale = false;    // DYT_OPT_LEARNABLE_SCALE: tuning_config.ffn_adapter_scalar == "learnable_scalar" (dynamic_adapter.py:101-102): the scale is
                                 // the trainable word off_sc of every block (a padding slot of the flat layout behind the gate bias)
    int64_t off_sc = 0;
    // fp16 build, 16-bit mode (round 6): between the row kernels of the backward the gradient stream is carried by the 16-bit gs-scaled copy each
    // of them writes for the GEMM behind it (ln_bwd: g_at, tok_bwd: du_at) instead of ALSO as an fp32 [M,768] stream that both read and
    // write: -230 MB per block and pass (tok_bwd / ln_bwd 336 -> 221 MB each).  Every hop rounds the stream to 11 bits (at 2^12 x its
    // value), so round-off accumulates over the 23 hops of a pass (fp16 mode, five seeds: up_proj 1.1e-3 -> 1.3e-3, head unchanged): not used by the
    // bfloat16 build (8 bits).  DYT_G16=0: the fp32 stream.
    bool g16 = false;
    // dyt_config::adapter_ln (tuning_config.ffn_adapter_layernorm_option): 0 none, 1 "in", 2 "out"; gamma / beta of block l at l * layer_stride + off_alw / off_alb
    int ad_ln = 0;
    int64_t off_alw = 0, off_alb = 0;
    void* ad_up_ws = nullptr;   // "out": [depth][768][RP] adapter_scale * up_proj.weight in the forward's operand type (the LayerNorm input is s (d_act W^T + b))
    bool pass_ran = false;       // a forward pass has run in this context: DYT_OPT_LEARNABLE_SCALE may no longer change
    float* ad_up_bp = nullptr;   // [depth][768] s * up_proj.bias (prep_adapters_kernel)
    float* ad_lift = nullptr;    // [2][depth] 2^e / 2^-e of the 16-bit up_proj dgrad operand (adapter_lift_kernel)
    float drop_path_rate = 0.f;  // timm DropPath rate of the LAST block (block l: rate * l / (depth - 1)); training forward passes only
    InputNorm in_norm = IN_NORM_IMAGENET;   // dyt_set_input_norm: per-channel mean / std of DYT_F_IMAGES_U8 passes (host values, carried in the launch arguments)
    int count_flops_tokens = 0;  // > 0: Block.forward_count_flops -- MLP on the first n tokens of every image
    // profiling
    bool prof = false;
    std::vector<ProfRec> recs;
    std::vector<hipEvent_t> pool;
};

// The functions that cross units, under the unit that defines them; everything else in those units is static.
namespace dyt {
// ctx.hip
int refuse_inference(const dyt_ctx* c, const char* what);
int set_matrix(dyt_ctx* c, const float* src, void* w, void* wT, int N, int K, hipStream_t s);
hipEvent_t get_event(dyt_ctx* c);
// mix.hip
int check_mix_batch(const dyt_ctx* c, int batch);   // mix on: an image count that cannot be paired, DYT_ERR_ARG with a text
// erase.hip
int check_erase_batch(const dyt_ctx* c, int batch);   // erasing on: a batch the table has no rows for, DYT_ERR_ARG with a text
// forward.hip
int prep_adapters(dyt_ctx* c, const float* trainable, hipStream_t s);
int prep_pool(dyt_ctx* c, const float* tr, hipStream_t s);
int branch_stream(dyt_ctx* c, Slot& S, hipStream_t* out);
int forward_impl(dyt_ctx* c, int slot, const float* images, int B, int flags, const float* trainable,
                 const float* g1, const float* g2, const uint8_t* keep_mask, uint64_t seed, float* logits,
                 float* token_select, float* token_logits, bool do_prep, hipStream_t s,
                 const Slot* share0 = nullptr, hipEvent_t ev_b0_record = nullptr, hipEvent_t ev_b0_wait = nullptr,
                 float* const* taps = nullptr);   // taps[l] (null: not wanted) := xs[l + 1], dyt_forward_taps
// backward.hip
int backward_impl(dyt_ctx* c, int slot, const float* trainable, const float* dlogits, const float* dtoken_select,
                  const float* dtok, const float* dtoken_logits, float* grad, hipStream_t s,
                  hipEvent_t ev_split = nullptr, int split = 0, const TokenGrads* tg = nullptr);
// debug.hip (measurement hooks behind CK / ISO / POISON)
bool dbg_ck_on();
int dbg_ck_reset(hipStream_t s);
int dbg_ck(int slot, hipStream_t s, const char* what, int layer, const void* p, size_t bytes);
int dbg_iso_enter(int slot, int cls, hipStream_t* s, hipStream_t* keep);
int dbg_iso_leave(int slot, hipStream_t* s, hipStream_t keep);
int dbg_poison(int bit, void* p, size_t bytes, hipStream_t s);
}  // namespace dyt

// ------------------------------------------------------------------------------------------
// orchestration macros of forward_impl / backward_impl and the pooling head (they expect c, s, P, S, T, slot, l in scope)
// ------------------------------------------------------------------------------------------
struct ProfScope {
    dyt_ctx* c; hipStream_t s; ProfRec r; bool on;
    ProfScope(dyt_ctx* c_, hipStream_t s_, int cat, double flops, const int* m_dev = nullptr, int M = 0)
        : c(c_), s(s_), on(c_->prof) {
        if (on) {
            r.cat = cat; r.flops = flops; r.m_dev = m_dev; r.M = M;
            r.a = get_event(c); r.b = get_event(c);
            hipEventRecord(r.a, s);
        }
    }
    ~ProfScope() { if (on) { hipEventRecord(r.b, s); c->recs.push_back(r); } }
};
#define RUN(cat, flops, call)                  \
    do {                                       \
        ProfScope _ps(c, s, (cat), (flops));   \
        int _rc = (call);                      \
        if (_rc) return _rc;                   \
    } while (0)
// GEMM whose valid row count lives on the device (compacted MLP): FLOPs are scaled by the
// count actually processed when the profile is read back
#define RUN_GEMM(kind, a)                                                \
    do {                                                                 \
        ProfScope _ps(c, s, 0, (a).flops(), (a).m_dev, (a).M);           \
        int _rc = launch_gemm(P, (kind), (a), s);                        \
        if (_rc) return _rc;                                             \
    } while (0)
#define FORK(sb)  do { if (sb) { DYT_HIP_CHECK(hipEventRecord(S.ev_f, s)); DYT_HIP_CHECK(hipStreamWaitEvent(sb, S.ev_f, 0)); } } while (0)
#define JOIN(sb)  do { if (sb) { DYT_HIP_CHECK(hipEventRecord(S.ev_j, sb)); DYT_HIP_CHECK(hipStreamWaitEvent(s, S.ev_j, 0)); } } while (0)
// run a launch on the branch stream when there is one
#define RUN_ON(sb, cat, flops, call)           \
    do {                                       \
        hipStream_t _keep = s;                 \
        if (sb) s = sb;                        \
        ProfScope _ps(c, s, (cat), (flops));   \
        int _rc = (call);                      \
        s = _keep;                             \
        if (_rc) return _rc;                   \
    } while (0)
#define SPLIT(a, w3) do { if (c->split16) { (a).W3 = (w3); (a).a3 = T.a3; } } while (0)
// forward GEMM class g (0 qkv, 1 proj, 2 fc1, 3 fc2) in the three-part or, where the pass's class mask fm says so, the fp8-correction form
// (w3b: the class's second image, used by the pass whose form differs from the student's)
#define SPLIT_F(a, w3, w3b, g) do { SPLIT(a, (((fm ^ c->f8_mask) >> (g)) & 1) ? (w3b) : (w3)); \
        if ((fm >> (g)) & 1) { (a).f8 = true; (a).w_exp = W.w_exp + (g); } } while (0)
// gradient operands: scaled by 2^12 before the split so that the lo parts stay fp16 normals (the loss scale of the fp16 mode)
// the producing kernel already wrote the split operand into `buf`
#define SPLIT_READY(a, buf) do { if (c->split16) { (a).a3 = (buf); (a).a3_ready = true; } } while (0)
#define SPLIT_G(a, w3) do { if (c->split16) { (a).W3 = (w3); (a).a3 = T.a3; (a).a3_scale = c->split_gs; (a).a3_parts = c->split_bwd_parts; } } while (0)
// measurement hooks of the backward pass (debug.hip says what each one finds)
#define CK(what, ptr, bytes) do { int _r = dbg_ck(slot, s, (what), l, (ptr), (bytes)); if (_r) return _r; } while (0)
#define ISO(cls, body)                                                        \
    do {                                                                      \
        hipStream_t _iso_keep;                                                \
        { int _r = dbg_iso_enter(slot, (cls), &s, &_iso_keep); if (_r) return _r; } \
        body                                                                  \
        { int _r = dbg_iso_leave(slot, &s, _iso_keep); if (_r) return _r; }   \
    } while (0)
#define POISON(bit, ptr, bytes) do { int _r = dbg_poison((bit), (ptr), (bytes), s); if (_r) return _r; } while (0)
