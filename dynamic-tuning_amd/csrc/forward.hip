// The forward pass: per-step operand refresh of the adapters and the pooling head, forward_impl, dyt_forward.
#include "ctx.h"
#include "image_items.h"

namespace dyt {

// ------------------------------------------------------------------------------------------
// small kernels private to this file
// ------------------------------------------------------------------------------------------
// Per-step refresh of the adapter weights in the layouts / dtype the GEMMs want:
//   down_w  [RP,768] (rows >= r zero)      forward down-projection (N = RP, K = 768)
//   down_wT [768,RP]                       dgrad through down_proj (N = 768, K = RP)
//   up_w    [768,RP] (cols >= r zero)      forward up-projection   (N = 768, K = RP)
//   up_wT   [RP,768]                       dgrad through up_proj   (N = RP, K = 768)
//   down_b  [RP] fp32
template <class AT>
__global__ void prep_adapters_kernel(const float* __restrict__ flat, int64_t layer_stride, int64_t off_dw, int64_t off_db,
                                     int64_t off_uw, int r, AT* __restrict__ down_w, AT* __restrict__ down_wT,
                                     AT* __restrict__ up_w, AT* __restrict__ up_wT, float* __restrict__ down_b,
                                     AT* __restrict__ up_ws, float scale, int64_t off_sc, int64_t off_ub, float* __restrict__ up_bp, float bias_scale,
                                     const float* __restrict__ up_t_lift) {
    // off_sc >= 0 ("learnable_scalar", DYT_OPT_LEARNABLE_SCALE): the up-projection copies and up_bp [depth][768] carry the block's trainable
    // scale s = flat[off_sc] (W' = s W_up, b' = s b_up), and every kernel downstream runs with scale 1
    const int l = blockIdx.y;
    const float* base = flat + (int64_t)l * layer_stride;
    const float ls = off_sc >= 0 ? base[off_sc] : 1.0f;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    constexpr int SZ = RP * D;
    if (idx >= SZ) return;
    {   // idx -> (j, c) of [RP,768]
        const int j = idx / D, c = idx - j * D;
        const float dw = j < r ? base[off_dw + (int64_t)j * D + c] : 0.f;   // down_proj.weight [r,768]
        const float uw = j < r ? ls * base[off_uw + (int64_t)c * r + j] : 0.f;   // up_proj.weight [768,r]
        down_w[(size_t)l * SZ + idx] = from_f32<AT>(dw);
        if (up_wT) up_wT[(size_t)l * SZ + idx] = from_f32<AT>(up_t_lift ? uw * up_t_lift[l] : uw);   // (null, like down_wT: inference-only contexts)
    }
    {   // idx -> (c, j) of [768,RP]
        const int c = idx / RP, j = idx - c * RP;
        const float dw = j < r ? base[off_dw + (int64_t)j * D + c] : 0.f;
        const float uw = j < r ? ls * base[off_uw + (int64_t)c * r + j] : 0.f;
        if (down_wT) down_wT[(size_t)l * SZ + idx] = from_f32<AT>(dw);
        up_w[(size_t)l * SZ + idx] = from_f32<AT>(uw);
        if (up_ws) up_ws[(size_t)l * SZ + idx] = from_f32<AT>(scale * uw);
    }
    if (idx < RP) down_b[l * RP + idx] = idx < r ? base[off_db + idx] : 0.f;
    if (up_bp && idx < D) up_bp[l * D + idx] = bias_scale * ls * base[off_ub + idx];   // bias_scale: the adapter's LayerNorm "out" form takes s b_up here
}

// up_t_lift of prep_adapters_kernel: lift[l] = 2^e, lift[depth + l] = 2^-e with e = adapter_lift_exp(max |s W_up|) of block l (s: the learnable
// scale, else 1).  The 16-bit up_proj dgrad operand up_wT carries 2^e, so its product ddz carries gs 2^e, and every consumer of ddz takes 2^-e
// back out (WgradArgs::alpha_dev, GemmArgs::out_dscale, TokBwdArgs::cat_ddz_dscale).  One workgroup per block, on the device: no host sync.
__global__ __launch_bounds__(256) void adapter_lift_kernel(const float* __restrict__ flat, int64_t layer_stride, int64_t off_uw, int64_t off_sc,
                                                           int r, int depth, float* __restrict__ lift) {
    __shared__ float red[256];
    const int l = blockIdx.x, tid = threadIdx.x;
    const float* base = flat + (int64_t)l * layer_stride;
    const float ls = off_sc >= 0 ? base[off_sc] : 1.0f;
    float m = 0.f;
    for (int i = tid; i < D * r; i += 256) m = fmaxf(m, fabsf(ls * base[off_uw + i]));
    red[tid] = m;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] = fmaxf(red[tid], red[tid + o]);
        __syncthreads();
    }
    if (tid == 0) {
        const int e = adapter_lift_exp(red[0]);
        lift[l] = ldexpf(1.0f, e);
        lift[depth + l] = ldexpf(1.0f, -e);
    }
}

}  // namespace dyt

// ------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------
int dyt::prep_adapters(dyt_ctx* c, const float* trainable, hipStream_t s) {
    const dim3 grid((RP * D + 255) / 256, c->cfg.depth);
    const int64_t sc_off = c->learn_scale ? c->off_sc : -1;
    // "out" form of the adapter's LayerNorm: its input is s (d_act W_up^T + b_up) -- scaled weight copies + a scaled bias copy for that GEMM
    const bool out_ln = c->ad_ln == 2;
    float* up_bp = (c->learn_scale || out_ln) ? c->ad_up_bp : nullptr;
    const float ws_scale = out_ln ? c->cfg.adapter_scale : 0.f, b_scale = out_ln ? c->cfg.adapter_scale : 1.0f;
    if ((c->prec != 0 || c->bwd16) && !c->inf)   // the 16-bit up_proj dgrad operand's power of two (read by prep_adapters_kernel<bf16> and the backward)
        hipLaunchKernelGGL(adapter_lift_kernel, dim3(c->cfg.depth), dim3(256), 0, s, trainable, c->layer_stride, c->off_uw, sc_off,
                           c->cfg.ffn_num, c->cfg.depth, c->ad_lift);
    if (c->prec == 0) {
        hipLaunchKernelGGL(prep_adapters_kernel<float>, grid, dim3(256), 0, s, trainable, c->layer_stride, c->off_dw, c->off_db,
                           c->off_uw, c->cfg.ffn_num, (float*)c->ad_down_w, (float*)c->ad_down_wT, (float*)c->ad_up_w,
                           (float*)c->ad_up_wT, c->ad_down_b, out_ln ? (float*)c->ad_up_ws : (float*)nullptr, ws_scale, sc_off, c->off_ub, up_bp, b_scale,
                           (const float*)nullptr);
        if (c->bwd16) {   // + the 16-bit transposes the 16-bit backward's adapter dgrads multiply by
            bf16* scr = (bf16*)c->ad_scratch16;
            if (!c->inf) {   // (an inference-only context has none of the four)
            hipLaunchKernelGGL(prep_adapters_kernel<bf16>, grid, dim3(256), 0, s, trainable, c->layer_stride, c->off_dw, c->off_db,
                               c->off_uw, c->cfg.ffn_num, scr, (bf16*)c->ad_down_wT16, scr + (size_t)c->cfg.depth * RP * D,
                               (bf16*)c->ad_up_wT16, c->ad_down_b, (bf16*)nullptr, 0.f, sc_off, c->off_ub, up_bp, b_scale, (const float*)c->ad_lift);
            }
            if (c->ad_up_w3) {   // [hi | lo] image of the fp32 up-projection copies just written (all blocks: depth * 768 rows of 64)
                int rc = launch_split3_w((const float*)c->ad_up_w, c->ad_up_w3, c->cfg.depth * D, RP, s);
                if (rc) return rc;
            }
        }
    } else
        hipLaunchKernelGGL(prep_adapters_kernel<bf16>, grid, dim3(256), 0, s, trainable, c->layer_stride, c->off_dw, c->off_db,
                           c->off_uw, c->cfg.ffn_num, (bf16*)c->ad_down_w, (bf16*)c->ad_down_wT, (bf16*)c->ad_up_w,
                           (bf16*)c->ad_up_wT, c->ad_down_b, out_ln ? (bf16*)c->ad_up_ws : (bf16*)nullptr, ws_scale, sc_off, c->off_ub, up_bp, b_scale,
                           (const float*)c->ad_lift);
    DYT_HIP_CHECK(hipGetLastError());
    return 0;
}

// adapter-branch side stream of a pass (created on first use); null when overlap is off / profiling
int dyt::branch_stream(dyt_ctx* c, Slot& S, hipStream_t* out) {
    *out = nullptr;
    if (!c->overlap || !c->ov_branch || c->prof) return 0;
    if (S.no_branch) return 0;
    if (!S.branch) {
        DYT_HIP_CHECK(hipStreamCreateWithFlags(&S.branch, hipStreamNonBlocking));
        DYT_HIP_CHECK(hipEventCreateWithFlags(&S.ev_f, hipEventDisableTiming));
        DYT_HIP_CHECK(hipEventCreateWithFlags(&S.ev_j, hipEventDisableTiming));
    }
    *out = S.branch;
    return 0;
}

static_assert(IN_F_TOKENS_IN == DYT_F_TOKENS_IN && IN_F_IMAGES_U8 == DYT_F_IMAGES_U8 && IN_F_IMAGES_NHWC == DYT_F_IMAGES_NHWC, "input_norm.h flag values");

static inline void* at_off(const dyt_ctx* c, void* base, size_t elems) { return static_cast<char*>(base) + elems * c->at; }

// ------------------------------------------------------------------------------------------
// video model: attentive pooling head (video_models/video_vision_transformer_IN21K.py:463-483)
// ------------------------------------------------------------------------------------------
int dyt::prep_pool(dyt_ctx* c, const float* tr, hipStream_t s) {
    if (c->frames <= 1) return 0;
    int rc = set_matrix(c, tr + c->off_pk_w, c->pk_w, c->pk_wT, D, D, s);
    if (rc) return rc;
    return set_matrix(c, tr + c->off_pv_w, c->pv_w, c->pv_wT, D, D, s);
}

static int pool_forward(dyt_ctx* c, Slot& S, const float* tr, float* logits, int B, hipStream_t s) {
    const int P = c->prec, t = c->frames, clips = B / t, M = B * NT, NK = t * NT, C = c->cfg.num_classes;
    PoolS& Q = S.pool;
    RUN(2, 0, launch_pool_ln_fwd(P, S.xs[c->cfg.depth], c->norm_w, c->norm_b, tr + c->off_pnk_w, tr + c->off_pnk_b,
                                 tr + c->off_pnv_w, tr + c->off_pnv_b, Q.xf, Q.st_f, Q.st_kv, Q.xk, Q.xv, M, s));
    {
        GemmArgs a; a.A = Q.xk; a.W = c->pk_w; a.M = M; a.N = D; a.K = D; a.out_at = Q.Kp;   // k has no bias
        RUN_GEMM(EPI_BIAS_AT, a);
    }
    {
        GemmArgs a; a.A = Q.xv; a.W = c->pv_w; a.M = M; a.N = D; a.K = D; a.bias = tr + c->off_pv_bias; a.out_at = Q.Vp;
        RUN_GEMM(EPI_BIAS_AT, a);
    }
    RUN(2, 0, launch_pool_q_fwd(tr + c->off_pquery, tr + c->off_pnq_w, tr + c->off_pnq_b, tr + c->off_pq_w,
                                tr + c->off_pq_bias, Q.qn, Q.qhat, Q.st_q, Q.qs, s));
    RUN(1, 4.0 * clips * NH * (double)NK * HD, launch_pool_attn_fwd(P, Q.qs, Q.Kp, Q.Vp, Q.P, Q.o, clips, NK, s));
    RUN(2, 0, launch_rows_linear(Q.o, tr + c->off_pproj_w, tr + c->off_pproj_b, Q.y, clips, D, D, 1.0f, s));
    RUN(2, 0, launch_rows_linear(Q.y, tr + c->off_hw, tr + c->off_hb, logits, clips, C, D, 1.0f, s));
    return 0;
}

int dyt::forward_impl(dyt_ctx* c, int slot, const float* images, int B, int flags, const float* trainable,
                      const float* g1, const float* g2, const uint8_t* keep_mask, uint64_t seed, float* logits,
                      float* token_select, float* token_logits, bool do_prep, hipStream_t s,
                      const Slot* share0, hipEvent_t ev_b0_record, hipEvent_t ev_b0_wait, float* const* taps) {
    // share0: reuse another pass's embedding + block-0 attention branch (same images, same frozen weights):
    //         its u / u_at of block 0 become this pass's (the step function aliases the pointers).
    if (slot < 0 || slot >= c->cfg.slots) { set_error("slot %d out of range", slot); return DYT_ERR_ARG; }
    if (B < 1 || B > c->cfg.max_batch) { set_error("batch %d exceeds max_batch %d", B, c->cfg.max_batch); return DYT_ERR_ARG; }
    if (!images || !trainable || !logits) { set_error("null argument"); return DYT_ERR_ARG; }
    if ((g1 == nullptr) != (g2 == nullptr)) { set_error("g1 and g2 must be given together"); return DYT_ERR_ARG; }
    { int rc = check_image_input(flags, images); if (rc) return rc; }   // DYT_F_IMAGES_U8 / _NHWC: `images` is a byte batch
    const bool mix = c->mix_params && !(flags & DYT_F_TOKENS_IN);   // dyt_set_mix: the embedding load mixes every image with its partner
    if (mix) { int rc = check_mix_batch(c, B); if (rc) return rc; }
    const bool erase = c->erase_table && (flags & DYT_F_TRAINING) && !(flags & DYT_F_TOKENS_IN);   // dyt_set_erase: training passes erase in the same load; an eval forward never does
    if (erase) { int rc = check_erase_batch(c, B); if (rc) return rc; }
    if (flags & DYT_F_SAVE) { int rc = refuse_inference(c, slot > 0 ? "dyt_forward with DYT_F_SAVE into a slot > 0" : "dyt_forward with DYT_F_SAVE"); if (rc) return rc; }
    if ((flags & DYT_F_TRAINING) && c->drop_path_rate > 0.f) { int rc = refuse_inference(c, "a training forward with stochastic depth"); if (rc) return rc; }
    const int P = c->prec, depth = c->cfg.depth, M = B * NT, r = c->cfg.ffn_num;
    const bool training = flags & DYT_F_TRAINING, complete = flags & DYT_F_COMPLETE, save = flags & DYT_F_SAVE;
    const bool masked_dense = (flags & DYT_F_MASKED_DENSE) && !complete;
    const bool dense = complete || masked_dense;
    const bool use_gate = !complete || (flags & DYT_F_GATE_ALWAYS);
    const float drop_p = training ? c->cfg.adapter_dropout : 0.f;
    const uint64_t* seed_dev = (flags & DYT_F_DEVICE_SEED) ? c->seed_dev : nullptr;
    const int fm = c->split16 ? (complete ? c->f8_mask_complete : c->f8_mask) : 0;   // classes (qkv 1, proj 2, fc1 4, fc2 8, embed 16) whose split operands are in the hi16 / fp8 form
    const bool planes = c->bwd16 && c->split16 && c->split_attn;   // q / k / v as 16-bit hi + lo planes (QKV epilogue -> split attention kernel; hi = what a 16-bit backward reads)
    const bool save16 = save && planes;   // "fp16x3h": what the backward reads is saved in the 16-bit operand type
    const bool fold = c->ln_fold && P != 0;   // LayerNorm-2 inside the fc1 GEMM (dyt_ctx::ln_fold)
    Slot& S = c->slots[c->inf ? 0 : slot];   // inference-only: one slot, whatever the index (it still seeds the pass's noise streams)
    Transients& T = S.T;
    // inference-only: what an eval forward stores for the backward alone is not stored -- the launchers take a null pointer
    // as "no-save variant"; values that flow on are computed by the same instructions
    const bool nosave = c->inf;
    S.valid = false;
    if (B % c->frames != 0) { set_error("video model: batch %d is not a multiple of frames %d", B, c->frames); return DYT_ERR_ARG; }
    if (do_prep) { int rc = prep_adapters(c, trainable, s); if (rc) return rc; rc = prep_pool(c, trainable, s); if (rc) return rc; }
    hipStream_t sb = nullptr;
    { int rc = branch_stream(c, S, &sb); if (rc) return rc; }

    // stochastic depth (reference vision_transformer_IN21K.py:121,131,148,159; dpr = linspace(0, rate, depth), :285): training passes only;
    // every pass draws its own factors, like every call of the reference's forward does.  dp[(branch * depth + l) * B + b]
    const float* dp = nullptr;
    if (training && (S.dp_inject || c->drop_path_rate > 0.f)) {
        if (c->count_flops_tokens) { set_error("drop_path with the count_flops forward"); return DYT_ERR_STATE; }
        dp = S.dp_inject;
        if (!dp) {
            RUN(2, 0, launch_drop_path_draw(S.dp_own, depth, B, c->drop_path_rate, seed, seed_dev, ((uint64_t)slot << 32) | 0x10000ull, s));
            dp = S.dp_own;
        }
    }
    S.dp = dp;
    const bool tokens_in = flags & DYT_F_TOKENS_IN, tokens_out = flags & DYT_F_TOKENS_OUT;
    if (tokens_in) {
        // stand-alone Block.forward (reference vision_transformer_IN21K.py:144-165 called on a token tensor, as
        // block_flops_dict.py:36-46 does): `images` IS the residual stream [B,197,768]
        DYT_HIP_CHECK(hipMemcpyAsync(S.xs[0], images, (size_t)M * D * sizeof(float), hipMemcpyDeviceToDevice, s));
    } else if (!share0) {
        // patch embedding: image load (im2col order; bytes are normalised in the load: the same operand bits as the float path on the
        // normalised image) + GEMM (+bias +pos_embed), cls rows
        {
            ImageLoadArgs a;
            a.src = images;
            a.src_kind = !(flags & DYT_F_IMAGES_U8) ? IMAGE_SRC_F32 : (flags & DYT_F_IMAGES_NHWC) ? IMAGE_SRC_U8_NHWC : IMAGE_SRC_U8;
            a.dst = T.xn; a.dst_kind = P == 0 ? IMAGE_DST_OPERAND_F32 : IMAGE_DST_OPERAND_16;
            a.batch = B; a.frames = erase ? c->erase_frames : c->mix_frames;
            a.norm = c->in_norm;
            if (mix) a.mix = c->mix_params;
            if (erase) { a.erase_table = c->erase_table; a.erase_capacity = c->erase_capacity; }
            RUN(2, 0, launch_image_load(a, s));
        }
        {
            GemmArgs a; a.A = T.xn; a.W = c->pe_w; a.M = B * NP; a.N = D; a.K = D;
            a.bias = c->pe_b; a.pos = c->pos; a.out_f32 = S.xs[0]; SPLIT(a, c->pe_w3);
            if (fm & 16) { a.f8 = true; a.w_exp = c->pe_w_exp; }
            RUN_GEMM(EPI_EMBED, a);
        }
        RUN(2, 0, launch_cls_rows(c->cls, c->pos, S.xs[0], B, s));
    } else if (ev_b0_wait) {
        DYT_HIP_CHECK(hipStreamWaitEvent(s, ev_b0_wait, 0));  // the other pass's block-0 `u` is complete
    }

    for (int l = 0; l < depth; ++l) {
        const LayerW& W = c->W[l];
        LayerS& L = S.L[l];
        const float* base = trainable + (int64_t)l * c->layer_stride;
        float* x = S.xs[l];
        float* xo = S.xs[l + 1];
        // learnable scale: the up-projection copies / up_bp are already multiplied by it (prep_adapters_kernel)
        const float ad_scale = c->learn_scale ? 1.0f : c->cfg.adapter_scale;
        const float* up_bias = c->learn_scale ? c->ad_up_bp + (size_t)l * D : base + c->off_ub;
        const float* dp1 = (dp && l > 0) ? dp + (size_t)l * B : nullptr;             // attention branch (block 0: rate 0, never dropped)
        const float* dp2 = (dp && l > 0) ? dp + (size_t)(depth + l) * B : nullptr;   // MLP branch
        if (!(share0 && l == 0)) {
            RUN(2, 0, launch_ln_fwd(P, x, W.ln1_w, W.ln1_b, T.xn, L.st1, M, s, c->split16 ? T.xn3 : nullptr, fm & 1));
            {
                GemmArgs a; a.A = T.xn; a.W = W.qkv_w; a.Wp = W.qkv_wp; a.M = M; a.N = 3 * D; a.K = D; a.bias = W.qkv_b;
                a.out_at = L.q; a.out_at2 = L.k; a.out_at3 = L.v; SPLIT_F(a, W.qkv_w3, W.qkv_w3b, 0); SPLIT_READY(a, T.xn3);
                if (planes) { a.out_at = L.q16; a.out_at2 = L.k16; a.out_at3 = L.v16; a.qkv_lo[0] = T.qlo; a.qkv_lo[1] = T.klo; a.qkv_lo[2] = T.vlo; }
                RUN_GEMM(EPI_QKV, a);
            }
            void* ao3 = (c->split16 && c->split_attn) ? ((save16 && L.ao3) ? L.ao3 : T.g3) : nullptr;   // the split attention kernel also writes the proj GEMM's operand
            // last block of a pass without a gate (teacher / complete model): the proj GEMM runs on the gathered cls rows of the fp32 output
            const bool tail_proj = c->cls_tail && l == depth - 1 && l > 0 && !tokens_out && !use_gate;
            {
                AttnFwdArgs a; a.batch = B; a.q = L.q; a.k = L.k; a.v = L.v;
                a.lse = L.lse; a.lse_optional = nosave;   // (the attention kernels without a no-save variant keep their lse store)
                a.split16 = c->split16 && c->split_attn; a.out3 = ao3; a.out3_f8 = (fm >> 1) & 1;
                a.out = (save16 && ao3 && !tail_proj) ? nullptr : L.attn_o;   // bwd16: the fp32 output is not needed once the proj operand is written (its 16-bit copy is the hi plane of ao3)
                if (planes) {   // the hi planes are also the 16-bit copies the backward reads
                    a.planar = true; a.q_hi = L.q16; a.k_hi = L.k16; a.v_hi = L.v16; a.q_lo = T.qlo; a.k_lo = T.klo; a.v_lo = T.vlo;
                    a.parts = (fm & 32) ? 1 : 3;
                }
                RUN(1, 4.0 * B * NH * (double)NT * NT * HD, launch_attn_fwd(P, a, s));
            }
            if (tail_proj) {
                // last block of a pass without a gate (teacher / complete model): only u[cls] is read downstream (LN2 / MLP / adapter of
                // the cls rows, their backward) -- the proj GEMM runs on the B gathered cls rows; same k order, same bits for those rows
                GemmArgs a; a.A = L.attn_o; a.a_map = c->cls_rows; a.W = W.proj_w; a.M = B; a.N = D; a.K = D; a.bias = W.proj_b;
                a.resid = x; a.out_f32 = L.u; a.scale = 1.0f; a.row_map = c->cls_rows; SPLIT_F(a, W.proj_w3, W.proj_w3b, 1);
                a.row_scale = dp1;
                RUN_GEMM(EPI_AD_UP, a);
            } else {
                GemmArgs a; a.A = L.attn_o; a.W = W.proj_w; a.Wp = W.proj_wp; a.M = M; a.N = D; a.K = D; a.bias = W.proj_b; a.resid = x;
                a.out_f32 = L.u; a.out_at = P == 0 ? nullptr : L.u_at; SPLIT_F(a, W.proj_w3, W.proj_w3b, 1);
                if (save16) { a.out_at = L.u16; a.save16 = true; }
                if (ao3) SPLIT_READY(a, ao3);
                if (fold) a.ln_part = L.ln_part;
                a.row_scale = dp1;
                RUN_GEMM(EPI_BIAS_RESID, a);
            }
            if (l == 0 && ev_b0_record) DYT_HIP_CHECK(hipEventRecord(ev_b0_record, s));
        }
        const bool tail = c->cls_tail && l == depth - 1 && !tokens_out;  // only the cls rows of the last block reach the head
        const int Mr = tail ? B : M;                       // rows the adapter / MLP of this block run on
        if (tail) {  // LN2 of the cls rows + their AT copy (adapter operand); everything below works on B rows
            RUN(2, 0, launch_ln_cls(P, L.u, W.ln2_w, W.ln2_b, T.xn, L.st2, S.ucls_at, B, s));
            if (save16) RUN(2, 0, launch_convert(1, (const float*)S.ucls_at, S.ucls16, (int64_t)B * D, s));
        }
        // ---- adapter branch: x_out = u + scale * up(dropout(relu(down(u)))) -- independent of the
        //      gate / gather / fc1 chain below, so it runs on the pass's side stream until fc2 needs x_out
        // 16-bit modes: wherever the MLP output h is not needed on its own (teacher pass, cls tail, inference) the
        // up-projection is the leading k-tile of the fc2 contraction (x_out = u + [d_act | h1] [s Wup | W2]^T + b): one read
        // of u and one write of x_out per row instead of two fp32 read-modify-write passes, and no up-projection launch.
        // In a compacted pass that covers the kept rows; the dropped rows get their u + adapter(u) from an
        // up-projection launch that skips the kept ones.  In a training student pass the saved MLP output h then includes the
        // adapter; the gate gradient <g, mlp(x)> is recovered in tok_bwd by subtracting <g, adapter(x)>, which the adapter's own
        // backward operands give for 128 B per token (TokBwdArgs::cat_*).  The masked mode keeps the two-launch form.
        const bool need_h = save && !complete && !tail;
        // the adapter's own LayerNorm (dyt_config::adapter_ln; reference models/dynamic_adapter.py:121-122 "in": down_proj reads LN_a(u); :132-133
        // "out": the scaled up-projection output goes through LN_a before it joins the residual stream).  Generic kernels, no fusion with fc2.
        const bool ad_in = c->ad_ln == 1, ad_out = c->ad_ln == 2;
        const float* aln_w = base + c->off_alw; const float* aln_b = base + c->off_alb;
        const bool cat = c->fc2_cat && P != 0 && !masked_dense && !dp2 && !ad_out;   // (a scaled MLP branch cannot share its accumulator with the adapter's)
        // Split fp32 forms whose backward runs on 16-bit operands ("fp16x3h", "fp16f8", "fp16x3q"; round 6): the same fusion with the up-projection as a
        // THREE-part product -- s d_act leaves the down-projection epilogue as a [hi | lo] image, W_up is split once per step (prep_adapters) --
        // contracted by the fc2 kernel as three leading tiles in front of its main loop (gemm.hip: LEAD); the dropped tokens' up-projection launch
        // runs on the same two images.  Until round 5 these modes ran the up-projection on the exact-fp32 MFMA kernel: an fp32
        // read-modify-write of [M,768] per block and pass (47 us) in front of the fc2 epilogue's own.
        const bool cat3 = !ad_out && c->fc2_cat && P == 0 && c->split16 && c->bwd16 && T.dact3 && c->ad_up_w3 && !masked_dense && !dp2;
        L.h_has_adapter = (cat || cat3) && need_h;   // the saved "MLP output" of this block then includes the adapter: tok_bwd corrects <g, h>
        FORK(sb);
        if (ad_in) RUN_ON(sb, 2, 0, launch_adapter_ln_fwd(P, L.u, aln_w, aln_b, T.xa, L.st_a, nullptr, Mr, s));
        {
            GemmArgs a; a.A = ad_in ? (const void*)T.xa : (tail ? S.ucls_at : L.u_at); a.W = at_off(c, c->ad_down_w, (size_t)l * RP * D); a.M = Mr; a.N = RP; a.K = D;
            a.bias = c->ad_down_b + l * RP; a.out_at = L.d_act; a.r = r; a.drop_p = drop_p;
            a.inv_keep = drop_p > 0.f ? 1.0f / (1.0f - drop_p) : 1.0f;
            a.keep = keep_mask ? keep_mask + (size_t)l * M * r : nullptr;
            a.row_map = tail ? c->cls_rows : nullptr;
            a.seed = seed; a.subseq = ((uint64_t)slot << 32) | (uint64_t)(l * 2 + 1); a.seed_dev = seed_dev;
            if (cat) { a.out_at2 = T.dact_s; a.scale = ad_scale; }
            if (save16) { a.out_at2 = L.dact16; a.scale = 1.0f; a.save16 = true; }
            if (cat3) { a.out3 = T.dact3; a.out3_scale = ad_scale; }
            RUN_ON(sb, 0, a.flops(), launch_gemm(P, EPI_AD_DOWN, a, s));
        }
        GemmArgs up; up.A = L.d_act; up.W = at_off(c, c->ad_up_w, (size_t)l * RP * D); up.M = Mr; up.N = D; up.K = RP;
        up.bias = up_bias; up.resid = L.u; up.out_f32 = xo; up.scale = ad_scale;
        up.row_map = tail ? c->cls_rows : nullptr;
        if (ad_out) {   // x_out = u + LN_a(s (d_act W_up^T + b_up)): the LayerNorm's input is kept (its backward needs x_hat), fc2 then adds in place
            GemmArgs g; g.A = L.d_act; g.W = at_off(c, c->ad_up_ws, (size_t)l * RP * D); g.M = Mr; g.N = D; g.K = RP;
            g.bias = c->ad_up_bp + (size_t)l * D; g.out_f32 = L.up32;
            RUN_ON(sb, 0, g.flops(), launch_gemm(P, EPI_BIAS_F32, g, s));
            RUN_ON(sb, 2, 0, launch_adapter_ln_fwd(0, L.up32, aln_w, aln_b, xo, L.st_a, L.u, Mr, s));
        } else if (!cat && !cat3) RUN_ON(sb, 0, up.flops(), launch_gemm(P, EPI_AD_UP, up, s));
        const uint16_t* up_w3 = cat3 ? (const uint16_t*)c->ad_up_w3 + (size_t)l * SPLIT_A * RP * D : nullptr;
        int* counts = S.counts + (size_t)l * B;
        if (use_gate) {
            GateArgs ga;
            ga.u = L.u; ga.w = base + c->off_gw; ga.b = base + c->off_gb;
            ga.g1 = g1 ? g1 + (size_t)l * B * NP : nullptr;
            ga.g2 = g2 ? g2 + (size_t)l * B * NP : nullptr;
            ga.batch = B; ga.training = training; ga.tau = c->cfg.tau; ga.threshold = c->cfg.threshold;
            ga.seed = seed; ga.subseq = ((uint64_t)slot << 32) | (uint64_t)(l * 2); ga.seed_dev = seed_dev;
            ga.soft = L.soft; ga.maskf = L.maskf;
            ga.out_select = token_select ? token_select + (size_t)l * NP : nullptr;
            ga.out_logits = token_logits ? token_logits + (size_t)l * NP : nullptr;
            ga.out_stride = depth * NP;
            ga.keep_local = L.keep_local; ga.counts = counts; ga.force_first = c->count_flops_tokens;
            RUN(2, 0, launch_gate(ga, s));
        }
        const bool fold2 = fold && !tail;   // LN2 inside fc1: (mean, rstd) from the proj epilogue's partials, no normalised copy of u
        if (fold2) {   // (the fc1 GEMM merges the partials itself)
            if (!dense || (masked_dense && save)) RUN(2, 0, launch_gather_index(L.keep_local, counts, L.total, L.maskf, L.row_src, L.dst_of, B, s, T.drop_src));
        } else if (tail) {
            // nothing: T.xn already holds LN2 of the cls rows
        } else if (!dense) {
            RUN(2, 0, launch_ln_gather(P, L.u, W.ln2_w, W.ln2_b, L.keep_local, counts, L.total, L.maskf, T.xn, L.st2,
                                       L.row_src, L.dst_of, B, s, c->split16 ? T.xn3 : nullptr, (fm >> 2) & 1, cat3 ? T.drop_src : nullptr));
        } else {
            RUN(2, 0, launch_ln_fwd(P, L.u, W.ln2_w, W.ln2_b, T.xn, L.st2, M, s, c->split16 ? T.xn3 : nullptr, (fm >> 2) & 1));
            // reference-style (masked) student pass: the MLP runs on every token, but its backward only has rows for the
            // kept ones (dH = mask * g) and is compacted -- it needs the dispatcher's index arrays too
            if (masked_dense && save) RUN(2, 0, launch_gather_index(L.keep_local, counts, L.total, L.maskf, L.row_src, L.dst_of, B, s));
        }
        // MLP on the kept (or all / cls) tokens, scatter-add into the residual stream
        const int* kdev = (dense || tail) ? nullptr : L.total;
        {
            GemmArgs a; a.A = T.xn; a.W = W.fc1_w; a.Wp = W.fc1_wp; a.M = Mr; a.N = DM; a.K = D; a.m_dev = kdev; a.bias = W.fc1_b;
            a.out_at = T.h1; a.out_at2 = save ? L.z : nullptr; SPLIT_F(a, W.fc1_w3, W.fc1_w3b, 2);
            if (save16) { a.out_at2 = L.z16; a.save16 = true; }
            if (!tail) SPLIT_READY(a, T.xn3);   // (the cls tail's LN2 rows come from ln_cls in fp32: pre-pass)
            if (c->split16) { a.out3 = T.h3; a.out3_f8 = (fm >> 3) & 1; }
            if (fold2) {
                a.A = L.u_at; a.a_map = dense ? nullptr : L.row_src; a.W = W.fc1_wf; a.Wp = W.fc1_wfp; a.bias = W.fc1_bf;
                a.ln_part = L.ln_part; a.ln_st_out = L.st2; a.ln_scratch = T.st_compact; a.ln_cs = W.fc1_cs;
            }
            RUN_GEMM(EPI_FC1, a);
        }
        JOIN(sb);  // x_out now holds u + adapter(u) (two-launch form) / d_act is complete
        if ((cat || cat3) && !dense && !tail) {   // dropped tokens: x_out = u + adapter(u) (the kept ones are written by fc2 below)
            if (cat3) {   // three-part on the [hi | lo] images; the operand carries the adapter scale, the bias takes it in the epilogue
                // (round 6b: over the list of dropped rows like the 16-bit modes' launch -- gathered operand rows, scattered output rows -- instead of
                // every row tile with the kept rows masked: 54 -> ~18 us)
                up.W3 = up_w3; up.a3 = T.dact3; up.a3_ready = true; up.scale = 1.0f; up.bias_scale = ad_scale;
                if (T.drop_src) { up.a3_mapped = true; up.a_map = T.drop_src; up.row_map = T.drop_src; up.m_dev = L.total + 1; }
                else up.row_mask = L.maskf;
            } else if (fold2) {   // over the dispatcher's list of dropped rows (gather + scatter) instead of every row with the kept ones skipped
                up.a_map = T.drop_src; up.row_map = T.drop_src; up.m_dev = L.total + 1;
            } else {
                up.row_mask = L.maskf;
            }
            RUN_GEMM(EPI_AD_UP, up);
        }
        {
            GemmArgs a; a.A = T.h1; a.W = W.fc2_w; a.M = Mr; a.N = D; a.K = DM; a.m_dev = kdev; a.bias = W.fc2_b;
            a.out_f32 = xo;
            a.row_map = tail ? c->cls_rows : (dense ? nullptr : L.row_src);
            a.row_mask = (masked_dense && !tail) ? L.maskf : nullptr;   // the cls token is never gated
            a.h_out = need_h ? L.h : nullptr;                           // cls rows carry no gate gradient
            if (save16 && need_h) { a.h_out = L.h16; a.save16 = true; }
            SPLIT_F(a, W.fc2_w3, W.fc2_w3b, 3); SPLIT_READY(a, T.h3);
            if (cat3) {
                a.A2 = T.dact3; a.W2 = up_w3;
                a.a2_map = (dense || tail) ? nullptr : L.row_src;
                a.bias2 = up_bias; a.scale = ad_scale; a.resid = L.u;
            }
            if (cat) {
                a.A2 = T.dact_s; a.W2 = at_off(c, c->ad_up_w, (size_t)l * RP * D);   // [s d_act | h] x [W_up | W2]^T
                a.a2_map = (dense || tail) ? nullptr : L.row_src;   // d_act is indexed by token (cls tail: by image, like h1)
                a.bias2 = up_bias; a.scale = ad_scale; a.resid = L.u;
            }
            a.row_scale = dp2;
            if (tail) { a.splitk_ws = (float*)T.dZ; a.splitk_ws_bytes = (size_t)M * DM * c->at; }   // (a backward-pass buffer: idle here)
            if (tail && c->inf) { a.splitk_ws = T.sk_ws; a.splitk_ws_bytes = (size_t)(DM / 256 + 1) * c->cfg.max_batch * D * sizeof(float); }   // (same decision in run_bf16: either size holds the B-row partials)
            RUN_GEMM(EPI_FC2, a);
        }
        // dyt_forward_taps: the residual stream behind this block, copied while it is there (an inference-only context keeps two streams in turn)
        if (taps && taps[l]) DYT_HIP_CHECK(hipMemcpyAsync(taps[l], xo, (size_t)M * D * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    if (tokens_out) {   // the block stack's output tokens instead of the head: `logits` receives [B,197,768]
        DYT_HIP_CHECK(hipMemcpyAsync(logits, S.xs[depth], (size_t)M * D * sizeof(float), hipMemcpyDeviceToDevice, s));
    } else if (c->frames > 1) {
        int rc = pool_forward(c, S, trainable, logits, B, s);
        if (rc) return rc;
    } else {
        // the head's input row per image and its LayerNorm: the cls row and the frozen final norm, or -- DYT_CREATE_FC_NORM -- the trainable
        // fc_norm of the flat buffer, on -- DYT_CREATE_AVG_POOL -- the mean of the patch rows (reference :375-380)
        const float* hx = S.xs[depth]; size_t hx_stride = (size_t)NT * D;
        if (c->avg_pool) { RUN(2, 0, launch_avg_pool_fwd(S.xs[depth], S.pooled, B, s)); hx = S.pooled; hx_stride = D; }
        const float* hnw = c->fc_norm ? trainable + c->off_fnw : c->norm_w; const float* hnb = c->fc_norm ? trainable + c->off_fnb : c->norm_b;
        if (c->wide_head)
            RUN(2, 0, launch_head_wide_fwd(hx, hx_stride, hnw, hnb, trainable + c->off_hw, trainable + c->off_hb, S.cls_n,
                                           S.head_stats, logits, B, c->cfg.num_classes, s));
        else
            RUN(2, 0, launch_head_fwd(hx, hnw, hnb, trainable + c->off_hw, trainable + c->off_hb, S.cls_n,
                                      S.head_stats, logits, B, c->cfg.num_classes, s, hx_stride));
    }
    c->pass_ran = true;
    S.batch = B; S.flags = flags; S.valid = save && !tokens_in; S.tokens = tokens_out; S.trainable = trainable; S.saved16 = save16;   // (a pass on a caller's residual stream is forward only; images in, tokens out: dyt_backward_tokens)
    return DYT_OK;
}

extern "C" int dyt_forward(dyt_ctx* c, int slot, const float* images, int batch, int flags, const float* trainable,
                           const float* g1, const float* g2, const uint8_t* keep_mask, uint64_t seed, float* logits,
                           float* token_select, float* token_logits, void* stream) {
    if (!c) { set_error("null ctx"); return DYT_ERR_ARG; }
    if (slot >= 0 && slot < c->cfg.slots) {  // a stand-alone pass owns its block-0 buffers
        Slot& S = c->slots[c->inf ? 0 : slot];
        S.L[0].u = S.u0_own; S.L[0].u_at = S.u0_at_own; S.L[0].u16 = S.u0_16_own; S.L[0].ln_part = S.part0_own;
    }
    return forward_impl(c, slot, images, batch, flags, trainable, g1, g2, keep_mask, seed, logits, token_select,
                        token_logits, true, static_cast<hipStream_t>(stream));
}

extern "C" int dyt_forward_taps(dyt_ctx* c, int slot, const float* images, int batch, int flags, const float* trainable,
                                const float* g1, const float* g2, const uint8_t* keep_mask, uint64_t seed, float* tokens,
                                float* const* taps, float* token_select, float* token_logits, void* stream) {
    if (!c) { set_error("null ctx"); return DYT_ERR_ARG; }
    if (!(flags & DYT_F_TOKENS_OUT) || (flags & DYT_F_TOKENS_IN)) {
        set_error("dyt_forward_taps: flags 0x%x -- a pass from images to tokens (DYT_F_TOKENS_OUT without DYT_F_TOKENS_IN)", flags);
        return DYT_ERR_ARG;
    }
    if (c->frames > 1) { set_error("dyt_forward_taps: image model only (frames=%d: the video model pools every frame's tokens inside its head)", c->frames); return DYT_ERR_ARG; }
    if (slot >= 0 && slot < c->cfg.slots) {  // a stand-alone pass owns its block-0 buffers
        Slot& S = c->slots[c->inf ? 0 : slot];
        S.L[0].u = S.u0_own; S.L[0].u_at = S.u0_at_own; S.L[0].u16 = S.u0_16_own; S.L[0].ln_part = S.part0_own;
    }
    return forward_impl(c, slot, images, batch, flags, trainable, g1, g2, keep_mask, seed, tokens, token_select,
                        token_logits, true, static_cast<hipStream_t>(stream), nullptr, nullptr, nullptr, taps);
}
