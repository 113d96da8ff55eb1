// The backward pass: backward_impl, dyt_backward.
#include "ctx.h"

namespace dyt {

// "learnable_scalar": the backward has left G' = dL/dW', gb' = dL/db' of the PRIMED up-projection (W' = s W_up, b' = s b_up) of every block
// in scr (the slot's scratch, flat layout); chain rule into the gradient buffer: dW_up += s G', db_up += s gb', ds += <G', W_up> + <gb', b_up>.
// One workgroup per block, fixed reduction order.
__global__ __launch_bounds__(256) void learn_scale_fixup_kernel(const float* __restrict__ scr, const float* __restrict__ flat, float* __restrict__ grad,
                                                                int64_t layer_stride, int64_t off_uw, int64_t off_ub, int64_t off_sc, int r, int l0) {
    __shared__ float red[256];
    const int l = l0 + blockIdx.x, tid = threadIdx.x;
    const int64_t b = (int64_t)l * layer_stride;
    const float ls = flat[b + off_sc];
    float dot = 0.f;
    for (int i = tid; i < D * r; i += 256) {
        const float g = scr[b + off_uw + i];
        dot = fmaf(g, flat[b + off_uw + i], dot);
        grad[b + off_uw + i] += ls * g;
    }
    for (int i = tid; i < D; i += 256) {
        const float g = scr[b + off_ub + i];
        dot = fmaf(g, flat[b + off_ub + i], dot);
        grad[b + off_ub + i] += ls * g;
    }
    red[tid] = dot;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) grad[b + off_sc] += red[0];
}

}  // namespace dyt

// dlogits [clips, C] -> pooling-head weight gradients (accumulated into grad) and T.g = dL/d x_last [M,768]
static int pool_backward(dyt_ctx* c, Slot& S, const float* tr, const float* dlogits, float* grad, hipStream_t s) {
    const int P = c->prec, t = c->frames, B = S.batch, clips = B / t, M = B * NT, NK = t * NT, C = c->cfg.num_classes;
    const int Mp = (M + 63) / 64 * 64;
    PoolS& Q = S.pool;
    Transients& T = S.T;
    const float gs = P == 0 ? 1.0f : c->gs, inv_gs = 1.0f / gs;   // 16-bit gradient operands carry gs (fp16 build)
    RUN(2, 0, launch_rows_linear_bwd(dlogits, Q.y, tr + c->off_hw, Q.dy, grad + c->off_hw, grad + c->off_hb, clips, C, D, s));
    RUN(2, 0, launch_rows_linear_bwd(Q.dy, Q.o, tr + c->off_pproj_w, Q.dO, grad + c->off_pproj_w, grad + c->off_pproj_b,
                                     clips, D, D, s));
    void* dK = T.dO; void* dV = T.dxn;   // [M,768] AT transients, free until the trunk backward starts
    RUN(1, 8.0 * clips * NH * (double)NK * HD,
        launch_pool_attn_bwd(P, Q.qs, Q.Kp, Q.Vp, Q.P, Q.dO, dK, dV, Q.dq_part, clips, NK, gs, s));
    RUN(2, 0, launch_pool_q_bwd(Q.dq_part, clips, Q.qn, Q.qhat, Q.st_q, tr + c->off_pq_w, tr + c->off_pnq_w, Q.gq, Q.dqn,
                                grad + c->off_pq_w, grad + c->off_pq_bias, grad + c->off_pnq_w, grad + c->off_pnq_b,
                                grad + c->off_pquery, s));
    // weight gradients of k / v: dW = dK^T xk over the token rows -- operands transposed to K-contiguous, NT GEMM.
    // A 768x768 output is only 36 workgroups, so the two GEMMs go to a side stream and run under the trunk's
    // backward (they touch nothing else: their operands are private copies, their outputs own regions of grad).
    RUN(2, 0, launch_transpose_rows(P, dK, Q.dKt, M, Mp, nullptr, s));
    RUN(2, 0, launch_transpose_rows(P, Q.xk, Q.xkt, M, Mp, nullptr, s));
    RUN(2, 0, launch_transpose_rows(P, dV, Q.dVt, M, Mp, T.tok_partial, s));   // + column sums of dV -> v_bias
    RUN(2, 0, launch_transpose_rows(P, Q.xv, Q.xvt, M, Mp, nullptr, s));
    RUN(2, 0, launch_reduce_partials(T.tok_partial, Mp / 64, D, grad + c->off_pv_bias, D, inv_gs, s));
    hipStream_t ws = nullptr;
    if (c->overlap && !c->prof && !S.no_branch) {   // (no_branch: a captured teacher pass -- a fork of the side stream crashes hipStreamEndCapture, see dyt_step_fwd_bwd)
        if (!Q.wstream) {
            DYT_HIP_CHECK(hipStreamCreateWithFlags(&Q.wstream, hipStreamNonBlocking));
            DYT_HIP_CHECK(hipEventCreateWithFlags(&Q.ev_wf, hipEventDisableTiming));
            DYT_HIP_CHECK(hipEventCreateWithFlags(&Q.ev_wj, hipEventDisableTiming));
        }
        ws = Q.wstream;
        DYT_HIP_CHECK(hipEventRecord(Q.ev_wf, s));
        DYT_HIP_CHECK(hipStreamWaitEvent(ws, Q.ev_wf, 0));
    }
    {
        GemmArgs a; a.A = Q.dKt; a.W = Q.xkt; a.M = D; a.N = D; a.K = Mp; a.out_f32 = grad + c->off_pk_w; a.accumulate = 1; a.scale = inv_gs;
        RUN_ON(ws, 0, a.flops(), launch_gemm(P, EPI_STORE_F32, a, s));
    }
    {
        GemmArgs a; a.A = Q.dVt; a.W = Q.xvt; a.M = D; a.N = D; a.K = Mp; a.out_f32 = grad + c->off_pv_w; a.accumulate = 1; a.scale = inv_gs;
        RUN_ON(ws, 0, a.flops(), launch_gemm(P, EPI_STORE_F32, a, s));
    }
    if (ws) { DYT_HIP_CHECK(hipEventRecord(Q.ev_wj, ws)); Q.wpending = true; }   // joined at the end of backward_impl
    // dgrads through k / v, then norm_k + norm_v + final norm backward in one row pass
    {
        GemmArgs a; a.A = dK; a.W = c->pk_wT; a.M = M; a.N = D; a.K = D; a.out_at = T.du_at;
        RUN_GEMM(EPI_STORE_AT, a);
    }
    {
        GemmArgs a; a.A = dV; a.W = c->pv_wT; a.M = M; a.N = D; a.K = D; a.out_at = T.dA2;
        RUN_GEMM(EPI_STORE_AT, a);
    }
    int nblk = 0;
    RUN(2, 0, launch_pool_ln_bwd(P, T.du_at, T.dA2, Q.xf, Q.st_kv, tr + c->off_pnk_w, tr + c->off_pnv_w, S.xs[c->cfg.depth],
                                 Q.st_f, c->norm_w, T.g, T.wg_partial, M, &nblk, gs, s));
    RUN(2, 0, launch_reduce_partials(T.wg_partial, nblk, 4 * D, grad + c->off_pnk_w, 4 * D, 1.0f, s));
    return 0;
}

// ev_split (optional) is recorded on `s` once the gradients of the head and of every block >= split are enqueued
int dyt::backward_impl(dyt_ctx* c, int slot, const float* trainable, const float* dlogits, const float* dtoken_select,
                       const float* dtok, const float* dtoken_logits, float* grad, hipStream_t s,
                       hipEvent_t ev_split, int split, const TokenGrads* tg) {
    { int rc = refuse_inference(c, "the backward pass"); if (rc) return rc; }
    if (slot < 0 || slot >= c->cfg.slots) { set_error("slot %d out of range", slot); return DYT_ERR_ARG; }
    Slot& S = c->slots[slot];
    Transients& T = S.T;
    if (!S.valid) { set_error("slot %d holds no saved forward (call dyt_forward with DYT_F_SAVE)", slot); return DYT_ERR_STATE; }
    // a slot serves the entry point of its own kind of pass
    if (S.tokens && !tg) {
        set_error("slot %d holds a token-level pass (dyt_forward_taps / DYT_F_TOKENS_OUT): its backward is dyt_backward_tokens, not dyt_backward", slot);
        return DYT_ERR_STATE;
    }
    if (!S.tokens && tg) {
        set_error("slot %d holds a pass that ran the head (dyt_forward without DYT_F_TOKENS_OUT): its backward is dyt_backward, not dyt_backward_tokens "
                  "(save a token-level pass with dyt_forward_taps and DYT_F_SAVE)", slot);
        return DYT_ERR_STATE;
    }
    if ((!dlogits && !tg) || !grad || !trainable) { set_error("null argument"); return DYT_ERR_ARG; }
    // b16 ("fp16x3h"): the saved pass came from the exact (split fp32) forward, this backward runs in the 16-bit mode: P = 1, the
    // 16-bit copies of the saved tensors and of the dgrad matrices, none of the split forms below
    const bool b16 = S.saved16;
    const int P = b16 ? 1 : c->prec, depth = c->cfg.depth, B = S.batch, M = B * NT, r = c->cfg.ffn_num;
    const bool split16 = c->split16 && !b16;
    const size_t atb = at_size(P);
    auto at_offb = [atb](void* base, size_t elems) { return static_cast<void*>(static_cast<char*>(base) + elems * atb); };
    const int flags = S.flags;
    const bool training = flags & DYT_F_TRAINING, complete = flags & DYT_F_COMPLETE;
    // masked_dense: the student forward evaluated the MLP for every token and multiplied by the mask (the reference's
    // training semantics: h and gelu' exist for all tokens, indexed by token row).  Its BACKWARD is compacted all the same:
    // the rows of dH = mask * g that belong to dropped tokens are exactly zero, so dZ / dA2 are computed for the kept rows
    // only (gathered through row_src) -- "exact-gradient" mode at 133.5 instead of 139.6 GFLOP per image.
    const bool masked_dense = (flags & DYT_F_MASKED_DENSE) && !complete;
    const bool dense = complete;               // MLP backward over all rows (teacher pass)
    const bool h_by_token = masked_dense;      // saved h / gelu' are indexed by token row, not by compact row
    const bool student = !complete;
    const float drop_p = training ? c->cfg.adapter_dropout : 0.f;
    const float inv_keep = drop_p > 0.f ? 1.0f / (1.0f - drop_p) : 1.0f;
    const float scale = c->learn_scale ? 1.0f : c->cfg.adapter_scale;   // (learnable: the dgrad matrices carry it, the weight gradients get it in learn_scale_fixup_kernel)
    if (c->learn_scale) DYT_HIP_CHECK(hipMemsetAsync(S.gscr, 0, (size_t)depth * c->layer_stride * sizeof(float), s));
    const float gs = P == 0 ? 1.0f : c->gs, inv_gs = 1.0f / gs;   // 16-bit gradient operands carry gs (dyt_ctx: gs)
    float* g = T.g;
    // ... in the split modes' 16-bit backward as well (fp16x3q: 35.2 -> 34.5 ms per step same-box; worst gradient over the five seeds 1.40e-3 -> 1.53e-3, typical
    // 7e-4 -> 1.1e-3: tests/test_gpu_round4.py prints the table); DYT_G16_B16=0 keeps the fp32 stream there
    static const bool g16_b16 = !(getenv("DYT_G16_B16") && atoi(getenv("DYT_G16_B16")) == 0);
    const bool g16 = c->g16 && P == 1 && (!b16 || g16_b16);   // the gradient stream between the row kernels as 16-bit operand copies only (dyt_ctx::g16)
    hipStream_t sb = nullptr;
    { int rc = branch_stream(c, S, &sb); if (rc) return rc; }

    const bool cls_tail = c->cls_tail && !tg;   // a token-level pass computed and saved every row of the last block: it is a block like the others
    const float* const* dtaps = tg ? tg->dtaps : nullptr;
    if (tg) {
        // top of the stack: g = LNbwd_final(dtokens) + dtaps[depth-1], in fp32 whatever the mode (the un-fused bwd_prep below then makes g_at / dmask,
        // as behind head_bwd).  The frozen final norm has no parameter gradient; its statistics over all rows are recomputed (no pass keeps them).
        // With DYT_CREATE_FC_NORM the final norm is an identity: g = dtokens + dtaps[depth-1].
        const float* top = dtaps ? dtaps[depth - 1] : nullptr;
        if (tg->dtokens && !c->fc_norm) {
            float2* st = reinterpret_cast<float2*>(T.delta);   // [M] of the [B,12,197] floats the first attention backward writes later
            RUN(2, 0, launch_ln_stats(S.xs[depth], st, M, s));
            RUN(2, 0, launch_ln_bwd(0, tg->dtokens, S.xs[depth], st, c->norm_w, top, g, M, nullptr, nullptr, nullptr, nullptr, 1.0f, s));
        } else if (tg->dtokens || top) {
            RUN(2, 0, launch_rows_add(tg->dtokens ? tg->dtokens : top, tg->dtokens ? top : nullptr, g, M, s));
        } else {
            DYT_HIP_CHECK(hipMemsetAsync(g, 0, (size_t)M * D * sizeof(float), s));
        }
        { const int l = depth; CK("tokens_top g", g, (size_t)M * D * 4); }
    } else if (c->frames > 1) {
        int rc = pool_backward(c, S, trainable, dlogits, grad, s);
        if (rc) return rc;
    } else {
        // (the head's input rows and LayerNorm as in forward_impl; under DYT_CREATE_AVG_POOL the head leaves dpooled in its compact form
        // and avg_pool_bwd is the one writer of the gradient stream)
        const float* hx = c->avg_pool ? S.pooled : S.xs[depth]; const size_t hx_stride = c->avg_pool ? (size_t)D : (size_t)NT * D;
        const float* hnw = c->fc_norm ? trainable + c->off_fnw : c->norm_w;
        const bool compact = cls_tail || c->avg_pool;
        if (c->wide_head)
            RUN(2, 0, launch_head_wide_bwd(dlogits, hx, hx_stride, S.cls_n, S.head_stats, hnw, trainable + c->off_hw,
                                           compact ? S.gcls : g, grad + c->off_hw, grad + c->off_hb, B, c->cfg.num_classes,
                                           compact ? 1 : 0, S.head_part, s, S.head_dy));
        else
        RUN(2, 0, launch_head_bwd(dlogits, hx, S.cls_n, S.head_stats, hnw, trainable + c->off_hw,
                                  compact ? S.gcls : g, grad + c->off_hw, grad + c->off_hb, B, c->cfg.num_classes,
                                  compact ? 1 : 0, s, hx_stride, S.head_dy));
        if (c->fc_norm) RUN(2, 0, launch_fc_norm_param_grad(S.head_dy, hx, hx_stride, S.head_stats, grad + c->off_fnw, grad + c->off_fnb, B, s));
        if (c->avg_pool) RUN(2, 0, launch_avg_pool_bwd(S.gcls, g, B, s));
        { const int l = depth; CK("head_bwd g", cls_tail ? S.gcls : g, (size_t)(cls_tail ? B : M) * D * 4); CK("head_bwd dW", grad + c->off_hw, (size_t)c->cfg.num_classes * D * 4); }
    }

    int fix_hi = depth;   // learnable scale: blocks [0, fix_hi) still await learn_scale_fixup_kernel
    ReduceQueue rq;   // adapter weight-gradient / gate-gradient reductions: queued per block, flushed where the gradients must be final
    bool prepped = false;  // the previous iteration's ln_bwd already produced g_at / dmask for this block
    bool g3_ready = false; // ... and (fp32 split form) T.g3 = g as the 16-bit split operand of this block's GELU' dgrad
    const bool split_prod = split16;   // ln_bwd / tok_bwd write the split operand of the GEMM that follows
    for (int l = depth - 1; l >= 0; --l) {
        const LayerW& W = c->W[l];
        LayerS& L = S.L[l];
        const float* base = trainable + (int64_t)l * c->layer_stride;
        float* gbase = grad + (int64_t)l * c->layer_stride;
        float* ubase = c->learn_scale ? S.gscr + (int64_t)l * c->layer_stride : gbase;   // where the up-projection's weight / bias gradients go
        const bool first = l == 0;
        // saved tensors / dgrad matrices in this backward's operand type
        const void* Lh = b16 ? L.h16 : L.h; const void* Ldact = b16 ? L.dact16 : L.d_act; const void* Lz = b16 ? L.z16 : L.z;
        const void* Luat = b16 ? L.u16 : L.u_at; const void* ucls = b16 ? S.ucls16 : S.ucls_at;
        const void *fc2_wT = b16 ? W.fc2_wT16 : W.fc2_wT, *fc2_wTp = b16 ? W.fc2_wTp16 : W.fc2_wTp, *fc1_wT = b16 ? W.fc1_wT16 : W.fc1_wT,
                   *fc1_wTp = b16 ? W.fc1_wTp16 : W.fc1_wTp, *proj_wT = b16 ? W.proj_wT16 : W.proj_wT, *proj_wTp = b16 ? W.proj_wTp16 : W.proj_wTp,
                   *qkv_wT = b16 ? W.qkv_wT16 : W.qkv_wT, *qkv_wTp = b16 ? W.qkv_wTp16 : W.qkv_wTp;
        void* ad_up_wT = b16 ? c->ad_up_wT16 : c->ad_up_wT; void* ad_down_wT = b16 ? c->ad_down_wT16 : c->ad_down_wT;
        void* Tdad = b16 ? T.dad16 : T.dad;
        // 16-bit backward: ad_up_wT carries 2^e (adapter_lift_kernel), so ddz carries gs 2^e; its consumers multiply by this 2^-e
        const float* ddz_unlift = P != 0 ? c->ad_lift + depth + l : nullptr;

        const bool tail = cls_tail && l == depth - 1;  // incoming gradient lives at the cls rows only (S.gcls)
        const int Mr = tail ? B : M;
        float* gin = tail ? S.gcls : g;
        // ---- 1. prep: AT copy of g, gathered/masked MLP gradient rows, <g,h> per token ----
        void* g_at = P == 0 ? nullptr : T.g_at;
        if (!prepped && (g_at || (student && !tail))) {
            BwdPrepArgs a;
            a.g = gin; a.h = (student && !tail) ? Lh : nullptr; a.dst_of = (dense || tail || h_by_token) ? nullptr : L.dst_of;
            a.row_mask = nullptr;
            a.g_at = g_at; a.dH = nullptr; a.dmask = (student && !tail) ? T.dmask : nullptr;
            a.M = Mr; a.gs = gs;
            ISO(64, RUN(2, 0, launch_bwd_prep(P, a, s)););
            if (g_at) CK("bwd_prep g_at", g_at, (size_t)Mr * D * atb);
            if (a.dmask) CK("bwd_prep dmask", T.dmask, (size_t)Mr * 4);
        }
        const void* A_g = g_at ? g_at : (const void*)gin;
        const int* kdev = (dense || tail) ? nullptr : L.total;
        // the adapter's own LayerNorm (dyt_config::adapter_ln).  "out": the adapter branch sees the gradient BEHIND the LayerNorm -- its parameter
        // gradients (dy = g, x_hat from the saved input) and dup = LNbwd(g), which replaces g as the operand of the up-projection's dgrad / wgrad.
        const bool ad_in = c->ad_ln == 1, ad_out = c->ad_ln == 2;
        const void* A_ad = A_g;
        if (ad_out) {
            RUN(2, 0, launch_ln_param_grad(P, A_g, L.up32, L.st_a, T.aln_part, gbase + c->off_alw, Mr, gs, s));
            RUN(2, 0, launch_ln_bwd(P, A_g, L.up32, L.st_a, base + c->off_alw, nullptr, P == 0 ? T.dup : nullptr, Mr, P != 0 ? (void*)T.dup : nullptr,
                                    nullptr, nullptr, nullptr, gs, s));
            A_ad = T.dup;
        }
        if (ad_in) RUN(2, 0, launch_adapter_ln_fwd(P, L.u, base + c->off_alw, base + c->off_alb, T.xa, nullptr, nullptr, Mr, s));   // down_proj's wgrad operand LN_a(u), recomputed
        // ---- 2. adapter branch on the side stream: dgrad through up_proj, both wgrads, bias grads ----
        FORK(sb);
        {
            GemmArgs a; a.A = A_ad; a.W = at_offb(ad_up_wT, (size_t)l * RP * D); a.M = Mr; a.N = RP; a.K = D;
            a.aux_at = Ldact; a.out_at = T.ddz; a.scale = scale; a.inv_keep = inv_keep;
            POISON(64, T.ddz, (size_t)Mr * RP * atb);
            ISO(16, RUN_ON(sb, 0, a.flops(), launch_gemm(P, EPI_AD_DGRAD_UP, a, s)););
            CK("ad_dgrad_up ddz", T.ddz, (size_t)Mr * RP * atb);
        }
        {   // both weight gradients (+ the two bias gradients as ones columns / rows) in one launch
            WgradArgs w[2];
            WgradArgs& a = w[0];
            a.X = A_ad; a.Y = Ldact; a.M = Mr; a.r = r; a.partial = S.wg_part[l];
            a.out_w = ubase + c->off_uw; a.sc = r; a.sj = 1; a.alpha = scale * inv_gs;       // up_proj.weight [768, r]  (X = g_at carries gs)
            a.out_xsum = ubase + c->off_ub; a.alpha_x = scale * inv_gs;                      // up_proj.bias
            WgradArgs& b = w[1];
            b.X = ad_in ? (const void*)T.xa : (tail ? ucls : Luat); b.Y = T.ddz; b.M = Mr; b.r = r; b.partial = S.wg_part2[l];
            b.out_w = gbase + c->off_dw; b.sc = 1; b.sj = D; b.alpha = inv_gs;      // down_proj.weight [r, 768]  (Y = ddz carries gs)
            b.out_xsum = nullptr; b.alpha_x = 0.f;
            b.out_ysum = gbase + c->off_db; b.alpha_y = inv_gs;                     // down_proj.bias
            b.alpha_dev = ddz_unlift;
            if (split16 && c->split_bwd_parts == 1) {   // "fp16x3f": gradient products one-part here too
                a.half_products = b.half_products = true;
                a.x_scale = c->split_gs;   // X = g (gradient-sized), Y = d_act
                b.y_scale = c->split_gs;   // X = u, Y = ddz (gradient-sized)
            }
            ISO(32, RUN_ON(sb, 2, 4.0 * Mr * D * (double)RP, launch_wgrad(P, w, 2, s, sb ? nullptr : &rq)););
            CK("wgrad up_w", gbase + c->off_uw, (size_t)D * r * 4); CK("wgrad down_w", gbase + c->off_dw, (size_t)D * r * 4);
        }
        // ---- 3. MLP dgrad (frozen weights) on the main stream: dZ = (dH W2) * gelu'(z) ; dA2 = dZ W1 ----
        if (!first) {
            {
                GemmArgs a; a.A = A_g; a.W = fc2_wT; a.Wp = fc2_wTp; a.M = Mr; a.N = DM; a.K = D; a.m_dev = kdev; a.aux_at = Lz;
                a.a_map = (dense || tail) ? nullptr : L.row_src; a.out_at = T.dZ;   // kept rows of g (mask = 1 there) gathered by the loader
                a.row_map = (h_by_token && !tail) ? L.row_src : nullptr; if (split16) SPLIT_G(a, W.fc2_wT3);
                if (g3_ready && !tail) { SPLIT_READY(a, T.g3); a.a3_mapped = true; }   // ln_bwd of the block above wrote g as the split operand
                if (split16) { a.out3 = T.h3; a.out3_scale = c->split_gs; a.out3_hi_only = c->split_bwd_parts == 1; }   // dZ as the split operand of the fc1 dgrad
                if (dense) POISON(128, T.dZ, (size_t)Mr * DM * atb);
                ISO(8, RUN_GEMM(EPI_GELU_BWD, a););
                CK("gelu_bwd dZ", T.dZ, (size_t)Mr * DM * atb);
            }
            {
                GemmArgs a; a.A = T.dZ; a.W = fc1_wT; a.Wp = fc1_wTp; a.M = Mr; a.N = D; a.K = DM; a.m_dev = kdev; a.out_at = T.dA2; if (split16) { SPLIT_G(a, W.fc1_wT3); SPLIT_READY(a, T.h3); }
                if (tail) { a.splitk_ws = (float*)T.dqkv; a.splitk_ws_bytes = (size_t)M * 3 * D * atb; }   // (written by this block's attention backward, later)
                if (dense) POISON(2, T.dA2, (size_t)Mr * D * atb);
                ISO(8, RUN_GEMM(EPI_STORE_AT, a););
                CK("fc1_dgrad dA2", T.dA2, (size_t)Mr * D * atb);
            }
        }
        JOIN(sb);
        // adapter dgrad ddz Wdown.  fp32 mode / cls tail: accumulated into g in place (fp32 read-modify-write of [M,768]);
        // bf16 mode: stored as a bf16 [M,768] operand that tok_bwd adds (half the bytes of the in-place update)
        const bool dad_at = P != 0 && !tail && !first;
        if (ad_in) {
            // "in": ddz W_down is the gradient w.r.t. LN_a(u): the LayerNorm's parameter gradients from it (block 0 included), then its input gradient --
            // 16-bit backward: a 16-bit operand tok_bwd adds (T.dup); fp32 backward: accumulated into g
            GemmArgs a; a.A = T.ddz; a.W = at_offb(ad_down_wT, (size_t)l * RP * D); a.M = Mr; a.N = D; a.K = RP; a.out_dscale = ddz_unlift;
            if (P != 0) { a.out_at = Tdad; ISO(16, RUN_GEMM(EPI_STORE_AT, a);); }
            else { a.out_f32 = T.dup; a.accumulate = 0; a.scale = 1.0f; ISO(16, RUN_GEMM(EPI_STORE_F32, a);); }
            const void* dln = P != 0 ? (const void*)Tdad : (const void*)T.dup;
            RUN(2, 0, launch_ln_param_grad(P, dln, L.u, L.st_a, T.aln_part, gbase + c->off_alw, Mr, gs, s));
            if (!first) {
                if (P != 0) RUN(2, 0, launch_ln_bwd(P, dln, L.u, L.st_a, base + c->off_alw, nullptr, nullptr, Mr, T.dup, nullptr, nullptr, nullptr, gs, s));
                else RUN(2, 0, launch_ln_bwd(P, dln, L.u, L.st_a, base + c->off_alw, gin, gin, Mr, nullptr, nullptr, nullptr, nullptr, gs, s));
            }
        } else if (!first) {
            GemmArgs a; a.A = T.ddz; a.W = at_offb(ad_down_wT, (size_t)l * RP * D); a.M = Mr; a.N = D; a.K = RP; a.out_dscale = ddz_unlift;
            if (dad_at) { a.out_at = Tdad; POISON(4, Tdad, (size_t)Mr * D * atb); ISO(16, RUN_GEMM(EPI_STORE_AT, a);); }
            else { a.out_f32 = gin; a.accumulate = 1; a.scale = inv_gs; ISO(16, RUN_GEMM(EPI_STORE_F32, a);); }
            if (dad_at) CK("ad_dgrad_down dad", Tdad, (size_t)Mr * D * atb);   // g <- g + ddz Wdown
        }

        // ---- 4. per-token tail: LN2 backward scattered back, gate backward, AT copy of dL/du ----
        if (!first || student) {
            TokBwdArgs a;
            a.du = g; a.dA2 = first ? nullptr : T.dA2;
            a.dst_of = (dense || tail) ? nullptr : L.dst_of; a.u = L.u; a.stats2 = L.st2;
            if (g16 && !first) { a.du = nullptr; a.du_in_at = tail ? nullptr : T.g_at; }   // in: ln_bwd's (or bwd_prep's) 16-bit copy; out: du_at only
            a.ln2_w = W.ln2_w; a.gate_w = student ? base + c->off_gw : nullptr; a.soft = L.soft; a.maskf = L.maskf;
            a.dmask = tail ? nullptr : T.dmask;
            a.g_cls = tail ? S.gcls : nullptr;
            a.dad = dad_at ? (ad_in ? (void*)T.dup : Tdad) : nullptr;
            a.gs = gs; a.inv_gs = inv_gs;
            if (L.h_has_adapter && student && !tail) {
                a.cat_dact = Ldact; a.cat_ddz = T.ddz; a.cat_bup = base + c->off_ub;
                a.cat_scale = scale; a.cat_ddz_scale = 1.0f / (inv_keep * gs); a.cat_ddz_dscale = ddz_unlift;
            }
            a.dtoken_select = dtoken_select ? dtoken_select + (size_t)l * NP : nullptr;
            a.dtoken_logits = dtoken_logits ? dtoken_logits + (size_t)l * NP : nullptr;
            a.dtok = dtok; a.out_stride = depth * NP; a.training = training; a.tau = c->cfg.tau;
            a.du_at = (P != 0 && !first) ? T.du_at : nullptr; a.partial = S.tok_part[l]; a.M = M; a.write_du = !first;
            a.branch_scale = (S.dp && l > 0) ? S.dp + (size_t)(depth + l) * B : nullptr;
            if (split_prod && !first) { a.du3 = T.g3; a.du3_scale = c->split_gs; a.du3_hi_only = c->split_bwd_parts == 1; }
            int nblk = 0;
            if (a.du_at) POISON(8, T.du_at, (size_t)M * D * atb);
            ISO(2, RUN(2, 0, launch_tok_bwd(P, a, &nblk, s)););
            if (student && !dbg_skip(8)) { int _r = queue_tok_reduce(rq, S.tok_part[l], nblk, gbase + c->off_gw); if (_r) return _r; }
            if (a.write_du && a.du) CK("tok_bwd g", g, (size_t)M * D * 4);
            if (a.dmask) CK("tok_in dmask", T.dmask, (size_t)M * 4);          // what tok_bwd consumed (unchanged by it)
            if (a.dA2) CK("tok_in dA2", T.dA2, (size_t)Mr * D * atb);
            if (a.dad) CK("tok_in dad", Tdad, (size_t)Mr * D * atb);
            if (a.du_at) CK("tok_bwd du_at", T.du_at, (size_t)M * D * atb);
            if (student) CK("tok_bwd gate grad", gbase + c->off_gw, (size_t)(D + 1) * 4);
        }
        if (l == split || first || dbg_ck_on()) RUN(2, 0, flush_reductions(rq, s));   // the gradients of blocks >= l are final after this
        if (c->learn_scale && ev_split && l == split && l > 0) {   // the upper blocks' up-projection / scale gradients must be final before the event as well
            hipLaunchKernelGGL(learn_scale_fixup_kernel, dim3(fix_hi - l), dim3(256), 0, s, S.gscr, trainable, grad, c->layer_stride, c->off_uw, c->off_ub, c->off_sc, r, l);
            DYT_HIP_CHECK(hipGetLastError());
            fix_hi = l;
        }
        if (ev_split && l == split) {
            // video model: the pooling head's k / v weight gradients (side stream, part 0 of the flat buffer) must be final
            // before the "upper gradients are final" event that the gradient sum and the early all-reduce wait for
            if (S.pool.wpending) { DYT_HIP_CHECK(hipStreamWaitEvent(s, S.pool.ev_wj, 0)); S.pool.wpending = false; }
            DYT_HIP_CHECK(hipEventRecord(ev_split, s));
        }
        if (first) break;
        // ---- 5. attention branch: proj dgrad, attention backward, qkv dgrad, LN1 backward ----
        {
            GemmArgs a; a.A = P == 0 ? (const void*)g : (const void*)T.du_at; a.W = proj_wT; a.Wp = proj_wTp; a.M = M; a.N = D; a.K = D;
            a.out_at = T.dO; if (split16) SPLIT_G(a, W.proj_wT3); if (split_prod) SPLIT_READY(a, T.g3);
            POISON(16, T.dO, (size_t)M * D * atb);
            ISO(8, RUN_GEMM(EPI_STORE_AT, a););
            if (S.dp) RUN(2, 0, launch_scale_rows(P, T.dO, S.dp + (size_t)l * B, M, D, s));   // stochastic depth: the attention branch's factor
            CK("proj_dgrad dO", T.dO, (size_t)M * D * atb);
        }
        POISON(32, T.dqkv, (size_t)M * 3 * D * atb);
        {
            AttnBwdArgs a; a.batch = B; a.q = b16 ? L.q16 : L.q; a.k = b16 ? L.k16 : L.k; a.v = b16 ? L.v16 : L.v;
            a.out = b16 ? L.ao3 : L.attn_o; a.out_ld = b16 ? SPLIT_A * D : 0;   // bwd16: the hi plane of the proj GEMM's operand image
            a.dout = T.dO; a.lse = L.lse; a.delta = T.delta; a.dqkv = T.dqkv;
            a.q_tiles = (tail && !student) ? 1 : 7;   // teacher tail: du, hence dO, is zero off the cls rows
            a.dqkv3 = split16 ? T.dqkv3 : nullptr; a.s3 = c->split_gs; a.out_hi_only = c->split_bwd_parts == 1;
            a.split16 = split16 && c->split_attn; a.grad_parts = c->split_bwd_attn_parts;
            ISO(1, RUN(1, 14.0 * B * NH * (double)NT * NT * HD, launch_attn_bwd(P, a, s)););
        }
        CK("attn_bwd delta", T.delta, (size_t)B * NH * NT * 4); CK("attn_bwd dqkv", T.dqkv, (size_t)M * 3 * D * atb);
        {
            GemmArgs a; a.A = T.dqkv; a.W = qkv_wT; a.Wp = qkv_wTp; a.M = M; a.N = D; a.K = 3 * D; a.out_at = T.dxn; if (split16) { SPLIT_G(a, W.qkv_wT3); SPLIT_READY(a, T.dqkv3); }
            POISON(1, T.dxn, (size_t)M * D * atb);
            ISO(8, RUN_GEMM(EPI_STORE_AT, a););
            CK("qkv_dgrad dxn", T.dxn, (size_t)M * D * atb);
        }
        {   // LN1 backward, fused with the next block's prep (AT copy of g, <g, h> for the gate gradient)
            const LayerS& Ln = S.L[l - 1];
            if (g_at) POISON(256, g_at, (size_t)M * D * atb);
            ISO(4, RUN(2, 0, launch_ln_bwd(P, T.dxn, S.xs[l], L.st1, W.ln1_w, g16 ? nullptr : g, g16 ? nullptr : g, M, g_at, student ? (b16 ? Ln.h16 : Ln.h) : nullptr,
                                    (!dense && !h_by_token) ? Ln.dst_of : nullptr, student ? T.dmask : nullptr, gs, s,
                                    (split_prod && l > 1) ? T.g3 : nullptr, c->split_gs, c->split_bwd_parts == 1, g16 ? T.du_at : nullptr,
                                    dtaps ? dtaps[l - 1] : nullptr)););   // xs[l] is taps[l - 1]: its gradient joins the stream inside this kernel
            g3_ready = split_prod && l > 1;
            if (!g16) CK("ln_bwd g", g, (size_t)M * D * 4);
            if (g_at) CK("ln_bwd g_at", g_at, (size_t)M * D * atb);
            if (student) CK("ln_bwd dmask", T.dmask, (size_t)M * 4);
            prepped = true;
        }
    }
    if (S.pool.wpending) { DYT_HIP_CHECK(hipStreamWaitEvent(s, S.pool.ev_wj, 0)); S.pool.wpending = false; }
    if (c->learn_scale && fix_hi > 0) {
        hipLaunchKernelGGL(learn_scale_fixup_kernel, dim3(fix_hi), dim3(256), 0, s, S.gscr, trainable, grad, c->layer_stride, c->off_uw, c->off_ub, c->off_sc, r, 0);
        DYT_HIP_CHECK(hipGetLastError());
    }
    return DYT_OK;
}

extern "C" int dyt_backward(dyt_ctx* c, int slot, const float* dlogits, const float* dtoken_select, const float* dtok,
                            const float* dtoken_logits, float* grad_flat, void* stream) {
    if (!c) { set_error("null ctx"); return DYT_ERR_ARG; }
    { int rc = refuse_inference(c, "dyt_backward"); if (rc) return rc; }
    if (slot < 0 || slot >= c->cfg.slots) { set_error("slot %d out of range", slot); return DYT_ERR_ARG; }
    return backward_impl(c, slot, c->slots[slot].trainable, dlogits, dtoken_select, dtok, dtoken_logits, grad_flat,
                         static_cast<hipStream_t>(stream));
}

extern "C" int dyt_backward_tokens(dyt_ctx* c, int slot, const float* dtokens, const float* const* dtaps, const float* dtoken_select,
                                   const float* dtok, const float* dtoken_logits, float* grad_flat, void* stream) {
    if (!c) { set_error("null ctx"); return DYT_ERR_ARG; }
    { int rc = refuse_inference(c, "dyt_backward_tokens"); if (rc) return rc; }
    if (c->frames > 1) {
        set_error("dyt_backward_tokens: image model only (frames=%d: the video model trains through its attentive pooling head, dyt_backward)", c->frames);
        return DYT_ERR_ARG;
    }
    if (slot < 0 || slot >= c->cfg.slots) { set_error("slot %d out of range", slot); return DYT_ERR_ARG; }
    bool any = dtokens || dtoken_select || dtok || dtoken_logits;
    for (int i = 0; dtaps && i < c->cfg.depth; ++i) any = any || dtaps[i];
    if (!any) { set_error("dyt_backward_tokens: every gradient input is NULL (dtokens, dtaps[0..%d], dtoken_select, dtok_uniform, dtoken_logits)", c->cfg.depth - 1); return DYT_ERR_ARG; }
    TokenGrads tg; tg.dtokens = dtokens; tg.dtaps = dtaps;
    return backward_impl(c, slot, c->slots[slot].trainable, nullptr, dtoken_select, dtok, dtoken_logits, grad_flat,
                         static_cast<hipStream_t>(stream), nullptr, 0, &tg);
}
