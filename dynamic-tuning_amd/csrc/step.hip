// Loss, AdamW and the fused step with its two-stream schedule; gradient hand-over, all-reduce and clipping.
#include "ctx.h"

// dyt_loss; mix_rows (dyt_step_fwd_bwd with mix on): the class-probability rows mix_targets_kernel wrote on this stream, read instead of
// the caller-set soft targets or the labels
static int loss_impl(dyt_ctx* c, int slot_student, const float* logits_s, const float* logits_t, const int64_t* targets,
                     int batch, float token_target_ratio, float token_loss_ratio, float token_minimal,
                     float token_minimal_weight, float* dlogits_s, float* dlogits_t, float* out_losses, float* dtok,
                     void* stream, const float* mix_rows) {
    if (!c || !logits_s || !logits_t || !targets || !dlogits_s || !dlogits_t || !out_losses || !dtok) {
        set_error("null argument");
        return DYT_ERR_ARG;
    }
    if (slot_student < 0 || slot_student >= c->cfg.slots) { set_error("slot out of range"); return DYT_ERR_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    LossArgs a;
    a.logits_s = logits_s; a.logits_t = logits_t; a.targets = targets; a.counts = c->slots[c->inf ? 0 : slot_student].counts;
    a.batch = batch; a.C = c->cfg.num_classes; a.depth = c->cfg.depth;
    a.count_batch = batch * c->frames;   // video: `batch` clips, the gates were evaluated on batch * t frames
    a.target_ratio = token_target_ratio; a.loss_ratio = token_loss_ratio; a.token_minimal = token_minimal;
    a.token_minimal_weight = token_minimal_weight;
    a.dlogits_s = dlogits_s; a.dlogits_t = dlogits_t; a.out_losses = out_losses; a.dtok = dtok;
    a.scratch = c->loss_part;
    if (batch * c->frames > c->cfg.max_batch) { set_error("batch %d exceeds max_batch", batch); return DYT_ERR_ARG; }
    if (mix_rows) {
        a.soft = mix_rows;
    } else if (c->soft_targets) {
        if (c->soft_batch != batch) { set_error("soft targets were set for %d rows, this loss has %d", c->soft_batch, batch); return DYT_ERR_STATE; }
        a.soft = c->soft_targets;
    }
    return launch_loss(a, s);
}

extern "C" int dyt_loss(dyt_ctx* c, int slot_student, const float* logits_s, const float* logits_t, const int64_t* targets,
                        int batch, float token_target_ratio, float token_loss_ratio, float token_minimal,
                        float token_minimal_weight, float* dlogits_s, float* dlogits_t, float* out_losses, float* dtok,
                        void* stream) {
    return loss_impl(c, slot_student, logits_s, logits_t, targets, batch, token_target_ratio, token_loss_ratio, token_minimal,
                     token_minimal_weight, dlogits_s, dlogits_t, out_losses, dtok, stream, nullptr);
}

extern "C" int dyt_adamw(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t numel, int step,
                         float lr, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                         void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || numel < 1 || step < 1) { set_error("bad argument"); return DYT_ERR_ARG; }
    // bias corrections in double (as torch.optim.AdamW forms them), handed to the kernel as floats: 1 - powf(0.999f, step) in fp32 is
    // up to 7e-6 relative off in the first steps, which is the whole update of a parameter that starts at zero
    const float bc1 = (float)(1.0 - pow((double)beta1, (double)step));
    const float rsqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow((double)beta2, (double)step)));
    return launch_adamw(param, grad, exp_avg, exp_avg_sq, numel, lr, beta1, beta2, eps, weight_decay, bc1, rsqrt_bc2, grad_scale,
                        static_cast<hipStream_t>(stream));
}

// The same update, guarded like the reference's GradScaler.step (misc.py:256-272): if grad holds an inf / NaN (a 16-bit operand
// overflowed somewhere in the step) parameters and moments are left untouched and the skip is counted.  Nothing returns to the host:
// state (device int32[4], zero-initialised by the caller, owned by the optimizer) = {updates applied, updates skipped, flag of this
// call, reserved}; the bias corrections use state[0] + 1 as the step.
extern "C" int dyt_adamw_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t numel, int32_t* state,
                                 float lr, float beta1, float beta2, float eps, float weight_decay, float grad_scale, void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || !state || numel < 1) { set_error("bad argument"); return DYT_ERR_ARG; }
    return launch_adamw_guarded(param, grad, exp_avg, exp_avg_sq, numel, state, lr, beta1, beta2, eps, weight_decay, grad_scale,
                                static_cast<hipStream_t>(stream));
}

// The same update with lr and weight_decay per segment of the flat buffer (torch.optim.AdamW with several param_groups).  `segments` is a
// host array, read here and never again: it is copied into the kernel's arguments.  state != NULL: dyt_adamw_guarded's semantics over the
// WHOLE buffer (`step` ignored); state == NULL: dyt_adamw's with the 1-based `step`.
static_assert(sizeof(dyt_adamw_segment) == sizeof(AdamwSeg) && offsetof(dyt_adamw_segment, lr) == offsetof(AdamwSeg, lr) &&
              offsetof(dyt_adamw_segment, weight_decay) == offsetof(AdamwSeg, wd) && DYT_ADAMW_MAX_SEGMENTS == 128, "segment table layout");
extern "C" int dyt_adamw_segments(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t numel, int32_t* state, int step,
                                  const dyt_adamw_segment* segments, int num_segments, float beta1, float beta2, float eps,
                                  float grad_scale, void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || !segments || numel < 1 || (!state && step < 1)) { set_error("bad argument"); return DYT_ERR_ARG; }
    if (num_segments < 1 || num_segments > DYT_ADAMW_MAX_SEGMENTS) {
        set_error("dyt_adamw_segments: %d segments (1 ... %d)", num_segments, DYT_ADAMW_MAX_SEGMENTS);
        return DYT_ERR_ARG;
    }
    AdamwSegTable table;
    memset(&table, 0, sizeof(table));
    int64_t prev = 0;
    for (int k = 0; k < num_segments; ++k) {
        if (segments[k].end <= prev) {
            set_error("dyt_adamw_segments: segment %d ends at %lld, not past %lld (ends must increase strictly)", k, (long long)segments[k].end, (long long)prev);
            return DYT_ERR_ARG;
        }
        prev = segments[k].end;
        table.s[k].end = segments[k].end; table.s[k].lr = segments[k].lr; table.s[k].wd = segments[k].weight_decay;
    }
    if (prev != numel) {
        set_error("dyt_adamw_segments: the last segment ends at %lld, the buffer has %lld elements", (long long)prev, (long long)numel);
        return DYT_ERR_ARG;
    }
    float bc1 = 1.0f, rsqrt_bc2 = 1.0f;
    if (!state) {   // dyt_adamw's lines
        bc1 = (float)(1.0 - pow((double)beta1, (double)step));
        rsqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow((double)beta2, (double)step)));
    }
    return launch_adamw_segments(param, grad, exp_avg, exp_avg_sq, numel, state, table, num_segments, beta1, beta2, eps, bc1, rsqrt_bc2,
                                 grad_scale, static_cast<hipStream_t>(stream));
}

extern "C" int dyt_step_fwd_bwd(dyt_ctx* c, const float* images, const int64_t* targets, int batch, int flags,
                                const float* trainable, const float* g1, const float* g2, const uint8_t* keep_mask,
                                uint64_t seed, float token_target_ratio, float token_loss_ratio, float token_minimal,
                                float token_minimal_weight, float* grad_flat, float* out_losses, float* logits_s,
                                float* logits_t, float* token_select, void* stream) {
    if (!c) { set_error("null argument"); return DYT_ERR_ARG; }
    { int rc = refuse_inference(c, "dyt_step_fwd_bwd"); if (rc) return rc; }
    if (!images || !targets || !grad_flat || !out_losses) { set_error("null argument"); return DYT_ERR_ARG; }
    { int rc = check_image_input(flags, images); if (rc) return rc; }   // byte images: refused here, before the step enqueues anything
    if (c->cfg.slots < 2) { set_error("dyt_step_fwd_bwd needs 2 slots"); return DYT_ERR_STATE; }
    if (c->mix_params) {   // dyt_set_mix: refused here, before the step enqueues anything
        if (c->soft_targets) { set_error("dyt_step_fwd_bwd: mix is on (dyt_set_mix) and class-probability targets are set (dyt_set_soft_targets)"); return DYT_ERR_STATE; }
        int rc = check_mix_batch(c, batch); if (rc) return rc;
    }
    { int rc = check_erase_batch(c, batch); if (rc) return rc; }   // dyt_set_erase: a batch the table has no rows for
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int depth = c->cfg.depth;
    const size_t nz = (size_t)depth * batch * NP;        // per-pass noise stride
    const size_t kz = (size_t)depth * batch * NT * c->cfg.ffn_num;
    float* ls = logits_s ? logits_s : c->logits_s;
    float* lt = logits_t ? logits_t : c->logits_t;
    // (the image flags reach both passes: the teacher's own embedding, when block 0 is not shared, reads the same bytes)
    const int fl = (flags & (DYT_F_MASKED_DENSE | DYT_F_DEVICE_SEED | DYT_F_IMAGES_U8 | DYT_F_IMAGES_NHWC)) | DYT_F_TRAINING | DYT_F_SAVE;
    // Two-stream schedule: student pass on the caller's stream, teacher pass on a side stream
    // (fork/join with events; graph-capturable).  Profiling mode runs serially for clean per-kernel times.
    const bool par = c->overlap && c->ov_pass && !c->prof;
    if (par && !c->side) {
        // measurement hook (tools/probes/determinism_cumask.py): DYT_DBG_SIDE_CU_MASK = "cu" | "xcd" pins the teacher pass to
        // the odd CU octets / the upper four XCDs (mask bit i -> XCD i % 8), the probe pins the caller's stream to the rest
        const char* dbg_mask = getenv("DYT_DBG_SIDE_CU_MASK");
        if (dbg_mask && (dbg_mask[0] == 'c' || dbg_mask[0] == 'x' || dbg_mask[0] == 'i' || dbg_mask[0] == 'a')) {
            uint32_t words[8];
            for (int i = 0; i < 8; ++i) words[i] = dbg_mask[0] == 'c' ? 0xFF00FF00u : (dbg_mask[0] == 'x' ? 0xF0F0F0F0u : (dbg_mask[0] == 'a' ? 0xF8F8F8F8u : 0x00FFFFFFu));   // a: five XCDs for the (heavier) teacher pass
            DYT_HIP_CHECK(hipExtStreamCreateWithCUMask(&c->side, 8, words));
        } else {
            DYT_HIP_CHECK(hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
        }
        DYT_HIP_CHECK(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
        DYT_HIP_CHECK(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
    }
    hipStream_t s2 = par ? c->side : s;
    if (batch % c->frames != 0) { set_error("video model: batch %d is not a multiple of frames %d", batch, c->frames); return DYT_ERR_ARG; }
    int rc = dbg_ck_reset(s);
    if (rc) return rc;
    rc = prep_adapters(c, trainable, s);
    if (rc) return rc;
    rc = prep_pool(c, trainable, s);
    if (rc) return rc;
    if (par) { DYT_HIP_CHECK(hipEventRecord(c->ev_fork, s)); DYT_HIP_CHECK(hipStreamWaitEvent(s2, c->ev_fork, 0)); }
    {
        // hipGraph stream capture (ROCm 7.2): a stream that forks from a stream which is itself a fork of the capture's
        // origin stream crashes hipStreamEndCapture (bisected on MI355X: origin -> side is fine, origin -> branch is fine,
        // side -> branch is not).  While capturing, the teacher pass (on the side stream) therefore keeps its adapter
        // branch on its own stream; the graph still carries the two passes and the student's branch as parallel chains.
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        DYT_HIP_CHECK(hipStreamIsCapturing(s, &cs));
        c->slots[1].no_branch = par && cs == hipStreamCaptureStatusActive;
        c->slots[0].no_branch = false;
    }
    // The two passes see the same images and the same frozen weights, and nothing trainable or random sits
    // in front of block 0's attention branch: the teacher pass reuses the student's embedding, LN1, qkv,
    // attention and proj of block 0 (its block-0 `u` pointers alias the student's for this step).
    const bool share = c->share_block0;
    if (share && !c->ev_b0) DYT_HIP_CHECK(hipEventCreateWithFlags(&c->ev_b0, hipEventDisableTiming));
    {
        Slot& S0 = c->slots[0]; Slot& S1 = c->slots[1];
        S0.L[0].u = S0.u0_own; S0.L[0].u_at = S0.u0_at_own;
        S1.L[0].u = share ? S0.u0_own : S1.u0_own;
        S1.L[0].u_at = share ? S0.u0_at_own : S1.u0_at_own;
        S0.L[0].u16 = S0.u0_16_own; S1.L[0].u16 = share ? S0.u0_16_own : S1.u0_16_own;
        S0.L[0].ln_part = S0.part0_own; S1.L[0].ln_part = share ? S0.part0_own : S1.part0_own;
    }
    rc = forward_impl(c, 0, images, batch, fl, trainable, g1, g2, keep_mask, seed, ls, token_select, nullptr, false, s,
                      nullptr, share ? c->ev_b0 : nullptr, nullptr);
    if (rc) return rc;
    // the teacher pass draws its own noise in the reference (mask discarded): only the dropout stream matters
    rc = forward_impl(c, 1, images, batch, fl | DYT_F_COMPLETE, trainable, g1 ? g1 + nz : nullptr, g2 ? g2 + nz : nullptr,
                      keep_mask ? keep_mask + kz : nullptr, seed, lt, nullptr, nullptr, false, s2,
                      share ? &c->slots[0] : nullptr, nullptr, (share && par) ? c->ev_b0 : nullptr);
    if (rc) return rc;
    if (par) { DYT_HIP_CHECK(hipEventRecord(c->ev_join, s2)); DYT_HIP_CHECK(hipStreamWaitEvent(s, c->ev_join, 0)); }
    if (c->mix_params) {   // the class-probability rows of this draw, from the integer labels, on the step's stream ahead of the loss
        rc = launch_mix_targets(targets, c->mix_soft, batch / c->frames, c->cfg.num_classes, c->mix_params, s);
        if (rc) return rc;
    }
    rc = loss_impl(c, 0, ls, lt, targets, batch / c->frames, token_target_ratio, token_loss_ratio, token_minimal, token_minimal_weight,
                   c->dl_s, c->dl_t, out_losses, c->dtok, stream, c->mix_params ? c->mix_soft : nullptr);
    if (rc) return rc;
    float* gt = par ? c->grad2 : grad_flat;  // teacher-pass gradients
    // measurement hook: DYT_DBG_TEACHER_NAN=1 feeds the teacher's backward pass NaN (every value it computes or stores is NaN) and
    // leaves the two passes' gradients unsummed: any NaN in grad_flat (the student's) is a write across the passes
    static const bool dbg_tnan = getenv("DYT_DBG_TEACHER_NAN") && atoi(getenv("DYT_DBG_TEACHER_NAN"));
    if (dbg_tnan && par) DYT_HIP_CHECK(hipMemsetAsync(c->dl_t, 0xFF, (size_t)batch * c->cfg.num_classes * sizeof(float), s));
    if (par) { DYT_HIP_CHECK(hipEventRecord(c->ev_fork, s)); DYT_HIP_CHECK(hipStreamWaitEvent(s2, c->ev_fork, 0)); }
    if (!(flags & DYT_F_ACCUM_GRAD)) DYT_HIP_CHECK(hipMemsetAsync(grad_flat, 0, (size_t)c->n_train * sizeof(float), s));
    if (par) DYT_HIP_CHECK(hipMemsetAsync(c->grad2, 0, (size_t)c->n_train * sizeof(float), s2));
    // Chunked all-reduce support (DDP fires its buckets inside loss.backward(), misc.py:258-259): the backward runs
    // block 11 -> 0, so the gradients of the head and of blocks >= depth/2 -- a contiguous tail of the flat buffer --
    // are final half-way through.  ev_upper marks that point (both passes summed) for dyt_stream_wait_grads().
    const int split = depth / 2;
    const int64_t up_off = (int64_t)split * c->layer_stride, up_n = c->n_train - up_off;
    if (!c->ev_upper) {
        DYT_HIP_CHECK(hipEventCreateWithFlags(&c->ev_half_s, hipEventDisableTiming));
        DYT_HIP_CHECK(hipEventCreateWithFlags(&c->ev_half_t, hipEventDisableTiming));
        DYT_HIP_CHECK(hipEventCreateWithFlags(&c->ev_upper, hipEventDisableTiming));
        DYT_HIP_CHECK(hipStreamCreateWithFlags(&c->aux, hipStreamNonBlocking));
    }
    g_dbg_in_backward = 1;
    rc = backward_impl(c, 0, trainable, c->dl_s, nullptr, c->dtok, nullptr, grad_flat, s, par ? c->ev_half_s : nullptr, split);
    if (rc) { g_dbg_in_backward = 0; return rc; }
    if (par && c->ov_bwd_serial) { DYT_HIP_CHECK(hipEventRecord(c->ev_fork, s)); DYT_HIP_CHECK(hipStreamWaitEvent(s2, c->ev_fork, 0)); }
    rc = backward_impl(c, 1, trainable, c->dl_t, nullptr, nullptr, nullptr, gt, s2, par ? c->ev_half_t : c->ev_upper, split);
    g_dbg_in_backward = 0;
    if (rc) return rc;
    if (par) {
        // upper part: summed on the aux stream as soon as both passes have left block `split`
        DYT_HIP_CHECK(hipStreamWaitEvent(c->aux, c->ev_half_s, 0));
        DYT_HIP_CHECK(hipStreamWaitEvent(c->aux, c->ev_half_t, 0));
        if (!dbg_tnan) rc = launch_reduce_partials(c->grad2 + up_off, 1, 0, grad_flat + up_off, (int)up_n, 1.0f, c->aux);
        if (rc) return rc;
        DYT_HIP_CHECK(hipEventRecord(c->ev_upper, c->aux));
        // lower part: after the teacher pass has finished
        DYT_HIP_CHECK(hipEventRecord(c->ev_join, s2));
        DYT_HIP_CHECK(hipStreamWaitEvent(s, c->ev_join, 0));
        if (!dbg_tnan) rc = launch_reduce_partials(c->grad2, 1, 0, grad_flat, (int)up_off, 1.0f, s);  // grad_flat[lower] += grad2[lower]
        if (rc) return rc;
        DYT_HIP_CHECK(hipStreamWaitEvent(s, c->ev_upper, 0));   // the caller's stream owns the whole buffer on return
    }
    c->upper_recorded = true;
    if (flags & DYT_F_DEVICE_SEED) rc = launch_seed_advance(c->seed_dev, s);
    return rc;
}

extern "C" int dyt_stream_wait_grads(dyt_ctx* c, int part, void* stream) {
    if (!c || part != 0) { set_error("dyt_stream_wait_grads: part 0 (head + upper blocks) is the only early part"); return DYT_ERR_ARG; }
    if (!c->upper_recorded) { set_error("no dyt_step_fwd_bwd has been enqueued yet"); return DYT_ERR_STATE; }
    DYT_HIP_CHECK(hipStreamWaitEvent(static_cast<hipStream_t>(stream), c->ev_upper, 0));
    return DYT_OK;
}

// ------------------------------------------------------------------------------------------
// gradient all-reduce on RCCL, behind the ABI (reference: DistributedDataParallel's bucket all-reduce inside loss.backward(),
// main_image.py:280-282 / misc.py:258-259).  librccl is NOT a link-time dependency: the symbol binds at load time to the RCCL that
// the host process already has (PyTorch's, promoted to the global scope by _lib.py, or the binder's own); absent -> an error.
// ------------------------------------------------------------------------------------------
extern "C" int ncclAllReduce(const void* sendbuff, void* recvbuff, size_t count, int datatype, int op, void* comm,
                             hipStream_t stream) __attribute__((weak));
extern "C" const char* ncclGetErrorString(int result) __attribute__((weak));

extern "C" int dyt_allreduce_grads(dyt_ctx* c, void* rccl_comm, float* grad_flat, void* comm_stream, void* stream) {
    { int rc = refuse_inference(c, "dyt_allreduce_grads"); if (rc) return rc; }
    if (!c || !rccl_comm || !grad_flat) { set_error("null argument"); return DYT_ERR_ARG; }
    if (!ncclAllReduce) { set_error("RCCL is not loaded in this process (ncclAllReduce unresolved)"); return DYT_ERR_STATE; }
    constexpr int kNcclFloat32 = 7, kNcclSum = 0;
    hipStream_t s = static_cast<hipStream_t>(stream), cs = static_cast<hipStream_t>(comm_stream);
    const int64_t up_off = (int64_t)(c->cfg.depth / 2) * c->layer_stride, up_n = c->n_train - up_off;
    auto chk = [](int rc) {
        if (rc != 0) { set_error("ncclAllReduce failed: %s", ncclGetErrorString ? ncclGetErrorString(rc) : "?"); return DYT_ERR_HIP; }
        return 0;
    };
    if (cs && cs != s && c->upper_recorded) {
        // part 0 (head + upper blocks): final half-way through the backward pass -> reduced on the communication stream while the
        // frozen-backbone backward of the lower blocks is still running on `stream`; part 1 follows on `stream`
        if (!c->ev_comm) DYT_HIP_CHECK(hipEventCreateWithFlags(&c->ev_comm, hipEventDisableTiming));
        DYT_HIP_CHECK(hipStreamWaitEvent(cs, c->ev_upper, 0));
        int rc = chk(ncclAllReduce(grad_flat + up_off, grad_flat + up_off, (size_t)up_n, kNcclFloat32, kNcclSum, rccl_comm, cs));
        if (rc) return rc;
        DYT_HIP_CHECK(hipEventRecord(c->ev_comm, cs));
        rc = chk(ncclAllReduce(grad_flat, grad_flat, (size_t)up_off, kNcclFloat32, kNcclSum, rccl_comm, s));
        if (rc) return rc;
        DYT_HIP_CHECK(hipStreamWaitEvent(s, c->ev_comm, 0));
        return DYT_OK;
    }
    return chk(ncclAllReduce(grad_flat, grad_flat, (size_t)c->n_train, kNcclFloat32, kNcclSum, rccl_comm, s));
}

extern "C" int dyt_clip_grad_norm(dyt_ctx* c, float* grad, int64_t numel, float max_norm, float pre_scale, float* norm_out,
                                  void* stream) {
    { int rc = refuse_inference(c, "dyt_clip_grad_norm"); if (rc) return rc; }
    if (!c || !grad || numel < 1 || !(max_norm > 0.f)) { set_error("bad argument"); return DYT_ERR_ARG; }
    return launch_clip_grad_norm(grad, numel, max_norm, pre_scale, c->clip_scratch, norm_out, static_cast<hipStream_t>(stream));
}
