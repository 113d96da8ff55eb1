// The context: error string, the two arena layouts, frozen-weight upload and its split / bwd16 / LN-fold refreshes, options, profile.
#include "ctx.h"

namespace dyt {

int g_dbg_in_backward = 0;   // measurement hook, see dbg_skip (kernels.h)
static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
}  // namespace dyt

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

template <class T>
static T* carve(dyt_ctx* c, size_t count, bool dry) {
    const size_t bytes = align_up(count * sizeof(T), 256);
    T* p = dry ? nullptr : reinterpret_cast<T*>(c->arena + c->arena_used);
    c->arena_used += bytes;
    return p;
}
static void* carve_at(dyt_ctx* c, size_t count, bool dry) {
    const size_t bytes = align_up(count * c->at, 256);
    void* p = dry ? nullptr : c->arena + c->arena_used;
    c->arena_used += bytes;
    return p;
}

static void layout(dyt_ctx* c, bool dry) {
    const dyt_config& cf = c->cfg;
    const size_t B = cf.max_batch, M = B * NT, depth = cf.depth, C = cf.num_classes;
    // inference-only contexts (dyt_ctx::inf) carve nothing that only the backward pass / the optimizer entries read: bwd_at / bwd_f32 return null there
    // (in a training context they carve in place, so its layout is byte for byte what it was)
    const bool inf = c->inf;
    auto bwd_at = [&](size_t n) -> void* { return inf ? nullptr : carve_at(c, n, dry); };
    auto bwd_f32 = [&](size_t n) -> float* { return inf ? nullptr : carve<float>(c, n, dry); };
    c->arena_used = 0;
    c->cls = carve<float>(c, D, dry);
    c->pos = carve<float>(c, NT * D, dry);
    c->pe_b = carve<float>(c, D, dry);
    c->norm_w = carve<float>(c, D, dry);
    c->norm_b = carve<float>(c, D, dry);
    c->pe_w = carve_at(c, (size_t)D * D, dry);
    c->W.resize(depth);
    for (size_t l = 0; l < depth; ++l) {
        LayerW& w = c->W[l];
        w.ln1_w = carve<float>(c, D, dry); w.ln1_b = carve<float>(c, D, dry);
        w.ln2_w = carve<float>(c, D, dry); w.ln2_b = carve<float>(c, D, dry);
        w.qkv_b = carve<float>(c, 3 * D, dry); w.proj_b = carve<float>(c, D, dry);
        w.fc1_b = carve<float>(c, DM, dry); w.fc2_b = carve<float>(c, D, dry);
        w.qkv_w = carve_at(c, (size_t)3 * D * D, dry); w.qkv_wT = bwd_at((size_t)3 * D * D);
        w.proj_w = carve_at(c, (size_t)D * D, dry); w.proj_wT = bwd_at((size_t)D * D);
        w.fc1_w = carve_at(c, (size_t)DM * D, dry); w.fc1_wT = bwd_at((size_t)DM * D);
        w.fc2_w = carve_at(c, (size_t)DM * D, dry); w.fc2_wT = bwd_at((size_t)DM * D);
        if (c->prec != 0) {
            w.qkv_wp = carve_at(c, (size_t)3 * D * D, dry); w.fc1_wp = carve_at(c, (size_t)DM * D, dry);
            w.fc2_wTp = bwd_at((size_t)DM * D);
            w.proj_wp = carve_at(c, (size_t)D * D, dry); w.proj_wTp = bwd_at((size_t)D * D);
            w.qkv_wTp = bwd_at((size_t)3 * D * D); w.fc1_wTp = bwd_at((size_t)DM * D);
            if (c->ln_fold) {
                w.fc1_wf = carve_at(c, (size_t)DM * D, dry); w.fc1_wfp = carve_at(c, (size_t)DM * D, dry);
                w.fc1_cs = carve<float>(c, DM, dry); w.fc1_bf = carve<float>(c, DM, dry); w.fc1_w32 = carve<float>(c, (size_t)DM * D, dry);
            }
        }
    }
    c->ad_down_w = carve_at(c, depth * RP * D, dry);
    c->ad_down_wT = bwd_at(depth * RP * D);
    c->ad_up_w = carve_at(c, depth * RP * D, dry);
    c->ad_up_wT = bwd_at(depth * RP * D);
    c->ad_down_b = carve<float>(c, depth * RP, dry);
    c->ad_lift = bwd_f32(2 * depth);
    const int nslots = inf ? 1 : cf.slots;   // inference-only: every slot index runs in the one slot (forward_impl)
    c->slots.resize(nslots);
    for (int s = 0; s < nslots; ++s) {
        Slot& S = c->slots[s];
        S.L.resize(depth);
        S.xs.resize(depth + 1);
        if (inf) {   // block l reads xs[l] and writes xs[l + 1]; nothing reads xs[l] once block l is through: two streams in turn
            float* pp[2] = {carve<float>(c, M * D, dry), carve<float>(c, M * D, dry)};
            for (size_t l = 0; l <= depth; ++l) S.xs[l] = pp[l & 1];
        } else
        for (size_t l = 0; l <= depth; ++l) S.xs[l] = carve<float>(c, M * D, dry);
        S.counts = carve<int>(c, depth * B, dry);
        S.ucls_at = carve_at(c, B * D, dry);
        S.gcls = bwd_f32(B * D);
        S.cls_n = carve<float>(c, B * D, dry);
        S.head_stats = carve<float2>(c, B, dry);
        if (c->wide_head) S.head_part = bwd_f32(head_wide_scratch_floats((int)B, (int)C));
        if (c->avg_pool) S.pooled = carve<float>(c, B * D, dry);
        if (c->fc_norm) S.head_dy = bwd_f32(B * D);
        for (size_t l = 0; l < depth; ++l) {
            LayerS& L = S.L[l];
            if (inf && l > 0) { L = S.L[0]; continue; }   // one set of per-block buffers: every block's launches run in stream order, each rewrites what it reads
            L.st1 = inf ? nullptr : carve<float2>(c, M, dry); L.st2 = carve<float2>(c, M, dry);   // (LN1's statistics are the backward's: ln_fwd skips the store on null)
            if (c->ad_ln) L.st_a = carve<float2>(c, M, dry);
            if (c->ad_ln == 2) L.up32 = carve<float>(c, M * D, dry);
            L.q = carve_at(c, M * D, dry); L.k = carve_at(c, M * D, dry); L.v = carve_at(c, M * D, dry);
            L.attn_o = carve_at(c, M * D, dry);
            L.lse = carve<float>(c, B * NH * NT, dry);
            L.u = carve<float>(c, M * D, dry);
            L.u_at = c->prec == 0 ? (void*)L.u : carve_at(c, M * D, dry);
            if (c->prec != 0 && c->ln_fold) L.ln_part = carve<float2>(c, M * LN_PARTS, dry);
            L.z = bwd_at(M * DM);      // (an eval forward stores neither gelu'(z) nor the MLP output h: forward_impl passes null for both)
            L.d_act = carve_at(c, M * RP, dry);
            L.h = bwd_at(M * D);
            L.soft = carve<float>(c, M, dry); L.maskf = carve<float>(c, M, dry);
            L.keep_local = carve<int>(c, M, dry); L.offsets = carve<int>(c, B, dry);
            L.total = carve<int>(c, 4, dry); L.row_src = carve<int>(c, M, dry); L.dst_of = carve<int>(c, M, dry);
        }
    }
    if (c->frames > 1) {
        c->pk_w = carve_at(c, (size_t)D * D, dry); c->pk_wT = bwd_at((size_t)D * D);
        c->pv_w = carve_at(c, (size_t)D * D, dry); c->pv_wT = bwd_at((size_t)D * D);
        const size_t clips = B / c->frames;
        for (int sl = 0; sl < nslots; ++sl) {
            PoolS& Q = c->slots[sl].pool;
            Q.xf = carve<float>(c, M * D, dry);
            Q.st_f = carve<float2>(c, M, dry); Q.st_kv = carve<float2>(c, M, dry);
            Q.xk = carve_at(c, M * D, dry); Q.xv = carve_at(c, M * D, dry);
            Q.Kp = carve_at(c, M * D, dry); Q.Vp = carve_at(c, M * D, dry);
            const size_t Mp = (M + 63) / 64 * 64;
            Q.dKt = bwd_at(Mp * D); Q.xkt = bwd_at(Mp * D);
            Q.dVt = bwd_at(Mp * D); Q.xvt = bwd_at(Mp * D);
            Q.P = carve<float>(c, B * NH * NT, dry);
            Q.o = carve<float>(c, clips * D, dry); Q.y = carve<float>(c, clips * D, dry);
            Q.dy = bwd_f32(clips * D); Q.dO = bwd_f32(clips * D);
            Q.dq_part = bwd_f32(clips * D);
            Q.qn = carve<float>(c, D, dry); Q.qhat = carve<float>(c, D, dry); Q.qs = carve<float>(c, D, dry);
            Q.gq = bwd_f32(D); Q.dqn = bwd_f32(D); Q.st_q = carve<float>(c, 4, dry);
        }
    }
    for (int sl = 0; sl < nslots; ++sl) {
        Transients& T = c->slots[sl].T;
        T.xn = carve_at(c, M * D, dry);
        if (c->prec != 0 && c->ln_fold) { T.st_compact = carve<float2>(c, M, dry); T.drop_src = carve<int>(c, M, dry); }
        T.h1 = carve_at(c, M * DM, dry);
        T.g_at = bwd_at(M * D);
        T.dZ = bwd_at(M * DM);
        // (the forward borrows T.dZ as the split-K workspace of the last block's cls-only fc2: [K / 256 + 1 slices][B][768] fp32 of its own here)
        if (inf) T.sk_ws = carve<float>(c, (size_t)(DM / 256 + 1) * B * D, dry);
        T.ddz = bwd_at(M * RP);
        T.du_at = bwd_at(M * D);
        T.dad = c->prec != DYT_PREC_FP32 ? bwd_at(M * D) : nullptr;
        T.dact_s = c->prec != DYT_PREC_FP32 ? carve_at(c, M * RP, dry) : nullptr;
        T.dO = bwd_at(M * D);
        T.dqkv = bwd_at(M * 3 * D);
        T.dA2 = bwd_at(M * D);
        T.dxn = bwd_at(M * D);
        T.g = bwd_f32(M * D);
        T.delta = bwd_f32(B * NH * NT);
        T.dmask = bwd_f32(M);
        if (c->ad_ln) {
            T.xa = carve<float>(c, M * D, dry); T.dup = bwd_f32(M * D);
            T.aln_part = bwd_f32((size_t)ln_param_grad_scratch_floats((int)M));
        }
        T.tok_partial = bwd_f32(((M + 31) / 32) * (D + 1));
        T.wg_partial = bwd_f32(((M + 511) / 512) * (size_t)(D + 8) * 80);
        T.wg_partial2 = bwd_f32(((M + 511) / 512) * (size_t)(D + 8) * 80);
        Slot& S = c->slots[sl];
        S.dp_own = bwd_f32(2 * depth * B);   // (stochastic depth belongs to training passes: dyt_set_drop_path refuses)
        S.gscr = bwd_f32((size_t)depth * c->layer_stride);
        S.wg_part.resize(depth); S.wg_part2.resize(depth); S.tok_part.resize(depth);
        for (size_t l = 0; l < depth; ++l) {
            S.wg_part[l] = bwd_f32(((M + 511) / 512) * (size_t)(D + 8) * 80);
            S.wg_part2[l] = bwd_f32(((M + 511) / 512) * (size_t)(D + 8) * 80);
            S.tok_part[l] = bwd_f32(((M + 31) / 32) * (D + 1));
        }
    }
    c->grad2 = bwd_f32((size_t)c->n_train);
    c->ad_up_bp = carve<float>(c, depth * D, dry);
    if (c->ad_ln == 2) c->ad_up_ws = carve_at(c, depth * RP * D, dry);
    c->cls_rows = carve<int>(c, B, dry);
    c->seed_dev = carve<uint64_t>(c, 2, dry);
    c->clip_scratch = bwd_f32(256);
    c->dl_s = bwd_f32(B * C); c->dl_t = bwd_f32(B * C);
    c->logits_s = bwd_f32(B * C); c->logits_t = bwd_f32(B * C);
    c->dtok = carve<float>(c, 4, dry);
    c->loss_part = carve<float>(c, 4 * B, dry);
    c->losses = carve<float>(c, 8, dry);
}

// The aux arena (fp32 contexts, allocated by DYT_OPT_F32_SPLIT16): [hi | lo] images of the frozen matrices ([N, SPLIT_A * K] 16-bit),
// the split A-operand scratch of a pass ([M, SPLIT_A * K]) and -- bwd16 -- the 16-bit tensors a 16-bit backward pass reads.
// Carved with the main arena's helpers (the caller swaps the arena fields around the call).
static void layout_aux(dyt_ctx* c, bool dry, bool bwd16) {
    const dyt_config& cf = c->cfg;
    const size_t B = cf.max_batch, M = B * NT, depth = cf.depth, SA = SPLIT_A;
    const bool inf = c->inf;   // inference-only: the forward's images and operand scratch alone, one set of per-block planes (as layout)
    auto bwd16_u16 = [&](size_t n) -> void* { return inf ? nullptr : (void*)carve<uint16_t>(c, n, dry); };
    c->arena_used = 0;
    c->pe_w3 = carve<uint16_t>(c, SA * D * D, dry);
    c->pe_w_exp = carve<int>(c, 4, dry);
    c->f8_scratch = carve<unsigned>(c, 4, dry);
    for (size_t l = 0; l < depth; ++l) {
        LayerW& w = c->W[l];
        w.w_exp = carve<int>(c, 4, dry);
        if (bwd16) {
            w.qkv_w3b = carve<uint16_t>(c, SA * 3 * D * D, dry); w.proj_w3b = carve<uint16_t>(c, SA * D * D, dry);
            w.fc1_w3b = carve<uint16_t>(c, SA * DM * D, dry); w.fc2_w3b = carve<uint16_t>(c, SA * DM * D, dry);
        }
        w.qkv_w3 = carve<uint16_t>(c, SA * 3 * D * D, dry); w.qkv_wT3 = bwd16_u16(SA * 3 * D * D);
        w.proj_w3 = carve<uint16_t>(c, SA * D * D, dry); w.proj_wT3 = bwd16_u16(SA * D * D);
        w.fc1_w3 = carve<uint16_t>(c, SA * DM * D, dry); w.fc1_wT3 = bwd16_u16(SA * DM * D);
        w.fc2_w3 = carve<uint16_t>(c, SA * DM * D, dry); w.fc2_wT3 = bwd16_u16(SA * DM * D);
        if (bwd16) {
            w.qkv_wT16 = bwd16_u16((size_t)3 * D * D); w.qkv_wTp16 = bwd16_u16((size_t)3 * D * D);
            w.proj_wT16 = bwd16_u16((size_t)D * D); w.proj_wTp16 = bwd16_u16((size_t)D * D);
            w.fc1_wT16 = bwd16_u16((size_t)DM * D); w.fc1_wTp16 = bwd16_u16((size_t)DM * D);
            w.fc2_wT16 = bwd16_u16((size_t)DM * D); w.fc2_wTp16 = bwd16_u16((size_t)DM * D);
        }
    }
    if (bwd16) {
        c->ad_up_wT16 = bwd16_u16(depth * RP * D);
        c->ad_down_wT16 = bwd16_u16(depth * RP * D);
        c->ad_scratch16 = bwd16_u16(2 * depth * RP * D);   // the two layouts of prep_adapters_kernel the backward does not read
        c->ad_up_w3 = carve<uint16_t>(c, SA * depth * RP * D, dry);
    }
    for (int sl = 0; sl < (int)c->slots.size(); ++sl) {
        Slot& S = c->slots[sl];
        Transients& T = S.T;
        const size_t Mp = (M + 255) / 256 * 256;   // whole 256-row tiles: the fp8-correction kernel reads the rows of its last tile unclamped
        T.a3 = carve<uint16_t>(c, Mp * SA * DM, dry);
        T.xn3 = carve<uint16_t>(c, Mp * SA * D, dry);
        T.g3 = carve<uint16_t>(c, Mp * SA * D, dry);
        T.h3 = carve<uint16_t>(c, Mp * SA * DM, dry);
        T.dqkv3 = bwd16_u16(M * SA * 3 * D);
        if (!bwd16) continue;
        T.dact3 = carve<uint16_t>(c, Mp * SA * RP, dry);
        T.drop_src = carve<int>(c, M, dry);   // (ln_gather writes the dropped rows' list for their three-part up-projection launch)
        T.dad16 = bwd16_u16(M * D);
        T.qlo = carve<uint16_t>(c, M * D, dry); T.klo = carve<uint16_t>(c, M * D, dry); T.vlo = carve<uint16_t>(c, M * D, dry);
        S.ucls16 = bwd16_u16(B * D);
        for (size_t l = 0; l < depth; ++l) {
            LayerS& L = S.L[l];
            if (inf && l > 0) {   // the hi planes of q / k / v are the attention kernel's inputs; the rest exists for a saved pass (save16)
                L.q16 = S.L[0].q16; L.k16 = S.L[0].k16; L.v16 = S.L[0].v16;
                L.o16 = nullptr; L.ao3 = nullptr; L.u16 = nullptr; L.h16 = nullptr; L.z16 = nullptr; L.dact16 = nullptr;
                continue;
            }
            L.q16 = carve<uint16_t>(c, M * D, dry); L.k16 = carve<uint16_t>(c, M * D, dry); L.v16 = carve<uint16_t>(c, M * D, dry);
            L.o16 = nullptr; L.ao3 = bwd16_u16(Mp * SA * D);   // padded to whole 256-row tiles like the other fp8-form operand images (the 256x256 kernel reads its last tile unclamped)
             L.u16 = bwd16_u16(M * D); L.h16 = bwd16_u16(M * D);
            L.z16 = bwd16_u16(M * DM); L.dact16 = bwd16_u16(M * RP);
        }
        if (!dry) S.u0_16_own = S.L[0].u16;
    }
}
// (re)allocates the aux arena; with_bwd16: including the 16-bit backward's buffers
static int alloc_aux(dyt_ctx* c, bool with_bwd16) {
    if (c->aux_arena && (c->aux_bwd16 || !with_bwd16)) return 0;
    DYT_HIP_CHECK(hipDeviceSynchronize());
    char* main_base = c->arena; const size_t main_used = c->arena_used;
    char* old_arena = c->aux_arena; const size_t old_size = c->aux_size; const bool old_bwd16 = c->aux_bwd16;
    layout_aux(c, true, with_bwd16);   // dry run: the new size (this nulls every aux pointer; they are re-carved below on either path)
    const size_t new_size = c->arena_used;
    char* fresh = nullptr;
    // the NEW arena first: if it cannot be had, the context keeps the old one (freeing first left every W.*_w3 / T.*3 /
    // L.*16 pointer null while split16 stayed set from the earlier option value)
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&fresh), new_size);
    if (e == hipSuccess) e = hipMemset(fresh, 0, new_size);
    if (e != hipSuccess) {
        set_error("aux arena: hipMalloc / hipMemset(%zu bytes) failed: %s", new_size, hipGetErrorString(e));
        if (fresh) (void)hipFree(fresh);
        if (old_arena) { c->arena = old_arena; layout_aux(c, false, old_bwd16); }   // the old arena's layout, contents untouched
        c->arena = main_base; c->arena_used = main_used;
        c->aux_size = old_size;
        return DYT_ERR_HIP;
    }
    if (old_arena) (void)hipFree(old_arena);
    c->aux_arena = fresh;
    c->aux_size = new_size;
    c->arena = c->aux_arena;
    layout_aux(c, false, with_bwd16);
    c->arena = main_base; c->arena_used = main_used;
    c->aux_bwd16 = with_bwd16;
    DYT_HIP_CHECK(hipDeviceSynchronize());
    return 0;
}

static void trainable_layout(dyt_ctx* c) {
    const int64_t r = c->cfg.ffn_num, C = c->cfg.num_classes;
    auto a4 = [](int64_t v) { return (v + 3) / 4 * 4; };
    int64_t o = 0;
    c->off_dw = o; o = a4(o + r * D);
    c->off_db = o; o = a4(o + r);
    c->off_uw = o; o = a4(o + (int64_t)D * r);
    c->off_ub = o; o = a4(o + D);
    c->off_gw = o; o += D;       // gate weight and bias stay adjacent (one 769-wide reduction)
    c->off_gb = o; c->off_sc = o + 1; o = a4(o + 2);   // + the adapter's learnable scale (used under DYT_OPT_LEARNABLE_SCALE; a zero padding word otherwise)
    if (c->cfg.adapter_ln) { c->off_alw = o; o += D; c->off_alb = o; o += D; }   // the adapter's LayerNorm: gamma and beta adjacent (one 1536-wide reduction)
    c->layer_stride = o;
    o = c->layer_stride * c->cfg.depth;
    c->off_hw = o; o = a4(o + C * D);
    c->off_hb = o; o = a4(o + C);
    if (c->fc_norm) { c->off_fnw = o; o += D; c->off_fnb = o; o += D; }   // fc_norm gamma / beta directly behind head.bias (inside part 0 of dyt_grad_part)
    if (c->frames > 1) {
        c->off_pquery = o; o += D;
        c->off_pnq_w = o; o += D; c->off_pnq_b = o; o += D;
        c->off_pnk_w = o; o += D; c->off_pnk_b = o; o += D;   // norm_k / norm_v {w,b} stay adjacent:
        c->off_pnv_w = o; o += D; c->off_pnv_b = o; o += D;   // one 4x768 partial reduction covers them
        c->off_pq_w = o; o += (int64_t)D * D;
        c->off_pk_w = o; o += (int64_t)D * D;
        c->off_pv_w = o; o += (int64_t)D * D;
        c->off_pq_bias = o; o += D; c->off_pv_bias = o; o += D;
        c->off_pproj_w = o; o += (int64_t)D * D;
        c->off_pproj_b = o; o += D;
    }
    c->n_train = o;
}

extern "C" const char* dyt_last_error(void) { return g_err; }
extern "C" int dyt_version(void) { return 5; }   // 2: dyt_config::adapter_ln appended (round 6); 3: dyt_config::inference_only appended; 4: dyt_ctx_create_ex, dyt_head_wide; 5: DYT_CREATE_AVG_POOL / _FC_NORM, dyt_pool_head

// dyt_config::inference_only: the entry points that need what such a context does not carve refuse before anything is enqueued
int dyt::refuse_inference(const dyt_ctx* c, const char* what) {
    if (!c || !c->inf) return 0;
    set_error("%s: the context was created with dyt_config.inference_only = 1 (eval forwards without DYT_F_SAVE only); create a training context for it", what);
    return DYT_ERR_ARG;
}
// 16-bit operand type of this build: 0 = bfloat16 (libdyt_hip.so), 1 = IEEE half (libdyt_hip_f16.so)
extern "C" int dyt_operand_type(void) {
#ifdef DYT_FP16
    return 1;
#else
    return 0;
#endif
}

extern "C" int dyt_ctx_create(const dyt_config* cfg, dyt_ctx** out) { return dyt_ctx_create_ex(cfg, 0, out); }

extern "C" int dyt_ctx_create_ex(const dyt_config* cfg, uint32_t create_flags, dyt_ctx** out) {
    if (!cfg || !out) { set_error("null argument"); return DYT_ERR_ARG; }
    const uint32_t known_flags = DYT_CREATE_WIDE_HEAD | DYT_CREATE_AVG_POOL | DYT_CREATE_FC_NORM;
    if (create_flags & ~known_flags) {
        set_error("dyt_ctx_create_ex: unknown create_flags 0x%x (known: DYT_CREATE_WIDE_HEAD = 0x%x, DYT_CREATE_AVG_POOL = 0x%x, DYT_CREATE_FC_NORM = 0x%x)",
                  create_flags, DYT_CREATE_WIDE_HEAD, DYT_CREATE_AVG_POOL, DYT_CREATE_FC_NORM);
        return DYT_ERR_ARG;
    }
    const bool wide = (create_flags & DYT_CREATE_WIDE_HEAD) != 0;
    const bool avg_pool = (create_flags & DYT_CREATE_AVG_POOL) != 0, fc_norm = (create_flags & DYT_CREATE_FC_NORM) != 0;
    if (avg_pool && !fc_norm) {   // the reference's ('avg', fc_norm=False): LayerNorm over all 197 rows in front of the mean, a frozen norm -- no HIP path
        set_error("dyt_ctx_create_ex: create_flags 0x%x: DYT_CREATE_AVG_POOL without DYT_CREATE_FC_NORM (global_pool='avg' with fc_norm=False) is not "
                  "implemented; pass both bits (0x%x)", create_flags, DYT_CREATE_AVG_POOL | DYT_CREATE_FC_NORM);
        return DYT_ERR_ARG;
    }
    if (fc_norm && cfg->frames > 1) {
        set_error("%s: image model only (frames=%d: the video model has its own attentive pooling head)", avg_pool ? "DYT_CREATE_AVG_POOL" : "DYT_CREATE_FC_NORM", cfg->frames);
        return DYT_ERR_ARG;
    }
    if (wide && cfg->num_classes > 65536) {
        set_error("unsupported config: num_classes=%d (1..65536 with DYT_CREATE_WIDE_HEAD; 1..1024 without)", cfg->num_classes);
        return DYT_ERR_ARG;
    }
    if (wide && cfg->frames > 1) { set_error("wide head: image model only (DYT_CREATE_WIDE_HEAD with frames=%d)", cfg->frames); return DYT_ERR_ARG; }
    if (cfg->ffn_num < 1 || cfg->ffn_num > RP || cfg->depth < 1 || cfg->depth > 64 || cfg->max_batch < 1 ||
        cfg->num_classes < 1 || (!wide && cfg->num_classes > 1024) || cfg->slots < 1 || cfg->slots > 4 ||
        (cfg->precision != DYT_PREC_FP32 && cfg->precision != DYT_PREC_BF16)) {
        set_error("unsupported config: ffn_num=%d (1..64) depth=%d max_batch=%d num_classes=%d (%s) slots=%d precision=%d",
                  cfg->ffn_num, cfg->depth, cfg->max_batch, cfg->num_classes, wide ? "1..65536" : "1..1024", cfg->slots, cfg->precision);
        return DYT_ERR_ARG;
    }
    int ndev = 0;
    DYT_HIP_CHECK(hipGetDeviceCount(&ndev));
    if (ndev < 1) { set_error("no HIP device"); return DYT_ERR_HIP; }
    if (cfg->frames > 1 && (cfg->max_batch % cfg->frames != 0 || cfg->frames * NT * 2 * sizeof(float) > 60 * 1024)) {
        set_error("video model: max_batch %d must be a multiple of frames %d (and frames <= 38)", cfg->max_batch, cfg->frames);
        return DYT_ERR_ARG;
    }
    if (cfg->adapter_ln < 0 || cfg->adapter_ln > 2 || (cfg->adapter_ln && cfg->frames > 1)) {
        set_error("adapter_ln=%d: 0 (none), 1 (in) or 2 (out); image model only", cfg->adapter_ln);
        return DYT_ERR_ARG;
    }
    if (cfg->inference_only != 0 && cfg->inference_only != 1) { set_error("inference_only=%d: 0 or 1", cfg->inference_only); return DYT_ERR_ARG; }
    dyt_ctx* c = new dyt_ctx();
    c->cfg = *cfg;
    c->inf = cfg->inference_only != 0;
    c->wide_head = wide;
    c->fc_norm = fc_norm; c->avg_pool = avg_pool;
    c->prec = cfg->precision;
    c->frames = cfg->frames > 1 ? cfg->frames : 1;
    c->ad_ln = cfg->adapter_ln;
    if (c->frames > 1) c->cls_tail = false;   // every token of the last block reaches the pooling head
    if (c->ad_ln) c->cls_tail = false;        // (generic path: the adapter's LayerNorm runs over all rows of every block)
    if (c->avg_pool) c->cls_tail = false;     // every patch token of the last block reaches the head
    c->at = at_size(c->prec);
#ifdef DYT_FP16
    if (c->prec != DYT_PREC_FP32) c->gs = 4096.0f;
#endif
    if (const char* e = getenv("DYT_LN_FOLD")) c->ln_fold = atoi(e) != 0;
    if (c->prec == 0) c->ln_fold = false;
#ifdef DYT_FP16
    c->g16 = true;   // (takes effect where the backward runs on 16-bit operands: P == 1)
    if (const char* e = getenv("DYT_G16")) c->g16 = c->g16 && atoi(e) != 0;
#endif
    trainable_layout(c);
    layout(c, true);
    c->arena_size = c->arena_used;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&c->arena), c->arena_size);
    if (e != hipSuccess) {
        set_error("hipMalloc(%zu bytes) failed: %s", c->arena_size, hipGetErrorString(e));
        delete c;
        return DYT_ERR_HIP;
    }
    layout(c, false);
    for (auto& S : c->slots) { S.u0_own = S.L[0].u; S.u0_at_own = S.L[0].u_at; S.part0_own = S.L[0].ln_part; }
    e = hipMemset(c->arena, 0, c->arena_size);
    if (e != hipSuccess) { set_error("hipMemset failed: %s", hipGetErrorString(e)); hipFree(c->arena); delete c; return DYT_ERR_HIP; }
    if (launch_cls_index(c->cls_rows, cfg->max_batch, nullptr) || hipDeviceSynchronize() != hipSuccess) {
        hipFree(c->arena); delete c; return DYT_ERR_HIP;
    }
    *out = c;
    return DYT_OK;
}

extern "C" int dyt_ctx_destroy(dyt_ctx* c) {
    if (!c) return DYT_OK;
    for (auto& r : c->recs) { hipEventDestroy(r.a); hipEventDestroy(r.b); }
    for (auto e : c->pool) hipEventDestroy(e);
    for (auto& S : c->slots) {
        if (S.ev_f) hipEventDestroy(S.ev_f);
        if (S.ev_j) hipEventDestroy(S.ev_j);
        if (S.branch) hipStreamDestroy(S.branch);
        if (S.pool.ev_wf) hipEventDestroy(S.pool.ev_wf);
        if (S.pool.ev_wj) hipEventDestroy(S.pool.ev_wj);
        if (S.pool.wstream) hipStreamDestroy(S.pool.wstream);
    }
    if (c->ev_b0) hipEventDestroy(c->ev_b0);
    if (c->ev_half_s) hipEventDestroy(c->ev_half_s);
    if (c->ev_half_t) hipEventDestroy(c->ev_half_t);
    if (c->ev_upper) hipEventDestroy(c->ev_upper);
    if (c->ev_comm) hipEventDestroy(c->ev_comm);
    if (c->aux) hipStreamDestroy(c->aux);
    if (c->ev_fork) hipEventDestroy(c->ev_fork);
    if (c->ev_join) hipEventDestroy(c->ev_join);
    if (c->side) hipStreamDestroy(c->side);
    if (c->arena) hipFree(c->arena);
    if (c->aux_arena) hipFree(c->aux_arena);
    if (c->mix_soft) hipFree(c->mix_soft);
    delete c;
    return DYT_OK;
}

extern "C" int dyt_ctx_bytes(const dyt_ctx* c, int64_t* bytes) {
    if (!c || !bytes) { set_error("null argument"); return DYT_ERR_ARG; }
    *bytes = (int64_t)(c->arena_size + c->aux_size + c->mix_soft_bytes);
    return DYT_OK;
}

extern "C" int dyt_trainable_numel(const dyt_ctx* c, int64_t* n) {
    if (!c || !n) { set_error("null argument"); return DYT_ERR_ARG; }
    *n = c->n_train;
    return DYT_OK;
}

extern "C" int dyt_trainable_offset(const dyt_ctx* c, int param, int layer, int64_t* off, int64_t* numel) {
    if (!c || !off || !numel) { set_error("null argument"); return DYT_ERR_ARG; }
    const int64_t r = c->cfg.ffn_num, C = c->cfg.num_classes;
    const int64_t base = (int64_t)layer * c->layer_stride;
    if (param >= DYT_P_AD_DOWN_W && param <= DYT_P_GATE_B && (layer < 0 || layer >= c->cfg.depth)) {
        set_error("layer %d out of range", layer);
        return DYT_ERR_ARG;
    }
    switch (param) {
        case DYT_P_AD_DOWN_W: *off = base + c->off_dw; *numel = r * D; break;
        case DYT_P_AD_DOWN_B: *off = base + c->off_db; *numel = r; break;
        case DYT_P_AD_UP_W: *off = base + c->off_uw; *numel = D * r; break;
        case DYT_P_AD_UP_B: *off = base + c->off_ub; *numel = D; break;
        case DYT_P_GATE_W: *off = base + c->off_gw; *numel = D; break;
        case DYT_P_GATE_B: *off = base + c->off_gb; *numel = 1; break;
        case DYT_P_AD_SCALE:
            if (layer < 0 || layer >= c->cfg.depth) { set_error("layer %d out of range", layer); return DYT_ERR_ARG; }
            *off = base + c->off_sc; *numel = 1; break;
        case DYT_P_AD_LN_W: case DYT_P_AD_LN_B:
            if (!c->ad_ln) { set_error("param %d exists with dyt_config.adapter_ln != 0 only", param); return DYT_ERR_ARG; }
            if (layer < 0 || layer >= c->cfg.depth) { set_error("layer %d out of range", layer); return DYT_ERR_ARG; }
            *off = base + (param == DYT_P_AD_LN_W ? c->off_alw : c->off_alb); *numel = D; break;
        case DYT_P_HEAD_W: *off = c->off_hw; *numel = C * D; break;
        case DYT_P_HEAD_B: *off = c->off_hb; *numel = C; break;
        case DYT_P_FC_NORM_W: case DYT_P_FC_NORM_B:
            if (!c->fc_norm) { set_error("param %d exists with DYT_CREATE_FC_NORM / DYT_CREATE_AVG_POOL only", param); return DYT_ERR_ARG; }
            *off = param == DYT_P_FC_NORM_W ? c->off_fnw : c->off_fnb; *numel = D; break;
        case DYT_P_POOL_QUERY: case DYT_P_POOL_NQ_W: case DYT_P_POOL_NQ_B: case DYT_P_POOL_NK_W: case DYT_P_POOL_NK_B:
        case DYT_P_POOL_NV_W: case DYT_P_POOL_NV_B: case DYT_P_POOL_Q_W: case DYT_P_POOL_K_W: case DYT_P_POOL_V_W:
        case DYT_P_POOL_Q_BIAS: case DYT_P_POOL_V_BIAS: case DYT_P_POOL_PROJ_W: case DYT_P_POOL_PROJ_B: {
            if (c->frames <= 1) { set_error("param %d exists in the video model only (cfg.frames > 1)", param); return DYT_ERR_ARG; }
            const int64_t offs[] = {c->off_pquery, c->off_pnq_w, c->off_pnq_b, c->off_pnk_w, c->off_pnk_b, c->off_pnv_w,
                                    c->off_pnv_b, c->off_pq_w, c->off_pk_w, c->off_pv_w, c->off_pq_bias, c->off_pv_bias,
                                    c->off_pproj_w, c->off_pproj_b};
            *off = offs[param - DYT_P_POOL_QUERY];
            const bool mat = param == DYT_P_POOL_Q_W || param == DYT_P_POOL_K_W || param == DYT_P_POOL_V_W || param == DYT_P_POOL_PROJ_W;
            *numel = mat ? (int64_t)D * D : D;
            break;
        }
        default: set_error("param %d is not trainable", param); return DYT_ERR_ARG;
    }
    return DYT_OK;
}

// weight [N,K] fp32 -> AT copy and transposed AT copy [K,N]
int dyt::set_matrix(dyt_ctx* c, const float* src, void* w, void* wT, int N, int K, hipStream_t s) {
    int rc = launch_pad_convert(c->prec, src, w, N, K, N, K, s);
    if (rc) return rc;
    if (wT) rc = launch_transpose_convert(c->prec, src, wT, N, K, K, N, s);
    return rc;
}
// fp32 mode: refresh the 16-bit [hi | lo] images of one layer's (layer < 0: the patch embedding's) frozen matrices
static int refresh_split(dyt_ctx* c, int layer, hipStream_t s) {
    if (c->prec != 0) return 0;
    if (c->f8) {   // forward images per class in the hi16 / fp8 or the [hi | lo] form (the backward of these modes runs on the 16-bit copies: no transposed images)
        const int fm = c->f8_mask, fmc = c->f8_mask_complete;
        auto one = [&](int bit, const void* src, void* dst, int N, int K, int* ew, void* dst_b = nullptr) {
            int rc = (fm & bit) ? launch_split_w_f8((const float*)src, dst, N, K, ew, c->f8_scratch, s) : launch_split3_w((const float*)src, dst, N, K, s);
            if (!rc && dst_b && ((fm ^ fmc) & bit))   // the complete_model pass takes the other form of this class: its own image
                rc = (fmc & bit) ? launch_split_w_f8((const float*)src, dst_b, N, K, ew, c->f8_scratch, s) : launch_split3_w((const float*)src, dst_b, N, K, s);
            return rc;
        };
        if (layer < 0) return one(16, c->pe_w, c->pe_w3, D, D, c->pe_w_exp);
        LayerW& w = c->W[layer];
        int rc = one(1, w.qkv_w, w.qkv_w3, 3 * D, D, w.w_exp + 0, w.qkv_w3b);
        if (!rc) rc = one(2, w.proj_w, w.proj_w3, D, D, w.w_exp + 1, w.proj_w3b);
        if (!rc) rc = one(4, w.fc1_w, w.fc1_w3, DM, D, w.w_exp + 2, w.fc1_w3b);
        if (!rc) rc = one(8, w.fc2_w, w.fc2_w3, D, DM, w.w_exp + 3, w.fc2_w3b);
        return rc;
    }
    if (layer < 0) return launch_split3_w((const float*)c->pe_w, c->pe_w3, D, D, s);
    LayerW& w = c->W[layer];
    const bool t = !c->inf;   // the transposed images are the gradient GEMMs': an inference-only context has neither them nor their fp32 sources
    int rc = launch_split3_w((const float*)w.qkv_w, w.qkv_w3, 3 * D, D, s);
    if (!rc && t) rc = launch_split3_w((const float*)w.qkv_wT, w.qkv_wT3, D, 3 * D, s);
    if (!rc) rc = launch_split3_w((const float*)w.proj_w, w.proj_w3, D, D, s);
    if (!rc && t) rc = launch_split3_w((const float*)w.proj_wT, w.proj_wT3, D, D, s);
    if (!rc) rc = launch_split3_w((const float*)w.fc1_w, w.fc1_w3, DM, D, s);
    if (!rc && t) rc = launch_split3_w((const float*)w.fc1_wT, w.fc1_wT3, D, DM, s);
    if (!rc) rc = launch_split3_w((const float*)w.fc2_w, w.fc2_w3, D, DM, s);
    if (!rc && t) rc = launch_split3_w((const float*)w.fc2_wT, w.fc2_wT3, DM, D, s);
    return rc;
}
// bwd16: the 16-bit transposed copies (plain + MFMA fragment order) of one layer's matrices, from the fp32 transposed copies
static int refresh_bwd16(dyt_ctx* c, int layer, hipStream_t s) {
    if (c->prec != 0 || !c->bwd16 || layer < 0 || c->inf) return 0;
    LayerW& w = c->W[layer];
    struct M16 { const void* src; void* dst; void* dstp; int N, K; };
    const M16 m[4] = {{w.qkv_wT, w.qkv_wT16, w.qkv_wTp16, D, 3 * D}, {w.proj_wT, w.proj_wT16, w.proj_wTp16, D, D},
                      {w.fc1_wT, w.fc1_wT16, w.fc1_wTp16, D, DM}, {w.fc2_wT, w.fc2_wT16, w.fc2_wTp16, DM, D}};
    for (const M16& x : m) {
        int rc = launch_convert(1, (const float*)x.src, x.dst, (int64_t)x.N * x.K, s);
        if (!rc) rc = launch_preshuffle_w(x.dst, x.dstp, x.N, x.K, s);
        if (rc) return rc;
    }
    return 0;
}
// 16-bit modes: the gamma-folded fc1 weight, its column sums and the beta-folded bias of one layer, from what the layer holds NOW (called
// after every upload of one of the four tensors involved: the last one leaves them consistent)
static int refresh_ln_fold(dyt_ctx* c, int layer, hipStream_t s) {
    LayerW& w = c->W[layer];
    if (c->prec == 0 || !w.fc1_wf) return 0;
    return launch_ln_fold_w(c->prec, w.fc1_w32, w.ln2_w, w.ln2_b, w.fc1_b, w.fc1_wf, w.fc1_wfp, w.fc1_cs, w.fc1_bf, DM, s);
}
static int copy_f32(float* dst, const float* src, size_t n, hipStream_t s) {
    DYT_HIP_CHECK(hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    return 0;
}

static int set_frozen_impl(dyt_ctx* c, int param, int layer, const float* src, void* stream);
extern "C" int dyt_set_frozen(dyt_ctx* c, int param, int layer, const float* src, void* stream) {
    int rc = set_frozen_impl(c, param, layer, src, stream);
    if (!rc && c->split16 && (param == DYT_P_PE_W || param == DYT_P_QKV_W || param == DYT_P_PROJ_W || param == DYT_P_FC1_W || param == DYT_P_FC2_W)) {
        rc = refresh_split(c, param == DYT_P_PE_W ? -1 : layer, static_cast<hipStream_t>(stream));
        if (!rc && param != DYT_P_PE_W) rc = refresh_bwd16(c, layer, static_cast<hipStream_t>(stream));
    }
    return rc;
}
static int set_frozen_impl(dyt_ctx* c, int param, int layer, const float* src, void* stream) {
    if (!c || !src) { set_error("null argument"); return DYT_ERR_ARG; }
    if (c->fc_norm && (param == DYT_P_NORM_W || param == DYT_P_NORM_B)) {
        set_error("DYT_P_NORM_%s: the context was created with DYT_CREATE_FC_NORM (the final norm is an identity there; the head's LayerNorm is the "
                  "trainable DYT_P_FC_NORM_W / _B of the flat buffer)", param == DYT_P_NORM_W ? "W" : "B");
        return DYT_ERR_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool per_layer = param >= DYT_P_LN1_W && param <= DYT_P_FC2_B;
    if (per_layer && (layer < 0 || layer >= c->cfg.depth)) { set_error("layer %d out of range", layer); return DYT_ERR_ARG; }
    LayerW* w = per_layer ? &c->W[layer] : nullptr;
    switch (param) {
        case DYT_P_CLS: return copy_f32(c->cls, src, D, s);
        case DYT_P_POS: return copy_f32(c->pos, src, (size_t)NT * D, s);
        case DYT_P_PE_W: return set_matrix(c, src, c->pe_w, nullptr, D, D, s);  // [768, 3*16*16]
        case DYT_P_PE_B: return copy_f32(c->pe_b, src, D, s);
        case DYT_P_LN1_W: return copy_f32(w->ln1_w, src, D, s);
        case DYT_P_LN1_B: return copy_f32(w->ln1_b, src, D, s);
        case DYT_P_QKV_W: {
            int rc = set_matrix(c, src, w->qkv_w, w->qkv_wT, 3 * D, D, s);
            if (!rc && w->qkv_wp) rc = launch_preshuffle_w(w->qkv_w, w->qkv_wp, 3 * D, D, s);
            if (!rc && w->qkv_wTp) rc = launch_preshuffle_w(w->qkv_wT, w->qkv_wTp, D, 3 * D, s);
            return rc;
        }
        case DYT_P_QKV_B: return copy_f32(w->qkv_b, src, 3 * D, s);
        case DYT_P_PROJ_W: {
            int rc = set_matrix(c, src, w->proj_w, w->proj_wT, D, D, s);
            if (!rc && w->proj_wp) rc = launch_preshuffle_w(w->proj_w, w->proj_wp, D, D, s);
            if (!rc && w->proj_wTp) rc = launch_preshuffle_w(w->proj_wT, w->proj_wTp, D, D, s);
            return rc;
        }
        case DYT_P_PROJ_B: return copy_f32(w->proj_b, src, D, s);
        case DYT_P_LN2_W: { int rc = copy_f32(w->ln2_w, src, D, s); return rc ? rc : refresh_ln_fold(c, layer, s); }
        case DYT_P_LN2_B: { int rc = copy_f32(w->ln2_b, src, D, s); return rc ? rc : refresh_ln_fold(c, layer, s); }
        case DYT_P_FC1_W: {
            int rc = set_matrix(c, src, w->fc1_w, w->fc1_wT, DM, D, s);
            if (!rc && w->fc1_wp) rc = launch_preshuffle_w(w->fc1_w, w->fc1_wp, DM, D, s);
            if (!rc && w->fc1_wTp) rc = launch_preshuffle_w(w->fc1_wT, w->fc1_wTp, D, DM, s);
            if (!rc && w->fc1_w32) rc = copy_f32(w->fc1_w32, src, (size_t)DM * D, s);
            return rc ? rc : refresh_ln_fold(c, layer, s);
        }
        case DYT_P_FC1_B: { int rc = copy_f32(w->fc1_b, src, DM, s); return rc ? rc : refresh_ln_fold(c, layer, s); }
        case DYT_P_FC2_W: {
            int rc = set_matrix(c, src, w->fc2_w, w->fc2_wT, D, DM, s);
            if (!rc && w->fc2_wTp) rc = launch_preshuffle_w(w->fc2_wT, w->fc2_wTp, DM, D, s);   // fc2^T: [3072, 768]
            return rc;
        }
        case DYT_P_FC2_B: return copy_f32(w->fc2_b, src, D, s);
        case DYT_P_NORM_W: return copy_f32(c->norm_w, src, D, s);
        case DYT_P_NORM_B: return copy_f32(c->norm_b, src, D, s);
        default: set_error("param %d is not a frozen parameter", param); return DYT_ERR_ARG;
    }
}

// ------------------------------------------------------------------------------------------
// profiling helpers
// ------------------------------------------------------------------------------------------
hipEvent_t dyt::get_event(dyt_ctx* c) {
    if (!c->pool.empty()) { hipEvent_t e = c->pool.back(); c->pool.pop_back(); return e; }
    hipEvent_t e;
    hipEventCreate(&e);
    return e;
}

// environment DYT_SPLIT_ATTN=0: the split modes keep the exact-fp32 attention kernels (include/dyt_hip.h)
static bool split_attn_env() { const char* e = getenv("DYT_SPLIT_ATTN"); return !e || atoi(e) != 0; }

extern "C" int dyt_ctx_set_option(dyt_ctx* c, int option, int value) {
    if (!c) { set_error("null ctx"); return DYT_ERR_ARG; }
    switch (option) {
        case DYT_OPT_STREAM_OVERLAP:   // 0 off, 1 on (the two passes), 2 passes + adapter branches, 3 adapter branches only, 4 forward passes only
            c->overlap = value != 0; c->ov_pass = value == 1 || value == 2 || value == 4; c->ov_branch = value == 2 || value == 3;
            c->ov_bwd_serial = value == 4;
            return DYT_OK;
        case DYT_OPT_CLS_TAIL: c->cls_tail = value != 0 && c->frames <= 1 && !c->ad_ln && !c->avg_pool; for (auto& S : c->slots) S.valid = false; return DYT_OK;
        case DYT_OPT_SHARE_BLOCK0: c->share_block0 = value != 0; return DYT_OK;
        case DYT_OPT_GRAD_SCALE_LOG2:   // 16-bit gradient operands carry 2^value (0 = none); fp32 mode ignores it
            if (value < 0 || value > 24) { set_error("grad scale log2 %d out of range 0..24", value); return DYT_ERR_ARG; }
            c->gs = (c->prec == DYT_PREC_FP32 && !c->bwd16) ? 1.0f : (float)(1u << value);
            return DYT_OK;
        case DYT_OPT_FC2_CAT: c->fc2_cat = value != 0; return DYT_OK;
        case DYT_OPT_F32_SPLIT16: {   // fp32 mode only: the frozen-weight GEMMs as hi*hi + hi*lo + lo*hi on the 16-bit matrix cores
            if (c->prec != 0) { set_error("DYT_OPT_F32_SPLIT16 applies to the fp32 mode"); return DYT_ERR_ARG; }
            if (value < 0 || value > 5) { set_error("DYT_OPT_F32_SPLIT16: value %d (0 off, 1 every product three-part, 2 gradient products one-part, 3 backward on 16-bit operands, 4 = 3 with fp8 correction products)", value); return DYT_ERR_ARG; }
            if (value != 0) { int rc = alloc_aux(c, value >= 3); if (rc) return rc; }
            c->split16 = value != 0;
            // 3 ("fp16x3h"): the forward as in 1 / 2 bit for bit, with what the backward needs saved in the 16-bit operand type (the hi
            // parts the forward computes anyway; ReLU / dropout / gate masks are the exact forward's), and the backward pass on the
            // 16-bit mode's data flow and kernels (fused attention backward, pre-shuffled-weight dgrads, 16-bit weight gradients)
            c->bwd16 = value >= 3;
            // 4 ("fp16f8"): the forward GEMMs' two correction products hi * lo + lo * hi on the fp8 matrix cores (twice the f16 rate per k:
            // 2K- instead of 3K-equivalent contractions; per-GEMM error ~2^-15 instead of 2^-20, logits ~5e-5 from the fp32 reference)
            c->f8 = value >= 4;
            // 5 ("fp16x3q"): only the attention branch's GEMMs (qkv, proj) that way -- the MLP's K = 3072 contractions and the GELU
            // between them carry most of the fp8 form's error: gate logits stay at the three-part level (emulated 1.0e-5 vs 4.4e-6 / 4.7e-5)
            c->f8_mask = value == 4 ? 31 : (value == 5 ? 3 : 0);
            // ... and the complete_model (teacher) pass of 5 takes the fp8-correction form for the MLP as well: its gate output is discarded, no
            // token-keep decision depends on it, only its logits (5e-5 from the reference instead of 7e-6) -- the dense pass is the heavier one
            c->f8_mask_complete = value == 4 ? 31 : (value == 5 ? 15 + 32 : 0);   // (32: that pass's attention forward as the hi * hi product alone)
            c->f8_mask_complete = (c->f8_mask_complete & ~16) | (c->f8_mask & 16);   // the patch embedding is shared between the passes
            c->gs = 1.0f;
#ifdef DYT_FP16
            if (c->bwd16) c->gs = 4096.0f;   // the fixed loss scale of the fp16 mode (dyt_ctx::gs)
#endif
            // 2 ("fp16x3f"): the forward (logits, gate decisions, losses, saved activations) as in 1; the gradient GEMMs contract
            // dY_hi * W_hi alone and the attention backward's dP / dQ / dK / dV take the hi * hi product (its score recomputation keeps three)
            c->split_bwd_parts = c->split_bwd_attn_parts = value == 2 ? 1 : 3;
            c->split_attn = c->bwd16 || split_attn_env();   // the 16-bit backward reads what the split attention kernel writes (planes, the per-layer proj operand image)
            for (auto& S : c->slots) S.valid = false;
            if (c->split16) {   // parts of the weights uploaded so far (later dyt_set_frozen calls refresh theirs)
                DYT_HIP_CHECK(hipDeviceSynchronize());   // uploads may be in flight on the caller's streams
                int rc = refresh_split(c, -1, nullptr);
                for (int l = 0; l < c->cfg.depth && !rc; ++l) { rc = refresh_split(c, l, nullptr); if (!rc) rc = refresh_bwd16(c, l, nullptr); }
                if (rc) return rc;
                DYT_HIP_CHECK(hipDeviceSynchronize());
            }
            return DYT_OK;
        }
        case DYT_OPT_ATTN_BWD_FUSED: set_attn_bwd_fused(value); return DYT_OK;   // process-wide
        case DYT_OPT_ATTN_V2: set_attn_v2(value & 3); return DYT_OK;             // process-wide
        case DYT_OPT_GEMM_SPLITK: set_gemm_splitk(value); return DYT_OK;         // process-wide
        case DYT_OPT_LEARNABLE_SCALE:
            // The scale words are the CALLER's (DYT_P_AD_SCALE of the flat trainable buffer handed to every call): a padding word -- zero -- until
            // the caller writes the reference's initial value 1.0 (models/dynamic_adapter.py:102).  Switching the meaning of that word between
            // passes would silently turn the adapters off (s = 0) or rescale them, so the option is fixed once a pass has run.
            if (value != 0 && c->ad_ln) { set_error("learnable adapter scale together with the adapter's LayerNorm option is not supported"); return DYT_ERR_ARG; }
            if ((value != 0) != c->learn_scale && c->pass_ran) {
                set_error("DYT_OPT_LEARNABLE_SCALE must be set before the first forward pass of the context");
                return DYT_ERR_STATE;
            }
            c->learn_scale = value != 0; for (auto& S : c->slots) S.valid = false; return DYT_OK;
        case DYT_OPT_COUNT_FLOPS_TOKENS:
            if (value < 0 || value > NT) { set_error("count_flops tokens %d out of range 0..197", value); return DYT_ERR_ARG; }
            c->count_flops_tokens = value; for (auto& S : c->slots) S.valid = false; return DYT_OK;
    }
    set_error("unknown option %d", option);
    return DYT_ERR_ARG;
}

extern "C" int dyt_set_drop_path(dyt_ctx* c, float rate) {
    if (!c) { set_error("null ctx"); return DYT_ERR_ARG; }
    if (!(rate >= 0.f) || rate >= 1.f) { set_error("drop_path rate %g out of [0, 1)", rate); return DYT_ERR_ARG; }
    if (rate > 0.f) { int rc = refuse_inference(c, "dyt_set_drop_path"); if (rc) return rc; }   // (training passes only)
    c->drop_path_rate = rate;
    return DYT_OK;
}
extern "C" int dyt_set_drop_path_scales(dyt_ctx* c, int slot, const float* scales) {
    if (!c) { set_error("null ctx"); return DYT_ERR_ARG; }
    if (slot < 0 || slot >= c->cfg.slots) { set_error("slot %d out of range", slot); return DYT_ERR_ARG; }
    if (scales) { int rc = refuse_inference(c, "dyt_set_drop_path_scales"); if (rc) return rc; }
    c->slots[c->inf ? 0 : slot].dp_inject = scales;
    return DYT_OK;
}

extern "C" int dyt_set_soft_targets(dyt_ctx* c, const float* targets, int rows) {
    if (!c) { set_error("null ctx"); return DYT_ERR_ARG; }
    if (targets && rows < 1) { set_error("soft targets: rows = %d", rows); return DYT_ERR_ARG; }
    if (targets) { int rc = refuse_inference(c, "dyt_set_soft_targets"); if (rc) return rc; }
    if (targets && c->mix_params) { set_error("dyt_set_soft_targets: mix is on (dyt_set_mix) and writes the class-probability targets itself"); return DYT_ERR_STATE; }
    c->soft_targets = targets; c->soft_batch = targets ? rows : 0;
    return DYT_OK;
}

extern "C" int dyt_set_global_option(int option, int value) {
    if (option == DYT_OPT_ATTN_BWD_FUSED) { set_attn_bwd_fused(value); return DYT_OK; }
    if (option == DYT_OPT_ATTN_V2) { set_attn_v2(value & 3); return DYT_OK; }
    if (option == DYT_OPT_GEMM_SPLITK) { set_gemm_splitk(value); return DYT_OK; }
    if (option == DYT_OPT_F32_SPLIT16) { set_attn_f32_split(value); return DYT_OK; }   // unit entry dyt_attention(precision 0): split forward kernel
    set_error("option %d is not process-wide", option);
    return DYT_ERR_ARG;
}

extern "C" int dyt_profile_enable(dyt_ctx* c, int on) {
    if (!c) { set_error("null ctx"); return DYT_ERR_ARG; }
    c->prof = on != 0;
    if (on) gemm_kernel_launch_count(1);
    return DYT_OK;
}
extern "C" int dyt_profile_read(dyt_ctx* c, int category, double* ms, int64_t* launches, double* flops) {
    if (!c || !ms || !launches || !flops) { set_error("null argument"); return DYT_ERR_ARG; }
    if (category == 3) {   // bf16 GEMM KERNEL launches since dyt_profile_enable(ctx, 1) (a GEMM may take two)
        *ms = 0; *flops = 0; *launches = gemm_kernel_launch_count(0);
        return DYT_OK;
    }
    DYT_HIP_CHECK(hipDeviceSynchronize());
    double t = 0, f = 0;
    int64_t n = 0;
    std::vector<ProfRec> keep;
    for (auto& r : c->recs) {
        if (r.cat != category) { keep.push_back(r); continue; }
        float e = 0.f;
        hipEventElapsedTime(&e, r.a, r.b);
        double fl = r.flops;
        if (r.m_dev && r.M > 0) {  // rows really processed (still holds the last step's count)
            int m = r.M;
            if (hipMemcpy(&m, r.m_dev, sizeof(int), hipMemcpyDeviceToHost) == hipSuccess && m < r.M) fl *= (double)m / r.M;
        }
        t += e; f += fl; ++n;
        c->pool.push_back(r.a); c->pool.push_back(r.b);
    }
    c->recs.swap(keep);
    *ms = t; *launches = n; *flops = f;
    return DYT_OK;
}

extern "C" int dyt_seed(dyt_ctx* c, uint64_t seed, void* stream) {
    if (!c) { set_error("null ctx"); return DYT_ERR_ARG; }
    return launch_seed_set(c->seed_dev, seed, static_cast<hipStream_t>(stream));
}

extern "C" int dyt_grad_part(const dyt_ctx* c, int part, int64_t* offset, int64_t* numel) {
    if (!c || !offset || !numel || part < 0 || part > 1) { set_error("bad argument"); return DYT_ERR_ARG; }
    const int64_t up_off = (int64_t)(c->cfg.depth / 2) * c->layer_stride;
    if (part == 0) { *offset = up_off; *numel = c->n_train - up_off; }
    else { *offset = 0; *numel = up_off; }
    return DYT_OK;
}
