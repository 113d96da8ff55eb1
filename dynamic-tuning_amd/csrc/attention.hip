// Multi-head self-attention for the DyT ViT-B/16 path: N = 197 tokens, 12 heads x 64.
// Replaces Attention.forward's F.scaled_dot_product_attention / explicit softmax
// (models/vision_transformer_IN21K.py:60-70 of the reference) and its autograd backward.
//
// This unit holds the process-wide switches and the two launchers: they fill the route's shape, ask attn_route.h which kernel the
// call gets, refuse with the route's error and hand over to the one family that owns that kernel:
//   attention_16.hip     the round-4 16-bit kernels (bf16 / fp16 operands; DYT_OPT_ATTN_V2 bits cleared)
//   attention_exact.hip  fp32 operands on the matrix cores: the fp32 mode
//   attention_split.hip  fp32 operands as 16-bit hi / lo parts: the parity modes
//   attention_v2.hip     the round-5 16-bit kernels (the default of the 16-bit modes)
// The layout notes of each family stand at the head of its unit; what more than one family uses is attn_common.h.
#include "attn_common.h"

namespace dyt {

// ------------------------------------------------------------------------------------------
// The process-wide switches the launchers read (C ABI: dyt_set_option / dyt_set_global_option); copied into the route's shape
struct AttnSwitches {
    int f32_split = 0;   // DYT_OPT_F32_SPLIT16: the split forward kernel for every fp32-mode call (unit entries; contexts pass their own flag)
    int v2 = -1;         // DYT_OPT_ATTN_V2; -1: not set yet -> DYT_ATTN_V2 from the environment (default 3: both round-5 kernels)
    int bwd_fused = 1;   // DYT_OPT_ATTN_BWD_FUSED
};
static AttnSwitches g_attn;
void set_attn_f32_split(int on) { g_attn.f32_split = on; }
void set_attn_v2(int mask) { g_attn.v2 = mask; }
void set_attn_bwd_fused(int on) { g_attn.bwd_fused = on; }
static int attn_v2_mask() {
    if (g_attn.v2 < 0) { const char* e = getenv("DYT_ATTN_V2"); g_attn.v2 = e ? (atoi(e) & 3) : 3; }
    return g_attn.v2;
}

int launch_attn_fwd(int precision, const AttnFwdArgs& a, hipStream_t s) {
    if (dbg_skip(2)) return 0;
    AttnFwdShape sh;
    sh.precision = precision; sh.split = a.split16 || g_attn.f32_split; sh.out = a.out != nullptr; sh.out3 = a.out3 != nullptr; sh.planes = a.planar;
    sh.saved = a.q16 || a.k16 || a.v16; sh.o16 = a.o16 != nullptr; sh.out3_f8 = a.out3_f8; sh.parts = a.parts; sh.lse_optional = a.lse_optional;
    sh.v2 = attn_v2_mask();
    const AttnFwdRoute r = attn_fwd_route(sh);
    if (r.error) { set_error("%s", r.error); return -1; }
    if (r.store_lse && !a.lse) { set_error("attention forward: this kernel writes lse"); return -1; }
    switch (r.kernel) {
        case AF_SPLIT_F32: case AF_SPLIT_P3: case AF_SPLIT_P1:
        case AF_SPLIT_F32_NOSAVE: case AF_SPLIT_P3_NOSAVE: case AF_SPLIT_P1_NOSAVE: return launch_attn_fwd_split(a, r, s);
        case AF_EXACT: return launch_attn_fwd_exact(a, s);
        case AF_16: return launch_attn_fwd_16(a, s);
        default: return launch_attn_fwd_v2(a, r, s);
    }
}

int launch_attn_bwd(int precision, const AttnBwdArgs& a, hipStream_t s) {
    if (dbg_skip(1)) return 0;
    const int out_ld = a.out_ld > 0 ? a.out_ld : D;
    AttnBwdShape sh;
    sh.precision = precision; sh.split = a.split16 || g_attn.f32_split; sh.grad_parts = a.grad_parts; sh.out_strided = out_ld != D;
    sh.v2 = attn_v2_mask(); sh.fused = g_attn.bwd_fused;
    const AttnBwdRoute r = attn_bwd_route(sh);
    if (r.error) { set_error("%s", r.error); return -1; }
    switch (r.kernel) {
        case AB_SPLIT3: case AB_SPLIT1: return launch_attn_bwd_split(a, r, s);
        case AB_EXACT: return launch_attn_bwd_exact(a, s);
        case AB_16_TWO: case AB_16_FUSED: case AB_16_FUSED_AHEAD: return launch_attn_bwd_16(a, r, out_ld, s);
        default: return launch_attn_bwd_v2(a, s);
    }
}

}  // namespace dyt
