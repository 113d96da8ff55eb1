// Which kernel an attention launch gets: two pure functions of the few properties of the call and of the process-wide switches the
// decision reads.  No HIP here: attention.hip fills a shape (copying the switches in), refuses with the route's error, and switches over
// the kernel id to the family unit that launches it (attention_16.hip, attention_exact.hip, attention_split.hip, attention_v2.hip); tools/attn_route_check.cpp walks the same functions on the CPU (tests/test_attn_route_host.py).
#pragma once

namespace dyt {

enum AttnFwdKernel {
    AF_ERROR,
    AF_SPLIT_F32, AF_SPLIT_F32_NOSAVE,   // attn_fwd_split_kernel<false>: fp32 q / k / v, three 16-bit products ("fp16x3" / "fp16x3f", the unit entry)
    AF_SPLIT_P3, AF_SPLIT_P3_NOSAVE,     // ... <true>: planar q / k / v, three products ("fp16x3h" / "fp16f8", the "fp16x3q" student pass)
    AF_SPLIT_P1, AF_SPLIT_P1_NOSAVE,     // ... <true, 1>: planar, hi * hi alone, for a caller that needs more than the operand image
    AF_EXACT,                            // attn_fwd_f32_kernel (no no-save variant)
    AF_16,                               // attn_fwd_bf16_kernel, the round-4 16-bit kernel (no no-save variant)
    AF_V2, AF_V2_NOSAVE,                 // av2::attn_fwd_v2_kernel, the round-5 16-bit kernel
    AF_V2_F8, AF_V2_F8_NOSAVE,           // ... on the hi planes, writing the proj GEMM's operand image in the hi16 / fp8 form (one-part teacher attention)
};
enum AttnBwdKernel {
    AB_ERROR,
    AB_SPLIT3, AB_SPLIT1,            // attn_bwd_dq_split_kernel + attn_bwd_dkv_split_kernel <3> / <1>
    AB_EXACT,                        // attn_bwd_dq_f32_kernel + attn_bwd_dkv_f32_kernel
    AB_16_TWO,                       // attn_bwd_dq_bf16_kernel + attn_bwd_dkv_bf16_kernel
    AB_16_FUSED, AB_16_FUSED_AHEAD,  // attn_bwd_fused_bf16_kernel<false> / <true> (row prefetch a head ahead)
    AB_V2,                           // av2::attn_bwd_v2_kernel
};

struct AttnFwdShape {
    int precision = 0;           // 0: fp32 q / k / v (or their planes), else the 16-bit operand type
    bool split = false;          // the call's split16 or the process-wide DYT_OPT_F32_SPLIT16
    bool out = false, out3 = false;   // which outputs the caller gave
    bool planes = false;         // q / k / v as hi + lo planes
    bool saved = false;          // 16-bit copies of q / k / v asked for
    bool o16 = false;            // ... of the output
    bool out3_f8 = false;
    int parts = 3;
    bool lse_optional = false;   // the caller does not read lse
    int v2 = 3;                  // DYT_OPT_ATTN_V2
};
struct AttnBwdShape {
    int precision = 0;
    bool split = false;
    int grad_parts = 3;
    bool out_strided = false;    // `out` is the hi plane of a split operand image
    int v2 = 3;                  // DYT_OPT_ATTN_V2
    int fused = 1;               // DYT_OPT_ATTN_BWD_FUSED
};

struct AttnFwdRoute {
    AttnFwdKernel kernel;
    bool store_lse;      // false: the kernel gets a null lse (a *_NOSAVE instance)
    const char* error;   // AF_ERROR: what the call violates
};
struct AttnBwdRoute {
    AttnBwdKernel kernel;
    const char* error;
};

inline AttnFwdRoute attn_fwd_route(const AttnFwdShape& a) {
    const auto error = [](const char* what) { return AttnFwdRoute{AF_ERROR, true, what}; };
    const auto pick = [&a](AttnFwdKernel save, AttnFwdKernel nosave) { return AttnFwdRoute{a.lse_optional ? nosave : save, !a.lse_optional, nullptr}; };
    const bool split = a.precision == 0 && a.split;
    if ((a.planes || a.saved || a.o16 || !a.out) && !split) return error("attention forward: 16-bit copies / no fp32 output need the split kernel");
    if (!a.out && !a.out3) return error("attention forward: no output");
    if (split) {
        if (a.parts != 3 && !(a.planes && a.parts == 1)) return error("attention forward: the one-part form needs the planar q / k / v");
        if (a.planes && a.parts == 1) {
            // nothing but the operand image to write (every block of a complete_model pass but the cls-only last one): the round-5 16-bit
            // kernel on the hi planes, its result split on the way out (DYT_OPT_ATTN_V2 bit 0)
            if (!a.out && a.out3_f8 && !a.o16 && (a.v2 & 1)) return pick(AF_V2_F8, AF_V2_F8_NOSAVE);
            return pick(AF_SPLIT_P1, AF_SPLIT_P1_NOSAVE);
        }
        return a.planes ? pick(AF_SPLIT_P3, AF_SPLIT_P3_NOSAVE) : pick(AF_SPLIT_F32, AF_SPLIT_F32_NOSAVE);
    }
    if (a.precision == 0) {
        if (a.out3) return error("attention forward: split output without the split kernel");
        return AttnFwdRoute{AF_EXACT, true, nullptr};
    }
    if (a.v2 & 1) return pick(AF_V2, AF_V2_NOSAVE);
    return AttnFwdRoute{AF_16, true, nullptr};
}

inline AttnBwdRoute attn_bwd_route(const AttnBwdShape& a) {
    const auto to = [](AttnBwdKernel k) { return AttnBwdRoute{k, nullptr}; };
    if (a.precision == 0) {
        if (a.out_strided) return AttnBwdRoute{AB_ERROR, "attention backward: a strided `out` is a 16-bit-kernel feature"};
        if (a.split) return to(a.grad_parts >= 3 ? AB_SPLIT3 : AB_SPLIT1);
        return to(AB_EXACT);
    }
    if (a.v2 & 2) return to(AB_V2);
    if (a.fused) return to(a.fused == 2 ? AB_16_FUSED_AHEAD : AB_16_FUSED);
    return to(AB_16_TWO);
}

}  // namespace dyt
