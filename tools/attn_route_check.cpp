// CPU walk of the attention routing (dynamic-tuning_amd/csrc/attn_route.h) -- which kernel an attention launch gets, checked without a GPU.
//   * a table of every configuration a call site produces, one row per (mode, pass, position), with the kernel it must get.  The rows are
//     read off forward_impl / backward_impl / attention_test (what each sets for the mode), not off the routing function;
//   * over the full cross product of the shapes' fields: an error if and only if a documented precondition is violated, lse dropped only on
//     an instance with a no-save variant, no round-5 kernel with its DYT_OPT_ATTN_V2 bit cleared, no 16-bit-input kernel at precision 0,
//     the one-part instances only on planes.
// Build and run (host only):
//   c++ -std=c++17 -O2 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I dynamic-tuning_amd/csrc
//     tools/attn_route_check.cpp -o /tmp/attn_route_check && /tmp/attn_route_check
#include <cstdio>
#include <cstdlib>

#include "attn_route.h"

using namespace dyt;

static const char* gRow = "";
#define CHECK(cond)                                                                             \
    do {                                                                                        \
        if (!(cond)) {                                                                          \
            fprintf(stderr, "%s:%d: CHECK(%s) failed (%s)\n", __FILE__, __LINE__, #cond, gRow); \
            abort();                                                                            \
        }                                                                                       \
    } while (0)

// forward_impl: split = split16 && split_attn; planes = bwd16 && split; out3 = split; out dropped when the pass is saved for a 16-bit
// backward (planes) except on the cls-tail proj block; out3_f8 = f8_mask bit 1; parts = 1 for planes under f8_mask bit 5; lse optional = inference
static AttnFwdShape fwd(int precision, bool split, bool planes, bool out, bool out3_f8, int parts, bool inference, int v2) {
    AttnFwdShape a;
    a.precision = precision; a.split = split; a.out3 = split; a.planes = planes; a.out = out; a.out3_f8 = out3_f8; a.parts = parts;
    a.lse_optional = inference; a.v2 = v2;
    return a;
}
static void expect(const char* row, const AttnFwdShape& a, AttnFwdKernel kernel, bool store_lse) {
    gRow = row;
    const AttnFwdRoute r = attn_fwd_route(a);
    CHECK(r.kernel == kernel && r.store_lse == store_lse && r.error == nullptr);
}
// backward_impl: a pass saved in 16 bits runs at precision 1 with the strided `out`; else split = split16 && split_attn
static void expect(const char* row, int precision, bool split, int grad_parts, bool strided, int v2, int fused, AttnBwdKernel kernel) {
    gRow = row;
    AttnBwdShape a;
    a.precision = precision; a.split = split; a.grad_parts = grad_parts; a.out_strided = strided; a.v2 = v2; a.fused = fused;
    const AttnBwdRoute r = attn_bwd_route(a);
    CHECK(r.kernel == kernel && (kernel == AB_ERROR) == (r.error != nullptr));
}

static void call_sites() {
    //                                                  prec split planes out   f8     parts inference v2
    expect("fp16 / bf16 training", fwd(1, false, false, true, false, 3, false, 3), AF_V2, true);
    expect("fp16 / bf16 inference-only", fwd(1, false, false, true, false, 3, true, 3), AF_V2_NOSAVE, false);
    expect("fp16 / bf16 training, v2 bit 0 off", fwd(1, false, false, true, false, 3, false, 2), AF_16, true);
    expect("fp16 / bf16 inference-only, v2 bit 0 off", fwd(1, false, false, true, false, 3, true, 2), AF_16, true);
    expect("fp32", fwd(0, false, false, true, false, 3, false, 3), AF_EXACT, true);
    expect("fp32 inference-only", fwd(0, false, false, true, false, 3, true, 3), AF_EXACT, true);
    expect("fp16x3 / fp16x3f with DYT_SPLIT_ATTN=0", fwd(0, false, false, true, false, 3, false, 3), AF_EXACT, true);
    expect("fp16x3 / fp16x3f", fwd(0, true, false, true, false, 3, false, 3), AF_SPLIT_F32, true);
    expect("fp16x3 / fp16x3f inference-only", fwd(0, true, false, true, false, 3, true, 3), AF_SPLIT_F32_NOSAVE, false);
    expect("fp16x3h saved pass", fwd(0, true, true, false, false, 3, false, 3), AF_SPLIT_P3, true);
    expect("fp16x3h saved pass, cls-tail proj block / unsaved pass", fwd(0, true, true, true, false, 3, false, 3), AF_SPLIT_P3, true);
    expect("fp16f8, fp16x3q student, saved pass", fwd(0, true, true, false, true, 3, false, 3), AF_SPLIT_P3, true);
    expect("fp16f8 cls-tail proj block; fp16f8, fp16x3q student, unsaved pass", fwd(0, true, true, true, true, 3, false, 3), AF_SPLIT_P3, true);
    expect("fp16x3q teacher", fwd(0, true, true, false, true, 1, false, 3), AF_V2_F8, true);
    expect("fp16x3q teacher, v2 bit 0 off", fwd(0, true, true, false, true, 1, false, 2), AF_SPLIT_P1, true);
    expect("fp16x3q teacher, cls-tail last block / unsaved pass", fwd(0, true, true, true, true, 1, false, 3), AF_SPLIT_P1, true);
    expect("dyt_attention fp32", fwd(0, false, false, true, false, 3, false, 3), AF_EXACT, true);
    {   // ... with the process-wide split option: no split output
        AttnFwdShape a = fwd(0, true, false, true, false, 3, false, 3);
        a.out3 = false;
        expect("dyt_attention fp32, DYT_OPT_F32_SPLIT16", a, AF_SPLIT_F32, true);
    }
    expect("dyt_attention 16-bit", fwd(1, false, false, true, false, 3, false, 3), AF_V2, true);
    expect("dyt_attention 16-bit, v2 bit 0 off", fwd(1, false, false, true, false, 3, false, 0), AF_16, true);

    //                                    prec split parts strided v2 fused
    expect("16-bit backward", 1, false, 3, false, 3, 1, AB_V2);
    expect("16-bit backward, v2 bit 1 off", 1, false, 3, false, 1, 1, AB_16_FUSED);
    expect("16-bit backward, v2 bit 1 off, fused 2", 1, false, 3, false, 1, 2, AB_16_FUSED_AHEAD);
    expect("16-bit backward, v2 bit 1 off, two kernels", 1, false, 3, false, 1, 0, AB_16_TWO);
    expect("fp16x3 backward", 0, true, 3, false, 3, 1, AB_SPLIT3);
    expect("fp16x3f backward", 0, true, 1, false, 3, 1, AB_SPLIT1);
    expect("fp32 backward", 0, false, 3, false, 3, 1, AB_EXACT);
    expect("fp16x3 / fp16x3f backward with DYT_SPLIT_ATTN=0 (dqkv3 from the exact kernels)", 0, false, 3, false, 3, 1, AB_EXACT);
    expect("bwd16 (fp16x3h / fp16f8 / fp16x3q) backward", 1, false, 3, true, 3, 1, AB_V2);
    expect("bwd16 backward, v2 bit 1 off", 1, false, 3, true, 0, 1, AB_16_FUSED);
    expect("a strided out at precision 0", 0, false, 3, true, 3, 1, AB_ERROR);
    expect("dyt_attention fp32 backward, DYT_OPT_F32_SPLIT16", 0, true, 3, false, 3, 1, AB_SPLIT3);
}

static void sweep() {
    gRow = "sweep";
    long long n = 0;
    for (int bits = 0; bits < 512; ++bits)
        for (int parts = 1; parts <= 3; ++parts)
            for (int v2 = 0; v2 < 4; ++v2) {
                AttnFwdShape a;
                a.precision = bits & 1; a.split = bits & 2; a.out = bits & 4; a.out3 = bits & 8; a.planes = bits & 16; a.saved = bits & 32;
                a.o16 = bits & 64; a.out3_f8 = bits & 128; a.lse_optional = bits & 256; a.parts = parts; a.v2 = v2;
                const AttnFwdRoute r = attn_fwd_route(a);
                const AttnFwdKernel k = r.kernel;
                const bool split = a.precision == 0 && a.split;
                const bool violated = ((a.planes || a.saved || a.o16 || !a.out) && !split) || (!a.out && !a.out3) ||
                                      (split && a.parts != 3 && !(a.planes && a.parts == 1)) || (a.precision == 0 && !split && a.out3);
                CHECK((k == AF_ERROR) == violated && (k == AF_ERROR) == (r.error != nullptr));
                const bool nosave = k == AF_SPLIT_F32_NOSAVE || k == AF_SPLIT_P3_NOSAVE || k == AF_SPLIT_P1_NOSAVE || k == AF_V2_NOSAVE || k == AF_V2_F8_NOSAVE;
                CHECK(r.store_lse == !nosave);
                if (!a.lse_optional) CHECK(r.store_lse);
                const bool v2k = k == AF_V2 || k == AF_V2_NOSAVE || k == AF_V2_F8 || k == AF_V2_F8_NOSAVE;
                if (!(a.v2 & 1)) CHECK(!v2k);
                const bool in16 = k == AF_16 || k == AF_V2 || k == AF_V2_NOSAVE;
                if (k != AF_ERROR) CHECK(in16 == (a.precision != 0));
                const bool one_part = k == AF_SPLIT_P1 || k == AF_SPLIT_P1_NOSAVE || k == AF_V2_F8 || k == AF_V2_F8_NOSAVE;
                if (one_part) CHECK(a.planes && a.parts == 1 && split);
                if (k == AF_SPLIT_P3 || k == AF_SPLIT_P3_NOSAVE) CHECK(a.planes);
                ++n;
            }
    for (int precision = 0; precision < 2; ++precision)
        for (int bits = 0; bits < 4; ++bits)
            for (int parts = 1; parts <= 3; ++parts)
                for (int v2 = 0; v2 < 4; ++v2)
                    for (int fused = 0; fused < 3; ++fused) {
                        AttnBwdShape a;
                        a.precision = precision; a.split = bits & 1; a.out_strided = bits & 2; a.grad_parts = parts; a.v2 = v2; a.fused = fused;
                        const AttnBwdRoute r = attn_bwd_route(a);
                        const AttnBwdKernel k = r.kernel;
                        CHECK((k == AB_ERROR) == (precision == 0 && a.out_strided) && (k == AB_ERROR) == (r.error != nullptr));
                        if (!(v2 & 2)) CHECK(k != AB_V2);
                        const bool in16 = k == AB_16_TWO || k == AB_16_FUSED || k == AB_16_FUSED_AHEAD || k == AB_V2;
                        if (k != AB_ERROR) CHECK(in16 == (precision != 0));
                        ++n;
                    }
    printf("attn route check: %lld shapes, invariants hold\n", n);
}

int main() {
    call_sites();
    printf("attn route check: call-site routes ok\n");
    sweep();
    return 0;
}
