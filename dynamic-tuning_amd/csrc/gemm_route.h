// Which kernel and tile shape a GEMM gets: one pure function of the shape and of the few operand properties the decision reads.
// No HIP here: gemm.hip fills a GemmShape, switches over the GemmRoute and launches; tools/gemm_route_check.cpp walks the same function
// on the CPU (tests/test_gemm_route_host.py, tests/golden/gemm_routes.json).  The measurements behind each rule: DESIGN.md 7.
#pragma once

namespace dyt {

constexpr int SK_SLICE = 256;   // split-K (gemm_skinny.h): k per workgroup, 16 MFMA steps of 32x32x16
constexpr int SK_MAX_M = 512;   // above this the 128x128 tiles fill enough CUs and the partials' round trip costs more than it saves
constexpr int ROUTE_NCU = 256;        // compute units: a round of one-per-CU 256x256 workgroups
constexpr int ROUTE_BIG_N = 2304;     // N >= this (and % 256 == 0): wide enough for 256-column tiles in every row
constexpr int ROUTE_BIG_M = 2048;     // fewer rows than this: 128x128 tiles
constexpr int ROUTE_SHORT_K = 768;    // K <= this: 12 k-steps, the launch is bound by its prologue / epilogue, not by its main loop
constexpr int ROUTE_BPRE_STORE_MAX_K = 3072;   // plain-store N = 768 GEMMs up to this K take the pre-shuffled-weight kernel (qkv / fc1 dgrads)

enum GemmFamily { GF_16, GF_F8, GF_F32 };   // 16-bit MFMA kernels; their f16 + fp8-correction form (K = 2 x the logical K); the exact-fp32 kernels
enum GemmKernel {
    GK_ERROR,
    GK_SPLITK,       // split-K over 256-wide slices + a reduce launch that runs the epilogue (gemm_skinny.h)
    GK_BPRE,         // pre-shuffled-weight kernel, 128x256 tiles (gemm_bpre.h)
    GK_256,          // 256x256 tiles on rows [0, body); 128x128 tiles on rows [body, M) when body < M (the whole-rounds scheme)
    GK_128,          // 128x128 tiles
    GK_128x64,       // 128x64 tiles
    GK_F32_128,      // exact-fp32 MFMA kernel, 128x128
    GK_F32_128x64,   // ... 128x64
};

struct GemmShape {
    int M = 0, N = 0, K = 0;
    GemmFamily family = GF_16;
    bool cat = false;           // the K-concatenated form: a second operand pair as the leading k-tile
    bool lead = false;          // ... as three leading tiles of a three-part product
    bool wp = false;            // a pre-shuffled copy of the weight exists
    bool store_epi = false;     // the epilogue is the plain 16-bit store
    bool a_map = false;         // the A rows are gathered
    bool a_ld = false;          // A is a split [hi | lo] operand
    bool a_fold = false;        // ... contracted as more than one part
    bool m_dev = false;         // the valid row count lives on the device (never changes the route: workgroups beyond it exit early)
    bool a2 = false, w2 = false;   // the second operand pair
    bool splitk_fits = false;   // the epilogue has the split-K form, it is switched on and the lent workspace holds splitk_slices() x M x N floats
    int f8_begin = 0;           // GF_F8: index of the first fp8 k-tile
};

struct GemmRoute {
    GemmKernel kernel;
    int body;            // rows [0, body) go to `kernel`; body < M (GK_256 only): rows [body, M) get a second launch of 128x128 tiles
    const char* error;   // GK_ERROR: what the shape or the operands violate
};

// workgroups of a launch of BM x BN tiles over rows [m_begin, m_end)
inline int tile_grid(int m_begin, int m_end, int N, int BM, int BN) { return ((m_end - m_begin + BM - 1) / BM) * (N / BN); }
inline int splitk_slices(int K, bool cat) { return K / SK_SLICE + (cat ? 1 : 0); }

// Narrow-N GEMMs (N = 768): per row, 256x256 tiles are ~1.6x cheaper than 128x128 tiles (half the L2->LDS bytes per FLOP), but 99 x 3 = 297
// tiles leave 41 for a second round.  The rows that fill whole rounds of the CUs get 256x256 tiles, the remaining rows 128x128 tiles, as two
// launches on the same stream.  Both kernels accumulate every dot product in the same k order, so results do not depend on where the split
// falls.  Returns the first row of the 128x128 tail: M = one 256x256 launch (the last round is full or at least 3/4 full), -1 = not even 3/4
// of one round: no 256x256 tiles at all.  Measured in the step: 28.5 vs 29.1 ms (all-128x128) vs 28.8 ms (all-256x256, two rounds).
inline int whole_rounds_body(int M, int N) {
    const int tn = N / 256, t256 = ((M + 255) / 256) * tn, rounds = t256 / ROUTE_NCU, rem = t256 - rounds * ROUTE_NCU;
    if (rounds < 1 && rem < 3 * ROUTE_NCU / 4) return -1;
    if (rem == 0 || rem >= 3 * ROUTE_NCU / 4) return M;
    return (rounds * ROUTE_NCU / tn) * 256;
}

inline GemmRoute gemm_route(const GemmShape& g) {
    const auto all = [&g](GemmKernel k) { return GemmRoute{k, g.M, nullptr}; };
    const auto error = [](const char* what) { return GemmRoute{GK_ERROR, 0, what}; };
    const bool wide = g.N % 256 == 0 && g.N >= ROUTE_BIG_N && g.M >= ROUTE_BIG_M;
    if (g.family == GF_F32) {
        if (g.K % 64 != 0 || g.N % 64 != 0 || g.M <= 0) return error("gemm_f32: N % 64, K % 64 and M > 0 required");
        return all(g.N % 128 == 0 ? GK_F32_128 : GK_F32_128x64);
    }
    if (g.family == GF_F8) {   // tile shapes as for the three-part form; the 256x256 fp8 kernel takes no row gather
        if (g.K % 256 != 0 || g.M <= 0 || g.N % 128 != 0 || g.f8_begin * 128 != g.K) return error("gemm f8 form: K % 256, N % 128, M > 0 and K / 2 of f16 tiles required");
        if (g.lead && (!g.a2 || !g.w2)) return error("gemm f8 form: leading tiles need A2 and W2");
        if (wide && !g.a_map) return all(GK_256);
        // logical K <= 768, N = 768 (proj forward of the split modes): like the 16-bit modes' proj below -- one launch of 128x128 tiles, two
        // workgroups per CU, instead of a 256x256 body + a 128x128 row tail
        if (g.K <= 2 * ROUTE_SHORT_K && g.N < ROUTE_BIG_N) return all(GK_128);
        if (g.N % 256 == 0 && !g.a_map) {
            const int body = whole_rounds_body(g.M, g.N);
            if (body >= 0) return GemmRoute{GK_256, body, nullptr};
        }
        return all(GK_128);
    }
    if (g.K % 64 != 0 || g.M <= 0) return error("gemm_bf16: K % 64 and M > 0 required");
    // the K = 3072 GEMMs of the cls-only last block (B = 128, serial: fc2 forward 56 -> see DESIGN.md 7d); DYT_OPT_GEMM_SPLITK 0 keeps the 6-tile launches
    if (g.splitk_fits && g.M <= SK_MAX_M && g.K >= 1024 && g.K % SK_SLICE == 0 && g.N % 64 == 0 && !g.m_dev && !g.a_fold && !g.a_ld && (!g.cat || (g.a2 && g.w2)))
        return all(GK_SPLITK);
    const bool plain = !g.cat && !g.lead;
    if (g.cat) {
        // (Round 6: this form through the pre-shuffled-weight kernel -- the leading tile in its prologue's DMA round, bit-identical results -- measured
        // 175 us serial against 123 + 28 us here and 23.4 vs 23.2 ms in the step: the fp32 read-modify-write epilogue of a 128x256 tile does not fit
        // beside 128 accumulators -- 20-37 spilled registers.  Not kept; profiles/round6/r6_fc2_bpre_ab.txt.)
        if (!g.a2 || !g.w2 || g.N % 128 != 0) return error("gemm_bf16: the K-concatenated form needs A2, W2 and N % 128 == 0");
    } else if (g.lead) {
        if (!g.a2 || !g.w2 || g.N % 128 != 0 || !g.a_fold) return error("gemm_bf16: leading three-part tiles need A2, W2, the split form and N % 128 == 0");
    } else {
        if (g.a2) return error("gemm_bf16: this epilogue has no K-concatenated form");
        // Wide-N GEMMs against a frozen weight: the pre-shuffled-weight kernel (128x256 tiles, two workgroups per CU, the weight never touches
        // LDS).  In the step: 28.10 vs 28.40 ms with the 256x256 kernel.  Plain-store N = 768 GEMMs take it as well.  K = 768 (proj dgrad): with
        // only 12 k-steps the 256x256 kernel's exposed prologue / epilogue (one workgroup per CU) weighs most, 45 vs 53.5 us serial.  K = 2304 /
        // 3072 (qkv dgrad, fc1 dgrad): slower in the serial profile (GEMM family 20.2 -> 20.7 ms per step), but the step is 23.85 vs 24.3 ms
        // same-box: 64 KB workgroups share CUs with the other pass's kernels, and the four-slot ring loses less on operands that come from HBM
        // (tools/gemm_bench.py COLD=1: +22 % vs +42 %).  Not the residual epilogues: 81.7 vs 73.3 us for the proj forward, and the row kernels
        // that read its fp32 output right after it got slower.
        if (g.wp && g.N % 256 == 0 && g.K % 256 == 0 && g.M >= ROUTE_BIG_M && (g.N >= ROUTE_BIG_N || (g.store_epi && g.K <= ROUTE_BPRE_STORE_MAX_K)))
            return all(GK_BPRE);
        // one-part split GEMMs with a wide N (GELU' dgrad of "fp16x3f": 12 k-tiles against an epilogue that reads gelu' and writes dZ): the
        // 256x256 kernel's exposed epilogue outweighs its main loop -> 128x128 tiles, two workgroups per CU
        if (g.a_ld && g.K <= ROUTE_SHORT_K && g.N >= ROUTE_BIG_N && g.N % 128 == 0) return all(GK_128);
    }
    if (wide) return all(GK_256);
    // K <= 768, N = 768 with a residual epilogue (proj forward, patch embedding): 12 k-steps against an epilogue that moves 194 MB -- the launch
    // is bound by its epilogue traffic, and 1182 tiles of 128x128 on 512 slots interleave main loops and epilogues where 255 big tiles run them
    // as two chip-wide phases: 74.6 vs 59 + 20.5 us (256x256 body + 128x128 row tail), step 24.98 vs 25.03 ms same-box, one launch instead of
    // two; same k order, same bits
    if (plain && g.K <= ROUTE_SHORT_K && g.N % 128 == 0 && g.M >= ROUTE_BIG_M && !g.a_ld) return all(GK_128);
    if (g.N % 256 == 0 && g.K >= 256) {
        const int body = whole_rounds_body(g.M, g.N);
        if (body >= 0) return GemmRoute{GK_256, body, nullptr};
    }
    if (g.N % 128 == 0) return all(GK_128);
    if (plain && g.N % 64 == 0) return all(GK_128x64);
    return error("gemm_bf16: N must be a multiple of 64 (128 in the K-concatenated forms)");
}

}  // namespace dyt
