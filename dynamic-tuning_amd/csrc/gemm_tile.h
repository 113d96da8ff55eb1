// C[M,N] = A[M,K] @ W[N,K]^T on 16-bit operands staged through LDS (included by gemm.hip): the tile function and its kernel.
#pragma once

namespace dyt {

// ------------------------------------------------------------------------------------------
// bf16 MFMA kernel
// ------------------------------------------------------------------------------------------
// LDS-DMA (global_load_lds) completion is tracked by vmcnt.  hipcc usually drains it before a
// __syncthreads(), but NOT reliably (the software-pipelined loop below was compiled with only
// lgkmcnt(0) in front of s_barrier -> stale tiles at full occupancy).  Every barrier that publishes
// DMA'd data is therefore preceded by this explicit wait.
__device__ __forceinline__ void dma_wait_all() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// phase timers (measurement builds only, ABL == 9): cycles of prologue / main loop / epilogue summed over
// workgroups (wave 0 lane 0), [3] = workgroups counted
__device__ unsigned long long g_gemm_dbg[4];

// Tile BM x BN x 64, WAVES_M x WAVES_N waves of 64 lanes (each wave owns a (BM/WAVES_M) x (BN/WAVES_N)
// block of 16x16 MFMA tiles).  Shipped configurations:
//   128x128, 2x2 waves, 64 KB LDS, 2 workgroups / CU  -- N = 768 GEMMs (tile quantisation) and default
//   256x256, 2x4 waves, 128 KB LDS, 1 workgroup / CU  -- wide-N GEMMs: half the L2->LDS bytes per FLOP
//   128x64,  2x2 waves                                 -- adapter bottleneck (N = 64)
// ABL: 0 = product, 9 = the same kernel with the three phase timers (tools/gemm_bench.py)
// CAT: the contraction gets ONE extra leading k-tile taken from a second operand pair -- A2 [rows, 64] (rows optionally
// gathered through a2_map) against W2 [N, 64] -- i.e. C = A2 W2^T + A W^T in one accumulator chain (adapter up-projection
// riding on the fc2 GEMM: K = 64 + 3072).  The extra tile is stage 0 of the ring, so the main loop, its pointer
// registers and its schedule are the plain kernel's (the A / W pointers are pre-decremented by one tile).
struct CatArgs {
    const bf16* A2;      // CAT / LEAD: the second operand pair's activations ...
    const bf16* W2;      // ... and weights
    const int* a2_map;   // optional row gather of A2
    float out_scale;     // accumulators x this before the epilogue functor (split fp32 form; 1 elsewhere)
    // k-tiles of ONE part of split operands stored [hi | lo] (row stride K - a_fold * 64): k-tile kt reads A column tile
    // kt - (kt >= a_fold ? a_fold : 0) and W column tile kt - (kt >= 2 a_fold ? 2 a_fold : 0), i.e. [A_hi | A_hi | A_lo] x [W_hi | W_lo | W_hi]; 0 = plain
    int a_fold;
    int a_ld;            // row stride of split operands when the contraction runs over fewer than three parts (0: K - a_fold * 64)
    int f8_begin;        // F8 kernels: first fp8 k-tile
    const int* w_exp;    // F8 kernels: device word with the weight image's exponent
};
// LEAD (split fp32 forms, round 6): the second operand pair as THREE leading k-tiles of a three-part product -- A2 [rows][hi 64 | lo 64] (rows
// optionally gathered through a2_map), W2 [N][hi 64 | lo 64]: tiles (A2_hi, W2_hi), (A2_hi, W2_lo), (A2_lo, W2_hi) -- contracted into the
// accumulators by a small synchronous loop BEFORE the pipelined main loop starts (stage, wait, barrier, 2 x TM x TN MFMAs, barrier), so the
// main loop -- three-part fold form or fp8-correction form -- its registers and its schedule stay exactly the plain kernel's.  Three exposed
// tile latencies per workgroup against the fp32 read-modify-write launch of [M,768] this replaces (adapter up-projection riding on fc2).
// One workgroup = one tile: `bid` of `nwg` logical workgroups that tile rows [m_begin, M) (gemm_bf16_nt_kernel below passes its block index).
// F8 ("fp16f8" form of the split contraction, dyt_common.h: store4_split_f8): both operand images are [hi16 | 2K bytes of fp8]; k-tiles
// [0, f8_begin) are f16 tiles of 64, the tiles after them fp8 tiles of 128 (the same 128 B per row and stage, the same fragment reads),
// multiplied by v_mfma_scale_f32_16x16x128_f8f6f4 -- ONE instruction per fragment pair and k-tile instead of two, at the time of one
// f16 MFMA per 64 k: the lane's 32 operand bytes are its two 16-B fragment chunks {g, 4 + g} of the row (the same k subset on both
// sides, so the order inside the tile does not matter).  The E8M0 scale operand takes the images' powers of two back out:
// 2^-(ew+11) for the A_hi8 x W_lo8 tiles (first half), 2^-(ew+12) for the A_lo8 x W_hi8 tiles.
template <int BM, int BN, int WAVES_M, int WAVES_N, class Epi, int ABL, bool CAT, bool F8 = false, int LEAD = 0>
__device__ __forceinline__ void gemm_bf16_nt_tile(
    const bf16* __restrict__ A, const bf16* __restrict__ W, int M, int N, int K, const int* __restrict__ m_dev,
    const int* __restrict__ a_map, int m_begin, const Epi& epi, const CatArgs& cat, int bid, int nwg) {
    extern __shared__ __attribute__((aligned(16))) char smem[];   // declared HERE, not passed in: a generic char* would lose the LDS address space
    constexpr int BK = 64;
    constexpr int NW = WAVES_M * WAVES_N, NTHR = 64 * NW;
    constexpr int A_BYTES = BM * BK * 2, B_BYTES = BN * BK * 2, STAGE = A_BYTES + B_BYTES;
    constexpr int WM = BM / WAVES_M, WN = BN / WAVES_N, TM = WM / 16, TN = WN / 16;
    constexpr int A_INSTR = BM / 8 / NW, B_INSTR = BN / 8 / NW;  // 1 KiB (8 rows x 128 B) per wave-instruction
    static_assert(BM % (8 * NW) == 0 && BN % (8 * NW) == 0 && WM % 16 == 0 && WN % 16 == 0, "tile/wave layout");
    constexpr bool BOTH_KS = (TM + TN) * 2 * 4 <= 72;  // hold both k-substeps' fragments when registers allow
    static_assert(!(F8 && CAT), "the fp8-correction form has no leading k-tile variant");
    static_assert(!(LEAD && CAT) && (LEAD == 0 || LEAD == 3), "LEAD: three leading tiles of a three-part product, split forms only");
    typedef int v4i __attribute__((ext_vector_type(4)));
    typedef int v8i __attribute__((ext_vector_type(8)));

    const int Mv = m_dev ? min(*m_dev, M) : M;
    // XCD-aware block remap (bijective): consecutive logical tiles share an A row panel and
    // should land on the same XCD's L2; hardware places block b on XCD b % 8.
    const int tiles_n = N / BN;
    // ... over the tiles that exist (device-side row count: see gemm_bpre.h), so that a compacted launch spreads over all eight XCDs
    const int nwg_v = min(nwg, ((max(Mv - m_begin, 0) + BM - 1) / BM) * tiles_n);
    if (bid >= nwg_v) return;
    const int q8 = nwg_v >> 3, r8 = nwg_v & 7, xcd = bid & 7, idx = bid >> 3;
    const int wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + idx;
    const int tm = wgid / tiles_n, tn = wgid - tm * tiles_n;
    const int m0 = m_begin + tm * BM, n0 = tn * BN;
    if (m0 >= Mv) return;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WAVES_N, wn = wave - wm * WAVES_N;
    unsigned long long t_start = 0, t_loop0 = 0, t_loop1 = 0;
    if (ABL == 9) t_start = __builtin_readcyclecounter();

    // ---- staging: lane -> (row-in-8, 16B slot); source chunk = slot ^ row ----
    const int lrow = lane >> 3, slot = lane & 7, chunk = slot ^ lrow;
    const bf16* a_src[A_INSTR];
    const bf16* b_src[B_INSTR];
    const int fold = cat.a_fold, lda = cat.a_ld ? cat.a_ld : K - fold * BK;   // split A operand stored [hi | lo]: the hi part serves the first two thirds of the contraction
    // F8 kernels: 32-bit byte offsets from the (uniform) operand bases instead of per-lane 64-bit pointers -- 8 VGPRs less where the
    // accumulators and two fragment generations already fill the register file (operand images stay below 4 GB: M x 4K bytes)
    unsigned a_o32[A_INSTR], b_o32[B_INSTR];
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);
    const unsigned lane_o32 = (unsigned)(lrow * lda + chunk * 8) * 2u;
#pragma unroll
    for (int t = 0; t < A_INSTR; ++t) {
        const int row = (t * NW + wave) * 8 + lrow;
        int grow = min(m0 + row, Mv - 1);
        if (a_map) grow = a_map[grow];  // gathered A rows (compacted MLP backward)
        a_src[t] = A + (size_t)grow * lda + chunk * 8 - (CAT ? BK : 0);
        a_o32[t] = (unsigned)(((size_t)grow * lda + chunk * 8) * 2);
    }
#pragma unroll
    for (int t = 0; t < B_INSTR; ++t) {
        const int row = (t * NW + wave) * 8 + lrow;
        b_src[t] = W + (size_t)(n0 + row) * lda + chunk * 8 - (CAT ? BK : 0);   // split form: W stored [hi | lo] like A (same row stride)
        b_o32[t] = (unsigned)(((size_t)(n0 + row) * lda + chunk * 8) * 2);
    }
    // one 1-KiB DMA piece (idx < A_INSTR: A rows, else W rows) -- issued interleaved with the MFMAs so the
    // in-order wave never sits behind a burst of LDS-DMA issues (each costs ~100+ cycles back-to-back)
    auto stage_one = [&](int buf, int kt, int idx) {
        char* base = smem + buf * STAGE;
        if constexpr (F8) {   // rows are read straight through: tile kt = bytes [128 kt, 128 kt + 128) of the row image
            if constexpr (!BOTH_KS) {
                // 256x256 kernel: everything but the lane's place inside a piece (row lrow of 8, 16-B chunk) is wave-uniform and stays
                // in scalar registers -- ONE vector register of addressing next to 128 accumulators and two fragment generations
                // (per-lane row pointers spilled, and a spill reload inside the loop waits for vmcnt(0), i.e. for the DMA in flight).
                // Hence no row gather and no clamp to the valid row count here: rows past it are read and never stored (the split
                // operand images are padded to whole 256-row tiles; gemm_route sends gathered launches to the 128x128 kernel).
                const bool isA = idx < A_INSTR;
                const int piece = isA ? idx : idx - A_INSTR;
                const size_t row0 = (size_t)((isA ? m0 : n0) + (piece * NW + wave_s) * 8);
                const char* g = reinterpret_cast<const char*>(isA ? A : W) + (row0 * (size_t)lda) * 2 + (size_t)kt * 128;
                unsigned o = lane_o32;
                asm volatile("" : "+v"(o));   // keeps the zero-extension in this block: "SGPR base + 32-bit VGPR offset" form of the load
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(g + o),
                                                 (__attribute__((address_space(3))) void*)(base + (isA ? 0 : A_BYTES) + (piece * NW + wave_s) * 1024), 16, 0, 0);
                return;
            }
            const char* ga = reinterpret_cast<const char*>(A) + (size_t)kt * 128;
            const char* gw = reinterpret_cast<const char*>(W) + (size_t)kt * 128;
            unsigned o = idx < A_INSTR ? a_o32[idx] : b_o32[idx - A_INSTR];
            asm volatile("" : "+v"(o));
            if (idx < A_INSTR)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ga + o),
                                                 (__attribute__((address_space(3))) void*)(base + (idx * NW + wave) * 1024), 16, 0, 0);
            else
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gw + o),
                                                 (__attribute__((address_space(3))) void*)(base + A_BYTES + ((idx - A_INSTR) * NW + wave) * 1024), 16, 0, 0);
            return;
        }
        if (idx < A_INSTR)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a_src[idx] + (kt - (kt >= fold ? fold : 0)) * BK),
                                             (__attribute__((address_space(3))) void*)(base + (idx * NW + wave) * 1024),
                                             16, 0, 0);
        else
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) void*)(b_src[idx - A_INSTR] + (kt - (kt >= 2 * fold ? 2 * fold : 0)) * BK),
                (__attribute__((address_space(3))) void*)(base + A_BYTES + ((idx - A_INSTR) * NW + wave) * 1024), 16, 0, 0);
    };
    auto stage = [&](int buf, int kt) {
        char* base = smem + buf * STAGE;
        if constexpr (F8) {
#pragma unroll
            for (int t = 0; t < A_INSTR + B_INSTR; ++t) stage_one(buf, kt, t);
            return;
        }
#pragma unroll
        for (int t = 0; t < A_INSTR; ++t)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a_src[t] + (kt - (kt >= fold ? fold : 0)) * BK),
                                             (__attribute__((address_space(3))) void*)(base + (t * NW + wave) * 1024),
                                             16, 0, 0);
#pragma unroll
        for (int t = 0; t < B_INSTR; ++t)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(b_src[t] + (kt - (kt >= 2 * fold ? 2 * fold : 0)) * BK),
                                             (__attribute__((address_space(3))) void*)(base + A_BYTES + (t * NW + wave) * 1024),
                                             16, 0, 0);
    };

    // CAT: stage 0 comes from the second operand pair (one 64-wide row = one 128-B ring row)
    auto stage_first = [&]() {
        if constexpr (CAT) {
#pragma unroll
            for (int t = 0; t < A_INSTR; ++t) {
                int grow = min(m0 + (t * NW + wave) * 8 + lrow, Mv - 1);
                if (cat.a2_map) grow = cat.a2_map[grow];
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(cat.A2 + (size_t)grow * BK + chunk * 8),
                                                 (__attribute__((address_space(3))) void*)(smem + (t * NW + wave) * 1024), 16, 0, 0);
            }
#pragma unroll
            for (int t = 0; t < B_INSTR; ++t) {
                const int row = (t * NW + wave) * 8 + lrow;
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(cat.W2 + (size_t)(n0 + row) * BK + chunk * 8),
                                                 (__attribute__((address_space(3))) void*)(smem + A_BYTES + (t * NW + wave) * 1024), 16, 0, 0);
            }
        } else {
            stage(0, 0);
        }
    };

    // ---- fragment read offsets: row = tilebase + (lane & 15), chunk = ks*4 + (lane >> 4) ----
    const int frow = lane & 15;
    const int fslot0 = ((lane >> 4)) ^ (lane & 7);
    const int fslot1 = (4 + (lane >> 4)) ^ (lane & 7);
    const int a_off = (wm * WM + frow) * 128;
    const int b_off = A_BYTES + (wn * WN + frow) * 128;

    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    if constexpr (LEAD > 0) {
        // ---- leading tiles of the second operand pair (see CatArgs).  The four operand tiles go out in ONE DMA round -- A2_hi / W2_hi into
        // ring slot 0, A2_lo / W2_lo into slot 1 -- so the three products pay one exposed load latency and two barriers:
        // (A2_hi, W2_hi), (A2_hi, W2_lo), (A2_lo, W2_hi)
#pragma unroll
        for (int part = 0; part < 2; ++part) {
#pragma unroll
            for (int q = 0; q < A_INSTR; ++q) {
                int grow = min(m0 + (q * NW + wave) * 8 + lrow, Mv - 1);
                if (cat.a2_map) grow = cat.a2_map[grow];
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(cat.A2 + (size_t)grow * (2 * BK) + part * BK + chunk * 8),
                                                 (__attribute__((address_space(3))) void*)(smem + part * STAGE + (q * NW + wave) * 1024), 16, 0, 0);
            }
#pragma unroll
            for (int q = 0; q < B_INSTR; ++q) {
                const int row = (q * NW + wave) * 8 + lrow;
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(cat.W2 + (size_t)(n0 + row) * (2 * BK) + part * BK + chunk * 8),
                                                 (__attribute__((address_space(3))) void*)(smem + part * STAGE + A_BYTES + (q * NW + wave) * 1024), 16, 0, 0);
            }
        }
        dma_wait_all();
        __syncthreads();
#pragma unroll 1
        for (int t = 0; t < LEAD; ++t) {
            const char* ab = smem + (t == 2 ? STAGE : 0);
            const char* wb = smem + (t == 1 ? STAGE : 0);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int so = (ks == 0 ? fslot0 : fslot1) * 16;
                bf16x8 la[TM], lw[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i) la[i] = *reinterpret_cast<const bf16x8*>(ab + a_off + i * 2048 + so);
#pragma unroll
                for (int j = 0; j < TN; ++j) lw[j] = *reinterpret_cast<const bf16x8*>(wb + b_off + j * 2048 + so);
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) acc[i][j] = DYT_MFMA_16x16x32(lw[j], la[i], acc[i][j]);
            }
        }
        __syncthreads();   // every wave's reads of the two slots have returned before the main loop's first stages land in them
    }
    const int nk = K / BK + (CAT ? 1 : 0);
    if (ABL == 9) t_loop0 = __builtin_readcyclecounter();
    // fp8 tiles: E8M0 scale operands of the two correction products (the W fragment is the MFMA's A operand: the whole factor goes there)
    int f8_sc1 = 127, f8_sc2 = 127, f8_half = 0;
    if constexpr (F8) {
        const int ew = cat.w_exp ? *cat.w_exp : 0;
        f8_sc1 = 127 - (ew + 11); f8_sc2 = 127 - (ew + F8_LO_LOG2);
        f8_half = cat.f8_begin + (nk - cat.f8_begin) / 2;
    }
#define DYT_MFMA_F8(w8, a8, c, sc) __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4((w8), (a8), (c), 0, 0, 0, (sc), 0, 127)
#define DYT_CAT8(lo, hi) __builtin_shufflevector((lo), (hi), 0, 1, 2, 3, 4, 5, 6, 7)
    // schedule of the half-stage pipeline (both !BOTH_KS forms): one block of TM x TN MFMAs, and the group barriers that slot reads (R) and
    // DMA pieces (D) in between them
#define DYT_MMA(FW, FA)                                                                                     \
    _Pragma("unroll") for (int i = 0; i < TM; ++i) _Pragma("unroll") for (int j = 0; j < TN; ++j)            \
        acc[i][j] = DYT_MFMA_16x16x32(FW[j], FA[i], acc[i][j]);
#define DYT_SG3R __builtin_amdgcn_sched_group_barrier(0x008, 3, 0); __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
#define DYT_SG2R __builtin_amdgcn_sched_group_barrier(0x008, 2, 0); __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
#define DYT_SGB /* per 8 MFMAs: M2 R M2 R M1 D M2 R M1 D */                                            \
    __builtin_amdgcn_sched_group_barrier(0x008, 2, 1); __builtin_amdgcn_sched_group_barrier(0x100, 1, 1); \
    __builtin_amdgcn_sched_group_barrier(0x008, 2, 1); __builtin_amdgcn_sched_group_barrier(0x100, 1, 1); \
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 1); __builtin_amdgcn_sched_group_barrier(0x010, 1, 1); \
    __builtin_amdgcn_sched_group_barrier(0x008, 2, 1); __builtin_amdgcn_sched_group_barrier(0x100, 1, 1); \
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 1); __builtin_amdgcn_sched_group_barrier(0x010, 1, 1);
    // one fragment of (the stage at `base`, k-substep chunk offset `so`) -> set A
#define DYT_RA(i) faA[i] = *reinterpret_cast<const bf16x8*>(base + a_off + (i) * 2048 + so);
#define DYT_RW(j) fwA[j] = *reinterpret_cast<const bf16x8*>(base + b_off + (j) * 2048 + so);
#define DYT_FENCE __builtin_amdgcn_sched_barrier(0);
    if constexpr (!BOTH_KS) {
        // two fragment sets, one per k-substep
        bf16x8 faA[TM], fwA[TN], faB[TM], fwB[TN];
        constexpr int NDMA = A_INSTR + B_INSTR;
        static_assert(TM == 8 && TN == 4 && NDMA == 8, "interleave pattern written for the 128x64 wave tile, 8 DMA pieces");
        if constexpr (F8) {
            // ---- the half-stage pipeline below with 8-register fragments: .lo = k-substep 0 (row chunk g of lane group g), .hi = k-substep 1
            // (chunk 4 + g).  f16 tiles run exactly the plain schedule on the halves.  An fp8 tile needs BOTH halves per MFMA, so its 32
            // MFMAs are split by ROW fragments instead: block 1 = rows 0..3 (while rows 4..7 of the tile are read), barrier, block 2 =
            // rows 4..7, j-major (while rows 0..3 of the NEXT tile, then -- each after its last use -- its W fragments are read and the
            // DMA of the tile after that goes out).  Same reads, DMA pieces and matrix-pipe cycles per k-tile as an f16 tile.
            // (the f16 tiles use the plain kernel's two fragment sets.  Their reads are written out: with the read_a / read_b lambdas of the plain
            // branch the 20 F8 256x256 instantiations come out with another register allocation)
#define DYT_LDS4(off) (*reinterpret_cast<const v4i*>(base + (off)))
            stage_first();
            stage(1, 1);
            dma_wait_all();
            __syncthreads();
            {
                const char* base = smem;
#pragma unroll
                for (int i = 0; i < TM; ++i) faA[i] = *reinterpret_cast<const bf16x8*>(base + a_off + i * 2048 + fslot0 * 16);
#pragma unroll
                for (int j = 0; j < TN; ++j) fwA[j] = *reinterpret_cast<const bf16x8*>(base + b_off + j * 2048 + fslot0 * 16);
            }
            const int n1 = cat.f8_begin;
            for (int kt = 0; kt < n1; ++kt) {   // f16 tiles: the plain kernel's iteration (a tile kt + 1 always exists: the fp8 tiles follow)
                {
                    const char* base = smem + (kt & 1) * STAGE;
#pragma unroll
                    for (int i = 0; i < TM; ++i) faB[i] = *reinterpret_cast<const bf16x8*>(base + a_off + i * 2048 + fslot1 * 16);
#pragma unroll
                    for (int j = 0; j < TN; ++j) fwB[j] = *reinterpret_cast<const bf16x8*>(base + b_off + j * 2048 + fslot1 * 16);
                }
                DYT_MMA(fwA, faA)
                DYT_SG3R DYT_SG3R DYT_SG3R DYT_SG3R DYT_SG3R DYT_SG3R DYT_SG3R DYT_SG3R
                DYT_SG2R DYT_SG2R DYT_SG2R DYT_SG2R
                __builtin_amdgcn_sched_barrier(0);
                dma_wait_all();
                __syncthreads();
                // block B in issue order, fenced (next to the opaque staging offsets the group barriers no longer reproduce the plain
                // kernel's interleave): per 8 MFMAs  M2 R M2 R M1 D M2 R M1 D
                const int nxt = min(kt + 2, nk - 1);
                {
                    const char* base = smem + ((kt + 1) & 1) * STAGE;
                    const int so = fslot0 * 16;
#define DYT_MB(i, j) acc[i][j] = DYT_MFMA_16x16x32(fwB[j], faB[i], acc[i][j]);
#define DYT_GRP(g, R0, R1, R2)                                                                     \
                    DYT_MB(2 * g, 0) DYT_MB(2 * g, 1) R0 DYT_FENCE DYT_MB(2 * g, 2) DYT_MB(2 * g, 3) R1 DYT_FENCE \
                    DYT_MB(2 * g + 1, 0) stage_one(kt & 1, nxt, 2 * g); DYT_FENCE                               \
                    DYT_MB(2 * g + 1, 1) DYT_MB(2 * g + 1, 2) R2 DYT_FENCE DYT_MB(2 * g + 1, 3) stage_one(kt & 1, nxt, 2 * g + 1); DYT_FENCE
                    DYT_GRP(0, DYT_RA(0), DYT_RA(1), DYT_RA(2))
                    DYT_GRP(1, DYT_RA(3), DYT_RA(4), DYT_RA(5))
                    DYT_GRP(2, DYT_RA(6), DYT_RA(7), DYT_RW(0))
                    DYT_GRP(3, DYT_RW(1), DYT_RW(2), DYT_RW(3))
                }
            }
            // fp8 tiles: 8-register fragments (.lo = the k-substep-0 chunk, .hi = the k-substep-1 chunk); they start with rows 0..3 and W of
            // tile n1 (the f16 loop's last prefetch into its own set is not reused: one exposed LDS round trip per GEMM tile)
            v8i fa[TM], fw[TN];
            {
                const char* base = smem + (n1 & 1) * STAGE;
#pragma unroll
                for (int i = 0; i < 4; ++i) fa[i] = DYT_CAT8(DYT_LDS4(a_off + i * 2048 + fslot0 * 16), DYT_LDS4(a_off + i * 2048 + fslot1 * 16));
#pragma unroll
                for (int j = 0; j < TN; ++j) fw[j] = DYT_CAT8(DYT_LDS4(b_off + j * 2048 + fslot0 * 16), DYT_LDS4(b_off + j * 2048 + fslot1 * 16));
            }
            // The scheduler's group barriers do not place the scaled MFMAs (the schedule came out as all reads first, then the MFMAs, with
            // ~250 spilled registers), so the fp8 blocks are written in issue order and fenced with sched_barrier(0) every four MFMAs.
#define DYT_M8(i, j) acc[i][j] = DYT_MFMA_F8(fw[j], fa[i], acc[i][j], sc);
#define DYT_RA8(i) fa[i] = DYT_CAT8(DYT_LDS4(a_off + (i) * 2048 + fslot0 * 16), DYT_LDS4(a_off + (i) * 2048 + fslot1 * 16));
#define DYT_RW8(j) fw[j] = DYT_CAT8(DYT_LDS4(b_off + (j) * 2048 + fslot0 * 16), DYT_LDS4(b_off + (j) * 2048 + fslot1 * 16));
            // block 1: rows 0..3 x all W fragments (16 MFMAs); both halves of rows 4..7 of the same tile are read meanwhile
#define DYT_F8_BLOCK1(kt_)                                                        \
            {                                                                         \
                const char* base = smem + ((kt_) & 1) * STAGE;                        \
                DYT_M8(0, 0) DYT_M8(0, 1) DYT_RA8(4) DYT_M8(0, 2) DYT_M8(0, 3) DYT_FENCE \
                DYT_M8(1, 0) DYT_M8(1, 1) DYT_RA8(5) DYT_M8(1, 2) DYT_M8(1, 3) DYT_FENCE \
                DYT_M8(2, 0) DYT_M8(2, 1) DYT_RA8(6) DYT_M8(2, 2) DYT_M8(2, 3) DYT_FENCE \
                DYT_M8(3, 0) DYT_M8(3, 1) DYT_RA8(7) DYT_M8(3, 2) DYT_M8(3, 3) DYT_FENCE \
            }
            DYT_FENCE
            for (int kt = n1; kt < nk - 1; ++kt) {
                const int sc = kt < f8_half ? f8_sc1 : f8_sc2;
                DYT_F8_BLOCK1(kt)
                dma_wait_all();   // this wave's pieces of stage kt+1 have landed ...
                __syncthreads();  // ... everywhere; every wave's reads of slot kt&1 have returned
                // block 2: rows 4..7, j-major (16 MFMAs); rows 0..3 of tile kt+1, its W fragments (each after the four MFMAs that read
                // the old one) and the 8 DMA pieces of stage kt+2 -> slot kt&1
                const int nxt = min(kt + 2, nk - 1);
                {
                    const char* base = smem + ((kt + 1) & 1) * STAGE;
                    DYT_M8(4, 0) DYT_M8(5, 0) DYT_RA8(0) stage_one(kt & 1, nxt, 0); DYT_FENCE
                    DYT_M8(6, 0) DYT_M8(7, 0) stage_one(kt & 1, nxt, 1); DYT_FENCE
                    DYT_M8(4, 1) DYT_M8(5, 1) DYT_RA8(1) stage_one(kt & 1, nxt, 2); DYT_FENCE
                    DYT_M8(6, 1) DYT_M8(7, 1) DYT_RW8(0) stage_one(kt & 1, nxt, 3); DYT_FENCE
                    DYT_M8(4, 2) DYT_M8(5, 2) DYT_RA8(2) stage_one(kt & 1, nxt, 4); DYT_FENCE
                    DYT_M8(6, 2) DYT_M8(7, 2) DYT_RW8(1) stage_one(kt & 1, nxt, 5); DYT_FENCE
                    DYT_M8(4, 3) DYT_M8(5, 3) DYT_RA8(3) stage_one(kt & 1, nxt, 6); DYT_FENCE
                    DYT_M8(6, 3) DYT_M8(7, 3) DYT_RW8(2) stage_one(kt & 1, nxt, 7); DYT_FENCE
                    DYT_RW8(3) DYT_FENCE
                }
            }
            {   // last tile: nothing left to prefetch
                const int kt = nk - 1;
                const int sc = kt < f8_half ? f8_sc1 : f8_sc2;
                DYT_F8_BLOCK1(kt)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int i = 4; i < TM; ++i) acc[i][j] = DYT_MFMA_F8(fw[j], fa[i], acc[i][j], sc);
            }
        } else {
            // ---- big wave tiles (128x64 per wave): half-stage software pipeline.  Two fragment sets, one per
            // k-substep; every LDS fragment read is issued one MFMA block (32 MFMAs) ahead of its use, the
            // single barrier of a stage sits between the two MFMA blocks, and the DMA of stage kt+2 is issued
            // right after it.  Invariant at the top of iteration kt: Fa holds (kt, ks=0); slot kt&1 holds
            // stage kt; slot (kt+1)&1 holds or is receiving stage kt+1.
            // (Round 5: an L2 prefetch of the stage 2-3 k-tiles ahead -- one global_load_dword per wave into a dead register behind the DMA pieces,
            // counted vmcnt(1) in front of the barrier -- was built to shorten the launch on operands that are not in the Infinity Cache (112 vs
            // 79 us, tools/gemm_bench.py COLD=1): cold launches unchanged, step 24.19 vs 24.01 ms same-box.  Not kept)
            auto read_a = [&](int buf) {   // (stage in `buf`, ks = 0) -> set A
                const char* base = smem + buf * STAGE;
#pragma unroll
                for (int i = 0; i < TM; ++i) faA[i] = *reinterpret_cast<const bf16x8*>(base + a_off + i * 2048 + fslot0 * 16);
#pragma unroll
                for (int j = 0; j < TN; ++j) fwA[j] = *reinterpret_cast<const bf16x8*>(base + b_off + j * 2048 + fslot0 * 16);
            };
            auto read_b = [&](int buf) {   // (stage in `buf`, ks = 1) -> set B
                const char* base = smem + buf * STAGE;
#pragma unroll
                for (int i = 0; i < TM; ++i) faB[i] = *reinterpret_cast<const bf16x8*>(base + a_off + i * 2048 + fslot1 * 16);
#pragma unroll
                for (int j = 0; j < TN; ++j) fwB[j] = *reinterpret_cast<const bf16x8*>(base + b_off + j * 2048 + fslot1 * 16);
            };
            stage_first();
            if (nk > 1) stage(1, 1);
            dma_wait_all();
            __syncthreads();
            read_a(0);
            for (int kt = 0; kt < nk - 1; ++kt) {
                // ---- block A: 32 MFMAs on set A, the 12 fragment reads of (kt, ks=1) -> set B slotted in between
                read_b(kt & 1);
                DYT_MMA(fwA, faA)
                DYT_SG3R DYT_SG3R DYT_SG3R DYT_SG3R DYT_SG3R DYT_SG3R DYT_SG3R DYT_SG3R   // 24 MFMA, 8 reads
                DYT_SG2R DYT_SG2R DYT_SG2R DYT_SG2R                                       //  8 MFMA, 4 reads
                __builtin_amdgcn_sched_barrier(0);
                dma_wait_all();   // this wave's pieces of stage kt+1 have landed ...
                __syncthreads();  // ... everywhere; every wave's reads of slot kt&1 have returned
                // ---- block B: 32 MFMAs on set B; the reads of (kt+1, ks=0) -> set A and the 8 DMA pieces of stage
                //      kt+2 -> slot kt&1 slotted in between.  (Past the end the last stage is simply re-fetched
                //      into the free slot: keeps this a single basic block for the scheduler.)
                // source order = issue order (LDS-DMA writes and ds_reads are kept in program order by the
                // scheduler's memory dependencies): R R D R D, four times = 12 reads + 8 DMA pieces
                const int nxt = min(kt + 2, nk - 1);
                {
                    const char* base = smem + ((kt + 1) & 1) * STAGE;
                    const int so = fslot0 * 16;
                    DYT_RA(0) DYT_RA(1) stage_one(kt & 1, nxt, 0); DYT_RA(2) stage_one(kt & 1, nxt, 1);
                    DYT_RA(3) DYT_RA(4) stage_one(kt & 1, nxt, 2); DYT_RA(5) stage_one(kt & 1, nxt, 3);
                    DYT_RA(6) DYT_RA(7) stage_one(kt & 1, nxt, 4); DYT_RW(0) stage_one(kt & 1, nxt, 5);
                    DYT_RW(1) DYT_RW(2) stage_one(kt & 1, nxt, 6); DYT_RW(3) stage_one(kt & 1, nxt, 7);
                }
                DYT_MMA(fwB, faB)
                DYT_SGB DYT_SGB DYT_SGB DYT_SGB
                __builtin_amdgcn_sched_barrier(0);
            }
            {   // last stage: nothing left to prefetch
                read_b((nk - 1) & 1);
                DYT_MMA(fwA, faA)
                DYT_SG3R DYT_SG3R DYT_SG3R DYT_SG3R DYT_SG3R DYT_SG3R DYT_SG3R DYT_SG3R
                DYT_SG2R DYT_SG2R DYT_SG2R DYT_SG2R
                __builtin_amdgcn_sched_barrier(0);
                DYT_MMA(fwB, faB)
            }
        }
    } else {
    stage_first();
    for (int kt = 0; kt < nk; ++kt) {
        dma_wait_all();
        __syncthreads();  // stage kt landed (vmcnt drained before the barrier); ring slot (kt+1)&1 is free
        if (kt + 1 < nk) stage((kt + 1) & 1, kt + 1);
        const char* base = smem + (kt & 1) * STAGE;
        // issue all fragment reads of the K step, then the MFMAs: one LDS-latency exposure per step
        bf16x8 af[2][TM], wf[2][TN];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int so = (ks == 0 ? fslot0 : fslot1) * 16;
#pragma unroll
            for (int i = 0; i < TM; ++i) af[ks][i] = *reinterpret_cast<const bf16x8*>(base + a_off + i * 2048 + so);
#pragma unroll
            for (int j = 0; j < TN; ++j) wf[ks][j] = *reinterpret_cast<const bf16x8*>(base + b_off + j * 2048 + so);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (F8 && kt >= cat.f8_begin) {   // fp8 tile: one MFMA per fragment pair over both k-substeps' chunks
            const int sc = kt < f8_half ? f8_sc1 : f8_sc2;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = DYT_MFMA_F8(DYT_CAT8(__builtin_bit_cast(v4i, wf[0][j]), __builtin_bit_cast(v4i, wf[1][j])),
                                            DYT_CAT8(__builtin_bit_cast(v4i, af[0][i]), __builtin_bit_cast(v4i, af[1][i])), acc[i][j], sc);
        } else {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = DYT_MFMA_16x16x32(wf[ks][j], af[ks][i], acc[i][j]);
        }
        __builtin_amdgcn_sched_barrier(0);
    }

    }  // main-loop variants
#undef DYT_MFMA_F8
#undef DYT_CAT8
#undef DYT_MMA
#undef DYT_SG3R
#undef DYT_SG2R
#undef DYT_SGB
#undef DYT_FENCE
#undef DYT_RA
#undef DYT_RW
#undef DYT_LDS4
#undef DYT_MB
#undef DYT_GRP
#undef DYT_M8
#undef DYT_RA8
#undef DYT_RW8
#undef DYT_F8_BLOCK1
    if (ABL == 9) t_loop1 = __builtin_readcyclecounter();

    {
        // ---- epilogue through LDS: acc[i][j][e] = C[wm*WM + i*16 + (lane&15)][wn*WN + j*16 + (lane>>4)*4 + e].
        // The fragment layout gives each store instruction 16 rows x 64 B; instead the tile is parked in the
        // (now free) staging ring as fp32 with the 16-B chunk index XOR-swizzled by (row & 7) (conflict-free
        // ds_write_b128 / ds_read_b128) and read back row-major, so every global access of the epilogue
        // functor is a full-row, 16-B-per-lane coalesced transaction.  If the whole fp32 tile does not fit
        // the ring it goes through in WAVES_M passes of WM rows.
        constexpr bool ONE_PASS = BM * BN * 4 <= 2 * STAGE;
        constexpr int PASSES = ONE_PASS ? 1 : WAVES_M;
        constexpr int PROWS = BM / PASSES;
        static_assert(PROWS * BN * 4 <= 2 * STAGE, "epilogue staging does not fit the LDS ring");
        float* Cs = reinterpret_cast<float*>(smem);
        constexpr int CH = BN / 4;                 // 16-B chunks per tile row
        static_assert(NTHR % CH == 0, "a lane must keep one column chunk for the whole tile");
        constexpr int RSTEP = NTHR / CH;           // rows covered by one sweep of the workgroup
        constexpr int ITERS = PROWS / RSTEP;
        constexpr int BATCH = ITERS % 8 == 0 ? 8 : ITERS;
        const int ch = tid % CH, rl0 = tid / CH;
        const int col = n0 + ch * 4;
        const typename Epi::Col cc = epi.col_init(col);   // bias etc.: once per tile, not once per chunk
        dma_wait_all();  // nothing may still be landing in the ring when it is reused as staging
#pragma unroll 1
        for (int p = 0; p < PASSES; ++p) {
            // the functor's own global loads for the whole pass go out first: their latency overlaps the
            // staging write, the barriers and the LDS read-back instead of serialising chunk by chunk
            // (functors with a large per-chunk context prefetch one read-back batch at a time instead: 16 x 24 B
            // next to 128 live accumulators spilled)
            constexpr bool PRE_ALL = sizeof(typename Epi::Pre) * ITERS <= 256;
            typename Epi::Pre pr[PRE_ALL ? ITERS : BATCH];
            if (PRE_ALL) {
#pragma unroll
                for (int it = 0; it < ITERS; ++it)
                    pr[it] = epi.pre(min(m0 + p * PROWS + rl0 + it * RSTEP, Mv - 1), col);
            }
            __syncthreads();
            if (ONE_PASS || wm == p) {
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const int rl = (ONE_PASS ? wm * WM : 0) + i * 16 + frow;
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        const int chw = ((wn * WN + j * 16) >> 2) + (lane >> 4);
                        *reinterpret_cast<f32x4*>(Cs + rl * BN + ((chw ^ (rl & 7)) << 2)) = acc[i][j];
                    }
                }
            }
            __syncthreads();
#pragma unroll
            for (int it0 = 0; it0 < ITERS; it0 += BATCH) {
                if (!PRE_ALL) {
#pragma unroll
                    for (int u = 0; u < BATCH; ++u)
                        pr[u] = epi.pre(min(m0 + p * PROWS + rl0 + (it0 + u) * RSTEP, Mv - 1), col);
                }
                f32x4 c4[BATCH];
#pragma unroll
                for (int u = 0; u < BATCH; ++u) {
                    const int rl = rl0 + (it0 + u) * RSTEP;
                    c4[u] = *reinterpret_cast<const f32x4*>(Cs + rl * BN + ((ch ^ (rl & 7)) << 2));
                }
#pragma unroll
                for (int u = 0; u < BATCH; ++u) {
                    const int row = m0 + p * PROWS + rl0 + (it0 + u) * RSTEP;
                    if (row < Mv) {
                        const float os = cat.out_scale;   // 1.0 (exact) except in the split fp32 form of a gradient GEMM
                        const float v[4] = {c4[u][0] * os, c4[u][1] * os, c4[u][2] * os, c4[u][3] * os};
                        epi.apply(row, col, v, cc, pr[PRE_ALL ? it0 + u : u]);
                    }
                }
            }
        }
    }
    if (ABL == 9 && tid == 0) {
        const unsigned long long t_end = __builtin_readcyclecounter();
        atomicAdd(&g_gemm_dbg[0], t_loop0 - t_start);
        atomicAdd(&g_gemm_dbg[1], t_loop1 - t_loop0);
        atomicAdd(&g_gemm_dbg[2], t_end - t_loop1);
        atomicAdd(&g_gemm_dbg[3], 1ull);
    }
}

template <int BM, int BN, int WAVES_M, int WAVES_N, class Epi, int ABL = 0, bool CAT = false, bool F8 = false, int LEAD = 0>
__global__ __launch_bounds__(64 * WAVES_M * WAVES_N, 2) void gemm_bf16_nt_kernel(
    const bf16* __restrict__ A, const bf16* __restrict__ W, int M, int N, int K, const int* __restrict__ m_dev,
    const int* __restrict__ a_map, int m_begin, Epi epi, CatArgs cat) {
    // rows [m_begin, M) are tiled by this launch
    gemm_bf16_nt_tile<BM, BN, WAVES_M, WAVES_N, Epi, ABL, CAT, F8, LEAD>(A, W, M, N, K, m_dev, a_map, m_begin, epi, cat, blockIdx.x, gridDim.x);
}

}  // namespace dyt
