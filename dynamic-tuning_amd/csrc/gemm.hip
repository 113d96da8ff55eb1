// Dense contractions of the DyT hot path for gfx950.
//
//   C[M,N] = A[M,K] @ W[N,K]^T  (+ fused epilogue)
//
// fast path  : bf16 operands, v_mfma_f32_16x16x32_bf16, fp32 accumulate.
//              128x128x64 (or 128x64x64) tile, 4 waves (2x2), operands staged HBM->LDS by
//              LDS-DMA (global_load_lds_dwordx4) into a 2-deep ring, one barrier per K step.
//              LDS image per operand: [row][8 x 16B chunks], chunk slot XOR-swizzled with
//              (row & 7) on the SOURCE address (the DMA destination is lane-linear), and the
//              same XOR on the ds_read_b128 -- conflict-free for the 16x16x32 fragment read.
//              The MFMA is issued with the W fragment as the A operand so that every lane ends
//              up with 4 CONSECUTIVE output columns of one row (8/16-byte epilogue stores).
// exact path : fp32 operands on the matrix cores (v_mfma_f32_32x32x2_f32, gemm_f32_mfma.h) -- the parity mode.
//
// Reference ops replaced: nn.Linear of Attention.qkv / .proj (models/vision_transformer_IN21K.py:56,73),
// timm Mlp fc1/fc2 (:124-129,159), Adapter.down_proj/up_proj (models/dynamic_adapter.py:124-128),
// PatchEmbed's Conv2d (:272-278) and their autograd dgrads.
//
// This file is launch and dispatch; the device code is in the headers below: the epilogue functors (gemm_epi.h), the LDS-staged tile
// kernel (gemm_tile.h) and its siblings (gemm_bpre.h, gemm_f32_mfma.h, gemm_skinny.h), the tile routing as a pure function (gemm_route.h).
#include <type_traits>
#include "kernels.h"
#include "gemm_epi.h"
#include "gemm_tile.h"
#include "gemm_bpre.h"
#include "gemm_f32_mfma.h"
#include "gemm_route.h"
#include "gemm_skinny.h"
namespace dyt {

// pre-pass for the other tile shapes: (mean, rstd) of logical row r = source row a_map[r] into st[r] and st_src[source row]
__global__ __launch_bounds__(256) void ln_finalize_kernel(const float2* __restrict__ part, const int* __restrict__ a_map, float2* __restrict__ st,
                                                          float2* __restrict__ st_src, int rows) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const int t = a_map ? a_map[r] : r;
    const float2 v = ln_merge_parts(part, t);
    st[r] = v;
    if (st_src) st_src[t] = v;
}

// ------------------------------------------------------------------------------------------
// launch
// ------------------------------------------------------------------------------------------
// kernel launches of the bf16 family since the last reset (a logical GEMM may be two launches: bench.py converts
// the per-kernel-launch PMC traffic to its per-GEMM unit with this)
static long long g_bf16_kernel_launches = 0;
long long gemm_kernel_launch_count(int reset) {
    const long long n = g_bf16_kernel_launches;
    if (reset) g_bf16_kernel_launches = 0;
    return n;
}

template <int BM, int BN, int WAVES_M, int WAVES_N, int ABL, class Epi, bool CAT = false, bool F8 = false, int LEAD = 0>
static int launch_bf16_cfg(const GemmArgs& a, const Epi& epi, hipStream_t s, int m_begin = 0, int m_end = -1) {
    constexpr int NTHR = 64 * WAVES_M * WAVES_N;
    if (m_end < 0) m_end = a.M;
    if (m_end <= m_begin) return 0;
    const int grid = tile_grid(m_begin, m_end, a.N, BM, BN);
    const size_t lds = 2 * (BM + BN) * 64 * 2;
    constexpr auto kern = gemm_bf16_nt_kernel<BM, BN, WAVES_M, WAVES_N, Epi, ABL, CAT, F8, LEAD>;
    if (int rc = ensure_dyn_lds<kern>(lds)) return rc;
    const CatArgs cat{static_cast<const bf16*>(a.A2), static_cast<const bf16*>(a.W2), a.a2_map, a.out_scale, a.a_fold, a.a_ld, a.f8_begin, a.w_exp};
    hipLaunchKernelGGL(kern, dim3(grid), dim3(NTHR), lds, s, static_cast<const bf16*>(a.A), static_cast<const bf16*>(a.W),
                       m_end, a.N, a.K, a.m_dev, a.a_map, m_begin, epi, cat);
    ++g_bf16_kernel_launches;
    DYT_HIP_CHECK(hipGetLastError());
    return 0;
}

template <int ABL, class Epi>
static int launch_bf16_bpre(const GemmArgs& a, const Epi& epi, hipStream_t s, int m_begin = 0, int m_end = -1) {
    if (m_end < 0) m_end = a.M;
    if (m_end <= m_begin) return 0;
    if (a.K % 256 != 0 || a.N % 256 != 0) { set_error("gemm_bpre: K=%d and N=%d must be multiples of 256", a.K, a.N); return -1; }
    const int grid = tile_grid(m_begin, m_end, a.N, 128, 256);
    hipLaunchKernelGGL((gemm_bf16_bpre_kernel<Epi, ABL>), dim3(grid), dim3(256), 0, s, static_cast<const bf16*>(a.A),
                       static_cast<const bf16*>(a.W), m_end, a.N, a.K, a.m_dev, a.a_map, m_begin, epi, a.out_scale);
    ++g_bf16_kernel_launches;
    DYT_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_preshuffle_w(const void* W, void* Wp, int N, int K, hipStream_t s) {
    if (N % 16 != 0 || K % 32 != 0) { set_error("preshuffle: N=%d %% 16, K=%d %% 32 required", N, K); return -1; }
    const size_t chunks = (size_t)N * K / 8;
    hipLaunchKernelGGL(preshuffle_w_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, s,
                       static_cast<const bf16*>(W), static_cast<bf16*>(Wp), N, K);
    DYT_HIP_CHECK(hipGetLastError());
    return 0;
}

static int g_splitk = -1;   // DYT_OPT_GEMM_SPLITK (process-wide; environment DYT_SPLITK sets the default)
void set_gemm_splitk(int v) { g_splitk = v != 0; }
int get_gemm_splitk() {
    if (g_splitk < 0) { const char* e = getenv("DYT_SPLITK"); g_splitk = e ? (atoi(e) != 0) : 1; }
    return g_splitk;
}
// what gemm_route() (gemm_route.h) reads of a GEMM
static GemmShape route_shape(const GemmArgs& a, GemmFamily family, bool cat = false, bool lead = false, bool store_epi = false, bool splitk_epi = false) {
    GemmShape g;
    g.M = a.M; g.N = a.N; g.K = a.K; g.family = family; g.cat = cat; g.lead = lead; g.store_epi = store_epi;
    g.wp = a.Wp != nullptr; g.a_map = a.a_map != nullptr; g.a_ld = a.a_ld != 0; g.a_fold = a.a_fold != 0; g.m_dev = a.m_dev != nullptr;
    g.a2 = a.A2 != nullptr; g.w2 = a.W2 != nullptr; g.f8_begin = a.f8_begin;
    g.splitk_fits = splitk_epi && family == GF_16 && get_gemm_splitk() && a.splitk_ws && !a.f8 &&
                    (size_t)splitk_slices(a.K, cat) * a.M * a.N * sizeof(float) <= a.splitk_ws_bytes;
    return g;
}
static int route_error(const GemmRoute& r, const GemmArgs& a) {
    set_error("%s (M=%d N=%d K=%d)", r.error ? r.error : "gemm: this epilogue has no kernel of the routed family", a.M, a.N, a.K);
    return -1;
}

// the 16-bit MFMA kernels.  CAT / LEAD: a second operand pair in front of the contraction; F8: the "fp16f8" split contraction
// (a.K = 2 x the logical K: K / 64 f16 tiles + K / 64 fp8 tiles)
template <class Epi, bool CAT = false, int LEAD = 0, bool F8 = false>
static int run_bf16(const GemmArgs& a, const Epi& epi, hipStream_t s) {
    constexpr bool PLAIN = !CAT && LEAD == 0 && !F8;
    const GemmRoute r = gemm_route(route_shape(a, F8 ? GF_F8 : GF_16, CAT, LEAD > 0, std::is_same<Epi, EpiStoreAT<bf16>>::value, SplitKEpi<Epi>::value));
    switch (r.kernel) {
        case GK_SPLITK:
            if constexpr (SplitKEpi<Epi>::value && !F8) {
                const int slices = splitk_slices(a.K, CAT);
                hipLaunchKernelGGL((gemm_splitk_kernel<CAT>), dim3(a.N / 32, (a.M + 127) / 128, slices), dim3(256), 0, s, static_cast<const bf16*>(a.A),
                                   static_cast<const bf16*>(a.W), a.M, a.N, a.K, a.a_map, static_cast<const bf16*>(a.A2), static_cast<const bf16*>(a.W2),
                                   a.a2_map, a.splitk_ws);   // (not counted in g_bf16_kernel_launches: tools/pmc_traffic.py selects the gemm_bf16_* kernels)
                hipLaunchKernelGGL((splitk_reduce_kernel<Epi>), dim3((unsigned)(((size_t)a.M * (a.N / 4) + 255) / 256)), dim3(256), 0, s, a.splitk_ws, slices, a.M,
                                   a.N, a.out_scale, epi);
                DYT_HIP_CHECK(hipGetLastError());
                return 0;
            }
            break;
        case GK_BPRE:
            if constexpr (PLAIN) {
                GemmArgs b = a; b.W = a.Wp;
                return launch_bf16_bpre<0>(b, epi, s);
            }
            break;
        case GK_256: {   // two launches on the same stream when the whole-rounds scheme leaves a tail; a compacted GEMM (device-side row count) leaves it empty
            const int rc = launch_bf16_cfg<256, 256, 2, 4, 0, Epi, CAT, F8, LEAD>(a, epi, s, 0, r.body);
            if (rc || r.body >= a.M) return rc;
            return launch_bf16_cfg<128, 128, 2, 2, 0, Epi, CAT, F8, LEAD>(a, epi, s, r.body, a.M);
        }
        case GK_128: return launch_bf16_cfg<128, 128, 2, 2, 0, Epi, CAT, F8, LEAD>(a, epi, s);
        case GK_128x64:
            if constexpr (PLAIN) return launch_bf16_cfg<128, 64, 2, 2, 0>(a, epi, s);
            break;
        default: break;
    }
    return route_error(r, a);
}

template <int BM, int BN, class Epi>
static int launch_f32_cfg(const GemmArgs& a, const Epi& epi, hipStream_t s) {
    const int grid = tile_grid(0, a.M, a.N, BM, BN);
    const size_t lds = 2 * (BM + BN) * 128;
    constexpr auto kern = gemm_f32_mfma_nt_kernel<BM, BN, 2, 2, Epi>;
    if (int rc = ensure_dyn_lds<kern>(lds)) return rc;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, s, static_cast<const float*>(a.A), static_cast<const float*>(a.W),
                       a.M, a.N, a.K, a.m_dev, a.a_map, 0, epi);
    DYT_HIP_CHECK(hipGetLastError());
    return 0;
}

template <class Epi>
static int run_f32(const GemmArgs& a, const Epi& epi, hipStream_t s) {
    const GemmRoute r = gemm_route(route_shape(a, GF_F32));
    switch (r.kernel) {
        case GK_F32_128: return launch_f32_cfg<128, 128>(a, epi, s);
        case GK_F32_128x64: return launch_f32_cfg<128, 64>(a, epi, s);
        default: return route_error(r, a);
    }
}

// epilogues of the forward GEMMs against frozen weights: the ones the fp8-correction kernels are built for
template <class Epi> struct F8Epi : std::false_type {};
template <> struct F8Epi<EpiQKV<float>> : std::true_type {};
template <> struct F8Epi<EpiQKVPlanes> : std::true_type {};
template <class OT> struct F8Epi<EpiBiasResid<float, OT>> : std::true_type {};
template <bool G, class GT, bool F> struct F8Epi<EpiFc1<float, G, GT, F>> : std::true_type {};
template <bool P, class HT> struct F8Epi<EpiFc2<float, P, HT>> : std::true_type {};
template <> struct F8Epi<EpiAdUp<true>> : std::true_type {};    // cls-row proj of the teacher's last block
template <> struct F8Epi<EpiEmbed> : std::true_type {};
template <> struct F8Epi<EpiBiasF32> : std::true_type {};       // unit entry dyt_linear_split
// SPLIT: fp32 epilogue functors on the 16-bit MFMA kernels (the fp32 operands arrive as K-concatenated 16-bit hi / lo parts)
template <class AT, bool SPLIT, class Epi, int LEAD = 0>
static int run(const GemmArgs& a, const Epi& epi, hipStream_t s) {
    if constexpr (SPLIT && F8Epi<Epi>::value) { if (a.f8) return run_bf16<Epi, false, LEAD, true>(a, epi, s); }
    if (a.f8) { set_error("gemm: this epilogue has no fp8-correction form"); return -1; }
    if constexpr (sizeof(AT) == 2 || SPLIT) return run_bf16<Epi, false, LEAD>(a, epi, s);
    else return run_f32(a, epi, s);
}

template <class AT, bool SPLIT = false>
static int dispatch(EpiKind kind, const GemmArgs& a, hipStream_t s) {
    switch (kind) {
        case EPI_BIAS_F32: return run<AT, SPLIT>(a, EpiBiasF32{a.bias, a.out_f32, a.N}, s);
        case EPI_QKV:
            if constexpr (SPLIT) {
                if (a.qkv_lo[0]) return run<AT, SPLIT>(a, EpiQKVPlanes{a.bias, (bf16*)a.out_at, (bf16*)a.out_at2, (bf16*)a.out_at3, (bf16*)a.qkv_lo[0],
                                                                     (bf16*)a.qkv_lo[1], (bf16*)a.qkv_lo[2]}, s);
            }
            return run<AT, SPLIT>(a, EpiQKV<AT>{a.bias, (AT*)a.out_at, (AT*)a.out_at2, (AT*)a.out_at3}, s);
        case EPI_BIAS_RESID:
            if constexpr (SPLIT) { if (a.save16) return run<AT, SPLIT>(a, EpiBiasResid<AT, bf16>{a.bias, a.resid, a.out_f32, (bf16*)a.out_at, a.N, nullptr, a.row_scale}, s); }
            if constexpr (sizeof(AT) == 2) {
                if (a.ln_part) {
                    if (a.N != LN_PARTS * 64) { set_error("gemm: LayerNorm partials need N = %d", LN_PARTS * 64); return -1; }
                    return run<AT, SPLIT>(a, EpiBiasResid<AT, AT, true>{a.bias, a.resid, a.out_f32, (AT*)a.out_at, a.N, a.ln_part, a.row_scale}, s);
                }
            }
            if (a.ln_part) { set_error("gemm: LayerNorm partials exist in the 16-bit modes only"); return -1; }
            return run<AT, SPLIT>(a, EpiBiasResid<AT>{a.bias, a.resid, a.out_f32, (AT*)a.out_at, a.N, nullptr, a.row_scale}, s);
        case EPI_FC1:
            if constexpr (SPLIT) {   // the split forms take the A&S GELU (EpiFc1<FAST>): 42.7 vs 43.1 ms/step, logits vs the oracle unchanged (2.4e-5 / 6e-6)
                if (a.save16 && a.out_at2) return run<AT, SPLIT>(a, EpiFc1<AT, true, bf16, true>{a.bias, (AT*)a.out_at, (bf16*)a.out_at2, a.N, (bf16*)a.out3, a.out3_f8}, s);
                if (a.out_at2) return run<AT, SPLIT>(a, EpiFc1<AT, true, AT, true>{a.bias, (AT*)a.out_at, (AT*)a.out_at2, a.N, (bf16*)a.out3, a.out3_f8}, s);
                return run<AT, SPLIT>(a, EpiFc1<AT, false, AT, true>{a.bias, (AT*)a.out_at, nullptr, a.N, (bf16*)a.out3, a.out3_f8}, s);
            }
            if constexpr (sizeof(AT) == 2) {
                if (a.ln_part) {   // LayerNorm folded in
                    if (!a.ln_cs || !a.ln_st_out || !a.ln_scratch || a.K != LN_PARTS * 64) { set_error("gemm: folded LayerNorm form needs ln_cs, ln_st_out, ln_scratch and K = 768"); return -1; }
                    const float2* st = nullptr;
                    if (gemm_route(route_shape(a, GF_16)).kernel != GK_BPRE) {   // no statistics prologue in these tile shapes: merge the partials in a pre-pass
                        hipLaunchKernelGGL(ln_finalize_kernel, dim3((a.M + 255) / 256), dim3(256), 0, s, a.ln_part, a.a_map, a.a_map ? a.ln_scratch : a.ln_st_out,
                                           a.a_map ? a.ln_st_out : nullptr, a.M);
                        DYT_HIP_CHECK(hipGetLastError());
                        st = a.a_map ? a.ln_scratch : a.ln_st_out;
                    }
                    if (a.out_at2) return run<AT, SPLIT>(a, EpiFc1<AT, true, AT, false, true>{a.bias, (AT*)a.out_at, (AT*)a.out_at2, a.N, nullptr, 0, a.ln_cs, st, a.ln_part, a.ln_st_out}, s);
                    return run<AT, SPLIT>(a, EpiFc1<AT, false, AT, false, true>{a.bias, (AT*)a.out_at, nullptr, a.N, nullptr, 0, a.ln_cs, st, a.ln_part, a.ln_st_out}, s);
                }
            }
            if (a.ln_part) { set_error("gemm: the folded LayerNorm form exists in the 16-bit modes only"); return -1; }
            if (a.out_at2) return run<AT, SPLIT>(a, EpiFc1<AT, true>{a.bias, (AT*)a.out_at, (AT*)a.out_at2, a.N, (bf16*)a.out3, a.out3_f8}, s);
            return run<AT, SPLIT>(a, EpiFc1<AT, false>{a.bias, (AT*)a.out_at, nullptr, a.N, (bf16*)a.out3, a.out3_f8}, s);
        case EPI_FC2: {
            const float* resid = a.resid ? a.resid : a.out_f32;   // null: in place
            if (a.A2) {   // adapter up-projection as the leading k-tile of the contraction (16-bit kernels only)
                if constexpr (sizeof(AT) == 2) {
                    if (!a.row_map && !a.row_mask)
                        return run_bf16<EpiFc2<AT, true>, true>(a, EpiFc2<AT, true>{a.bias, a.out_f32, nullptr, nullptr, (AT*)a.h_out, resid, a.bias2, a.scale, a.row_scale}, s);
                    return run_bf16<EpiFc2<AT, false>, true>(a, EpiFc2<AT, false>{a.bias, a.out_f32, a.row_map, a.row_mask, (AT*)a.h_out, resid, a.bias2, a.scale, a.row_scale}, s);
                } else if constexpr (SPLIT) {
                    // split fp32 forms whose backward runs on 16-bit operands: the up-projection as three leading tiles of a three-part product (CatArgs: LEAD)
                    if (!a.save16) {   // passes that save nothing (evaluation): the MLP output, if wanted at all, in fp32
                        if (!a.row_map && !a.row_mask)
                            return run<AT, SPLIT, EpiFc2<AT, true>, 3>(a, EpiFc2<AT, true>{a.bias, a.out_f32, nullptr, nullptr, (AT*)a.h_out, resid, a.bias2, a.scale, a.row_scale}, s);
                        return run<AT, SPLIT, EpiFc2<AT, false>, 3>(a, EpiFc2<AT, false>{a.bias, a.out_f32, a.row_map, a.row_mask, (AT*)a.h_out, resid, a.bias2, a.scale, a.row_scale}, s);
                    }
                    if (!a.row_map && !a.row_mask)
                        return run<AT, SPLIT, EpiFc2<AT, true, bf16>, 3>(a, EpiFc2<AT, true, bf16>{a.bias, a.out_f32, nullptr, nullptr, (bf16*)a.h_out, resid, a.bias2, a.scale, a.row_scale}, s);
                    return run<AT, SPLIT, EpiFc2<AT, false, bf16>, 3>(a, EpiFc2<AT, false, bf16>{a.bias, a.out_f32, a.row_map, a.row_mask, (bf16*)a.h_out, resid, a.bias2, a.scale, a.row_scale}, s);
                } else {
                    set_error("gemm: the K-concatenated fc2 form exists in the 16-bit and the 16-bit-backward split modes only");
                    return -1;
                }
            }
            if constexpr (SPLIT) {
                if (a.save16 && a.h_out) {
                    if (!a.row_map && !a.row_mask) return run<AT, SPLIT>(a, EpiFc2<AT, true, bf16>{a.bias, a.out_f32, nullptr, nullptr, (bf16*)a.h_out, resid, nullptr, 0.f, a.row_scale}, s);
                    return run<AT, SPLIT>(a, EpiFc2<AT, false, bf16>{a.bias, a.out_f32, a.row_map, a.row_mask, (bf16*)a.h_out, resid, nullptr, 0.f, a.row_scale}, s);
                }
            }
            if (!a.row_map && !a.row_mask) return run<AT, SPLIT>(a, EpiFc2<AT, true>{a.bias, a.out_f32, nullptr, nullptr, (AT*)a.h_out, resid, nullptr, 0.f, a.row_scale}, s);
            return run<AT, SPLIT>(a, EpiFc2<AT, false>{a.bias, a.out_f32, a.row_map, a.row_mask, (AT*)a.h_out, resid, nullptr, 0.f, a.row_scale}, s);
        }
        case EPI_GELU_BWD:
            if (a.row_map) return run<AT, SPLIT>(a, EpiGeluBwd<AT, true>{(const AT*)a.aux_at, (AT*)a.out_at, a.N, a.row_map, (bf16*)a.out3, a.out3_scale, a.out3_hi_only}, s);
            return run<AT, SPLIT>(a, EpiGeluBwd<AT, false>{(const AT*)a.aux_at, (AT*)a.out_at, a.N, nullptr, (bf16*)a.out3, a.out3_scale, a.out3_hi_only}, s);
        case EPI_STORE_F32: return run<AT, SPLIT>(a, EpiStoreF32{a.out_f32, a.N, a.accumulate, a.scale, a.out_dscale}, s);
        case EPI_STORE_AT: return run<AT, SPLIT>(a, EpiStoreAT<AT>{(AT*)a.out_at, a.N, a.out_dscale}, s);
        case EPI_AD_DOWN:
            if constexpr (!SPLIT && sizeof(AT) == 4) {
                if (a.save16) return run<AT, SPLIT>(a, EpiAdDown<AT, bf16>{a.bias, (AT*)a.out_at, a.keep, a.r, a.inv_keep, a.drop_p, a.seed, a.subseq, a.row_map, a.seed_dev, (bf16*)a.out_at2, a.scale, (bf16*)a.out3, a.out3_scale}, s);
            }
            return run<AT, SPLIT>(a, EpiAdDown<AT>{a.bias, (AT*)a.out_at, a.keep, a.r, a.inv_keep, a.drop_p, a.seed, a.subseq, a.row_map, a.seed_dev, (AT*)a.out_at2, a.scale, (bf16*)a.out3, a.out3_scale}, s);
        case EPI_AD_UP:
            if (a.row_map) return run<AT, SPLIT>(a, EpiAdUp<true>{a.bias, a.resid, a.out_f32, a.scale, a.row_map, nullptr, a.row_scale, a.bias_scale}, s);
            return run<AT, SPLIT>(a, EpiAdUp<false>{a.bias, a.resid, a.out_f32, a.scale, nullptr, a.row_mask, nullptr, a.bias_scale}, s);
        case EPI_AD_DGRAD_UP:
            return run<AT, SPLIT>(a, EpiAdDgradUp<AT>{(const AT*)a.aux_at, (AT*)a.out_at, a.scale, a.inv_keep}, s);
        case EPI_EMBED: return run<AT, SPLIT>(a, EpiEmbed{a.bias, a.pos, a.out_f32}, s);
        case EPI_BIAS_AT: return run<AT, SPLIT>(a, EpiBiasAT<AT>{a.bias, (AT*)a.out_at, a.N}, s);
    }
    set_error("gemm: unknown epilogue %d", (int)kind);
    return -1;
}

// measurement hook: plain bf16 GEMM into a bf16 C with a selectable kernel variant
int launch_gemm_raw(const void* A, const void* W, void* C, int M, int N, int K, int variant, hipStream_t s) {
    if (K % 64 != 0 || N % 256 != 0 || M <= 0) { set_error("gemm_raw: bad shape"); return -1; }
    GemmArgs a; a.A = A; a.W = W; a.M = M; a.N = N; a.K = K;
    EpiStoreAT<bf16> epi{static_cast<bf16*>(C), N};
    switch (variant) {
        case 0: return launch_bf16_cfg<128, 128, 2, 2, 0>(a, epi, s);
        case 9: return launch_bf16_cfg<128, 128, 2, 2, 9>(a, epi, s);     // + phase timers
        case 10: return launch_bf16_cfg<256, 256, 2, 4, 0>(a, epi, s);
        case 19: return launch_bf16_cfg<256, 256, 2, 4, 9>(a, epi, s);
        case 30: return run_bf16(a, epi, s);                               // the product dispatch (incl. the split-row scheme)
        // residual epilogues with the phase timers: C is read as the fp32 residual stream [M,N] (the same bytes as bf16 [2M,N]), updated in place
        case 21: return launch_bf16_cfg<256, 256, 2, 4, 9>(a, EpiFc2<bf16, true>{nullptr, static_cast<float*>(C), nullptr, nullptr, nullptr, static_cast<const float*>(C), nullptr, 0.f}, s);
        case 22: return launch_bf16_cfg<128, 128, 2, 2, 9>(a, EpiBiasResid<bf16>{nullptr, static_cast<const float*>(C), static_cast<float*>(C), nullptr, N}, s);
        case 23: return launch_bf16_cfg<256, 256, 2, 4, 9>(a, EpiBiasResid<bf16>{nullptr, static_cast<const float*>(C), static_cast<float*>(C), nullptr, N}, s);
        case 40: case 41: case 42: {   // C = A2 W2^T + A W^T, A2 [M,64] stored behind A, W2 [N,64] behind W (leading k-tile form)
            a.A2 = static_cast<const bf16*>(A) + (size_t)M * K; a.W2 = static_cast<const bf16*>(W) + (size_t)N * K;
            if (variant == 40) return launch_bf16_cfg<128, 128, 2, 2, 0, EpiStoreAT<bf16>, true>(a, epi, s);
            if (variant == 41) return launch_bf16_cfg<256, 256, 2, 4, 0, EpiStoreAT<bf16>, true>(a, epi, s);
            return run_bf16<EpiStoreAT<bf16>, true>(a, epi, s);
        }
        case 70: case 79: {   // pre-shuffled-weight kernel (test-only: shuffles W into a cached scratch buffer first)
            static bf16* wp = nullptr; static size_t wp_elems = 0;
            const size_t need = (size_t)N * K;
            if (need > wp_elems) {
                if (wp) (void)hipFree(wp);
                DYT_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&wp), need * 2));
                wp_elems = need;
            }
            if (launch_preshuffle_w(W, wp, N, K, s)) return -2;
            GemmArgs b = a; b.W = wp;
            if (variant == 70) return launch_bf16_bpre<0>(b, epi, s);
            return launch_bf16_bpre<9>(b, epi, s);
        }
    }
    set_error("gemm_raw: unknown variant %d", variant);
    return -1;
}

// measurement hook: fp32 GEMM (exact-fp32 MFMA kernel, product dispatch) into an fp32 C [M,N]
// variant 0: plain store; 1: EpiAdUp reading the residual from C + M*N and writing C; 2: EpiStoreF32 accumulate (C += A W^T)
int launch_gemm_f32_raw(const void* A, const void* W, void* C, int M, int N, int K, int variant, hipStream_t s) {
    GemmArgs a; a.A = A; a.W = W; a.M = M; a.N = N; a.K = K;
    float* c = static_cast<float*>(C);
    if (variant == 1) return run_f32(a, EpiAdUp<false>{nullptr, c + (size_t)M * N, c, 0.1f, nullptr, nullptr}, s);
    if (variant == 2) return run_f32(a, EpiStoreF32{c, N, 1, 1.0f}, s);
    return run_f32(a, EpiStoreAT<float>{c, N}, s);
}

int gemm_debug_counters(unsigned long long* out4, int reset) {
    DYT_HIP_CHECK(hipDeviceSynchronize());
    DYT_HIP_CHECK(hipMemcpyFromSymbol(out4, HIP_SYMBOL(g_gemm_dbg), 4 * sizeof(unsigned long long)));
    if (reset) {
        unsigned long long z[4] = {0, 0, 0, 0};
        DYT_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_gemm_dbg), z, sizeof(z)));
    }
    return 0;
}

// ---- fp32 operands as 16-bit hi / lo parts ----
// A [M,K] fp32 (rows optionally gathered) -> out [M, 3K] = [hi | hi | lo]; one thread = 8 consecutive k of a row
__global__ __launch_bounds__(256) void split3_a_kernel(const float* __restrict__ A, const int* __restrict__ a_map,
                                                       const int* __restrict__ m_dev, bf16* __restrict__ out, int M, int K, float scale, int f8) {
    const int kc = K / 8;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int row = (int)(idx / kc), c = (int)(idx - (size_t)row * kc);
    const int Mv = m_dev ? min(*m_dev, M) : M;
    if (row >= Mv) return;
    const float* src = A + (size_t)(a_map ? a_map[row] : row) * K + c * 8;
    const f32x4 x0 = *reinterpret_cast<const f32x4*>(src) * scale, x1 = *reinterpret_cast<const f32x4*>(src + 4) * scale;
    if (f8) {   // hi16 / fp8 form (store4_split_f8)
        bf16* rowp = out + (size_t)row * SPLIT_A * K;
        store4_split_f8(rowp, K, c * 8, x0[0], x0[1], x0[2], x0[3]);
        store4_split_f8(rowp, K, c * 8 + 4, x1[0], x1[1], x1[2], x1[3]);
        return;
    }
    bf16x8 hi, lo;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const Split2 s0 = split2(x0[i]), s1 = split2(x1[i]);
        hi[i] = s0.hi; lo[i] = s0.lo;
        hi[4 + i] = s1.hi; lo[4 + i] = s1.lo;
    }
    bf16* dst = out + (size_t)row * SPLIT_A * K + c * 8;
    *reinterpret_cast<bf16x8*>(dst) = hi;
    *reinterpret_cast<bf16x8*>(dst + K) = lo;
}
// W [N,K] fp32 -> [N, 2K] = [hi | lo]; the contraction reads it as [hi | lo | hi] (the B loader folds the last third onto the first)
__global__ __launch_bounds__(256) void split3_w_kernel(const float* __restrict__ W, bf16* __restrict__ out, int N, int K) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)N * K) return;
    const size_t row = idx / K; const int k = (int)(idx - row * K);
    const float w = W[idx];
    const Split2 sw = split2(w);
    const bf16 hi = sw.hi, lo = sw.lo;
    bf16* dst = out + row * SPLIT_A * K;
    dst[k] = hi; dst[K + k] = lo;
}
// hi16 / fp8 form of a weight: [N][hi16 (K) | e4m3(lo 2^(ew+11)) (K bytes) | e4m3(hi 2^ew) (K bytes)], ew = 7 - ceil(log2 max|w|)
__global__ __launch_bounds__(256) void absmax_kernel(const float* __restrict__ W, size_t n, unsigned* __restrict__ out) {
    float m = 0.f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) m = fmaxf(m, fabsf(W[i]));
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) atomicMax(out, __float_as_uint(m));   // non-negative floats order like their bit patterns
}
__device__ __forceinline__ int weight_exp(unsigned maxbits) {
    const float m = __uint_as_float(maxbits);
    if (!(m > 0.f) || !(m < 3.0e38f)) return 0;
    int e;
    const float f = frexpf(m, &e);          // m = f 2^e, f in [0.5, 1): ceil(log2 m) = e, or e - 1 when m is a power of two
    const int cl = f == 0.5f ? e - 1 : e;
    return max(-60, min(60, 7 - cl));
}
__global__ __launch_bounds__(256) void split_w_f8_kernel(const float* __restrict__ W, bf16* __restrict__ out, int N, int K,
                                                         const unsigned* __restrict__ maxbits, int* __restrict__ ew_out) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;   // 4 consecutive k of a row
    const int ew = weight_exp(*maxbits);
    if (idx == 0) *ew_out = ew;
    if (idx >= (size_t)N * K / 4) return;
    const size_t row = idx / (K / 4); const int k = (int)(idx - row * (K / 4)) * 4;
    f32x4 w = *reinterpret_cast<const f32x4*>(W + row * K + k);
    asm("" : "+v"(w));
    const bf16 h0 = (bf16)w[0], h1 = (bf16)w[1], h2 = (bf16)w[2], h3 = (bf16)w[3];
    bf16* rowp = out + row * SPLIT_A * K;
    *reinterpret_cast<bf16x4*>(rowp + k) = bf16x4{h0, h1, h2, h3};
    const float sh = ldexpf(1.0f, ew), sl = ldexpf(1.0f, ew + 11);
    unsigned char* r8 = reinterpret_cast<unsigned char*>(rowp) + 2 * (size_t)K + k;
    *reinterpret_cast<int*>(r8) = pack4_e4m3((w[0] - (float)h0) * sl, (w[1] - (float)h1) * sl, (w[2] - (float)h2) * sl, (w[3] - (float)h3) * sl);
    *reinterpret_cast<int*>(r8 + K) = pack4_e4m3((float)h0 * sh, (float)h1 * sh, (float)h2 * sh, (float)h3 * sh);
}
int launch_split_w_f8(const float* W, void* W3, int N, int K, int* ew_dev, unsigned* scratch, hipStream_t s) {
    DYT_HIP_CHECK(hipMemsetAsync(scratch, 0, sizeof(unsigned), s));
    const size_t n = (size_t)N * K;
    hipLaunchKernelGGL(absmax_kernel, dim3((unsigned)std::min<size_t>(1024, (n + 255) / 256)), dim3(256), 0, s, W, n, scratch);
    hipLaunchKernelGGL(split_w_f8_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, s, W, static_cast<bf16*>(W3), N, K, scratch, ew_dev);
    DYT_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_split3_w(const float* W, void* W3, int N, int K, hipStream_t s) {
    hipLaunchKernelGGL(split3_w_kernel, dim3((unsigned)(((size_t)N * K + 255) / 256)), dim3(256), 0, s, W, static_cast<bf16*>(W3), N, K);
    DYT_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_gemm(int precision, EpiKind kind, const GemmArgs& a, hipStream_t s) {
    if (precision == 0 && a.W3 && a.a3) {
        if (a.K % 64 != 0 || (a.A2 && kind != EPI_FC2)) { set_error("gemm split form: K=%d %% 64", a.K); return -1; }
        const size_t tasks = (size_t)a.M * (a.K / 8);
        if (!a.a3_ready)
        hipLaunchKernelGGL(split3_a_kernel, dim3((unsigned)((tasks + 255) / 256)), dim3(256), 0, s, static_cast<const float*>(a.A), a.a_map,
                           a.m_dev, static_cast<bf16*>(a.a3), a.M, a.K, a.a3_scale, a.f8 ? 1 : 0);
        GemmArgs b = a;
        // a3_parts products of the contraction: 3 = hi*hi + hi*lo + lo*hi, 2 = hi * (hi + lo) (A rounded to half, W exact), 1 = hi*hi
        b.A = a.a3; b.W = a.W3; b.K = a.a3_parts * a.K; b.a_fold = a.K / 64; b.a_ld = 2 * a.K; b.a_map = (a.a3_ready && a.a3_mapped) ? a.a_map : nullptr; b.Wp = nullptr; b.W3 = nullptr; b.out_scale = 1.0f / a.a3_scale;
        if (a.f8) {   // hi * hi as f16 tiles, then the two correction products as fp8 tiles along the same rows
            if (a.K % 128 != 0 || a.a3_parts != 3 || a.a3_scale != 1.0f || !a.w_exp) { set_error("gemm f8 form: K=%d %% 128, forward operands only", a.K); return -1; }
            b.K = 2 * a.K; b.a_fold = 0; b.f8_begin = a.K / 64;
        }
        return dispatch<float, true>(kind, b, s);
    }
    if (dbg_skip(64) && (a.K == RP || a.N == RP)) return 0;
    if (dbg_skip(128) && a.N == D && a.K >= 256) return 0;
    if (dbg_skip(256) && a.N >= 2304) return 0;
    return precision == 0 ? dispatch<float>(kind, a, s) : dispatch<bf16>(kind, a, s);
}

}  // namespace dyt
