// Wide classification head (DYT_CREATE_WIDE_HEAD): final LayerNorm of the cls rows + Linear(768, C) for C up to 65 536, forward
// and backward, as exact-fp32 MFMA GEMMs (v_mfma_f32_32x32x2_f32: bit for bit a k-ordered fmaf chain, in every precision mode).
//
// The row kernels of step_tail.hip (head_fwd / head_bwd_dx / head_bwd_dw) walk all C rows of head.weight once per image and stage a
// dlogits row in a 1024-float LDS array: right at C = 100 ... 1000, where the head is microseconds.  At C = 21 843 (the
// ImageNet-21K classifier) and B = 128 the three products are 4.3 GFLOP GEMMs over a 67 MB matrix; here each reads it once per
// 64 images:
//   head_wide_ln_kernel        cls_n = LN(x[cls rows]), stats                     (the first half of head_fwd_kernel, same arithmetic)
//   head_wide_logits_kernel    logits [B,C] = cls_n x head_w^T + head_b           NT product, K = 768
//   head_wide_dx_kernel        P[slice] [B,768] = dlogits[:, slice] x head_w[slice]   contraction over <= 1024 classes per slice
//   head_wide_dx_finish_kernel g = LNbwd(sum_slices P[slice]) in slice order     (the second half of head_bwd_dx_kernel)
//   head_wide_dw_kernel        dW [C,768] += dlogits^T x cls_n, db += colsum      TN product, contraction over the batch
// No 16-bit operand, no atomic: every output element has one writer and one summation order, so results are bit-reproducible.
// The class slices of dx are a CONDITION: an unsliced fp32 chain over 21 843 classes is 11x the fp32 reference's own error; slices
// of at most 1024 classes, each summed as chains of 256 and added in order, stay near 1x.
//
// Every index below comes from head_wide_idx.h, which tools/head_wide_index_check.cpp walks on the CPU.  head_w lives in the
// CALLER's flat trainable buffer: rows >= C are clamped (logits) or zero-filled without a read (dx), columns >= C never stored.
#include "kernels.h"
#include "rowhelp.h"
#include "head_wide_idx.h"

namespace dyt {

using namespace hw;

// ------------------------------------------------------------------------------------------------------------------------------
// final LayerNorm of the cls rows (x row b at x + b * x_stride)
// ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void head_wide_ln_kernel(const float* __restrict__ x, size_t x_stride, const float* __restrict__ nw,
                                                           const float* __restrict__ nb, float* __restrict__ cls_n,
                                                           float2* __restrict__ stats) {
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* xp = x + (size_t)b * x_stride;
    float v[3];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) { v[i] = xp[tid + 256 * i]; s += v[i]; }
    const float mean = block_sum256(s, red) * (1.0f / D);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) { const float d = v[i] - mean; q = fmaf(d, d, q); }
    const float rstd = 1.0f / sqrtf(block_sum256(q, red) * (1.0f / D) + LN_EPS);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int c = tid + 256 * i;
        cls_n[(size_t)b * D + c] = (v[i] - mean) * rstd * nw[c] + nb[c];
    }
    if (tid == 0) stats[b] = make_float2(mean, rstd);
}

// ------------------------------------------------------------------------------------------------------------------------------
// logits
// ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void head_wide_logits_kernel(const float* __restrict__ A, const float* __restrict__ W,
                                                               const float* __restrict__ bias, float* __restrict__ out, int B, int C) {
    __shared__ __attribute__((aligned(16))) float lds[LG_LDS_FLOATS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = blockIdx.x * BN, m0 = blockIdx.y * BM;
    f32x16 acc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    f32x4 ga[LG_A_PER_THREAD], gw[LG_W_PER_THREAD];
    auto gload = [&](int kt) {
#pragma unroll
        for (int t = 0; t < LG_A_PER_THREAD; ++t) ga[t] = *reinterpret_cast<const f32x4*>(A + lg_stage(tid, t, kt, m0, B, 0).off);
#pragma unroll
        for (int t = 0; t < LG_W_PER_THREAD; ++t) gw[t] = *reinterpret_cast<const f32x4*>(W + lg_stage(tid, t, kt, n0, C, LG_A_FLOATS).off);
    };
    auto gstore = [&]() {
#pragma unroll
        for (int t = 0; t < LG_A_PER_THREAD; ++t) *reinterpret_cast<f32x4*>(lds + lg_stage(tid, t, 0, m0, B, 0).lds) = ga[t];
#pragma unroll
        for (int t = 0; t < LG_W_PER_THREAD; ++t) *reinterpret_cast<f32x4*>(lds + lg_stage(tid, t, 0, n0, C, LG_A_FLOATS).lds) = gw[t];
    };
    constexpr int nk = D / BK;
    gload(0);
    for (int kt = 0; kt < nk; ++kt) {
        DYT_VMEM_DRAIN();
        gstore();
        __syncthreads();
        if (kt + 1 < nk) gload(kt + 1);   // in flight under this stage's MFMAs
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const f32x4 w = *reinterpret_cast<const f32x4*>(lds + lg_frag(LG_A_FLOATS, wave * 32 + (lane & 31), lane, j));
            const f32x4 a0 = *reinterpret_cast<const f32x4*>(lds + lg_frag(0, (lane & 31), lane, j));
            const f32x4 a1 = *reinterpret_cast<const f32x4*>(lds + lg_frag(0, 32 + (lane & 31), lane, j));
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[t], a0[t], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[t], a1[t], acc[1], 0, 0, 0);
            }
        }
        __syncthreads();   // every wave has read this stage before the next one is parked
    }
    // acc[i][4g + e] = logits[m0 + 32 i + (lane & 31)][n0 + 32 wave + 8g + 4(lane >> 5) + e]
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const Out o = lg_out(m0, n0, wave, lane, i, g, B, C);
            if (o.nvalid == 0) continue;
            const int n = n0 + acc_col(wave, lane, g);
            if (o.vec) {
                const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + n);
                const f32x4 v = {acc[i][4 * g] + bv[0], acc[i][4 * g + 1] + bv[1], acc[i][4 * g + 2] + bv[2], acc[i][4 * g + 3] + bv[3]};
                *reinterpret_cast<f32x4*>(out + o.off) = v;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (e < o.nvalid) out[o.off + e] = acc[i][4 * g + e] + bias[n + e];
            }
        }
}

// ------------------------------------------------------------------------------------------------------------------------------
// dx partial sums per class slice
// ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void head_wide_dx_kernel(const float* __restrict__ dl, const float* __restrict__ W,
                                                           float* __restrict__ part, int B, int C) {
    __shared__ __attribute__((aligned(16))) float lds[DX_LDS_FLOATS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = blockIdx.x * BN, m0 = blockIdx.y * BM, sl = blockIdx.z;
    f32x16 acc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    float ga[DX_A_PER_THREAD];
    f32x4 gw[DX_W_PER_THREAD];
    auto gload = [&](int kt) {
#pragma unroll
        for (int t = 0; t < DX_A_PER_THREAD; ++t) {
            const Src r = dx_stage_a(tid, t, kt, m0, sl, B, C);
            ga[t] = r.valid ? dl[r.off] : 0.f;
        }
#pragma unroll
        for (int t = 0; t < DX_W_PER_THREAD; ++t) {
            const Src r = dx_stage_w(tid, t, kt, n0, sl, C);
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            gw[t] = r.valid ? *reinterpret_cast<const f32x4*>(W + r.off) : z;
        }
    };
    auto gstore = [&]() {
#pragma unroll
        for (int t = 0; t < DX_A_PER_THREAD; ++t) lds[dx_stage_a(tid, t, 0, m0, sl, B, C).lds] = ga[t];
#pragma unroll
        for (int t = 0; t < DX_W_PER_THREAD; ++t) *reinterpret_cast<f32x4*>(lds + dx_stage_w(tid, t, 0, n0, sl, C).lds) = gw[t];
    };
    // The fmaf chain of one accumulator is DX_CHAIN_STAGES * 32 = 256 classes long: after that many stages it is added to the slice's
    // running sum and restarted (a 1024-class chain measured 4.08x the fp32 reference's own error at C = 1025, chains of 256 stay near 1x).
    f32x16 tot[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) tot[i][r] = 0.f;
    const int nk = slice_stages(sl, C);
    gload(0);
    for (int kt = 0; kt < nk; ++kt) {
        DYT_VMEM_DRAIN();
        gstore();
        __syncthreads();
        if (kt + 1 < nk) gload(kt + 1);
#pragma unroll
        for (int kp = 0; kp < BK / 2; ++kp) {
            const float w = lds[dx_frag_w(wave, lane, kp)];
            const float a0 = lds[dx_frag_a(0, lane, kp)], a1 = lds[dx_frag_a(1, lane, kp)];
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(w, a0, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(w, a1, acc[1], 0, 0, 0);
        }
        if ((kt % DX_CHAIN_STAGES) == DX_CHAIN_STAGES - 1 || kt == nk - 1) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) { tot[i][r] += acc[i][r]; acc[i][r] = 0.f; }
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) acc[i] = tot[i];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const Out o = dx_out(m0, n0, sl, wave, lane, i, g, B);
            if (o.nvalid == 0) continue;
            const f32x4 v = {acc[i][4 * g], acc[i][4 * g + 1], acc[i][4 * g + 2], acc[i][4 * g + 3]};
            *reinterpret_cast<f32x4*>(part + o.off) = v;
        }
}

// slices added in ascending order, then the LayerNorm backward of the cls row (head_bwd_dx_kernel's second half)
__global__ __launch_bounds__(256) void head_wide_dx_finish_kernel(const float* __restrict__ part, int nslices,
                                                                  const float* __restrict__ x, size_t x_stride,
                                                                  const float2* __restrict__ stats, const float* __restrict__ nw,
                                                                  float* __restrict__ g, size_t g_stride, int B,
                                                                  float* __restrict__ dy_out) {
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float2 st = stats[b];
    float dy[3], xh[3];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int ch = tid + 256 * i;
        float acc = part[(size_t)b * D + ch];
        for (int s = 1; s < nslices; ++s) acc += part[((size_t)s * B + b) * D + ch];
        if (dy_out) dy_out[(size_t)b * D + ch] = acc;   // the gradient behind the LayerNorm (a trainable fc_norm's parameter gradients)
        xh[i] = (x[(size_t)b * x_stride + ch] - st.x) * st.y;
        dy[i] = acc * nw[ch];
        s1 += dy[i];
        s2 = fmaf(dy[i], xh[i], s2);
    }
    s1 = block_sum256(s1, red) * (1.0f / D);
    s2 = block_sum256(s2, red) * (1.0f / D);
#pragma unroll
    for (int i = 0; i < 3; ++i) g[(size_t)b * g_stride + tid + 256 * i] = st.y * (dy[i] - s1 - xh[i] * s2);
}

// ------------------------------------------------------------------------------------------------------------------------------
// dW, db (accumulated: += like head_bwd_dw_kernel)
// ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void head_wide_dw_kernel(const float* __restrict__ dl, const float* __restrict__ X,
                                                           float* __restrict__ dW, float* __restrict__ db, int B, int C) {
    __shared__ __attribute__((aligned(16))) float lds[DW_LDS_FLOATS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = blockIdx.x * BN, c0 = blockIdx.y * BM;
    const bool do_db = db != nullptr && blockIdx.x == 0 && tid < BM;
    f32x16 acc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    float sb = 0.f;
    float ga[DW_A_PER_THREAD];
    f32x4 gx[DW_X_PER_THREAD];
    auto gload = [&](int kt) {
#pragma unroll
        for (int t = 0; t < DW_A_PER_THREAD; ++t) {
            const Src r = dw_stage_a(tid, t, kt, c0, B, C);
            ga[t] = r.valid ? dl[r.off] : 0.f;
        }
#pragma unroll
        for (int t = 0; t < DW_X_PER_THREAD; ++t) {
            const Src r = dw_stage_x(tid, t, kt, n0, B);
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            gx[t] = r.valid ? *reinterpret_cast<const f32x4*>(X + r.off) : z;
        }
    };
    auto gstore = [&]() {
#pragma unroll
        for (int t = 0; t < DW_A_PER_THREAD; ++t) lds[dw_stage_a(tid, t, 0, c0, B, C).lds] = ga[t];
#pragma unroll
        for (int t = 0; t < DW_X_PER_THREAD; ++t) *reinterpret_cast<f32x4*>(lds + dw_stage_x(tid, t, 0, n0, B).lds) = gx[t];
    };
    const int nk = dw_stages(B);
    gload(0);
    for (int kt = 0; kt < nk; ++kt) {
        DYT_VMEM_DRAIN();
        gstore();
        __syncthreads();
        if (kt + 1 < nk) gload(kt + 1);
        if (dW) {
#pragma unroll
            for (int kp = 0; kp < BK / 2; ++kp) {
                const float w = lds[dw_frag_x(wave, lane, kp)];
                const float a0 = lds[dw_frag_a(0, lane, kp)], a1 = lds[dw_frag_a(1, lane, kp)];
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(w, a0, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(w, a1, acc[1], 0, 0, 0);
            }
        }
        if (do_db) {   // the staged dlogits image's column of class c0 + tid, images in ascending order (zero-filled rows add 0)
#pragma unroll
            for (int k = 0; k < BK; ++k) sb += lds[dw_db_lds(tid, k)];
        }
        __syncthreads();
    }
    if (dW) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const Out o = dw_out(c0, n0, wave, lane, i, g, C);
                if (o.nvalid == 0) continue;
                f32x4* p = reinterpret_cast<f32x4*>(dW + o.off);
                f32x4 v = *p;
                v[0] += acc[i][4 * g]; v[1] += acc[i][4 * g + 1]; v[2] += acc[i][4 * g + 2]; v[3] += acc[i][4 * g + 3];
                *p = v;
            }
    }
    if (do_db && c0 + tid < C) db[c0 + tid] += sb;
}

// ------------------------------------------------------------------------------------------------------------------------------
// launches
// ------------------------------------------------------------------------------------------------------------------------------
size_t head_wide_scratch_floats(int batch, int C) { return (size_t)n_slices(C) * batch * D; }

static int head_wide_args(const char* what, int batch, int C) {
    if (batch < 1 || C < 1 || C > MAX_C) { set_error("%s: batch %d, num_classes %d (1..%d)", what, batch, C, MAX_C); return -1; }
    return 0;
}

int launch_head_wide_fwd(const float* x, size_t x_stride, const float* nw, const float* nb, const float* hw, const float* hb,
                         float* cls_n, float2* stats, float* logits, int batch, int C, hipStream_t s) {
    if (head_wide_args("head_wide_fwd", batch, C)) return -1;
    hipLaunchKernelGGL(head_wide_ln_kernel, dim3(batch), dim3(256), 0, s, x, x_stride, nw, nb, cls_n, stats);
    hipLaunchKernelGGL(head_wide_logits_kernel, dim3(ceil_div(C, BN), ceil_div(batch, BM)), dim3(THREADS), 0, s, cls_n, hw, hb,
                       logits, batch, C);
    LAUNCH_CHECK();
    return 0;
}

int launch_head_wide_bwd(const float* dlogits, const float* x, size_t x_stride, const float* cls_n, const float2* stats,
                         const float* nw, const float* hw, float* g, float* dWh, float* dbh, int batch, int C, int compact,
                         float* part, hipStream_t s, float* dy_out) {
    if (head_wide_args("head_wide_bwd", batch, C)) return -1;
    if (g) {
        if (!part) { set_error("head_wide_bwd: no slice scratch"); return -1; }
        if (!compact) DYT_HIP_CHECK(hipMemsetAsync(g, 0, (size_t)batch * NT * D * sizeof(float), s));
        hipLaunchKernelGGL(head_wide_dx_kernel, dim3(D / BN, ceil_div(batch, BM), n_slices(C)), dim3(THREADS), 0, s, dlogits, hw, part,
                           batch, C);
        hipLaunchKernelGGL(head_wide_dx_finish_kernel, dim3(batch), dim3(256), 0, s, part, n_slices(C), x, x_stride, stats, nw, g,
                           compact ? (size_t)D : (size_t)NT * D, batch, dy_out);
    }
    if (dWh || dbh)
        hipLaunchKernelGGL(head_wide_dw_kernel, dim3(D / BN, ceil_div(C, BM)), dim3(THREADS), 0, s, dlogits, cls_n, dWh, dbh, batch, C);
    LAUNCH_CHECK();
    return 0;
}

}  // namespace dyt
