// LayerNorm row kernels of the DyT hot path (gfx950): forward, backward, the adapter's own LayerNorm with its parameter
// gradients, and the weight side of the folded form.  HBM-bound: one 64-lane wave owns one 768-channel token row
// (3 x float4 per lane, fully coalesced), reductions are wave shuffles.
//
// Reference ops replaced (paths relative to the reference root):
//   nn.LayerNorm(eps=1e-6)                      models/vision_transformer_IN21K.py:110,123,314
#include "kernels.h"
#include "rowhelp.h"

namespace dyt {

// A/B switches of the probes (tools/probes/README.md): which of the full drains of ln_bwd are compiled in
#if defined(DYT_NOPIN_LN) || defined(DYT_NOPIN_ROWS)
#define LN_ROWPIN(x)
#else
#define LN_ROWPIN(x) (x).landed()
#endif
#if defined(DYT_NOPIN_LN) || defined(DYT_NOPIN_SCALARS)
#define LN_SCALPIN3(a, b, c)
#else
#define LN_SCALPIN3(a, b, c) DYT_PIN3(a, b, c)
#endif

// ------------------------------------------------------------------------------------------
// LayerNorm forward / backward
// ------------------------------------------------------------------------------------------
template <class AT>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                     const float* __restrict__ b, AT* __restrict__ out,
                                                     float2* __restrict__ stats, int rows, bf16* __restrict__ out3, int f8) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    Row12 xr, wr, br;
    xr.load(x + (size_t)row * D, lane);
    wr.load(w, lane);
    br.load(b, lane);
    xr.landed(); wr.landed(); br.landed();   // one full drain for the whole load group (DYT_PIN*, dyt_common.h)
    const float2 st = ln_stats(xr);
#pragma unroll
    for (int i = 0; i < 12; ++i) xr.v[i] = (xr.v[i] - st.x) * st.y * wr.v[i] + br.v[i];
    if (out3) {   // fp32 split form: the row as the 16-bit hi / hi / lo operand of the next GEMM
#pragma unroll
        for (int i = 0; i < 3; ++i)
            if (f8) store4_split_f8(out3 + (size_t)row * SPLIT_A * D, D, i * 256 + lane * 4, xr.v[4 * i], xr.v[4 * i + 1], xr.v[4 * i + 2], xr.v[4 * i + 3]);
            else store4_split3(out3 + (size_t)row * SPLIT_A * D + i * 256 + lane * 4, D, xr.v[4 * i], xr.v[4 * i + 1], xr.v[4 * i + 2], xr.v[4 * i + 3]);
    } else {
        xr.store(out + (size_t)row * D, lane);
    }
    if (stats && lane == 0) stats[row] = st;
}

// dx = base + LNbwd(dy).  Optionally also does the NEXT (lower) block's backward prep on the row it just
// produced (saves re-reading the 77 MB gradient): AT copy of dx, and <dx, h_next> for the gate gradient.
// The kernel's body, shared by the two kernels below as TEXT (a macro, not a device function: behind a function the compiler orders the
// operands of some commutative instructions of the untapped kernels differently, and those kernels are to stay the code they were).
// Every load of the row is issued up front and completed by ONE full drain that names all of them (DYT_PIN*, dyt_common.h).
// base_at (fp16 mode): the gradient stream this row's LayerNorm gradient is added to arrives as the 16-bit, gs-scaled copy the kernel before
// wrote for its GEMM (tok_bwd's du_at) instead of as an fp32 [M,768] stream; dx == null: no fp32 copy is written either.
// TAP (a compile-time constant; token-gradient entry, dyt_backward_tokens): one more fp32 row, the caller's gradient of this residual-stream
// snapshot, loaded up front with the others (same drain) and added in fp32 behind base / base_at -- before dx, out3, g_at and <dx, h_next>
// are formed, so a tap gradient costs one row read and no rounding of its own.
#define LN_BWD_BODY(TAP) \
    const int lane = threadIdx.x & 63;                                               \
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);                             \
    if (row >= rows) return;                                                         \
    Row12 g, xr, wr, br, tr;                                                         \
    g.load_at(dy + (size_t)row * D, lane);                                           \
    xr.load_nt(x + (size_t)row * D, lane);                                           \
    wr.load(w, lane);                                                                \
    float2 st = stats[row];                                                          \
    int r = dst_of_next ? dst_of_next[row] : row;                                    \
    if (base_at) br.load_at(base_at + (size_t)row * D, lane);                        \
    else if (base) br.load(base + (size_t)row * D, lane);                            \
    if (TAP) tr.load(tap + (size_t)row * D, lane);                                   \
    LN_ROWPIN(g); LN_ROWPIN(xr); LN_ROWPIN(wr);                                      \
    LN_SCALPIN3(st.x, st.y, r);                                                      \
    if (base || base_at) LN_ROWPIN(br);                                              \
    if (TAP) LN_ROWPIN(tr);                                                          \
    ln_bwd_row(g, xr, wr, st);                                                       \
_Pragma("unroll")                                                                    \
    for (int i = 0; i < 12; ++i) g.v[i] *= inv_gs;                                   \
    if (base_at) {                                                                   \
_Pragma("unroll")                                                                    \
        for (int i = 0; i < 12; ++i) g.v[i] = fmaf(br.v[i], inv_gs, g.v[i]);         \
    } else if (base) {                                                               \
_Pragma("unroll")                                                                    \
        for (int i = 0; i < 12; ++i) g.v[i] += br.v[i];                              \
    }                                                                                \
    if (TAP) {                                                                       \
_Pragma("unroll")                                                                    \
        for (int i = 0; i < 12; ++i) g.v[i] += tr.v[i];                              \
    }                                                                                \
    if (dx) g.store(dx + (size_t)row * D, lane);                                     \
    if (out3) g.store_split3(out3 + (size_t)row * SPLIT_A * D, lane, s3, hi3 != 0);  \
    if (g_at) {                                                                      \
        Row12 gsc;                                                                   \
_Pragma("unroll")                                                                    \
        for (int i = 0; i < 12; ++i) gsc.v[i] = g.v[i] * gs;                         \
        gsc.store(g_at + (size_t)row * D, lane);                                     \
    }                                                                                \
    if (dmask_next) {                                                                \
        float dm = 0.f;                                                              \
        if (h_next && r >= 0) {                                                      \
            Row12 hr;                                                                \
            hr.load_at(h_next + (size_t)r * D, lane);                                \
            LN_ROWPIN(hr);                                                           \
            dm = dot12(g, hr);                                                       \
        }                                                                            \
        if (lane == 0) dmask_next[row] = dm;                                         \
    }
template <class AT>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const AT* __restrict__ dy, const float* __restrict__ x,
                                                     const float2* __restrict__ stats, const float* __restrict__ w,
                                                     const float* __restrict__ base, float* __restrict__ dx, int rows,
                                                     AT* __restrict__ g_at, const AT* __restrict__ h_next,
                                                     const int* __restrict__ dst_of_next, float* __restrict__ dmask_next,
                                                     float gs, float inv_gs, bf16* __restrict__ out3, float s3, int hi3,
                                                     const AT* __restrict__ base_at) {
    constexpr const float* tap = nullptr;   // (named by the body's TAP branches, which are not compiled in here)
    LN_BWD_BODY(false)
}
template <class AT>
__global__ __launch_bounds__(256) void ln_bwd_tap_kernel(const AT* __restrict__ dy, const float* __restrict__ x,
                                                         const float2* __restrict__ stats, const float* __restrict__ w,
                                                         const float* __restrict__ base, float* __restrict__ dx, int rows,
                                                         AT* __restrict__ g_at, const AT* __restrict__ h_next,
                                                         const int* __restrict__ dst_of_next, float* __restrict__ dmask_next,
                                                         float gs, float inv_gs, bf16* __restrict__ out3, float s3, int hi3,
                                                         const AT* __restrict__ base_at, const float* __restrict__ tap) {
    LN_BWD_BODY(true)
}

// (mean, rstd) of every row alone: the final norm's statistics over all 197 rows of an image, which no forward pass keeps (the head
// normalises the cls row only) -- dyt_backward_tokens recomputes them in front of the final norm's backward
__global__ __launch_bounds__(256) void ln_stats_kernel(const float* __restrict__ x, float2* __restrict__ stats, int rows) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    Row12 xr;
    xr.load(x + (size_t)row * D, lane);
    xr.landed();
    const float2 st = ln_stats(xr);
    if (lane == 0) stats[row] = st;
}
// out = a + b (b null: a copy): the top of the gradient stream where the final norm is an identity, or where only the top tap has a gradient
__global__ __launch_bounds__(256) void rows_add_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, int rows) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    Row12 ar, br;
    ar.load(a + (size_t)row * D, lane);
    if (b) br.load(b + (size_t)row * D, lane);
    ar.landed();
    if (b) {
        br.landed();
#pragma unroll
        for (int i = 0; i < 12; ++i) ar.v[i] += br.v[i];
    }
    ar.store(out + (size_t)row * D, lane);
}

int launch_ln_fwd(int precision, const float* x, const float* w, const float* b, void* out, float2* stats, int rows,
                  hipStream_t s, void* out3, int out3_f8) {
    const int grid = (rows + 3) / 4;
    if (dbg_skip(32)) return 0;
    if (precision == 0)
        hipLaunchKernelGGL(ln_fwd_kernel<float>, dim3(grid), dim3(256), 0, s, x, w, b, (float*)out, stats, rows, (bf16*)out3, out3_f8);
    else
        hipLaunchKernelGGL(ln_fwd_kernel<bf16>, dim3(grid), dim3(256), 0, s, x, w, b, (bf16*)out, stats, rows, (bf16*)nullptr, 0);
    LAUNCH_CHECK();
    return 0;
}
int launch_ln_fwd_f32out(const float* x, const float* w, const float* b, float* out, int rows, hipStream_t s) {
    return launch_ln_fwd(0, x, w, b, out, nullptr, rows, s);
}
int launch_ln_bwd(int precision, const void* dy, const float* x, const float2* stats, const float* w, const float* base,
                  float* dx, int rows, void* g_at, const void* h_next, const int* dst_of_next, float* dmask_next,
                  float gs, hipStream_t s, void* out3, float s3, int out3_hi_only, const void* base_at, const float* tap) {
    if (dbg_skip(16)) return 0;
    if (tap) {   // the tapped instantiations (dyt_backward_tokens); everything else launches the kernels it always did
        if (precision == 0)
            hipLaunchKernelGGL(ln_bwd_tap_kernel<float>, dim3((rows + 3) / 4), dim3(256), 0, s, (const float*)dy, x, stats, w, base, dx,
                               rows, (float*)g_at, (const float*)h_next, dst_of_next, dmask_next, 1.0f, 1.0f, (bf16*)out3, s3, out3_hi_only, (const float*)nullptr, tap);
        else
            hipLaunchKernelGGL(ln_bwd_tap_kernel<bf16>, dim3((rows + 3) / 4), dim3(256), 0, s, (const bf16*)dy, x, stats, w, base, dx,
                               rows, (bf16*)g_at, (const bf16*)h_next, dst_of_next, dmask_next, gs, 1.0f / gs, (bf16*)nullptr, 1.0f, 0, (const bf16*)base_at, tap);
        LAUNCH_CHECK();
        return 0;
    }
    if (precision == 0)
        hipLaunchKernelGGL(ln_bwd_kernel<float>, dim3((rows + 3) / 4), dim3(256), 0, s, (const float*)dy, x, stats, w, base, dx,
                           rows, (float*)g_at, (const float*)h_next, dst_of_next, dmask_next, 1.0f, 1.0f, (bf16*)out3, s3, out3_hi_only, (const float*)nullptr);
    else
        hipLaunchKernelGGL(ln_bwd_kernel<bf16>, dim3((rows + 3) / 4), dim3(256), 0, s, (const bf16*)dy, x, stats, w, base, dx,
                           rows, (bf16*)g_at, (const bf16*)h_next, dst_of_next, dmask_next, gs, 1.0f / gs, (bf16*)nullptr, 1.0f, 0, (const bf16*)base_at);
    LAUNCH_CHECK();
    return 0;
}

int launch_ln_stats(const float* x, float2* stats, int rows, hipStream_t s) {
    hipLaunchKernelGGL(ln_stats_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, x, stats, rows);
    LAUNCH_CHECK();
    return 0;
}
int launch_rows_add(const float* a, const float* b, float* out, int rows, hipStream_t s) {
    hipLaunchKernelGGL(rows_add_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, a, b, out, rows);
    LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------
// The adapter's own LayerNorm (tuning_config.ffn_adapter_layernorm_option "in" / "out"; reference models/dynamic_adapter.py:95-98,
// 121-122,132-133: nn.LayerNorm(768) with the default eps 1e-5, trainable, applied to the adapter's input or to its scaled output).
// Round 6: generic row kernels behind dyt_config::adapter_ln -- no shipped script uses the option, so nothing is fused.
//   adapter_ln_fwd:     out = LN(x) w + b (+ resid)   as OT (the 16-bit operand type: down-projection input; float: x_out = u + LN(up))
//   ln_param_grad:      per 32-row block:  partial[blk][0:768] = sum_t dy[t] xhat[t],  partial[blk][768:1536] = sum_t dy[t]   (x inv_gs)
//   ln_param_reduce:    out[i] += sum_blk partial[blk][i]   (fixed order)
// ------------------------------------------------------------------------------------------
constexpr float AD_LN_EPS = 1e-5f;
template <class OT>
__global__ __launch_bounds__(256) void adapter_ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                             OT* __restrict__ out, float2* __restrict__ stats, const float* __restrict__ resid, int rows) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    Row12 xr, wr, br, rr;
    xr.load(x + (size_t)row * D, lane);
    wr.load(w, lane);
    br.load(b, lane);
    if (resid) rr.load(resid + (size_t)row * D, lane);
    xr.landed(); wr.landed(); br.landed();
    if (resid) rr.landed();
    float mean = xr.sum() * (1.0f / D);
    // The mean is pinned in ONE register (as split2 pins its source, dyt_common.h).  Without that the 16-bit instance folds the product into
    // the subtraction for half of a lane's channels (v_fmac x + sum * -(1/768): the product unrounded) and not for the other half, so
    // those channels are centred on another mean than the one in `stats`: a constant row c came out as b - c 2^-25 rstd w, not as b
    asm("" : "+v"(mean));
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < 12; ++i) { const float d = xr.v[i] - mean; sq = fmaf(d, d, sq); }
    const float rstd = 1.0f / sqrtf(wave_sum(sq) * (1.0f / D) + AD_LN_EPS);
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        xr.v[i] = (xr.v[i] - mean) * rstd * wr.v[i] + br.v[i];
        if (resid) xr.v[i] += rr.v[i];
    }
    xr.store(out + (size_t)row * D, lane);
    if (stats && lane == 0) stats[row] = make_float2(mean, rstd);
}
int launch_adapter_ln_fwd(int out_at_precision, const float* x, const float* w, const float* b, void* out, float2* stats, const float* resid,
                          int rows, hipStream_t s) {
    const int grid = (rows + 3) / 4;
    if (out_at_precision == 0)
        hipLaunchKernelGGL(adapter_ln_fwd_kernel<float>, dim3(grid), dim3(256), 0, s, x, w, b, (float*)out, stats, resid, rows);
    else
        hipLaunchKernelGGL(adapter_ln_fwd_kernel<bf16>, dim3(grid), dim3(256), 0, s, x, w, b, (bf16*)out, stats, resid, rows);
    LAUNCH_CHECK();
    return 0;
}

constexpr int LNPG_ROWS = 32;   // rows per workgroup
template <class AT>
__global__ __launch_bounds__(256) void ln_param_grad_kernel(const AT* __restrict__ dy, const float* __restrict__ x, const float2* __restrict__ stats,
                                                            float* __restrict__ partial, int rows, float inv_gs) {
    __shared__ float red[4][2 * D];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    Row12 dg, db;
#pragma unroll
    for (int i = 0; i < 12; ++i) { dg.v[i] = 0.f; db.v[i] = 0.f; }
    const int r0 = blockIdx.x * LNPG_ROWS;
    for (int k = wave; k < LNPG_ROWS; k += 4) {
        const int r = r0 + k;
        if (r >= rows) break;
        Row12 g, xr;
        g.load_at(dy + (size_t)r * D, lane);
        xr.load(x + (size_t)r * D, lane);
        float2 st = stats[r];
        g.landed(); xr.landed();
        DYT_PIN2(st.x, st.y);
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            const float gv = g.v[i] * inv_gs;
            db.v[i] += gv;
            dg.v[i] = fmaf(gv, (xr.v[i] - st.x) * st.y, dg.v[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            red[wave][i * 256 + lane * 4 + e] = dg.v[4 * i + e];
            red[wave][D + i * 256 + lane * 4 + e] = db.v[4 * i + e];
        }
    __syncthreads();
    for (int c = tid; c < 2 * D; c += 256)
        partial[(size_t)blockIdx.x * (2 * D) + c] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
}
__global__ __launch_bounds__(256) void ln_param_reduce_kernel(const float* __restrict__ partial, int nparts, float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * D) return;
    float t = 0.f;
    for (int p = 0; p < nparts; ++p) t += partial[(size_t)p * (2 * D) + i];
    out[i] += t;
}
// dgamma -> out[0:768], dbeta -> out[768:1536] (+=); dy carries the 16-bit gradient factor gs when precision != 0
int launch_ln_param_grad(int precision, const void* dy, const float* x, const float2* stats, float* partial, float* out, int rows, float gs, hipStream_t s) {
    const int nblk = (rows + LNPG_ROWS - 1) / LNPG_ROWS;
    if (precision == 0)
        hipLaunchKernelGGL(ln_param_grad_kernel<float>, dim3(nblk), dim3(256), 0, s, (const float*)dy, x, stats, partial, rows, 1.0f);
    else
        hipLaunchKernelGGL(ln_param_grad_kernel<bf16>, dim3(nblk), dim3(256), 0, s, (const bf16*)dy, x, stats, partial, rows, 1.0f / gs);
    hipLaunchKernelGGL(ln_param_reduce_kernel, dim3((2 * D + 255) / 256), dim3(256), 0, s, partial, nblk, out);
    LAUNCH_CHECK();
    return 0;
}
int64_t ln_param_grad_scratch_floats(int rows) { return (int64_t)((rows + LNPG_ROWS - 1) / LNPG_ROWS) * 2 * D; }

// the folded LayerNorm form's weight side (GemmArgs::ln_part), one wave per output feature n, from the fp32 weight (one rounding, like the
// plain 16-bit copy): Wf[n,:] = AT(gamma * W[n,:]), cs[n] = sum of the ROUNDED Wf[n,:] (what the matrix cores contract), bf[n] = bias[n] + <W[n,:], beta>
template <class AT>
__global__ __launch_bounds__(256) void ln_fold_w_kernel(const float* __restrict__ W, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        const float* __restrict__ bias, AT* __restrict__ Wf, float* __restrict__ cs,
                                                        float* __restrict__ bf, int N) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    Row12 wr, gr, br;
    wr.load(W + (size_t)n * D, lane);
    gr.load(gamma, lane);
    br.load(beta, lane);
    float s = 0.f, t = 0.f;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        t = fmaf(wr.v[i], br.v[i], t);
        wr.v[i] = to_f32(from_f32<AT>(wr.v[i] * gr.v[i]));
        s += wr.v[i];
    }
    s = wave_sum(s);
    t = wave_sum(t);
    wr.store(Wf + (size_t)n * D, lane);
    if (lane == 0) { cs[n] = s; bf[n] = bias[n] + t; }
}
int launch_ln_fold_w(int precision, const float* W, const float* gamma, const float* beta, const float* bias, void* Wf, void* Wfp, float* cs,
                     float* bf, int N, hipStream_t s) {
    if (precision == 0) { set_error("ln_fold_w: 16-bit modes only"); return -1; }
    hipLaunchKernelGGL(ln_fold_w_kernel<bf16>, dim3((N + 3) / 4), dim3(256), 0, s, W, gamma, beta, bias, (bf16*)Wf, cs, bf, N);
    LAUNCH_CHECK();
    if (Wfp) return launch_preshuffle_w(Wf, Wfp, N, D, s);
    return 0;
}

}  // namespace dyt
