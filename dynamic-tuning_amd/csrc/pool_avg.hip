// Mean-pooled classification head (DYT_CREATE_AVG_POOL / DYT_CREATE_FC_NORM): the row kernels around the head's LayerNorm.
//
//   avg_pool_fwd_kernel        pooled [B,768] = mean over the 196 patch rows of x [B,197,768] (cls row excluded)
//                              (reference models/vision_transformer_IN21K.py:377  x[:, num_prefix_tokens:].mean(dim=1))
//   avg_pool_bwd_kernel        g [B,197,768]: cls row = 0, every patch row = dpooled[b] / 196 (autograd of the line above); the ONE
//                              write of the gradient stream (no zero fill in front of it)
//   fc_norm_param_grad_kernel  d_gamma[c] += sum_b dy[b][c] * xhat[b][c], d_beta[c] += sum_b dy[b][c]   (fc_norm, :378; trainable
//                              because the checkpoint has no fc_norm.*: main_image.py:250-256)
//
// All fp32, no atomics, one writer and one fixed summation order per output element: bit-reproducible like the rest of the step.
//
// Summation order of avg_pool_fwd (per output channel): the 196 patch rows are cut into 7 runs of 28 consecutive rows
// (t = 1 + 28 w ... 28 + 28 w for wave w); a run is one chain  ((x[t0] + x[t0+1]) + x[t0+2]) + ...  in ascending t; the seven run
// sums are added in ascending w,  ((r0 + r1) + r2) + ... + r6;  the result is divided by 196.  The 16-byte and the 4-byte load form
// add in the same order, so the pointer's alignment never changes a bit of the result.
#include "kernels.h"
#include "rowhelp.h"

namespace dyt {

namespace {
constexpr int AP_WAVES = 7;                  // runs per output channel
constexpr int AP_RUN = NP / AP_WAVES;        // 28 rows per run
constexpr int AP_CHUNK = 256;                // channels per workgroup: 64 lanes x 4
constexpr int AP_INFLIGHT = 7;               // row loads a wave issues before it adds them
static_assert(AP_WAVES * AP_RUN == NP && AP_RUN % AP_INFLIGHT == 0 && D % AP_CHUNK == 0, "avg_pool tiling");
}  // namespace

// grid (768 / 256, B), block 7 x 64: wave w owns rows 1 + 28 w ... 28 + 28 w, lane l the four channels c0 + 4 l ... c0 + 4 l + 3
template <bool V4>
__global__ __launch_bounds__(AP_WAVES * 64) void avg_pool_fwd_kernel(const float* __restrict__ x, float* __restrict__ pooled) {
    __shared__ float part[AP_WAVES][AP_CHUNK];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = blockIdx.x * AP_CHUNK + lane * 4;
    const float* p = x + ((size_t)b * NT + 1 + (size_t)wave * AP_RUN) * D + c;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int t = 0; t < AP_RUN; t += AP_INFLIGHT) {
        float v[AP_INFLIGHT][4];
#pragma unroll
        for (int u = 0; u < AP_INFLIGHT; ++u) {
            const float* q = p + (size_t)(t + u) * D;
            if (V4) {
                const f32x4 r = *reinterpret_cast<const f32x4*>(q);
                v[u][0] = r[0]; v[u][1] = r[1]; v[u][2] = r[2]; v[u][3] = r[3];
            } else {
                v[u][0] = q[0]; v[u][1] = q[1]; v[u][2] = q[2]; v[u][3] = q[3];
            }
        }
#pragma unroll
        for (int u = 0; u < AP_INFLIGHT; ++u) { a0 += v[u][0]; a1 += v[u][1]; a2 += v[u][2]; a3 += v[u][3]; }
    }
    part[wave][lane * 4] = a0; part[wave][lane * 4 + 1] = a1; part[wave][lane * 4 + 2] = a2; part[wave][lane * 4 + 3] = a3;
    __syncthreads();
    if (tid < AP_CHUNK) {
        float s = part[0][tid];
#pragma unroll
        for (int w = 1; w < AP_WAVES; ++w) s += part[w][tid];
        pooled[(size_t)b * D + blockIdx.x * AP_CHUNK + tid] = s / (float)NP;
    }
}

// grid (8, B), block 192: thread i holds channels 4 i ... 4 i + 3 of dpooled[b] / 196 and writes them to rows blockIdx.x, + 8, ...
template <bool V4>
__global__ __launch_bounds__(192) void avg_pool_bwd_kernel(const float* __restrict__ dpooled, float* __restrict__ g) {
    const int b = blockIdx.y, c = threadIdx.x * 4;
    const float* d = dpooled + (size_t)b * D + c;
    const f32x4 v = {d[0] / (float)NP, d[1] / (float)NP, d[2] / (float)NP, d[3] / (float)NP};
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    for (int t = blockIdx.x; t < NT; t += gridDim.x) {
        float* q = g + ((size_t)b * NT + t) * D + c;
        const f32x4 w = t == 0 ? z : v;
        if (V4) *reinterpret_cast<f32x4*>(q) = w;
        else { q[0] = w[0]; q[1] = w[1]; q[2] = w[2]; q[3] = w[3]; }
    }
}

// grid 3, block 256: one thread per channel, images in ascending order (8 rows of loads in flight; the chains keep the image order)
__global__ __launch_bounds__(256) void fc_norm_param_grad_kernel(const float* __restrict__ dy, const float* __restrict__ x, size_t x_stride,
                                                                 const float2* __restrict__ stats, float* __restrict__ d_gamma,
                                                                 float* __restrict__ d_beta, int batch) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    float sg = 0.f, sb = 0.f;
    int b = 0;
    for (; b + 8 <= batch; b += 8) {
        float dv[8], xv[8]; float2 st[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { dv[u] = dy[(size_t)(b + u) * D + c]; xv[u] = x[(size_t)(b + u) * x_stride + c]; st[u] = stats[b + u]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) { sg = fmaf(dv[u], (xv[u] - st[u].x) * st[u].y, sg); sb += dv[u]; }
    }
    for (; b < batch; ++b) {
        const float2 st = stats[b];
        const float d = dy[(size_t)b * D + c];
        sg = fmaf(d, (x[(size_t)b * x_stride + c] - st.x) * st.y, sg);
        sb += d;
    }
    if (d_gamma) d_gamma[c] += sg;
    if (d_beta) d_beta[c] += sb;
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int launch_avg_pool_fwd(const float* x, float* pooled, int batch, hipStream_t s) {
    if (!x || !pooled || batch < 1) { set_error("avg_pool_fwd: bad argument (batch %d)", batch); return -1; }
    const dim3 grid(D / AP_CHUNK, batch), block(AP_WAVES * 64);
    if (aligned16(x)) hipLaunchKernelGGL(avg_pool_fwd_kernel<true>, grid, block, 0, s, x, pooled);
    else hipLaunchKernelGGL(avg_pool_fwd_kernel<false>, grid, block, 0, s, x, pooled);
    LAUNCH_CHECK();
    return 0;
}

int launch_avg_pool_bwd(const float* dpooled, float* g, int batch, hipStream_t s) {
    if (!dpooled || !g || batch < 1) { set_error("avg_pool_bwd: bad argument (batch %d)", batch); return -1; }
    const dim3 grid(8, batch), block(192);
    if (aligned16(g)) hipLaunchKernelGGL(avg_pool_bwd_kernel<true>, grid, block, 0, s, dpooled, g);
    else hipLaunchKernelGGL(avg_pool_bwd_kernel<false>, grid, block, 0, s, dpooled, g);
    LAUNCH_CHECK();
    return 0;
}

int launch_fc_norm_param_grad(const float* dy, const float* x, size_t x_stride, const float2* stats, float* d_gamma, float* d_beta,
                              int batch, hipStream_t s) {
    if (!dy || !x || !stats || batch < 1) { set_error("fc_norm_param_grad: bad argument (batch %d)", batch); return -1; }
    if (!d_gamma && !d_beta) return 0;
    hipLaunchKernelGGL(fc_norm_param_grad_kernel, dim3(D / 256), dim3(256), 0, s, dy, x, x_stride, stats, d_gamma, d_beta, batch);
    LAUNCH_CHECK();
    return 0;
}

}  // namespace dyt
