// The kernels that finish a step (gfx950): classification head, step loss, AdamW (plain, guarded, per-segment), the device
// seed word and gradient clipping -- what tests/test_gpu_step_tail.py and tests/test_gpu_param_groups.py cover.
//
// Reference ops replaced (paths relative to the reference root):
//   head / cls pooling                          models/vision_transformer_IN21K.py:375-380
//   CE + KL + AdaLoss                           engine_finetune.py:52-63, models/losses.py:48-84
//   torch.optim.AdamW                           main_image.py:285
#include <algorithm>
#include "kernels.h"
#include "rowhelp.h"

namespace dyt {

// ------------------------------------------------------------------------------------------
// head: final LayerNorm on the cls rows + Linear(768, C)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void head_fwd_kernel(const float* __restrict__ x, const float* __restrict__ nw,
                                                       const float* __restrict__ nb, const float* __restrict__ hw,
                                                       const float* __restrict__ hb, float* __restrict__ cls_n,
                                                       float2* __restrict__ stats, float* __restrict__ logits, int C,
                                                       size_t x_stride) {
    __shared__ float row[D];
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
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
        const float y = (v[i] - mean) * rstd * nw[c] + nb[c];
        row[c] = y;
        cls_n[(size_t)b * D + c] = y;
    }
    if (tid == 0) stats[b] = make_float2(mean, rstd);
    __syncthreads();
    for (int c = wave; c < C; c += 4) {
        float acc = 0.f;
        const float* wp = hw + (size_t)c * D;
#pragma unroll
        for (int i = 0; i < 12; ++i) acc = fmaf(row[lane + 64 * i], wp[lane + 64 * i], acc);
        acc = wave_sum(acc);
        if (lane == 0) logits[(size_t)b * C + c] = acc + hb[c];
    }
}
int launch_head_fwd(const float* x, const float* nw, const float* nb, const float* hw, const float* hb, float* cls_n,
                    float2* stats, float* logits, int batch, int C, hipStream_t s, size_t x_stride) {
    hipLaunchKernelGGL(head_fwd_kernel, dim3(batch), dim3(256), 0, s, x, nw, nb, hw, hb, cls_n, stats, logits, C, x_stride);
    LAUNCH_CHECK();
    return 0;
}

__global__ __launch_bounds__(256) void head_bwd_dx_kernel(const float* __restrict__ dlogits, const float* __restrict__ x,
                                                          const float2* __restrict__ stats, const float* __restrict__ nw,
                                                          const float* __restrict__ hw, float* __restrict__ g, int C,
                                                          int g_stride, size_t x_stride, float* __restrict__ dy_out) {
    __shared__ float red[4];
    __shared__ float dl[1024];
    const int b = blockIdx.x, tid = threadIdx.x;
    for (int c = tid; c < C; c += 256) dl[c] = dlogits[(size_t)b * C + c];
    __syncthreads();
    const float2 st = stats[b];
    float dy[3], xh[3];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int ch = tid + 256 * i;
        float acc = 0.f;
#pragma unroll 8
        for (int c = 0; c < C; ++c) acc = fmaf(dl[c], hw[(size_t)c * D + ch], acc);
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
__global__ __launch_bounds__(256) void head_bwd_dw_kernel(const float* __restrict__ dlogits, const float* __restrict__ cls_n,
                                                          float* __restrict__ dW, float* __restrict__ db, int batch, int C) {
    // one class per workgroup; the batch loop is a latency chain (52 us at B=128 when every iteration waited for its own
    // loads), so the class's dlogits column goes to LDS first and the row loads of 8 images are issued together; the fmaf
    // chain per output keeps the image order
    __shared__ float dl[1024];
    const int c = blockIdx.x, tid = threadIdx.x;
    float acc[3] = {0.f, 0.f, 0.f};
    float sb = 0.f;
    for (int b0 = 0; b0 < batch; b0 += 1024) {
        const int nb = min(1024, batch - b0);
        __syncthreads();
        for (int b = tid; b < nb; b += 256) dl[b] = dlogits[(size_t)(b0 + b) * C + c];
        __syncthreads();
        int b = 0;
        for (; b + 8 <= nb; b += 8) {
            float v[8][3];
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int i = 0; i < 3; ++i) v[u][i] = cls_n[(size_t)(b0 + b + u) * D + tid + 256 * i];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float d = dl[b + u];
                sb += d;
#pragma unroll
                for (int i = 0; i < 3; ++i) acc[i] = fmaf(d, v[u][i], acc[i]);
            }
        }
        for (; b < nb; ++b) {
            const float d = dl[b];
            sb += d;
#pragma unroll
            for (int i = 0; i < 3; ++i) acc[i] = fmaf(d, cls_n[(size_t)(b0 + b) * D + tid + 256 * i], acc[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) if (dW) dW[(size_t)c * D + tid + 256 * i] += acc[i];   // (either may be null: dyt_pool_head)
    if (tid == 0 && db) db[c] += sb;
}
int launch_head_bwd(const float* dlogits, const float* x, const float* cls_n, const float2* stats, const float* nw,
                    const float* hw, float* g, float* dWh, float* dbh, int batch, int C, int compact, hipStream_t s,
                    size_t x_stride, float* dy_out) {
    if (C > 1024) { set_error("head_bwd: num_classes %d > 1024 unsupported", C); return -1; }
    if (!compact) DYT_HIP_CHECK(hipMemsetAsync(g, 0, (size_t)batch * NT * D * sizeof(float), s));
    hipLaunchKernelGGL(head_bwd_dx_kernel, dim3(batch), dim3(256), 0, s, dlogits, x, stats, nw, hw, g, C,
                       compact ? D : NT * D, x_stride, dy_out);
    if (dWh || dbh) hipLaunchKernelGGL(head_bwd_dw_kernel, dim3(C), dim3(256), 0, s, dlogits, cls_n, dWh, dbh, batch, C);
    LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------
// step loss (one workgroup; B x C is tiny)
// ------------------------------------------------------------------------------------------
// stage 1: one wave per image (4 per workgroup): log-softmax of both logit rows, their gradients, and the
// per-image CE / KL terms into part[b] = {ce_s, ce_t, kl}
__global__ __launch_bounds__(256) void loss_rows_kernel(LossArgs a, float* __restrict__ part) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int C = a.C, B = a.batch;
    if (b >= B) return;
    const float invB = 1.0f / B;
    const float* ls = a.logits_s + (size_t)b * C;
    const float* lt = a.logits_t + (size_t)b * C;
    float ms = -INFINITY, mt = -INFINITY;
    for (int c = lane; c < C; c += 64) { ms = fmaxf(ms, ls[c]); mt = fmaxf(mt, lt[c]); }
    ms = wave_max(ms); mt = wave_max(mt);
    float ss = 0.f, st = 0.f;
    for (int c = lane; c < C; c += 64) { ss += expf(ls[c] - ms); st += expf(lt[c] - mt); }
    // log p = (logit - max) - log(sum): the row maximum is never added to the O(1) log-sum, so a common shift of the logits (1e4, say)
    // does not round log p to an ulp of the shift
    const float lgs_s = logf(wave_sum(ss)), lgs_t = logf(wave_sum(st));
    if (a.soft) {   // class-probability targets (LossArgs::soft): same form with the one-hot row replaced by t
        const float* tg = a.soft + (size_t)b * C;
        float tsum = 0.f;
        for (int c = lane; c < C; c += 64) tsum += tg[c];
        tsum = wave_sum(tsum);
        float klb = 0.f, ces = 0.f, cet = 0.f;
        for (int c = lane; c < C; c += 64) {
            const float lps = (ls[c] - ms) - lgs_s, lpt = (lt[c] - mt) - lgs_t;
            const float ps = expf(lps), pt = expf(lpt), t = tg[c];
            klb += pt * (lpt - lps);
            ces -= t * lps; cet -= t * lpt;
            a.dlogits_s[(size_t)b * C + c] = ((ps * tsum - t) + (ps - pt)) * invB;
            a.dlogits_t[(size_t)b * C + c] = (pt * tsum - t) * invB;
        }
        klb = wave_sum(klb); ces = wave_sum(ces); cet = wave_sum(cet);
        if (lane == 0) { part[b * 4 + 0] = ces; part[b * 4 + 1] = cet; part[b * 4 + 2] = klb; }
        return;
    }
    const int y = (int)a.targets[b];
    float klb = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float lps = (ls[c] - ms) - lgs_s, lpt = (lt[c] - mt) - lgs_t;
        const float ps = expf(lps), pt = expf(lpt);
        klb += pt * (lpt - lps);
        const float oh = c == y ? 1.0f : 0.0f;
        a.dlogits_s[(size_t)b * C + c] = ((ps - oh) + (ps - pt)) * invB;
        a.dlogits_t[(size_t)b * C + c] = (pt - oh) * invB;
    }
    klb = wave_sum(klb);
    if (lane == 0) {
        part[b * 4 + 0] = -((ls[y] - ms) - lgs_s);
        part[b * 4 + 1] = -((lt[y] - mt) - lgs_t);
        part[b * 4 + 2] = klb;
    }
}
// stage 2: one workgroup reduces the per-image terms (fixed order) and the kept-token counts
__global__ __launch_bounds__(256) void loss_final_kernel(LossArgs a, const float* __restrict__ part) {
    __shared__ float red[4][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int B = a.batch;
    float ce_s = 0.f, ce_t = 0.f, kl = 0.f, kept = 0.f;
    for (int b = tid; b < B; b += 256) { ce_s += part[b * 4]; ce_t += part[b * 4 + 1]; kl += part[b * 4 + 2]; }
    const int Bc = a.count_batch > 0 ? a.count_batch : B;   // images the gate statistics span
    if (a.counts)
        for (int i = tid; i < a.depth * Bc; i += 256) kept += (float)(a.counts[i] - 1);
    ce_s = wave_sum(ce_s); ce_t = wave_sum(ce_t); kl = wave_sum(kl); kept = wave_sum(kept);
    if (lane == 0) { red[wave][0] = ce_s; red[wave][1] = ce_t; red[wave][2] = kl; red[wave][3] = kept; }
    __syncthreads();
    if (tid == 0) {
        const float invB = 1.0f / B;
        const float base = (red[0][0] + red[1][0] + red[2][0] + red[3][0]) * invB;
        const float teacher = (red[0][1] + red[1][1] + red[2][1] + red[3][1]) * invB;
        const float klv = (red[0][2] + red[1][2] + red[2][2] + red[3][2]) * invB;
        float tok = 0.f, mean = 0.f, keptv = 0.f;
        float d0 = 0.f, d1 = 0.f, d2 = 0.f;
        if (a.counts) {
            keptv = red[0][3] + red[1][3] + red[2][3] + red[3][3];
            const float N = (float)a.depth * Bc * NP;
            mean = keptv / N;
            const float diff = mean - a.target_ratio;
            tok = diff * diff;
            d0 = a.loss_ratio * 2.0f * diff / N;
            if (a.token_minimal_weight > 0.f) {
                tok += a.token_minimal_weight * ((N - keptv) * fmaxf(a.token_minimal, 0.f) + keptv * fmaxf(a.token_minimal - 1.0f, 0.f));
                // clamp(min=0)'s backward passes the gradient AT the bound too (autograd: x >= min), so token_minimal == 0 / == 1 count
                d1 = a.token_minimal >= 0.f ? -a.loss_ratio * a.token_minimal_weight : 0.f;
                d2 = a.token_minimal >= 1.f ? -a.loss_ratio * a.token_minimal_weight : 0.f;
            }
        }
        const float token_loss = a.loss_ratio * tok;
        a.out_losses[0] = base + token_loss + teacher + klv;
        a.out_losses[1] = base;
        a.out_losses[2] = token_loss;
        a.out_losses[3] = teacher;
        a.out_losses[4] = klv;
        a.out_losses[5] = mean;
        a.out_losses[6] = keptv;
        a.out_losses[7] = 0.f;
        a.dtok[0] = d0; a.dtok[1] = d1; a.dtok[2] = d2;
    }
}
int launch_loss(const LossArgs& a, hipStream_t s) {
    if (!a.scratch) { set_error("loss: scratch missing"); return -1; }
    hipLaunchKernelGGL(loss_rows_kernel, dim3((a.batch + 3) / 4), dim3(256), 0, s, a, a.scratch);
    hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(256), 0, s, a, a.scratch);
    LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------
// AdamW over the flat trainable buffer
// ------------------------------------------------------------------------------------------
// The per-element update: ONE expression for adamw_kernel, adamw_guarded_kernel and adamw_segments_kernel, so that the compiler contracts
// it (fma) the same way in all three and their results agree bit for bit.  bc1 / rsqrt_bc2: the bias corrections, formed in double and
// rounded to float once by the caller.
__device__ __forceinline__ void adamw_update(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                             float* __restrict__ v, int64_t i, float lr, float b1, float b2, float eps, float wd,
                                             float bc1, float rsqrt_bc2, float gscale) {
    const float gi = g[i] * gscale;
    float pi = p[i] * (1.0f - lr * wd);
    const float mi = b1 * m[i] + (1.0f - b1) * gi;
    const float vi = b2 * v[i] + (1.0f - b2) * gi * gi;
    const float denom = sqrtf(vi) * rsqrt_bc2 + eps;
    pi -= (lr / bc1) * (mi / denom);
    p[i] = pi; m[i] = mi; v[i] = vi;
}
__global__ void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                             float* __restrict__ v, int64_t n, float lr, float b1, float b2, float eps, float wd,
                             float bc1, float rsqrt_bc2, float gscale) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    adamw_update(p, g, m, v, i, lr, b1, b2, eps, wd, bc1, rsqrt_bc2, gscale);
}
// ---- overflow-guarded update (the reference's GradScaler.step / update, misc.py:256-272: an update whose gradient holds inf / NaN is
// ---- skipped and counted; everything stays on the device: state = {updates applied, updates skipped, non-finite flag of this call, -}
__global__ __launch_bounds__(256) void grad_nonfinite_kernel(const float* __restrict__ g, int64_t n, int* __restrict__ state) {
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float v = g[i];
        bad |= !(fabsf(v) <= 3.0e38f);   // inf and NaN
    }
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(state + 2, 1);
}
__global__ __launch_bounds__(256) void adamw_guarded_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                     float* __restrict__ v, int64_t n, float lr, float b1, float b2, float eps, float wd,
                                     float gscale, const int* __restrict__ state) {
    // bias corrections in double, once per workgroup, rounded to fp32 exactly as dyt_adamw's host code hands them to adamw_kernel
    // (1 - powf(0.999f, step) in fp32 is up to 7e-6 relative off in the first steps: the whole update of a zero-initialised parameter)
    __shared__ float bc_s[2];
    if (threadIdx.x == 0) {
        const double step = (double)(state[0] + 1);
        bc_s[0] = (float)(1.0 - pow((double)b1, step));
        bc_s[1] = (float)(1.0 / sqrt(1.0 - pow((double)b2, step)));
    }
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || state[2] != 0) return;   // non-finite gradient somewhere: parameters and moments stay as they are
    adamw_update(p, g, m, v, i, lr, b1, b2, eps, wd, bc_s[0], bc_s[1], gscale);
}
// ---- parameter groups: the same update with lr and weight_decay taken per SEGMENT of the flat buffer (torch.optim.AdamW with several
// ---- param_groups; util/lr_decay.py makes ~26).  The table travels by value in the kernel arguments, so it is captured at launch and the
// ---- caller may rewrite its own copy at once.  Lookup without any per-thread indexing of the argument (that would be copied to scratch):
// ---- a workgroup owns elements [base, base + 256); it binary-searches the first segment that ends past `base` with a workgroup-uniform
// ---- index (scalar loads), then walks the segments that begin inside its range, again uniformly, and every thread keeps the
// ---- hyper-parameters of the last segment that begins at or before its element.  state == null: bc1 / rsqrt_bc2 come from the host
// ---- (adamw_kernel's form); else adamw_guarded_kernel's form.  (The search's ~log2(segments) dependent scalar loads stand in front of the
// ---- element's loads: +9 % kernel time at 26 segments over 18 M elements, none with one segment -- DESIGN.md 7k, also on why the loads
// ---- are not hoisted above it.)
__global__ __launch_bounds__(256) void adamw_segments_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                      float* __restrict__ v, int64_t n, const AdamwSegTable T, int nseg, float b1, float b2, float eps,
                                      float bc1_host, float rsqrt_bc2_host, float gscale, const int* __restrict__ state) {
    __shared__ float bc_s[2];
    if (threadIdx.x == 0) {
        if (state) {   // bias corrections in double, rounded to fp32 once: adamw_guarded_kernel's lines
            const double step = (double)(state[0] + 1);
            bc_s[0] = (float)(1.0 - pow((double)b1, step));
            bc_s[1] = (float)(1.0 / sqrt(1.0 - pow((double)b2, step)));
        } else {
            bc_s[0] = bc1_host;
            bc_s[1] = rsqrt_bc2_host;
        }
    }
    const int64_t base = (int64_t)blockIdx.x * 256;
    int lo = 0, hi = nseg - 1;   // the last segment ends at n > base: the answer exists
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (T.s[mid].end > base) hi = mid; else lo = mid + 1;
    }
    const int64_t i = base + threadIdx.x;
    float lr = T.s[lo].lr, wd = T.s[lo].wd;
    for (int s = lo + 1; s < nseg; ++s) {
        const int64_t begin = T.s[s - 1].end;
        if (begin >= base + 256) break;
        if (i >= begin) { lr = T.s[s].lr; wd = T.s[s].wd; }
    }
    __syncthreads();
    if (i >= n || (state && state[2] != 0)) return;   // non-finite gradient somewhere: every segment stays as it is
    adamw_update(p, g, m, v, i, lr, b1, b2, eps, wd, bc_s[0], bc_s[1], gscale);
}
__global__ void adamw_count_kernel(int* __restrict__ state) {
    if (threadIdx.x == 0) { if (state[2]) state[1] += 1; else state[0] += 1; }
}
int launch_adamw_guarded(float* p, const float* g, float* m, float* v, int64_t n, int* state, float lr, float b1, float b2, float eps,
                         float wd, float gscale, hipStream_t s) {
    if (hipMemsetAsync(state + 2, 0, sizeof(int), s) != hipSuccess) { set_error("hipMemsetAsync failed"); return -2; }
    hipLaunchKernelGGL(grad_nonfinite_kernel, dim3((unsigned)std::min<int64_t>(256, (n + 255) / 256)), dim3(256), 0, s, g, n, state);
    hipLaunchKernelGGL(adamw_guarded_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p, g, m, v, n, lr, b1, b2, eps, wd, gscale, state);
    hipLaunchKernelGGL(adamw_count_kernel, dim3(1), dim3(64), 0, s, state);
    LAUNCH_CHECK();
    return 0;
}
int launch_adamw_segments(float* p, const float* g, float* m, float* v, int64_t n, int* state, const AdamwSegTable& table, int nseg,
                          float b1, float b2, float eps, float bc1, float rsqrt_bc2, float gscale, hipStream_t s) {
    const dim3 grid((unsigned)((n + 255) / 256));
    if (state) {
        if (hipMemsetAsync(state + 2, 0, sizeof(int), s) != hipSuccess) { set_error("hipMemsetAsync failed"); return -2; }
        hipLaunchKernelGGL(grad_nonfinite_kernel, dim3((unsigned)std::min<int64_t>(256, (n + 255) / 256)), dim3(256), 0, s, g, n, state);
    }
    hipLaunchKernelGGL(adamw_segments_kernel, grid, dim3(256), 0, s, p, g, m, v, n, table, nseg, b1, b2, eps, bc1, rsqrt_bc2, gscale,
                       (const int*)state);
    if (state) hipLaunchKernelGGL(adamw_count_kernel, dim3(1), dim3(64), 0, s, state);
    LAUNCH_CHECK();
    return 0;
}
__global__ void seed_set_kernel(uint64_t* seed_dev, uint64_t value, int advance) {
    if (threadIdx.x == 0) seed_dev[0] = advance ? seed_dev[0] + 1 : value;
}
int launch_seed_set(uint64_t* seed_dev, uint64_t value, hipStream_t s) {
    hipLaunchKernelGGL(seed_set_kernel, dim3(1), dim3(64), 0, s, seed_dev, value, 0);
    LAUNCH_CHECK();
    return 0;
}
int launch_seed_advance(uint64_t* seed_dev, hipStream_t s) {
    hipLaunchKernelGGL(seed_set_kernel, dim3(1), dim3(64), 0, s, seed_dev, 0ull, 1);
    LAUNCH_CHECK();
    return 0;
}

// ---- global-norm clipping of the flat gradient (engine_finetune.py:74 -> misc.py:262-266 clip_grad_norm_) ----
__global__ __launch_bounds__(256) void sqsum_kernel(const float* __restrict__ g, int64_t n, float* __restrict__ part) {
    __shared__ float ws[4];
    float acc = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) acc = fmaf(g[i], g[i], acc);
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}
__global__ __launch_bounds__(256) void clip_scale_kernel(float* __restrict__ g, int64_t n, const float* __restrict__ part, int nparts,
                                                         float max_norm, float pre_scale, float* __restrict__ norm_out) {
    __shared__ float coef_s;
    if (threadIdx.x < 64) {   // every block re-derives the (deterministic, fixed-order) total: no second launch, no atomics
        float acc = 0.f;
        for (int i = threadIdx.x; i < nparts; i += 64) acc += part[i];
        acc = wave_sum(acc);
        if (threadIdx.x == 0) {
            const float norm = sqrtf(acc) * fabsf(pre_scale);
            coef_s = fminf(1.0f, max_norm / (norm + 1e-6f));
            if (blockIdx.x == 0 && norm_out) norm_out[0] = norm;
        }
    }
    __syncthreads();
    const float coef = coef_s;
    if (coef >= 1.0f) return;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) g[i] *= coef;
}
int launch_clip_grad_norm(float* g, int64_t n, float max_norm, float pre_scale, float* scratch, float* norm_out, hipStream_t s) {
    const int nparts = 256;
    hipLaunchKernelGGL(sqsum_kernel, dim3(nparts), dim3(256), 0, s, g, n, scratch);
    hipLaunchKernelGGL(clip_scale_kernel, dim3(nparts), dim3(256), 0, s, g, n, scratch, nparts, max_norm, pre_scale, norm_out);
    LAUNCH_CHECK();
    return 0;
}

int launch_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2, float eps,
                 float wd, float bc1, float rsqrt_bc2, float gscale, hipStream_t s) {
    hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p, g, m, v, n, lr, b1, b2, eps,
                       wd, bc1, rsqrt_bc2, gscale);
    LAUNCH_CHECK();
    return 0;
}

}  // namespace dyt
