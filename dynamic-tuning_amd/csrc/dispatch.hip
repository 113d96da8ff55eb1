// The token dispatcher of the DyT hot path (gfx950): gate logits and selection with index compaction, the LN2 gather of the
// kept rows, and the cls-only forms of the last block.  One 64-lane wave owns one 768-channel token row.
//
// Reference ops replaced (paths relative to the reference root):
//   TokenSelect.forward / _gumbel_sigmoid       models/dynamic_adapter.py:25-77
//   nonzero + gather of model_speed_test        models/model_speed_test.py:297-304
#include "kernels.h"
#include "rowhelp.h"

namespace dyt {

// ------------------------------------------------------------------------------------------
// token dispatcher: logits, (Gumbel-)sigmoid, hard threshold, per-image index compaction in LDS
// ------------------------------------------------------------------------------------------
// (1) logits for every patch token: one wave per token, whole chip
__global__ __launch_bounds__(256) void gate_logits_kernel(const float* __restrict__ u, const float* __restrict__ w,
                                                          const float* __restrict__ bias, float* __restrict__ logit, int M) {
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= M) return;
    if (t % NT == 0) return;  // cls token is never gated
    Row12 wr, ur;
    wr.load(w, lane);
    ur.load(u + (size_t)t * D, lane);
    float bs = bias[0];
    wr.landed(); ur.landed(); DYT_PIN1(bs);
    const float l = dot12(ur, wr) + bs;
    if (lane == 0) logit[t] = l;
}
// (2) per image: (Gumbel-)sigmoid, hard threshold, ballot/popcount compaction of the kept-token list
__global__ __launch_bounds__(256) void gate_select_kernel(GateArgs a) {
    __shared__ int wave_cnt[4];
    const int b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    bool keep = false;
    const int n = tid;
    if (n < NT) {
        const size_t t = (size_t)b * NT + n;
        if (n == 0) {
            keep = true;
            a.maskf[t] = 1.0f;
            a.soft[t] = 1.0f;
        } else {
            const float l = a.soft[t];  // gate_logits_kernel parked the logit here
            float z = l;
            if (a.training) {
                if (a.g1) {
                    z = (l + a.g1[(size_t)b * NP + n - 1] - a.g2[(size_t)b * NP + n - 1]) / a.tau;
                } else {
                    Philox ph(a.seed_dev ? *a.seed_dev : a.seed, a.subseq, t);
                    const float u = ph.u01(0);
                    z = (l + (logf(u) - log1pf(-u))) / a.tau;  // Gumbel - Gumbel ~ Logistic(0,1)
                }
            }
            const float sft = sigmoidf(z);
            keep = a.force_first > 0 ? n < a.force_first : sft > a.threshold;
            a.soft[t] = sft;
            a.maskf[t] = keep ? 1.0f : 0.0f;
            if (a.out_select) a.out_select[(size_t)b * a.out_stride + n - 1] = keep ? 1.0f : 0.0f;
            if (a.out_logits) a.out_logits[(size_t)b * a.out_stride + n - 1] = l;
        }
    }
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) wave_cnt[wave] = __popcll(bal);
    __syncthreads();
    int off = 0;
    for (int w = 0; w < wave; ++w) off += wave_cnt[w];
    if (keep) a.keep_local[(size_t)b * NT + off + __popcll(bal & ((1ull << lane) - 1ull))] = n;
    if (tid == 0) a.counts[b] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

int launch_gate(const GateArgs& a, hipStream_t s) {
    const int M = a.batch * NT;
    hipLaunchKernelGGL(gate_logits_kernel, dim3((M + 3) / 4), dim3(256), 0, s, a.u, a.w, a.b, a.soft, M);
    hipLaunchKernelGGL(gate_select_kernel, dim3(a.batch), dim3(256), 0, s, a);
    LAUNCH_CHECK();
    return 0;
}

template <class AT>
__global__ __launch_bounds__(256) void ln_gather_kernel(const float* __restrict__ u, const float* __restrict__ w,
                                                        const float* __restrict__ bb, const int* __restrict__ keep_local,
                                                        const int* __restrict__ counts, int* __restrict__ total,
                                                        const float* __restrict__ maskf, AT* __restrict__ out,
                                                        float2* __restrict__ stats, int* __restrict__ row_src,
                                                        int* __restrict__ dst_of, int batch, bf16* __restrict__ out3, int f8,
                                                        int* __restrict__ drop_src) {
    const int lane = threadIdx.x & 63;
    const int slot = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (slot >= batch * NT) return;
    const int b = slot / NT, j = slot - b * NT;
    const int cnt = counts[b];
    // exclusive prefix of the per-image counts, recomputed by every wave (B <= 1024 ints: cheaper than a
    // separate single-thread scan kernel on the critical path); wave 0 also publishes the grand total
    int off = 0;
    {
        const int lim = slot == 0 ? batch : b;
        int part = 0;
        for (int i = lane; i < lim; i += 64) part += counts[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
        if (slot == 0) { if (lane == 0) { total[0] = part; if (drop_src) total[1] = batch * NT - part; } }
        else off = part;
    }
    // role 1: this wave owns TOKEN `slot`: a dropped token has no compact row
    if (maskf[slot] == 0.f) {
        if (lane == 0) dst_of[slot] = -1;
        if (drop_src) {   // ... and is entry (tokens before it - kept tokens before it) of the ascending list of dropped rows (gather_index_kernel's)
            int kept = 0;
            for (int i = lane; i < j; i += 64) kept += maskf[b * NT + i] != 0.f;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) kept += __shfl_xor(kept, o, 64);
            if (lane == 0) drop_src[slot - off - kept] = slot;
        }
    }
    // role 2: this wave owns COMPACT slot j of image b
    if (j >= cnt) return;
    const int src = b * NT + keep_local[(size_t)b * NT + j];
    const int dst = off + j;
    Row12 xr, wr, br;
    xr.load(u + (size_t)src * D, lane);
    wr.load(w, lane);
    br.load(bb, lane);
    xr.landed(); wr.landed(); br.landed();
    const float2 st = ln_stats(xr);
#pragma unroll
    for (int i = 0; i < 12; ++i) xr.v[i] = (xr.v[i] - st.x) * st.y * wr.v[i] + br.v[i];
    if (out3) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
            if (f8) store4_split_f8(out3 + (size_t)dst * SPLIT_A * D, D, i * 256 + lane * 4, xr.v[4 * i], xr.v[4 * i + 1], xr.v[4 * i + 2], xr.v[4 * i + 3]);
            else store4_split3(out3 + (size_t)dst * SPLIT_A * D + i * 256 + lane * 4, D, xr.v[4 * i], xr.v[4 * i + 1], xr.v[4 * i + 2], xr.v[4 * i + 3]);
    } else {
        xr.store(out + (size_t)dst * D, lane);
    }
    if (lane == 0) {
        stats[src] = st;
        row_src[dst] = src;
        dst_of[src] = dst;
    }
}

// token dispatcher index arrays without the gather (one thread per token): see ln_gather_kernel for the roles
__global__ __launch_bounds__(256) void gather_index_kernel(const int* __restrict__ keep_local, const int* __restrict__ counts,
                                                           int* __restrict__ total, const float* __restrict__ maskf,
                                                           int* __restrict__ row_src, int* __restrict__ dst_of, int batch,
                                                           int* __restrict__ drop_src) {
    __shared__ int off_s;
    __shared__ int wave_cnt[4];
    const int b = blockIdx.x, j = threadIdx.x;
    if (j < 64) {   // exclusive prefix of the per-image counts (block 0 also publishes the grand total)
        const int lim = b == 0 ? batch : b;
        int part = 0;
        for (int i = j; i < lim; i += 64) part += counts[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
        if (j == 0) {
            off_s = b == 0 ? 0 : part;
            if (b == 0) { total[0] = part; total[1] = batch * NT - part; }
        }
    }
    const int slot = b * NT + j;
    const bool dropped = j < NT && maskf[slot] == 0.f;
    const unsigned long long bal = __ballot(dropped);
    if ((j & 63) == 0) wave_cnt[j >> 6] = __popcll(bal);
    __syncthreads();
    if (j >= NT) return;
    if (dropped) {
        dst_of[slot] = -1;
        if (drop_src) {   // the dropped tokens, ascending: the row list of their up-projection launch (total[1] of them)
            int before = b * NT - off_s;   // dropped tokens of the images before this one
            for (int w = 0; w < (j >> 6); ++w) before += wave_cnt[w];
            drop_src[before + __popcll(bal & ((1ull << (j & 63)) - 1ull))] = slot;
        }
    }
    if (j < counts[b]) {
        const int src = b * NT + keep_local[(size_t)b * NT + j];
        row_src[off_s + j] = src;
        dst_of[src] = off_s + j;
    }
}
int launch_gather_index(const int* keep_local, const int* counts, int* total, const float* maskf, int* row_src, int* dst_of,
                        int batch, hipStream_t s, int* drop_src) {
    hipLaunchKernelGGL(gather_index_kernel, dim3(batch), dim3(256), 0, s, keep_local, counts, total, maskf, row_src, dst_of, batch, drop_src);
    LAUNCH_CHECK();
    return 0;
}

int launch_ln_gather(int precision, const float* u, const float* w, const float* b, const int* keep_local,
                     const int* counts, int* total, const float* maskf, void* out, float2* stats,
                     int* row_src, int* dst_of, int batch, hipStream_t s, void* out3, int out3_f8, int* drop_src) {
    const int grid = (batch * NT + 3) / 4;
    if (precision == 0)
        hipLaunchKernelGGL(ln_gather_kernel<float>, dim3(grid), dim3(256), 0, s, u, w, b, keep_local, counts, total,
                           maskf, (float*)out, stats, row_src, dst_of, batch, (bf16*)out3, out3_f8, drop_src);
    else
        hipLaunchKernelGGL(ln_gather_kernel<bf16>, dim3(grid), dim3(256), 0, s, u, w, b, keep_local, counts, total,
                           maskf, (bf16*)out, stats, row_src, dst_of, batch, (bf16*)nullptr, 0, drop_src);
    LAUNCH_CHECK();
    return 0;
}

template <class AT>
__global__ __launch_bounds__(256) void ln_cls_kernel(const float* __restrict__ u, const float* __restrict__ w,
                                                     const float* __restrict__ bb, AT* __restrict__ out,
                                                     float2* __restrict__ stats, AT* __restrict__ u_cls, int batch) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= batch) return;
    const size_t t = (size_t)b * NT;
    Row12 xr, wr, br;
    xr.load(u + t * D, lane);
    wr.load(w, lane);
    br.load(bb, lane);
    xr.landed(); wr.landed(); br.landed();
    if (u_cls) xr.store(u_cls + (size_t)b * D, lane);
    const float2 st = ln_stats(xr);
#pragma unroll
    for (int i = 0; i < 12; ++i) xr.v[i] = (xr.v[i] - st.x) * st.y * wr.v[i] + br.v[i];
    xr.store(out + (size_t)b * D, lane);
    if (lane == 0) stats[t] = st;
}
int launch_ln_cls(int precision, const float* u, const float* w, const float* b, void* out, float2* stats, void* u_cls,
                  int batch, hipStream_t s) {
    const int grid = (batch + 3) / 4;
    if (precision == 0)
        hipLaunchKernelGGL(ln_cls_kernel<float>, dim3(grid), dim3(256), 0, s, u, w, b, (float*)out, stats, (float*)u_cls, batch);
    else
        hipLaunchKernelGGL(ln_cls_kernel<bf16>, dim3(grid), dim3(256), 0, s, u, w, b, (bf16*)out, stats, (bf16*)u_cls, batch);
    LAUNCH_CHECK();
    return 0;
}
__global__ void cls_index_kernel(int* __restrict__ cls_rows, int batch) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < batch) cls_rows[b] = b * NT;
}
int launch_cls_index(int* cls_rows, int batch, hipStream_t s) {
    hipLaunchKernelGGL(cls_index_kernel, dim3((batch + 255) / 256), dim3(256), 0, s, cls_rows, batch);
    LAUNCH_CHECK();
    return 0;
}

}  // namespace dyt
