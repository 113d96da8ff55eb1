// Model EMA over the flat trainable buffer, one context-free entry (dyt_ema_update):
//
//   ema[i] = fl( fl(decay * ema[i]) + fl(one_minus_decay * param[i]) ),  in place
//
// which is `ema_v.copy_(decay * ema_v + (1. - decay) * model_v)` of timm's ModelEmaV2 as torch evaluates it on fp32 tensors: three fp32
// roundings, no fused multiply-add.  The expression is mix.h's mix_value (contraction switched off by its pragma), so the Mixup blend and
// this update cannot drift apart.  Nothing flushes denormals (the Makefile sets no such flag): they pass through like any other value.
//
// One launch, no atomics, no context.  The range is cut on the host into a scalar head (up to three elements, until `ema` reaches a
// 16-byte boundary), a body of 16-byte accesses, and a scalar tail; where `param` is not 16-byte aligned at the point where `ema` is,
// the body is empty and every element goes the scalar way.  An element sees the same three operations on either path: the same bits.
// Pure fp32: the bf16 and the fp16 build of the library hold the same code.
#include <cmath>
#include <cstdint>

#include "../../include/dyt_hip.h"
#include "dyt_common.h"
#include "mix.h"

namespace dyt {

namespace {

constexpr int EMA_BLOCK = 256;
constexpr int64_t EMA_MAX_GRID = 1 << 20;   // more work than this many workgroups hold is walked by a grid-stride loop

// items [0, nvec): float4 number `item` of the body, elements head + 4 item ... + 3; items [nvec, nvec + nscalar): scalar element
// s = item - nvec, which lies in the head for s < head and behind the body otherwise
__global__ void __launch_bounds__(EMA_BLOCK) ema_update_kernel(float* __restrict__ ema, const float* __restrict__ param, int64_t head,
                                                                int64_t nvec, int64_t nscalar, float decay, float omd) {
    const int64_t stride = (int64_t)gridDim.x * EMA_BLOCK;
    for (int64_t item = (int64_t)blockIdx.x * EMA_BLOCK + threadIdx.x; item < nvec + nscalar; item += stride) {
        if (item < nvec) {
            float4* e4 = reinterpret_cast<float4*>(ema + head) + item;
            const float4 p = reinterpret_cast<const float4*>(param + head)[item];
            float4 e = *e4;
            e.x = mix_value(e.x, p.x, decay, omd);
            e.y = mix_value(e.y, p.y, decay, omd);
            e.z = mix_value(e.z, p.z, decay, omd);
            e.w = mix_value(e.w, p.w, decay, omd);
            *e4 = e;
        } else {
            const int64_t s = item - nvec;
            const int64_t i = s < head ? s : s + 4 * nvec;
            ema[i] = mix_value(ema[i], param[i], decay, omd);
        }
    }
}

inline bool unit_interval(float v) { return std::isfinite(v) && v >= 0.0f && v <= 1.0f; }

}  // namespace

}  // namespace dyt

using namespace dyt;

extern "C" int dyt_ema_update(float* ema, const float* param, int64_t numel, float decay, float one_minus_decay, void* stream) {
    if (numel < 0) { set_error("dyt_ema_update: numel %lld < 0", (long long)numel); return DYT_ERR_ARG; }
    if (!unit_interval(decay) || !unit_interval(one_minus_decay)) {
        set_error("dyt_ema_update: decay %g / one_minus_decay %g: both are finite values in [0, 1]", (double)decay, (double)one_minus_decay);
        return DYT_ERR_ARG;
    }
    if (numel == 0) return DYT_OK;
    if (!ema || !param) { set_error("dyt_ema_update: null %s with numel %lld", !ema ? "ema" : "param", (long long)numel); return DYT_ERR_ARG; }
    const uintptr_t ea = reinterpret_cast<uintptr_t>(ema), pa = reinterpret_cast<uintptr_t>(param);
    if ((ea | pa) & 3) { set_error("dyt_ema_update: ema / param are not aligned to 4 bytes"); return DYT_ERR_ARG; }
    int64_t head = (int64_t)(((16 - (ea & 15)) & 15) >> 2);   // elements in front of ema's next 16-byte boundary
    int64_t nvec = 0;
    if (head > numel) head = numel;
    if (((pa + 4 * (uintptr_t)head) & 15) == 0) nvec = (numel - head) / 4;
    if (nvec == 0) head = 0;   // all scalar: element s of the scalar items is element s
    const int64_t items = nvec + (numel - 4 * nvec);
    const int64_t grid = std::min<int64_t>((items + EMA_BLOCK - 1) / EMA_BLOCK, EMA_MAX_GRID);
    hipLaunchKernelGGL(ema_update_kernel, dim3((unsigned)grid), dim3(EMA_BLOCK), 0, static_cast<hipStream_t>(stream), ema, param, head, nvec,
                       numel - 4 * nvec, decay, one_minus_decay);
    DYT_HIP_CHECK(hipGetLastError());
    return DYT_OK;
}
