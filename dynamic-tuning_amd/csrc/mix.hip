// On-device Mixup / CutMix, fused into the patch-embedding load (dyt_set_mix) and as two context-free entries (dyt_mix_images,
// dyt_mix_targets).  The scalar formula, the pairing, the source predicate and every argument check are mix.h.  The run-level helpers
// (mix_run, unpack, lookup) are mix_dev.h, shared with erase.hip.
//
//   im2col_mix_kernel<AT>            fp32 [B,3,224,224] -> the EPI_EMBED GEMM's A operand: im2col_kernel's work items (4 pixels of one image
//                                    row, one 16-byte load) and element order
//   im2col_mix_u8_kernel<AT, NHWC>   bytes -> the same operand: im2col_u8_kernel's work items (16 pixels of one image row) and its 3 x 256
//                                    LDS table; the values mixed are the normalised ones
//   mix_images_kernel<KIND>          either input -> fp32 [B,3,224,224] (the analogue of normalize_u8_kernel)
//   mix_targets_kernel<VEC>          int64 labels -> fp32 [rows, C] class-probability rows
//
// Every kernel reads its MixParams block from DEVICE memory (one 64-byte load per thread, the same address for all: it stays in the
// cache), so the mode -- identity, mixup, cutmix -- is a run-time value and a captured step replays with whatever the block holds by then.
// The partner's run is loaded only when the mode needs it: always for mixup, for cutmix only when the run's row lies in [yl, yh) and its
// columns meet [xl, xh), never for identity (whose output is a copy of the own pixels: -0.0, NaN and inf pass, nothing of the partner
// leaks in).  Nothing read from the block is used as an index: a block with any content cannot make a kernel leave its buffers.  One
// writer per output element, no atomics.
#include "mix_dev.h"

namespace dyt {

#define LAUNCH_CHECK() DYT_HIP_CHECK(hipGetLastError())

template <class AT>
__global__ __launch_bounds__(256) void im2col_mix_kernel(const float* __restrict__ img, AT* __restrict__ out, int batch, int frames,
                                                         const MixParams* __restrict__ params) {
    // out[(b*196 + py*14 + px)*768 + c*256 + i*16 + j]: im2col_kernel's work item, 4 consecutive j per thread
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t total = (size_t)batch * NP * (D / 4);
    if (idx >= total) return;
    const MixParams p = *params;
    const int k4 = (int)(idx % (D / 4));
    const size_t row = idx / (D / 4);
    const int pt = (int)(row % NP);
    const int b = (int)(row / NP);
    const int k = k4 * 4, c = k >> 8, i = (k >> 4) & 15, j = k & 15;
    const int py = pt / GRID_P, px = pt - py * GRID_P;
    const int y = py * PS + i, x0 = px * PS + j;
    const size_t at = ((size_t)c * IMG + y) * IMG + x0;
    float v[4];
    unpack(v, *reinterpret_cast<const float4*>(img + (size_t)b * 3 * PLANE + at));
    if (mix_run_needs_partner(p, y, x0, 4)) {
        float w[4];
        unpack(w, *reinterpret_cast<const float4*>(img + (size_t)mix_partner(b, batch, frames) * 3 * PLANE + at));
        mix_run(v, w, p, y, x0);
    }
    store4(out + row * D + k, v[0], v[1], v[2], v[3]);
}

template <class AT, bool NHWC>
__global__ __launch_bounds__(256) void im2col_mix_u8_kernel(const uint8_t* __restrict__ img, AT* __restrict__ out, int batch, int frames,
                                                            InputNorm nm, const MixParams* __restrict__ params) {
    __shared__ float tab[3 * 256];
    build_table(tab, nm);
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t total = (size_t)batch * NP * PS * (NHWC ? 1 : 3);
    if (idx >= total) return;
    const MixParams p = *params;
    if (NHWC) {
        // work item = (b, patch, i): 48 contiguous bytes = 16 pixels x 3 channels -> three 16-element runs of the operand row
        const int i = (int)(idx % PS);
        const size_t row = idx / PS;                       // b * 196 + patch
        const int pt = (int)(row % NP);
        const int b = (int)(row / NP);
        const int py = pt / GRID_P, px = pt - py * GRID_P;
        const int y = py * PS + i, x0 = px * PS;
        const size_t at = ((size_t)y * IMG + x0) * 3;
        const uint4* src = reinterpret_cast<const uint4*>(img + (size_t)b * 3 * PLANE + at);
        const uint4 w[3] = {src[0], src[1], src[2]};
        const bool need = mix_run_needs_partner(p, y, x0, 16);
        uint4 q[3] = {w[0], w[1], w[2]};
        if (need) {
            const uint4* ps = reinterpret_cast<const uint4*>(img + (size_t)mix_partner(b, batch, frames) * 3 * PLANE + at);
            q[0] = ps[0]; q[1] = ps[1]; q[2] = ps[2];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v[16];
            lookup(v, tab, w, c);
            if (need) {
                float u[16];
                lookup(u, tab, q, c);
                mix_run(v, u, p, y, x0);
            }
            store16(out + row * D + c * 256 + i * PS, v);
        }
    } else {
        // work item = (b, patch, c, i) = 16-element group idx of the operand: out + idx * 16
        const int i = (int)(idx % PS);
        const int c = (int)((idx / PS) % 3);
        const size_t row = idx / (3 * PS);
        const int pt = (int)(row % NP);
        const int b = (int)(row / NP);
        const int py = pt / GRID_P, px = pt - py * GRID_P;
        const int y = py * PS + i, x0 = px * PS;
        const size_t at = ((size_t)c * IMG + y) * IMG + x0;
        float v[16];
        lookup(v, tab, *reinterpret_cast<const uint4*>(img + (size_t)b * 3 * PLANE + at), c);
        if (mix_run_needs_partner(p, y, x0, 16)) {
            float u[16];
            lookup(u, tab, *reinterpret_cast<const uint4*>(img + (size_t)mix_partner(b, batch, frames) * 3 * PLANE + at), c);
            mix_run(v, u, p, y, x0);
        }
        store16(out + idx * 16, v);
    }
}

// KIND 0: fp32 NCHW, 4 pixels per thread; 1: uint8 NCHW, 16 pixels per thread; 2: uint8 NHWC, 16 pixels x 3 channels per thread.  A row of
// 224 pixels is a whole number of either run, so a run never crosses a row.
template <int KIND>
__global__ __launch_bounds__(256) void mix_images_kernel(const void* __restrict__ src_, float* __restrict__ dst, int batch, int frames,
                                                         InputNorm nm, const MixParams* __restrict__ params) {
    __shared__ float tab[KIND == 0 ? 1 : 3 * 256];
    if (KIND != 0) build_table(tab, nm);
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (KIND == 0) {
        const float* src = static_cast<const float*>(src_);
        const size_t total = (size_t)batch * 3 * PLANE / 4;
        if (idx >= total) return;
        const MixParams p = *params;
        const int b = (int)(idx / (3 * PLANE / 4));
        const size_t at = (idx - (size_t)b * (3 * PLANE / 4)) * 4;       // element within the image
        const int pix = (int)(at % PLANE), y = pix / IMG, x0 = pix - y * IMG;
        float v[4];
        unpack(v, *reinterpret_cast<const float4*>(src + (size_t)b * 3 * PLANE + at));
        if (mix_run_needs_partner(p, y, x0, 4)) {
            float w[4];
            unpack(w, *reinterpret_cast<const float4*>(src + (size_t)mix_partner(b, batch, frames) * 3 * PLANE + at));
            mix_run(v, w, p, y, x0);
        }
        store4(dst + idx * 4, v[0], v[1], v[2], v[3]);
    } else if (KIND == 1) {
        const uint8_t* src = static_cast<const uint8_t*>(src_);
        const size_t total = (size_t)batch * 3 * PLANE / 16;
        if (idx >= total) return;
        const MixParams p = *params;
        const int b = (int)(idx / (3 * PLANE / 16));
        const size_t at = (idx - (size_t)b * (3 * PLANE / 16)) * 16;
        const int c = (int)(at / PLANE), pix = (int)(at - (size_t)c * PLANE), y = pix / IMG, x0 = pix - y * IMG;
        float v[16];
        lookup(v, tab, *reinterpret_cast<const uint4*>(src + (size_t)b * 3 * PLANE + at), c);
        if (mix_run_needs_partner(p, y, x0, 16)) {
            float u[16];
            lookup(u, tab, *reinterpret_cast<const uint4*>(src + (size_t)mix_partner(b, batch, frames) * 3 * PLANE + at), c);
            mix_run(v, u, p, y, x0);
        }
        store16(dst + idx * 16, v);
    } else {
        const uint8_t* src = static_cast<const uint8_t*>(src_);
        const size_t total = (size_t)batch * PLANE / 16;
        if (idx >= total) return;
        const MixParams p = *params;
        const int b = (int)(idx / (PLANE / 16));
        const int q16 = (int)(idx - (size_t)b * (PLANE / 16));            // 16-pixel group within the image
        const int pix = q16 * 16, y = pix / IMG, x0 = pix - y * IMG;
        const uint4* s4 = reinterpret_cast<const uint4*>(src + (size_t)b * 3 * PLANE + (size_t)pix * 3);
        const uint4 w[3] = {s4[0], s4[1], s4[2]};
        const bool need = mix_run_needs_partner(p, y, x0, 16);
        uint4 q[3] = {w[0], w[1], w[2]};
        if (need) {
            const uint4* ps = reinterpret_cast<const uint4*>(src + (size_t)mix_partner(b, batch, frames) * 3 * PLANE + (size_t)pix * 3);
            q[0] = ps[0]; q[1] = ps[1]; q[2] = ps[2];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v[16];
            lookup(v, tab, w, c);
            if (need) {
                float u[16];
                lookup(u, tab, q, c);
                mix_run(v, u, p, y, x0);
            }
            store16(dst + ((size_t)b * 3 + c) * PLANE + pix, v);
        }
    }
}

// out[row][c] = mix_value(t(y_row)[c], t(y_partner)[c]) (+ the criterion's smoothing); 4 classes per thread.  VEC: C % 4 == 0, so every
// group of 4 is 16-byte aligned in the [rows, C] buffer and is stored at once; else the row stride is odd and the stores are scalar.
template <bool VEC>
__global__ __launch_bounds__(256) void mix_targets_kernel(const int64_t* __restrict__ labels, float* __restrict__ out, int rows, int C,
                                                          const MixParams* __restrict__ params) {
    const int groups = (C + 3) / 4;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)rows * groups) return;
    const MixParams p = *params;
    const int row = (int)(idx / groups), c0 = (int)(idx - (size_t)row * groups) * 4;
    const int64_t ya = labels[row], yb = labels[mix_partner(row, rows, 1)];
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = c0 + j;
        const float t = mix_value(c == ya ? p.on : p.off, c == yb ? p.on : p.off, p.lam_f, p.oml_f);
        v[j] = p.smooth_on ? mix_smooth(t, p.sm_keep, p.sm_add) : t;
    }
    float* dst = out + (size_t)row * C + c0;
    if (VEC) {
        store4(dst, v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (c0 + j < C) dst[j] = v[j];
    }
}

int launch_im2col_mix(int precision, const float* images, void* out, int batch, int frames, const MixParams* params, hipStream_t s) {
    const size_t total = (size_t)batch * NP * (D / 4);
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    if (precision == 0) hipLaunchKernelGGL(im2col_mix_kernel<float>, grid, block, 0, s, images, (float*)out, batch, frames, params);
    else hipLaunchKernelGGL(im2col_mix_kernel<bf16>, grid, block, 0, s, images, (bf16*)out, batch, frames, params);
    LAUNCH_CHECK();
    return 0;
}

int launch_im2col_mix_u8(int precision, const uint8_t* images, int nhwc, const InputNorm& nm, void* out, int batch, int frames,
                         const MixParams* params, hipStream_t s) {
    const size_t total = (size_t)batch * NP * PS * (nhwc ? 1 : 3);
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    if (precision == 0) {
        if (nhwc) hipLaunchKernelGGL((im2col_mix_u8_kernel<float, true>), grid, block, 0, s, images, (float*)out, batch, frames, nm, params);
        else hipLaunchKernelGGL((im2col_mix_u8_kernel<float, false>), grid, block, 0, s, images, (float*)out, batch, frames, nm, params);
    } else {
        if (nhwc) hipLaunchKernelGGL((im2col_mix_u8_kernel<bf16, true>), grid, block, 0, s, images, (bf16*)out, batch, frames, nm, params);
        else hipLaunchKernelGGL((im2col_mix_u8_kernel<bf16, false>), grid, block, 0, s, images, (bf16*)out, batch, frames, nm, params);
    }
    LAUNCH_CHECK();
    return 0;
}

int launch_mix_images(const void* src, float* dst, int count, int frames, int src_kind, const InputNorm& nm, const MixParams* params,
                      hipStream_t s) {
    const size_t total = src_kind == 0 ? (size_t)count * 3 * PLANE / 4 : (src_kind == 1 ? (size_t)count * 3 * PLANE / 16 : (size_t)count * PLANE / 16);
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    if (src_kind == 0) hipLaunchKernelGGL(mix_images_kernel<0>, grid, block, 0, s, src, dst, count, frames, nm, params);
    else if (src_kind == 1) hipLaunchKernelGGL(mix_images_kernel<1>, grid, block, 0, s, src, dst, count, frames, nm, params);
    else hipLaunchKernelGGL(mix_images_kernel<2>, grid, block, 0, s, src, dst, count, frames, nm, params);
    LAUNCH_CHECK();
    return 0;
}

int launch_mix_targets(const int64_t* labels, float* out, int rows, int num_classes, const MixParams* params, hipStream_t s) {
    const size_t total = (size_t)rows * ((num_classes + 3) / 4);
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    if (num_classes % 4 == 0) hipLaunchKernelGGL(mix_targets_kernel<true>, grid, block, 0, s, labels, out, rows, num_classes, params);
    else hipLaunchKernelGGL(mix_targets_kernel<false>, grid, block, 0, s, labels, out, rows, num_classes, params);
    LAUNCH_CHECK();
    return 0;
}

// the check of a pass that runs while mix is on (dyt_forward, dyt_step_fwd_bwd): before anything is enqueued
int check_mix_batch(const dyt_ctx* c, int batch) {
    if (!c->mix_params) return 0;
    if (const char* e = mix_count_error(batch, c->mix_frames)) { set_error("%s (batch %d, frames %d)", e, batch, c->mix_frames); return DYT_ERR_ARG; }
    return 0;
}

}  // namespace dyt

extern "C" int dyt_set_mix(dyt_ctx* c, const void* params_dev, int frames) {
    if (!c) { set_error("null ctx"); return DYT_ERR_ARG; }
    if (!params_dev) { c->mix_params = nullptr; return DYT_OK; }   // off: the passes enqueued from now on launch the plain kernels again
    { int rc = refuse_inference(c, "dyt_set_mix"); if (rc) return rc; }
    if (const char* e = mix_params_ptr_error((unsigned long long)reinterpret_cast<uintptr_t>(params_dev))) { set_error("dyt_set_mix: %s", e); return DYT_ERR_ARG; }
    if (frames != c->frames) { set_error("dyt_set_mix: frames = %d, the context folds %d frame(s) per clip", frames, c->frames); return DYT_ERR_ARG; }
    if (c->soft_targets) { set_error("dyt_set_mix: class-probability targets are set (dyt_set_soft_targets); mix writes its own"); return DYT_ERR_STATE; }
    if (!c->mix_soft) {   // once per context, outside any capture: the rows mix_targets_kernel writes and the loss reads
        const size_t bytes = (size_t)c->cfg.max_batch * c->cfg.num_classes * sizeof(float);
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&c->mix_soft), bytes);
        if (e != hipSuccess) { c->mix_soft = nullptr; set_error("dyt_set_mix: hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e)); return DYT_ERR_HIP; }
        c->mix_soft_bytes = bytes;
    }
    c->mix_params = static_cast<const MixParams*>(params_dev);
    c->mix_frames = frames;
    return DYT_OK;
}

extern "C" int dyt_mix_images(const void* src, float* dst, int count, int frames, int src_kind, const float mean[3], const float std[3],
                              const void* params_dev, void* stream) {
    if (!src || !dst) { set_error("dyt_mix_images: null pointer"); return DYT_ERR_ARG; }
    if (const char* e = mix_count_error(count, frames)) { set_error("dyt_mix_images: %s", e); return DYT_ERR_ARG; }
    if (const char* e = mix_src_error(src_kind, (unsigned long long)reinterpret_cast<uintptr_t>(src), (unsigned long long)reinterpret_cast<uintptr_t>(dst))) {
        set_error("dyt_mix_images: %s", e);
        return DYT_ERR_ARG;
    }
    if (const char* e = mix_params_ptr_error((unsigned long long)reinterpret_cast<uintptr_t>(params_dev))) { set_error("dyt_mix_images: %s", e); return DYT_ERR_ARG; }
    InputNorm nm = IN_NORM_IMAGENET;
    if (src_kind != 0) {   // float images are mixed as they are: mean / std may be null
        if (const char* e = input_norm_error(mean, std)) { set_error("dyt_mix_images: %s", e); return DYT_ERR_ARG; }
        for (int k = 0; k < 3; ++k) { nm.mean[k] = mean[k]; nm.std[k] = std[k]; }
    }
    return launch_mix_images(src, dst, count, frames, src_kind, nm, static_cast<const MixParams*>(params_dev), static_cast<hipStream_t>(stream));
}

extern "C" int dyt_mix_targets(const int64_t* labels, float* out, int rows, int num_classes, const void* params_dev, void* stream) {
    if (!labels || !out) { set_error("dyt_mix_targets: null pointer"); return DYT_ERR_ARG; }
    if (const char* e = mix_count_error(rows, 1)) { set_error("dyt_mix_targets: %s", e); return DYT_ERR_ARG; }
    if (const char* e = mix_classes_error(num_classes)) { set_error("dyt_mix_targets: %s", e); return DYT_ERR_ARG; }
    if (reinterpret_cast<uintptr_t>(out) % 16 != 0 || reinterpret_cast<uintptr_t>(labels) % 8 != 0) {
        set_error("dyt_mix_targets: out must be 16-byte aligned, labels 8-byte aligned");
        return DYT_ERR_ARG;
    }
    if (const char* e = mix_params_ptr_error((unsigned long long)reinterpret_cast<uintptr_t>(params_dev))) { set_error("dyt_mix_targets: %s", e); return DYT_ERR_ARG; }
    return launch_mix_targets(labels, out, rows, num_classes, static_cast<const MixParams*>(params_dev), static_cast<hipStream_t>(stream));
}
