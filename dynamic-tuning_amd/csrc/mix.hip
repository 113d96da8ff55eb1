// On-device Mixup / CutMix: the entries and checks of the mix fused into the patch-embedding load (dyt_set_mix) and of the two
// context-free forms (dyt_mix_images, dyt_mix_targets), and the kernel of the class-probability rows.  The image kernel is
// image_load.hip's; the scalar formula, the pairing, the source predicate and every argument check are mix.h.
//
//   mix_targets_kernel<VEC>   int64 labels -> fp32 [rows, C] class-probability rows; reads its MixParams block from DEVICE memory (one
//                             64-byte load per thread, the same address for all), uses nothing of it as an index
#include "ctx.h"
#include "image_items.h"

namespace dyt {

#define LAUNCH_CHECK() DYT_HIP_CHECK(hipGetLastError())

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
    ImageLoadArgs a;
    a.src = src; a.src_kind = src_kind;
    a.dst = dst; a.dst_kind = IMAGE_DST_PLANES;
    a.batch = count; a.frames = frames;
    a.mix = static_cast<const MixParams*>(params_dev);
    if (src_kind != IMAGE_SRC_F32) {   // float images are mixed as they are: mean / std may be null
        if (const char* e = input_norm_error(mean, std)) { set_error("dyt_mix_images: %s", e); return DYT_ERR_ARG; }
        for (int k = 0; k < 3; ++k) { a.norm.mean[k] = mean[k]; a.norm.std[k] = std[k]; }
    }
    return launch_image_load(a, static_cast<hipStream_t>(stream));
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
