// Byte-image input: uint8 batches normalised where the patch embedding loads them (DYT_F_IMAGES_U8), and dyt_normalize_u8.
//
//   im2col_u8_kernel<AT, NHWC>   bytes [B,3,224,224] / [B,224,224,3] -> the EPI_EMBED GEMM's A operand, the buffer and element order of
//                                im2col_kernel (embed.hip): out[(b*196 + py*14 + px)*768 + c*256 + i*16 + j]
//   normalize_u8_kernel<NHWC>    the same bytes -> fp32 [B,3,224,224]
//
// Both evaluate input_norm_value (input_norm.h) -- ((float)u / 255.0f - mean[c]) / std[c], three correctly rounded fp32 operations --
// once per (channel, byte value): every workgroup builds the 3 x 256 table in LDS (6 divisions per thread) and then looks its pixels
// up, instead of two divisions per pixel.  A thread owns 16 consecutive pixels of one image row: one 16-byte load per channel-major
// run, three for a channels-last run (48 contiguous bytes, de-interleaved in registers), and 16 consecutive output elements per
// channel.  In the im2col element order the 16 pixels of a patch row are 16 consecutive operand elements, and consecutive work items
// are consecutive 16-element groups, so a wave's stores are contiguous.  No atomics; every output element has one writer.
#include "input_u8_dev.h"

namespace dyt {

#define LAUNCH_CHECK() DYT_HIP_CHECK(hipGetLastError())

template <class AT, bool NHWC>
__global__ __launch_bounds__(256) void im2col_u8_kernel(const uint8_t* __restrict__ img, AT* __restrict__ out, int batch, InputNorm nm) {
    __shared__ float tab[3 * 256];
    build_table(tab, nm);
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (NHWC) {
        // work item = (b, patch, i): 48 contiguous bytes = 16 pixels x 3 channels -> three 16-element runs of the operand row
        const size_t total = (size_t)batch * NP * PS;
        if (idx >= total) return;
        const int i = (int)(idx % PS);
        const size_t row = idx / PS;                       // b * 196 + patch
        const int p = (int)(row % NP);
        const size_t b = row / NP;
        const int py = p / GRID_P, px = p - py * GRID_P;
        const uint4* src = reinterpret_cast<const uint4*>(img + ((b * IMG + py * PS + i) * IMG + px * PS) * 3);
        const uint4 w[3] = {src[0], src[1], src[2]};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) v[j] = tab[c * 256 + byte_of(w, j * 3 + c)];
            store16(out + row * D + c * 256 + i * PS, v);
        }
    } else {
        // work item = (b, patch, c, i) = 16-element group idx of the operand: out + idx * 16
        const size_t total = (size_t)batch * NP * 3 * PS;
        if (idx >= total) return;
        const int i = (int)(idx % PS);
        const int c = (int)((idx / PS) % 3);
        const size_t row = idx / (3 * PS);
        const int p = (int)(row % NP);
        const size_t b = row / NP;
        const int py = p / GRID_P, px = p - py * GRID_P;
        const uint4 w = *reinterpret_cast<const uint4*>(img + ((b * 3 + c) * IMG + py * PS + i) * IMG + px * PS);
        const float* t = tab + c * 256;
        float v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = t[byte_of(w, j)];
        store16(out + idx * 16, v);
    }
}

template <bool NHWC>
__global__ __launch_bounds__(256) void normalize_u8_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, int batch, InputNorm nm) {
    __shared__ float tab[3 * 256];
    build_table(tab, nm);
    constexpr size_t PLANE = (size_t)IMG * IMG;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (NHWC) {
        // work item = 16 consecutive pixels of an image (48 contiguous bytes) -> 16 floats in each of its three planes
        const size_t total = (size_t)batch * PLANE / 16;
        if (idx >= total) return;
        const size_t b = idx / (PLANE / 16), q = idx - b * (PLANE / 16);
        const uint4* s4 = reinterpret_cast<const uint4*>(src + idx * 48);
        const uint4 w[3] = {s4[0], s4[1], s4[2]};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) v[j] = tab[c * 256 + byte_of(w, j * 3 + c)];
            store16(dst + (b * 3 + c) * PLANE + q * 16, v);
        }
    } else {
        const size_t total = (size_t)batch * 3 * PLANE / 16;
        if (idx >= total) return;
        const int c = (int)((idx / (PLANE / 16)) % 3);
        const uint4 w = *reinterpret_cast<const uint4*>(src + idx * 16);
        const float* t = tab + c * 256;
        float v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = t[byte_of(w, j)];
        store16(dst + idx * 16, v);
    }
}

int launch_im2col_u8(int precision, const uint8_t* images, int nhwc, const InputNorm& nm, void* out, int batch, hipStream_t s) {
    const size_t total = (size_t)batch * NP * PS * (nhwc ? 1 : 3);
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    if (precision == 0) {
        if (nhwc) hipLaunchKernelGGL((im2col_u8_kernel<float, true>), grid, block, 0, s, images, (float*)out, batch, nm);
        else hipLaunchKernelGGL((im2col_u8_kernel<float, false>), grid, block, 0, s, images, (float*)out, batch, nm);
    } else {
        if (nhwc) hipLaunchKernelGGL((im2col_u8_kernel<bf16, true>), grid, block, 0, s, images, (bf16*)out, batch, nm);
        else hipLaunchKernelGGL((im2col_u8_kernel<bf16, false>), grid, block, 0, s, images, (bf16*)out, batch, nm);
    }
    LAUNCH_CHECK();
    return 0;
}

int launch_normalize_u8(const uint8_t* src, float* dst, int batch, int nhwc, const InputNorm& nm, hipStream_t s) {
    const size_t total = (size_t)batch * IMG * IMG / 16 * (nhwc ? 1 : 3);
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    if (nhwc) hipLaunchKernelGGL(normalize_u8_kernel<true>, grid, block, 0, s, src, dst, batch, nm);
    else hipLaunchKernelGGL(normalize_u8_kernel<false>, grid, block, 0, s, src, dst, batch, nm);
    LAUNCH_CHECK();
    return 0;
}

// the checks of a pass that takes `images` (dyt_forward, dyt_step_fwd_bwd): before anything is enqueued
int check_image_input(int flags, const void* images) {
    if (const char* e = input_flags_error(flags)) { set_error("%s", e); return DYT_ERR_ARG; }
    if (flags & DYT_F_IMAGES_U8)
        if (const char* e = input_ptr_error((unsigned long long)reinterpret_cast<uintptr_t>(images))) { set_error("%s", e); return DYT_ERR_ARG; }
    return 0;
}

}  // namespace dyt

extern "C" int dyt_set_input_norm(dyt_ctx* c, const float mean[3], const float std[3]) {
    if (!c) { set_error("null ctx"); return DYT_ERR_ARG; }
    if (const char* e = input_norm_error(mean, std)) { set_error("dyt_set_input_norm: %s", e); return DYT_ERR_ARG; }
    // host values only: they travel in the arguments of the launches enqueued from now on; a step in flight keeps the ones it was enqueued with
    for (int k = 0; k < 3; ++k) { c->in_norm.mean[k] = mean[k]; c->in_norm.std[k] = std[k]; }
    return DYT_OK;
}

extern "C" int dyt_normalize_u8(const uint8_t* src, float* dst, int batch, int nhwc, const float mean[3], const float std[3], void* stream) {
    if (!src || !dst || batch < 1) { set_error("dyt_normalize_u8: null pointer or batch < 1"); return DYT_ERR_ARG; }
    if (const char* e = input_norm_error(mean, std)) { set_error("dyt_normalize_u8: %s", e); return DYT_ERR_ARG; }
    if (const char* e = input_ptr_error((unsigned long long)reinterpret_cast<uintptr_t>(src))) { set_error("dyt_normalize_u8: %s", e); return DYT_ERR_ARG; }
    if (reinterpret_cast<uintptr_t>(dst) % 16 != 0) { set_error("dyt_normalize_u8: dst must be 16-byte aligned"); return DYT_ERR_ARG; }
    InputNorm nm;
    for (int k = 0; k < 3; ++k) { nm.mean[k] = mean[k]; nm.std[k] = std[k]; }
    return launch_normalize_u8(src, dst, batch, nhwc != 0, nm, static_cast<hipStream_t>(stream));
}
