// Small kernels in front of the first block (gfx950): the cls rows, and the dtype / layout converters of the weights.  (The image load
// of the patch embedding is image_load.hip.)
#include "kernels.h"
#include "rowhelp.h"

namespace dyt {

// ------------------------------------------------------------------------------------------
// patch embedding prologue
// ------------------------------------------------------------------------------------------
__global__ void cls_rows_kernel(const float* __restrict__ cls, const float* __restrict__ pos, float* __restrict__ x0, int batch) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= batch * D) return;
    const int b = idx / D, c = idx - b * D;
    x0[(size_t)b * NT * D + c] = cls[c] + pos[c];
}
int launch_cls_rows(const float* cls, const float* pos, float* x0, int batch, hipStream_t s) {
    hipLaunchKernelGGL(cls_rows_kernel, dim3((batch * D + 255) / 256), dim3(256), 0, s, cls, pos, x0, batch);
    LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------
// dtype / layout conversion of weights
// ------------------------------------------------------------------------------------------
template <class AT>
__global__ void pad_convert_kernel(const float* __restrict__ src, AT* __restrict__ dst, int rows, int cols, int drows,
                                   int dcols, int transpose) {
    // dst[dr][dc] = transpose ? src[dc][dr] : src[dr][dc], zero outside the source
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)drows * dcols) return;
    const int dr = (int)(idx / dcols), dc = (int)(idx - (size_t)dr * dcols);
    float v = 0.f;
    if (transpose) { if (dc < rows && dr < cols) v = src[(size_t)dc * cols + dr]; }
    else { if (dr < rows && dc < cols) v = src[(size_t)dr * cols + dc]; }
    dst[idx] = from_f32<AT>(v);
}
static int pad_convert(int precision, const float* src, void* dst, int rows, int cols, int drows, int dcols, int tr,
                       hipStream_t s) {
    const size_t total = (size_t)drows * dcols;
    const int grid = (int)((total + 255) / 256);
    if (precision == 0)
        hipLaunchKernelGGL(pad_convert_kernel<float>, dim3(grid), dim3(256), 0, s, src, (float*)dst, rows, cols, drows, dcols, tr);
    else
        hipLaunchKernelGGL(pad_convert_kernel<bf16>, dim3(grid), dim3(256), 0, s, src, (bf16*)dst, rows, cols, drows, dcols, tr);
    LAUNCH_CHECK();
    return 0;
}
int launch_convert(int precision, const float* src, void* dst, int64_t n, hipStream_t s) {
    return pad_convert(precision, src, dst, 1, (int)n, 1, (int)n, 0, s);
}
int launch_transpose_convert(int precision, const float* src, void* dst, int rows, int cols, int dst_rows, int dst_cols,
                             hipStream_t s) {
    return pad_convert(precision, src, dst, rows, cols, dst_rows, dst_cols, 1, s);
}
int launch_pad_convert(int precision, const float* src, void* dst, int rows, int cols, int dst_rows, int dst_cols,
                       hipStream_t s) {
    return pad_convert(precision, src, dst, rows, cols, dst_rows, dst_cols, 0, s);
}

}  // namespace dyt
