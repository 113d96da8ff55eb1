// Device helper shared by the kernels that normalise byte images (image_load.hip, resample_clip.hip): the 3 x 256 table of input_norm_value
// in LDS.  Private to those units.
#pragma once
#include "ctx.h"

namespace dyt {
namespace {

__device__ __forceinline__ void build_table(float* tab, const InputNorm& nm) {
    const unsigned u = threadIdx.x;   // 256 threads: one byte value each, all three channels
#pragma unroll
    for (int c = 0; c < 3; ++c) tab[c * 256 + u] = input_norm_value(u, nm.mean[c], nm.std[c]);
    __syncthreads();
}

}  // namespace
}  // namespace dyt
