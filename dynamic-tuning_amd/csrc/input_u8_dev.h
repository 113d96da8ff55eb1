// Device helpers shared by the kernels that read byte images (input_u8.hip, mix.hip, erase.hip): the 3 x 256 table of input_norm_value in LDS, byte
// extraction from 16- and 48-byte runs, and the 16-element store.  Private to those units.
#pragma once
#include "ctx.h"

namespace dyt {
namespace {

constexpr int IMG = 224, PS = 16, GRID_P = IMG / PS;   // 14 x 14 patches of 16 x 16

__device__ __forceinline__ void build_table(float* tab, const InputNorm& nm) {
    const unsigned u = threadIdx.x;   // 256 threads: one byte value each, all three channels
#pragma unroll
    for (int c = 0; c < 3; ++c) tab[c * 256 + u] = input_norm_value(u, nm.mean[c], nm.std[c]);
    __syncthreads();
}

__device__ __forceinline__ unsigned byte_of(const uint4 (&w)[3], int n) {   // byte n of 48 (n is a constant after unrolling)
    const uint4& q = w[n >> 4];
    const int m = n & 15;
    const unsigned word = (m >> 2) == 0 ? q.x : (m >> 2) == 1 ? q.y : (m >> 2) == 2 ? q.z : q.w;
    return (word >> ((m & 3) * 8)) & 0xFFu;
}
__device__ __forceinline__ unsigned byte_of(const uint4& q, int m) {        // byte m of 16
    const unsigned word = (m >> 2) == 0 ? q.x : (m >> 2) == 1 ? q.y : (m >> 2) == 2 ? q.z : q.w;
    return (word >> ((m & 3) * 8)) & 0xFFu;
}

// 16 consecutive output elements from 16 table entries
template <class T>
__device__ __forceinline__ void store16(T* dst, const float (&v)[16]) {
#pragma unroll
    for (int j = 0; j < 16; j += 4) store4(dst + j, v[j], v[j + 1], v[j + 2], v[j + 3]);
}

}  // namespace
}  // namespace dyt
