// Device helpers shared by the units that mix in the image load (mix.hip, erase.hip): the run-level Mixup / CutMix of mix.h, the unpacking
// of a 16-byte float load and the table lookups of a 16-pixel byte run.  Private to those two units.
#pragma once
#include "input_u8_dev.h"

namespace dyt {
namespace {

constexpr size_t PLANE = (size_t)IMG * IMG;

// v: N own pixels of row y from column x0; w: the partner's.  Called only when mix_run_needs_partner.
template <int N>
__device__ __forceinline__ void mix_run(float (&v)[N], const float (&w)[N], const MixParams& p, int y, int x0) {
    if (p.mode == MIX_MIXUP) {
#pragma unroll
        for (int j = 0; j < N; ++j) v[j] = mix_value(v[j], w[j], p.lam_f, p.oml_f);
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j)
            if (mix_from_partner(p.mode, y, x0 + j, p.yl, p.yh, p.xl, p.xh)) v[j] = w[j];
    }
}

__device__ __forceinline__ void unpack(float (&v)[4], const float4& q) { v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }

// 16 pixels of channel c (NCHW run: the 16 bytes of w; NHWC run: every third byte of the 48) through the table
__device__ __forceinline__ void lookup(float (&v)[16], const float* tab, const uint4& w, int c) {
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = tab[c * 256 + byte_of(w, j)];
}
__device__ __forceinline__ void lookup(float (&v)[16], const float* tab, const uint4 (&w)[3], int c) {
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = tab[c * 256 + byte_of(w, j * 3 + c)];
}

}  // namespace
}  // namespace dyt
