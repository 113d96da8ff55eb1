// What more than one attention family uses (attention_16.hip, attention_exact.hip, attention_split.hip): the padded tile geometry
// and the 16-bit LDS image strides, the fragment helpers, the register-staged image fill, and the per-family launch entries that
// attention.hip's two launchers hand over to.  N = 197 is padded to 224 = 7 x 32: K and V of one (image, head) live in LDS for the
// whole workgroup and a wave keeps the complete 32 x 224 score block of its tile in registers (pad keys are masked).
#pragma once
#include "kernels.h"

namespace dyt {

// one entry per family and direction; `r` is the route attention.hip got from attn_route.h (a kernel id of that family)
int launch_attn_fwd_16(const AttnFwdArgs& a, hipStream_t s);
int launch_attn_bwd_16(const AttnBwdArgs& a, const AttnBwdRoute& r, int out_ld, hipStream_t s);
int launch_attn_fwd_exact(const AttnFwdArgs& a, hipStream_t s);
int launch_attn_bwd_exact(const AttnBwdArgs& a, hipStream_t s);
int launch_attn_fwd_split(const AttnFwdArgs& a, const AttnFwdRoute& r, hipStream_t s);
int launch_attn_bwd_split(const AttnBwdArgs& a, const AttnBwdRoute& r, hipStream_t s);

constexpr int NPAD = 224;   // 7 tiles of 32
constexpr int RLD = 72;     // bf16 per row of a row-major [224][64] LDS image (144 B: conflict-free b128 fragment reads)
constexpr int TLD = 228;    // bf16 per row of a transposed [64][224] LDS image (456 B = 8 x odd: conflict-free b64 reads)
constexpr int ROW_IMG = NPAD * RLD * 2;  // 32256 B
constexpr int TR_IMG = HD * TLD * 2;     // 29184 B

__device__ __forceinline__ bf16x8 zero8() {
    bf16x8 z;
#pragma unroll
    for (int i = 0; i < 8; ++i) z[i] = (bf16)0.0f;
    return z;
}
__device__ __forceinline__ bf16x8 pack8(const f32x16& v, int base) {
    bf16x8 o;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = (bf16)v[base + i];
    return o;
}
__device__ __forceinline__ bf16x8 join44(const bf16* p) {  // p[0..3] and p[8..11]
    const bf16x4 a = *reinterpret_cast<const bf16x4*>(p);
    const bf16x4 b = *reinterpret_cast<const bf16x4*>(p + 8);
    bf16x8 o = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    return o;
}

// Stage a [197][64] matrix (row stride `ld` elements in global) into a row-major and/or a transposed LDS image; rows >= 197 are
// zero.  In two halves (load, store), so that a persistent workgroup can have the NEXT head's rows in flight (registers) while it
// computes on the current one: 896 tasks (row pair x 16-B chunk) over 448 threads = 2 tasks = 4 x 16 B per thread and matrix.
struct StageRegs { bf16x8 a[2], b[2]; };
__device__ __forceinline__ void stage_load(StageRegs& r, const bf16* __restrict__ src, int ld, int tid) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int t = tid + u * 448, pr = t >> 3, c = t & 7, r0 = pr * 2;
        // unconditional loads from clamped rows (no exec-masked branches in front of the loads); pad rows are zeroed afterwards
        r.a[u] = *reinterpret_cast<const bf16x8*>(src + (size_t)min(r0, NT - 1) * ld + c * 8);
        r.b[u] = *reinterpret_cast<const bf16x8*>(src + (size_t)min(r0 + 1, NT - 1) * ld + c * 8);
    }
}
__device__ __forceinline__ void stage_store(const StageRegs& r, bf16* rowimg, bf16* trimg, int tid) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int t = tid + u * 448, pr = t >> 3, c = t & 7, r0 = pr * 2;
        const bf16x8 a = r0 < NT ? r.a[u] : zero8(), b = r0 + 1 < NT ? r.b[u] : zero8();
        if (rowimg) {
            *reinterpret_cast<bf16x8*>(rowimg + r0 * RLD + c * 8) = a;
            *reinterpret_cast<bf16x8*>(rowimg + (r0 + 1) * RLD + c * 8) = b;
        }
        if (trimg) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                bf16x2 pv = {a[i], b[i]};
                *reinterpret_cast<bf16x2*>(trimg + (c * 8 + i) * TLD + r0) = pv;
            }
        }
    }
}

#define MFMA32(a, b, c) DYT_MFMA_32x32x16((a), (b), (c))

}  // namespace dyt
