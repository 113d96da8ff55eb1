// Device helpers of the image-load kernel (image_load.hip): a run's raw load and its conversion to floats (bytes through the LDS table of
// input_u8_dev.h), the run-level Mixup / CutMix of mix.h, the run-level Random Erasing of erase.h, and the store.  Private to that unit.
#pragma once
#include "input_u8_dev.h"
#include "image_items.h"

namespace dyt {
namespace {

// ---- a run as loaded, and as floats ---------------------------------------------------------------------------------------------------------
struct Bytes48 { uint4 w[3]; };   // 16 pixels x 3 channels of a channels-last row
template <int KIND> struct RunOf { typedef uint8_t Elem; typedef uint4 Raw; };
template <> struct RunOf<IMAGE_SRC_F32> { typedef float Elem; typedef float4 Raw; };
template <> struct RunOf<IMAGE_SRC_U8_NHWC> { typedef uint8_t Elem; typedef Bytes48 Raw; };

__device__ __forceinline__ unsigned byte_of(const uint4& q, int m) {        // byte m of 16 (m is a constant after unrolling)
    const unsigned word = (m >> 2) == 0 ? q.x : (m >> 2) == 1 ? q.y : (m >> 2) == 2 ? q.z : q.w;
    return (word >> ((m & 3) * 8)) & 0xFFu;
}

// the floats of channel c of a run: the fp32 pixels themselves; the 16 bytes, or every third byte of the 48, through the table
__device__ __forceinline__ void run_values(float (&v)[4], const float*, const float4& q, int) { v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
__device__ __forceinline__ void run_values(float (&v)[16], const float* tab, const uint4& w, int c) {
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = tab[c * 256 + byte_of(w, j)];
}
__device__ __forceinline__ void run_values(float (&v)[16], const float* tab, const Bytes48& r, int c) {
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = tab[c * 256 + byte_of(r.w[(j * 3 + c) >> 4], (j * 3 + c) & 15)];
}

// N consecutive output elements
template <class T, int N>
__device__ __forceinline__ void store_run(T* dst, const float (&v)[N]) {
#pragma unroll
    for (int j = 0; j < N; j += 4) store4(dst + j, v[j], v[j + 1], v[j + 2], v[j + 3]);
}

// ---- mix -------------------------------------------------------------------------------------------------------------------------------------
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

// ---- erase -----------------------------------------------------------------------------------------------------------------------------------
struct EraseCtl { int mode, cube, units; unsigned long long seed; };

__device__ __forceinline__ EraseCtl erase_ctl(const int* __restrict__ table) {
    const int4 a = *reinterpret_cast<const int4*>(table);
    const int2 b = *reinterpret_cast<const int2*>(table + 4);
    EraseCtl h;
    h.mode = (a.x < ERASE_CONST || a.x > ERASE_PIXEL) ? ERASE_OFF : a.x;
    h.cube = a.z;
    h.units = a.w;
    h.seed = (unsigned long long)(unsigned)b.x | ((unsigned long long)(unsigned)b.y << 32);
    return h;
}

// false: image n has no box (mode off, no row, count 0) and `row` is not filled
__device__ __forceinline__ bool erase_row(const int* __restrict__ table, const EraseCtl& h, int n, int frames, int capacity, EraseRow& row) {
    if (h.mode == ERASE_OFF) return false;
    const int u = erase_unit(n, frames, h.cube, h.units, capacity);
    if (u < 0) return false;
    const int4* q = reinterpret_cast<const int4*>(table + ERASE_HEADER_WORDS + (size_t)u * ERASE_ROW_WORDS);
    const int4 q0 = q[0];
    row.n = erase_clamp_n(q0.x);
    if (row.n == 0) return false;
    const int4 q1 = q[1], q2 = q[2], q3 = q[3], q4 = q[4];
    row.box[0][0] = q0.y; row.box[0][1] = q0.z; row.box[0][2] = q0.w; row.box[0][3] = q1.x;
    row.box[1][0] = q1.y; row.box[1][1] = q1.z; row.box[1][2] = q1.w; row.box[1][3] = q2.x;
    row.box[2][0] = q2.y; row.box[2][1] = q2.z; row.box[2][2] = q2.w; row.box[2][3] = q3.x;
    row.box[3][0] = q3.y; row.box[3][1] = q3.z; row.box[3][2] = q3.w; row.box[3][3] = q4.x;
    return true;
}

// The boxes of image n over the run of N pixels (N a multiple of 4, at most 16) of row y from column x0, channel-independent: 3 bits per
// pixel, erase_hit + 1.  0: the run is untouched (mode off, no row, no box, or no box meets the run).
template <int N>
__device__ __forceinline__ unsigned long long erase_code(const int* __restrict__ table, const EraseCtl& h, int n, int frames, int capacity, int y, int x0) {
    EraseRow row;
    if (!erase_row(table, h, n, frames, capacity, row)) return 0;
    if (!erase_run_hits(row, y, x0, N)) return 0;
    unsigned long long code = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) code |= (unsigned long long)(erase_hit(row, y, x0 + j) + 1) << (3 * j);
    return code;
}

// The noise of erase.h behind calls: a run meets a box rarely, and up to 24 inlined copies of logf / sinf / cosf (16 pixels x 3 channels, own
// and partner) would cost every thread of the load their registers.
__device__ __noinline__ float4 erase_noise4(unsigned long long seed, int n, int c, int y, int x4) {
    float z[4];
    erase_pixel_noise4<Philox>(seed, n, c, y, x4, z);
    return make_float4(z[0], z[1], z[2], z[3]);
}
__device__ __noinline__ float erase_colour(unsigned long long seed, int n, int box, int c) { return erase_box_colour<Philox>(seed, n, box, c); }

// v: N pixels of channel c, row y of image n from column x0 (a multiple of 4); code: erase_code of that run
template <int N>
__device__ __forceinline__ void erase_run(float (&v)[N], const EraseCtl& h, unsigned long long code, int n, int c, int y, int x0) {
    if (code == 0) return;
    int cached = -1;
    float colour = 0.f;
#pragma unroll
    for (int g = 0; g < N; g += 4) {
        const unsigned bits = (unsigned)(code >> (3 * g)) & 0xFFFu;
        if (bits == 0) continue;
        if (h.mode == ERASE_PIXEL) {
            const float4 z4 = erase_noise4(h.seed, n, c, y, (x0 + g) >> 2);
            const float z[4] = {z4.x, z4.y, z4.z, z4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if ((bits >> (3 * j)) & 7u) v[g + j] = z[j];
        } else if (h.mode == ERASE_RAND) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int hit = (int)((bits >> (3 * j)) & 7u) - 1;
                if (hit >= 0) {
                    if (hit != cached) { cached = hit; colour = erase_colour(h.seed, n, cached, c); }
                    v[g + j] = colour;
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if ((bits >> (3 * j)) & 7u) v[g + j] = 0.f;
        }
    }
}

}  // namespace
}  // namespace dyt
