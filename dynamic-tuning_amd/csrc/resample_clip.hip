// Device clip pipeline from byte clips: two context-free entries (dyt_resample_clip_f32, dyt_resample_clip_coeffs).  The row check, the
// index / weight function, the two-tap arithmetic and every argument check are resample_clip.h; the table layout is resample.h's; the
// row loader and the staging of a source row segment into LDS are resample_dev.h's, shared with the bicubic routes.
//
//   resample_clip_kernel         one block per (band of 8 output rows, frame, unit).  The block builds the 3 x 256 table of
//                                input_norm_value in LDS (as the byte loaders do), reads ITS row of the table -- one row serves all
//                                frames of its clip -- and then, per output row: stages the two source rows' column span (the bytes
//                                between the first and the last tap of the window) into LDS with 16-byte loads, and computes the 224 x 3
//                                values out of LDS, indices and weights in registers.  Work item = (channel, column): consecutive lanes
//                                store consecutive floats of one channel plane.
//   resample_clip_coeff_kernel   i0, i1, bits(l0), bits(l1) of both axes of one row, from the same clip_axis calls
//
// Source uint8 [batch, frames, Hs, Ws, 3] (padded; a clip's valid extent is its row's src_h x src_w), destination fp32
// [units, frames, 3, 224, 224].  The mirror is applied in the OUTPUT column (column x is computed from window position 223 - x).
// The kernels read the table from DEVICE memory when they run, so a captured graph replays with whatever the table holds by then.
// Nothing read from the table is used as an index before clip_row_ok has compared it (64-bit) against the batch's shape; a unit whose
// row fails the check, or that has no row, is written as zeros.  A 16-byte load is issued only where all 16 bytes lie inside the source
// allocation; the chunk that would cross its end is read byte by byte.  One writer per value, no atomics.  The same code in both builds.
#include "input_u8_dev.h"
#include "resample_dev.h"
#include "resample_clip.h"

namespace dyt {

namespace {

constexpr int RC_BAND = 8;                                   // output rows per block
constexpr int RC_STAGE = RS_MAX_SIDE * 3 + 32;               // bytes of one staged source row: the widest span plus the alignment slack at both ends
static_assert(RS_OUT % RC_BAND == 0 && RC_STAGE % 16 == 0, "bands tile the window; staged rows stay 16-byte aligned");

// false: unit u has no valid row (filter, units, capacity, clip_row_ok) and is written as zeros
__device__ __forceinline__ bool load_row(const int* __restrict__ table, int u, int capacity, int batch, int Hs, int Ws, ResampleRow& r) {
    return resample_load_row(table, RS_BILINEAR_F32, u, capacity, r) && clip_row_ok(r, batch, Hs, Ws);
}

}  // namespace

__global__ __launch_bounds__(256) void resample_clip_kernel(const uint8_t* __restrict__ src, int batch, int frames, int Hs, int Ws,
                                                            float* __restrict__ dst, const int* __restrict__ table, int capacity, InputNorm nm) {
    __shared__ float tab[3 * 256];
    __shared__ __attribute__((aligned(16))) uint8_t stage[2][RC_STAGE];
    const int tid = threadIdx.x, oy0 = blockIdx.x * RC_BAND, f = blockIdx.y, u = blockIdx.z;
    float* out = dst + ((size_t)u * frames + f) * 3 * RS_OUT * RS_OUT;
    ResampleRow row;
    if (!load_row(table, u, capacity, batch, Hs, Ws, row)) {   // uniform over the block
        for (int i = tid; i < 3 * RC_BAND * RS_OUT / 4; i += 256) {
            const int c = i / (RC_BAND * RS_OUT / 4), j = i - c * (RC_BAND * RS_OUT / 4);
            reinterpret_cast<float4*>(out + (size_t)c * RS_OUT * RS_OUT + oy0 * RS_OUT)[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
        return;
    }
    build_table(tab, nm);   // (ends with a barrier)
    const bool mirror = (row.flags & RS_FLAG_MIRROR) != 0;
    // the columns (relative to the box) the window's taps touch: [xs_lo, xs_hi]; taps are monotone in the position
    int xs_lo, xs_hi, t0, t1;
    float w0, w1;
    clip_axis(row.box_w, row.full_w, row.off_x, xs_lo, t1, w0, w1);
    clip_axis(row.box_w, row.full_w, row.off_x + RS_OUT - 1, t0, xs_hi, w0, w1);
    const long long total = (long long)batch * frames * Hs * Ws * 3;                 // bytes of the source allocation
    const long long plane = ((long long)clip_row_src(row) * frames + f) * Hs;        // first padded row of this frame
    const int span = (xs_hi - xs_lo + 1) * 3;                                        // <= 3 * box_w <= 3 * 4096
    // this thread's work items: (channel, column) i = tid, tid + 256, tid + 512 of 672; their taps do not depend on the output row
    int px0[3], px1[3];
    float lx0[3], lx1[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int i = tid + 256 * k, c = i / RS_OUT, x = i - c * RS_OUT;
        int a = 0, b = 0;
        lx0[k] = lx1[k] = 0.0f;
        if (i < 3 * RS_OUT) clip_axis(row.box_w, row.full_w, row.off_x + (mirror ? RS_OUT - 1 - x : x), a, b, lx0[k], lx1[k]);
        px0[k] = (a - xs_lo) * 3 + c;
        px1[k] = (b - xs_lo) * 3 + c;
    }
    for (int j = 0; j < RC_BAND; ++j) {
        const int oy = oy0 + j;
        int y[2];
        float ly0, ly1;
        clip_axis(row.box_h, row.full_h, row.off_y + oy, y[0], y[1], ly0, ly1);
        int shift[2];
#pragma unroll
        for (int s = 0; s < 2; ++s)   // the span's bytes of source rows y[0], y[1]
            shift[s] = resample_stage_row(src, total, ((plane + row.top + y[s]) * Ws + row.left + xs_lo) * 3, span, stage[s], RC_STAGE / 16, tid);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int i = tid + 256 * k;
            if (i < 3 * RS_OUT) {
                const int c = i / RS_OUT, x = i - c * RS_OUT;
                const float* t = tab + c * 256;
                const float r0 = clip_lerp(lx0[k], t[stage[0][shift[0] + px0[k]]], lx1[k], t[stage[0][shift[0] + px1[k]]]);
                const float r1 = clip_lerp(lx0[k], t[stage[1][shift[1] + px0[k]]], lx1[k], t[stage[1][shift[1] + px1[k]]]);
                out[(size_t)c * RS_OUT * RS_OUT + oy * RS_OUT + x] = clip_lerp(ly0, r0, ly1, r1);
            }
        }
        __syncthreads();   // the next row's staging overwrites what this row read
    }
}

__global__ __launch_bounds__(256) void resample_clip_coeff_kernel(const int* __restrict__ table, int capacity, int Hs, int Ws, int unit,
                                                                  int* __restrict__ out) {
    const int axis = blockIdx.x, t = threadIdx.x;
    if (t >= RS_OUT) return;
    ResampleRow r;
    const bool ok = load_row(table, unit, capacity, 0x7FFFFFFF, Hs, Ws, r);   // (no source is read here: any src >= 0 passes)
    int i0 = 0, i1 = 0;
    float l0 = 0.0f, l1 = 0.0f;
    if (ok) {
        if (axis == 0) clip_axis(r.box_h, r.full_h, r.off_y + t, i0, i1, l0, l1);
        else clip_axis(r.box_w, r.full_w, r.off_x + t, i0, i1, l0, l1);
    }
    int* o = out + axis * 4 * RS_OUT + t;
    o[0] = i0;
    o[RS_OUT] = i1;
    o[2 * RS_OUT] = ok ? __float_as_int(l0) : 0;
    o[3 * RS_OUT] = ok ? __float_as_int(l1) : 0;
}

}  // namespace dyt

using namespace dyt;

extern "C" int dyt_resample_clip_f32(const uint8_t* src, int batch, int frames, int src_h, int src_w, float* dst, int units,
                                     const void* table_dev, int capacity, const float mean[3], const float std[3], void* stream) {
    if (const char* e = clip_ptr_error(resample_addr(src), resample_addr(dst), resample_addr(table_dev))) { set_error("dyt_resample_clip_f32: %s", e); return DYT_ERR_ARG; }
    if (const char* e = clip_shape_error(batch, frames, src_h, src_w, units, capacity)) {
        set_error("dyt_resample_clip_f32: %s (batch %d, frames %d, source %d x %d, units %d, table capacity %d)", e, batch, frames, src_h, src_w,
                  units, capacity);
        return DYT_ERR_ARG;
    }
    if (const char* e = clip_norm_error(mean, std)) { set_error("dyt_resample_clip_f32: %s", e); return DYT_ERR_ARG; }
    InputNorm nm;
    for (int k = 0; k < 3; ++k) { nm.mean[k] = mean[k]; nm.std[k] = std[k]; }
    hipLaunchKernelGGL(resample_clip_kernel, dim3(RS_OUT / RC_BAND, (unsigned)frames, (unsigned)units), dim3(256), 0,
                       static_cast<hipStream_t>(stream), src, batch, frames, src_h, src_w, dst, static_cast<const int*>(table_dev), capacity, nm);
    DYT_HIP_CHECK(hipGetLastError());
    return DYT_OK;
}

extern "C" int dyt_resample_clip_coeffs(const void* table_dev, int capacity, int row, int src_h, int src_w, int32_t* out_dev, void* stream) {
    if (resample_coeffs_refusal("dyt_resample_clip_coeffs", clip_ptr_error(16, resample_addr(out_dev), resample_addr(table_dev)),
                                clip_shape_error(1, 1, src_h, src_w, 1, capacity), row, capacity)) return DYT_ERR_ARG;
    hipLaunchKernelGGL(resample_clip_coeff_kernel, dim3(2, 1), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const int*>(table_dev), capacity, src_h, src_w, row, out_dev);
    DYT_HIP_CHECK(hipGetLastError());
    return DYT_OK;
}
