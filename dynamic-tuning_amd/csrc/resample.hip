// Device RandomResizedCrop / flip / Resize + CenterCrop from byte sources: three context-free entries (dyt_resample_u8,
// dyt_resample_scratch_bytes, dyt_resample_coeffs).  The table layout, the row check, the coefficient function and every argument check
// are resample.h.
//
//   resample_coeff_kernel   one block per (axis, image): thread t computes resample_coeffs of window position t -- first tap, tap count,
//                           11 coefficients, fp64 without contraction -- into the scratch buffer, [axis][field][224] ints per image
//   resample_band_kernel    one block per (band of 16 output rows, image): the horizontal pass over the source rows the band's vertical
//                           taps need (at most 48) into LDS as bytes, then the vertical pass out of LDS, 16 bytes per work item and store
//
// Source uint8 [B, Hs, Ws, 3] (padded; an image's valid extent is its row's src_h x src_w), destination uint8 [B, 224, 224, 3].  The
// arithmetic of both passes is Pillow's: int32, ss = 2^21 + sum(pixel * k), clamp(ss >> 22, 0, 255); the horizontal pass rounds to uint8.
// The mirror is applied where the horizontal pass stores into LDS, so the vertical pass and the global stores stay 16-byte runs.
// Every kernel reads the table from DEVICE memory when it runs, so a captured graph replays with whatever the table holds by then.
// Nothing read from the table is used as an index before resample_row_ok has compared it (64-bit) against the batch's shape; the
// coefficient bounds read back from scratch are clamped against the box again.  An image whose row fails the check is written as zeros.
// One writer per byte, no atomics, no floating point in the pixel passes.  The same code in both builds of the library.
#include "../../include/dyt_hip.h"
#include "dyt_common.h"
#include "resample.h"

namespace dyt {

namespace {

constexpr int RS_BAND = 16;                 // output rows per block
constexpr int RS_ROWB = RS_OUT * 3;         // bytes of one 224-pixel row: 672 = 42 x 16
constexpr int RS_GROUPS = RS_ROWB / 16;
constexpr int RS_MAXROWS = 48;              // source rows one band's vertical taps span: 15 * 2.5 + 2 * 5 + 1 (truncation), rounded down
static_assert(RS_ROWB % 16 == 0, "a 224-pixel byte row is a whole number of 16-byte runs");

// false: image b has no valid row (filter, units, capacity, resample_row_ok) and is written as zeros
__device__ __forceinline__ bool resample_load_row(const int* __restrict__ table, int b, int capacity, int Hs, int Ws, ResampleRow& r) {
    const int2 h = *reinterpret_cast<const int2*>(table);
    if (h.x != RS_BICUBIC) return false;
    const int u = resample_unit(b, h.y, capacity);
    if (u < 0) return false;
    const int4* q = reinterpret_cast<const int4*>(table + RS_HEADER_WORDS + (size_t)u * RS_ROW_WORDS);
    const int4 q0 = q[0], q1 = q[1], q2 = q[2];
    r.src_h = q0.x; r.src_w = q0.y; r.top = q0.z; r.left = q0.w;
    r.box_h = q1.x; r.box_w = q1.y; r.full_h = q1.z; r.full_w = q1.w;
    r.off_y = q2.x; r.off_x = q2.y; r.flags = q2.z; r.pad = 0;
    return resample_row_ok(r, Hs, Ws);
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

}  // namespace

__global__ __launch_bounds__(256) void resample_coeff_kernel(const int* __restrict__ table, int capacity, int Hs, int Ws, int img_base,
                                                             int* __restrict__ out) {
    const int axis = blockIdx.x, t = threadIdx.x;
    if (t >= RS_OUT) return;
    ResampleRow r;
    const bool ok = resample_load_row(table, img_base + (int)blockIdx.y, capacity, Hs, Ws, r);
    int xmin = 0, count = 0;
    int k[RS_KMAX];
#pragma unroll
    for (int x = 0; x < RS_KMAX; ++x) k[x] = 0;
    if (ok) {
        if (axis == 0) resample_coeffs(r.box_h, r.full_h, r.off_y + t, xmin, count, k);
        else resample_coeffs(r.box_w, r.full_w, r.off_x + t, xmin, count, k);
    }
    int* o = out + (size_t)blockIdx.y * RS_COEFF_WORDS + axis * RS_COEFF_FIELDS * RS_OUT + t;
    o[0] = xmin;
    o[RS_OUT] = count;
#pragma unroll
    for (int x = 0; x < RS_KMAX; ++x) o[(2 + x) * RS_OUT] = k[x];
}

__global__ __launch_bounds__(256) void resample_band_kernel(const uint8_t* __restrict__ src, int Hs, int Ws, uint8_t* __restrict__ dst,
                                                            const int* __restrict__ table, int capacity, const int* __restrict__ coeffs) {
    __shared__ __attribute__((aligned(16))) uint8_t tmp[RS_MAXROWS * RS_ROWB];   // horizontally resampled source rows, window columns (mirrored if asked)
    __shared__ int hc[RS_COEFF_FIELDS * RS_OUT];                                  // column coefficients [field][224]
    __shared__ int vc[RS_COEFF_FIELDS * RS_BAND];                                 // row coefficients of this band [field][16]
    const int b = blockIdx.y, oy0 = blockIdx.x * RS_BAND, tid = threadIdx.x;
    uint8_t* out = dst + ((size_t)b * RS_OUT + oy0) * RS_ROWB;
    ResampleRow row;
    if (!resample_load_row(table, b, capacity, Hs, Ws, row)) {   // uniform over the block
        for (int i = tid; i < RS_BAND * RS_GROUPS; i += 256) reinterpret_cast<uint4*>(out)[i] = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    const int* cf = coeffs + (size_t)b * RS_COEFF_WORDS;
    for (int i = tid; i < RS_COEFF_FIELDS * RS_OUT; i += 256) hc[i] = cf[RS_COEFF_FIELDS * RS_OUT + i];
    for (int i = tid; i < RS_COEFF_FIELDS * RS_BAND; i += 256) {
        const int f = i / RS_BAND, j = i - f * RS_BAND;
        vc[i] = cf[f * RS_OUT + oy0 + j];
    }
    __syncthreads();
    // the source rows (relative to the box) the band reads: [r0, r0 + nrows).  Bounds from scratch are clamped against the box again.
    int r0 = row.box_h, r1 = 0;
#pragma unroll
    for (int j = 0; j < RS_BAND; ++j) {
        const int lo = clampi(vc[j], 0, row.box_h - 1);
        const int n = clampi(vc[RS_BAND + j], 0, min(RS_KMAX, row.box_h - lo));
        r0 = min(r0, lo);
        r1 = max(r1, lo + n);
    }
    const int nrows = clampi(r1 - r0, 0, RS_MAXROWS);
    const bool mirror = (row.flags & RS_FLAG_MIRROR) != 0;
    const uint8_t* base = src + (((size_t)b * Hs + row.top + r0) * Ws + row.left) * 3;
    for (int idx = tid; idx < nrows * RS_OUT; idx += 256) {
        const int r = idx / RS_OUT, ox = idx - r * RS_OUT;
        const int lo = clampi(hc[ox], 0, row.box_w - 1);
        const int n = clampi(hc[RS_OUT + ox], 0, min(RS_KMAX, row.box_w - lo));
        const uint8_t* p = base + ((size_t)r * Ws + lo) * 3;
        int s0 = 1 << (RS_PRECISION_BITS - 1), s1 = s0, s2 = s0;
#pragma unroll
        for (int x = 0; x < RS_KMAX; ++x) {
            if (x < n) {
                const int k = hc[(2 + x) * RS_OUT + ox];
                s0 += (int)p[3 * x] * k;
                s1 += (int)p[3 * x + 1] * k;
                s2 += (int)p[3 * x + 2] * k;
            }
        }
        uint8_t* q = tmp + r * RS_ROWB + (mirror ? RS_OUT - 1 - ox : ox) * 3;
        q[0] = (uint8_t)resample_clip8(s0);
        q[1] = (uint8_t)resample_clip8(s1);
        q[2] = (uint8_t)resample_clip8(s2);
    }
    __syncthreads();
    for (int idx = tid; idx < RS_BAND * RS_GROUPS; idx += 256) {
        const int j = idx / RS_GROUPS, g = idx - j * RS_GROUPS;
        const int lo = clampi(vc[j], 0, row.box_h - 1);
        const int n = clampi(vc[RS_BAND + j], 0, min(RS_KMAX, row.box_h - lo));
        int acc[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 1 << (RS_PRECISION_BITS - 1);
#pragma unroll
        for (int x = 0; x < RS_KMAX; ++x) {
            const int rr = lo - r0 + x;
            if (x < n && rr < nrows) {
                const int k = vc[(2 + x) * RS_BAND + j];
                const uint4 v = *reinterpret_cast<const uint4*>(tmp + rr * RS_ROWB + g * 16);
                const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] += (int)((w[i >> 2] >> (8 * (i & 3))) & 0xFFu) * k;
            }
        }
        unsigned w[4];
#pragma unroll
        for (int d = 0; d < 4; ++d)
            w[d] = (unsigned)resample_clip8(acc[4 * d]) | ((unsigned)resample_clip8(acc[4 * d + 1]) << 8) |
                   ((unsigned)resample_clip8(acc[4 * d + 2]) << 16) | ((unsigned)resample_clip8(acc[4 * d + 3]) << 24);
        *reinterpret_cast<uint4*>(out + j * RS_ROWB + g * 16) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

}  // namespace dyt

using namespace dyt;

static unsigned long long rs_addr(const void* p) { return (unsigned long long)reinterpret_cast<uintptr_t>(p); }

extern "C" int64_t dyt_resample_scratch_bytes(int batch) { return resample_scratch_bytes(batch); }

extern "C" int dyt_resample_u8(const uint8_t* src, int batch, int src_h, int src_w, uint8_t* dst, const void* table_dev, int capacity,
                               void* scratch_dev, int64_t scratch_bytes, void* stream) {
    if (const char* e = resample_ptr_error(rs_addr(src), rs_addr(dst), rs_addr(table_dev), rs_addr(scratch_dev))) { set_error("dyt_resample_u8: %s", e); return DYT_ERR_ARG; }
    if (const char* e = resample_shape_error(batch, src_h, src_w, capacity)) {
        set_error("dyt_resample_u8: %s (batch %d, source %d x %d, table capacity %d)", e, batch, src_h, src_w, capacity);
        return DYT_ERR_ARG;
    }
    if (const char* e = resample_scratch_error(batch, scratch_bytes)) {
        set_error("dyt_resample_u8: %s (%lld bytes given, %lld needed)", e, (long long)scratch_bytes, resample_scratch_bytes(batch));
        return DYT_ERR_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int* table = static_cast<const int*>(table_dev);
    int* coeffs = static_cast<int*>(scratch_dev);
    hipLaunchKernelGGL(resample_coeff_kernel, dim3(2, (unsigned)batch), dim3(256), 0, s, table, capacity, src_h, src_w, 0, coeffs);
    DYT_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(resample_band_kernel, dim3(RS_OUT / 16, (unsigned)batch), dim3(256), 0, s, src, src_h, src_w, dst, table, capacity,
                       (const int*)coeffs);
    DYT_HIP_CHECK(hipGetLastError());
    return DYT_OK;
}

extern "C" int dyt_resample_coeffs(const void* table_dev, int capacity, int row, int src_h, int src_w, int32_t* out_dev, void* stream) {
    if (const char* e = resample_ptr_error(16, rs_addr(out_dev), rs_addr(table_dev), 16)) { set_error("dyt_resample_coeffs: %s", e); return DYT_ERR_ARG; }
    if (const char* e = resample_shape_error(1, src_h, src_w, capacity)) { set_error("dyt_resample_coeffs: %s", e); return DYT_ERR_ARG; }
    if (row < 0 || row >= capacity) { set_error("dyt_resample_coeffs: row %d is outside the table's %d rows", row, capacity); return DYT_ERR_ARG; }
    hipLaunchKernelGGL(resample_coeff_kernel, dim3(2, 1), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const int*>(table_dev),
                       capacity, src_h, src_w, row, out_dev);
    DYT_HIP_CHECK(hipGetLastError());
    return DYT_OK;
}
