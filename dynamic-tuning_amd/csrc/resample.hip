// Device RandomResizedCrop / flip / Resize + CenterCrop from byte sources: three context-free entries (dyt_resample_u8,
// dyt_resample_scratch_bytes, dyt_resample_coeffs).  The table layout, the row check, the coefficient function and every argument check
// are resample.h; the device pieces shared with the other two routes (row loader, tap range, accumulate and pack, zero fill, the
// coefficient kernel) are resample_dev.h.
//
//   resample_coeff_kernel<11>   resample_dev.h's: first tap, tap count and 11 coefficients per window position into the scratch buffer
//   resample_band_kernel        one block per (band of 16 output rows, image): the horizontal pass over the source rows the band's vertical
//                               taps need (at most 48) into LDS as bytes, then the vertical pass out of LDS, 16 bytes per work item and store
//
// Source uint8 [B, Hs, Ws, 3] (padded; an image's valid extent is its row's src_h x src_w), destination uint8 [B, 224, 224, 3].  The
// arithmetic of both passes is Pillow's: int32, ss = 2^21 + sum(pixel * k), clamp(ss >> 22, 0, 255); the horizontal pass rounds to uint8.
// The mirror is applied where the horizontal pass stores into LDS, so the vertical pass and the global stores stay 16-byte runs.
// Every kernel reads the table from DEVICE memory when it runs, so a captured graph replays with whatever the table holds by then.
// Nothing read from the table is used as an index before resample_row_ok has compared it (64-bit) against the batch's shape; the
// coefficient bounds read back from scratch are clamped against the box again.  An image whose row fails the check is written as zeros.
// One writer per byte, no atomics, no floating point in the pixel passes.  The same code in both builds of the library.
#include "resample_dev.h"

namespace dyt {

namespace {

constexpr int RS_MAXROWS = 48;              // source rows one band's vertical taps span: 15 * 2.5 + 2 * 5 + 1 (truncation), rounded down

// false: image b has no valid row (filter, units, capacity, resample_row_ok) and is written as zeros
__device__ __forceinline__ bool load_row(const int* __restrict__ table, int b, int capacity, int Hs, int Ws, ResampleRow& r) {
    return resample_load_row(table, RS_BICUBIC, b, capacity, r) && resample_row_ok(r, Hs, Ws);
}

}  // namespace

__global__ __launch_bounds__(256) void resample_band_kernel(const uint8_t* __restrict__ src, int Hs, int Ws, uint8_t* __restrict__ dst,
                                                            const int* __restrict__ table, int capacity, const int* __restrict__ coeffs) {
    __shared__ __attribute__((aligned(16))) uint8_t tmp[RS_MAXROWS * RS_ROWB];   // horizontally resampled source rows, window columns (mirrored if asked)
    __shared__ int hc[RS_COEFF_FIELDS * RS_OUT];                                  // column coefficients [field][224]
    __shared__ int vc[RS_COEFF_FIELDS * RS_BAND];                                 // row coefficients of this band [field][16]
    const int b = blockIdx.y, oy0 = blockIdx.x * RS_BAND, tid = threadIdx.x;
    uint8_t* out = dst + ((size_t)b * RS_OUT + oy0) * RS_ROWB;
    ResampleRow row;
    if (!load_row(table, b, capacity, Hs, Ws, row)) {   // uniform over the block
        resample_zero_band(out, tid);
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
        int lo, n;
        resample_tap_range<RS_KMAX>(vc[j], vc[RS_BAND + j], row.box_h, lo, n);
        r0 = min(r0, lo);
        r1 = max(r1, lo + n);
    }
    const int nrows = resample_clampi(r1 - r0, 0, RS_MAXROWS);
    const bool mirror = (row.flags & RS_FLAG_MIRROR) != 0;
    const uint8_t* base = src + (((size_t)b * Hs + row.top + r0) * Ws + row.left) * 3;
    for (int idx = tid; idx < nrows * RS_OUT; idx += 256) {
        const int r = idx / RS_OUT, ox = idx - r * RS_OUT;
        int lo, n;
        resample_tap_range<RS_KMAX>(hc[ox], hc[RS_OUT + ox], row.box_w, lo, n);
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
        int lo, n, acc[16];
        resample_tap_range<RS_KMAX>(vc[j], vc[RS_BAND + j], row.box_h, lo, n);
        resample_acc_start(acc);
#pragma unroll
        for (int x = 0; x < RS_KMAX; ++x) {
            const int rr = lo - r0 + x;
            if (x < n && rr < nrows) resample_acc_add(acc, *reinterpret_cast<const uint4*>(tmp + rr * RS_ROWB + g * 16), vc[(2 + x) * RS_BAND + j]);
        }
        *reinterpret_cast<uint4*>(out + j * RS_ROWB + g * 16) = resample_acc_pack(acc);
    }
}

}  // namespace dyt

using namespace dyt;

extern "C" int64_t dyt_resample_scratch_bytes(int batch) { return resample_scratch_bytes(batch); }

extern "C" int dyt_resample_u8(const uint8_t* src, int batch, int src_h, int src_w, uint8_t* dst, const void* table_dev, int capacity,
                               void* scratch_dev, int64_t scratch_bytes, void* stream) {
    if (const char* e = resample_ptr_error(resample_addr(src), resample_addr(dst), resample_addr(table_dev), resample_addr(scratch_dev))) { set_error("dyt_resample_u8: %s", e); return DYT_ERR_ARG; }
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
    hipLaunchKernelGGL(resample_coeff_kernel<RS_KMAX>, dim3(2, (unsigned)batch), dim3(256), 0, s, table, capacity, src_h, src_w, 0, coeffs);
    DYT_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(resample_band_kernel, dim3(RS_OUT / 16, (unsigned)batch), dim3(256), 0, s, src, src_h, src_w, dst, table, capacity,
                       (const int*)coeffs);
    DYT_HIP_CHECK(hipGetLastError());
    return DYT_OK;
}

extern "C" int dyt_resample_coeffs(const void* table_dev, int capacity, int row, int src_h, int src_w, int32_t* out_dev, void* stream) {
    if (resample_coeffs_refusal("dyt_resample_coeffs", resample_ptr_error(16, resample_addr(out_dev), resample_addr(table_dev), 16),
                                resample_shape_error(1, src_h, src_w, capacity), row, capacity)) return DYT_ERR_ARG;
    hipLaunchKernelGGL(resample_coeff_kernel<RS_KMAX>, dim3(2, 1), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const int*>(table_dev),
                       capacity, src_h, src_w, row, out_dev);
    DYT_HIP_CHECK(hipGetLastError());
    return DYT_OK;
}
