// Device crop / resize at any downscale: three context-free entries (dyt_resample_wide_u8, dyt_resample_wide_scratch_bytes,
// dyt_resample_wide_coeffs) beside the 11-tap route of resample.hip.  The table layout, the filter and the coefficient template are
// resample.h; the row check without the 2.5 bound, the tap bound and every argument check are resample_wide.h; the device pieces shared
// with the other two routes (row loader, tap range, staging, accumulate and guarded pack, zero fill, the coefficient kernel) are
// resample_dev.h.
//
//   resample_coeff_kernel<75>    resample_dev.h's: first tap, tap count and 75 coefficients per window position into the scratch buffer
//   resample_wide_h_kernel       one block per (4 source rows, image): the box segment of each row that the window's vertical taps need is
//                                staged in LDS with aligned 16-byte loads; work item ox forms output pixel ox of all 4 rows, reading each
//                                coefficient once, and stores the bytes (mirrored if asked) to tmp[image][source row][672] in scratch
//   resample_wide_v_kernel       one block per (band of 16 output rows, image): each work item owns 16 output bytes and walks the `count`
//                                rows of tmp its position needs with 16-byte loads
//
// Source uint8 [B, Hs, Ws, 3] (padded; an image's valid extent is its row's src_h x src_w), destination uint8 [B, 224, 224, 3].  The
// arithmetic of both passes is Pillow's: int32, ss = 2^21 + sum(pixel * k), clamp(ss >> 22, 0, 255); the horizontal pass rounds to uint8
// before the vertical pass reads it.  2^21 + 255 * sum|k| stays below 2^31 for every scale up to 4096 / 224, so int32 never wraps.
// Every kernel reads the table from DEVICE memory when it runs, and the three grids depend on (batch, Hs, Ws) alone, so a captured
// graph replays with whatever the table holds by then.  Nothing read from the table is used as an index before resample_wide_row_ok has
// compared it (64-bit) against the batch's shape; the coefficient bounds read back from scratch are clamped against the box again.  An
// image whose row fails the check is written as zeros.  One writer per byte, no atomics, no floating point in the pixel passes.  The
// 16-byte loads that stage a row may take in bytes beside the box (never beyond the source allocation); no output depends on them.
#include "resample_dev.h"
#include "resample_wide.h"

namespace dyt {

namespace {

constexpr int RSW_HROWS = 4;                // source rows per block of the horizontal pass
static_assert(RSW_ROW_BYTES == RS_ROWB, "a row of tmp is a 224-pixel byte row");
constexpr int RSW_FIELD_WORDS = RSW_COEFF_FIELDS * RS_OUT;   // one axis of one image

// bytes of LDS one staged row takes: the widest box segment, the bytes in front of it down to a 16-byte boundary and behind it up to one
__host__ __device__ inline int rsw_lds_stride(int Ws) { return ((Ws * 3 + 15) & ~15) + 32; }

// false: image b has no valid row (filter, units, capacity, resample_wide_row_ok) and is written as zeros
__device__ __forceinline__ bool load_row(const int* __restrict__ table, int b, int capacity, int Hs, int Ws, ResampleRow& r) {
    return resample_load_row(table, RS_BICUBIC, b, capacity, r) && resample_wide_row_ok(r, Hs, Ws);
}

}  // namespace

// grid (ceil(Hs / RSW_HROWS), B), 256 work items, rsw_lds_stride(Ws) * RSW_HROWS bytes of dynamic LDS
__global__ __launch_bounds__(256) void resample_wide_h_kernel(const uint8_t* __restrict__ src, int Hs, int Ws, long long src_bytes,
                                                              const int* __restrict__ table, int capacity, const int* __restrict__ coeffs,
                                                              uint8_t* __restrict__ tmp) {
    extern __shared__ __attribute__((aligned(16))) uint8_t seg[];   // [RSW_HROWS][stride]: the rows' box segments from a 16-byte boundary on
    const int b = blockIdx.y, tid = threadIdx.x;
    ResampleRow row;
    if (!load_row(table, b, capacity, Hs, Ws, row)) return;     // uniform over the block; the vertical pass writes the zeros
    const int* vc = coeffs + (size_t)b * RSW_COEFF_WORDS;
    const int* hc = vc + RSW_FIELD_WORDS;
    // the source rows (relative to the box) the window's vertical taps read: the first position's first tap to the last position's last
    // (both bounds grow with the position).  Bounds from scratch are clamped against the box again.
    const int lo_a = resample_clampi(vc[0], 0, row.box_h - 1);
    int lo_z, n_z;
    resample_tap_range<RSW_KMAX>(vc[RS_OUT - 1], vc[RS_OUT + RS_OUT - 1], row.box_h, lo_z, n_z);
    const int y0 = max(row.top + lo_a, (int)blockIdx.x * RSW_HROWS);                    // absolute source rows [y0, y1) of this block
    const int y1 = min(row.top + lo_z + n_z, (int)blockIdx.x * RSW_HROWS + RSW_HROWS);
    const int nr = y1 - y0;
    if (nr <= 0) return;                                                                // rows outside the box or the needed range
    const int stride = rsw_lds_stride(Ws);
    int head[RSW_HROWS];                                                                // bytes in front of the segment in the row's LDS
#pragma unroll
    for (int r = 0; r < RSW_HROWS; ++r) {
        head[r] = 0;
        if (r < nr)                                                                     // (first < src_bytes: the box lies inside the batch)
            head[r] = resample_stage_row(src, src_bytes, (((long long)b * Hs + y0 + r) * Ws + row.left) * 3, row.box_w * 3, seg + r * stride,
                                         stride / 16, tid);
    }
    __syncthreads();
    if (tid >= RS_OUT) return;
    const int ox = tid;
    int lo, n;
    resample_tap_range<RSW_KMAX>(hc[ox], hc[RS_OUT + ox], row.box_w, lo, n);
    int acc[RSW_HROWS][3];
    const uint8_t* p[RSW_HROWS];
#pragma unroll
    for (int r = 0; r < RSW_HROWS; ++r) {
        acc[r][0] = acc[r][1] = acc[r][2] = 1 << (RS_PRECISION_BITS - 1);
        p[r] = seg + r * stride + head[r] + lo * 3;
    }
    for (int x = 0; x < n; ++x) {
        const int k = hc[(2 + x) * RS_OUT + ox];
#pragma unroll
        for (int r = 0; r < RSW_HROWS; ++r) {
            if (r < nr) {
                acc[r][0] += (int)p[r][3 * x] * k;
                acc[r][1] += (int)p[r][3 * x + 1] * k;
                acc[r][2] += (int)p[r][3 * x + 2] * k;
            }
        }
    }
    const int col = (row.flags & RS_FLAG_MIRROR) ? RS_OUT - 1 - ox : ox;
#pragma unroll
    for (int r = 0; r < RSW_HROWS; ++r) {
        if (r < nr) {
            uint8_t* q = tmp + ((size_t)b * Hs + y0 + r) * RSW_ROW_BYTES + col * 3;
            q[0] = (uint8_t)resample_clip8(acc[r][0]);
            q[1] = (uint8_t)resample_clip8(acc[r][1]);
            q[2] = (uint8_t)resample_clip8(acc[r][2]);
        }
    }
}

// grid (224 / RS_BAND, B), 256 work items
__global__ __launch_bounds__(256) void resample_wide_v_kernel(int Hs, int Ws, uint8_t* __restrict__ dst, const int* __restrict__ table,
                                                              int capacity, const int* __restrict__ coeffs, const uint8_t* __restrict__ tmp) {
    __shared__ int vc[RSW_COEFF_FIELDS * RS_BAND];   // row coefficients of this band [field][16]
    const int b = blockIdx.y, oy0 = blockIdx.x * RS_BAND, tid = threadIdx.x;
    uint8_t* out = dst + ((size_t)b * RS_OUT + oy0) * RSW_ROW_BYTES;
    ResampleRow row;
    if (!load_row(table, b, capacity, Hs, Ws, row)) {   // uniform over the block
        resample_zero_band(out, tid);
        return;
    }
    const int* cf = coeffs + (size_t)b * RSW_COEFF_WORDS;
    for (int i = tid; i < RSW_COEFF_FIELDS * RS_BAND; i += 256) {
        const int f = i / RS_BAND, j = i - f * RS_BAND;
        vc[i] = cf[f * RS_OUT + oy0 + j];
    }
    __syncthreads();
    const uint8_t* rows = tmp + ((size_t)b * Hs + row.top) * RSW_ROW_BYTES;   // the box's first row
    for (int idx = tid; idx < RS_BAND * RS_GROUPS; idx += 256) {
        const int j = idx / RS_GROUPS, g = idx - j * RS_GROUPS;
        int lo, n, acc[16];
        resample_tap_range<RSW_KMAX>(vc[j], vc[RS_BAND + j], row.box_h, lo, n);
        resample_acc_start(acc);
        const uint8_t* p = rows + (size_t)lo * RSW_ROW_BYTES + g * 16;
        for (int x = 0; x < n; ++x) resample_acc_add(acc, *reinterpret_cast<const uint4*>(p + (size_t)x * RSW_ROW_BYTES), vc[(2 + x) * RS_BAND + j]);
        *reinterpret_cast<uint4*>(out + j * RSW_ROW_BYTES + g * 16) = resample_acc_pack(acc);
    }
}

}  // namespace dyt

using namespace dyt;

extern "C" int64_t dyt_resample_wide_scratch_bytes(int batch, int src_h) { return resample_wide_scratch_bytes(batch, src_h); }

extern "C" int dyt_resample_wide_u8(const uint8_t* src, int batch, int src_h, int src_w, uint8_t* dst, const void* table_dev, int capacity,
                                    void* scratch_dev, int64_t scratch_bytes, void* stream) {
    if (const char* e = resample_wide_args_error(resample_addr(src), resample_addr(dst), resample_addr(table_dev), resample_addr(scratch_dev), batch, src_h, src_w,
                                                 capacity, scratch_bytes)) {
        set_error("dyt_resample_wide_u8: %s (batch %d, source %d x %d, table capacity %d, %lld scratch bytes given, %lld needed)", e, batch,
                  src_h, src_w, capacity, (long long)scratch_bytes, resample_wide_scratch_bytes(batch, src_h));
        return DYT_ERR_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int* table = static_cast<const int*>(table_dev);
    int* coeffs = static_cast<int*>(scratch_dev);
    uint8_t* tmp = static_cast<uint8_t*>(scratch_dev) + resample_wide_coeff_bytes(batch);
    const long long src_bytes = (long long)batch * src_h * src_w * 3;
    hipLaunchKernelGGL(resample_coeff_kernel<RSW_KMAX>, dim3(2, (unsigned)batch), dim3(256), 0, s, table, capacity, src_h, src_w, 0, coeffs);
    DYT_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(resample_wide_h_kernel, dim3((unsigned)((src_h + RSW_HROWS - 1) / RSW_HROWS), (unsigned)batch), dim3(256),
                       (size_t)rsw_lds_stride(src_w) * RSW_HROWS, s, src, src_h, src_w, src_bytes, table, capacity, (const int*)coeffs, tmp);
    DYT_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(resample_wide_v_kernel, dim3(RS_OUT / RS_BAND, (unsigned)batch), dim3(256), 0, s, src_h, src_w, dst, table, capacity,
                       (const int*)coeffs, (const uint8_t*)tmp);
    DYT_HIP_CHECK(hipGetLastError());
    return DYT_OK;
}

extern "C" int dyt_resample_wide_coeffs(const void* table_dev, int capacity, int row, int src_h, int src_w, int32_t* out_dev, void* stream) {
    if (resample_coeffs_refusal("dyt_resample_wide_coeffs", resample_ptr_error(16, resample_addr(out_dev), resample_addr(table_dev), 16),
                                resample_shape_error(1, src_h, src_w, capacity), row, capacity)) return DYT_ERR_ARG;
    hipLaunchKernelGGL(resample_coeff_kernel<RSW_KMAX>, dim3(2, 1), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const int*>(table_dev), capacity, src_h, src_w, row, out_dev);
    DYT_HIP_CHECK(hipGetLastError());
    return DYT_OK;
}
