// RandAugment on the device for byte clips and images: two context-free entries (dyt_randaug_u8, dyt_randaug_table).  The table layout, the
// row check, the table builders, the blend, the SMOOTH filter, the affine gather and every argument check are randaug.h.
//
//   randaug_stats_kernel         per (unit, frame) the R, G, B histograms (AutoContrast, Equalize) or the L histogram (Contrast) of the valid
//                                region of the layer's input: counted in LDS per block, combined with integer adds -- the sums do not
//                                depend on the schedule.  Launched for a layer only when its launch mask says some row needs it.
//   randaug_apply_kernel<FAM>    one instantiation per operation family: table operations (a 3 x 256 table built in the prologue with the
//                                header's function, from the histograms where the operation needs them), blends against a per-pixel or
//                                per-frame degenerate value, Sharpness with its 3 x 3 neighbourhood, Affine with its gather (taps read
//                                through the cache).  One block per (2048 pixels of the padded frame, frame, unit); the block reads ITS
//                                unit's rows, validates them and leaves at once when the unit's operation of this layer is another family's.
//   randaug_table_kernel         the table / the Contrast constant of one (unit, frame, layer), for tests
//
// Source, destination and work buffer are uint8 [units, frames, Hs, Ws, 3].  Layers run one after another on the stream; each row names the
// buffer it reads and the one it writes (the host knows every unit's sequence): layer 0 reads the source, pixel-local operations may work
// in place, Sharpness and Affine never write what they read, the last layer writes dst.  Every launch carries the padded frame across, so
// bytes outside a unit's valid h x w arrive in dst unchanged.  Nothing of a row is used before aug_row_ok has seen it; a unit with an invalid
// row in ANY layer, a broken buffer sequence or no row is written as zeros (by the table instantiation of the last layer, which is always
// launched, last).  One writer per byte, no float atomics; fp64 only in Affine and the table builders.  The same code in both builds.
#include "../../include/dyt_hip.h"
#include "dyt_common.h"
#include "randaug.h"

namespace dyt {

namespace {

constexpr int AUG_PIX = 8;                       // pixels per thread
constexpr int AUG_BLOCK_PIX = 256 * AUG_PIX;     // pixels of the padded frame per block

struct AugArgs {
    const uint8_t* src;
    uint8_t* dst;
    uint8_t* work;
    int* stats;
    const int* table;
    int units, frames, Hs, Ws, capacity, layers, layer;
};

__device__ __forceinline__ AugRow aug_read_row(const int* table, long long at) {
    const int4* q = reinterpret_cast<const int4*>(table + at);
    int4 w[5] = {q[0], q[1], q[2], q[3], q[4]};
    AugRow r;
    __builtin_memcpy(&r, w, sizeof(AugRow));
    return r;
}

// false: unit u has no valid sequence of rows and is written as zeros.  `row` = its row of layer a.layer.
__device__ __forceinline__ bool aug_load_unit(const AugArgs& a, int u, AugRow& row) {
    const int4 h = *reinterpret_cast<const int4*>(a.table);
    if (h.x != AUG_MAGIC || h.z != a.layers || u >= a.units) return false;
    AugRow prev;
    for (int l = 0; l < a.layers; ++l) {
        const long long at = aug_row_at(l, u, a.layers, h.y, a.capacity);
        if (at < 0) return false;
        const AugRow r = aug_read_row(a.table, at);
        if (!aug_row_ok(r, l, a.Hs, a.Ws)) return false;
        if (l > 0 && !aug_link_ok(prev, r)) return false;
        if (l == a.layers - 1 && !aug_last_ok(r)) return false;
        if (l == a.layer) row = r;
        prev = r;
    }
    return true;
}

__device__ __forceinline__ const uint8_t* aug_rd(const AugArgs& a, int id) { return id == AUG_BUF_SRC ? a.src : (id == AUG_BUF_DST ? a.dst : a.work); }
__device__ __forceinline__ uint8_t* aug_wr(const AugArgs& a, int id) { return id == AUG_BUF_DST ? a.dst : a.work; }

}  // namespace

__global__ __launch_bounds__(256) void randaug_stats_kernel(AugArgs a) {
    __shared__ int hist[AUG_HIST_WORDS];
    const int tid = threadIdx.x, uf = blockIdx.y, u = uf / a.frames;
    AugRow row;
    if (!aug_load_unit(a, u, row) || !aug_needs_stats(row.op)) return;   // uniform over the block
    const int npix = row.h * row.w, p0 = blockIdx.x * AUG_BLOCK_PIX;     // the VALID region, row-major
    if (p0 >= npix) return;
    for (int i = tid; i < AUG_HIST_WORDS; i += 256) hist[i] = 0;
    __syncthreads();
    const uint8_t* in = aug_rd(a, aug_row_src(row)) + (size_t)uf * a.Hs * a.Ws * 3;
    const bool luma = row.op == AUG_CONTRAST;
    for (int k = 0; k < AUG_PIX; ++k) {
        const int p = p0 + k * 256 + tid;
        if (p < npix) {
            const int y = p / row.w, x = p - y * row.w;
            const uint8_t* q = in + ((size_t)y * a.Ws + x) * 3;
            const int r = q[0], g = q[1], b = q[2];
            if (luma) {
                atomicAdd(&hist[768 + aug_luma(r, g, b)], 1);
            } else {
                atomicAdd(&hist[r], 1);
                atomicAdd(&hist[256 + g], 1);
                atomicAdd(&hist[512 + b], 1);
            }
        }
    }
    __syncthreads();
    int* out = a.stats + (size_t)uf * AUG_HIST_WORDS;
    for (int i = tid; i < AUG_HIST_WORDS; i += 256)
        if (hist[i] != 0) atomicAdd(&out[i], hist[i]);
}

template <int FAM>
__global__ __launch_bounds__(256) void randaug_apply_kernel(AugArgs a) {
    __shared__ uint8_t lut[3 * 256];
    __shared__ int mean_l;
    const int tid = threadIdx.x, uf = blockIdx.y, u = uf / a.frames;
    const int npix = a.Hs * a.Ws, p0 = blockIdx.x * AUG_BLOCK_PIX;       // the PADDED frame, row-major
    const size_t off = (size_t)uf * a.Hs * a.Ws * 3;
    AugRow row;
    if (!aug_load_unit(a, u, row)) {   // uniform over the block
        if (FAM == AUG_FAM_TABLE && a.layer == a.layers - 1) {
            const int end = (p0 + AUG_BLOCK_PIX < npix ? p0 + AUG_BLOCK_PIX : npix) * 3;
            for (int i = p0 * 3 + tid; i < end; i += 256) a.dst[off + i] = 0;
        }
        return;
    }
    if (aug_family(row.op) != FAM) return;
    const uint8_t* in = aug_rd(a, aug_row_src(row)) + off;
    uint8_t* out = aug_wr(a, aug_row_dst(row)) + off;
    const bool inplace = in == out;
    const int h = row.h, w = row.w, Ws = a.Ws;
    const int* hist = a.stats + (size_t)uf * AUG_HIST_WORDS;
    if (FAM == AUG_FAM_TABLE) {
        if (row.op == AUG_IDENTITY && inplace) return;
        if (tid < 3) aug_build_table(row.op, row.iarg, hist + tid * 256, lut + tid * 256);
        __syncthreads();
    }
    if (FAM == AUG_FAM_BLEND) {
        if (tid == 0) mean_l = row.op == AUG_CONTRAST ? aug_contrast_mean(hist + 768) : 0;
        __syncthreads();
    }
    for (int k = 0; k < AUG_PIX; ++k) {
        const int p = p0 + k * 256 + tid;
        if (p >= npix) break;
        const int y = p / Ws, x = p - y * Ws;
        const size_t at = (size_t)p * 3;
        const int v0 = in[at], v1 = in[at + 1], v2 = in[at + 2];
        if (y >= h || x >= w) {   // the loader's padding travels unchanged
            if (!inplace) { out[at] = (uint8_t)v0; out[at + 1] = (uint8_t)v1; out[at + 2] = (uint8_t)v2; }
            continue;
        }
        uint8_t o[3];
        if (FAM == AUG_FAM_TABLE) {
            o[0] = lut[v0]; o[1] = lut[256 + v1]; o[2] = lut[512 + v2];
        } else if (FAM == AUG_FAM_BLEND) {
            const int d = row.op == AUG_BRIGHTNESS ? 0 : (row.op == AUG_COLOR ? aug_luma(v0, v1, v2) : mean_l);
            o[0] = aug_blend(d, v0, row.factor); o[1] = aug_blend(d, v1, row.factor); o[2] = aug_blend(d, v2, row.factor);
        } else if (FAM == AUG_FAM_SHARP) {
            if (y >= 1 && y < h - 1 && x >= 1 && x < w - 1) {
                const uint8_t *ra = in + at - (size_t)Ws * 3 - 3, *rm = in + at - 3, *rb = in + at + (size_t)Ws * 3 - 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int qa[3] = {ra[c], ra[3 + c], ra[6 + c]}, qm[3] = {rm[c], rm[3 + c], rm[6 + c]}, qb[3] = {rb[c], rb[3 + c], rb[6 + c]};
                    o[c] = aug_blend(aug_smooth(qa, qm, qb), c == 0 ? v0 : (c == 1 ? v1 : v2), row.factor);
                }
            } else {   // SMOOTH copies the one-pixel border (and a frame with a side under 3)
                o[0] = aug_blend(v0, v0, row.factor); o[1] = aug_blend(v1, v1, row.factor); o[2] = aug_blend(v2, v2, row.factor);
            }
        } else {
            aug_affine_pixel(row.c, row.filter, row.fill, w, h, x, y, [in, Ws](int yy, int xx) { return in + ((size_t)yy * Ws + xx) * 3; }, o);
        }
        out[at] = o[0]; out[at + 1] = o[1]; out[at + 2] = o[2];
    }
}

__global__ __launch_bounds__(256) void randaug_table_kernel(AugArgs a, int unit, int frame, int* __restrict__ out) {
    __shared__ uint8_t lut[3 * 256];
    const int tid = threadIdx.x;
    AugRow row;
    const bool ok = aug_load_unit(a, unit, row);
    const int* hist = a.stats + ((size_t)unit * a.frames + frame) * AUG_HIST_WORDS;
    if (ok && tid < 3) {
        if (aug_family(row.op) == AUG_FAM_TABLE) aug_build_table(row.op, row.iarg, hist + tid * 256, lut + tid * 256);
        else aug_build_table(AUG_IDENTITY, 0, hist, lut + tid * 256);
    }
    __syncthreads();
    for (int i = tid; i < 3 * 256; i += 256) out[i] = ok ? (int)lut[i] : 0;
    if (tid == 0) out[3 * 256] = ok && row.op == AUG_CONTRAST ? aug_contrast_mean(hist + 768) : 0;
}

}  // namespace dyt

using namespace dyt;

static unsigned long long ra_addr(const void* p) { return (unsigned long long)reinterpret_cast<uintptr_t>(p); }

template <int FAM>
static void ra_launch(const AugArgs& a, dim3 grid, hipStream_t s) {
    hipLaunchKernelGGL(randaug_apply_kernel<FAM>, grid, dim3(256), 0, s, a);
}

static int ra_stats(const AugArgs& a, hipStream_t s) {
    DYT_HIP_CHECK(hipMemsetAsync(a.stats, 0, (size_t)a.units * a.frames * AUG_HIST_WORDS * sizeof(int), s));
    const dim3 grid((unsigned)((a.Hs * a.Ws + AUG_BLOCK_PIX - 1) / AUG_BLOCK_PIX), (unsigned)(a.units * a.frames));
    hipLaunchKernelGGL(randaug_stats_kernel, grid, dim3(256), 0, s, a);
    DYT_HIP_CHECK(hipGetLastError());
    return DYT_OK;
}

extern "C" int dyt_randaug_u8(const uint8_t* src, int units, int frames, int src_h, int src_w, uint8_t* dst, uint8_t* work, int32_t* stats,
                              const void* table_dev, int capacity, int layers, const uint32_t* launch_mask, void* stream) {
    if (const char* e = aug_ptr_error(ra_addr(src), ra_addr(dst), ra_addr(work), ra_addr(stats), ra_addr(table_dev))) {
        set_error("dyt_randaug_u8: %s", e);
        return DYT_ERR_ARG;
    }
    if (const char* e = aug_shape_error(units, frames, src_h, src_w, capacity, layers)) {
        set_error("dyt_randaug_u8: %s (units %d, frames %d, source %d x %d, table capacity %d, layers %d)", e, units, frames, src_h, src_w, capacity, layers);
        return DYT_ERR_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    AugArgs a{src, dst, work, stats, static_cast<const int*>(table_dev), units, frames, src_h, src_w, capacity, layers, 0};
    const dim3 grid((unsigned)((src_h * src_w + AUG_BLOCK_PIX - 1) / AUG_BLOCK_PIX), (unsigned)(units * frames));
    for (int l = 0; l < layers; ++l) {
        a.layer = l;
        unsigned m = launch_mask ? (launch_mask[l] & AUG_LAUNCH_ALL) : AUG_LAUNCH_ALL;
        if (l == layers - 1) m |= 1u << AUG_FAM_TABLE;   // it also writes the zeros of a unit without a valid sequence of rows
        if (m & AUG_LAUNCH_STATS)
            if (int rc = ra_stats(a, s)) return rc;
        if (m & (1u << AUG_FAM_BLEND)) ra_launch<AUG_FAM_BLEND>(a, grid, s);
        if (m & (1u << AUG_FAM_SHARP)) ra_launch<AUG_FAM_SHARP>(a, grid, s);
        if (m & (1u << AUG_FAM_AFFINE)) ra_launch<AUG_FAM_AFFINE>(a, grid, s);
        if (m & (1u << AUG_FAM_TABLE)) ra_launch<AUG_FAM_TABLE>(a, grid, s);
        DYT_HIP_CHECK(hipGetLastError());
    }
    return DYT_OK;
}

extern "C" int dyt_randaug_table(const uint8_t* src, int units, int frames, int src_h, int src_w, int32_t* stats, const void* table_dev,
                                 int capacity, int layers, int unit, int frame, int layer, int32_t* out_dev, void* stream) {
    if (const char* e = aug_ptr_error(ra_addr(src), ra_addr(out_dev), 16, ra_addr(stats), ra_addr(table_dev))) {
        set_error("dyt_randaug_table: %s", e);
        return DYT_ERR_ARG;
    }
    if (const char* e = aug_shape_error(units, frames, src_h, src_w, capacity, layers)) { set_error("dyt_randaug_table: %s", e); return DYT_ERR_ARG; }
    if (unit < 0 || unit >= units || frame < 0 || frame >= frames || layer < 0 || layer >= layers) {
        set_error("dyt_randaug_table: randaug: (unit %d, frame %d, layer %d) lies outside %d units, %d frames, %d layers", unit, frame, layer, units, frames, layers);
        return DYT_ERR_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t* in = const_cast<uint8_t*>(src);   // the layer's input, whatever buffer its row names: only read
    AugArgs a{src, in, in, stats, static_cast<const int*>(table_dev), units, frames, src_h, src_w, capacity, layers, layer};
    if (int rc = ra_stats(a, s)) return rc;
    hipLaunchKernelGGL(randaug_table_kernel, dim3(1), dim3(256), 0, s, a, unit, frame, out_dev);
    DYT_HIP_CHECK(hipGetLastError());
    return DYT_OK;
}
