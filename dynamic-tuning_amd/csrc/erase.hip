// On-device Random Erasing, fused into the patch-embedding load (dyt_set_erase) and as a context-free entry (dyt_erase_images).  The table
// layout, the box test, the noise and every argument check are erase.h.
//
//   im2col_erase_kernel<AT>            fp32 [B,3,224,224] -> the EPI_EMBED GEMM's A operand: im2col_kernel's work items (4 pixels of one image
//                                      row, one 16-byte load) and element order
//   im2col_erase_u8_kernel<AT, NHWC>   bytes -> the same operand: im2col_u8_kernel's work items (16 pixels of one image row) and its 3 x 256
//                                      LDS table; the values erased are the normalised ones
//   erase_images_kernel<KIND>          either input -> fp32 [B,3,224,224] (the analogue of mix_images_kernel)
//
// Erasing comes BEFORE the mix: with a MixParams block set, a thread erases its own run with its image's row, the partner's run with the
// partner's row, and then mixes the two with mix_run (mix_dev.h), so the partner's erased pixels are what gets blended or cut in.
// Every kernel reads the table from DEVICE memory when it runs, so a captured step replays with whatever the table holds by then.  Nothing
// read from the table is used as an index or address: the row is chosen from the thread's own image number and checked against the
// `capacity` argument, the box count is clamped, boxes enter only through comparisons.  A run that no box meets costs the header, one word
// of the row (its count) or the whole row, and the comparisons; Philox runs only for groups of 4 pixels that a box meets.  A pixel's noise
// is keyed by (image, channel, row, column), so the three kernel forms write the same bits.  One writer per output element, no atomics.
#include "mix_dev.h"

namespace dyt {

#define LAUNCH_CHECK() DYT_HIP_CHECK(hipGetLastError())

namespace {

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
            float z[4];
            unpack(z, erase_noise4(h.seed, n, c, y, (x0 + g) >> 2));
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

// what every kernel below does with its run(s): own run erased; with a mix block, the partner's run erased with the partner's row, then mixed
struct EraseArgs { const int* table; int capacity; const MixParams* mix; };

}  // namespace

template <class AT>
__global__ __launch_bounds__(256) void im2col_erase_kernel(const float* __restrict__ img, AT* __restrict__ out, int batch, int frames, EraseArgs ea) {
    // out[(b*196 + py*14 + px)*768 + c*256 + i*16 + j]: im2col_kernel's work item, 4 consecutive j per thread
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t total = (size_t)batch * NP * (D / 4);
    if (idx >= total) return;
    const EraseCtl h = erase_ctl(ea.table);
    const int k4 = (int)(idx % (D / 4));
    const size_t row = idx / (D / 4);
    const int pt = (int)(row % NP);
    const int b = (int)(row / NP);
    const int k = k4 * 4, c = k >> 8, i = (k >> 4) & 15, j = k & 15;
    const int py = pt / GRID_P, px = pt - py * GRID_P;
    const int y = py * PS + i, x0 = px * PS + j;
    const size_t at = ((size_t)c * IMG + y) * IMG + x0;
    float v[4];
    unpack(v, *reinterpret_cast<const float4*>(img + (size_t)b * 3 * PLANE + at));
    erase_run(v, h, erase_code<4>(ea.table, h, b, frames, ea.capacity, y, x0), b, c, y, x0);
    if (ea.mix) {
        const MixParams p = *ea.mix;
        if (mix_run_needs_partner(p, y, x0, 4)) {
            const int pb = mix_partner(b, batch, frames);
            float w[4];
            unpack(w, *reinterpret_cast<const float4*>(img + (size_t)pb * 3 * PLANE + at));
            erase_run(w, h, erase_code<4>(ea.table, h, pb, frames, ea.capacity, y, x0), pb, c, y, x0);
            mix_run(v, w, p, y, x0);
        }
    }
    store4(out + row * D + k, v[0], v[1], v[2], v[3]);
}

template <class AT, bool NHWC>
__global__ __launch_bounds__(256) void im2col_erase_u8_kernel(const uint8_t* __restrict__ img, AT* __restrict__ out, int batch, int frames,
                                                              InputNorm nm, EraseArgs ea) {
    __shared__ float tab[3 * 256];
    build_table(tab, nm);
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t total = (size_t)batch * NP * PS * (NHWC ? 1 : 3);
    if (idx >= total) return;
    const EraseCtl h = erase_ctl(ea.table);
    MixParams p;
    p.mode = MIX_IDENTITY;
    if (ea.mix) p = *ea.mix;
    if (NHWC) {
        // work item = (b, patch, i): 48 contiguous bytes = 16 pixels x 3 channels -> three 16-element runs of the operand row
        const int i = (int)(idx % PS);
        const size_t row = idx / PS;                       // b * 196 + patch
        const int pt = (int)(row % NP);
        const int b = (int)(row / NP);
        const int py = pt / GRID_P, px = pt - py * GRID_P;
        const int y = py * PS + i, x0 = px * PS;
        const size_t at = ((size_t)y * IMG + x0) * 3;
        const uint4* src = reinterpret_cast<const uint4*>(img + (size_t)b * 3 * PLANE + at);
        const uint4 w[3] = {src[0], src[1], src[2]};
        const unsigned long long own = erase_code<16>(ea.table, h, b, frames, ea.capacity, y, x0);
        const bool need = mix_run_needs_partner(p, y, x0, 16);
        const int pb = mix_partner(b, batch, frames);
        uint4 q[3] = {w[0], w[1], w[2]};
        unsigned long long part = 0;
        if (need) {
            const uint4* ps = reinterpret_cast<const uint4*>(img + (size_t)pb * 3 * PLANE + at);
            q[0] = ps[0]; q[1] = ps[1]; q[2] = ps[2];
            part = erase_code<16>(ea.table, h, pb, frames, ea.capacity, y, x0);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v[16];
            lookup(v, tab, w, c);
            erase_run(v, h, own, b, c, y, x0);
            if (need) {
                float u[16];
                lookup(u, tab, q, c);
                erase_run(u, h, part, pb, c, y, x0);
                mix_run(v, u, p, y, x0);
            }
            store16(out + row * D + c * 256 + i * PS, v);
        }
    } else {
        // work item = (b, patch, c, i) = 16-element group idx of the operand: out + idx * 16
        const int i = (int)(idx % PS);
        const int c = (int)((idx / PS) % 3);
        const size_t row = idx / (3 * PS);
        const int pt = (int)(row % NP);
        const int b = (int)(row / NP);
        const int py = pt / GRID_P, px = pt - py * GRID_P;
        const int y = py * PS + i, x0 = px * PS;
        const size_t at = ((size_t)c * IMG + y) * IMG + x0;
        float v[16];
        lookup(v, tab, *reinterpret_cast<const uint4*>(img + (size_t)b * 3 * PLANE + at), c);
        erase_run(v, h, erase_code<16>(ea.table, h, b, frames, ea.capacity, y, x0), b, c, y, x0);
        if (mix_run_needs_partner(p, y, x0, 16)) {
            const int pb = mix_partner(b, batch, frames);
            float u[16];
            lookup(u, tab, *reinterpret_cast<const uint4*>(img + (size_t)pb * 3 * PLANE + at), c);
            erase_run(u, h, erase_code<16>(ea.table, h, pb, frames, ea.capacity, y, x0), pb, c, y, x0);
            mix_run(v, u, p, y, x0);
        }
        store16(out + idx * 16, v);
    }
}

// KIND 0: fp32 NCHW, 4 pixels per thread; 1: uint8 NCHW, 16 pixels per thread; 2: uint8 NHWC, 16 pixels x 3 channels per thread.  A row of
// 224 pixels is a whole number of either run, so a run never crosses a row.
template <int KIND>
__global__ __launch_bounds__(256) void erase_images_kernel(const void* __restrict__ src_, float* __restrict__ dst, int batch, int frames,
                                                           InputNorm nm, EraseArgs ea) {
    __shared__ float tab[KIND == 0 ? 1 : 3 * 256];
    if (KIND != 0) build_table(tab, nm);
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t total = KIND == 0 ? (size_t)batch * 3 * PLANE / 4 : (KIND == 1 ? (size_t)batch * 3 * PLANE / 16 : (size_t)batch * PLANE / 16);
    if (idx >= total) return;
    const EraseCtl h = erase_ctl(ea.table);
    MixParams p;
    p.mode = MIX_IDENTITY;
    if (ea.mix) p = *ea.mix;
    if (KIND == 0) {
        const float* src = static_cast<const float*>(src_);
        const int b = (int)(idx / (3 * PLANE / 4));
        const size_t at = (idx - (size_t)b * (3 * PLANE / 4)) * 4;       // element within the image
        const int c = (int)(at / PLANE), pix = (int)(at % PLANE), y = pix / IMG, x0 = pix - y * IMG;
        float v[4];
        unpack(v, *reinterpret_cast<const float4*>(src + (size_t)b * 3 * PLANE + at));
        erase_run(v, h, erase_code<4>(ea.table, h, b, frames, ea.capacity, y, x0), b, c, y, x0);
        if (mix_run_needs_partner(p, y, x0, 4)) {
            const int pb = mix_partner(b, batch, frames);
            float w[4];
            unpack(w, *reinterpret_cast<const float4*>(src + (size_t)pb * 3 * PLANE + at));
            erase_run(w, h, erase_code<4>(ea.table, h, pb, frames, ea.capacity, y, x0), pb, c, y, x0);
            mix_run(v, w, p, y, x0);
        }
        store4(dst + idx * 4, v[0], v[1], v[2], v[3]);
    } else if (KIND == 1) {
        const uint8_t* src = static_cast<const uint8_t*>(src_);
        const int b = (int)(idx / (3 * PLANE / 16));
        const size_t at = (idx - (size_t)b * (3 * PLANE / 16)) * 16;
        const int c = (int)(at / PLANE), pix = (int)(at - (size_t)c * PLANE), y = pix / IMG, x0 = pix - y * IMG;
        float v[16];
        lookup(v, tab, *reinterpret_cast<const uint4*>(src + (size_t)b * 3 * PLANE + at), c);
        erase_run(v, h, erase_code<16>(ea.table, h, b, frames, ea.capacity, y, x0), b, c, y, x0);
        if (mix_run_needs_partner(p, y, x0, 16)) {
            const int pb = mix_partner(b, batch, frames);
            float u[16];
            lookup(u, tab, *reinterpret_cast<const uint4*>(src + (size_t)pb * 3 * PLANE + at), c);
            erase_run(u, h, erase_code<16>(ea.table, h, pb, frames, ea.capacity, y, x0), pb, c, y, x0);
            mix_run(v, u, p, y, x0);
        }
        store16(dst + idx * 16, v);
    } else {
        const uint8_t* src = static_cast<const uint8_t*>(src_);
        const int b = (int)(idx / (PLANE / 16));
        const int q16 = (int)(idx - (size_t)b * (PLANE / 16));            // 16-pixel group within the image
        const int pix = q16 * 16, y = pix / IMG, x0 = pix - y * IMG;
        const uint4* s4 = reinterpret_cast<const uint4*>(src + (size_t)b * 3 * PLANE + (size_t)pix * 3);
        const uint4 w[3] = {s4[0], s4[1], s4[2]};
        const unsigned long long own = erase_code<16>(ea.table, h, b, frames, ea.capacity, y, x0);
        const bool need = mix_run_needs_partner(p, y, x0, 16);
        const int pb = mix_partner(b, batch, frames);
        uint4 q[3] = {w[0], w[1], w[2]};
        unsigned long long part = 0;
        if (need) {
            const uint4* ps = reinterpret_cast<const uint4*>(src + (size_t)pb * 3 * PLANE + (size_t)pix * 3);
            q[0] = ps[0]; q[1] = ps[1]; q[2] = ps[2];
            part = erase_code<16>(ea.table, h, pb, frames, ea.capacity, y, x0);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v[16];
            lookup(v, tab, w, c);
            erase_run(v, h, own, b, c, y, x0);
            if (need) {
                float u[16];
                lookup(u, tab, q, c);
                erase_run(u, h, part, pb, c, y, x0);
                mix_run(v, u, p, y, x0);
            }
            store16(dst + ((size_t)b * 3 + c) * PLANE + pix, v);
        }
    }
}

int launch_im2col_erase(int precision, const float* images, void* out, int batch, int frames, const void* table, int capacity,
                        const MixParams* mix, hipStream_t s) {
    const size_t total = (size_t)batch * NP * (D / 4);
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    const EraseArgs ea{static_cast<const int*>(table), capacity, mix};
    if (precision == 0) hipLaunchKernelGGL(im2col_erase_kernel<float>, grid, block, 0, s, images, (float*)out, batch, frames, ea);
    else hipLaunchKernelGGL(im2col_erase_kernel<bf16>, grid, block, 0, s, images, (bf16*)out, batch, frames, ea);
    LAUNCH_CHECK();
    return 0;
}

int launch_im2col_erase_u8(int precision, const uint8_t* images, int nhwc, const InputNorm& nm, void* out, int batch, int frames,
                           const void* table, int capacity, const MixParams* mix, hipStream_t s) {
    const size_t total = (size_t)batch * NP * PS * (nhwc ? 1 : 3);
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    const EraseArgs ea{static_cast<const int*>(table), capacity, mix};
    if (precision == 0) {
        if (nhwc) hipLaunchKernelGGL((im2col_erase_u8_kernel<float, true>), grid, block, 0, s, images, (float*)out, batch, frames, nm, ea);
        else hipLaunchKernelGGL((im2col_erase_u8_kernel<float, false>), grid, block, 0, s, images, (float*)out, batch, frames, nm, ea);
    } else {
        if (nhwc) hipLaunchKernelGGL((im2col_erase_u8_kernel<bf16, true>), grid, block, 0, s, images, (bf16*)out, batch, frames, nm, ea);
        else hipLaunchKernelGGL((im2col_erase_u8_kernel<bf16, false>), grid, block, 0, s, images, (bf16*)out, batch, frames, nm, ea);
    }
    LAUNCH_CHECK();
    return 0;
}

int launch_erase_images(const void* src, float* dst, int count, int frames, int src_kind, const InputNorm& nm, const void* table, int capacity,
                        const MixParams* mix, hipStream_t s) {
    const size_t total = src_kind == 0 ? (size_t)count * 3 * PLANE / 4 : (src_kind == 1 ? (size_t)count * 3 * PLANE / 16 : (size_t)count * PLANE / 16);
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    const EraseArgs ea{static_cast<const int*>(table), capacity, mix};
    if (src_kind == 0) hipLaunchKernelGGL(erase_images_kernel<0>, grid, block, 0, s, src, dst, count, frames, nm, ea);
    else if (src_kind == 1) hipLaunchKernelGGL(erase_images_kernel<1>, grid, block, 0, s, src, dst, count, frames, nm, ea);
    else hipLaunchKernelGGL(erase_images_kernel<2>, grid, block, 0, s, src, dst, count, frames, nm, ea);
    LAUNCH_CHECK();
    return 0;
}

// the check of a pass that runs while erasing is on (dyt_forward, dyt_step_fwd_bwd): before anything is enqueued
int check_erase_batch(const dyt_ctx* c, int batch) {
    if (!c->erase_table) return 0;
    if (const char* e = erase_capacity_error(c->erase_capacity, batch, c->erase_frames)) {
        set_error("%s (batch %d, frames %d, table capacity %d)", e, batch, c->erase_frames, c->erase_capacity);
        return DYT_ERR_ARG;
    }
    return 0;
}

}  // namespace dyt

extern "C" int dyt_set_erase(dyt_ctx* c, const void* table_dev, int units_capacity, int frames) {
    if (!c) { set_error("null ctx"); return DYT_ERR_ARG; }
    if (!table_dev) { c->erase_table = nullptr; return DYT_OK; }   // off: the passes enqueued from now on launch the former kernels again
    { int rc = refuse_inference(c, "dyt_set_erase"); if (rc) return rc; }
    if (const char* e = erase_table_ptr_error((unsigned long long)reinterpret_cast<uintptr_t>(table_dev))) { set_error("dyt_set_erase: %s", e); return DYT_ERR_ARG; }
    if (frames != c->frames) { set_error("dyt_set_erase: frames = %d, the context folds %d frame(s) per clip", frames, c->frames); return DYT_ERR_ARG; }
    if (units_capacity < 1) { set_error("dyt_set_erase: units_capacity = %d (the rows the table's allocation holds)", units_capacity); return DYT_ERR_ARG; }
    c->erase_table = table_dev;
    c->erase_capacity = units_capacity;
    c->erase_frames = frames;
    return DYT_OK;
}

extern "C" int dyt_erase_images(const void* src, float* dst, int count, int frames, int src_kind, const float mean[3], const float std[3],
                                const void* table_dev, const void* mix_params_dev, void* stream) {
    if (!src || !dst) { set_error("dyt_erase_images: null pointer"); return DYT_ERR_ARG; }
    if (const char* e = erase_capacity_error(count, count, frames)) { set_error("dyt_erase_images: %s", e); return DYT_ERR_ARG; }
    if (const char* e = erase_src_error(src_kind, (unsigned long long)reinterpret_cast<uintptr_t>(src), (unsigned long long)reinterpret_cast<uintptr_t>(dst))) {
        set_error("dyt_erase_images: %s", e);
        return DYT_ERR_ARG;
    }
    if (const char* e = erase_table_ptr_error((unsigned long long)reinterpret_cast<uintptr_t>(table_dev))) { set_error("dyt_erase_images: %s", e); return DYT_ERR_ARG; }
    if (mix_params_dev) {
        if (const char* e = mix_count_error(count, frames)) { set_error("dyt_erase_images: %s", e); return DYT_ERR_ARG; }
        if (const char* e = mix_params_ptr_error((unsigned long long)reinterpret_cast<uintptr_t>(mix_params_dev))) { set_error("dyt_erase_images: %s", e); return DYT_ERR_ARG; }
    }
    InputNorm nm = IN_NORM_IMAGENET;
    if (src_kind != 0) {   // float images are erased as they are: mean / std may be null
        if (const char* e = input_norm_error(mean, std)) { set_error("dyt_erase_images: %s", e); return DYT_ERR_ARG; }
        for (int k = 0; k < 3; ++k) { nm.mean[k] = mean[k]; nm.std[k] = std[k]; }
    }
    // the table holds a row for every image of the batch (`count` rows at least): that is the caller's side of the contract
    return launch_erase_images(src, dst, count, frames, src_kind, nm, table_dev, count, static_cast<const MixParams*>(mix_params_dev),
                               static_cast<hipStream_t>(stream));
}
