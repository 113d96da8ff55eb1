// The image load in front of the patch-embedding GEMM, and its stand-alone forms (dyt_normalize_u8, dyt_mix_images, dyt_erase_images): one
// kernel template over the source kind, the destination and the transform, and its launcher.
//
//   image_load_kernel<KIND, DST, XFORM>   KIND:  fp32 [B,3,224,224] | uint8 [B,3,224,224] | uint8 [B,224,224,3]       (image_items.h)
//                                         DST:   the EPI_EMBED GEMM's A operand, fp32 or 16-bit | fp32 [B,3,224,224]
//                                         XFORM: none | Mixup / CutMix (mix.h) | Random Erasing, then the mix if a block is given (erase.h)
//
// A thread owns one run of an image row (image_items.h maps the work item; consecutive items store consecutive 16- or 64-byte groups, so
// a wave's stores are contiguous).  Bytes are normalised through input_norm_value (input_norm.h) evaluated once per (channel, byte
// value): every workgroup builds the 3 x 256 table in LDS (6 divisions per thread) and then looks its pixels up; the values mixed and
// erased are the normalised ones.
// The MixParams block and the erase table are read from DEVICE memory when the kernel runs, so the mode is a run-time value and a captured
// step replays with whatever they hold by then.  The partner's run is loaded only when the mix needs it: always for mixup, for cutmix only
// when the run's row lies in [yl, yh) and its columns meet [xl, xh), never for identity (whose output is a copy of the own pixels: -0.0,
// NaN and inf pass, nothing of the partner leaks in).  Erasing comes BEFORE the mix: a thread erases its own run with its image's row,
// the partner's run with the partner's row, and then mixes the two, so the partner's erased pixels are what gets blended or cut in.
// Nothing read from the block or the table is used as an index or address: the table row is chosen from the thread's own image number
// and checked against the `capacity` argument, the box count is clamped, boxes enter only through comparisons.  A run that no box meets
// costs the header, one word of the row (its count) or the whole row, and the comparisons; Philox runs only for groups of 4 pixels that
// a box meets.  A pixel's noise is keyed by (image, channel, row, column), so every form writes the same bits.  One writer per output
// element, no atomics.
#include "image_load_dev.h"

namespace dyt {

#define LAUNCH_CHECK() DYT_HIP_CHECK(hipGetLastError())

namespace {

constexpr int XF_NONE = 0, XF_MIX = 1, XF_ERASE = 2;
struct XformArgs { const int* table; int capacity; const MixParams* mix; };   // XF_MIX: mix; XF_ERASE: table, capacity and an optional mix

template <int DST> struct OutOf { typedef float type; };
template <> struct OutOf<IMAGE_DST_OPERAND_16> { typedef bf16 type; };

}  // namespace

template <int KIND, int DST, int XFORM>
__global__ __launch_bounds__(256) void image_load_kernel(const void* __restrict__ src_, void* __restrict__ dst_, int batch, int frames, InputNorm nm,
                                                         XformArgs xa) {
    typedef typename RunOf<KIND>::Elem Elem;
    typedef typename RunOf<KIND>::Raw Raw;
    constexpr int N = image_run(KIND);
    constexpr bool PLANES = DST == IMAGE_DST_PLANES;
    __shared__ float tab[KIND == IMAGE_SRC_F32 ? 1 : 3 * 256];
    if (KIND != IMAGE_SRC_F32) build_table(tab, nm);   // its barrier comes before any thread leaves
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= image_item_count(KIND, batch)) return;
    MixParams p;
    p.mode = MIX_IDENTITY;
    if (XFORM == XF_MIX || (XFORM == XF_ERASE && xa.mix)) p = *xa.mix;
    EraseCtl h = {};
    if (XFORM == XF_ERASE) h = erase_ctl(xa.table);
    const ImageItem it = image_item<KIND, PLANES>(idx);
    const Elem* src = static_cast<const Elem*>(src_) + it.src;
    typename OutOf<DST>::type* dst = static_cast<typename OutOf<DST>::type*>(dst_) + it.dst;

    // the own run; the partner's only when the mix needs it; the erase codes once for all channels
    const Raw own = *reinterpret_cast<const Raw*>(src + (size_t)it.b * 3 * PLANE);
    unsigned long long own_code = 0, part_code = 0;
    if (XFORM == XF_ERASE) own_code = erase_code<N>(xa.table, h, it.b, frames, xa.capacity, it.y, it.x0);
    const bool need = XFORM != XF_NONE && mix_run_needs_partner(p, it.y, it.x0, N);
    Raw part = own;
    int pb = it.b;
    if (need) {
        pb = mix_partner(it.b, batch, frames);
        if (XFORM == XF_ERASE) part_code = erase_code<N>(xa.table, h, pb, frames, xa.capacity, it.y, it.x0);
        part = *reinterpret_cast<const Raw*>(src + (size_t)pb * 3 * PLANE);
    }
#pragma unroll
    for (int k = 0; k < image_item_channels(KIND); ++k) {
        const int c = it.c + k;
        float v[N];
        run_values(v, tab, own, c);
        if (XFORM == XF_ERASE) erase_run(v, h, own_code, it.b, c, it.y, it.x0);
        if (need) {
            float u[N];
            run_values(u, tab, part, c);
            if (XFORM == XF_ERASE) erase_run(u, h, part_code, pb, c, it.y, it.x0);
            mix_run(v, u, p, it.y, it.x0);
        }
        store_run(dst + k * image_channel_stride(PLANES), v);
    }
}

namespace {

template <int KIND, int DST>
int launch_kind_dst(const ImageLoadArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)((image_item_count(KIND, a.batch) + 255) / 256)), block(256);
    const XformArgs xa{static_cast<const int*>(a.erase_table), a.erase_capacity, a.mix};
    if (a.erase_table) hipLaunchKernelGGL((image_load_kernel<KIND, DST, XF_ERASE>), grid, block, 0, s, a.src, a.dst, a.batch, a.frames, a.norm, xa);
    else if (a.mix) hipLaunchKernelGGL((image_load_kernel<KIND, DST, XF_MIX>), grid, block, 0, s, a.src, a.dst, a.batch, a.frames, a.norm, xa);
    else if constexpr (KIND == IMAGE_SRC_F32 && DST == IMAGE_DST_PLANES) { set_error("image load: fp32 images to fp32 planes with no transform is a copy"); return DYT_ERR_ARG; }
    else hipLaunchKernelGGL((image_load_kernel<KIND, DST, XF_NONE>), grid, block, 0, s, a.src, a.dst, a.batch, a.frames, a.norm, xa);
    LAUNCH_CHECK();
    return 0;
}

template <int KIND>
int launch_kind(const ImageLoadArgs& a, hipStream_t s) {
    switch (a.dst_kind) {
    case IMAGE_DST_OPERAND_F32: return launch_kind_dst<KIND, IMAGE_DST_OPERAND_F32>(a, s);
    case IMAGE_DST_OPERAND_16: return launch_kind_dst<KIND, IMAGE_DST_OPERAND_16>(a, s);
    case IMAGE_DST_PLANES: return launch_kind_dst<KIND, IMAGE_DST_PLANES>(a, s);
    }
    set_error("image load: dst_kind = %d", a.dst_kind);
    return DYT_ERR_ARG;
}

}  // namespace

int launch_image_load(const ImageLoadArgs& a, hipStream_t s) {
    switch (a.src_kind) {
    case IMAGE_SRC_F32: return launch_kind<IMAGE_SRC_F32>(a, s);
    case IMAGE_SRC_U8: return launch_kind<IMAGE_SRC_U8>(a, s);
    case IMAGE_SRC_U8_NHWC: return launch_kind<IMAGE_SRC_U8_NHWC>(a, s);
    }
    set_error("image load: src_kind = %d", a.src_kind);
    return DYT_ERR_ARG;
}

}  // namespace dyt
