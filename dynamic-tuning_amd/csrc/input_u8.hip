// Byte-image input: the entries and checks of uint8 batches normalised where the patch embedding loads them (DYT_F_IMAGES_U8,
// dyt_set_input_norm), and dyt_normalize_u8.  The kernel is image_load.hip's; the scalar formula and the argument checks are input_norm.h.
#include "ctx.h"
#include "image_items.h"

namespace dyt {

// the checks of a pass that takes `images` (dyt_forward, dyt_step_fwd_bwd): before anything is enqueued
int check_image_input(int flags, const void* images) {
    if (const char* e = input_flags_error(flags)) { set_error("%s", e); return DYT_ERR_ARG; }
    if (flags & DYT_F_IMAGES_U8)
        if (const char* e = input_ptr_error((unsigned long long)reinterpret_cast<uintptr_t>(images))) { set_error("%s", e); return DYT_ERR_ARG; }
    return 0;
}

}  // namespace dyt

extern "C" int dyt_set_input_norm(dyt_ctx* c, const float mean[3], const float std[3]) {
    if (!c) { set_error("null ctx"); return DYT_ERR_ARG; }
    if (const char* e = input_norm_error(mean, std)) { set_error("dyt_set_input_norm: %s", e); return DYT_ERR_ARG; }
    // host values only: they travel in the arguments of the launches enqueued from now on; a step in flight keeps the ones it was enqueued with
    for (int k = 0; k < 3; ++k) { c->in_norm.mean[k] = mean[k]; c->in_norm.std[k] = std[k]; }
    return DYT_OK;
}

extern "C" int dyt_normalize_u8(const uint8_t* src, float* dst, int batch, int nhwc, const float mean[3], const float std[3], void* stream) {
    if (!src || !dst || batch < 1) { set_error("dyt_normalize_u8: null pointer or batch < 1"); return DYT_ERR_ARG; }
    if (const char* e = input_norm_error(mean, std)) { set_error("dyt_normalize_u8: %s", e); return DYT_ERR_ARG; }
    if (const char* e = input_ptr_error((unsigned long long)reinterpret_cast<uintptr_t>(src))) { set_error("dyt_normalize_u8: %s", e); return DYT_ERR_ARG; }
    if (reinterpret_cast<uintptr_t>(dst) % 16 != 0) { set_error("dyt_normalize_u8: dst must be 16-byte aligned"); return DYT_ERR_ARG; }
    ImageLoadArgs a;
    a.src = src; a.src_kind = nhwc ? IMAGE_SRC_U8_NHWC : IMAGE_SRC_U8;
    a.dst = dst; a.dst_kind = IMAGE_DST_PLANES;
    a.batch = batch;
    for (int k = 0; k < 3; ++k) { a.norm.mean[k] = mean[k]; a.norm.std[k] = std[k]; }
    return launch_image_load(a, static_cast<hipStream_t>(stream));
}
