// On-device Random Erasing: the entries and checks of the erasing fused into the patch-embedding load (dyt_set_erase) and of the
// context-free form (dyt_erase_images).  The kernel is image_load.hip's; the table layout, the box test, the noise and every argument
// check are erase.h.
#include "ctx.h"
#include "image_items.h"

namespace dyt {

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
    ImageLoadArgs a;
    a.src = src; a.src_kind = src_kind;
    a.dst = dst; a.dst_kind = IMAGE_DST_PLANES;
    a.batch = count; a.frames = frames;
    a.mix = static_cast<const MixParams*>(mix_params_dev);
    // the table holds a row for every image of the batch (`count` rows at least): that is the caller's side of the contract
    a.erase_table = table_dev; a.erase_capacity = count;
    if (src_kind != IMAGE_SRC_F32) {   // float images are erased as they are: mean / std may be null
        if (const char* e = input_norm_error(mean, std)) { set_error("dyt_erase_images: %s", e); return DYT_ERR_ARG; }
        for (int k = 0; k < 3; ++k) { a.norm.mean[k] = mean[k]; a.norm.std[k] = std[k]; }
    }
    return launch_image_load(a, static_cast<hipStream_t>(stream));
}
