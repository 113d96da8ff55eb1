// Device crop / resize at any downscale (dyt_resample_wide_u8, dyt_resample_wide_scratch_bytes, dyt_resample_wide_coeffs; kernels in
// resample_wide.hip): the wide-tap companion of resample.h.  The table (ResampleHeader / ResampleRow, filter word 3), the filter and the
// rounding are resample.h's; what differs is that a crop box may be ANY multiple of the size it is resized to, so a window position takes
// up to RSW_KMAX taps instead of 11, and the scratch buffer holds the horizontally resampled rows besides the coefficient tables.
// No HIP type is used here, so a host compiler reads this file on its own (tools/resample_wide_check.cpp walks it without a GPU).
#pragma once

#include "resample.h"

namespace dyt {

// Taps per output position.  A box side is at most RS_MAX_SIDE = 4096 and `full` at least RS_OUT = 224, so the scale is at most 18.29,
// the support 36.58, and (int)(center + support + 0.5) - (int)(center - support + 0.5) <= 74; Pillow's ksize = ceil(support) * 2 + 1 = 75.
constexpr int RSW_KMAX = 75;
constexpr int RSW_COEFF_FIELDS = 2 + RSW_KMAX;   // per output position: first tap, tap count, RSW_KMAX coefficients
constexpr int RSW_COEFF_WORDS = 2 * RSW_COEFF_FIELDS * RS_OUT;   // scratch words per image: [axis 0 = rows, 1 = columns][field][224]
constexpr int RSW_ROW_BYTES = RS_OUT * 3;        // one horizontally resampled source row: 224 pixels, 672 = 42 x 16 bytes
static_assert((RSW_COEFF_WORDS * 4) % 16 == 0 && RSW_ROW_BYTES % 16 == 0, "the parts of the scratch buffer stay 16-byte aligned");

// resample_row_ok without the 2.5 bound; a batch side above RS_MAX_SIDE is refused, which bounds the taps by RSW_KMAX.
DYT_RESAMPLE_HD inline bool resample_wide_row_ok(const ResampleRow& r, int batch_src_h, int batch_src_w) {
    return resample_row_ok_core(r, batch_src_h, batch_src_w, false);
}

// resample_coeffs with the wider array: for every (in, out, xx) the narrow function takes, xmin, count and the first RS_KMAX integers are
// its own, the rest 0 (both are resample.h's one template).
DYT_RESAMPLE_HD inline void resample_wide_coeffs(int in, int out, int xx, int& xmin, int& count, int (&k)[RSW_KMAX]) {
    resample_coeffs_taps<RSW_KMAX>(in, out, xx, xmin, count, k);
}

// ---- host side: each check returns the text of the refusal, or a null pointer -----------------------------------------------------------
// The scratch buffer: the coefficient tables of every image, then the horizontally resampled rows tmp[batch][src_h][672] bytes.
inline long long resample_wide_coeff_bytes(int batch) { return batch < 1 ? 0 : (long long)batch * RSW_COEFF_WORDS * 4; }
inline long long resample_wide_scratch_bytes(int batch, int src_h) {
    if (batch < 1 || src_h < 1 || src_h > RS_MAX_SIDE) return 0;
    return resample_wide_coeff_bytes(batch) + (long long)batch * src_h * RSW_ROW_BYTES;
}
inline const char* resample_wide_scratch_error(int batch, int src_h, long long scratch_bytes) {
    if (scratch_bytes < resample_wide_scratch_bytes(batch, src_h)) return "resample: the scratch buffer is too small (dyt_resample_wide_scratch_bytes)";
    return nullptr;
}
// Every argument check of dyt_resample_wide_u8, in the order the entry reports them
inline const char* resample_wide_args_error(unsigned long long src, unsigned long long dst, unsigned long long table, unsigned long long scratch,
                                            int batch, int src_h, int src_w, int capacity, long long scratch_bytes) {
    if (const char* e = resample_ptr_error(src, dst, table, scratch)) return e;
    if (const char* e = resample_shape_error(batch, src_h, src_w, capacity)) return e;
    return resample_wide_scratch_error(batch, src_h, scratch_bytes);
}

}  // namespace dyt
