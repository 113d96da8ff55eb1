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

// resample_row_ok without the 2.5 bound: everything a kernel later indexes with, compared in 64-bit first.  box <= src <= batch <= 4096
// and full >= 224 bound the taps by RSW_KMAX.
DYT_RESAMPLE_HD inline bool resample_wide_row_ok(const ResampleRow& r, int batch_src_h, int batch_src_w) {
    const long long sh = r.src_h, sw = r.src_w, t = r.top, l = r.left, bh = r.box_h, bw = r.box_w;
    const long long fh = r.full_h, fw = r.full_w, oy = r.off_y, ox = r.off_x;
    if (batch_src_h > RS_MAX_SIDE || batch_src_w > RS_MAX_SIDE) return false;
    if (sh < 1 || sw < 1 || sh > batch_src_h || sw > batch_src_w) return false;
    if (bh < 1 || bw < 1 || t < 0 || l < 0 || t + bh > sh || l + bw > sw) return false;
    if (fh < RS_OUT || fw < RS_OUT || oy < 0 || ox < 0 || oy + RS_OUT > fh || ox + RS_OUT > fw) return false;
    return true;
}

// resample_coeffs with the wider array: the first tap, the tap count (<= RSW_KMAX for in <= 4096, out >= 224) and the 22-bit coefficients
// of output position xx; k[count..RSW_KMAX) = 0.  The same fp64 operations in the same order, without contraction, so for every
// (in, out, xx) the narrow function takes, xmin, count and the first RS_KMAX integers are its own.  The weights are formed twice (once
// for their sum, once to be normalised) instead of being kept: a device thread then needs no array of 75 doubles.
DYT_RESAMPLE_HD inline void resample_wide_coeffs(int in, int out, int xx, int& xmin, int& count, int (&k)[RSW_KMAX]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * fs;
    const double center = (xx + 0.5) * scale;
    const double ss = 1.0 / fs;
    int lo = (int)(center - support + 0.5);
    if (lo < 0) lo = 0;
    int hi = (int)(center + support + 0.5);
    if (hi > in) hi = in;
    int n = hi - lo;
    if (n < 0) n = 0;
    if (n > RSW_KMAX) n = RSW_KMAX;
    double ww = 0.0;
    for (int x = 0; x < n; ++x) ww += resample_bicubic((x + lo - center + 0.5) * ss);   // summed in index order
    for (int x = 0; x < RSW_KMAX; ++x) {
        double v = 0.0;
        if (x < n) {
            v = resample_bicubic((x + lo - center + 0.5) * ss);
            if (ww != 0.0) v = v / ww;
        }
        k[x] = v < 0 ? (int)(-0.5 + v * (double)(1 << RS_PRECISION_BITS)) : (int)(0.5 + v * (double)(1 << RS_PRECISION_BITS));
    }
    xmin = lo;
    count = n;
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
