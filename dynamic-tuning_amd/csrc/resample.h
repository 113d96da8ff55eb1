// Device RandomResizedCrop / flip / Resize + CenterCrop from byte sources (dyt_resample_u8, dyt_resample_coeffs; kernels in resample.hip):
// the table the kernels read from device memory, the row check, the filter coefficients and every argument check, as plain functions of
// plain values.  A restatement of Pillow's Image.resize for 8-bit images with the bicubic filter (precompute_coeffs +
// normalize_coeffs_8bpc: fp64 coefficients quantised to 22 bits, a horizontal pass that rounds to uint8, then a vertical pass on those
// bytes), applied to a crop box that acts as the image -- what img.crop(box).resize(...) computes.  No HIP type is used here, so a host
// compiler reads this file on its own (tools/resample_check.cpp walks it without a GPU).
#pragma once

#if defined(__HIP__) || defined(__HIPCC__)
#define DYT_RESAMPLE_HD __host__ __device__
#else
#include <math.h>
#define DYT_RESAMPLE_HD
#endif

namespace dyt {

constexpr int RS_OUT = 224;                      // the window written is 224 x 224
constexpr int RS_BICUBIC = 3;                    // ResampleHeader::filter (PIL.Image.BICUBIC); every other value is refused
constexpr int RS_KMAX = 11;                      // taps per output position: ceil(2 * 2.5) * 2 + 1
constexpr int RS_PRECISION_BITS = 22;            // 32 - 8 - 2: Pillow's PRECISION_BITS
constexpr int RS_MAX_SIDE = 4096;                // largest padded source side an entry takes
constexpr int RS_HEADER_WORDS = 16, RS_ROW_WORDS = 12;
constexpr int RS_FLAG_MIRROR = 1;
constexpr int RS_COEFF_FIELDS = 2 + RS_KMAX;     // per output position: first tap, tap count, RS_KMAX coefficients
constexpr int RS_COEFF_WORDS = 2 * RS_COEFF_FIELDS * RS_OUT;   // scratch words per image: [axis 0 = rows, 1 = columns][field][224]

// The table: a 16-word header, then one fixed-stride row per image.  Every kernel reads it at run time (never from its arguments), so a
// captured graph replayed after the table was overwritten resamples with the new draw.
struct ResampleHeader {
    int filter;                  // RS_BICUBIC
    int units;                   // rows that hold a draw: an image whose number is >= units is written as zeros
    int reserved[14];
};
static_assert(sizeof(ResampleHeader) == RS_HEADER_WORDS * 4, "ResampleHeader is 16 words");

struct ResampleRow {
    int src_h, src_w;            // the valid extent of the image inside the batch's padded [Hs, Ws]
    int top, left, box_h, box_w; // the crop box; it acts as the image: taps clamp at its edges
    int full_h, full_w;          // the size the box is resized to
    int off_y, off_x;            // the 224 x 224 window inside full_h x full_w
    int flags;                   // bit 0: mirror the output columns
    int pad;
};
static_assert(sizeof(ResampleRow) == RS_ROW_WORDS * 4 && sizeof(ResampleRow) % 16 == 0, "ResampleRow is 12 words: rows stay 16-byte aligned");

// Everything a kernel later indexes with, compared in 64-bit first: the one row check of both bicubic routes.  bounded: box <= 2.5 * full
// per axis, which bounds the taps by RS_KMAX (the 11-tap route).  Not bounded (resample_wide.h): a batch side above RS_MAX_SIDE is refused
// instead, so that box <= src <= batch <= 4096 and full >= 224 bound the taps by RSW_KMAX.
DYT_RESAMPLE_HD inline bool resample_row_ok_core(const ResampleRow& r, int batch_src_h, int batch_src_w, bool bounded) {
    const long long sh = r.src_h, sw = r.src_w, t = r.top, l = r.left, bh = r.box_h, bw = r.box_w;
    const long long fh = r.full_h, fw = r.full_w, oy = r.off_y, ox = r.off_x;
    if (!bounded && (batch_src_h > RS_MAX_SIDE || batch_src_w > RS_MAX_SIDE)) return false;
    if (sh < 1 || sw < 1 || sh > batch_src_h || sw > batch_src_w) return false;
    if (bh < 1 || bw < 1 || t < 0 || l < 0 || t + bh > sh || l + bw > sw) return false;
    if (fh < RS_OUT || fw < RS_OUT || oy < 0 || ox < 0 || oy + RS_OUT > fh || ox + RS_OUT > fw) return false;
    if (bounded && (2 * bh > 5 * fh || 2 * bw > 5 * fw)) return false;
    return true;
}
DYT_RESAMPLE_HD inline bool resample_row_ok(const ResampleRow& r, int batch_src_h, int batch_src_w) {
    return resample_row_ok_core(r, batch_src_h, batch_src_w, true);
}

// The row of image n, chosen from the image number alone; -1: no row
DYT_RESAMPLE_HD inline int resample_unit(int n, int units, int capacity) { return (n >= 0 && n < capacity && n < units) ? n : -1; }

DYT_RESAMPLE_HD inline double resample_bicubic(double x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// Output position xx of an axis that resizes `in` source pixels to `out`: the first tap, the tap count (<= KMAX: RS_KMAX for in <= 2.5 out,
// resample_wide.h's RSW_KMAX for in <= 4096 and out >= 224) and the 22-bit coefficients; k[count..KMAX) = 0.  One definition for every tap
// bound, so xmin, count and the first integers of a wider instantiation are a narrower one's.  All of it in fp64 without contraction: a
// fused multiply-add rounds once where Pillow's x86-64 build rounds twice, and the integers would differ.  The weights are formed twice
// (once for their sum, in index order, once to be normalised) instead of being kept: a device thread then needs no array of KMAX doubles.
template <int KMAX>
DYT_RESAMPLE_HD inline void resample_coeffs_taps(int in, int out, int xx, int& xmin, int& count, int (&k)[KMAX]) {
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
    if (n > KMAX) n = KMAX;
    double ww = 0.0;
    for (int x = 0; x < n; ++x) ww += resample_bicubic((x + lo - center + 0.5) * ss);
    for (int x = 0; x < KMAX; ++x) {
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
DYT_RESAMPLE_HD inline void resample_coeffs(int in, int out, int xx, int& xmin, int& count, int (&k)[RS_KMAX]) {
    resample_coeffs_taps<RS_KMAX>(in, out, xx, xmin, count, k);
}

// Pillow's clip8 of an accumulator that started at 2^21
DYT_RESAMPLE_HD inline int resample_clip8(int ss) {
    const int v = ss >> RS_PRECISION_BITS;   // arithmetic shift
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// ---- host side: each check returns the text of the refusal, or a null pointer -----------------------------------------------------------
inline const char* resample_ptr_error(unsigned long long src, unsigned long long dst, unsigned long long table, unsigned long long scratch) {
    if (src == 0 || dst == 0 || table == 0 || scratch == 0) return "resample: null pointer";
    if (src % 16 != 0) return "resample: the source must be 16-byte aligned";
    if (dst % 16 != 0) return "resample: dst must be 16-byte aligned (the kernel stores 16 bytes at a time)";
    if (table % 16 != 0) return "resample: the table must be 16-byte aligned";
    if (scratch % 16 != 0) return "resample: the scratch buffer must be 16-byte aligned";
    return nullptr;
}
inline const char* resample_shape_error(int batch, int src_h, int src_w, int capacity) {
    if (batch < 1) return "resample: batch < 1";
    if (src_h < 1 || src_w < 1) return "resample: a source side is < 1";
    if (src_h > RS_MAX_SIDE || src_w > RS_MAX_SIDE) return "resample: a source side is above 4096";
    if (capacity < 1) return "resample: the table holds no row";
    if (batch > capacity) return "resample: the batch has more images than the table has rows";
    return nullptr;
}
inline long long resample_scratch_bytes(int batch) { return batch < 1 ? 0 : (long long)batch * RS_COEFF_WORDS * 4; }
inline const char* resample_scratch_error(int batch, long long scratch_bytes) {
    if (scratch_bytes < resample_scratch_bytes(batch)) return "resample: the scratch buffer is too small (dyt_resample_scratch_bytes)";
    return nullptr;
}

}  // namespace dyt
