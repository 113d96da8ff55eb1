// RandAugment on the device for byte clips and images (dyt_randaug_u8, dyt_randaug_table; kernels in randaug.hip): the table the kernels
// read, the row check, the table builders, the blend, the 3 x 3 SMOOTH filter, the affine gather with both filters and every argument
// check, as plain functions of plain values.  A restatement of Pillow's 8-bit arithmetic behind the reference's
// video_datasets/rand_augment.py -- ImageOps.autocontrast / equalize / invert / posterize / solarize, Image.point, ImageEnhance (Image.blend
// against a degenerate image), ImageFilter.SMOOTH and Image.transform(AFFINE) with a fill colour -- byte for byte.  One definition serves
// host and device; every floating-point step is evaluated as written (fp contract off).  No HIP type is used here, so a host compiler reads
// this file on its own (tools/randaug_check.cpp walks it without a GPU).
#pragma once
#include <stdint.h>

#include "resample.h"

namespace dyt {

constexpr int AUG_MAGIC = 0x31475541;            // AugHeader::magic ("AUG1"); with any other value every unit is written as zeros
constexpr int AUG_HEADER_WORDS = 16, AUG_ROW_WORDS = 20;
constexpr int AUG_MAX_LAYERS = 8, AUG_MAX_GRID = 65535;   // num_layers of a config; units * frames is grid dimension y
constexpr int AUG_BILINEAR = 2, AUG_BICUBIC = 3;          // PIL.Image.BILINEAR / BICUBIC
constexpr int AUG_HIST_WORDS = 4 * 256;          // per (unit, frame): the R, G, B and L histograms of the valid region
constexpr int AUG_TABLE_WORDS = 3 * 256 + 1;     // dyt_randaug_table: the 3 x 256 table and the Contrast constant
constexpr double AUG_MAX_COEFF = 1099511627776.0;   // 2^40: every coordinate stays finite

enum AugOp { AUG_IDENTITY = 0, AUG_INVERT, AUG_SOLARIZE, AUG_SOLARIZE_ADD, AUG_POSTERIZE, AUG_AUTO_CONTRAST, AUG_EQUALIZE, AUG_BRIGHTNESS,
             AUG_COLOR, AUG_CONTRAST, AUG_SHARPNESS, AUG_AFFINE, AUG_OPS };
enum AugFamily { AUG_FAM_TABLE = 0, AUG_FAM_BLEND, AUG_FAM_SHARP, AUG_FAM_AFFINE, AUG_FAMILIES };
constexpr unsigned AUG_LAUNCH_STATS = 1u << AUG_FAMILIES, AUG_LAUNCH_ALL = (1u << (AUG_FAMILIES + 1)) - 1;   // bits of a layer's launch mask
enum AugBuffer { AUG_BUF_SRC = 0, AUG_BUF_DST = 1, AUG_BUF_WORK = 2 };

// The table: a 16-word header, then rows [layers][capacity], one per (layer, unit).  The kernels read it from device memory when they run.
struct AugHeader {
    int magic;                   // AUG_MAGIC
    int units;                   // units that hold a draw: a unit whose number is >= units is written as zeros
    int layers;                  // must equal the entry's `layers`
    int reserved[13];
};
static_assert(sizeof(AugHeader) == AUG_HEADER_WORDS * 4, "AugHeader is 16 words");

struct AugRow {
    int op;                      // AugOp
    int h, w;                    // the unit's valid extent inside the batch's padded [Hs, Ws]
    int iarg;                    // Solarize: threshold 0..256, SolarizeAdd: 0..255, Posterize: bits 0..8
    int filter;                  // AUG_BILINEAR / AUG_BICUBIC (read by Affine)
    int fill;                    // r | g << 8 | b << 16 (read by Affine)
    float factor;                // Brightness / Color / Contrast / Sharpness
    int bufs;                    // source buffer | destination buffer << 8 (AugBuffer)
    double c[6];                 // Affine: output (x, y) reads input (c0 x + c1 y + c2, c3 x + c4 y + c5)
};
static_assert(sizeof(AugRow) == AUG_ROW_WORDS * 4 && sizeof(AugRow) % 16 == 0, "AugRow is 20 words: rows stay 16-byte aligned");

DYT_RESAMPLE_HD inline int aug_row_src(const AugRow& r) { return r.bufs & 0xFF; }
DYT_RESAMPLE_HD inline int aug_row_dst(const AugRow& r) { return (r.bufs >> 8) & 0xFF; }
DYT_RESAMPLE_HD inline int aug_family(int op) {
    return op <= AUG_EQUALIZE ? AUG_FAM_TABLE : (op <= AUG_CONTRAST ? AUG_FAM_BLEND : (op == AUG_SHARPNESS ? AUG_FAM_SHARP : AUG_FAM_AFFINE));
}
DYT_RESAMPLE_HD inline bool aug_needs_stats(int op) { return op == AUG_AUTO_CONTRAST || op == AUG_EQUALIZE || op == AUG_CONTRAST; }
DYT_RESAMPLE_HD inline bool aug_finite(double v) { return v - v == 0.0; }

// Everything a kernel later indexes or branches with, compared first.  Layer 0 reads the source batch and no other layer does; the
// neighbourhood operations never write the buffer they read.
DYT_RESAMPLE_HD inline bool aug_row_ok(const AugRow& r, int layer, int batch_src_h, int batch_src_w) {
    const long long h = r.h, w = r.w;
    if (h < 1 || w < 1 || h > batch_src_h || w > batch_src_w) return false;
    if (r.op < 0 || r.op >= AUG_OPS) return false;
    if (r.iarg < 0 || r.iarg > 256) return false;
    if (r.op == AUG_SOLARIZE_ADD && r.iarg > 255) return false;
    if (r.op == AUG_POSTERIZE && r.iarg > 8) return false;
    if (r.filter != AUG_BILINEAR && r.filter != AUG_BICUBIC) return false;
    if (r.fill < 0 || r.fill > 0xFFFFFF) return false;
    if (!aug_finite((double)r.factor)) return false;
    for (int k = 0; k < 6; ++k)
        if (!aug_finite(r.c[k]) || r.c[k] > AUG_MAX_COEFF || r.c[k] < -AUG_MAX_COEFF) return false;
    const int s = aug_row_src(r), d = aug_row_dst(r);
    if ((r.bufs >> 16) != 0 || s > AUG_BUF_WORK || (d != AUG_BUF_DST && d != AUG_BUF_WORK)) return false;
    if ((layer == 0) != (s == AUG_BUF_SRC)) return false;
    if (aug_family(r.op) >= AUG_FAM_SHARP && s == d) return false;
    return true;
}
// Layer l reads what layer l - 1 wrote, of the same extent
DYT_RESAMPLE_HD inline bool aug_link_ok(const AugRow& prev, const AugRow& cur) { return aug_row_src(cur) == aug_row_dst(prev) && cur.h == prev.h && cur.w == prev.w; }
// The last layer leaves the unit in dst
DYT_RESAMPLE_HD inline bool aug_last_ok(const AugRow& r) { return aug_row_dst(r) == AUG_BUF_DST; }

// The row of (layer, unit) in words from the table's start; -1: no row
DYT_RESAMPLE_HD inline long long aug_row_at(int layer, int unit, int layers, int units, int capacity) {
    if (layer < 0 || layer >= layers || unit < 0 || unit >= units || unit >= capacity) return -1;
    return AUG_HEADER_WORDS + ((long long)layer * capacity + unit) * AUG_ROW_WORDS;
}

// ---- arithmetic ---------------------------------------------------------------------------------------------------------------------------
DYT_RESAMPLE_HD inline int aug_luma(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }   // convert("L")

DYT_RESAMPLE_HD inline uint8_t aug_clip8f(float t) { return t <= 0.0f ? (uint8_t)0 : (t >= 255.0f ? (uint8_t)255 : (uint8_t)t); }
DYT_RESAMPLE_HD inline uint8_t aug_clip8d(double t) { return t <= 0.0 ? (uint8_t)0 : (t >= 255.0 ? (uint8_t)255 : (uint8_t)t); }

// Image.blend(degenerate, image, alpha): fp32; truncated for 0 <= alpha <= 1 (the value lies in 0..255), clipped otherwise
DYT_RESAMPLE_HD inline uint8_t aug_blend(int d, int v, float alpha) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float p = alpha * (float)(v - d);
    const float t = (float)d + p;
    if (alpha >= 0.0f && alpha <= 1.0f) return (uint8_t)t;
    return aug_clip8f(t);
}

// ImageFilter.SMOOTH of one channel: a = the row above, m = the row itself, b = the row below, three consecutive columns each
DYT_RESAMPLE_HD inline uint8_t aug_smooth(const int a[3], const int m[3], const int b[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float k1 = 1.0f / 13.0f, k5 = 5.0f / 13.0f;
    float ss = 0.5f;
    float t0 = (float)b[0] * k1, t1 = (float)b[1] * k1, t2 = (float)b[2] * k1;
    ss = ss + ((t0 + t1) + t2);
    t0 = (float)m[0] * k1; t1 = (float)m[1] * k5; t2 = (float)m[2] * k1;
    ss = ss + ((t0 + t1) + t2);
    t0 = (float)a[0] * k1; t1 = (float)a[1] * k1; t2 = (float)a[2] * k1;
    ss = ss + ((t0 + t1) + t2);
    return aug_clip8f(ss);
}

// int(ImageStat.Stat(L).mean[0] + 0.5) from the L histogram
DYT_RESAMPLE_HD inline int aug_contrast_mean(const int* hist_l) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    long long sum = 0, n = 0;
    for (int i = 0; i < 256; ++i) { sum += (long long)i * hist_l[i]; n += hist_l[i]; }
    if (n <= 0) return 0;
    const double mean = (double)sum / (double)n;
    return (int)(mean + 0.5);
}

// The 256-entry table of one channel of a table operation; `hist` (the channel's histogram) is read by AutoContrast and Equalize only
DYT_RESAMPLE_HD inline void aug_build_table(int op, int iarg, const int* hist, uint8_t* lut) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    for (int i = 0; i < 256; ++i) lut[i] = (uint8_t)i;
    if (op == AUG_INVERT) {
        for (int i = 0; i < 256; ++i) lut[i] = (uint8_t)(255 - i);
    } else if (op == AUG_SOLARIZE) {
        for (int i = 0; i < 256; ++i) lut[i] = (uint8_t)(i < iarg ? i : 255 - i);
    } else if (op == AUG_SOLARIZE_ADD) {
        for (int i = 0; i < 128; ++i) lut[i] = (uint8_t)(i + iarg > 255 ? 255 : i + iarg);
    } else if (op == AUG_POSTERIZE) {
        if (iarg < 8) {
            const int mask = ~((1 << (8 - iarg)) - 1);
            for (int i = 0; i < 256; ++i) lut[i] = (uint8_t)(i & mask);
        }
    } else if (op == AUG_AUTO_CONTRAST) {
        int lo = 0, hi = 255;
        while (lo < 256 && hist[lo] == 0) ++lo;
        while (hi >= 0 && hist[hi] == 0) --hi;
        if (hi > lo) {
            const double scale = 255.0 / (double)(hi - lo);
            const double offset = (double)(-lo) * scale;
            for (int i = 0; i < 256; ++i) {
                const double p = (double)i * scale;
                const int v = (int)(p + offset);
                lut[i] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
            }
        }
    } else if (op == AUG_EQUALIZE) {
        long long total = 0, last = 0;
        int bins = 0;
        for (int i = 0; i < 256; ++i)
            if (hist[i] != 0) { total += hist[i]; last = hist[i]; ++bins; }
        const long long step = (total - last) / 255;
        if (bins >= 2 && step > 0) {
            long long n = step / 2;
            for (int i = 0; i < 256; ++i) {
                const long long v = n / step;
                lut[i] = (uint8_t)(v > 255 ? 255 : v);
                n += hist[i];
            }
        }
    }
}

// Pillow's affine_transform: the input position of output pixel (x, y); false: outside the image, the pixel is the fill colour
DYT_RESAMPLE_HD inline bool aug_affine_coord(const double* c, int x, int y, int w, int h, double& xin, double& yin) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double xc = (double)x + 0.5, yc = (double)y + 0.5;
    double px = c[0] * xc, py = c[1] * yc;
    xin = (px + py) + c[2];
    px = c[3] * xc; py = c[4] * yc;
    yin = (px + py) + c[5];
    return xin >= 0.0 && xin < (double)w && yin >= 0.0 && yin < (double)h;
}

DYT_RESAMPLE_HD inline double aug_cubic(double v1, double v2, double v3, double v4, double d) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double p1 = v2;
    const double p2 = -v1 + v3;
    const double p3 = 2.0 * (v1 - v2) + v3 - v4;
    const double p4 = -v1 + v2 - v3 + v4;
    const double q = d * p4;
    const double r = d * (p3 + q);
    const double s = d * (p2 + r);
    return p1 + s;
}

DYT_RESAMPLE_HD inline double aug_lerp(double a, double b, double d) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double p = (b - a) * d;
    return a + p;
}

DYT_RESAMPLE_HD inline int aug_clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// One output pixel of Image.transform(size, AFFINE, c, resample=filter, fillcolor=fill) of a frame of w x h whose pixel (yy, xx), both
// inside the frame, is the three bytes at px(yy, xx).  Taps are clamped to the frame.
template <class Px>
DYT_RESAMPLE_HD inline void aug_affine_pixel(const double* c, int filter, int fill, int w, int h, int x, int y, Px px, uint8_t out[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double xin, yin;
    if (!aug_affine_coord(c, x, y, w, h, xin, yin)) {
        out[0] = (uint8_t)(fill & 0xFF); out[1] = (uint8_t)((fill >> 8) & 0xFF); out[2] = (uint8_t)((fill >> 16) & 0xFF);
        return;
    }
    xin -= 0.5;
    yin -= 0.5;
    const double fx = floor(xin), fy = floor(yin);
    const double dx = xin - fx, dy = yin - fy;
    const int x0 = (int)fx, y0 = (int)fy;          // -1 <= x0 < w, -1 <= y0 < h
    if (filter == AUG_BILINEAR) {
        const int xa = aug_clampi(x0, w - 1), xb = aug_clampi(x0 + 1, w - 1), ya = aug_clampi(y0, h - 1), yb = aug_clampi(y0 + 1, h - 1);
        const uint8_t *p00 = px(ya, xa), *p01 = px(ya, xb), *p10 = px(yb, xa), *p11 = px(yb, xb);
        for (int k = 0; k < 3; ++k) {
            const double r0 = aug_lerp((double)p00[k], (double)p01[k], dx), r1 = aug_lerp((double)p10[k], (double)p11[k], dx);
            out[k] = (uint8_t)aug_lerp(r0, r1, dy);
        }
        return;
    }
    const int xs[4] = {aug_clampi(x0 - 1, w - 1), aug_clampi(x0, w - 1), aug_clampi(x0 + 1, w - 1), aug_clampi(x0 + 2, w - 1)};
    double v[4][3];
    for (int j = 0; j < 4; ++j) {
        const int yy = aug_clampi(y0 - 1 + j, h - 1);
        const uint8_t *a = px(yy, xs[0]), *b = px(yy, xs[1]), *cc = px(yy, xs[2]), *d = px(yy, xs[3]);
        for (int k = 0; k < 3; ++k) v[j][k] = aug_cubic((double)a[k], (double)b[k], (double)cc[k], (double)d[k], dx);
    }
    for (int k = 0; k < 3; ++k) out[k] = aug_clip8d(aug_cubic(v[0][k], v[1][k], v[2][k], v[3][k], dy));
}

// ---- host side: each check returns the text of the refusal, or a null pointer -----------------------------------------------------------------
inline const char* aug_ptr_error(unsigned long long src, unsigned long long dst, unsigned long long work, unsigned long long stats,
                                 unsigned long long table) {
    if (src == 0 || dst == 0 || work == 0 || stats == 0 || table == 0) return "randaug: null pointer";
    if (src % 16 != 0) return "randaug: the source must be 16-byte aligned";
    if (dst % 16 != 0) return "randaug: dst must be 16-byte aligned";
    if (work % 16 != 0) return "randaug: work must be 16-byte aligned";
    if (stats % 16 != 0) return "randaug: stats must be 16-byte aligned";
    if (table % 16 != 0) return "randaug: the table must be 16-byte aligned";
    if (src == dst) return "randaug: src and dst are the same buffer (the source batch is never written)";
    if (src == work || dst == work) return "randaug: work must be a buffer of its own";
    return nullptr;
}
inline const char* aug_shape_error(int units, int frames, int src_h, int src_w, int capacity, int layers) {
    if (units < 1) return "randaug: units < 1";
    if (frames < 1) return "randaug: frames < 1";
    if (layers < 1) return "randaug: layers < 1";
    if (layers > AUG_MAX_LAYERS) return "randaug: more than 8 layers";
    if (units > AUG_MAX_GRID || frames > AUG_MAX_GRID || (long long)units * frames > AUG_MAX_GRID) return "randaug: units * frames is above 65535";
    if (src_h < 1 || src_w < 1) return "randaug: a source side is < 1";
    if (src_h > RS_MAX_SIDE || src_w > RS_MAX_SIDE) return "randaug: a source side is above 4096";
    if (capacity < 1) return "randaug: the table holds no row";
    if (units > capacity) return "randaug: more units than the table has rows per layer";
    return nullptr;
}

}  // namespace dyt
