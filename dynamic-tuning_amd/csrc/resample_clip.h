// Device clip pipeline -- short-side scale jitter + random crop, random resized crop, uniform (1 or 3 view) crops, mirror -- from byte
// clips (dyt_resample_clip_f32, dyt_resample_clip_coeffs; kernels in resample_clip.hip): the row check, the index / weight function, the
// two-tap arithmetic and every argument check, as plain functions of plain values.  A restatement of
// torch.nn.functional.interpolate(x, size, mode='bilinear', align_corners=False) on NORMALISED fp32 frames, applied to a box that acts
// as the image (crop, then resize), bit for bit: no antialiasing, two taps per axis whatever the scale, nothing rounded to bytes.  The
// table is resample.h's (same header, same 12-word rows) with the header's filter = RS_BILINEAR_F32 and the rows' 12th word = src.
// No HIP type is used here, so a host compiler reads this file on its own (tools/resample_clip_check.cpp walks it without a GPU).
#pragma once
#include "resample.h"

namespace dyt {

constexpr int RS_BILINEAR_F32 = 2;               // ResampleHeader::filter of a clip table (PIL.Image.BILINEAR's number): float bilinear
constexpr int RS_CLIP_MAX_FULL = 1 << 23;        // largest `full` side: d < 2^23, so (float)d + 0.5f = (2d + 1) / 2 is exact in 24 bits
constexpr int RS_CLIP_MAX_FRAMES = 65535, RS_CLIP_MAX_UNITS = 65535;   // grid dimensions y and z
constexpr int RS_CLIP_COEFF_WORDS = 2 * 4 * RS_OUT;   // dyt_resample_clip_coeffs: [axis 0 = rows, 1 = columns][i0, i1, bits(l0), bits(l1)][224]

// A clip row is a ResampleRow whose 12th word is the SOURCE CLIP it reads: output unit r is written from table row r, so several rows
// (spatial views) can share one source clip.
DYT_RESAMPLE_HD inline int clip_row_src(const ResampleRow& r) { return r.pad; }

// Everything a kernel later indexes with, compared in 64-bit first.  There is no 2.5x bound (two taps whatever the scale); `full` is
// bounded by RS_CLIP_MAX_FULL instead, which keeps (float)d + 0.5f exact.
DYT_RESAMPLE_HD inline bool clip_row_ok(const ResampleRow& r, int batch, int batch_src_h, int batch_src_w) {
    const long long sh = r.src_h, sw = r.src_w, t = r.top, l = r.left, bh = r.box_h, bw = r.box_w;
    const long long fh = r.full_h, fw = r.full_w, oy = r.off_y, ox = r.off_x, s = r.pad;
    if (sh < 1 || sw < 1 || sh > batch_src_h || sw > batch_src_w) return false;
    if (bh < 1 || bw < 1 || t < 0 || l < 0 || t + bh > sh || l + bw > sw) return false;
    if (fh < RS_OUT || fw < RS_OUT || fh > RS_CLIP_MAX_FULL || fw > RS_CLIP_MAX_FULL) return false;
    if (oy < 0 || ox < 0 || oy + RS_OUT > fh || ox + RS_OUT > fw) return false;
    if (s < 0 || s >= batch) return false;
    return true;
}

// Position d of an axis that resizes `in` box pixels to `out`: the two taps (relative to the box origin) and their weights, torch's
// area_pixel_compute_source_index + compute_source_index_and_lambda in fp32.  The multiply-add is FUSED (one rounding), as torch's
// build evaluates it.  in >= 1, out >= 1, 0 <= d < out <= RS_CLIP_MAX_FULL.  real < in - 0.5 + 2^-11 for in <= 4096, so i0 <= in - 1;
// the clamp below only states it.
DYT_RESAMPLE_HD inline void clip_axis(int in, int out, int d, int& i0, int& i1, float& l0, float& l1) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float scale = (float)in / (float)out;
    float real = fmaf(scale, (float)d + 0.5f, -0.5f);
    if (!(real > 0.0f)) real = 0.0f;
    int a = (int)real;
    if (a > in - 1) a = in - 1;
    const int b = a + 1 < in ? a + 1 : in - 1;
    float w = real - (float)a;
    w = w < 0.0f ? 0.0f : (w > 1.0f ? 1.0f : w);
    i0 = a;
    i1 = b;
    l1 = w;
    l0 = 1.0f - w;
}

// One axis of the two-tap sum: the second product rounded on its own, the first fused into the sum.  Horizontal first
// (r(y) = clip_lerp(lx0, v[y][x0], lx1, v[y][x1])), then vertical (clip_lerp(ly0, r(y0), ly1, r(y1))).
DYT_RESAMPLE_HD inline float clip_lerp(float w0, float v0, float w1, float v1) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float p = w1 * v1;
    return fmaf(w0, v0, p);
}

// ---- host side: each check returns the text of the refusal, or a null pointer -----------------------------------------------------------
inline const char* clip_ptr_error(unsigned long long src, unsigned long long dst, unsigned long long table) {
    if (src == 0 || dst == 0 || table == 0) return "resample clip: null pointer";
    if (src % 16 != 0) return "resample clip: the source must be 16-byte aligned (the kernel loads 16 bytes at a time)";
    if (dst % 16 != 0) return "resample clip: dst must be 16-byte aligned";
    if (table % 16 != 0) return "resample clip: the table must be 16-byte aligned";
    return nullptr;
}
inline const char* clip_shape_error(int batch, int frames, int src_h, int src_w, int units, int capacity) {
    if (batch < 1) return "resample clip: batch < 1";
    if (frames < 1) return "resample clip: frames < 1";
    if (units < 1) return "resample clip: units < 1";
    if (frames > RS_CLIP_MAX_FRAMES) return "resample clip: more than 65535 frames per clip";
    if (units > RS_CLIP_MAX_UNITS) return "resample clip: more than 65535 units";
    if (src_h < 1 || src_w < 1) return "resample clip: a source side is < 1";
    if (src_h > RS_MAX_SIDE || src_w > RS_MAX_SIDE) return "resample clip: a source side is above 4096";
    if (capacity < 1) return "resample clip: the table holds no row";
    if (units > capacity) return "resample clip: more units than the table has rows";
    return nullptr;
}
inline const char* clip_norm_error(const float* mean, const float* std) {
    if (!mean || !std) return "resample clip: null mean / std";
    for (int c = 0; c < 3; ++c) {
        if (!(mean[c] - mean[c] == 0.0f)) return "resample clip: mean must be finite";
        if (!(std[c] - std[c] == 0.0f) || std[c] == 0.0f) return "resample clip: std must be finite and not zero";
    }
    return nullptr;
}

}  // namespace dyt
