// On-device Mixup / CutMix (dyt_set_mix, dyt_mix_images, dyt_mix_targets; kernels in image_load.hip and mix.hip): the parameter block the kernels read from
// device memory, the pairing, the scalar formula, the per-pixel source predicate, the CutMix box and every argument check, as plain
// functions of plain values.  A restatement of timm 0.9.12's Mixup(mode='batch', correct_lam=True) + rand_bbox.  No HIP type and no
// header is used here, so a host compiler reads this file on its own (tools/mix_check.cpp walks it without a GPU; build that with
// -ffp-contract=off, see mix_value).
#pragma once

#if defined(__HIP__) || defined(__HIPCC__)
#define DYT_MIX_HD __host__ __device__
#else
#define DYT_MIX_HD
#endif

namespace dyt {

constexpr int MIX_IMG = 224;                                   // image side: the box is drawn in pixels of the 224 x 224 input
constexpr int MIX_IDENTITY = 0, MIX_MIXUP = 1, MIX_CUTMIX = 2;   // MixParams::mode

// One draw, 16 plain 32-bit words in device memory.  Every kernel reads it at run time (never from its arguments), so a captured step
// replayed after the block was overwritten mixes with the new draw.
struct MixParams {
    int mode;              // MIX_IDENTITY: images untouched; MIX_MIXUP: lam_f x + oml_f x_partner; MIX_CUTMIX: the box comes from the partner
    float lam_f, oml_f;    // (float)lam and (float)(1.0 - lam), lam the CORRECTED one for cutmix: images (mixup) and targets (always)
    int yl, yh, xl, xh;    // cutmix: rows [yl, yh) x columns [xl, xh) of every image come from its partner
    float on, off;         // target row t(y): off = smoothing / C everywhere, on = 1 - smoothing + off at y
    int smooth_on;         // the criterion's own label_smoothing e > 0: the mixed row t becomes t * sm_keep + sm_add
    float sm_keep, sm_add; // (float)(1.0 - e), (float)(e / C)
    int reserved[4];
};
static_assert(sizeof(MixParams) == 64, "MixParams is 16 words");

// Image n of `count` (= clips * frames, clip-major) pairs with the same frame of the mirrored clip: x.flip(0) for frames == 1.
DYT_MIX_HD inline int mix_partner(int n, int count, int frames) {
    const int clips = count / frames, b = n / frames, f = n - b * frames;
    return (clips - 1 - b) * frames + f;
}

// lam * a + (1 - lam) * b as torch evaluates it: three fp32 operations, each correctly rounded.  An fma of either product into the sum
// gives other bits, so contraction is switched off for these two functions: by the pragma where the compiler is clang (hipcc contracts
// by default, and HIP's __fmul_rn / __fadd_rn are plain operators there, which it fuses all the same -- the pragma is what holds), by
// -ffp-contract=off on the command line of any other host compiler.
DYT_MIX_HD inline float mix_value(float a, float b, float lam_f, float oml_f) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float pa = lam_f * a, pb = oml_f * b;
    return pa + pb;
}
// the criterion's label smoothing on a mixed target value: two more roundings
DYT_MIX_HD inline float mix_smooth(float t, float sm_keep, float sm_add) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float p = t * sm_keep;
    return p + sm_add;
}

// true: pixel (y, x) of the output is the partner's pixel (cutmix only; mixup blends every pixel, identity none)
DYT_MIX_HD inline bool mix_from_partner(int mode, int y, int x, int yl, int yh, int xl, int xh) {
    return mode == MIX_CUTMIX && y >= yl && y < yh && x >= xl && x < xh;
}
// true: a run of n pixels of row y starting at column x0 needs the partner's pixels at all
DYT_MIX_HD inline bool mix_run_needs_partner(const MixParams& p, int y, int x0, int n) {
    if (p.mode == MIX_MIXUP) return true;
    return p.mode == MIX_CUTMIX && y >= p.yl && y < p.yh && x0 < p.xh && x0 + n > p.xl;
}

// Host side.  rand_bbox(img_shape, lam) with the centre (cy, cx) already drawn (randint(0, 224) each), then correct_lam.
struct MixBox { int yl, yh, xl, xh; };
inline int mix_clip(int v) { return v < 0 ? 0 : (v > MIX_IMG ? MIX_IMG : v); }
inline MixBox mix_box(double lam, int cy, int cx) {
    const double ratio = __builtin_sqrt(1.0 - lam);
    const int cut_h = (int)(MIX_IMG * ratio), cut_w = (int)(MIX_IMG * ratio);
    MixBox b;
    b.yl = mix_clip(cy - cut_h / 2); b.yh = mix_clip(cy + cut_h / 2);
    b.xl = mix_clip(cx - cut_w / 2); b.xh = mix_clip(cx + cut_w / 2);
    return b;
}
inline double mix_corrected_lam(const MixBox& b) { return 1.0 - (double)((b.yh - b.yl) * (b.xh - b.xl)) / (double)(MIX_IMG * MIX_IMG); }

// Each check returns the text of the refusal, or a null pointer.
inline const char* mix_count_error(int count, int frames) {
    if (frames < 1) return "mix: frames < 1";
    if (count < 1 || count % frames != 0) return "mix: the image count is not a positive multiple of frames";
    if ((count / frames) % 2 != 0) return "mix: an odd number of images / clips cannot be paired (batch must be even)";
    return nullptr;
}
inline const char* mix_lam_error(double lam) {
    if (!(lam >= 0.0 && lam <= 1.0)) return "mix: lam outside [0, 1]";
    return nullptr;
}
inline const char* mix_box_error(int yl, int yh, int xl, int xh) {
    if (yl < 0 || xl < 0 || yh > MIX_IMG || xh > MIX_IMG) return "mix: the cutmix box lies outside the 224 x 224 image";
    if (yl > yh || xl > xh) return "mix: the cutmix box is reversed (yl > yh or xl > xh)";
    return nullptr;
}
inline const char* mix_mode_error(int mode) {
    if (mode != MIX_IDENTITY && mode != MIX_MIXUP && mode != MIX_CUTMIX) return "mix: mode is 0 (identity), 1 (mixup) or 2 (cutmix)";
    return nullptr;
}
// src_kind of dyt_mix_images: 0 fp32 [n,3,224,224], 1 uint8 [n,3,224,224], 2 uint8 [n,224,224,3]
inline const char* mix_src_error(int src_kind, unsigned long long src, unsigned long long dst) {
    if (src_kind < 0 || src_kind > 2) return "mix: src_kind is 0 (fp32), 1 (uint8 NCHW) or 2 (uint8 NHWC)";
    if (src % 16 != 0) return "mix: images must be 16-byte aligned (the kernels load 16 bytes at a time)";
    if (dst % 16 != 0) return "mix: dst must be 16-byte aligned";
    return nullptr;
}
inline const char* mix_params_ptr_error(unsigned long long params) {
    if (params == 0) return "mix: null parameter block";
    if (params % 16 != 0) return "mix: the parameter block must be 16-byte aligned";
    return nullptr;
}
inline const char* mix_classes_error(int num_classes) {
    if (num_classes < 1) return "mix: num_classes < 1";
    if (num_classes > 65536) return "mix: num_classes > 65536";
    return nullptr;
}

}  // namespace dyt
