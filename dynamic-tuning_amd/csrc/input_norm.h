// Byte-image input (DYT_F_IMAGES_U8 / DYT_F_IMAGES_NHWC, dyt_set_input_norm, dyt_normalize_u8): the scalar formula the byte forms of
// image_load.hip evaluate and every argument check the entries make, as plain functions of plain values.  No HIP type and no header is
// used here, so a host compiler reads this file on its own (tools/input_norm_check.cpp walks it without a GPU).
#pragma once

#if defined(__HIP__) || defined(__HIPCC__)
#define DYT_IN_HD __host__ __device__
#else
#define DYT_IN_HD
#endif

namespace dyt {

// the flag values of include/dyt_hip.h (forward.hip asserts the equality)
constexpr int IN_F_TOKENS_IN = 128, IN_F_IMAGES_U8 = 512, IN_F_IMAGES_NHWC = 1024;

// per-channel statistics of torchvision's Normalize(mean, std); travels by value in the kernels' arguments
struct InputNorm {
    float mean[3];
    float std[3];
};
// the ImageNet statistics (timm's IMAGENET_DEFAULT_MEAN / _STD): what a context holds until dyt_set_input_norm is called
constexpr InputNorm IN_NORM_IMAGENET = {{0.485f, 0.456f, 0.406f}, {0.229f, 0.224f, 0.225f}};

// ToTensor() + Normalize(mean, std) of one byte: three fp32 operations, each correctly rounded, in this order.  No reciprocal, no
// 1/255 constant, nothing an fma could fold (there is no product): with any of those the fp32 result differs for 26-201 of the 256
// byte values of a channel.
DYT_IN_HD inline float input_norm_value(unsigned u, float mean, float std) { return ((float)u / 255.0f - mean) / std; }

inline bool in_finite(float x) { return x - x == 0.0f; }   // false for +-inf and NaN

// Each check returns the text of the refusal, or a null pointer.
inline const char* input_flags_error(int flags) {
    const bool u8 = flags & IN_F_IMAGES_U8, nhwc = flags & IN_F_IMAGES_NHWC, tokens = flags & IN_F_TOKENS_IN;
    if (nhwc && !u8) return "DYT_F_IMAGES_NHWC is a layout of byte images: it needs DYT_F_IMAGES_U8";
    if ((u8 || nhwc) && tokens) return "DYT_F_IMAGES_U8 / DYT_F_IMAGES_NHWC with DYT_F_TOKENS_IN: a token tensor is not an image";
    return nullptr;
}
inline const char* input_ptr_error(unsigned long long address) {
    if (address % 16 != 0) return "byte images must be 16-byte aligned (the kernels load 16 bytes at a time)";
    return nullptr;
}
inline const char* input_norm_error(const float* mean, const float* std) {
    if (!mean || !std) return "input norm: null mean / std";
    for (int c = 0; c < 3; ++c) {
        if (!in_finite(mean[c])) return "input norm: mean must be finite";
        if (!(in_finite(std[c]) && std[c] > 0.0f)) return "input norm: std must be finite and > 0";
    }
    return nullptr;
}

}  // namespace dyt
