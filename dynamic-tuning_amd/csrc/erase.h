// On-device Random Erasing (dyt_set_erase, dyt_erase_images; the kernel is image_load.hip): the table the kernels read from device memory, the
// per-pixel box test, the noise and every argument check, as plain functions of plain values.  A restatement of the "erase a normalised
// batch" RandomErasing of timm / SlowFast (modes const, rand, pixel; cube = one draw per clip).  No HIP type is used here, so a host
// compiler reads this file on its own (tools/erase_check.cpp walks it without a GPU).  The noise functions are templates over the
// Philox4x32-10 type: the kernels pass dyt_common.h's Philox, a host program passes its own restatement of the same rounds.
#pragma once

#if defined(__HIP__) || defined(__HIPCC__)
#define DYT_ERASE_HD __host__ __device__
#else
#include <math.h>
#define DYT_ERASE_HD
#endif

namespace dyt {

constexpr int ERASE_IMG = 224;                                                      // the boxes are drawn in pixels of the 224 x 224 input
constexpr int ERASE_OFF = 0, ERASE_CONST = 1, ERASE_RAND = 2, ERASE_PIXEL = 3;      // EraseHeader::mode
constexpr int ERASE_MAX_BOXES = 4;
constexpr int ERASE_HEADER_WORDS = 16, ERASE_ROW_WORDS = 20;

// The table: a 16-word header, then one fixed-stride row per unit.  A unit is an image; with `cube` it is a clip (image i reads row
// i / frames, so all frames of a clip share the boxes).  Every kernel reads the table at run time (never from its arguments), so a
// captured step replayed after the table was overwritten erases with the new draw.
struct EraseHeader {
    int mode;                    // ERASE_OFF: nothing is erased; ERASE_CONST: 0.0f; ERASE_RAND: one N(0,1) colour per image, box and channel; ERASE_PIXEL: one per pixel and channel
    int frames;                  // informative (the kernels take the frame count from their arguments)
    int cube;                    // != 0: a unit is a clip of `frames` images
    int units;                   // rows that hold a draw: an image whose unit is >= units is not erased
    unsigned seed_lo, seed_hi;   // the draw's 64-bit Philox seed
    int reserved[10];
};
static_assert(sizeof(EraseHeader) == ERASE_HEADER_WORDS * 4, "EraseHeader is 16 words");

struct EraseRow {
    int n;                            // boxes in use, clamped to [0, ERASE_MAX_BOXES] by the reader
    int box[ERASE_MAX_BOXES][4];      // (top, h, left, w): rows [top, top + h) x columns [left, left + w)
    int pad[3];
};
static_assert(sizeof(EraseRow) == ERASE_ROW_WORDS * 4 && sizeof(EraseRow) % 16 == 0, "EraseRow is 20 words: rows stay 16-byte aligned");

DYT_ERASE_HD inline int erase_clamp_n(int n) { return n < 0 ? 0 : (n > ERASE_MAX_BOXES ? ERASE_MAX_BOXES : n); }

// The row of image n: chosen from the image number alone (never from a table value used as an index); -1: no row, the image is not
// erased.  `capacity` is the number of rows the table's allocation holds, `units` the header's word (compared, not indexed with).
DYT_ERASE_HD inline int erase_unit(int n, int frames, int cube, int units, int capacity) {
    const int u = cube ? n / frames : n;
    return (u < capacity && u < units) ? u : -1;
}

// Box tests in 64-bit, so that no table content overflows: they are comparisons only.
DYT_ERASE_HD inline bool erase_in_box(const int (&b)[4], int y, int x) {
    const long long t = b[0], l = b[2];
    return y >= t && y < t + b[1] && x >= l && x < l + b[3];
}
// index of the LAST box that contains pixel (y, x), or -1: a later box overwrites an earlier one
DYT_ERASE_HD inline int erase_hit(const EraseRow& r, int y, int x) {
    const int n = erase_clamp_n(r.n);
    int hit = -1;
    for (int k = 0; k < ERASE_MAX_BOXES; ++k)
        if (k < n && erase_in_box(r.box[k], y, x)) hit = k;
    return hit;
}
// true: some pixel of the run of n pixels of row y from column x0 may lie in a box (false: the run is untouched)
DYT_ERASE_HD inline bool erase_run_hits(const EraseRow& r, int y, int x0, int n) {
    const int nb = erase_clamp_n(r.n);
    bool any = false;
    for (int k = 0; k < ERASE_MAX_BOXES; ++k) {
        const long long t = r.box[k][0], l = r.box[k][2];
        if (k < nb && y >= t && y < t + r.box[k][1] && x0 < l + r.box[k][3] && (long long)x0 + n > l) any = true;
    }
    return any;
}

// ---- noise: one definition for host and device -----------------------------------------------------------------------------------------
// PH(seed, subseq, offset) is Philox4x32-10 with its four output words in PH::c.  A pair of words gives two normals by Box-Muller with the
// accurate logf / cosf / sinf.  Every value is keyed by its position, not by the thread that computes it.
DYT_ERASE_HD inline float erase_u01(unsigned w) { return ((float)(w >> 8) + 0.5f) * (1.0f / 16777216.0f); }
DYT_ERASE_HD inline void erase_normal_pair(unsigned w0, unsigned w1, float& z0, float& z1) {
    const float r = sqrtf(-2.0f * logf(erase_u01(w0)));
    const float t = 6.2831855f * erase_u01(w1);
    z0 = r * cosf(t);
    z1 = r * sinf(t);
}
// the four values of channel c, row y at columns x4 * 4 .. x4 * 4 + 3 of image n (ERASE_PIXEL)
template <class PH>
DYT_ERASE_HD inline void erase_pixel_noise4(unsigned long long seed, int n, int c, int y, int x4, float (&z)[4]) {
    const PH ph(seed, (unsigned long long)n, (unsigned long long)((c * ERASE_IMG + y) * (ERASE_IMG / 4) + x4));
    erase_normal_pair(ph.c[0], ph.c[1], z[0], z[1]);
    erase_normal_pair(ph.c[2], ph.c[3], z[2], z[3]);
}
// the colour of box `box` of image n in channel c (ERASE_RAND)
template <class PH>
DYT_ERASE_HD inline float erase_box_colour(unsigned long long seed, int n, int box, int c) {
    const PH ph(seed, (unsigned long long)n, (1ull << 32) + (unsigned long long)box);
    float a, b;
    if (c < 2) erase_normal_pair(ph.c[0], ph.c[1], a, b);
    else erase_normal_pair(ph.c[2], ph.c[3], a, b);
    return c == 1 ? b : a;
}

// ---- host side: each check returns the text of the refusal, or a null pointer -----------------------------------------------------------
inline const char* erase_mode_error(int mode) {
    if (mode < ERASE_OFF || mode > ERASE_PIXEL) return "erase: mode is 0 (off), 1 (const), 2 (rand) or 3 (pixel)";
    return nullptr;
}
inline const char* erase_box_error(int top, int h, int left, int w) {
    if (h < 1 || w < 1) return "erase: a box has h < 1 or w < 1";
    if (top < 0 || left < 0 || top > ERASE_IMG - h || left > ERASE_IMG - w) return "erase: a box lies outside the 224 x 224 image";
    return nullptr;
}
inline const char* erase_count_error(int n) {
    if (n < 0 || n > ERASE_MAX_BOXES) return "erase: a unit holds 0 to 4 boxes";
    return nullptr;
}
inline const char* erase_table_ptr_error(unsigned long long table) {
    if (table == 0) return "erase: null table";
    if (table % 16 != 0) return "erase: the table must be 16-byte aligned";
    return nullptr;
}
// a batch of `count` images (clips * frames, clip-major) against a table of `units` rows
inline const char* erase_units_error(int units, int count, int frames, int cube) {
    if (frames < 1) return "erase: frames < 1";
    if (count < 1 || count % frames != 0) return "erase: the image count is not a positive multiple of frames";
    if (units < 1) return "erase: the table holds no unit";
    if (units != (cube ? count / frames : count)) return "erase: the table's units do not match the batch (one per image; one per clip with cube)";
    return nullptr;
}
// a pass over `count` images against a table whose allocation holds `capacity` rows
inline const char* erase_capacity_error(int capacity, int count, int frames) {
    if (frames < 1) return "erase: frames < 1";
    if (count < 1 || count % frames != 0) return "erase: the image count is not a positive multiple of frames";
    if (capacity < count) return "erase: the table holds fewer units than the batch has images";
    return nullptr;
}
// src_kind of dyt_erase_images: 0 fp32 [n,3,224,224], 1 uint8 [n,3,224,224], 2 uint8 [n,224,224,3]
inline const char* erase_src_error(int src_kind, unsigned long long src, unsigned long long dst) {
    if (src_kind < 0 || src_kind > 2) return "erase: src_kind is 0 (fp32), 1 (uint8 NCHW) or 2 (uint8 NHWC)";
    if (src % 16 != 0) return "erase: images must be 16-byte aligned (the kernels load 16 bytes at a time)";
    if (dst % 16 != 0) return "erase: dst must be 16-byte aligned";
    return nullptr;
}

}  // namespace dyt
