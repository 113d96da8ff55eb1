// CPU walk of the device clip pipeline's host logic (dynamic-tuning_amd/csrc/resample_clip.h), without a GPU and without input files:
//   * clip_row_ok for valid rows of every kind, each single violation of its conditions, and hostile words (INT_MIN / INT_MAX in every
//     one of the 12 fields): a row that passes can be indexed with, which the walk proves by forming every extreme index in 64-bit;
//   * clip_axis at the edges -- d = 0, the last d, 1-pixel boxes, scale 1, scales from 1/8 to 18, the largest `full` -- against a
//     restatement in double (the product of two floats is exact there): taps inside the box, i1 - i0 <= 1, weights in [0, 1] that sum
//     to 1 within an ulp, taps monotone in d (what the kernel's staged span relies on), scale 1 = the identity;
//   * clip_lerp against the same restatement, and every argument check the entries make, with the valid neighbours.
// `resample_clip_check axis IN OUT D0 N` prints i0, i1 and the bit patterns of l0, l1 of N positions from D0;
// `resample_clip_check row BATCH HS WS W0 .. W11` prints clip_row_ok of the 12 words;
// `resample_clip_check lerp W0 V0 W1 V1` (bit patterns, hexadecimal) prints the bit pattern of clip_lerp: for a comparison against
// another restatement.
// Build and run (host only):
//   c++ -std=c++17 -O2 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I dynamic-tuning_amd/csrc tools/resample_clip_check.cpp
//     -o /tmp/resample_clip_check && /tmp/resample_clip_check
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "resample_clip.h"

using namespace dyt;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            abort();                                                                 \
        }                                                                            \
    } while (0)

static uint32_t bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
static float from_bits(uint32_t u) { float x; memcpy(&x, &u, 4); return x; }

static ResampleRow make_row(int sh, int sw, int t, int l, int bh, int bw, int fh, int fw, int oy, int ox, int flags = 0, int src = 0) {
    ResampleRow r;
    r.src_h = sh; r.src_w = sw; r.top = t; r.left = l; r.box_h = bh; r.box_w = bw;
    r.full_h = fh; r.full_w = fw; r.off_y = oy; r.off_x = ox; r.flags = flags; r.pad = src;
    return r;
}

// what the kernel forms from a row that passed: every tap of the window inside the box, the box inside the padded shape, the last byte
// of the staged span inside the source allocation
static void index_walk(const ResampleRow& r, int batch, int frames, int Hs, int Ws) {
    CHECK(r.top >= 0 && r.left >= 0 && (long long)r.top + r.box_h <= r.src_h && (long long)r.left + r.box_w <= r.src_w);
    CHECK(r.src_h <= Hs && r.src_w <= Ws && clip_row_src(r) >= 0 && clip_row_src(r) < batch);
    CHECK((long long)r.off_y + RS_OUT <= r.full_h && (long long)r.off_x + RS_OUT <= r.full_w);
    const long long total = (long long)batch * frames * Hs * Ws * 3;
    for (int axis = 0; axis < 2; ++axis) {
        const int in = axis ? r.box_w : r.box_h, out = axis ? r.full_w : r.full_h, off = axis ? r.off_x : r.off_y;
        int lo = INT_MAX, hi = -1, prev0 = -1, prev1 = -1;
        for (int t = 0; t < RS_OUT; ++t) {
            int i0, i1;
            float l0, l1;
            clip_axis(in, out, off + t, i0, i1, l0, l1);
            CHECK(i0 >= 0 && i0 <= i1 && i1 <= in - 1 && i1 - i0 <= 1);
            CHECK(i0 >= prev0 && i1 >= prev1);
            prev0 = i0; prev1 = i1;
            lo = i0 < lo ? i0 : lo;
            hi = i1 > hi ? i1 : hi;
        }
        int f0, f1, g0, g1;
        float a, b;
        clip_axis(in, out, off, f0, f1, a, b);
        clip_axis(in, out, off + RS_OUT - 1, g0, g1, a, b);
        CHECK(f0 == lo && g1 == hi);   // the span the kernel stages covers every tap
    }
    const long long last = ((((long long)clip_row_src(r) * frames + (frames - 1)) * Hs + r.top + r.box_h - 1) * Ws + r.left + r.box_w - 1) * 3 + 2;
    CHECK(last < total);
}

static void walk_rows() {
    const int B = 3, T = 2, Hs = 512, Ws = 640;
    const std::vector<ResampleRow> good = {
        make_row(512, 640, 0, 0, 512, 640, 224, 224, 0, 0),                     // scale 2.29 / 2.86: no 2.5x bound
        make_row(300, 400, 0, 0, 300, 400, 224, 298, 0, 74, 0, 2),              // the third evaluation view, of the last clip
        make_row(64, 64, 63, 63, 1, 1, 224, 224, 0, 0, 1),                      // 1 x 1 box in the last corner, mirrored
        make_row(1, 1, 0, 0, 1, 1, 224, 224, 0, 0),
        make_row(512, 640, 288, 416, 224, 224, 224, 224, 0, 0, 0, 1),           // identity
        make_row(500, 333, 10, 20, 8, 10, 224, 224, 0, 0),                      // upsampling
        make_row(512, 640, 0, 0, 512, 640, 1000, 1000, 776, 776),               // a window in the far corner of a large `full`
        make_row(512, 640, 0, 0, 512, 640, RS_CLIP_MAX_FULL, RS_CLIP_MAX_FULL, RS_CLIP_MAX_FULL - 224, RS_CLIP_MAX_FULL - 224),
    };
    for (const ResampleRow& r : good) { CHECK(clip_row_ok(r, B, Hs, Ws)); index_walk(r, B, T, Hs, Ws); }
    const ResampleRow base = make_row(300, 400, 10, 20, 200, 300, 256, 341, 16, 58, 1, 1);
    CHECK(clip_row_ok(base, B, Hs, Ws));
    CHECK(!clip_row_ok(base, B, 299, Ws) && !clip_row_ok(base, B, Hs, 399) && clip_row_ok(base, B, 300, 400));
    CHECK(!clip_row_ok(base, 1, Hs, Ws) && clip_row_ok(base, 2, Hs, Ws) && !clip_row_ok(base, 0, Hs, Ws) && !clip_row_ok(base, -1, Hs, Ws));
    const int bad_values[] = {INT_MIN, INT_MIN + 1, -1, 0, INT_MAX, INT_MAX - 1, 1 << 30, 4097, RS_CLIP_MAX_FULL + 1};
    int rejected = 0, accepted = 0;
    for (int field = 0; field < RS_ROW_WORDS; ++field)
        for (int v : bad_values) {
            ResampleRow r = base;
            int* w = &r.src_h + field;
            *w = v;
            if (field == 10) { CHECK(clip_row_ok(r, B, Hs, Ws)); index_walk(r, B, T, Hs, Ws); ++accepted; continue; }   // flags: any word
            if (clip_row_ok(r, B, Hs, Ws)) { index_walk(r, B, T, Hs, Ws); ++accepted; }
            else ++rejected;
        }
    CHECK(rejected + accepted == RS_ROW_WORDS * 9 && rejected >= 80);
    // each condition, violated by one
    ResampleRow r = base; r.top = 101; CHECK(!clip_row_ok(r, B, Hs, Ws));                 // box below the valid extent
    r = base; r.top = 100; CHECK(clip_row_ok(r, B, Hs, Ws));
    r = base; r.left = 101; CHECK(!clip_row_ok(r, B, Hs, Ws));
    r = base; r.top = -1; CHECK(!clip_row_ok(r, B, Hs, Ws));
    r = base; r.left = -1; CHECK(!clip_row_ok(r, B, Hs, Ws));
    r = base; r.box_h = 0; CHECK(!clip_row_ok(r, B, Hs, Ws));
    r = base; r.box_w = 0; CHECK(!clip_row_ok(r, B, Hs, Ws));
    r = base; r.src_h = 0; CHECK(!clip_row_ok(r, B, Hs, Ws));
    r = base; r.src_w = 641; CHECK(!clip_row_ok(r, B, Hs, Ws));
    r = base; r.full_h = 223; r.off_y = 0; CHECK(!clip_row_ok(r, B, Hs, Ws));
    r = base; r.full_w = 223; r.off_x = 0; CHECK(!clip_row_ok(r, B, Hs, Ws));
    r = base; r.full_h = RS_CLIP_MAX_FULL + 1; CHECK(!clip_row_ok(r, B, Hs, Ws));
    r = base; r.full_w = RS_CLIP_MAX_FULL + 1; CHECK(!clip_row_ok(r, B, Hs, Ws));
    r = base; r.full_w = RS_CLIP_MAX_FULL; CHECK(clip_row_ok(r, B, Hs, Ws));
    r = base; r.off_y = 33; CHECK(!clip_row_ok(r, B, Hs, Ws));                            // 33 + 224 > 256
    r = base; r.off_y = 32; CHECK(clip_row_ok(r, B, Hs, Ws));
    r = base; r.off_x = 118; CHECK(!clip_row_ok(r, B, Hs, Ws));
    r = base; r.off_x = -1; CHECK(!clip_row_ok(r, B, Hs, Ws));
    r = base; r.off_y = -1; CHECK(!clip_row_ok(r, B, Hs, Ws));
    r = base; r.pad = B; CHECK(!clip_row_ok(r, B, Hs, Ws));
    r = base; r.pad = -1; CHECK(!clip_row_ok(r, B, Hs, Ws));
    r = base; r.pad = B - 1; CHECK(clip_row_ok(r, B, Hs, Ws));
    r = make_row(512, 640, 0, 0, 512, 640, 224, 224, 0, 0); CHECK(clip_row_ok(r, B, Hs, Ws) && !resample_row_ok(r, Hs, Ws));   // the bicubic bound is not this one
    for (int fill : {INT_MIN, INT_MAX, -1}) {                                             // every word hostile at once
        ResampleRow h;
        int* p = &h.src_h;
        for (int i = 0; i < RS_ROW_WORDS; ++i) p[i] = fill;
        CHECK(!clip_row_ok(h, B, Hs, Ws));
        CHECK(!clip_row_ok(h, INT_MAX, RS_MAX_SIDE, RS_MAX_SIDE));
    }
    printf("resample clip check: rows ok (%d hostile rows rejected, %d accepted and indexed)\n", rejected, accepted);
}

// the restatement: torch's area_pixel_compute_source_index / compute_source_index_and_lambda with the fused step in double
static void brute_axis(int in, int out, int d, int& i0, int& i1, float& l0, float& l1) {
    const float scale = (float)in / (float)out;
    const float x = (float)d + 0.5f;
    CHECK((double)x == (double)d + 0.5);                                   // exact below 2^23
    float real = (float)((double)scale * (double)x - 0.5);                 // the product is exact in double; one rounding to float
    if (real < 0.0f) real = 0.0f;
    const int a = (int)real;
    i0 = a;
    i1 = a + (a < in - 1 ? 1 : 0);
    float w = real - (float)a;
    w = w < 0.0f ? 0.0f : (w > 1.0f ? 1.0f : w);
    l1 = w;
    l0 = 1.0f - w;
}

static long long walk_pair(int in, int out, const std::vector<int>& ds) {
    long long n = 0;
    for (int d : ds) {
        if (d < 0 || d >= out) continue;
        int i0, i1, j0, j1;
        float l0, l1, m0, m1;
        clip_axis(in, out, d, i0, i1, l0, l1);
        brute_axis(in, out, d, j0, j1, m0, m1);
        CHECK(i0 == j0 && i1 == j1 && bits(l0) == bits(m0) && bits(l1) == bits(m1));
        CHECK(i0 >= 0 && i0 <= i1 && i1 <= in - 1 && i1 - i0 <= 1);
        CHECK(l1 >= 0.0f && l1 <= 1.0f && l0 >= 0.0f && l0 <= 1.0f && fabsf(l0 + l1 - 1.0f) <= 1.2e-7f);
        if (in == out) CHECK(i0 == d && bits(l1) == 0 && bits(l0) == bits(1.0f));
        if (in == 1) CHECK(i0 == 0 && i1 == 0);
        if (d == 0 && in <= 3 * out) CHECK(i0 == 0);   // real = scale / 2 - 1 / 2 < 1
        ++n;
    }
    return n;
}

static void walk_axis() {
    long long positions = 0;
    // scales from 1/8 to 18, scale 1, 1-pixel boxes, every position
    const int pairs[][2] = {{28, 224}, {32, 256}, {64, 224}, {128, 224}, {171, 299}, {224, 224}, {256, 256}, {4096, 4096}, {240, 224}, {320, 298}, {300, 224},
                            {400, 298}, {480, 258}, {640, 344}, {512, 224}, {1000, 224}, {2016, 224}, {4032, 224}, {4096, 228}, {4096, 224}, {1, 224}, {1, 1000},
                            {2, 224}, {3, 224}, {8, 224}, {10, 224}, {33, 224}, {57, 386}, {4095, 4096}, {4096, 4095}, {223, 224}, {225, 224}};
    for (const auto& p : pairs) {
        std::vector<int> ds(p[1]);
        for (int d = 0; d < p[1]; ++d) ds[d] = d;
        positions += walk_pair(p[0], p[1], ds);
    }
    // the largest `full`: the first and the last positions, where (float)d + 0.5f runs out of bits
    for (int in : {1, 2, 224, 4096}) {
        const int out = RS_CLIP_MAX_FULL;
        std::vector<int> ds;
        for (int k = 0; k < 300; ++k) { ds.push_back(k); ds.push_back(out - 1 - k); ds.push_back(out / 2 + k); ds.push_back((1 << 22) - 150 + k); }
        positions += walk_pair(in, out, ds);
    }
    // every pair of a coarse sweep, the edges of each
    for (int in = 1; in <= 4096; in += (in < 70 ? 1 : 97))
        for (int out : {224, 225, 256, 258, 298, 341, 1000, 4096, 100000})
            positions += walk_pair(in, out, {0, 1, 2, 111, 223, out / 2, out - 2, out - 1});
    printf("resample clip check: axis ok (%lld positions)\n", positions);
}

static void walk_lerp() {
    uint32_t s = 12345u;
    auto next = [&]() { s = s * 1664525u + 1013904223u; return s; };
    long long n = 0;
    for (int k = 0; k < 200000; ++k) {
        const float w1 = (float)(next() >> 8) / 16777216.0f, w0 = 1.0f - w1;
        const float v0 = ((float)(next() >> 8) / 16777216.0f - 0.5f) * 5.4f, v1 = ((float)(next() >> 8) / 16777216.0f - 0.5f) * 5.4f;
        const float p = w1 * v1;
        const double a = (double)w0 * (double)v0, b = (double)p;           // the product is exact in double
        const double sum = a + b, bv = sum - a, err = (a - (sum - bv)) + (b - bv);   // TwoSum: sum + err = a + b exactly
        if (err != 0.0) continue;                                          // (rare: the double sum itself rounded; no single-rounding witness)
        CHECK(bits(clip_lerp(w0, v0, w1, v1)) == bits((float)sum));
        ++n;
    }
    CHECK(bits(clip_lerp(1.0f, 0.75f, 0.0f, -2.0f)) == bits(0.75f));       // weight 0 drops its tap
    CHECK(bits(clip_lerp(0.0f, 0.75f, 1.0f, -2.0f)) == bits(-2.0f));
    printf("resample clip check: lerp ok (%lld values)\n", n);
}

static void walk_refusals() {
    CHECK(!clip_ptr_error(0x1000, 0x2000, 0x3000));
    CHECK(clip_ptr_error(0, 0x2000, 0x3000) && clip_ptr_error(0x1000, 0, 0x3000) && clip_ptr_error(0x1000, 0x2000, 0));
    CHECK(clip_ptr_error(0x1004, 0x2000, 0x3000) && clip_ptr_error(0x1000, 0x2008, 0x3000) && clip_ptr_error(0x1000, 0x2000, 0x3004));
    CHECK(!clip_shape_error(2, 2, 64, 64, 2, 4) && !clip_shape_error(1, 1, 4096, 4096, 1, 1) && !clip_shape_error(1, 65535, 1, 1, 65535, 65535));
    CHECK(!clip_shape_error(1, 8, 64, 64, 3, 3));                                          // three views of one clip
    CHECK(clip_shape_error(0, 2, 64, 64, 2, 4) && clip_shape_error(2, 0, 64, 64, 2, 4) && clip_shape_error(2, 2, 64, 64, 0, 4));
    CHECK(clip_shape_error(-1, 2, 64, 64, 2, 4) && clip_shape_error(2, -1, 64, 64, 2, 4) && clip_shape_error(2, 2, 64, 64, -1, 4));
    CHECK(clip_shape_error(2, 65536, 64, 64, 2, 4) && clip_shape_error(2, 2, 64, 64, 65536, 70000));
    CHECK(clip_shape_error(2, 2, 0, 64, 2, 4) && clip_shape_error(2, 2, 64, 0, 2, 4) && clip_shape_error(2, 2, 4097, 64, 2, 4));
    CHECK(clip_shape_error(2, 2, 64, 4097, 2, 4) && clip_shape_error(2, 2, 64, -1, 2, 4));
    CHECK(clip_shape_error(2, 2, 64, 64, 5, 4) && clip_shape_error(2, 2, 64, 64, 1, 0));
    const float m[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
    CHECK(!clip_norm_error(m, sd) && clip_norm_error(nullptr, sd) && clip_norm_error(m, nullptr));
    for (int c = 0; c < 3; ++c) {
        float a[3] = {m[0], m[1], m[2]}, b[3] = {sd[0], sd[1], sd[2]};
        b[c] = 0.0f; CHECK(clip_norm_error(m, b));
        b[c] = -0.0f; CHECK(clip_norm_error(m, b));
        b[c] = INFINITY; CHECK(clip_norm_error(m, b));
        b[c] = NAN; CHECK(clip_norm_error(m, b));
        b[c] = -0.5f; CHECK(!clip_norm_error(m, b));                                      // finite and not zero
        a[c] = NAN; CHECK(clip_norm_error(a, sd));
        a[c] = -INFINITY; CHECK(clip_norm_error(a, sd));
    }
    printf("resample clip check: refusals ok\n");
}

int main(int argc, char** argv) {
    if (argc == 6 && !strcmp(argv[1], "axis")) {
        const int in = atoi(argv[2]), out = atoi(argv[3]), d0 = atoi(argv[4]), n = atoi(argv[5]);
        for (int d = d0; d < d0 + n; ++d) {
            int i0, i1;
            float l0, l1;
            clip_axis(in, out, d, i0, i1, l0, l1);
            printf("%d %d %u %u\n", i0, i1, bits(l0), bits(l1));
        }
        return 0;
    }
    if (argc == 5 + RS_ROW_WORDS && !strcmp(argv[1], "row")) {   // row BATCH HS WS and the row's 12 words: prints clip_row_ok
        ResampleRow r;
        int* w = &r.src_h;
        for (int k = 0; k < RS_ROW_WORDS; ++k) w[k] = (int)strtoll(argv[5 + k], nullptr, 10);
        printf("%d\n", clip_row_ok(r, atoi(argv[2]), atoi(argv[3]), atoi(argv[4])) ? 1 : 0);
        return 0;
    }
    if (argc == 6 && !strcmp(argv[1], "lerp")) {
        uint32_t a[4];
        for (int k = 0; k < 4; ++k) a[k] = (uint32_t)strtoul(argv[2 + k], nullptr, 16);
        printf("%08x\n", bits(clip_lerp(from_bits(a[0]), from_bits(a[1]), from_bits(a[2]), from_bits(a[3]))));
        return 0;
    }
    walk_rows();
    walk_axis();
    walk_lerp();
    walk_refusals();
    printf("resample clip check: all ok\n");
    return 0;
}
