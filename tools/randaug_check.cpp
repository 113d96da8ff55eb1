// CPU walk of the device RandAugment's host-and-device logic (dynamic-tuning_amd/csrc/randaug.h), without a GPU:
//   * aug_row_ok / aug_link_ok / aug_last_ok for valid rows of every operation, each single violation and hostile words; a row that passes
//     can be indexed with, which the walk proves by running every operation with a bounds-checking pixel accessor, hostile coefficients
//     (+-2^40, denormals) included;
//   * identities of the arithmetic: the identity matrix copies the frame with both filters, factor 1 copies it through every blend, SMOOTH
//     of a constant is the constant, the tables of Invert / Solarize / Posterize at their edge arguments;
//   * every argument check the entries make, with the valid neighbours.
// `randaug_check row LAYER HS WS W0 .. W19` (the row's 20 words, hexadecimal) prints aug_row_ok;
// `randaug_check file PATH` reads cases recorded from Pillow and compares byte for byte (tests/test_randaug_draw_host.py writes the file
// from tests/golden/randaug/randaug.npz):
//     T op iarg / 256 histogram counts / 256 expected entries (-1: not observed)          a table builder
//     C mean / 256 counts of the L histogram                                              the Contrast constant
//     P op iarg factor filter c0 .. c5 h w / h * w * 3 source bytes / h * w * 3 expected  one operation on one frame
// (floating-point values as C99 hexadecimal literals).
// Build and run (host only):
//   c++ -std=c++17 -O2 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I dynamic-tuning_amd/csrc tools/randaug_check.cpp
//     -o /tmp/randaug_check && /tmp/randaug_check
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "randaug.h"

using namespace dyt;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            abort();                                                                 \
        }                                                                            \
    } while (0)

static AugRow make_row(int op, int h, int w, int iarg = 0, float factor = 1.0f, int filter = AUG_BICUBIC, int src = AUG_BUF_SRC, int dst = AUG_BUF_DST) {
    AugRow r;
    memset(&r, 0, sizeof(r));
    r.op = op; r.h = h; r.w = w; r.iarg = iarg; r.filter = filter; r.fill = 128 | 128 << 8 | 128 << 16; r.factor = factor; r.bufs = src | dst << 8;
    r.c[0] = 1.0; r.c[4] = 1.0;
    return r;
}

// One operation on one frame [h, w, 3], as the kernels run it: histograms, the table or the constant, then every pixel.  The accessor
// aborts on any index outside the frame.
static std::vector<uint8_t> apply(const AugRow& r, const std::vector<uint8_t>& in) {
    const int h = r.h, w = r.w;
    CHECK((long long)in.size() == (long long)h * w * 3);
    std::vector<uint8_t> out(in.size());
    std::vector<int> hist(AUG_HIST_WORDS, 0);
    for (int p = 0; p < h * w; ++p) {
        const int a = in[p * 3], b = in[p * 3 + 1], c = in[p * 3 + 2];
        ++hist[a]; ++hist[256 + b]; ++hist[512 + c]; ++hist[768 + aug_luma(a, b, c)];
    }
    const uint8_t* base = in.data();
    auto px = [base, h, w](int yy, int xx) {
        CHECK(yy >= 0 && yy < h && xx >= 0 && xx < w);
        return base + ((size_t)yy * w + xx) * 3;
    };
    const int fam = aug_family(r.op);
    uint8_t lut[3 * 256];
    if (fam == AUG_FAM_TABLE)
        for (int c = 0; c < 3; ++c) aug_build_table(r.op, r.iarg, hist.data() + c * 256, lut + c * 256);
    const int mean = r.op == AUG_CONTRAST ? aug_contrast_mean(hist.data() + 768) : 0;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const uint8_t* v = px(y, x);
            uint8_t* o = out.data() + ((size_t)y * w + x) * 3;
            if (fam == AUG_FAM_TABLE) {
                for (int c = 0; c < 3; ++c) o[c] = lut[c * 256 + v[c]];
            } else if (fam == AUG_FAM_BLEND) {
                const int d = r.op == AUG_BRIGHTNESS ? 0 : (r.op == AUG_COLOR ? aug_luma(v[0], v[1], v[2]) : mean);
                for (int c = 0; c < 3; ++c) o[c] = aug_blend(d, v[c], r.factor);
            } else if (fam == AUG_FAM_SHARP) {
                for (int c = 0; c < 3; ++c) {
                    int d = v[c];
                    if (y >= 1 && y < h - 1 && x >= 1 && x < w - 1) {
                        const int a[3] = {px(y - 1, x - 1)[c], px(y - 1, x)[c], px(y - 1, x + 1)[c]}, m[3] = {px(y, x - 1)[c], v[c], px(y, x + 1)[c]},
                                  b[3] = {px(y + 1, x - 1)[c], px(y + 1, x)[c], px(y + 1, x + 1)[c]};
                        d = aug_smooth(a, m, b);
                    }
                    o[c] = aug_blend(d, v[c], r.factor);
                }
            } else {
                aug_affine_pixel(r.c, r.filter, r.fill, w, h, x, y, px, o);
            }
        }
    return out;
}

static std::vector<uint8_t> noise(int h, int w, uint32_t seed) {
    std::vector<uint8_t> v((size_t)h * w * 3);
    uint32_t s = seed;
    for (auto& b : v) { s = s * 1664525u + 1013904223u; b = (uint8_t)(s >> 24); }
    return v;
}

static void walk_rows() {
    const int Hs = 64, Ws = 80;
    for (int op = 0; op < AUG_OPS; ++op) {
        AugRow r = make_row(op, 33, 57);
        CHECK(aug_row_ok(r, 0, Hs, Ws) && aug_last_ok(r));
        CHECK(!aug_row_ok(r, 1, Hs, Ws));                                      // only layer 0 reads the source
        r = make_row(op, 33, 57, 0, 1.0f, AUG_BILINEAR, AUG_BUF_DST, AUG_BUF_WORK);
        CHECK(aug_row_ok(r, 3, Hs, Ws) && !aug_row_ok(r, 0, Hs, Ws) && !aug_last_ok(r));
        r = make_row(op, 33, 57, 0, 1.0f, AUG_BICUBIC, AUG_BUF_WORK, AUG_BUF_WORK);
        CHECK(aug_row_ok(r, 1, Hs, Ws) == (aug_family(op) < AUG_FAM_SHARP));   // the neighbourhood operations never work in place
    }
    const AugRow base = make_row(AUG_AFFINE, 64, 80, 0, 0.5f, AUG_BICUBIC);
    CHECK(aug_row_ok(base, 0, Hs, Ws) && !aug_row_ok(base, 0, 63, Ws) && !aug_row_ok(base, 0, Hs, 79));
    AugRow r = base; r.h = 0; CHECK(!aug_row_ok(r, 0, Hs, Ws));
    r = base; r.w = 0; CHECK(!aug_row_ok(r, 0, Hs, Ws));
    r = base; r.h = 65; CHECK(!aug_row_ok(r, 0, Hs, Ws));
    r = base; r.op = AUG_OPS; CHECK(!aug_row_ok(r, 0, Hs, Ws));
    r = base; r.op = -1; CHECK(!aug_row_ok(r, 0, Hs, Ws));
    r = base; r.filter = 0; CHECK(!aug_row_ok(r, 0, Hs, Ws));
    r = base; r.filter = 4; CHECK(!aug_row_ok(r, 0, Hs, Ws));
    r = base; r.fill = -1; CHECK(!aug_row_ok(r, 0, Hs, Ws));
    r = base; r.fill = 0x1000000; CHECK(!aug_row_ok(r, 0, Hs, Ws));
    r = base; r.factor = NAN; CHECK(!aug_row_ok(r, 0, Hs, Ws));
    r = base; r.factor = -INFINITY; CHECK(!aug_row_ok(r, 0, Hs, Ws));
    r = base; r.factor = 3.0e38f; CHECK(aug_row_ok(r, 0, Hs, Ws));
    for (int k = 0; k < 6; ++k) {
        r = base; r.c[k] = NAN; CHECK(!aug_row_ok(r, 0, Hs, Ws));
        r = base; r.c[k] = INFINITY; CHECK(!aug_row_ok(r, 0, Hs, Ws));
        r = base; r.c[k] = AUG_MAX_COEFF * 2; CHECK(!aug_row_ok(r, 0, Hs, Ws));
        r = base; r.c[k] = -AUG_MAX_COEFF; CHECK(aug_row_ok(r, 0, Hs, Ws));
    }
    r = base; r.bufs = AUG_BUF_SRC; CHECK(!aug_row_ok(r, 0, Hs, Ws));             // destination 0: the source is never written
    r = base; r.bufs = AUG_BUF_SRC | 3 << 8; CHECK(!aug_row_ok(r, 0, Hs, Ws));
    r = base; r.bufs = 3 | AUG_BUF_DST << 8; CHECK(!aug_row_ok(r, 1, Hs, Ws));
    r = base; r.bufs |= 1 << 16; CHECK(!aug_row_ok(r, 0, Hs, Ws));
    r = make_row(AUG_SOLARIZE, 8, 8, 256); CHECK(aug_row_ok(r, 0, Hs, Ws)); r.iarg = 257; CHECK(!aug_row_ok(r, 0, Hs, Ws)); r.iarg = -1; CHECK(!aug_row_ok(r, 0, Hs, Ws));
    r = make_row(AUG_SOLARIZE_ADD, 8, 8, 255); CHECK(aug_row_ok(r, 0, Hs, Ws)); r.iarg = 256; CHECK(!aug_row_ok(r, 0, Hs, Ws));
    r = make_row(AUG_POSTERIZE, 8, 8, 8); CHECK(aug_row_ok(r, 0, Hs, Ws)); r.iarg = 9; CHECK(!aug_row_ok(r, 0, Hs, Ws));
    int rejected = 0;
    for (int fill : {INT_MIN, INT_MAX, -1}) {                                     // every word hostile at once
        AugRow hst;
        int words[AUG_ROW_WORDS];
        for (int i = 0; i < AUG_ROW_WORDS; ++i) words[i] = fill;
        memcpy(&hst, words, sizeof(hst));
        for (int layer = 0; layer < AUG_MAX_LAYERS; ++layer) { CHECK(!aug_row_ok(hst, layer, RS_MAX_SIDE, RS_MAX_SIDE)); ++rejected; }
    }
    // links
    const AugRow a = make_row(AUG_AFFINE, 33, 57, 0, 1.0f, AUG_BICUBIC, AUG_BUF_SRC, AUG_BUF_WORK), b = make_row(AUG_INVERT, 33, 57, 0, 1.0f, AUG_BICUBIC, AUG_BUF_WORK, AUG_BUF_WORK);
    const AugRow c = make_row(AUG_SHARPNESS, 33, 57, 0, 1.0f, AUG_BICUBIC, AUG_BUF_WORK, AUG_BUF_DST), d = make_row(AUG_INVERT, 33, 56, 0, 1.0f, AUG_BICUBIC, AUG_BUF_WORK, AUG_BUF_WORK);
    CHECK(aug_link_ok(a, b) && aug_link_ok(b, c) && aug_last_ok(c) && aug_link_ok(a, c) && !aug_link_ok(c, b) && !aug_link_ok(a, d) && !aug_last_ok(b));
    CHECK(aug_row_at(0, 0, 4, 2, 8) == AUG_HEADER_WORDS && aug_row_at(3, 1, 4, 2, 8) == AUG_HEADER_WORDS + (3 * 8 + 1) * AUG_ROW_WORDS);
    CHECK(aug_row_at(4, 0, 4, 2, 8) < 0 && aug_row_at(0, 2, 4, 2, 8) < 0 && aug_row_at(0, 8, 4, 9, 8) < 0 && aug_row_at(-1, 0, 4, 2, 8) < 0 && aug_row_at(0, -1, 4, 2, 8) < 0);
    printf("randaug check: rows ok (%d hostile rows rejected)\n", rejected);
}

static void walk_arithmetic() {
    long long pixels = 0;
    const int sizes[][2] = {{1, 1}, {2, 5}, {3, 3}, {5, 2}, {1, 7}, {33, 57}, {64, 40}};
    for (const auto& s : sizes) {
        const int h = s[0], w = s[1];
        const std::vector<uint8_t> in = noise(h, w, 7u + h * 131 + w);
        for (int filter : {AUG_BILINEAR, AUG_BICUBIC}) {
            AugRow r = make_row(AUG_AFFINE, h, w, 0, 1.0f, filter);
            CHECK(apply(r, in) == in);                                         // the identity matrix copies the frame
            // every extreme of a row that passes the check forms indices inside the frame only (the accessor aborts otherwise)
            const double ext[] = {AUG_MAX_COEFF, -AUG_MAX_COEFF, 4.9e-324, -0.0, 0.3, -1.0, 1e-9, (double)w, (double)-h, 0.5, -0.5};
            for (double e : ext)
                for (int k = 0; k < 6; ++k) {
                    AugRow q = r;
                    q.c[k] = e;
                    CHECK(aug_row_ok(q, 0, h, w));
                    pixels += (long long)apply(q, in).size() / 3;
                }
            AugRow q = r; q.c[2] = (double)w;                                  // everything moves out: the fill colour
            for (uint8_t v : apply(q, in)) CHECK(v == 128);
        }
        for (int op : {AUG_BRIGHTNESS, AUG_COLOR, AUG_CONTRAST, AUG_SHARPNESS, AUG_IDENTITY}) CHECK(apply(make_row(op, h, w, 0, 1.0f), in) == in);
        CHECK(apply(make_row(AUG_POSTERIZE, h, w, 8), in) == in && apply(make_row(AUG_SOLARIZE, h, w, 256), in) == in && apply(make_row(AUG_SOLARIZE_ADD, h, w, 0), in) == in);
        for (uint8_t v : apply(make_row(AUG_POSTERIZE, h, w, 0), in)) CHECK(v == 0);
        for (uint8_t v : apply(make_row(AUG_BRIGHTNESS, h, w, 0, 0.0f), in)) CHECK(v == 0);
        const std::vector<uint8_t> inv = apply(make_row(AUG_INVERT, h, w), in);
        CHECK(inv == apply(make_row(AUG_SOLARIZE, h, w, 0), in) && apply(make_row(AUG_INVERT, h, w), inv) == in);
        for (float f : {-5.0f, 0.0f, 0.1f, 1.9f, 7.0f, 3.0e38f, -3.0e38f})        // any finite factor
            for (int op : {AUG_BRIGHTNESS, AUG_COLOR, AUG_CONTRAST, AUG_SHARPNESS}) pixels += (long long)apply(make_row(op, h, w, 0, f), in).size() / 3;
        pixels += (long long)apply(make_row(AUG_EQUALIZE, h, w), in).size() / 3 + (long long)apply(make_row(AUG_AUTO_CONTRAST, h, w), in).size() / 3;
    }
    const int k[3] = {91, 91, 91};
    CHECK(aug_smooth(k, k, k) == 91);                                          // 0.5 + 13 * 91 / 13 truncates to 91
    CHECK(aug_luma(255, 255, 255) == 255 && aug_luma(0, 0, 0) == 0 && aug_luma(255, 0, 0) == 76 && aug_luma(0, 255, 0) == 150 && aug_luma(0, 0, 255) == 29);
    CHECK(aug_blend(0, 200, 1.9f) == 255 && aug_blend(255, 0, 1.9f) == 0 && aug_blend(100, 200, 0.5f) == 150 && aug_blend(10, 11, 0.37f) == 10);
    CHECK(aug_clip8d(-0.5) == 0 && aug_clip8d(254.999) == 254 && aug_clip8d(255.0) == 255 && aug_clip8d(1e300) == 255 && aug_clip8f(0.99f) == 0);
    int hist[256] = {0};
    hist[0] = 10; hist[200] = 3000; hist[255] = 62;
    uint8_t lut[256];
    aug_build_table(AUG_EQUALIZE, 0, hist, lut);
    CHECK(lut[0] == 0 && lut[1] == 1 && lut[200] == 1 && lut[201] == 255 && lut[255] == 255);   // step 11: the clamp to 255 binds
    aug_build_table(AUG_AUTO_CONTRAST, 0, hist, lut);
    CHECK(lut[0] == 0 && lut[255] == 255 && lut[100] == 100);
    int one[256] = {0};
    one[77] = 500;
    aug_build_table(AUG_AUTO_CONTRAST, 0, one, lut);
    CHECK(lut[77] == 77 && lut[0] == 0);                                       // hi <= lo: the identity
    aug_build_table(AUG_EQUALIZE, 0, one, lut);
    CHECK(lut[77] == 77 && lut[255] == 255);
    CHECK(aug_contrast_mean(one) == 77 && aug_contrast_mean(hist) == (int)((200.0 * 3000 + 255.0 * 62) / 3072 + 0.5));
    printf("randaug check: arithmetic ok (%lld pixels)\n", pixels);
}

static void walk_refusals() {
    CHECK(!aug_ptr_error(0x1000, 0x2000, 0x3000, 0x4000, 0x5000));
    CHECK(aug_ptr_error(0, 0x2000, 0x3000, 0x4000, 0x5000) && aug_ptr_error(0x1000, 0, 0x3000, 0x4000, 0x5000) && aug_ptr_error(0x1000, 0x2000, 0, 0x4000, 0x5000));
    CHECK(aug_ptr_error(0x1000, 0x2000, 0x3000, 0, 0x5000) && aug_ptr_error(0x1000, 0x2000, 0x3000, 0x4000, 0));
    CHECK(aug_ptr_error(0x1008, 0x2000, 0x3000, 0x4000, 0x5000) && aug_ptr_error(0x1000, 0x2004, 0x3000, 0x4000, 0x5000) && aug_ptr_error(0x1000, 0x2000, 0x3001, 0x4000, 0x5000));
    CHECK(aug_ptr_error(0x1000, 0x2000, 0x3000, 0x4008, 0x5000) && aug_ptr_error(0x1000, 0x2000, 0x3000, 0x4000, 0x5004));
    CHECK(aug_ptr_error(0x1000, 0x1000, 0x3000, 0x4000, 0x5000) && aug_ptr_error(0x1000, 0x2000, 0x1000, 0x4000, 0x5000) && aug_ptr_error(0x1000, 0x2000, 0x2000, 0x4000, 0x5000));
    CHECK(!aug_shape_error(2, 2, 64, 64, 4, 4) && !aug_shape_error(1, 1, 4096, 4096, 1, 1) && !aug_shape_error(65535, 1, 1, 1, 65535, 8) && !aug_shape_error(1, 65535, 1, 1, 1, 1));
    CHECK(aug_shape_error(0, 2, 64, 64, 4, 4) && aug_shape_error(2, 0, 64, 64, 4, 4) && aug_shape_error(2, 2, 64, 64, 4, 0) && aug_shape_error(2, 2, 64, 64, 4, 9));
    CHECK(aug_shape_error(-1, 2, 64, 64, 4, 4) && aug_shape_error(2, -1, 64, 64, 4, 4) && aug_shape_error(2, 2, 64, 64, 4, -1));
    CHECK(aug_shape_error(256, 256, 64, 64, 256, 4) && !aug_shape_error(255, 257, 64, 64, 255, 4) && aug_shape_error(65536, 1, 64, 64, 70000, 4) && aug_shape_error(INT_MAX, INT_MAX, 64, 64, INT_MAX, 4));
    CHECK(aug_shape_error(2, 2, 0, 64, 4, 4) && aug_shape_error(2, 2, 64, 0, 4, 4) && aug_shape_error(2, 2, 4097, 64, 4, 4) && aug_shape_error(2, 2, 64, 4097, 4, 4));
    CHECK(aug_shape_error(5, 2, 64, 64, 4, 4) && aug_shape_error(1, 2, 64, 64, 0, 4));
    printf("randaug check: refusals ok\n");
}

static bool read_ints(FILE* f, std::vector<int>& v, size_t n) {
    v.resize(n);
    for (size_t i = 0; i < n; ++i)
        if (fscanf(f, "%d", &v[i]) != 1) return false;
    return true;
}

static int walk_file(const char* path) {
    FILE* f = fopen(path, "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return 2; }
    char kind[8];
    int tables = 0, means = 0, frames = 0;
    long long bad = 0;
    while (fscanf(f, "%7s", kind) == 1) {
        if (!strcmp(kind, "T")) {
            int op, iarg;
            std::vector<int> hist, want;
            CHECK(fscanf(f, "%d %d", &op, &iarg) == 2 && read_ints(f, hist, 256) && read_ints(f, want, 256));
            uint8_t lut[256];
            aug_build_table(op, iarg, hist.data(), lut);
            for (int i = 0; i < 256; ++i)
                if (want[i] >= 0 && want[i] != lut[i]) { ++bad; fprintf(stderr, "table %d: entry %d is %d, Pillow used %d\n", tables, i, lut[i], want[i]); }
            ++tables;
        } else if (!strcmp(kind, "C")) {
            int mean;
            std::vector<int> hist;
            CHECK(fscanf(f, "%d", &mean) == 1 && read_ints(f, hist, 256));
            if (aug_contrast_mean(hist.data()) != mean) { ++bad; fprintf(stderr, "mean %d: %d, Pillow used %d\n", means, aug_contrast_mean(hist.data()), mean); }
            ++means;
        } else if (!strcmp(kind, "P")) {
            int op, iarg, filter, h, w;
            char num[7][64];
            CHECK(fscanf(f, "%d %d %63s %d %63s %63s %63s %63s %63s %63s %d %d", &op, &iarg, num[0], &filter, num[1], num[2], num[3], num[4], num[5], num[6], &h, &w) == 12);
            AugRow r = make_row(op, h, w, iarg, (float)strtod(num[0], nullptr), filter);
            for (int k = 0; k < 6; ++k) r.c[k] = strtod(num[1 + k], nullptr);
            CHECK(aug_row_ok(r, 0, h, w));
            std::vector<int> a, b;
            CHECK(read_ints(f, a, (size_t)h * w * 3) && read_ints(f, b, (size_t)h * w * 3));
            const std::vector<uint8_t> got = apply(r, std::vector<uint8_t>(a.begin(), a.end()));
            long long n = 0;
            for (size_t i = 0; i < got.size(); ++i) n += got[i] != b[i];
            if (n) { bad += n; fprintf(stderr, "frame %d (op %d): %lld bytes differ\n", frames, op, n); }
            ++frames;
        } else {
            fprintf(stderr, "unknown record %s\n", kind);
            fclose(f);
            return 2;
        }
    }
    fclose(f);
    printf("randaug check: file ok (%d tables, %d means, %d frames, %lld bytes differ)\n", tables, means, frames, bad);
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 5 + AUG_ROW_WORDS && !strcmp(argv[1], "row")) {   // row LAYER HS WS and the row's 20 words: prints aug_row_ok
        int words[AUG_ROW_WORDS];
        for (int k = 0; k < AUG_ROW_WORDS; ++k) words[k] = (int)(uint32_t)strtoul(argv[5 + k], nullptr, 16);
        AugRow r;
        memcpy(&r, words, sizeof(r));
        printf("%d\n", aug_row_ok(r, atoi(argv[2]), atoi(argv[3]), atoi(argv[4])) ? 1 : 0);
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "file")) return walk_file(argv[2]);
    walk_rows();
    walk_arithmetic();
    walk_refusals();
    printf("randaug check: all ok\n");
    return 0;
}
