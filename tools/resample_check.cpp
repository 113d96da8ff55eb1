// CPU walk of the device resample's host logic (dynamic-tuning_amd/csrc/resample.h), without a GPU and without input files:
//   * resample_row_ok for valid rows of every kind, each single violation of its conditions, and hostile words (INT_MIN / INT_MAX in every
//     field): a row that passes can be indexed with, which the walk proves by forming every extreme index in 64-bit;
//   * resample_unit: the row an image reads, never outside the table;
//   * resample_coeffs against a brute-force restatement of Pillow's precompute_coeffs + normalize_coeffs_8bpc on heap arrays of ksize
//     doubles per position, integer for integer, over box / full pairs from 1 pixel to 4096, up- and downsampling up to the 2.5 bound;
//     the tap count never exceeds RS_KMAX, taps never leave the box, the coefficients of a position sum to 2^22 within the rounding;
//   * resample_clip8 and every argument check the entries make, with the valid neighbours.
// `resample_check coeffs IN OUT XX` prints the first tap, the tap count and the 11 coefficients of one position, for a comparison against
// another restatement.
// Build and run (host only):
//   c++ -std=c++17 -O2 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I dynamic-tuning_amd/csrc tools/resample_check.cpp
//     -o /tmp/resample_check && /tmp/resample_check
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "resample.h"

using namespace dyt;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            abort();                                                                 \
        }                                                                            \
    } while (0)

static ResampleRow make_row(int sh, int sw, int t, int l, int bh, int bw, int fh, int fw, int oy, int ox, int flags = 0) {
    ResampleRow r;
    r.src_h = sh; r.src_w = sw; r.top = t; r.left = l; r.box_h = bh; r.box_w = bw;
    r.full_h = fh; r.full_w = fw; r.off_y = oy; r.off_x = ox; r.flags = flags; r.pad = 0;
    return r;
}

// what a kernel forms from a row that passed: all of it must lie inside the batch's padded shape and the 224 x 224 window inside `full`
static void index_walk(const ResampleRow& r, int Hs, int Ws) {
    const long long last_row = (long long)r.top + r.box_h - 1, last_col = (long long)r.left + r.box_w - 1;
    CHECK(r.top >= 0 && r.left >= 0 && last_row < r.src_h && last_col < r.src_w && r.src_h <= Hs && r.src_w <= Ws);
    CHECK((long long)r.off_y + RS_OUT <= r.full_h && (long long)r.off_x + RS_OUT <= r.full_w);
    for (int axis = 0; axis < 2; ++axis) {
        const int in = axis ? r.box_w : r.box_h, out = axis ? r.full_w : r.full_h, off = axis ? r.off_x : r.off_y;
        for (int t : {0, 1, 111, 222, 223}) {
            int lo, n, k[RS_KMAX];
            resample_coeffs(in, out, off + t, lo, n, k);
            CHECK(lo >= 0 && n >= 1 && n <= RS_KMAX && lo + n <= in);
        }
    }
}

static void walk_rows() {
    const int Hs = 512, Ws = 640;
    const std::vector<ResampleRow> good = {
        make_row(512, 640, 0, 0, 512, 560, 224, 224, 0, 0),            // scale 2.29 / 2.5: the bound itself
        make_row(300, 400, 0, 0, 300, 400, 256, 341, 16, 58),          // the evaluation row
        make_row(64, 64, 63, 63, 1, 1, 224, 224, 0, 0, 1),             // 1 x 1 box in the last corner, mirrored
        make_row(1, 1, 0, 0, 1, 1, 224, 224, 0, 0),
        make_row(512, 640, 288, 416, 224, 224, 224, 224, 0, 0),        // identity
        make_row(500, 333, 10, 20, 8, 10, 224, 224, 0, 0),             // upsampling
        make_row(512, 640, 0, 0, 512, 640, 1000, 1000, 776, 776),      // a window in the far corner of a large `full`
        make_row(512, 640, 0, 0, 512, 640, INT_MAX, INT_MAX, INT_MAX - 224, INT_MAX - 224),
    };
    for (const ResampleRow& r : good) { CHECK(resample_row_ok(r, Hs, Ws)); index_walk(r, Hs, Ws); }
    const ResampleRow base = make_row(300, 400, 10, 20, 200, 300, 256, 341, 16, 58);
    CHECK(resample_row_ok(base, Hs, Ws));
    CHECK(!resample_row_ok(base, 299, Ws) && !resample_row_ok(base, Hs, 399) && resample_row_ok(base, 300, 400));
    int* w = nullptr;
    const int bad_values[] = {INT_MIN, INT_MIN + 1, -1, 0, INT_MAX, INT_MAX - 1, 1 << 30, 4097};
    int rejected = 0, accepted = 0;
    for (int field = 0; field < 10; ++field)
        for (int v : bad_values) {
            ResampleRow r = base;
            w = &r.src_h + field;
            *w = v;
            if (resample_row_ok(r, Hs, Ws)) { index_walk(r, Hs, Ws); ++accepted; }
            else ++rejected;
        }
    CHECK(rejected == 68 && accepted == 12);
    // each condition, violated by one
    ResampleRow r = base; r.top = 101; CHECK(!resample_row_ok(r, Hs, Ws));                 // box below the valid extent
    r = base; r.left = 101; CHECK(!resample_row_ok(r, Hs, Ws));
    r = base; r.box_h = 0; CHECK(!resample_row_ok(r, Hs, Ws));
    r = base; r.box_w = 0; CHECK(!resample_row_ok(r, Hs, Ws));
    r = base; r.full_h = 223; r.off_y = 0; CHECK(!resample_row_ok(r, Hs, Ws));
    r = base; r.full_w = 223; r.off_x = 0; CHECK(!resample_row_ok(r, Hs, Ws));
    r = base; r.off_y = 33; CHECK(!resample_row_ok(r, Hs, Ws));                            // 33 + 224 > 256
    r = base; r.off_y = 32; CHECK(resample_row_ok(r, Hs, Ws));
    r = base; r.off_x = 118; CHECK(!resample_row_ok(r, Hs, Ws));
    r = base; r.off_x = -1; CHECK(!resample_row_ok(r, Hs, Ws));
    r = make_row(512, 640, 0, 0, 512, 561, 224, 224, 0, 0); CHECK(!resample_row_ok(r, Hs, Ws));   // 561 > 2.5 * 224
    r = make_row(512, 640, 0, 0, 512, 560, 224, 224, 0, 0); CHECK(resample_row_ok(r, Hs, Ws));
    for (int fill : {INT_MIN, INT_MAX, -1}) {                                              // every word hostile at once
        ResampleRow h;
        int* p = &h.src_h;
        for (int i = 0; i < RS_ROW_WORDS; ++i) p[i] = fill;
        CHECK(!resample_row_ok(h, Hs, Ws));
    }
    for (int n = -2; n < 20; ++n)
        for (int units : {INT_MIN, -1, 0, 1, 4, 1000, INT_MAX})
            for (int capacity : {0, 1, 4, 16}) {
                const int u = resample_unit(n, units, capacity);
                CHECK(u >= -1 && u < capacity);
                if (n >= 0 && n < capacity && n < units) CHECK(u == n);
                else CHECK(u == -1);
            }
    printf("resample check: rows ok (%d hostile rows rejected, %d accepted and indexed)\n", rejected, accepted);
}

// Pillow's precompute_coeffs + normalize_coeffs_8bpc for the bicubic filter, as written there (heap arrays, ksize per position)
static double brute_filter(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}
static int brute_coeffs(int inSize, int outSize, std::vector<int>& bounds, std::vector<int>& kk_out) {
    double filterscale, scale;
    filterscale = scale = (double)inSize / outSize;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = 2.0 * filterscale;
    const int ksize = (int)ceil(support) * 2 + 1;
    std::vector<double> kk((size_t)outSize * ksize);
    bounds.assign((size_t)outSize * 2, 0);
    for (int xx = 0; xx < outSize; xx++) {
        const double center = 0 + (xx + 0.5) * scale;
        double ww = 0.0;
        const double ss = 1.0 / filterscale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > inSize) xmax = inSize;
        xmax -= xmin;
        double* k = &kk[(size_t)xx * ksize];
        int x;
        for (x = 0; x < xmax; x++) {
            const double w = brute_filter((x + xmin - center + 0.5) * ss);
            k[x] = w;
            ww += w;
        }
        for (x = 0; x < xmax; x++)
            if (ww != 0.0) k[x] /= ww;
        for (; x < ksize; x++) k[x] = 0;
        bounds[xx * 2 + 0] = xmin;
        bounds[xx * 2 + 1] = xmax;
    }
    kk_out.assign((size_t)outSize * ksize, 0);
    for (size_t x = 0; x < (size_t)outSize * ksize; x++) {
        if (kk[x] < 0) kk_out[x] = (int)(-0.5 + kk[x] * (1 << RS_PRECISION_BITS));
        else kk_out[x] = (int)(0.5 + kk[x] * (1 << RS_PRECISION_BITS));
    }
    return ksize;
}

static void walk_coeffs() {
    const int pairs[][2] = {{1, 224}, {2, 224}, {3, 224}, {8, 224}, {10, 224}, {64, 224}, {223, 224}, {224, 224}, {225, 224}, {256, 224},
                            {300, 256}, {400, 341}, {490, 224}, {512, 224}, {559, 224}, {560, 224}, {4096, 1639}, {4096, 4096}, {17, 4096},
                            {333, 500}, {500, 333}, {640, 256}, {1, 1000}, {2500, 1000}};
    long long positions = 0;
    int widest = 0, widest_ksize = 0;
    for (const auto& p : pairs) {
        const int in = p[0], out = p[1];
        CHECK(2LL * in <= 5LL * out);
        std::vector<int> bounds, kk;
        const int ksize = brute_coeffs(in, out, bounds, kk);
        CHECK(ksize <= RS_KMAX);
        widest_ksize = ksize > widest_ksize ? ksize : widest_ksize;
        for (int xx = 0; xx < out; ++xx) {
            int lo, n, k[RS_KMAX];
            resample_coeffs(in, out, xx, lo, n, k);
            CHECK(lo == bounds[xx * 2] && n == bounds[xx * 2 + 1]);
            CHECK(lo >= 0 && n >= 1 && n <= ksize && lo + n <= in);
            long long sum = 0;
            for (int x = 0; x < RS_KMAX; ++x) {
                CHECK(k[x] == (x < ksize ? kk[(size_t)xx * ksize + x] : 0));
                if (x >= n) CHECK(k[x] == 0);
                sum += k[x];
            }
            CHECK(sum >= (1 << RS_PRECISION_BITS) - RS_KMAX && sum <= (1 << RS_PRECISION_BITS) + RS_KMAX);
            widest = n > widest ? n : widest;
            ++positions;
        }
    }
    CHECK(widest == RS_KMAX - 1 && widest_ksize == RS_KMAX);   // ksize = ceil(2 * 2.5) * 2 + 1 = 11 words per position, of which at most 2 * 5 are taps
    // identity: one tap of 2^22 per position
    for (int xx = 0; xx < 224; ++xx) {
        int lo, n, k[RS_KMAX];
        resample_coeffs(224, 224, xx, lo, n, k);
        for (int x = 0; x < n; ++x) CHECK(k[x] == ((lo + x == xx) ? (1 << RS_PRECISION_BITS) : 0));
    }
    printf("resample check: coefficients ok (%lld positions, widest %d taps)\n", positions, widest);
}

static void walk_refusals() {
    CHECK(resample_clip8(1 << 21) == 0 && resample_clip8((255 << 22) + (1 << 21)) == 255 && resample_clip8(INT_MAX) == 255);
    CHECK(resample_clip8(-1) == 0 && resample_clip8(INT_MIN) == 0 && resample_clip8((7 << 22) - 1) == 6 && resample_clip8(7 << 22) == 7);
    CHECK(!resample_ptr_error(0x1000, 0x2000, 0x3000, 0x4000));
    CHECK(resample_ptr_error(0, 0x2000, 0x3000, 0x4000) && resample_ptr_error(0x1000, 0, 0x3000, 0x4000));
    CHECK(resample_ptr_error(0x1000, 0x2000, 0, 0x4000) && resample_ptr_error(0x1000, 0x2000, 0x3000, 0));
    CHECK(resample_ptr_error(0x1004, 0x2000, 0x3000, 0x4000) && resample_ptr_error(0x1000, 0x2008, 0x3000, 0x4000));
    CHECK(resample_ptr_error(0x1000, 0x2000, 0x3004, 0x4000) && resample_ptr_error(0x1000, 0x2000, 0x3000, 0x4001));
    CHECK(!resample_shape_error(4, 64, 64, 4) && !resample_shape_error(1, 4096, 4096, 128) && !resample_shape_error(1, 1, 1, 1));
    CHECK(resample_shape_error(0, 64, 64, 4) && resample_shape_error(5, 64, 64, 4) && resample_shape_error(4, 0, 64, 4));
    CHECK(resample_shape_error(4, 64, 4097, 4) && resample_shape_error(4, 4097, 64, 4) && resample_shape_error(4, 64, -1, 4));
    CHECK(resample_shape_error(1, 64, 64, 0) && resample_shape_error(-1, 64, 64, 4));
    CHECK(resample_scratch_bytes(1) == 2 * 13 * 224 * 4 && resample_scratch_bytes(128) == 128LL * 23296 && resample_scratch_bytes(0) == 0);
    CHECK(!resample_scratch_error(4, 4 * 23296) && resample_scratch_error(4, 4 * 23296 - 1) && resample_scratch_error(1, 0));
    printf("resample check: refusals ok\n");
}

int main(int argc, char** argv) {
    if (argc == 5 && !strcmp(argv[1], "coeffs")) {
        int lo, n, k[RS_KMAX];
        resample_coeffs(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), lo, n, k);
        printf("%d %d", lo, n);
        for (int x = 0; x < RS_KMAX; ++x) printf(" %d", k[x]);
        printf("\n");
        return 0;
    }
    walk_rows();
    walk_coeffs();
    walk_refusals();
    printf("resample check: all ok\n");
    return 0;
}
