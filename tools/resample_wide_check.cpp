// CPU walk of the wide-tap resample's host logic (dynamic-tuning_amd/csrc/resample_wide.h), without a GPU and without input files:
//   * resample_wide_row_ok for valid rows of every kind -- among them the ones resample_row_ok refuses for their scale alone --, each
//     single violation of its conditions, and hostile words (INT_MIN / INT_MAX in every field): a row that passes can be indexed with,
//     which the walk proves by forming every extreme index in 64-bit; on every row both functions take they agree;
//   * resample_wide_coeffs against a brute-force restatement of Pillow's precompute_coeffs + normalize_coeffs_8bpc on heap arrays of ksize
//     doubles per position, integer for integer, over box / full pairs from 1 pixel to 4096 at scales up to 4096 / 224; the tap count
//     never exceeds RSW_KMAX, taps never leave the box, 2^21 + 255 * sum|k| stays inside int32; and against resample_coeffs wherever the
//     narrow function applies: the same first tap, tap count and first 11 integers, zeros behind them;
//   * the scratch size and every argument check the entries make, with the valid neighbours.
// `resample_wide_check coeffs IN OUT XX` prints the first tap, the tap count and the 75 coefficients of one position;
// `resample_wide_check narrow IN OUT XX` what resample.h's resample_coeffs gives (first tap, tap count, 11 coefficients).
// Build and run (host only):
//   c++ -std=c++17 -O2 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I dynamic-tuning_amd/csrc tools/resample_wide_check.cpp
//     -o /tmp/resample_wide_check && /tmp/resample_wide_check
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "resample_wide.h"

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
    CHECK(Hs <= RS_MAX_SIDE && Ws <= RS_MAX_SIDE);
    CHECK(r.top >= 0 && r.left >= 0 && last_row < r.src_h && last_col < r.src_w && r.src_h <= Hs && r.src_w <= Ws);
    CHECK((long long)r.off_y + RS_OUT <= r.full_h && (long long)r.off_x + RS_OUT <= r.full_w);
    for (int axis = 0; axis < 2; ++axis) {
        const int in = axis ? r.box_w : r.box_h, out = axis ? r.full_w : r.full_h, off = axis ? r.off_x : r.off_y;
        int prev_lo = 0, prev_hi = 0;
        for (int t = 0; t < RS_OUT; ++t) {
            int lo, n, k[RSW_KMAX];
            resample_wide_coeffs(in, out, off + t, lo, n, k);
            CHECK(lo >= 0 && n >= 1 && n <= RSW_KMAX && lo + n <= in);
            CHECK(lo >= prev_lo && lo + n >= prev_hi);   // both bounds grow with the position: the horizontal pass relies on it
            prev_lo = lo;
            prev_hi = lo + n;
        }
    }
}

static void walk_rows() {
    const int Hs = 4096, Ws = 4000;
    const std::vector<ResampleRow> good = {
        make_row(4096, 4000, 0, 0, 4096, 4000, 224, 224, 0, 0),        // the largest scale: 18.29
        make_row(700, 700, 0, 0, 700, 700, 256, 256, 16, 16),          // Resize(256) + CenterCrop(224) of 700 x 700
        make_row(1200, 1300, 7, 13, 561, 1100, 224, 224, 0, 0, 1),     // one pixel above the narrow bound, mirrored
        make_row(375, 1242, 0, 0, 375, 1242, 224, 224, 0, 0),          // Resize((224, 224)) of a 375 x 1242 image
        make_row(512, 640, 0, 0, 512, 560, 224, 224, 0, 0),            // the narrow bound itself
        make_row(300, 400, 0, 0, 300, 400, 256, 341, 16, 58),          // the narrow evaluation row
        make_row(64, 64, 63, 63, 1, 1, 224, 224, 0, 0, 1),             // 1 x 1 box in the last corner
        make_row(1, 1, 0, 0, 1, 1, 224, 224, 0, 0),
        make_row(32, 32, 0, 0, 32, 32, 224, 224, 0, 0),                // upsampling
        make_row(4096, 8, 0, 0, 4096, 8, 224, 224, 0, 0),              // a strip: 74 taps down, an upscale across
        make_row(512, 640, 0, 0, 512, 640, INT_MAX, INT_MAX, INT_MAX - 224, INT_MAX - 224),
    };
    int beyond = 0;
    for (const ResampleRow& r : good) {
        CHECK(resample_wide_row_ok(r, Hs, Ws));
        index_walk(r, Hs, Ws);
        if (!resample_row_ok(r, Hs, Ws)) ++beyond;
    }
    CHECK(beyond == 5);   // the first four and the strip
    const ResampleRow base = make_row(300, 400, 10, 20, 200, 300, 256, 341, 16, 58);
    CHECK(resample_wide_row_ok(base, Hs, Ws));
    CHECK(!resample_wide_row_ok(base, 299, Ws) && !resample_wide_row_ok(base, Hs, 399) && resample_wide_row_ok(base, 300, 400));
    CHECK(!resample_wide_row_ok(base, 4097, Ws) && !resample_wide_row_ok(base, Hs, 4097));   // a batch the entries refuse
    int* w = nullptr;
    const int bad_values[] = {INT_MIN, INT_MIN + 1, -1, 0, INT_MAX, INT_MAX - 1, 1 << 30, 4097};
    int rejected = 0, accepted = 0;
    for (int field = 0; field < 10; ++field)
        for (int v : bad_values) {
            ResampleRow r = base;
            w = &r.src_h + field;
            *w = v;
            const bool ok = resample_wide_row_ok(r, 512, 640);
            CHECK(ok == resample_row_ok(r, 512, 640));    // no variant of this row is refused for its scale alone
            if (ok) { index_walk(r, 512, 640); ++accepted; }
            else ++rejected;
        }
    CHECK(rejected == 68 && accepted == 12);
    // each condition, violated by one
    ResampleRow r = base; r.top = 101; CHECK(!resample_wide_row_ok(r, Hs, Ws));                 // box below the valid extent
    r = base; r.left = 101; CHECK(!resample_wide_row_ok(r, Hs, Ws));
    r = base; r.box_h = 0; CHECK(!resample_wide_row_ok(r, Hs, Ws));
    r = base; r.box_w = 0; CHECK(!resample_wide_row_ok(r, Hs, Ws));
    r = base; r.full_h = 223; r.off_y = 0; CHECK(!resample_wide_row_ok(r, Hs, Ws));
    r = base; r.full_w = 223; r.off_x = 0; CHECK(!resample_wide_row_ok(r, Hs, Ws));
    r = base; r.off_y = 33; CHECK(!resample_wide_row_ok(r, Hs, Ws));                            // 33 + 224 > 256
    r = base; r.off_y = 32; CHECK(resample_wide_row_ok(r, Hs, Ws));
    r = base; r.off_x = 118; CHECK(!resample_wide_row_ok(r, Hs, Ws));
    r = base; r.off_x = -1; CHECK(!resample_wide_row_ok(r, Hs, Ws));
    r = make_row(512, 640, 0, 0, 512, 561, 224, 224, 0, 0);                                     // 561 > 2.5 * 224: the one difference
    CHECK(!resample_row_ok(r, 512, 640) && resample_wide_row_ok(r, 512, 640));
    for (int fill : {INT_MIN, INT_MAX, -1}) {                                                   // every word hostile at once
        ResampleRow h;
        int* p = &h.src_h;
        for (int i = 0; i < RS_ROW_WORDS; ++i) p[i] = fill;
        CHECK(!resample_wide_row_ok(h, Hs, Ws));
    }
    printf("resample wide check: rows ok (%d hostile rows rejected, %d accepted and indexed, %d valid rows beyond the narrow bound)\n",
           rejected, accepted, beyond);
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
    const int pairs[][2] = {{1, 224}, {2, 224}, {8, 224}, {32, 224}, {223, 224}, {224, 224}, {225, 224}, {300, 256}, {400, 341}, {512, 224},
                            {559, 224}, {560, 224}, {561, 224}, {600, 224}, {640, 239}, {700, 256}, {1100, 224}, {1242, 224}, {375, 224},
                            {1500, 224}, {1600, 341}, {2400, 256}, {3000, 224}, {4095, 224}, {4096, 224}, {4096, 225}, {4096, 1639},
                            {4096, 4096}, {17, 4096}, {2500, 1000}};
    long long positions = 0, shared = 0, largest_abs = 0;
    int widest = 0, widest_ksize = 0;
    for (const auto& p : pairs) {
        const int in = p[0], out = p[1];
        CHECK(in <= RS_MAX_SIDE && out >= RS_OUT);
        std::vector<int> bounds, kk;
        const int ksize = brute_coeffs(in, out, bounds, kk);
        CHECK(ksize <= RSW_KMAX);
        widest_ksize = ksize > widest_ksize ? ksize : widest_ksize;
        const bool narrow = 2LL * in <= 5LL * out;
        for (int xx = 0; xx < out; ++xx) {
            int lo, n, k[RSW_KMAX];
            resample_wide_coeffs(in, out, xx, lo, n, k);
            CHECK(lo == bounds[xx * 2] && n == bounds[xx * 2 + 1]);
            CHECK(lo >= 0 && n >= 1 && n <= ksize && lo + n <= in);
            long long sum = 0, abs_sum = 0;
            for (int x = 0; x < RSW_KMAX; ++x) {
                CHECK(k[x] == (x < ksize ? kk[(size_t)xx * ksize + x] : 0));
                if (x >= n) CHECK(k[x] == 0);
                sum += k[x];
                abs_sum += k[x] < 0 ? -(long long)k[x] : k[x];
            }
            CHECK(sum >= (1 << RS_PRECISION_BITS) - RSW_KMAX && sum <= (1 << RS_PRECISION_BITS) + RSW_KMAX);
            CHECK((1LL << 21) + 255 * abs_sum < (1LL << 31));   // Pillow's int32 accumulator, and the kernels', never wraps
            largest_abs = abs_sum > largest_abs ? abs_sum : largest_abs;
            widest = n > widest ? n : widest;
            if (narrow) {                                        // resample.h's function gives the same integers
                int lo11, n11, k11[RS_KMAX];
                resample_coeffs(in, out, xx, lo11, n11, k11);
                CHECK(lo11 == lo && n11 == n);
                for (int x = 0; x < RSW_KMAX; ++x) CHECK(k[x] == (x < RS_KMAX ? k11[x] : 0));
                ++shared;
            }
            ++positions;
        }
    }
    CHECK(widest == RSW_KMAX - 1 && widest_ksize == RSW_KMAX);   // ksize = ceil(2 * 4096 / 224) * 2 + 1 = 75 words, of which at most 74 are taps
    printf("resample wide check: coefficients ok (%lld positions, %lld of them shared with the 11-tap function, widest %d taps, "
           "largest sum|k| %.4f x 2^22)\n", positions, shared, widest, (double)largest_abs / (double)(1 << RS_PRECISION_BITS));
}

static void walk_refusals() {
    const long long per_image = 2LL * 77 * 224 * 4;
    CHECK(RSW_COEFF_FIELDS == 77 && RSW_COEFF_WORDS * 4LL == per_image && per_image == 137984);
    CHECK(resample_wide_scratch_bytes(1, 1) == per_image + 672 && resample_wide_scratch_bytes(4, 700) == 4 * (per_image + 700LL * 672));
    CHECK(resample_wide_scratch_bytes(128, 4096) == 128 * (per_image + 4096LL * 672));
    CHECK(resample_wide_scratch_bytes(0, 64) == 0 && resample_wide_scratch_bytes(-3, 64) == 0 && resample_wide_scratch_bytes(4, 0) == 0);
    CHECK(resample_wide_scratch_bytes(4, 4097) == 0 && resample_wide_scratch_bytes(4, 64) % 16 == 0 && resample_wide_coeff_bytes(3) % 16 == 0);
    const long long need = resample_wide_scratch_bytes(4, 64);
    CHECK(!resample_wide_scratch_error(4, 64, need) && resample_wide_scratch_error(4, 64, need - 1) && resample_wide_scratch_error(1, 1, 0));
    CHECK(!resample_wide_args_error(0x1000, 0x2000, 0x3000, 0x4000, 4, 64, 64, 4, need));
    CHECK(!resample_wide_args_error(0x1000, 0x2000, 0x3000, 0x4000, 1, 4096, 4096, 128, resample_wide_scratch_bytes(1, 4096)));
    CHECK(resample_wide_args_error(0, 0x2000, 0x3000, 0x4000, 4, 64, 64, 4, need) && resample_wide_args_error(0x1000, 0, 0x3000, 0x4000, 4, 64, 64, 4, need));
    CHECK(resample_wide_args_error(0x1000, 0x2000, 0, 0x4000, 4, 64, 64, 4, need) && resample_wide_args_error(0x1000, 0x2000, 0x3000, 0, 4, 64, 64, 4, need));
    CHECK(resample_wide_args_error(0x1008, 0x2000, 0x3000, 0x4000, 4, 64, 64, 4, need) && resample_wide_args_error(0x1000, 0x2004, 0x3000, 0x4000, 4, 64, 64, 4, need));
    CHECK(resample_wide_args_error(0x1000, 0x2000, 0x3004, 0x4000, 4, 64, 64, 4, need) && resample_wide_args_error(0x1000, 0x2000, 0x3000, 0x4002, 4, 64, 64, 4, need));
    CHECK(resample_wide_args_error(0x1000, 0x2000, 0x3000, 0x4000, 0, 64, 64, 4, need) && resample_wide_args_error(0x1000, 0x2000, 0x3000, 0x4000, 5, 64, 64, 4, 2 * need));
    CHECK(resample_wide_args_error(0x1000, 0x2000, 0x3000, 0x4000, 4, 0, 64, 4, need) && resample_wide_args_error(0x1000, 0x2000, 0x3000, 0x4000, 4, 64, 4097, 4, need));
    CHECK(resample_wide_args_error(0x1000, 0x2000, 0x3000, 0x4000, 4, 4097, 64, 4, 1LL << 40) && resample_wide_args_error(0x1000, 0x2000, 0x3000, 0x4000, 1, 64, 64, 0, need));
    CHECK(resample_wide_args_error(0x1000, 0x2000, 0x3000, 0x4000, 4, 64, 64, 4, need - 1) && resample_wide_args_error(0x1000, 0x2000, 0x3000, 0x4000, 4, 65, 64, 4, need));
    printf("resample wide check: refusals ok\n");
}

int main(int argc, char** argv) {
    if (argc == 5 && !strcmp(argv[1], "coeffs")) {
        int lo, n, k[RSW_KMAX];
        resample_wide_coeffs(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), lo, n, k);
        printf("%d %d", lo, n);
        for (int x = 0; x < RSW_KMAX; ++x) printf(" %d", k[x]);
        printf("\n");
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "narrow")) {
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
    printf("resample wide check: all ok\n");
    return 0;
}
