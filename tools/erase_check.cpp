// CPU walk of the on-device Random Erasing host logic (dynamic-tuning_amd/csrc/erase.h), without a GPU and without input files:
//   * erase_hit and erase_run_hits for a set of rows (corner, edge, 1 x 1, run-straddling, overlapping, clamped and hostile boxes) against
//     a brute-force loop over all 224 x 224 pixels, for the run lengths 4 and 16 the kernels use;
//   * erase_unit: the row an image reads, never outside the table;
//   * every argument check the entries make, with the valid neighbours;
//   * the noise: erase.h's templates over a host restatement of Philox4x32-10 (pinned by the published known answers).
//     `erase_check noise SEED IMAGE C Y X4` prints the four pixel values of that group and `erase_check colour SEED IMAGE BOX C` the box
//     colour, as fp32 bit patterns, for a comparison against an fp64 reference.
// Build and run (host only):
//   c++ -std=c++17 -O2 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I dynamic-tuning_amd/csrc tools/erase_check.cpp
//     -o /tmp/erase_check && /tmp/erase_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "erase.h"

using namespace dyt;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            abort();                                                                 \
        }                                                                            \
    } while (0)

// Philox4x32-10 as dyt_common.h's device struct computes it: key = seed, counter = (offset, subseq)
struct HostPhilox {
    uint32_t c[4];
    HostPhilox(uint64_t seed, uint64_t subseq, uint64_t offset) {
        uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
        c[0] = (uint32_t)offset; c[1] = (uint32_t)(offset >> 32);
        c[2] = (uint32_t)subseq; c[3] = (uint32_t)(subseq >> 32);
        for (int i = 0; i < 10; ++i) {
            const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
            const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
            c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
            k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
        }
    }
};

static EraseRow make_row(int n, std::vector<std::vector<int>> boxes) {
    EraseRow r;
    memset(&r, 0, sizeof r);
    r.n = n;
    for (size_t k = 0; k < boxes.size() && k < (size_t)ERASE_MAX_BOXES; ++k)
        for (int j = 0; j < 4; ++j) r.box[k][j] = boxes[k][j];
    return r;
}

static int brute_hit(const EraseRow& r, int y, int x) {
    const int n = r.n < 0 ? 0 : (r.n > 4 ? 4 : r.n);
    int hit = -1;
    for (int k = 0; k < n; ++k) {
        const long long top = r.box[k][0], h = r.box[k][1], left = r.box[k][2], w = r.box[k][3];
        if ((long long)y >= top && (long long)y < top + h && (long long)x >= left && (long long)x < left + w) hit = k;
    }
    return hit;
}

static void walk_boxes() {
    const int big = 2147483647, low = -2147483647 - 1;
    const std::vector<EraseRow> rows = {
        make_row(0, {}),
        make_row(1, {{0, 5, 0, 7}}),                                  // corner
        make_row(1, {{200, 24, 190, 34}}),                            // ends at row and column 223
        make_row(1, {{100, 1, 101, 1}}),                              // 1 x 1
        make_row(2, {{10, 3, 3, 2}, {20, 3, 15, 2}}),                 // straddle a 4- and a 16-pixel run boundary
        make_row(2, {{30, 50, 30, 50}, {60, 50, 60, 50}}),            // overlap: the later box wins
        make_row(4, {{0, 223, 0, 223}, {1, 1, 1, 1}, {5, 9, 220, 4}, {223, 1, 0, 224}}),
        make_row(1, {{1, 1, 1, 1}, {0, 224, 0, 224}}),                // the second box is not in use
        make_row(9, {{0, 1, 0, 1}, {2, 1, 2, 1}, {4, 1, 4, 1}, {6, 1, 6, 1}}),   // count clamped to 4
        make_row(-3, {{0, 224, 0, 224}}),                             // count clamped to 0
        make_row(4, {{low, big, low, big}, {big, big, big, big}, {-5, 10, -5, 10}, {100, -1, 100, 7}}),   // hostile words: comparisons only
        make_row(2, {{0, big, 0, big}, {50, 0, 50, 10}}),
    };
    long long pixels = 0, hits = 0;
    for (const EraseRow& r : rows) {
        for (int y = 0; y < ERASE_IMG; ++y) {
            for (int x = 0; x < ERASE_IMG; ++x) {
                const int want = brute_hit(r, y, x), got = erase_hit(r, y, x);
                CHECK(got == want);
                CHECK(got >= -1 && got < ERASE_MAX_BOXES);
                ++pixels;
                hits += got >= 0;
            }
            for (int len : {4, 16}) {
                for (int x0 = 0; x0 < ERASE_IMG; x0 += len) {
                    bool any = false;
                    for (int j = 0; j < len; ++j) any = any || brute_hit(r, y, x0 + j) >= 0;
                    const bool run = erase_run_hits(r, y, x0, len);
                    CHECK(!any || run);   // a run that holds an erased pixel is never skipped
                    bool valid = true;    // for boxes with h, w >= 1 the run test is exact
                    for (int k = 0; k < 4; ++k) valid = valid && (k >= r.n || (r.box[k][1] >= 1 && r.box[k][3] >= 1));
                    if (valid && r.n <= 4) CHECK(run == any);
                }
            }
        }
    }
    CHECK(hits > 0);
    printf("erase check: boxes ok (%zu rows, %lld pixels, %lld erased)\n", rows.size(), pixels, hits);
}

static void walk_units() {
    for (int frames : {1, 2, 3, 8})
        for (int cube : {0, 1, 7})
            for (int units : {-1, 0, 1, 3, 4, 1000})
                for (int capacity : {0, 1, 4, 16})
                    for (int n = 0; n < 24; ++n) {
                        const int u = erase_unit(n, frames, cube, units, capacity);
                        CHECK(u >= -1 && u < capacity);
                        const int want = cube ? n / frames : n;
                        if (want < capacity && want < units) CHECK(u == want);
                        else CHECK(u == -1);
                    }
    CHECK(erase_clamp_n(-1) == 0 && erase_clamp_n(0) == 0 && erase_clamp_n(4) == 4 && erase_clamp_n(5) == 4);
    printf("erase check: units ok\n");
}

static void walk_refusals() {
    for (int m = -2; m < 7; ++m) CHECK((erase_mode_error(m) == nullptr) == (m >= 0 && m <= 3));
    for (int n = -2; n < 8; ++n) CHECK((erase_count_error(n) == nullptr) == (n >= 0 && n <= 4));
    CHECK(!erase_box_error(0, 1, 0, 1) && !erase_box_error(223, 1, 223, 1) && !erase_box_error(0, 224, 0, 224) && !erase_box_error(1, 223, 0, 1));
    CHECK(erase_box_error(0, 0, 0, 1) && erase_box_error(0, 1, 0, 0) && erase_box_error(0, -1, 0, 1));
    CHECK(erase_box_error(-1, 1, 0, 1) && erase_box_error(0, 1, -1, 1) && erase_box_error(1, 224, 0, 1) && erase_box_error(0, 1, 1, 224));
    CHECK(erase_box_error(224, 1, 0, 1) && erase_box_error(0, 225, 0, 1) && erase_box_error(0, 2147483647, 0, 1));
    CHECK(erase_table_ptr_error(0) && erase_table_ptr_error(0x1004) && erase_table_ptr_error(0x1008) && !erase_table_ptr_error(0x1010));
    CHECK(!erase_units_error(4, 4, 1, 0) && !erase_units_error(2, 4, 2, 1) && !erase_units_error(4, 4, 2, 0));
    CHECK(erase_units_error(3, 4, 1, 0) && erase_units_error(4, 4, 2, 1) && erase_units_error(0, 4, 1, 0) && erase_units_error(4, 4, 0, 0));
    CHECK(erase_units_error(5, 5, 2, 0) && erase_units_error(1, 0, 1, 0));
    CHECK(!erase_capacity_error(4, 4, 1) && !erase_capacity_error(128, 4, 2));
    CHECK(erase_capacity_error(3, 4, 1) && erase_capacity_error(4, 4, 0) && erase_capacity_error(4, 0, 1) && erase_capacity_error(8, 5, 2));
    CHECK(!erase_src_error(0, 0x1000, 0x2000) && !erase_src_error(2, 0x1000, 0x2000));
    CHECK(erase_src_error(3, 0x1000, 0x2000) && erase_src_error(-1, 0x1000, 0x2000) && erase_src_error(1, 0x1004, 0x2000) && erase_src_error(0, 0x1000, 0x2008));
    printf("erase check: refusals ok\n");
}

static uint32_t bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }

static void walk_noise() {
    const HostPhilox a(0, 0, 0), b(~0ull, ~0ull, ~0ull);   // the published known answers of Philox4x32-10
    CHECK(a.c[0] == 0x6627e8d5u && a.c[1] == 0xe169c58du && a.c[2] == 0xbc57ac4cu && a.c[3] == 0x9b00dbd8u);
    CHECK(b.c[0] == 0x408f276du && b.c[1] == 0x41c83b0eu && b.c[2] == 0xa20bc7c6u && b.c[3] == 0x6d5451fdu);
    CHECK(erase_u01(0) > 0.f && erase_u01(0xFFFFFFFFu) <= 1.f);   // (2^24 - 0.5 rounds to 2^24 in fp32: u = 1 gives r = 0, never a log of 0)
    double sum = 0, sq = 0;
    long long n = 0;
    for (int y = 0; y < ERASE_IMG; ++y)
        for (int x4 = 0; x4 < ERASE_IMG / 4; ++x4) {
            float z[4], again[4];
            erase_pixel_noise4<HostPhilox>(0x1234567890abcdefull, 3, 1, y, x4, z);
            erase_pixel_noise4<HostPhilox>(0x1234567890abcdefull, 3, 1, y, x4, again);
            for (int j = 0; j < 4; ++j) { CHECK(bits(z[j]) == bits(again[j]) && z[j] == z[j] && z[j] > -8.f && z[j] < 8.f); sum += z[j]; sq += (double)z[j] * z[j]; ++n; }
        }
    const double mean = sum / n, var = sq / n - mean * mean;
    CHECK(mean > -0.03 && mean < 0.03 && var > 0.95 && var < 1.05);   // 50 176 values: 5 sigma is 0.022 / 0.032
    float z0[4], z1[4];
    erase_pixel_noise4<HostPhilox>(1, 0, 0, 0, 0, z0);
    erase_pixel_noise4<HostPhilox>(2, 0, 0, 0, 0, z1);
    CHECK(bits(z0[0]) != bits(z1[0]));
    const float c0 = erase_box_colour<HostPhilox>(7, 2, 1, 0), c1 = erase_box_colour<HostPhilox>(7, 2, 1, 1), c2 = erase_box_colour<HostPhilox>(7, 2, 1, 2);
    CHECK(bits(c0) != bits(c1) && bits(c1) != bits(c2) && bits(c0) == bits(erase_box_colour<HostPhilox>(7, 2, 1, 0)));
    CHECK(bits(c0) != bits(erase_box_colour<HostPhilox>(7, 2, 0, 0)) && bits(c0) != bits(erase_box_colour<HostPhilox>(7, 3, 1, 0)));
    printf("erase check: noise ok (mean %.4f, var %.4f over %lld values)\n", mean, var, n);
}

int main(int argc, char** argv) {
    if (argc == 7 && !strcmp(argv[1], "noise")) {
        float z[4];
        erase_pixel_noise4<HostPhilox>(strtoull(argv[2], nullptr, 0), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), z);
        printf("%08x %08x %08x %08x\n", bits(z[0]), bits(z[1]), bits(z[2]), bits(z[3]));
        return 0;
    }
    if (argc == 6 && !strcmp(argv[1], "colour")) {
        printf("%08x\n", bits(erase_box_colour<HostPhilox>(strtoull(argv[2], nullptr, 0), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]))));
        return 0;
    }
    walk_boxes();
    walk_units();
    walk_refusals();
    walk_noise();
    printf("erase check: all ok\n");
    return 0;
}
