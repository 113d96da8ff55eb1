// CPU walk of the byte-image input's host logic (dynamic-tuning_amd/csrc/input_norm.h), checked without a GPU.
//   * input_norm_value -- the scalar formula the byte forms of image_load.hip evaluate -- over all 3 x 256 (channel, byte) pairs, for the
//     ImageNet and the Inception statistics, bit for bit against a table of 2 x 3 x 256 little-endian fp32 values read from the file
//     named on the command line (tests/test_input_u8_host.py writes it from tests/golden/input_u8/input_norm_table.npz, which numpy's
//     ((u / 255) - mean) / std in float32 produced);
//   * every argument combination the entries refuse, and their valid neighbours.
// Build and run (host only):
//   c++ -std=c++17 -O2 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I dynamic-tuning_amd/csrc
//     tools/input_norm_check.cpp -o /tmp/input_norm_check && /tmp/input_norm_check table.bin
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "input_norm.h"

using namespace dyt;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            abort();                                                                 \
        }                                                                            \
    } while (0)

static void formula(const char* path) {
    static float want[2][3][256];
    FILE* f = fopen(path, "rb");
    CHECK(f != nullptr);
    CHECK(fread(want, sizeof(float), 2 * 3 * 256, f) == 2 * 3 * 256);
    CHECK(fgetc(f) == EOF);
    fclose(f);
    const InputNorm stats[2] = {IN_NORM_IMAGENET, {{0.5f, 0.5f, 0.5f}, {0.5f, 0.5f, 0.5f}}};
    CHECK(stats[0].mean[0] == 0.485f && stats[0].mean[1] == 0.456f && stats[0].mean[2] == 0.406f);
    CHECK(stats[0].std[0] == 0.229f && stats[0].std[1] == 0.224f && stats[0].std[2] == 0.225f);
    int differ = 0;
    for (int s = 0; s < 2; ++s)
        for (int c = 0; c < 3; ++c)
            for (unsigned u = 0; u < 256; ++u) {
                const float got = input_norm_value(u, stats[s].mean[c], stats[s].std[c]);
                if (memcmp(&got, &want[s][c][u], sizeof(float)) != 0) {
                    if (differ++ < 8) fprintf(stderr, "stats %d channel %d byte %u: %.9g, table %.9g\n", s, c, u, got, want[s][c][u]);
                }
            }
    CHECK(differ == 0);
    // the shortcuts the header's comment rules out do change bits somewhere (so this table can tell them apart)
    int recip = 0;
    for (unsigned u = 0; u < 256; ++u) {
        const float a = ((float)u * (1.0f / 255.0f) - 0.485f) * (1.0f / 0.229f);
        recip += a != want[0][0][u];
    }
    CHECK(recip > 0);
    printf("input norm check: formula ok (2 x 3 x 256 values; a reciprocal form would differ in %d of 256)\n", recip);
}

static void refusals() {
    const int U8 = IN_F_IMAGES_U8, NHWC = IN_F_IMAGES_NHWC, TOK = IN_F_TOKENS_IN;
    CHECK(U8 == 512 && NHWC == 1024 && TOK == 128);
    // flags: every combination of the three bits, with and without unrelated bits around them
    for (int other : {0, 1 | 2 | 4 | 8 | 16 | 32 | 64 | 256})
        for (int bits = 0; bits < 8; ++bits) {
            const bool u8 = bits & 1, nhwc = bits & 2, tok = bits & 4;
            const int flags = other | (u8 ? U8 : 0) | (nhwc ? NHWC : 0) | (tok ? TOK : 0);
            const bool refused = (nhwc && !u8) || ((u8 || nhwc) && tok);
            CHECK((input_flags_error(flags) != nullptr) == refused);
        }
    CHECK(input_flags_error(NHWC) && input_flags_error(U8 | TOK) && input_flags_error(NHWC | TOK) && input_flags_error(U8 | NHWC | TOK));
    CHECK(!input_flags_error(0) && !input_flags_error(U8) && !input_flags_error(U8 | NHWC) && !input_flags_error(TOK));
    // alignment of the byte pointer
    for (unsigned long long a = 0; a < 64; ++a) CHECK((input_ptr_error(0x7f0000000000ull + a) != nullptr) == (a % 16 != 0));
    // statistics
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float ok_m[3] = {0.485f, -3.0f, 0.0f}, ok_s[3] = {0.229f, 1e-30f, 1e30f};
    CHECK(!input_norm_error(ok_m, ok_s));
    CHECK(input_norm_error(nullptr, ok_s) && input_norm_error(ok_m, nullptr));
    for (int c = 0; c < 3; ++c) {
        for (float bad : {inf, -inf, nan}) {
            float m[3] = {ok_m[0], ok_m[1], ok_m[2]};
            m[c] = bad;
            CHECK(input_norm_error(m, ok_s));
        }
        for (float bad : {0.0f, -0.0f, -0.5f, inf, -inf, nan}) {
            float s[3] = {ok_s[0], ok_s[1], ok_s[2]};
            s[c] = bad;
            CHECK(input_norm_error(ok_m, s));
        }
    }
    printf("input norm check: refusals ok\n");
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s TABLE  (2 x 3 x 256 fp32 values: ImageNet, Inception statistics)\n", argv[0]);
        return 2;
    }
    formula(argv[1]);
    refusals();
    return 0;
}
