// CPU walk of the on-device Mixup / CutMix host logic (dynamic-tuning_amd/csrc/mix.h), checked without a GPU against tables that
// tests/test_mix_host.py computes with numpy and writes to the file named on the command line (little-endian):
//   int32 n_partner, n_value, n_pred, n_box
//   n_partner x int32 {n, count, frames, want}                          mix_partner
//   n_value   x fp32  {a, b, lam_f, oml_f, want}                        mix_value, bit for bit
//   n_pred    x int32 {mode, y, x, yl, yh, xl, xh, want}                mix_from_partner (and mix_run_needs_partner, derived from it here)
//   n_box     x {fp64 lam, fp64 want_lam, int32 cy, cx, yl, yh, xl, xh} mix_box, mix_corrected_lam
// and every argument combination the entries refuse, with their valid neighbours.
// Build and run (host only; -ffp-contract=off keeps mix_value's three roundings apart):
//   c++ -std=c++17 -O2 -ffp-contract=off -g -fsanitize=address,undefined -fno-sanitize-recover=all -I dynamic-tuning_amd/csrc
//     tools/mix_check.cpp -o /tmp/mix_check && /tmp/mix_check tables.bin
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "mix.h"

using namespace dyt;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            abort();                                                                 \
        }                                                                            \
    } while (0)

template <class T>
static std::vector<T> read_n(FILE* f, size_t n) {
    std::vector<T> v(n);
    CHECK(fread(v.data(), sizeof(T), n, f) == n);
    return v;
}

struct BoxRec { double lam, want_lam; int32_t cy, cx, yl, yh, xl, xh; };
static_assert(sizeof(BoxRec) == 40, "box record layout");

static void tables(const char* path) {
    FILE* f = fopen(path, "rb");
    CHECK(f != nullptr);
    const std::vector<int32_t> head = read_n<int32_t>(f, 4);
    for (int32_t n : head) CHECK(n > 0 && n < (1 << 24));

    const std::vector<int32_t> partner = read_n<int32_t>(f, (size_t)head[0] * 4);
    for (int k = 0; k < head[0]; ++k) {
        const int32_t* r = &partner[(size_t)k * 4];
        const int got = mix_partner(r[0], r[1], r[2]);
        CHECK(got == r[3]);
        CHECK(got >= 0 && got < r[1]);
        CHECK(mix_partner(got, r[1], r[2]) == r[0]);   // pairing is an involution
    }
    printf("mix check: partner ok (%d cases)\n", head[0]);

    const std::vector<float> value = read_n<float>(f, (size_t)head[1] * 5);
    int differ = 0, fused = 0;
    for (int k = 0; k < head[1]; ++k) {
        const float* r = &value[(size_t)k * 5];
        const float got = mix_value(r[0], r[1], r[2], r[3]);
        if (memcmp(&got, &r[4], sizeof(float)) != 0 && !(got != got && r[4] != r[4])) {
            if (differ++ < 8) fprintf(stderr, "mix_value(%.9g, %.9g, %.9g, %.9g) = %.9g, table %.9g\n", r[0], r[1], r[2], r[3], got, r[4]);
        }
        // the contracted form the header's comment rules out: one rounding fewer
        const float c = (float)((double)r[2] * (double)r[0] + (double)(r[3] * r[1]));
        fused += memcmp(&c, &r[4], sizeof(float)) != 0;
    }
    CHECK(differ == 0);
    CHECK(fused > 0);   // so this table can tell an fma apart
    printf("mix check: value ok (%d pairs; a contracted form would differ in %d)\n", head[1], fused);

    const std::vector<int32_t> pred = read_n<int32_t>(f, (size_t)head[2] * 8);
    for (int k = 0; k < head[2]; ++k) {
        const int32_t* r = &pred[(size_t)k * 8];
        CHECK((int)mix_from_partner(r[0], r[1], r[2], r[3], r[4], r[5], r[6]) == r[7]);
        // a run needs the partner exactly when the mode blends or one of its pixels comes from there
        MixParams p;
        memset(&p, 0, sizeof(p));
        p.mode = r[0]; p.yl = r[3]; p.yh = r[4]; p.xl = r[5]; p.xh = r[6];
        for (int n : {1, 4, 16}) {
            bool any = p.mode == MIX_MIXUP;
            for (int j = 0; j < n; ++j) any = any || mix_from_partner(r[0], r[1], r[2] + j, r[3], r[4], r[5], r[6]);
            CHECK(mix_run_needs_partner(p, r[1], r[2], n) == any);
        }
    }
    printf("mix check: predicate ok (%d cases)\n", head[2]);

    const std::vector<BoxRec> box = read_n<BoxRec>(f, (size_t)head[3]);
    for (const BoxRec& r : box) {
        const MixBox b = mix_box(r.lam, r.cy, r.cx);
        CHECK(b.yl == r.yl && b.yh == r.yh && b.xl == r.xl && b.xh == r.xh);
        const double lam = mix_corrected_lam(b);
        CHECK(memcmp(&lam, &r.want_lam, sizeof(double)) == 0);
        CHECK(!mix_box_error(b.yl, b.yh, b.xl, b.xh) && !mix_lam_error(lam));
    }
    printf("mix check: box ok (%d cases)\n", head[3]);
    CHECK(fgetc(f) == EOF);
    fclose(f);
}

static void refusals() {
    // pairing: frames >= 1, a positive multiple of frames, an even number of clips
    for (int frames : {1, 2, 3})
        for (int count = -2; count <= 14; ++count) {
            const bool ok = count >= 1 && count % frames == 0 && (count / frames) % 2 == 0;
            CHECK((mix_count_error(count, frames) == nullptr) == ok);
        }
    CHECK(mix_count_error(4, 0) && mix_count_error(4, -1));
    CHECK(mix_count_error(1, 1) && mix_count_error(3, 1) && mix_count_error(6, 2) && mix_count_error(5, 2));
    CHECK(!mix_count_error(2, 1) && !mix_count_error(4, 2) && !mix_count_error(128, 1));
    // lam
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    for (double lam : {0.0, 1.0, 0.5, 1e-300, 0.999}) CHECK(!mix_lam_error(lam));
    for (double lam : {-1e-12, 1.0 + 1e-12, -1.0, 2.0, inf, -inf, nan}) CHECK(mix_lam_error(lam));
    // mode
    for (int mode = -2; mode <= 4; ++mode) CHECK((mix_mode_error(mode) == nullptr) == (mode >= 0 && mode <= 2));
    // box: inside [0, 224], not reversed; empty boxes are fine
    CHECK(!mix_box_error(0, 224, 0, 224) && !mix_box_error(0, 0, 0, 0) && !mix_box_error(224, 224, 224, 224) && !mix_box_error(5, 37, 3, 50));
    CHECK(!mix_box_error(0, 1, 223, 224) && !mix_box_error(7, 7, 0, 224));
    CHECK(mix_box_error(-1, 10, 0, 10) && mix_box_error(0, 10, -1, 10) && mix_box_error(0, 225, 0, 10) && mix_box_error(0, 10, 0, 225));
    CHECK(mix_box_error(10, 9, 0, 10) && mix_box_error(0, 10, 10, 9));
    // image pointers and the kind of the source
    const unsigned long long base = 0x7f0000000000ull;
    for (int kind = -1; kind <= 3; ++kind) CHECK((mix_src_error(kind, base, base) == nullptr) == (kind >= 0 && kind <= 2));
    for (unsigned long long a = 0; a < 64; ++a) {
        CHECK((mix_src_error(1, base + a, base) != nullptr) == (a % 16 != 0));   // misaligned byte pointer
        CHECK((mix_src_error(0, base, base + a) != nullptr) == (a % 16 != 0));
        CHECK((mix_params_ptr_error(base + a) != nullptr) == (a % 16 != 0));
    }
    CHECK(mix_params_ptr_error(0));
    // classes
    for (int c : {1, 10, 1000, 1031, 65536}) CHECK(!mix_classes_error(c));
    for (int c : {0, -1, 65537}) CHECK(mix_classes_error(c));
    printf("mix check: refusals ok\n");
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s TABLES  (written by tests/test_mix_host.py)\n", argv[0]);
        return 2;
    }
    tables(argv[1]);
    refusals();
    return 0;
}
