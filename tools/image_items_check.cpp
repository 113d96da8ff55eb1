// CPU walk of the image-load work items (dynamic-tuning_amd/csrc/image_items.h) -- the map the image-load kernel and its launcher share, checked
// without a GPU.  For batch 1 and 2 and every (source kind, destination) all items are walked:
//   * the item count is the closed form (every pixel of every channel in one run) and is what the destination needs;
//   * every destination element -- [0, batch*196*768) of the operand, [0, batch*3*224*224) of the planes -- is written by exactly one
//     (item, channel, lane of the run);
//   * x0 is a multiple of the run length and the run ends inside its row;
//   * the source offset is in bounds, 16-byte aligned in bytes, and is where pixel (b, c, y, x0) lies in its layout;
//   * the destination element is the one that pixel belongs to: operand element (b*196+py*14+px)*768 + c*256 + i*16 + j holds pixel
//     [b][c][py*16+i][px*16+j]; plane element ((b*3+c)*224+y)*224+x holds pixel [b][c][y][x];
//   * consecutive items own consecutive 16-byte (fp32 source) or 64-byte groups of the destination (per channel for a channels-last item).
// Build and run (host only):
//   c++ -std=c++17 -O2 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I dynamic-tuning_amd/csrc
//     tools/image_items_check.cpp -o /tmp/image_items_check && /tmp/image_items_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "image_items.h"

using namespace dyt;

static char gRow[96] = "";
#define CHECK(cond)                                                                             \
    do {                                                                                        \
        if (!(cond)) {                                                                          \
            fprintf(stderr, "%s:%d: CHECK(%s) failed (%s)\n", __FILE__, __LINE__, #cond, gRow); \
            abort();                                                                            \
        }                                                                                       \
    } while (0)

typedef unsigned long long u64;

template <int KIND, bool PLANES>
static u64 walk(int batch) {
    constexpr int N = image_run(KIND), NC = image_item_channels(KIND);
    constexpr bool NHWC = KIND == IMAGE_SRC_U8_NHWC;
    constexpr u64 ELEM = KIND == IMAGE_SRC_F32 ? 4 : 1, IMAGE = 3ull * 224 * 224;
    const u64 dst_elems = PLANES ? (u64)batch * 3 * 224 * 224 : (u64)batch * 196 * 768;
    const u64 count = image_item_count(KIND, batch);
    CHECK(count == (u64)batch * 3 * 224 * 224 / (u64)(N * NC));
    CHECK(count * N * NC == dst_elems);
    std::vector<unsigned char> writers(dst_elems, 0);
    for (u64 idx = 0; idx < count; ++idx) {
        snprintf(gRow, sizeof gRow, "kind %d, %s, batch %d, item %llu", KIND, PLANES ? "planes" : "operand", batch, idx);
        const ImageItem t = image_item<KIND, PLANES>(idx);
        CHECK(t.b >= 0 && t.b < batch && t.c >= 0 && t.c + NC <= 3 && t.y >= 0 && t.y < 224);
        CHECK(t.x0 >= 0 && t.x0 % N == 0 && t.x0 + N <= 224);
        CHECK(t.src + (u64)N * NC <= IMAGE && (t.src * ELEM) % 16 == 0 && (IMAGE * ELEM) % 16 == 0);
        CHECK(t.src == (NHWC ? ((u64)t.y * 224 + t.x0) * 3 : ((u64)t.c * 224 + t.y) * 224 + t.x0));
        // consecutive items, consecutive groups
        if (!NHWC) CHECK(t.dst == idx * N);
        else CHECK(t.dst == (PLANES ? (u64)t.b * IMAGE + (idx % (224 * 224 / 16)) * 16 : (idx / 16) * 768 + (idx % 16) * 16));
        for (int k = 0; k < NC; ++k)
            for (int j = 0; j < N; ++j) {
                const int c = t.c + k, x = t.x0 + j;
                const u64 e = t.dst + k * image_channel_stride(PLANES) + j;
                CHECK(e < dst_elems);
                CHECK(writers[e]++ == 0);
                if (PLANES) {
                    CHECK(e == (((u64)t.b * 3 + c) * 224 + t.y) * 224 + x);
                } else {
                    const u64 row = e / 768;
                    const int col = (int)(e % 768), p = (int)(row % 196), py = p / 14, px = p % 14;
                    CHECK((int)(row / 196) == t.b && col / 256 == c && py * 16 + (col / 16) % 16 == t.y && px * 16 + col % 16 == x);
                }
            }
    }
    for (u64 e = 0; e < dst_elems; ++e) CHECK(writers[e] == 1);
    return count;
}

template <int KIND>
static u64 walk_kind() {
    u64 n = 0;
    for (int batch = 1; batch <= 2; ++batch) n += walk<KIND, false>(batch) + walk<KIND, true>(batch);
    return n;
}

int main() {
    static_assert(IMG == 224 && PS == 16 && GRID_P == 14 && PLANE == 224ull * 224, "image constants");
    static_assert(IMAGE_SRC_F32 == 0 && IMAGE_SRC_U8 == 1 && IMAGE_SRC_U8_NHWC == 2, "the src_kind values of dyt_mix_images / dyt_erase_images");
    const u64 n = walk_kind<IMAGE_SRC_F32>() + walk_kind<IMAGE_SRC_U8>() + walk_kind<IMAGE_SRC_U8_NHWC>();
    printf("image items check: %llu items, every destination element has one writer and its own pixel\n", n);
    return 0;
}
