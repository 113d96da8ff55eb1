// CPU walk of the streaming-evaluation host logic (dynamic-tuning_amd/csrc/eval_stats.h) without a GPU: the partition of the row kernel is
// played workgroup by workgroup, thread by thread, for every shape tests/test_gpu_eval_stats.py runs (the full cross product of its class
// counts, row counts and the four memory layouts), against a host buffer of exactly the extent the device buffer has, and asserts
//   * every load lies inside the buffer, every 16-byte load is 16-byte aligned, every scalar load 4-byte aligned;
//   * every element of every row is covered exactly once, no element outside a row is touched, no row >= rows is read;
//   * the keep kernel's waves cover every (image, layer) once and their histogram words lie inside the state;
//   * the layout offsets (head, rank bins, keep histogram rows) do not overlap;
//   * every argument combination the entries refuse is refused, and its valid neighbours pass.
// Build and run (host only):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I dynamic-tuning_amd/csrc tools/eval_stats_check.cpp
//     -o /tmp/eval_stats_check && /tmp/eval_stats_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "eval_stats.h"

using namespace dyt;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            abort();                                                                 \
        }                                                                            \
    } while (0)

static const int CLASSES[] = {1, 2, 5, 63, 64, 65, 255, 256, 257, 1000, 1024, 1025, 4099, 21843, 65536};
static const int ROWS[] = {1, 3, 4, 5, 64, 65, 257};

// One (rows, classes) batch in a buffer of `extent` floats whose first element sits at fp32 address `base` (so base % 4 is the misalignment
// of the view); row r starts `offset + r * ld` elements into the buffer.
static long long play_rows(int rows, int classes, long long ld, int offset, unsigned long long base) {
    const long long extent = offset + (long long)(rows - 1) * ld + classes;
    std::vector<uint8_t> seen((size_t)extent, 0);
    const unsigned long long logits_addr = (base + (unsigned long long)offset) * 4;   // what the entry receives
    long long loads = 0;
    auto touch = [&](long long at, int width) {   // `at`: element index in the buffer
        CHECK(at >= 0 && at + width <= extent);
        CHECK(((base + (unsigned long long)at) * 4) % (width * 4) == 0);
        for (int k = 0; k < width; ++k) { CHECK(seen[(size_t)(at + k)] == 0); seen[(size_t)(at + k)] = 1; }
        ++loads;
    };
    const int blocks = eval_row_blocks(rows, classes), lanes = eval_row_lanes(classes);
    CHECK(blocks >= 1 && (long long)blocks * eval_rows_per_block(classes) >= rows && (long long)(blocks - 1) * eval_rows_per_block(classes) < rows);
    std::vector<int> lanes_of_row((size_t)rows, 0);
    for (int b = 0; b < blocks; ++b) {
        for (int tid = 0; tid < EVAL_BLOCK; ++tid) {
            const int row = eval_thread_row(b, tid, classes), lane = eval_thread_lane(tid, classes);
            CHECK(row >= 0 && lane >= 0 && lane < lanes);
            if (row >= rows) continue;   // the kernel returns before any load
            ++lanes_of_row[(size_t)row];
            const EvalSpan sp = eval_span(logits_addr, ld, row, classes);
            CHECK(sp.head >= 0 && sp.head <= 3 && sp.tail >= 0 && sp.tail <= 3 && sp.nvec >= 0);
            CHECK(sp.head + 4 * sp.nvec + sp.tail == classes);
            const long long x = offset + (long long)row * ld;   // the row's first element in the buffer
            if (lane < sp.head) touch(x + lane, 1);
            for (int k = lane; k < sp.nvec; k += lanes) {
                const int j = eval_vec_first(sp, k);
                CHECK(j >= 0 && j + 4 <= classes);
                touch(x + j, 4);
            }
            if (lane < sp.tail) {
                const int j = eval_tail_first(sp) + lane;
                CHECK(j >= 0 && j < classes);
                touch(x + j, 1);
            }
        }
    }
    for (int r = 0; r < rows; ++r) {
        CHECK(lanes_of_row[(size_t)r] == lanes);   // every row has all its lanes, in one workgroup
        for (int j = 0; j < classes; ++j) CHECK(seen[(size_t)(offset + (long long)r * ld + j)] == 1);
    }
    long long covered = 0;
    for (uint8_t v : seen) covered += v;
    CHECK(covered == (long long)rows * classes);   // nothing between the rows, nothing in front of the view
    return loads;
}

static void rows_partition() {
    long long shapes = 0, loads = 0, vec_rows = 0;
    for (int classes : CLASSES) {
        for (int rows : ROWS) {
            loads += play_rows(rows, classes, classes, 0, 0x1000);          // contiguous, 16-byte aligned base
            loads += play_rows(rows, classes, classes + 1, 0, 0x1000);      // ld = C + 1
            loads += play_rows(rows, classes, classes + 3, 0, 0x1000);      // ld = C + 3
            loads += play_rows(rows, classes, classes, 1, 0x1000);          // a view offset by one element
            shapes += 4;
        }
        // an aligned base with ld % 4 == 0 never takes a scalar head
        if (classes % 4 == 0)
            for (int r = 0; r < 9; ++r) { CHECK(eval_span(0x4000, classes, r, classes).head == 0 && eval_span(0x4000, classes, r, classes).tail == 0); ++vec_rows; }
    }
    CHECK(eval_wide(EVAL_WAVE_ROW_MAX + 1) && !eval_wide(EVAL_WAVE_ROW_MAX) && eval_rows_per_block(1) == 4 && eval_rows_per_block(65536) == 1);
    CHECK(eval_row_blocks(EVAL_MAX_ROWS, 1) == EVAL_MAX_ROWS / 4 && eval_row_blocks(EVAL_MAX_ROWS, EVAL_MAX_CLASSES) == EVAL_MAX_ROWS);
    printf("eval stats check: rows ok (%lld shapes, %lld loads, %lld aligned rows)\n", shapes, loads, vec_rows);
}

static void layout_and_keep() {
    CHECK(EVAL_ROWS < EVAL_HEAD_WORDS && EVAL_IGNORED < EVAL_HEAD_WORDS && EVAL_NAN_ROWS < EVAL_HEAD_WORDS && EVAL_MASK_ROWS < EVAL_HEAD_WORDS);
    CHECK(EVAL_ROWS != EVAL_IGNORED && EVAL_ROWS != EVAL_NAN_ROWS && EVAL_ROWS != EVAL_MASK_ROWS && EVAL_IGNORED != EVAL_NAN_ROWS &&
          EVAL_IGNORED != EVAL_MASK_ROWS && EVAL_NAN_ROWS != EVAL_MASK_ROWS);
    CHECK(EVAL_OFF_RANK == EVAL_HEAD_WORDS && EVAL_OFF_KEEP == EVAL_OFF_RANK + EVAL_RANK_BINS);
    for (int rank = 0; rank <= EVAL_MAX_CLASSES; ++rank) {
        const int b = eval_rank_bin(rank);
        CHECK(b >= 0 && b < EVAL_RANK_BINS && (rank < EVAL_RANK_BINS - 1 ? b == rank : b == EVAL_RANK_BINS - 1));
    }
    const int shapes[][2] = {{12, 196}, {12, 1}, {1, 1}, {EVAL_MAX_LAYERS, EVAL_MAX_TOKENS}, {3, 65}};
    for (const auto& s : shapes) {
        const int layers = s[0], tokens = s[1];
        const long long words = eval_counts_words(layers, tokens);
        std::vector<uint8_t> used((size_t)words, 0);
        for (int w = 0; w < EVAL_OFF_KEEP; ++w) used[(size_t)w] = 1;
        for (int l = 0; l < layers; ++l)
            for (int kept = 0; kept <= tokens; ++kept) {
                const long long at = eval_keep_offset(l, kept, tokens);
                CHECK(at >= EVAL_OFF_KEEP && at < words && used[(size_t)at] == 0);
                used[(size_t)at] = 1;
            }
        for (uint8_t u : used) CHECK(u == 1);   // dense: every word of the state has one meaning
        // the keep kernel: waves -> (image, layer), loads inside [images, layers, tokens]
        for (int images : {1, 3, 65}) {
            const long long waves = eval_keep_waves(images, layers), extent = waves * tokens;
            const int blocks = eval_keep_blocks(images, layers);
            CHECK((long long)blocks * 4 >= waves && (long long)(blocks - 1) * 4 < waves);
            std::vector<uint8_t> pair((size_t)waves, 0);
            for (int b = 0; b < blocks; ++b)
                for (int w = 0; w < 4; ++w) {
                    const long long wave = (long long)b * 4 + w;
                    if (wave >= waves) continue;
                    CHECK(pair[(size_t)wave] == 0);
                    pair[(size_t)wave] = 1;
                    const int layer = (int)(wave % layers);
                    CHECK(wave / layers < images && layer < layers);
                    for (int j0 = 0; j0 < tokens; j0 += EVAL_WAVE)
                        for (int lane = 0; lane < EVAL_WAVE; ++lane)
                            if (j0 + lane < tokens) CHECK(wave * tokens + j0 + lane < extent);
                }
            for (uint8_t p : pair) CHECK(p == 1);
        }
    }
    printf("eval stats check: layout ok\n");
}

static void refusals() {
    const unsigned long long P = 0x10000, Q = 0x20000;
    auto rows_err = [&](unsigned long long lg, long long ld, unsigned long long lb, int rows, int classes, unsigned long long cn,
                        unsigned long long ls, unsigned long long rr, unsigned long long rl) { return eval_rows_error(lg, ld, lb, rows, classes, cn, ls, rr, rl); };
    CHECK(rows_err(P, 10, Q, 4, 10, Q, Q, Q, Q) == nullptr);
    CHECK(rows_err(P + 4, 13, Q, 4, 10, Q, Q, Q, Q) == nullptr);          // a view at an odd element, a row stride
    CHECK(rows_err(P, 65536, Q, EVAL_MAX_ROWS, 65536, Q, Q, Q, Q) == nullptr);
    CHECK(rows_err(P, 1, Q, 1, 1, Q, Q, Q, Q) == nullptr);
    CHECK(rows_err(0, 10, Q, 4, 10, Q, Q, Q, Q) && rows_err(P, 10, 0, 4, 10, Q, Q, Q, Q) && rows_err(P, 10, Q, 4, 10, 0, Q, Q, Q));
    CHECK(rows_err(P, 10, Q, 4, 10, Q, 0, Q, Q) && rows_err(P, 10, Q, 4, 10, Q, Q, 0, Q) && rows_err(P, 10, Q, 4, 10, Q, Q, Q, 0));
    CHECK(rows_err(P, 10, Q, 0, 10, Q, Q, Q, Q) && rows_err(P, 10, Q, -1, 10, Q, Q, Q, Q) && rows_err(P, 10, Q, EVAL_MAX_ROWS + 1, 10, Q, Q, Q, Q));
    CHECK(rows_err(P, 10, Q, 4, 0, Q, Q, Q, Q) && rows_err(P, 65537, Q, 4, 65537, Q, Q, Q, Q) && rows_err(P, 10, Q, 4, -3, Q, Q, Q, Q));
    CHECK(rows_err(P, 9, Q, 4, 10, Q, Q, Q, Q) && rows_err(P, 0, Q, 4, 10, Q, Q, Q, Q) && rows_err(P, -10, Q, 4, 10, Q, Q, Q, Q));
    CHECK(rows_err(P + 2, 10, Q, 4, 10, Q, Q, Q, Q) && rows_err(P, 10, Q + 4, 4, 10, Q, Q, Q, Q) && rows_err(P, 10, Q, 4, 10, Q + 4, Q, Q, Q));
    CHECK(rows_err(P, 10, Q, 4, 10, Q, Q + 4, Q, Q) && rows_err(P, 10, Q, 4, 10, Q, Q, Q + 2, Q) && rows_err(P, 10, Q, 4, 10, Q, Q, Q, Q + 1));
    CHECK(eval_per_class_error(0) == nullptr && eval_per_class_error(Q) == nullptr && eval_per_class_error(Q + 4));
    CHECK(eval_keep_error(P, 3, 12, 196, Q) == nullptr && eval_keep_error(P + 4, 1, 1, 1, Q) == nullptr);
    CHECK(eval_keep_error(P, EVAL_MAX_ROWS, EVAL_MAX_LAYERS, EVAL_MAX_TOKENS, Q) == nullptr);
    CHECK(eval_keep_error(0, 3, 12, 196, Q) && eval_keep_error(P, 3, 12, 196, 0) && eval_keep_error(P, 0, 12, 196, Q));
    CHECK(eval_keep_error(P, EVAL_MAX_ROWS + 1, 12, 196, Q) && eval_keep_error(P, 3, 0, 196, Q) && eval_keep_error(P, 3, 65, 196, Q));
    CHECK(eval_keep_error(P, 3, 12, 0, Q) && eval_keep_error(P, 3, 12, 1025, Q) && eval_keep_error(P + 2, 3, 12, 196, Q) && eval_keep_error(P, 3, 12, 196, Q + 4));
    printf("eval stats check: refusals ok\n");
}

int main() {
    rows_partition();
    layout_and_keep();
    refusals();
    printf("eval stats check: all ok\n");
    return 0;
}
