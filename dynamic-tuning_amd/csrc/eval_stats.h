// Streaming evaluation statistics (dyt_eval_rows, dyt_eval_keep; kernels in eval_stats.hip): the layout of the device-resident state, every
// argument check, and the partition of a batch of logit rows over workgroups, lanes and load widths, as plain functions of plain values.
// No HIP type and no header is used here, so a host compiler reads this file on its own (tools/eval_stats_check.cpp plays the partition
// lane by lane without a GPU).
#pragma once

#if defined(__HIP__) || defined(__HIPCC__)
#define DYT_EVAL_HD __host__ __device__
#else
#define DYT_EVAL_HD
#endif

namespace dyt {

// ---- the state: `counts`, a flat int64 buffer (additive: every entry accumulates, ranks merge with a SUM) ----------------------------------
//   [0, 8)                      head: rows counted, rows ignored, rows with a NaN, mask rows (images) counted, 4 spare words
//   [8, 24)                     rank histogram: bin r < 15 = exactly r classes rank ahead of the label, bin 15 = 15 or more (NaN rows too)
//   [24, 24 + L * (T + 1))      keep histogram [layers][tokens + 1]: (image, layer) pairs by their number of kept patch tokens
// `per_class` (int64 [2 * classes]): class totals, then class top-1 hits.  `loss_sum`: one double.
constexpr int EVAL_HEAD_WORDS = 8;
constexpr int EVAL_ROWS = 0, EVAL_IGNORED = 1, EVAL_NAN_ROWS = 2, EVAL_MASK_ROWS = 3;
constexpr int EVAL_RANK_BINS = 16;
constexpr int EVAL_OFF_RANK = EVAL_HEAD_WORDS;
constexpr int EVAL_OFF_KEEP = EVAL_OFF_RANK + EVAL_RANK_BINS;
DYT_EVAL_HD inline long long eval_keep_offset(int layer, int kept, int tokens) { return EVAL_OFF_KEEP + (long long)layer * (tokens + 1) + kept; }
DYT_EVAL_HD inline long long eval_counts_words(int layers, int tokens) { return EVAL_OFF_KEEP + (long long)layers * (tokens + 1); }
DYT_EVAL_HD inline int eval_rank_bin(int rank) { return rank < EVAL_RANK_BINS - 1 ? rank : EVAL_RANK_BINS - 1; }

// per-row results: rank >= 0 of an ordinary row; EVAL_RANK_IGNORED for a label outside [0, classes); `classes` for a row holding a NaN
constexpr int EVAL_RANK_IGNORED = -1;

constexpr int EVAL_MAX_ROWS = 1 << 20, EVAL_MAX_CLASSES = 65536, EVAL_MAX_LAYERS = 64, EVAL_MAX_TOKENS = 1024;

// ---- the row kernel's partition ----------------------------------------------------------------------------------------------------------
// A row of up to EVAL_WAVE_ROW_MAX classes is read by one wave (4 rows per 256-thread workgroup), a wider one by a whole workgroup.
constexpr int EVAL_WAVE = 64, EVAL_BLOCK = 256, EVAL_WAVE_ROW_MAX = 1024;
DYT_EVAL_HD inline bool eval_wide(int classes) { return classes > EVAL_WAVE_ROW_MAX; }
DYT_EVAL_HD inline int eval_row_lanes(int classes) { return eval_wide(classes) ? EVAL_BLOCK : EVAL_WAVE; }
DYT_EVAL_HD inline int eval_rows_per_block(int classes) { return EVAL_BLOCK / eval_row_lanes(classes); }
DYT_EVAL_HD inline int eval_row_blocks(int rows, int classes) { const int r = eval_rows_per_block(classes); return (rows + r - 1) / r; }
// thread `tid` of workgroup `block`: its row (may be >= rows in the last workgroup of the narrow form) and its lane within that row
DYT_EVAL_HD inline int eval_thread_row(int block, int tid, int classes) { return eval_wide(classes) ? block : block * (EVAL_BLOCK / EVAL_WAVE) + tid / EVAL_WAVE; }
DYT_EVAL_HD inline int eval_thread_lane(int tid, int classes) { return eval_wide(classes) ? tid : tid % EVAL_WAVE; }

// Load widths of one row.  The row starts at element `first` = (address of logits) / 4 + row * ld of the fp32 address space; `head` scalar
// loads bring it to a 16-byte boundary, `nvec` 16-byte loads follow, `tail` scalar loads end it: head + 4 * nvec + tail = classes.  With a
// 16-byte aligned base and ld % 4 == 0 every row has head = 0; with an odd ld, or a view that starts at an odd element, the scalar loads are
// the (at most 3 + 3) elements at the ends and the body still moves 16 bytes per lane.
struct EvalSpan { int head, nvec, tail; };
DYT_EVAL_HD inline EvalSpan eval_span(unsigned long long logits_addr, long long ld, int row, int classes) {
    const unsigned long long first = logits_addr / 4 + (unsigned long long)((long long)row * ld);
    EvalSpan s;
    s.head = (int)((4 - (first & 3)) & 3);
    if (s.head > classes) s.head = classes;
    s.nvec = (classes - s.head) / 4;
    s.tail = classes - s.head - 4 * s.nvec;
    return s;
}
// What lane `lane` of the row's `lanes` lanes reads: element `lane` of the head if lane < head; the vectors lane, lane + lanes, ... below nvec,
// vector k covering elements [head + 4k, head + 4k + 4); element head + 4 nvec + lane of the tail if lane < tail.
DYT_EVAL_HD inline int eval_vec_first(const EvalSpan& s, int k) { return s.head + 4 * k; }
DYT_EVAL_HD inline int eval_tail_first(const EvalSpan& s) { return s.head + 4 * s.nvec; }

// ---- the keep kernel: one wave per (image, layer), 4 per workgroup ---------------------------------------------------------------------------
DYT_EVAL_HD inline long long eval_keep_waves(int images, int layers) { return (long long)images * layers; }
DYT_EVAL_HD inline int eval_keep_blocks(int images, int layers) { return (int)((eval_keep_waves(images, layers) + 3) / 4); }

// ---- argument checks: the text of the refusal, or a null pointer.  Addresses as integers. -----------------------------------------------------
inline const char* eval_rows_error(unsigned long long logits, long long ld, unsigned long long labels, int rows, int classes,
                                   unsigned long long counts, unsigned long long loss_sum, unsigned long long row_rank, unsigned long long row_loss) {
    if (!logits || !labels || !counts || !loss_sum || !row_rank || !row_loss) return "eval: null pointer";
    if (rows < 1 || rows > EVAL_MAX_ROWS) return "eval: rows outside 1 ... 2^20";
    if (classes < 1 || classes > EVAL_MAX_CLASSES) return "eval: classes outside 1 ... 65536";
    if (ld < classes) return "eval: ld < classes";
    if (ld > (1ll << 40)) return "eval: ld beyond 2^40";
    if (logits % 4 != 0 || row_rank % 4 != 0 || row_loss % 4 != 0) return "eval: logits, row_rank and row_loss must be 4-byte aligned";
    if (counts % 8 != 0 || labels % 8 != 0 || loss_sum % 8 != 0) return "eval: counts, labels and loss_sum must be 8-byte aligned";
    return nullptr;
}
inline const char* eval_per_class_error(unsigned long long per_class) {
    if (per_class % 8 != 0) return "eval: per_class must be 8-byte aligned";
    return nullptr;
}
inline const char* eval_keep_error(unsigned long long token_select, int images, int layers, int tokens, unsigned long long counts) {
    if (!token_select || !counts) return "eval: null pointer";
    if (images < 1 || images > EVAL_MAX_ROWS) return "eval: images outside 1 ... 2^20";
    if (layers < 1 || layers > EVAL_MAX_LAYERS) return "eval: layers outside 1 ... 64";
    if (tokens < 1 || tokens > EVAL_MAX_TOKENS) return "eval: tokens outside 1 ... 1024";
    if (token_select % 4 != 0) return "eval: token_select must be 4-byte aligned";
    if (counts % 8 != 0) return "eval: counts must be 8-byte aligned";
    return nullptr;
}

}  // namespace dyt
