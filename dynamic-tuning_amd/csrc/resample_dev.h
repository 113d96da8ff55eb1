// Device pieces the three resample routes share (resample.hip: 11-tap bicubic, resample_wide.hip: 75-tap bicubic, resample_clip.hip:
// float bilinear clips): the row loader, the tap range read back from scratch, the aligned staging of a source row segment into LDS, the
// vertical pass's accumulate and pack, the zero fill of an invalid band, the coefficient kernel and the refusals of the *_coeffs entries.
// One definition each, so a fix made for one route holds for all.  No atomics and no floating point in the pixel helpers; the coefficient
// kernel's fp64 is resample.h's.  Device-only: the host-readable parts stay in resample.h / resample_wide.h / resample_clip.h.
#pragma once
#include "../../include/dyt_hip.h"
#include "dyt_common.h"
#include "resample.h"

namespace dyt {

constexpr int RS_BAND = 16;                 // output rows per block of a vertical pass
constexpr int RS_ROWB = RS_OUT * 3;         // bytes of one 224-pixel row: 672 = 42 x 16
constexpr int RS_GROUPS = RS_ROWB / 16;
static_assert(RS_ROWB % 16 == 0 && RS_OUT % RS_BAND == 0, "a 224-pixel byte row is a whole number of 16-byte runs; bands tile the window");

// Row n of the table, all 12 words.  false: the header's filter is not `filter`, or n has no row (units, capacity).  The caller applies
// its own row check next, and writes zeros where either fails.  The bicubic routes never read r.pad (it is the clip route's source
// clip); the int4 that holds it is loaded for its other words anyway.
__device__ __forceinline__ bool resample_load_row(const int* __restrict__ table, int filter, int n, int capacity, ResampleRow& r) {
    const int2 h = *reinterpret_cast<const int2*>(table);
    if (h.x != filter) return false;
    const int u = resample_unit(n, h.y, capacity);
    if (u < 0) return false;
    const int4* q = reinterpret_cast<const int4*>(table + RS_HEADER_WORDS + (size_t)u * RS_ROW_WORDS);
    const int4 q0 = q[0], q1 = q[1], q2 = q[2];
    r.src_h = q0.x; r.src_w = q0.y; r.top = q0.z; r.left = q0.w;
    r.box_h = q1.x; r.box_w = q1.y; r.full_h = q1.z; r.full_w = q1.w;
    r.off_y = q2.x; r.off_x = q2.y; r.flags = q2.z; r.pad = q2.w;
    return true;
}

__device__ __forceinline__ int resample_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The taps [lo, lo + n) of one output position, from the first tap and the count read back from scratch, clamped against the box again
template <int KMAX>
__device__ __forceinline__ void resample_tap_range(int first, int count, int box, int& lo, int& n) {
    lo = resample_clampi(first, 0, box - 1);
    n = resample_clampi(count, 0, min(KMAX, box - lo));
}

// Bytes [first, first + nbytes) of the source allocation (src_bytes long, 16-byte aligned) into the LDS row `lds`, by the block's 256 work
// items, from the 16-byte boundary at or below `first` on; returns the head, the offset of byte `first` in `lds`.  At most max_chunks
// chunks of 16 bytes are written.  A 16-byte load is issued only where all 16 bytes lie inside the allocation; the chunk that crosses its
// end is filled byte by byte, with zeros behind the end.  Bytes beside the segment come along; no output depends on them.
__device__ __forceinline__ int resample_stage_row(const uint8_t* __restrict__ src, long long src_bytes, long long first, int nbytes,
                                                  uint8_t* lds, int max_chunks, int tid) {
    const long long from = first & ~15LL;
    const int head = (int)(first - from);
    const int chunks = min((head + nbytes + 15) >> 4, max_chunks);
    for (int i = tid; i < chunks; i += 256) {
        const long long at = from + 16LL * i;
        if (at + 16 <= src_bytes) {
            *reinterpret_cast<uint4*>(lds + 16 * i) = *reinterpret_cast<const uint4*>(src + at);
        } else {
            for (int j = 0; j < 16; ++j) lds[16 * i + j] = at + j < src_bytes ? src[at + j] : (uint8_t)0;
        }
    }
    return head;
}

// ---- the vertical pass: sixteen int32 accumulators per work item, Pillow's ss = 2^21 + sum(byte * k) -----------------------------------
__device__ __forceinline__ void resample_acc_start(int (&acc)[16]) {
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 1 << (RS_PRECISION_BITS - 1);
}

// acc += k times the 16 bytes of v
__device__ __forceinline__ void resample_acc_add(int (&acc)[16], const uint4 v, int k) {
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] += (int)((w[i >> 2] >> (8 * (i & 3))) & 0xFFu) * k;
}

// resample_clip8 as an opaque 32-bit value.  Left to itself hipcc fuses two neighbouring shift-and-clamps of a packed word into
// v_ashr_pk_u8_i32 and then takes the upper half of that instruction's destination for zero; the instruction leaves it as it was, and the
// stray bits are ORed into bytes 2 and 3 of the word (seen on the MI355X: those bytes came out as supersets of the right bits).  The empty
// asm statement keeps each byte a value of its own, so the word is built from four clamps, three shifts and an OR.
__device__ __forceinline__ unsigned resample_byte(int ss) {
    unsigned v = (unsigned)resample_clip8(ss);
    asm("" : "+v"(v));
    return v;
}

// the 16 clamped bytes of acc, every one through resample_byte
__device__ __forceinline__ uint4 resample_acc_pack(const int (&acc)[16]) {
    unsigned w[4];
#pragma unroll
    for (int d = 0; d < 4; ++d)
        w[d] = resample_byte(acc[4 * d]) | (resample_byte(acc[4 * d + 1]) << 8) | (resample_byte(acc[4 * d + 2]) << 16) |
               (resample_byte(acc[4 * d + 3]) << 24);
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// an image without a valid row: its band of RS_BAND output rows (contiguous, 16-byte aligned) as zeros
__device__ __forceinline__ void resample_zero_band(uint8_t* __restrict__ out, int tid) {
    for (int i = tid; i < RS_BAND * RS_GROUPS; i += 256) reinterpret_cast<uint4*>(out)[i] = make_uint4(0u, 0u, 0u, 0u);
}

// ---- the coefficient kernel of a bicubic route with KMAX taps ---------------------------------------------------------------------------
// One block per (axis, image), 256 work items: thread t computes resample_coeffs_taps<KMAX> of window position t -- first tap, tap count,
// KMAX coefficients, fp64 without contraction -- into `out`, [axis][field][224] ints per image.  The row check keeps the 2.5 bound for
// KMAX = RS_KMAX, which needs it; any wider KMAX is resample_wide.h's.  An image without a valid row gets zeros.
template <int KMAX>
__global__ __launch_bounds__(256) void resample_coeff_kernel(const int* __restrict__ table, int capacity, int Hs, int Ws, int img_base,
                                                             int* __restrict__ out) {
    constexpr int FIELDS = 2 + KMAX;
    const int axis = blockIdx.x, t = threadIdx.x;
    if (t >= RS_OUT) return;
    ResampleRow r;
    const bool ok = resample_load_row(table, RS_BICUBIC, img_base + (int)blockIdx.y, capacity, r) && resample_row_ok_core(r, Hs, Ws, KMAX == RS_KMAX);
    int xmin = 0, count = 0;
    int k[KMAX];
    for (int x = 0; x < KMAX; ++x) k[x] = 0;
    if (ok) {
        if (axis == 0) resample_coeffs_taps<KMAX>(r.box_h, r.full_h, r.off_y + t, xmin, count, k);
        else resample_coeffs_taps<KMAX>(r.box_w, r.full_w, r.off_x + t, xmin, count, k);
    }
    int* o = out + ((size_t)blockIdx.y * 2 + axis) * FIELDS * RS_OUT + t;
    o[0] = xmin;
    o[RS_OUT] = count;
    for (int x = 0; x < KMAX; ++x) o[(2 + x) * RS_OUT] = k[x];
}

// ---- host side --------------------------------------------------------------------------------------------------------------------------
inline unsigned long long resample_addr(const void* p) { return (unsigned long long)reinterpret_cast<uintptr_t>(p); }

// What the three *_coeffs entries refuse alike: the text of the entry's own pointer check, else of its shape check (null: passed), else
// a row outside the table.  DYT_OK: go on.
inline int resample_coeffs_refusal(const char* entry, const char* ptr_error, const char* shape_error, int row, int capacity) {
    if (const char* e = ptr_error ? ptr_error : shape_error) { set_error("%s: %s", entry, e); return DYT_ERR_ARG; }
    if (row < 0 || row >= capacity) { set_error("%s: row %d is outside the table's %d rows", entry, row, capacity); return DYT_ERR_ARG; }
    return DYT_OK;
}

}  // namespace dyt
