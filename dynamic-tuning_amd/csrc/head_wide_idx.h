// Index arithmetic of the wide classification head (head_wide.hip): every global and LDS index the three MFMA kernels form
// comes from one of the functions below, and tools/head_wide_index_check.cpp walks them on the CPU -- every lane of every
// workgroup, for the shapes the tests use -- asserting that no global index leaves [0, B) x [0, C) / [0, C) x [0, 768), that no
// LDS index leaves its image and that every output element is written exactly once.  Plain C++: no HIP type in here.
//
// Common to the three kernels: 256 threads = 4 waves; a K stage is 32 contraction steps; wave w owns 32 of the tile's 128 output
// columns and both 32-row halves of its 64 rows.  The operand of v_mfma_f32_32x32x2_f32 is one fp32 per lane (lane l: row l & 31,
// k = l >> 5); the result register 4g + e of lane l is C[row l & 31][column 8g + 4(l >> 5) + e].
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DYT_HWI __host__ __device__ inline
#else
#define DYT_HWI inline
#endif

namespace dyt {
namespace hw {

constexpr int HD768 = 768;     // channels of a cls row / columns of head.weight
constexpr int THREADS = 256;
constexpr int BK = 32;         // contraction steps per LDS stage
constexpr int BM = 64;         // output rows per workgroup (2 MFMA tiles per wave)
constexpr int BN = 128;        // output columns per workgroup (one 32-wide MFMA tile per wave)
constexpr int SLICE = 1024;    // dx: classes per partial sum (a condition of the accuracy bound, not a tuning knob)
constexpr int MAX_C = 65536;

struct Src { long long off; int lds; bool valid; };   // global element offset, LDS float offset, whether the global element exists
struct Out { long long off; int nvalid; bool vec; };  // first element, how many of the 4 consecutive ones exist, one 16-byte store?

DYT_HWI int ceil_div(int a, int b) { return (a + b - 1) / b; }
DYT_HWI int imin(int a, int b) { return a < b ? a : b; }
DYT_HWI int imax(int a, int b) { return a > b ? a : b; }

// output column (within the workgroup's 128) of result register quad g of a lane; row-in-32 is lane & 31
DYT_HWI int acc_col(int wave, int lane, int g) { return wave * 32 + 8 * g + 4 * (lane >> 5); }

// ------------------------------------------------------------------------------------------------------------------------------
// logits [B,C] = cls_n [B,768] x head_w [C,768]^T + head_b.  grid (ceil(C/128), ceil(B/64)).  Both operands are staged as 16-byte
// chunks of a 128-byte row, chunk slot XOR-swizzled with (row >> 1) & 7 (gemm_f32_mfma.h); rows past the end are CLAMPED (their
// results are never stored).  LDS: A image [64][32], W image [128][32] floats.
// ------------------------------------------------------------------------------------------------------------------------------
constexpr int LG_A_FLOATS = BM * BK, LG_W_FLOATS = BN * BK, LG_LDS_FLOATS = LG_A_FLOATS + LG_W_FLOATS;
constexpr int LG_A_PER_THREAD = BM * 8 / THREADS, LG_W_PER_THREAD = BN * 8 / THREADS;   // 16-byte chunks per thread and stage
DYT_HWI int lg_swz(int row, int chunk) { return (chunk ^ ((row >> 1) & 7)) << 2; }
// chunk t of thread tid of K stage kt; `rows` = B for the A image (row0 = first batch row), C for the W image (row0 = first class)
DYT_HWI Src lg_stage(int tid, int t, int kt, int row0, int rows, int lds_base) {
    const int idx = t * THREADS + tid, row = idx >> 3, chunk = idx & 7;
    Src s;
    s.off = (long long)imin(row0 + row, rows - 1) * HD768 + kt * BK + chunk * 4;
    s.lds = lds_base + row * BK + lg_swz(row, chunk);
    s.valid = true;
    return s;
}
// fragment read j (0..3) of a lane: the 16-byte chunk 2j + (lane >> 5) of row `row` (tile-local); register t of it is k = 8j + 4(lane >> 5) + t
DYT_HWI int lg_frag(int lds_base, int row, int lane, int j) { return lds_base + row * BK + lg_swz(row, 2 * j + (lane >> 5)); }
// the 4 consecutive logits of register quad g, tile i of a lane
DYT_HWI Out lg_out(int m0, int n0, int wave, int lane, int i, int g, int B, int C) {
    const int m = m0 + i * 32 + (lane & 31), n = n0 + acc_col(wave, lane, g);
    Out o;
    o.off = (long long)m * C + n;
    o.nvalid = m < B ? imax(0, imin(4, C - n)) : 0;
    o.vec = o.nvalid == 4 && (C & 3) == 0;   // the row stride is C floats: 16-byte aligned only for C % 4 == 0
    return o;
}

// ------------------------------------------------------------------------------------------------------------------------------
// dx partials P[slice][B][768] = dlogits[B, slice] x head_w[slice, 768].  grid (768/128, ceil(B/64), ceil(C/1024)).
// A image [64 rows][32 k] with row stride 33 (dlogits rows are not 16-byte aligned for odd C: scalar loads), W image [32 k][128
// channels] with row stride 160 (the two half-waves of a transposed ds_read_b32 then use disjoint banks).  Batch rows >= B and
// classes >= the slice's end are ZERO-FILLED, never read.
// ------------------------------------------------------------------------------------------------------------------------------
constexpr int DX_A_LD = BK + 1, DX_W_LD = BN + 32;
constexpr int DX_A_FLOATS = BM * DX_A_LD, DX_W_FLOATS = BK * DX_W_LD, DX_LDS_FLOATS = DX_A_FLOATS + DX_W_FLOATS;
constexpr int DX_CHAIN_STAGES = 8;   // stages (of 32 classes) one accumulator chain runs before it joins the slice's running sum
constexpr int DX_A_PER_THREAD = BM * BK / THREADS, DX_W_PER_THREAD = BK * BN / 4 / THREADS;
DYT_HWI int n_slices(int C) { return ceil_div(C, SLICE); }
DYT_HWI int slice_begin(int s) { return s * SLICE; }
DYT_HWI int slice_end(int s, int C) { return imin(C, (s + 1) * SLICE); }
DYT_HWI int slice_stages(int s, int C) { return ceil_div(slice_end(s, C) - slice_begin(s), BK); }
// scalar element t of thread tid: dlogits[m0 + row][slice_begin + kt*32 + k]
DYT_HWI Src dx_stage_a(int tid, int t, int kt, int m0, int s, int B, int C) {
    const int idx = t * THREADS + tid, row = idx >> 5, k = idx & 31;
    const int b = m0 + row, c = slice_begin(s) + kt * BK + k;
    Src r;
    r.valid = b < B && c < slice_end(s, C);
    r.off = (long long)b * C + c;
    r.lds = row * DX_A_LD + k;
    return r;
}
// 16-byte chunk t of thread tid: head_w[slice_begin + kt*32 + k][n0 + 4 chunk ..]
DYT_HWI Src dx_stage_w(int tid, int t, int kt, int n0, int s, int C) {
    const int idx = t * THREADS + tid, k = idx >> 5, chunk = idx & 31;
    const int c = slice_begin(s) + kt * BK + k;
    Src r;
    r.valid = c < slice_end(s, C);
    r.off = (long long)c * HD768 + n0 + chunk * 4;
    r.lds = DX_A_FLOATS + k * DX_W_LD + chunk * 4;
    return r;
}
DYT_HWI int dx_frag_a(int i, int lane, int kp) { return (i * 32 + (lane & 31)) * DX_A_LD + 2 * kp + (lane >> 5); }
DYT_HWI int dx_frag_w(int wave, int lane, int kp) { return DX_A_FLOATS + (2 * kp + (lane >> 5)) * DX_W_LD + wave * 32 + (lane & 31); }
DYT_HWI Out dx_out(int m0, int n0, int s, int wave, int lane, int i, int g, int B) {
    const int m = m0 + i * 32 + (lane & 31), n = n0 + acc_col(wave, lane, g);
    Out o;
    o.off = ((long long)s * B + m) * HD768 + n;
    o.nvalid = m < B ? 4 : 0;
    o.vec = o.nvalid == 4;
    return o;
}

// ------------------------------------------------------------------------------------------------------------------------------
// dW [C,768] += dlogits^T [C,B] x cls_n [B,768]; db[c] += sum_b dlogits[b][c].  grid (768/128, ceil(C/64)).  The contraction
// runs over the batch: A image [32 b][64 classes] with row stride 96, X image [32 b][128 channels] with row stride 160; batch rows
// >= B and classes >= C are ZERO-FILLED, never read.  The workgroups of channel tile 0 also sum the A image's columns into db.
// ------------------------------------------------------------------------------------------------------------------------------
constexpr int DW_A_LD = BM + 32, DW_X_LD = BN + 32;
constexpr int DW_A_FLOATS = BK * DW_A_LD, DW_X_FLOATS = BK * DW_X_LD, DW_LDS_FLOATS = DW_A_FLOATS + DW_X_FLOATS;
constexpr int DW_A_PER_THREAD = BK * BM / THREADS, DW_X_PER_THREAD = BK * BN / 4 / THREADS;
DYT_HWI int dw_stages(int B) { return ceil_div(B, BK); }
DYT_HWI Src dw_stage_a(int tid, int t, int kt, int c0, int B, int C) {
    const int idx = t * THREADS + tid, k = idx >> 6, cc = idx & 63;
    const int b = kt * BK + k, c = c0 + cc;
    Src r;
    r.valid = b < B && c < C;
    r.off = (long long)b * C + c;
    r.lds = k * DW_A_LD + cc;
    return r;
}
DYT_HWI Src dw_stage_x(int tid, int t, int kt, int n0, int B) {
    const int idx = t * THREADS + tid, k = idx >> 5, chunk = idx & 31;
    const int b = kt * BK + k;
    Src r;
    r.valid = b < B;
    r.off = (long long)b * HD768 + n0 + chunk * 4;
    r.lds = DW_A_FLOATS + k * DW_X_LD + chunk * 4;
    return r;
}
DYT_HWI int dw_frag_a(int i, int lane, int kp) { return (2 * kp + (lane >> 5)) * DW_A_LD + i * 32 + (lane & 31); }
DYT_HWI int dw_frag_x(int wave, int lane, int kp) { return DW_A_FLOATS + (2 * kp + (lane >> 5)) * DW_X_LD + wave * 32 + (lane & 31); }
DYT_HWI int dw_db_lds(int tid, int k) { return k * DW_A_LD + tid; }   // tid < 64: class c0 + tid
DYT_HWI Out dw_out(int c0, int n0, int wave, int lane, int i, int g, int C) {
    const int c = c0 + i * 32 + (lane & 31), n = n0 + acc_col(wave, lane, g);
    Out o;
    o.off = (long long)c * HD768 + n;
    o.nvalid = c < C ? 4 : 0;
    o.vec = o.nvalid == 4;
    return o;
}

}  // namespace hw
}  // namespace dyt
