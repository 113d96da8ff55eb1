// Streaming evaluation statistics, two context-free entries (dyt_eval_rows, dyt_eval_keep).  The state layout, the partition of rows over
// workgroups / lanes / load widths and every argument check are eval_stats.h.
//
//   eval_rows_kernel<WIDE>   fp32 logits [rows, ld] + int64 labels -> row_rank [rows], row_loss [rows]; writes nothing else
//   eval_fold_kernel         ONE workgroup: row_rank / row_loss / labels -> counts (head, rank histogram), per_class, loss_sum
//   eval_keep_kernel         fp32 token_select [images, layers, tokens] -> counts (keep histogram), one wave per (image, layer)
//
// Row kernel: ONE pass over the row with an online rescale, for every class count 1 ... 65 536.  The label's logit x_t is loaded first (one
// extra load), so the rank -- #{x_j > x_t} + #{j < t : x_j == x_t} -- is counted while the row streams by, and the running maximum starts at
// x_t: it is finite from the first element on, -inf on other classes is exp(-inf) = 0, and no -inf - -inf can arise.  Each lane keeps
// (m, s) with s = sum exp(x - m) over its elements; a group of up to 16 elements (four 16-byte loads in flight) first raises m, rescales s once, then adds its terms.  Lanes, then waves
// (through LDS, in wave order), are merged at the row's maximum: the order is fixed, the result is the same bits run to run.  Keeping
// the row on chip instead would bound the class count by the LDS (65 536 fp32 = 256 KB do not fit) for no saving: either form reads memory
// once.
// Pure fp32 / integer: the bf16 and the fp16 build of the library hold the same code.  No float atomic; integer atomics only inside the
// single fold workgroup and one per wave of the keep kernel.
#include "../../include/dyt_hip.h"
#include "dyt_common.h"
#include "eval_stats.h"

namespace dyt {

namespace {

struct RowAcc {
    float xt, m, s;   // the label's logit; running maximum (starts at xt); sum of exp(x - m)
    int ahead;        // classes ranked ahead of the label so far
    int nan;
    int64_t t;
};

__device__ __forceinline__ void visit_rank(RowAcc& a, float v, int j) {
    a.nan |= (v != v);
    a.ahead += (v > a.xt) || (v == a.xt && j < a.t);
}
__device__ __forceinline__ void visit1(RowAcc& a, float v, int j) {
    visit_rank(a, v, j);
    const float m = fmaxf(a.m, v);
    a.s = a.s * expf(a.m - m) + expf(v - m);
    a.m = m;
}
__device__ __forceinline__ float max4(const float4& q) { return fmaxf(fmaxf(q.x, q.y), fmaxf(q.z, q.w)); }
__device__ __forceinline__ float sum_exp4(const float4& q, float m) { return (expf(q.x - m) + expf(q.y - m)) + (expf(q.z - m) + expf(q.w - m)); }
__device__ __forceinline__ void rank4(RowAcc& a, const float4& q, int j) {
    visit_rank(a, q.x, j); visit_rank(a, q.y, j + 1); visit_rank(a, q.z, j + 2); visit_rank(a, q.w, j + 3);
}
// N vectors whose loads are all in flight before the first is used; j0 + 4 * k * stride is the class index of vector k's first element
template <int N>
__device__ __forceinline__ void visit_vectors(RowAcc& a, const float4 (&q)[N], int j0, int stride) {
    float m = a.m;
#pragma unroll
    for (int k = 0; k < N; ++k) { rank4(a, q[k], j0 + 4 * k * stride); m = fmaxf(m, max4(q[k])); }
    if (m != a.m) a.s *= expf(a.m - m);   // one rescale per group
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < N; ++k) s += sum_exp4(q[k], m);
    a.s += s;
    a.m = m;
}

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

}  // namespace

template <bool WIDE>
__global__ __launch_bounds__(EVAL_BLOCK) void eval_rows_kernel(const float* __restrict__ logits, long long ld, const int64_t* __restrict__ labels,
                                                               int rows, int classes, int32_t* __restrict__ row_rank, float* __restrict__ row_loss) {
    constexpr int LANES = WIDE ? EVAL_BLOCK : EVAL_WAVE;
    const int row = eval_thread_row(blockIdx.x, threadIdx.x, classes), lane = eval_thread_lane(threadIdx.x, classes);
    if (row >= rows) return;   // narrow form only, a whole wave at a time (no barrier there)
    const int64_t t = labels[row];
    if (t < 0 || t >= classes) {   // uniform over the row's lanes
        if (lane == 0) { row_rank[row] = EVAL_RANK_IGNORED; row_loss[row] = 0.f; }
        return;
    }
    const float* __restrict__ x = logits + (long long)row * ld;
    RowAcc a;
    a.xt = x[t]; a.m = a.xt; a.s = 0.f; a.ahead = 0; a.nan = 0; a.t = t;
    const EvalSpan sp = eval_span((unsigned long long)reinterpret_cast<uintptr_t>(logits), ld, row, classes);
    if (lane < sp.head) visit1(a, x[lane], lane);
    const float4* __restrict__ xv = reinterpret_cast<const float4*>(x + sp.head);
    int k = lane;
    for (; k + 3 * LANES < sp.nvec; k += 4 * LANES) {   // four 16-byte loads per lane in flight
        const float4 q[4] = {xv[k], xv[k + LANES], xv[k + 2 * LANES], xv[k + 3 * LANES]};
        visit_vectors<4>(a, q, eval_vec_first(sp, k), LANES);
    }
    for (; k < sp.nvec; k += LANES) {
        const float4 q[1] = {xv[k]};
        visit_vectors<1>(a, q, eval_vec_first(sp, k), LANES);
    }
    if (lane < sp.tail) { const int j = eval_tail_first(sp) + lane; visit1(a, x[j], j); }

    // lanes of a wave, at the wave's maximum
    float m = wave_max(a.m);
    float s = wave_sum(a.s * expf(a.m - m));
    int ahead = wave_sum_i32(a.ahead);
    int nan = __any(a.nan) ? 1 : 0;
    if (WIDE) {   // the 4 waves, in wave order
        __shared__ float sm[4], ss[4];
        __shared__ int sa[4], sn[4];
        const int w = threadIdx.x / EVAL_WAVE;
        if (threadIdx.x % EVAL_WAVE == 0) { sm[w] = m; ss[w] = s; sa[w] = ahead; sn[w] = nan; }
        __syncthreads();
        if (threadIdx.x != 0) return;
        m = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
        s = (ss[0] * expf(sm[0] - m) + ss[1] * expf(sm[1] - m)) + (ss[2] * expf(sm[2] - m) + ss[3] * expf(sm[3] - m));
        ahead = sa[0] + sa[1] + sa[2] + sa[3];
        nan = sn[0] | sn[1] | sn[2] | sn[3];
    } else if (lane != 0) {
        return;
    }
    if (nan) { row_rank[row] = classes; row_loss[row] = 0.f; return; }
    row_rank[row] = ahead;
    row_loss[row] = -((a.xt - m) - logf(s));   // the shift stays inside
}

// One workgroup.  Thread i takes rows i, i + 256, ...: its loss terms are summed in double in that order, the 256 partial sums by a fixed
// tree; the counters go through integer atomics (LDS for the head and the rank bins, memory for per_class), whose sums do not depend on order.
__global__ __launch_bounds__(EVAL_BLOCK) void eval_fold_kernel(const int32_t* __restrict__ row_rank, const float* __restrict__ row_loss,
                                                               const int64_t* __restrict__ labels, int rows, int classes,
                                                               unsigned long long* __restrict__ counts, unsigned long long* __restrict__ per_class,
                                                               double* __restrict__ loss_sum) {
    __shared__ unsigned int bins[EVAL_OFF_KEEP];   // head + rank histogram of this launch (rows <= 2^20 fit 32 bits)
    __shared__ double part[EVAL_BLOCK];
    const int tid = threadIdx.x;
    if (tid < EVAL_OFF_KEEP) bins[tid] = 0;
    __syncthreads();
    double sum = 0.0;
    for (int r = tid; r < rows; r += EVAL_BLOCK) {
        const int rank = row_rank[r];
        if (rank == EVAL_RANK_IGNORED) { atomicAdd(&bins[EVAL_IGNORED], 1u); continue; }
        atomicAdd(&bins[EVAL_ROWS], 1u);
        const bool nan = rank >= classes;
        if (nan) atomicAdd(&bins[EVAL_NAN_ROWS], 1u);
        else sum += (double)row_loss[r];
        atomicAdd(&bins[EVAL_OFF_RANK + eval_rank_bin(rank)], 1u);
        if (per_class) {
            const int64_t t = labels[r];   // in [0, classes): the row kernel has checked it
            atomicAdd(&per_class[t], 1ull);
            if (rank == 0) atomicAdd(&per_class[classes + t], 1ull);
        }
    }
    part[tid] = sum;
    __syncthreads();
    for (int o = EVAL_BLOCK / 2; o > 0; o >>= 1) {
        if (tid < o) part[tid] += part[tid + o];
        __syncthreads();
    }
    if (tid < EVAL_OFF_KEEP && bins[tid]) counts[tid] += bins[tid];   // one writer per word, one workgroup per launch
    if (tid == 0) *loss_sum += part[0];
}

__global__ __launch_bounds__(EVAL_BLOCK) void eval_keep_kernel(const float* __restrict__ token_select, int images, int layers, int tokens,
                                                               unsigned long long* __restrict__ counts) {
    const long long wave = (long long)blockIdx.x * (EVAL_BLOCK / EVAL_WAVE) + threadIdx.x / EVAL_WAVE;
    if (wave >= eval_keep_waves(images, layers)) return;
    const int lane = threadIdx.x % EVAL_WAVE;
    const int layer = (int)(wave % layers);
    const float* __restrict__ m = token_select + wave * tokens;
    int kept = 0;   // wave-uniform
    for (int j0 = 0; j0 < tokens; j0 += EVAL_WAVE) {
        const int j = j0 + lane;
        const bool on = j < tokens && m[j] != 0.f;
        kept += __popcll(__ballot(on));
    }
    if (lane == 0) {
        atomicAdd(&counts[eval_keep_offset(layer, kept, tokens)], 1ull);
        if (wave == 0) atomicAdd(&counts[EVAL_MASK_ROWS], (unsigned long long)images);
    }
}

}  // namespace dyt

using namespace dyt;

static unsigned long long addr(const void* p) { return (unsigned long long)reinterpret_cast<uintptr_t>(p); }

extern "C" int dyt_eval_rows(const float* logits, int64_t ld, const int64_t* labels, int rows, int classes, int64_t* counts, int64_t* per_class,
                             double* loss_sum, int32_t* row_rank, float* row_loss, void* stream) {
    if (const char* e = eval_rows_error(addr(logits), ld, addr(labels), rows, classes, addr(counts), addr(loss_sum), addr(row_rank), addr(row_loss))) {
        set_error("dyt_eval_rows: %s (rows %d, classes %d, ld %lld)", e, rows, classes, (long long)ld);
        return DYT_ERR_ARG;
    }
    if (const char* e = eval_per_class_error(addr(per_class))) { set_error("dyt_eval_rows: %s", e); return DYT_ERR_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)eval_row_blocks(rows, classes)), block(EVAL_BLOCK);
    if (eval_wide(classes)) hipLaunchKernelGGL(eval_rows_kernel<true>, grid, block, 0, s, logits, (long long)ld, labels, rows, classes, row_rank, row_loss);
    else hipLaunchKernelGGL(eval_rows_kernel<false>, grid, block, 0, s, logits, (long long)ld, labels, rows, classes, row_rank, row_loss);
    DYT_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(eval_fold_kernel, dim3(1), block, 0, s, row_rank, row_loss, labels, rows, classes, reinterpret_cast<unsigned long long*>(counts),
                       reinterpret_cast<unsigned long long*>(per_class), loss_sum);
    DYT_HIP_CHECK(hipGetLastError());
    return DYT_OK;
}

extern "C" int dyt_eval_keep(const float* token_select, int images, int layers, int tokens, int64_t* counts, void* stream) {
    if (const char* e = eval_keep_error(addr(token_select), images, layers, tokens, addr(counts))) {
        set_error("dyt_eval_keep: %s (images %d, layers %d, tokens %d)", e, images, layers, tokens);
        return DYT_ERR_ARG;
    }
    hipLaunchKernelGGL(eval_keep_kernel, dim3((unsigned)eval_keep_blocks(images, layers)), dim3(EVAL_BLOCK), 0, static_cast<hipStream_t>(stream),
                       token_select, images, layers, tokens, reinterpret_cast<unsigned long long*>(counts));
    DYT_HIP_CHECK(hipGetLastError());
    return DYT_OK;
}
