// Adapter / gate weight gradients of the DyT hot path (gfx950): the per-chunk MFMA products and the fixed-order reductions
// of their partials, immediate or queued into one batched launch per flush.
#include <stdlib.h>
#include <algorithm>
#include "kernels.h"
#include "rowhelp.h"

namespace dyt {

// 32 outputs x 8 partial-groups per workgroup; fixed summation order (deterministic)
__global__ __launch_bounds__(256) void reduce_partials_kernel(const float* __restrict__ partial, int nparts, int stride,
                                                              float* __restrict__ out, int n, float alpha) {
    __shared__ float red[8][32];
    const int o = threadIdx.x & 31, grp = threadIdx.x >> 5;
    const int i = blockIdx.x * 32 + o;
    float acc = 0.f;
    if (i < n) {
        const int per = (nparts + 7) / 8;
        const int p0 = grp * per, p1 = min(nparts, p0 + per);
#pragma unroll 4
        for (int p = p0; p < p1; ++p) acc += partial[(size_t)p * stride + i];
    }
    red[grp][o] = acc;
    __syncthreads();
    if (grp == 0 && i < n) {
        float t = 0.f;
#pragma unroll
        for (int g = 0; g < 8; ++g) t += red[g][o];
        out[i] += alpha * t;
    }
}
int launch_reduce_partials(const float* partial, int nparts, int stride, float* out, int n, float alpha, hipStream_t s) {
    hipLaunchKernelGGL(reduce_partials_kernel, dim3((n + 31) / 32), dim3(256), 0, s, partial, nparts, stride, out, n, alpha);
    LAUNCH_CHECK();
    return 0;
}

// the same for several (partial, out) pairs in one launch: blockIdx.y selects the pair
struct TokReduceBatch { const float* partial[ReduceQueue::MAX_TOK]; float* out[ReduceQueue::MAX_TOK]; int nparts[ReduceQueue::MAX_TOK]; };
__global__ __launch_bounds__(256) void reduce_partials_batch_kernel(TokReduceBatch b, int stride, int n) {
    __shared__ float red[8][32];
    const float* __restrict__ partial = b.partial[blockIdx.y];
    const int nparts = b.nparts[blockIdx.y];
    const int o = threadIdx.x & 31, grp = threadIdx.x >> 5;
    const int i = blockIdx.x * 32 + o;
    float acc = 0.f;
    if (i < n) {
        const int per = (nparts + 7) / 8;
        const int p0 = grp * per, p1 = min(nparts, p0 + per);
#pragma unroll 4
        for (int p = p0; p < p1; ++p) acc += partial[(size_t)p * stride + i];
    }
    red[grp][o] = acc;
    __syncthreads();
    if (grp == 0 && i < n) {
        float t = 0.f;
#pragma unroll
        for (int g = 0; g < 8; ++g) t += red[g][o];
        b.out[blockIdx.y][i] += t;
    }
}
int queue_tok_reduce(ReduceQueue& q, const float* partial, int nparts, float* out) {
    if (q.n_tok >= ReduceQueue::MAX_TOK) { set_error("reduce queue full"); return -1; }
    q.tok_partial[q.n_tok] = partial; q.tok_out[q.n_tok] = out; q.tok_nparts[q.n_tok] = nparts; ++q.n_tok;
    return 0;
}

// ------------------------------------------------------------------------------------------
// adapter weight gradients:  C[c][j] = sum_m X[m][c] Y[m][j]   (+ column sums of X in j = 64)
// ------------------------------------------------------------------------------------------
constexpr int WG_J = 80;        // 64 adapter columns + the ones column (+ pad)
constexpr int WG_CHUNK = 512;   // minimum tokens per workgroup (the partial buffers are sized for M / 512 chunks)

// bf16: MFMA 32x32x16 with the token dimension as K; tiles are transposed while staged to LDS.
// 64 tokens per step; the next step's rows are prefetched into registers while the current step's
// fragments are read and multiplied (the loads were fully exposed before: 1.3 TB/s).  The column sums
// of X (-> partial[..][c][64]) and of Y (wave 0 of the first channel block, -> partial[..][768][j]) are
// taken from the same fragments on the vector ALU.
constexpr int WG_ROWS = D + 8;  // partial rows per chunk: 768 channels + 1 row of Y column sums (+pad)
struct WgSrc { const void* X; const void* Y; float* partial; float xscale, yscale; };   // x / yscale: fp32 inputs of the half-product form are multiplied by these before the 16-bit conversion
struct WgPair { WgSrc p[2]; };   // blockIdx.z selects the product: both adapter weight gradients of a block are ONE launch
// IT = float: the same kernel on fp32 inputs, converted (times a power of two that keeps gradient-sized values out of the 16-bit
// subnormals) as they are loaded -- the one-part gradient products of the "fp16x3f" form (wgrad_f32_kernel runs at the fp32-MFMA rate)
template <class IT>
__device__ __forceinline__ bf16x8 wg_load8(const IT* p, float scale) {
    if constexpr (sizeof(IT) == 2) {
        return *reinterpret_cast<const bf16x8*>(p);
    } else {
        const f32x4 a = *reinterpret_cast<const f32x4*>(p) * scale, b = *reinterpret_cast<const f32x4*>(p + 4) * scale;
        bf16x8 v = {(bf16)a[0], (bf16)a[1], (bf16)a[2], (bf16)a[3], (bf16)b[0], (bf16)b[1], (bf16)b[2], (bf16)b[3]};
        return v;
    }
}
template <class IT>
__global__ __launch_bounds__(256, 2) void wgrad_bf16_kernel(WgPair src, int M, int chunk) {
    const IT* __restrict__ X = static_cast<const IT*>(src.p[blockIdx.z].X);
    const IT* __restrict__ Y = static_cast<const IT*>(src.p[blockIdx.z].Y);
    const float xscale = src.p[blockIdx.z].xscale, yscale = src.p[blockIdx.z].yscale;
    float* __restrict__ partial = src.p[blockIdx.z].partial;
    constexpr int TS = 64;        // tokens per step
    // LDS rows of 64 tokens (128 B) with the eight 16-B chunks of row r XOR-swizzled by s(r) = ((r >> 3) ^ r) & 7.  Round 6: the round 1-5 layout
    // (144-B rows, no swizzle) kept the ds_read_b128 fragment reads conflict-free but put all 16 channel-chunk lanes of a ds_write_b32
    // lane group on ONE bank (8 rows = 288 words = 0 mod 32): 16-way conflicts on the 24 transposing writes of every step, i.e. the kernel
    // ran on LDS-write cycles (37 us for 84 MB).  With the swizzle the reads stay conflict-free and the writes are 2-way (X) / conflict-free
    // (Y); enumerated for every lane group of both instructions in tools/probes/r6/wgrad_swizzle.py.
    constexpr int LDT = TS;
    auto swz = [](int r) { return ((r >> 3) ^ r) & 7; };
    __shared__ __attribute__((aligned(16))) bf16 Xt[128 * LDT];
    __shared__ __attribute__((aligned(16))) bf16 Yt[64 * LDT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c0 = blockIdx.x * 128;
    const int m0 = blockIdx.y * chunk;
    const int mend = min(m0 + chunk, M);
    f32x16 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;
    float xs = 0.f, ys[2] = {0.f, 0.f};   // column sums of X (own channel) / Y (own columns) over this lane's tokens
    const bool do_ysum = blockIdx.x == 0 && wave == 0;

    // loader roles: X tile = 32 token pairs x 16 channel chunks = 512 tasks (2 / thread); Y = 32 x 8 (1 / thread)
    const int xp0 = tid >> 4, xc = tid & 15;
    const int yp = tid >> 3, yc = tid & 7;
    bf16x8 xr[2][2], yr[2];
    auto zero = [](bf16x8& v) {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (bf16)0.f;
    };
    auto load_step = [&](int tb) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int t = tb + 2 * (xp0 + 16 * h);
            zero(xr[h][0]); zero(xr[h][1]);
            if (t < mend) xr[h][0] = wg_load8<IT>(X + (size_t)t * D + c0 + xc * 8, xscale);
            if (t + 1 < mend) xr[h][1] = wg_load8<IT>(X + (size_t)(t + 1) * D + c0 + xc * 8, xscale);
        }
        const int ty = tb + 2 * yp;
        zero(yr[0]); zero(yr[1]);
        if (ty < mend) yr[0] = wg_load8<IT>(Y + (size_t)ty * RP + yc * 8, yscale);
        if (ty + 1 < mend) yr[1] = wg_load8<IT>(Y + (size_t)(ty + 1) * RP + yc * 8, yscale);
    };
    if (m0 < mend) load_step(m0);
    for (int tb = m0; tb < mend; tb += TS) {
        __syncthreads();  // previous step's fragment reads are done
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                bf16x2 pv = {xr[h][0][i], xr[h][1][i]};
                const int tk = 2 * (xp0 + 16 * h);   // token (pair) column of row xc * 8 + i: chunk tk / 8 goes to slot (tk / 8) ^ s(row), s = (xc ^ i) & 7
                *reinterpret_cast<bf16x2*>(&Xt[(xc * 8 + i) * LDT + ((((tk >> 3) ^ xc ^ i) & 7) << 3) + (tk & 7)]) = pv;
            }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            bf16x2 pv = {yr[0][i], yr[1][i]};
            const int tk = 2 * yp;
            *reinterpret_cast<bf16x2*>(&Yt[(yc * 8 + i) * LDT + ((((tk >> 3) ^ yc ^ i) & 7) << 3) + (tk & 7)]) = pv;
        }
        __syncthreads();
        if (tb + TS < mend) load_step(tb + TS);  // in flight during the reads + MFMAs below
        const int lr = lane & 31, lk = lane >> 5;
        auto sum8 = [](const bf16x8& v) {   // sum of the 8 operands in fp32
#ifdef DYT_FP16
            float t = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) t += (float)v[i];
            return t;
#else
            typedef __attribute__((ext_vector_type(4))) unsigned u32x4;   // bf16 -> fp32 is a 16-bit shift
            const u32x4 u = __builtin_bit_cast(u32x4, v);
            float t = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) t += __builtin_bit_cast(float, u[i] << 16) + __builtin_bit_cast(float, u[i] & 0xffff0000u);
            return t;
#endif
        };
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {  // four 16-token k blocks; lane = (row lr, tokens kk*16 + lk*8 .. +7)
            const int xrow = wave * 32 + lr;
            const bf16x8 xf = *reinterpret_cast<const bf16x8*>(&Xt[xrow * LDT + (((kk * 2 + lk) ^ swz(xrow)) << 3)]);
            bf16x8 yf[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) yf[j] = *reinterpret_cast<const bf16x8*>(&Yt[(j * 32 + lr) * LDT + (((kk * 2 + lk) ^ swz(j * 32 + lr)) << 3)]);
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[j] = DYT_MFMA_32x32x16(xf, yf[j], acc[j]);
            xs += sum8(xf);
            if (do_ysum) { ys[0] += sum8(yf[0]); ys[1] += sum8(yf[1]); }
        }
    }
    // D register i of block j: row = (i / 4) * 8 + (lane >> 5) * 4 + (i % 4) -> channel, col = lane & 31 -> column j * 32 + col
    float* pp = partial + (size_t)blockIdx.y * WG_ROWS * WG_J;
    const int lr = lane & 31, lk = lane >> 5;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int c = c0 + wave * 32 + (i >> 2) * 8 + lk * 4 + (i & 3);
            pp[(size_t)c * WG_J + j * 32 + lr] = acc[j][i];
        }
    xs += __shfl_xor(xs, 32, 64);   // the two token groups of a channel
    if (lk == 0) pp[(size_t)(c0 + wave * 32 + lr) * WG_J + 64] = xs;
    if (do_ysum) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float v = ys[j] + __shfl_xor(ys[j], 32, 64);
            if (lk == 0) pp[(size_t)D * WG_J + j * 32 + lr] = v;
        }
    }
}

// fp32 exact variant on the matrix cores: v_mfma_f32_32x32x2_f32 with the TOKEN dimension as k.  One fp32 per lane and
// operand: lane l supplies (row l % 32, k = l / 32), so an A operand is X[token m + l/32][channel] and a B operand
// Y[token m + l/32][column] -- both straight from global memory, no transposition and no LDS staging.  A lane loads a
// float4 of X (4 consecutive channels) and a float2 of Y per token pair and feeds register t / u to MFMA (t, u): that
// MFMA owns channels c0 + 4*row + t and columns 2*col + u (only the ownership is permuted).  A wave covers 128 channels x
// 64 columns (8 MFMAs, 128 accumulator registers) and every 4th token pair of the chunk; the 4 waves of a workgroup are
// summed through LDS in wave order (deterministic).  Column sums of X / Y ride along on the vector ALU.
__global__ __launch_bounds__(256) void wgrad_f32_kernel(WgPair src, int M, int chunk) {
    const float* __restrict__ X = static_cast<const float*>(src.p[blockIdx.z].X);
    const float* __restrict__ Y = static_cast<const float*>(src.p[blockIdx.z].Y);
    float* __restrict__ partial = src.p[blockIdx.z].partial;
    __shared__ float red[134 * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c0 = blockIdx.x * 128;
    const int m0 = blockIdx.y * chunk, mend = min(m0 + chunk, M);
    const int lr = lane & 31, lk = lane >> 5;
    f32x16 acc[4][2];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[t][u][i] = 0.f;
    float xs[4] = {0.f, 0.f, 0.f, 0.f}, ys[2] = {0.f, 0.f};
    const float* xp = X + (size_t)c0 + 4 * lr;
    const float* yp = Y + 2 * lr;
    constexpr int PF = 4;   // token pairs in flight per wave
    f32x4 xa[PF];
    f32x2 yb[PF];
    auto load_pair = [&](int slot, int m) {   // m = first token of the pair; this lane reads token m + lk
        const int t = m + lk;
        xa[slot] = f32x4{0.f, 0.f, 0.f, 0.f};
        yb[slot] = f32x2{0.f, 0.f};
        if (t < mend) {
            xa[slot] = *reinterpret_cast<const f32x4*>(xp + (size_t)t * D);
            yb[slot] = *reinterpret_cast<const f32x2*>(yp + (size_t)t * RP);
        }
    };
    int m = m0 + 2 * wave;   // this wave's token pairs: m, m + 8, m + 16, ...
#pragma unroll
    for (int q = 0; q < PF; ++q) load_pair(q, m + 8 * q);
    for (; m < mend; m += 8 * PF) {
#pragma unroll
        for (int q = 0; q < PF; ++q) {
            const f32x4 a = xa[q];
            const f32x2 b = yb[q];
            load_pair(q, m + 8 * (PF + q));   // refill the slot (zeros beyond the chunk)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                acc[t][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b[0], acc[t][0], 0, 0, 0);
                acc[t][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b[1], acc[t][1], 0, 0, 0);
                xs[t] += a[t];
            }
            ys[0] += b[0]; ys[1] += b[1];
        }
    }
    // ---- sum the 4 waves in wave order through LDS: element k of lane l lives at red[k * 64 + l] ----
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        float* q = &red[((t * 2 + u) * 16 + i) * 64 + lane];
                        if (w == 0) *q = acc[t][u][i]; else if (w < 3) *q += acc[t][u][i]; else acc[t][u][i] += *q;
                    }
#pragma unroll
            for (int t = 0; t < 4; ++t) { float* q = &red[(128 + t) * 64 + lane]; if (w == 0) *q = xs[t]; else if (w < 3) *q += xs[t]; else xs[t] += *q; }
#pragma unroll
            for (int u = 0; u < 2; ++u) { float* q = &red[(132 + u) * 64 + lane]; if (w == 0) *q = ys[u]; else if (w < 3) *q += ys[u]; else ys[u] += *q; }
        }
        __syncthreads();
    }
    if (wave != 3) return;
    // D register i of MFMA (t, u): row = (i / 4) * 8 + lk * 4 + (i % 4), col = lr -> channel c0 + 4 * row + t, column 2 * lr + u
    float* pp = partial + (size_t)blockIdx.y * WG_ROWS * WG_J;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = (i >> 2) * 8 + lk * 4 + (i & 3);
            const int c = c0 + 4 * row + t;
            *reinterpret_cast<f32x2*>(&pp[(size_t)c * WG_J + 2 * lr]) = f32x2{acc[t][0][i], acc[t][1][i]};
        }
    // column sums: the two token parities (lanes l and l ^ 32) are still separate
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const float v = xs[t] + __shfl_xor(xs[t], 32, 64);
        if (lk == 0) pp[(size_t)(c0 + 4 * lr + t) * WG_J + 64] = v;
    }
    if (blockIdx.x == 0) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const float v = ys[u] + __shfl_xor(ys[u], 32, 64);
            if (lk == 0) pp[(size_t)D * WG_J + 2 * lr + u] = v;
        }
    }
}

struct WgOut {
    const float* partial; float* out_w; int sc, sj; float alpha; float* out_xsum; float alpha_x; float* out_ysum; float alpha_y;
    const float* alpha_dev;
};
struct WgOutPair { WgOut p[2]; };
__global__ void wgrad_reduce_kernel(WgOutPair outs, int nchunks, int r) {
    const WgOut& o = outs.p[blockIdx.y];
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= (D + 1) * (r + 1)) return;
    const int c = idx / (r + 1), j = idx - c * (r + 1);
    const int col = j < r ? j : 64;
    if (c == D && j == r) return;
    float acc = 0.f;
    for (int p = 0; p < nchunks; ++p) acc += o.partial[((size_t)p * WG_ROWS + c) * WG_J + col];
    const float ad = o.alpha_dev ? *o.alpha_dev : 1.0f;
    if (c == D) { if (o.out_ysum) o.out_ysum[j] += (o.alpha_y * ad) * acc; }
    else if (j < r) o.out_w[(size_t)c * o.sc + (size_t)j * o.sj] += (o.alpha * ad) * acc;
    else if (o.out_xsum) o.out_xsum[c] += (o.alpha_x * ad) * acc;
}

// the reduce of several products (each with its own partial buffer and chunk count) in one launch: blockIdx.y selects the product
struct WgReduceBatch { WgReduceDesc e[ReduceQueue::MAX_WG]; };
__global__ void wgrad_reduce_batch_kernel(WgReduceBatch b, int r) {
    const WgReduceDesc& o = b.e[blockIdx.y];
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= (D + 1) * (r + 1)) return;
    const int c = idx / (r + 1), j = idx - c * (r + 1);
    const int col = j < r ? j : 64;
    if (c == D && j == r) return;
    float acc = 0.f;
    for (int p = 0; p < o.nchunks; ++p) acc += o.partial[((size_t)p * WG_ROWS + c) * WG_J + col];
    const float ad = o.alpha_dev ? *o.alpha_dev : 1.0f;
    if (c == D) { if (o.out_ysum) o.out_ysum[j] += (o.alpha_y * ad) * acc; }
    else if (j < r) o.out_w[(size_t)c * o.sc + (size_t)j * o.sj] += (o.alpha * ad) * acc;
    else if (o.out_xsum) o.out_xsum[c] += (o.alpha_x * ad) * acc;
}
int flush_reductions(ReduceQueue& q, hipStream_t s) {
    if (q.n_wg > 0) {
        WgReduceBatch b;
        for (int i = 0; i < q.n_wg; ++i) b.e[i] = q.wg[i];
        hipLaunchKernelGGL(wgrad_reduce_batch_kernel, dim3(((D + 1) * (q.r + 1) + 255) / 256, q.n_wg), dim3(256), 0, s, b, q.r);
        q.n_wg = 0;
    }
    if (q.n_tok > 0) {
        TokReduceBatch b;
        for (int i = 0; i < q.n_tok; ++i) { b.partial[i] = q.tok_partial[i]; b.out[i] = q.tok_out[i]; b.nparts[i] = q.tok_nparts[i]; }
        hipLaunchKernelGGL(reduce_partials_batch_kernel, dim3((D + 1 + 31) / 32, q.n_tok), dim3(256), 0, s, b, D + 1, D + 1);
        q.n_tok = 0;
    }
    LAUNCH_CHECK();
    return 0;
}

// one or two products (same M and r; separate partial buffers) in one launch + one reduce launch
int launch_wgrad(int precision, const WgradArgs* a, int n, hipStream_t s, ReduceQueue* defer) {
    // tokens per workgroup: at least WG_CHUNK, and large enough that the (channel blocks x chunks) grid of ONE product is
    // one round of the 256 CUs (B=128: 6 x 50 = 300 workgroups would leave a 44-workgroup second round; 6 x 40 does not);
    // a pair is two workgroups per CU, which hides the staging latency of the single-product launch
    const int M = a[0].M, r = a[0].r;
    if (dbg_skip(4)) return 0;
    if (n < 1 || n > 2 || (n == 2 && (a[1].M != M || a[1].r != r || a[1].partial == a[0].partial))) {
        set_error("launch_wgrad: bad pair");
        return -1;
    }
    const int cblocks = D / 128;
    const int want = (M + 256 / cblocks - 1) / (256 / cblocks);
    const int chunk = max(WG_CHUNK, (want + 63) / 64 * 64);
    const int nchunks = (M + chunk - 1) / chunk;
    WgPair src;
    WgOutPair outs;
    for (int i = 0; i < 2; ++i) {
        const WgradArgs& w = a[i < n ? i : 0];
        const bool half = precision == 0 && w.half_products;
        const float xs = half ? w.x_scale : 1.f, ys = half ? w.y_scale : 1.f;
        src.p[i] = WgSrc{w.X, w.Y, w.partial, xs, ys};
        outs.p[i] = WgOut{w.partial, w.out_w, w.sc, w.sj, w.alpha / (xs * ys), w.out_xsum, w.alpha_x / xs, w.out_ysum, w.alpha_y / ys, w.alpha_dev};
    }
    if (precision == 0 && a[0].half_products != (n == 2 ? a[1].half_products : a[0].half_products)) { set_error("launch_wgrad: mixed product forms in a pair"); return -1; }
    // (refused before the product kernel is enqueued: a refused call writes nothing, `partial` included)
    if (defer && (defer->n_wg + n > ReduceQueue::MAX_WG || (defer->n_wg > 0 && defer->r != r))) { set_error("reduce queue full / mixed ranks"); return -1; }
    if (precision == 0 && a[0].half_products) hipLaunchKernelGGL(wgrad_bf16_kernel<float>, dim3(D / 128, nchunks, n), dim3(256), 0, s, src, M, chunk);
    else if (precision == 0) hipLaunchKernelGGL(wgrad_f32_kernel, dim3(D / 128, nchunks, n), dim3(256), 0, s, src, M, chunk);
    else {
        // measurement hook: DYT_DBG_WGRAD_LDS = extra dynamic LDS bytes per workgroup (keeps other workgroups off the CU)
        static int extra = -1;
        if (extra < 0) {
            const char* e = getenv("DYT_DBG_WGRAD_LDS");
            extra = e ? atoi(e) : 0;
            if (extra > 0) DYT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(wgrad_bf16_kernel<bf16>), hipFuncAttributeMaxDynamicSharedMemorySize, extra));
        }
        hipLaunchKernelGGL(wgrad_bf16_kernel<bf16>, dim3(D / 128, nchunks, n), dim3(256), extra, s, src, M, chunk);
    }
    if (defer) {
        defer->r = r;
        for (int i = 0; i < n; ++i) {
            const WgOut& o = outs.p[i];
            defer->wg[defer->n_wg++] = WgReduceDesc{o.partial, o.out_w, o.sc, o.sj, o.alpha, o.out_xsum, o.alpha_x, o.out_ysum, o.alpha_y, nchunks, o.alpha_dev};
        }
        LAUNCH_CHECK();
        return 0;
    }
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(((D + 1) * (r + 1) + 255) / 256, n), dim3(256), 0, s, outs, nchunks, r);
    LAUNCH_CHECK();
    return 0;
}
int launch_wgrad(int precision, const WgradArgs& a, hipStream_t s) { return launch_wgrad(precision, &a, 1, s, nullptr); }

}  // namespace dyt
