// Attention on fp32 operands taken as 16-bit hi / lo parts (x = hi + lo, hi = rn16(x), lo = rn16(x - hi)): the parity modes
// ("fp16x3" and its variants; routes AF_SPLIT_*, AB_SPLIT3 / AB_SPLIT1 of attn_route.h).  Every product runs on the 16-bit matrix
// cores as hi*hi + hi*lo + lo*hi with fp32 accumulation and fp32 softmax statistics; the tiling, LDS image layouts and lane mapping
// are those of the 16-bit kernels (attention_16.hip, whose head describes them; strides and fragment helpers in attn_common.h).
#include "attn_common.h"

namespace dyt {

// ------------------------------------------------------------------------------------------
// forward, fp32 operands as 16-bit hi / lo parts (the fp32 mode's DYT_OPT_F32_SPLIT16 form)
// ------------------------------------------------------------------------------------------
// The tiling, layouts and lane mapping of attn_fwd_bf16_kernel (attention_16.hip) with every product computed as hi*hi + hi*lo + lo*hi of two
// 16-bit parts per fp32 operand (x = hi + lo, hi = rn16(x), lo = rn16(x - hi); the dropped lo*lo term is 2^-22 relative): K as
// two row images, V^T as two transposed images (122.9 KB of LDS), q split in registers, the probabilities split per key tile
// right where they are packed.  fp32 accumulation, fp32 softmax statistics, fp32 output.  Persistent over heads, no
// cross-head prefetch (the fp32 rows would double the staging registers).
// exp(x) for the split kernels: v_exp_f32 of the compensated product x * log2(e) -- h = rn(x * L2E), l = the product's remainder plus
// x times the low part of log2(e), exp(x) = 2^h (1 + l ln 2) -- six instructions instead of libm expf's ~25, within ~1.5 ulp
// (a bare __expf is off by |x| 2^-24 relative: 2e-6 at the scores' range, the level of the whole split mode's error)
__device__ __forceinline__ float exp_c(float x) {
    x = fmaxf(x, -104.0f);   // masked scores (-inf, -1e30) would make h - h a NaN; exp(-104) is 0 in fp32 anyway
    const float L2E = 1.44269502162933349609375f, L2E_LO = 1.925962991e-8f;
    const float h = x * L2E;
    const float l = __fmaf_rn(x, L2E_LO, __fmaf_rn(x, L2E, -h));
    const float e = __builtin_amdgcn_exp2f(h);
    return __fmaf_rn(e * 0.693147182464599609375f, l, e);
}
__device__ __forceinline__ void split8(const f32x4& x0, const f32x4& x1, bf16x8& hi, bf16x8& lo) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const Split2 s0 = split2(x0[i]), s1 = split2(x1[i]);
        hi[i] = s0.hi; lo[i] = s0.lo;
        hi[4 + i] = s1.hi; lo[4 + i] = s1.lo;
    }
}
// PARTS = 1: the hi * hi product alone for S and P V (IEEE-half attention on the same planes, fp32 softmax): the complete_model pass of
// "fp16x3q", whose output no token-keep decision depends on (its budget is the 1e-3 logit bar, not the gate's 1e-5)
// LSE = false: the no-save variant (inference-only contexts; `lse` is null): the backward's row statistics are neither computed nor stored
template <bool PLANES, int PARTS = 3, bool LSE = true>   // PLANES: q / k / v arrive as 16-bit hi (q16 / k16 / v16) + lo planes written by the QKV epilogue: staged without conversion
__global__ __launch_bounds__(448) void attn_fwd_split_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                             const float* __restrict__ v, float* __restrict__ out,
                                                             float* __restrict__ lse, int nheads, bf16* __restrict__ out3,
                                                             bf16* __restrict__ q16, bf16* __restrict__ k16, bf16* __restrict__ v16,
                                                             bf16* __restrict__ o16, int f8, const bf16* __restrict__ qlo,
                                                             const bf16* __restrict__ klo, const bf16* __restrict__ vlo) {
    // q16 / k16 / v16 / o16 (optional): the hi parts = the 16-bit roundings of q, k, v and the output, saved for a backward pass that
    // runs on 16-bit operands ("fp16x3h"); `out` may then be null (the proj GEMM reads out3)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16* Kh = reinterpret_cast<bf16*>(smem);
    bf16* Kl = reinterpret_cast<bf16*>(smem + ROW_IMG);
    bf16* Vth = reinterpret_cast<bf16*>(smem + 2 * ROW_IMG);
    bf16* Vtl = reinterpret_cast<bf16*>(smem + 2 * ROW_IMG + TR_IMG);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int qrow = wave * 32 + l31, qr = min(qrow, NT - 1);
    for (int bh = blockIdx.x; bh < nheads; bh += gridDim.x) {
        const int b = bh / NH, h = bh - b * NH;
        // ---- stage K (two row images) and V (two transposed images): task = (row pair, 8-column chunk), 896 tasks / 448 threads
        const float* kb = k + (size_t)bh * NT * HD;
        const float* vb = v + (size_t)bh * NT * HD;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int t = tid + u * 448, pr = t >> 3, c = t & 7, r0 = pr * 2;
            bf16x8 ah, al, bhh, bl, vah, val, vbh, vbl;
            if constexpr (PLANES) {
                const size_t o0 = ((size_t)bh * NT + min(r0, NT - 1)) * HD + c * 8, o1 = ((size_t)bh * NT + min(r0 + 1, NT - 1)) * HD + c * 8;
                ah = *reinterpret_cast<const bf16x8*>(k16 + o0); bhh = *reinterpret_cast<const bf16x8*>(k16 + o1);
                vah = *reinterpret_cast<const bf16x8*>(v16 + o0); vbh = *reinterpret_cast<const bf16x8*>(v16 + o1);
                if constexpr (PARTS == 3) {
                    al = *reinterpret_cast<const bf16x8*>(klo + o0); bl = *reinterpret_cast<const bf16x8*>(klo + o1);
                    val = *reinterpret_cast<const bf16x8*>(vlo + o0); vbl = *reinterpret_cast<const bf16x8*>(vlo + o1);
                } else {
                    al = zero8(); bl = zero8(); val = zero8(); vbl = zero8();
                }
            } else {
            const float* k0 = kb + (size_t)min(r0, NT - 1) * HD + c * 8;
            const float* k1 = kb + (size_t)min(r0 + 1, NT - 1) * HD + c * 8;
            const float* v0 = vb + (size_t)min(r0, NT - 1) * HD + c * 8;
            const float* v1 = vb + (size_t)min(r0 + 1, NT - 1) * HD + c * 8;
            const f32x4 ka0 = *reinterpret_cast<const f32x4*>(k0), ka1 = *reinterpret_cast<const f32x4*>(k0 + 4);
            const f32x4 kb0 = *reinterpret_cast<const f32x4*>(k1), kb1 = *reinterpret_cast<const f32x4*>(k1 + 4);
            const f32x4 va0 = *reinterpret_cast<const f32x4*>(v0), va1 = *reinterpret_cast<const f32x4*>(v0 + 4);
            const f32x4 vb0 = *reinterpret_cast<const f32x4*>(v1), vb1 = *reinterpret_cast<const f32x4*>(v1 + 4);
            split8(ka0, ka1, ah, al); split8(kb0, kb1, bhh, bl);
            split8(va0, va1, vah, val); split8(vb0, vb1, vbh, vbl);
            }
            if (r0 >= NT) { ah = zero8(); al = zero8(); }
            if (r0 + 1 >= NT) { bhh = zero8(); bl = zero8(); }
            *reinterpret_cast<bf16x8*>(Kh + r0 * RLD + c * 8) = ah;
            *reinterpret_cast<bf16x8*>(Kh + (r0 + 1) * RLD + c * 8) = bhh;
            if constexpr (PARTS == 3) {
                *reinterpret_cast<bf16x8*>(Kl + r0 * RLD + c * 8) = al;
                *reinterpret_cast<bf16x8*>(Kl + (r0 + 1) * RLD + c * 8) = bl;
            }
            if (!PLANES && k16) {
                if (r0 < NT) *reinterpret_cast<bf16x8*>(k16 + ((size_t)bh * NT + r0) * HD + c * 8) = ah;
                if (r0 + 1 < NT) *reinterpret_cast<bf16x8*>(k16 + ((size_t)bh * NT + r0 + 1) * HD + c * 8) = bhh;
            }
            ah = vah; al = val; bhh = vbh; bl = vbl;
            if (r0 >= NT) { ah = zero8(); al = zero8(); }
            if (r0 + 1 >= NT) { bhh = zero8(); bl = zero8(); }
            if (!PLANES && v16) {
                if (r0 < NT) *reinterpret_cast<bf16x8*>(v16 + ((size_t)bh * NT + r0) * HD + c * 8) = ah;
                if (r0 + 1 < NT) *reinterpret_cast<bf16x8*>(v16 + ((size_t)bh * NT + r0 + 1) * HD + c * 8) = bhh;
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                bf16x2 ph = {ah[i], bhh[i]}, pl = {al[i], bl[i]};
                *reinterpret_cast<bf16x2*>(Vth + (c * 8 + i) * TLD + r0) = ph;
                if constexpr (PARTS == 3) *reinterpret_cast<bf16x2*>(Vtl + (c * 8 + i) * TLD + r0) = pl;
            }
        }
        // ---- this wave's 32 query rows, split
        bf16x8 qh[4], ql[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            if constexpr (PLANES) {
                const size_t o = ((size_t)bh * NT + qr) * HD + ks * 16 + hi * 8;
                qh[ks] = *reinterpret_cast<const bf16x8*>(q16 + o);
                if constexpr (PARTS == 3) ql[ks] = *reinterpret_cast<const bf16x8*>(qlo + o);
            } else {
            const float* qp = q + ((size_t)bh * NT + qr) * HD + ks * 16 + hi * 8;
            split8(*reinterpret_cast<const f32x4*>(qp), *reinterpret_cast<const f32x4*>(qp + 4), qh[ks], ql[ks]);
            if (q16 && qrow < NT) *reinterpret_cast<bf16x8*>(q16 + ((size_t)bh * NT + qrow) * HD + ks * 16 + hi * 8) = qh[ks];
            }
        }
        __syncthreads();
        f32x16 st[7];
#pragma unroll
        for (int kt = 0; kt < 7; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) st[kt][r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
            for (int kt = 0; kt < 7; ++kt) {
                const bf16x8 ah = *reinterpret_cast<const bf16x8*>(Kh + (kt * 32 + l31) * RLD + ks * 16 + hi * 8);
                if constexpr (PARTS == 3) {
                    const bf16x8 al = *reinterpret_cast<const bf16x8*>(Kl + (kt * 32 + l31) * RLD + ks * 16 + hi * 8);
                    st[kt] = MFMA32(al, qh[ks], st[kt]);   // small terms first
                    st[kt] = MFMA32(ah, ql[ks], st[kt]);
                }
                st[kt] = MFMA32(ah, qh[ks], st[kt]);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = 192 + (r & 3) + 8 * (r >> 2) + 4 * hi;
            if (key >= NT) st[6][r] = -INFINITY;
        }
        float mp[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
        for (int kt = 0; kt < 7; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) mp[r & 3] = fmaxf(mp[r & 3], st[kt][r]);
        float m = fmaxf(fmaxf(mp[0], mp[1]), fmaxf(mp[2], mp[3]));
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        float sp[4] = {0.f, 0.f, 0.f, 0.f};
        f32x16 o[2];
#pragma unroll
        for (int r = 0; r < 16; ++r) { o[0][r] = 0.f; o[1][r] = 0.f; }
#pragma unroll
        for (int kt = 0; kt < 7; ++kt) {
            bf16x8 vh[2][2], vl[2][2];
#pragma unroll
            for (int half = 0; half < 2; ++half)
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    vh[half][dt] = join44(Vth + (dt * 32 + l31) * TLD + kt * 32 + half * 16 + 4 * hi);
                    if constexpr (PARTS == 3) vl[half][dt] = join44(Vtl + (dt * 32 + l31) * TLD + kt * 32 + half * 16 + 4 * hi);
                }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                // (one-part form: a bare v_exp_f32 -- its |x| 2^-24 relative error is far below the half rounding of p)
                const float p = PARTS == 3 ? exp_c(st[kt][r] - m) : __builtin_amdgcn_exp2f((st[kt][r] - m) * 1.44269502162933349609375f);
                st[kt][r] = p;
                sp[r & 3] += p;
            }
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                bf16x8 ph, pl;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const Split2 sp2 = split2(st[kt][half * 8 + i]);
                    ph[i] = sp2.hi; pl[i] = sp2.lo;
                }
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    if constexpr (PARTS == 3) {
                        o[dt] = MFMA32(vl[half][dt], ph, o[dt]);
                        o[dt] = MFMA32(vh[half][dt], pl, o[dt]);
                    }
                    o[dt] = MFMA32(vh[half][dt], ph, o[dt]);
                }
            }
        }
        float sum = (sp[0] + sp[1]) + (sp[2] + sp[3]);
        sum += __shfl_xor(sum, 32, 64);
        if constexpr (LSE) { if (hi == 0 && qrow < NT) lse[(size_t)bh * NT + qrow] = m + logf(sum); }
        if (qrow < NT) {
            const float inv = 1.0f / sum;
            float* op = out ? out + ((size_t)b * NT + qrow) * D + h * HD : nullptr;
            bf16* op16 = o16 ? o16 + ((size_t)b * NT + qrow) * D + h * HD : nullptr;
            bf16* op3 = out3 ? out3 + ((size_t)b * NT + qrow) * (SPLIT_A * D) + h * HD : nullptr;   // + the split operand of the proj GEMM
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int d = dt * 32 + 8 * g + 4 * hi;
                    const float o0 = o[dt][4 * g] * inv, o1 = o[dt][4 * g + 1] * inv, o2 = o[dt][4 * g + 2] * inv, o3 = o[dt][4 * g + 3] * inv;
                    if (op) store4(op + d, o0, o1, o2, o3);
                    if (op16) store4(op16 + d, o0, o1, o2, o3);
                    if (op3) { if (f8) store4_split_f8(op3 - h * HD, D, h * HD + d, o0, o1, o2, o3); else store4_split3(op3 + d, D, o0, o1, o2, o3); }
                }
        }
        __syncthreads();   // every wave is done with this head's images before they are overwritten
    }
}

// ------------------------------------------------------------------------------------------
// backward, fp32 operands as 16-bit hi / lo parts (DYT_OPT_F32_SPLIT16)
// ------------------------------------------------------------------------------------------
// The two-kernel backward of the bf16 path (dQ per query tile, dK/dV per key tile, lane mapping and fragment layouts unchanged)
// with every product as hi*hi + hi*lo + lo*hi.  Every LDS image exists twice (hi, lo), so a head is staged in two HALVES of
// 128 rows (keys for dQ: 108 KB; queries for dK/dV: 142 KB); the accumulators live across the halves.  fp32 in, fp32
// statistics (lse, delta), output either fp32 or -- times s3 -- directly as the split operand of the qkv dgrad GEMM.
// dO is multiplied by gs (a power of two) before it is split, which carries through dP, dS, dQ, dK, dV: gradient-sized values
// would otherwise put their lo parts (and many hi parts) into the fp16 subnormals; the outputs are divided by gs again.
constexpr int HROWS = 128;                 // rows staged per half (4 tiles of 32; the second half holds tiles 4..6)
constexpr int TLDH = HROWS + 4;            // 16-bit elements per row of a transposed half image (264 B: conflict-free b64 reads)
constexpr int ROW_H = HROWS * RLD * 2;     // 18432 B
constexpr int TR_H = HD * TLDH * 2;        // 16896 B

// rows [row0, row0 + 128) of a [197][64] fp32 matrix (row stride ld) -> hi / lo row images and / or hi / lo transposed images
__device__ __forceinline__ void stage_split_half(const float* __restrict__ src, size_t ld, int row0, bf16* rH, bf16* rL, bf16* tH,
                                                 bf16* tL, int tid, float scale = 1.0f) {
    for (int t = tid; t < (HROWS / 2) * 8; t += 448) {
        const int pr = t >> 3, c = t & 7, r0 = pr * 2, g0 = row0 + r0;
        const float* p0 = src + (size_t)min(g0, NT - 1) * ld + c * 8;
        const float* p1 = src + (size_t)min(g0 + 1, NT - 1) * ld + c * 8;
        const f32x4 a0 = *reinterpret_cast<const f32x4*>(p0) * scale, a1 = *reinterpret_cast<const f32x4*>(p0 + 4) * scale;
        const f32x4 b0 = *reinterpret_cast<const f32x4*>(p1) * scale, b1 = *reinterpret_cast<const f32x4*>(p1 + 4) * scale;
        bf16x8 ah, al, bh, bl;
        split8(a0, a1, ah, al); split8(b0, b1, bh, bl);
        if (g0 >= NT) { ah = zero8(); al = zero8(); }
        if (g0 + 1 >= NT) { bh = zero8(); bl = zero8(); }
        if (rH) {
            *reinterpret_cast<bf16x8*>(rH + r0 * RLD + c * 8) = ah;
            *reinterpret_cast<bf16x8*>(rH + (r0 + 1) * RLD + c * 8) = bh;
        }
        if (rL) {   // (null where only one-part products read the image: the lo half is never looked at)
            *reinterpret_cast<bf16x8*>(rL + r0 * RLD + c * 8) = al;
            *reinterpret_cast<bf16x8*>(rL + (r0 + 1) * RLD + c * 8) = bl;
        }
        if (tH) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                bf16x2 ph = {ah[i], bh[i]};
                *reinterpret_cast<bf16x2*>(tH + (c * 8 + i) * TLDH + r0) = ph;
            }
        }
        if (tL) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                bf16x2 pl = {al[i], bl[i]};
                *reinterpret_cast<bf16x2*>(tL + (c * 8 + i) * TLDH + r0) = pl;
            }
        }
    }
}
__device__ __forceinline__ void split_pack8(const f32x16& v, int base, bf16x8& hi, bf16x8& lo) {
#pragma unroll
    for (int i = 0; i < 8; ++i) { const Split2 s2 = split2(v[base + i]); hi[i] = s2.hi; lo[i] = s2.lo; }
}
// acc += A B with A = (ah, al), B = (bh, bl): small terms first
#define MFMA3(acc, ah, al, bh, bl) do { acc = MFMA32(al, bh, acc); acc = MFMA32(ah, bl, acc); acc = MFMA32(ah, bh, acc); } while (0)
// the gradient products (dP, dQ, dK, dV) of the backward kernels: GP = 3 as above, GP = 1 the hi * hi product alone (the score
// recomputation always takes three: an error of S is an error of the exponent)
#define MFMAG(acc, ah, al, bh, bl) do { if constexpr (GP == 3) MFMA3(acc, ah, al, bh, bl); else acc = MFMA32(ah, bh, acc); } while (0)

template <int GP>
__global__ __launch_bounds__(448) void attn_bwd_dq_split_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                const float* __restrict__ v, const float* __restrict__ o,
                                                                const float* __restrict__ dout, const float* __restrict__ lse,
                                                                float* __restrict__ delta, float* __restrict__ dqkv,
                                                                bf16* __restrict__ dqkv3, float s3, int nheads, float gs, int hi_only) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16* Kh = reinterpret_cast<bf16*>(smem);
    bf16* Kl = reinterpret_cast<bf16*>(smem + ROW_H);
    bf16* Vh = reinterpret_cast<bf16*>(smem + 2 * ROW_H);
    bf16* Vl = reinterpret_cast<bf16*>(smem + 3 * ROW_H);
    bf16* Kth = reinterpret_cast<bf16*>(smem + 4 * ROW_H);
    bf16* Ktl = reinterpret_cast<bf16*>(smem + 4 * ROW_H + TR_H);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int qrow = wave * 32 + l31, qr = min(qrow, NT - 1);
    for (int bh = blockIdx.x; bh < nheads; bh += gridDim.x) {
        const int b = bh / NH, h = bh - b * NH;
        bf16x8 qh[4], ql[4], doh[4], dol[4];
        float dl = 0.f;
        {
            const float* qp = q + ((size_t)bh * NT + qr) * HD + hi * 8;
            const size_t trow = ((size_t)b * NT + qr) * D + h * HD + hi * 8;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const f32x4 q0 = *reinterpret_cast<const f32x4*>(qp + ks * 16), q1 = *reinterpret_cast<const f32x4*>(qp + ks * 16 + 4);
                const f32x4 d0 = *reinterpret_cast<const f32x4*>(dout + trow + ks * 16), d1 = *reinterpret_cast<const f32x4*>(dout + trow + ks * 16 + 4);
                const f32x4 o0 = *reinterpret_cast<const f32x4*>(o + trow + ks * 16), o1 = *reinterpret_cast<const f32x4*>(o + trow + ks * 16 + 4);
                split8(q0, q1, qh[ks], ql[ks]);
                split8(d0 * gs, d1 * gs, doh[ks], dol[ks]);
#pragma unroll
                for (int i = 0; i < 4; ++i) dl += d0[i] * o0[i] + d1[i] * o1[i];
            }
        }
        const float L = lse[(size_t)bh * NT + qr];
        dl += __shfl_xor(dl, 32, 64);
        if (hi == 0 && qrow < NT) delta[(size_t)bh * NT + qrow] = dl;
        const float dlg = dl * gs;
        f32x16 dq[2];
#pragma unroll
        for (int r = 0; r < 16; ++r) { dq[0][r] = 0.f; dq[1][r] = 0.f; }
#pragma unroll 1
        for (int hf = 0; hf < 2; ++hf) {
            __syncthreads();   // the previous half's (head's) images are no longer read
            stage_split_half(k + (size_t)bh * NT * HD, HD, hf * HROWS, Kh, Kl, Kth, GP == 3 ? Ktl : nullptr, tid);
            stage_split_half(v + (size_t)bh * NT * HD, HD, hf * HROWS, Vh, GP == 3 ? Vl : nullptr, nullptr, nullptr, tid);
            __syncthreads();
            const int ntile = hf == 0 ? 4 : 3;
#pragma unroll 1
            for (int t = 0; t < ntile; ++t) {
                f32x16 s_, dp_;
#pragma unroll
                for (int r = 0; r < 16; ++r) { s_[r] = 0.f; dp_[r] = 0.f; }
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    const int off = (t * 32 + l31) * RLD + ks * 16 + hi * 8;
                    const bf16x8 kah = *reinterpret_cast<const bf16x8*>(Kh + off), kal = *reinterpret_cast<const bf16x8*>(Kl + off);
                    const bf16x8 vah = *reinterpret_cast<const bf16x8*>(Vh + off), val = *reinterpret_cast<const bf16x8*>(Vl + off);
                    MFMA3(s_, kah, kal, qh[ks], ql[ks]);
                    MFMAG(dp_, vah, val, doh[ks], dol[ks]);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = (hf * 4 + t) * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    const float p = key < NT ? exp_c(s_[r] - L) : 0.f;
                    s_[r] = p * (dp_[r] - dlg);       // gs * dS^T
                }
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    bf16x8 dsh, dsl;
                    split_pack8(s_, half * 8, dsh, dsl);
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt) {
                        const int toff = (dt * 32 + l31) * TLDH + t * 32 + half * 16 + 4 * hi;
                        const bf16x8 kth = join44(Kth + toff), ktl = join44(Ktl + toff);
                        MFMAG(dq[dt], kth, ktl, dsh, dsl);   // dQ^T[d][q] += K^T[d][key] dS^T[key][q]
                    }
                }
            }
        }
        if (qrow < NT) {
            const float sc = 0.125f * (dqkv3 ? s3 : 1.0f) / gs;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int d = dt * 32 + 8 * g + 4 * hi;
                    if (dqkv3) store4_split3(dqkv3 + ((size_t)b * NT + qrow) * (SPLIT_A * 3 * D) + h * HD + d, 3 * D, dq[dt][4 * g] * sc, dq[dt][4 * g + 1] * sc,
                                             dq[dt][4 * g + 2] * sc, dq[dt][4 * g + 3] * sc, hi_only != 0);
                    else store4(dqkv + ((size_t)b * NT + qrow) * (3 * D) + h * HD + d, dq[dt][4 * g] * sc, dq[dt][4 * g + 1] * sc,
                                dq[dt][4 * g + 2] * sc, dq[dt][4 * g + 3] * sc);
                }
        }
    }
}

template <int GP>
__global__ __launch_bounds__(448) void attn_bwd_dkv_split_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                 const float* __restrict__ v, const float* __restrict__ dout,
                                                                 const float* __restrict__ lse, const float* __restrict__ delta,
                                                                 float* __restrict__ dqkv, bf16* __restrict__ dqkv3, float s3, int nheads, float gs, int hi_only) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16* Qh = reinterpret_cast<bf16*>(smem);
    bf16* Ql = reinterpret_cast<bf16*>(smem + ROW_H);
    bf16* Dh = reinterpret_cast<bf16*>(smem + 2 * ROW_H);
    bf16* Dl = reinterpret_cast<bf16*>(smem + 3 * ROW_H);
    bf16* Qth = reinterpret_cast<bf16*>(smem + 4 * ROW_H);
    bf16* Qtl = reinterpret_cast<bf16*>(smem + 4 * ROW_H + TR_H);
    bf16* Dth = reinterpret_cast<bf16*>(smem + 4 * ROW_H + 2 * TR_H);
    bf16* Dtl = reinterpret_cast<bf16*>(smem + 4 * ROW_H + 3 * TR_H);
    float* lse_s = reinterpret_cast<float*>(smem + 4 * ROW_H + 4 * TR_H);
    float* del_s = lse_s + HROWS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int key = wave * 32 + l31, kr_ = min(key, NT - 1);
    for (int bh = blockIdx.x; bh < nheads; bh += gridDim.x) {
        const int b = bh / NH, h = bh - b * NH;
        bf16x8 kh[4], kl[4], vh[4], vl[4];
        {
            const float* kp = k + ((size_t)bh * NT + kr_) * HD + hi * 8;
            const float* vp = v + ((size_t)bh * NT + kr_) * HD + hi * 8;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                split8(*reinterpret_cast<const f32x4*>(kp + ks * 16), *reinterpret_cast<const f32x4*>(kp + ks * 16 + 4), kh[ks], kl[ks]);
                split8(*reinterpret_cast<const f32x4*>(vp + ks * 16), *reinterpret_cast<const f32x4*>(vp + ks * 16 + 4), vh[ks], vl[ks]);
            }
        }
        f32x16 aK[2], aV[2];
#pragma unroll
        for (int r = 0; r < 16; ++r) { aK[0][r] = 0.f; aK[1][r] = 0.f; aV[0][r] = 0.f; aV[1][r] = 0.f; }
#pragma unroll 1
        for (int hf = 0; hf < 2; ++hf) {
            __syncthreads();
            stage_split_half(q + (size_t)bh * NT * HD, HD, hf * HROWS, Qh, Ql, Qth, GP == 3 ? Qtl : nullptr, tid);
            stage_split_half(dout + (size_t)b * NT * D + h * HD, D, hf * HROWS, Dh, GP == 3 ? Dl : nullptr, Dth, GP == 3 ? Dtl : nullptr, tid, gs);
            if (tid < HROWS) {
                const int qg = hf * HROWS + tid;
                lse_s[tid] = qg < NT ? lse[(size_t)bh * NT + qg] : 0.f;
                del_s[tid] = qg < NT ? delta[(size_t)bh * NT + qg] * gs : 0.f;
            }
            __syncthreads();
            const int ntile = hf == 0 ? 4 : 3;
#pragma unroll 1
            for (int t = 0; t < ntile; ++t) {
                f32x16 s, dp;
#pragma unroll
                for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    const int off = (t * 32 + l31) * RLD + ks * 16 + hi * 8;
                    const bf16x8 qah = *reinterpret_cast<const bf16x8*>(Qh + off), qal = *reinterpret_cast<const bf16x8*>(Ql + off);
                    const bf16x8 dah = *reinterpret_cast<const bf16x8*>(Dh + off), dal = *reinterpret_cast<const bf16x8*>(Dl + off);
                    MFMA3(s, qah, qal, kh[ks], kl[ks]);      // S[q][key]
                    MFMAG(dp, dah, dal, vh[ks], vl[ks]);     // dP[q][key]
                }
                f32x16 p;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int q0 = t * 32 + 8 * g + 4 * hi;   // row inside the half
                    const float4 L4 = *reinterpret_cast<const float4*>(lse_s + q0);
                    const float4 D4 = *reinterpret_cast<const float4*>(del_s + q0);
                    const float Ls[4] = {L4.x, L4.y, L4.z, L4.w};
                    const float Ds[4] = {D4.x, D4.y, D4.z, D4.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int r = 4 * g + e;
                        const bool ok = (hf * HROWS + q0 + e < NT) && (key < NT);
                        const float pv = ok ? exp_c(s[r] - Ls[e]) : 0.f;
                        p[r] = pv;
                        s[r] = pv * (dp[r] - Ds[e]);  // dS
                    }
                }
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    bf16x8 ph, pl, dsh, dsl;
                    split_pack8(p, half * 8, ph, pl);
                    split_pack8(s, half * 8, dsh, dsl);
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt) {
                        const int toff = (dt * 32 + l31) * TLDH + t * 32 + half * 16 + 4 * hi;
                        const bf16x8 doth = join44(Dth + toff), dotl = join44(Dtl + toff);
                        const bf16x8 qth = join44(Qth + toff), qtl = join44(Qtl + toff);
                        MFMAG(aV[dt], doth, dotl, ph, pl);    // dV^T[d][key] += dO^T[d][q] P[q][key]
                        MFMAG(aK[dt], qth, qtl, dsh, dsl);    // dK^T[d][key] += Q^T[d][q] dS[q][key]
                    }
                }
            }
        }
        if (key < NT) {
            const float sc = (dqkv3 ? s3 : 1.0f) / gs;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int d = dt * 32 + 8 * g + 4 * hi;
                    if (dqkv3) {
                        bf16* op3 = dqkv3 + ((size_t)b * NT + key) * (SPLIT_A * 3 * D) + h * HD + d;
                        store4_split3(op3 + D, 3 * D, aK[dt][4 * g] * sc, aK[dt][4 * g + 1] * sc, aK[dt][4 * g + 2] * sc, aK[dt][4 * g + 3] * sc, hi_only != 0);
                        store4_split3(op3 + 2 * D, 3 * D, aV[dt][4 * g] * sc, aV[dt][4 * g + 1] * sc, aV[dt][4 * g + 2] * sc, aV[dt][4 * g + 3] * sc, hi_only != 0);
                    } else {
                        float* op = dqkv + ((size_t)b * NT + key) * (3 * D) + h * HD + d;
                        store4(op + D, aK[dt][4 * g] * sc, aK[dt][4 * g + 1] * sc, aK[dt][4 * g + 2] * sc, aK[dt][4 * g + 3] * sc);
                        store4(op + 2 * D, aV[dt][4 * g] * sc, aV[dt][4 * g + 1] * sc, aV[dt][4 * g + 2] * sc, aV[dt][4 * g + 3] * sc);
                    }
                }
        }
    }
}

template <bool PLANES, int PARTS, bool LSE>   // PLANES: the hi planes take the place of the 16-bit copies of q / k / v
static int launch_fwd_split(const AttnFwdArgs& a, hipStream_t s) {
    constexpr auto kern = attn_fwd_split_kernel<PLANES, PARTS, LSE>;
    const int grid = a.batch * NH;
    const size_t lds = 2 * ROW_IMG + 2 * TR_IMG;
    if (int rc = ensure_dyn_lds<kern>(lds)) return rc;
    hipLaunchKernelGGL(kern, dim3(min(grid, 256)), dim3(448), lds, s, (const float*)(PLANES ? nullptr : a.q), (const float*)(PLANES ? nullptr : a.k),
                       (const float*)(PLANES ? nullptr : a.v), (float*)a.out, LSE ? a.lse : nullptr, grid, (bf16*)a.out3,
                       (bf16*)(PLANES ? a.q_hi : a.q16), (bf16*)(PLANES ? a.k_hi : a.k16), (bf16*)(PLANES ? a.v_hi : a.v16), (bf16*)a.o16, (int)a.out3_f8,
                       (const bf16*)(PLANES ? a.q_lo : nullptr), (const bf16*)(PLANES ? a.k_lo : nullptr), (const bf16*)(PLANES ? a.v_lo : nullptr));
    DYT_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_attn_fwd_split(const AttnFwdArgs& a, const AttnFwdRoute& r, hipStream_t s) {
    switch (r.kernel) {
        case AF_SPLIT_F32: return launch_fwd_split<false, 3, true>(a, s);
        case AF_SPLIT_P3: return launch_fwd_split<true, 3, true>(a, s);
        case AF_SPLIT_P1: return launch_fwd_split<true, 1, true>(a, s);
        case AF_SPLIT_F32_NOSAVE: return launch_fwd_split<false, 3, false>(a, s);
        case AF_SPLIT_P3_NOSAVE: return launch_fwd_split<true, 3, false>(a, s);
        case AF_SPLIT_P1_NOSAVE: return launch_fwd_split<true, 1, false>(a, s);
        default: set_error("attention forward: not a split kernel"); return -1;
    }
}

int launch_attn_bwd_split(const AttnBwdArgs& a, const AttnBwdRoute& r, hipStream_t s) {
    const int grid = a.batch * NH;
    const size_t lds1 = 4 * ROW_H + 2 * TR_H, lds2 = 4 * ROW_H + 4 * TR_H + 2 * HROWS * sizeof(float);
    if (int rc = ensure_dyn_lds<attn_bwd_dq_split_kernel<3>, attn_bwd_dq_split_kernel<1>>(lds1)) return rc;
    if (int rc = ensure_dyn_lds<attn_bwd_dkv_split_kernel<3>, attn_bwd_dkv_split_kernel<1>>(lds2)) return rc;
    auto* kq = r.kernel == AB_SPLIT3 ? attn_bwd_dq_split_kernel<3> : attn_bwd_dq_split_kernel<1>;
    auto* kkv = r.kernel == AB_SPLIT3 ? attn_bwd_dkv_split_kernel<3> : attn_bwd_dkv_split_kernel<1>;
    const float gs = a.dqkv3 ? a.s3 : 4096.0f;   // (4096: unit entries, no context)
    hipLaunchKernelGGL(kq, dim3(min(grid, 256)), dim3(448), lds1, s, (const float*)a.q, (const float*)a.k, (const float*)a.v, (const float*)a.out,
                       (const float*)a.dout, a.lse, a.delta, (float*)a.dqkv, (bf16*)a.dqkv3, a.s3, grid, gs, (int)a.out_hi_only);
    hipLaunchKernelGGL(kkv, dim3(min(grid, 256)), dim3(448), lds2, s, (const float*)a.q, (const float*)a.k, (const float*)a.v, (const float*)a.dout,
                       a.lse, a.delta, (float*)a.dqkv, (bf16*)a.dqkv3, a.s3, grid, gs, (int)a.out_hi_only);
    DYT_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace dyt
