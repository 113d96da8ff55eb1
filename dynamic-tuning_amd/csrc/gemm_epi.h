// Epilogue functors of the GEMM family (included by gemm.hip): what each EpiKind of kernels.h does with an accumulator tile.
#pragma once

namespace dyt {

// ------------------------------------------------------------------------------------------
// epilogues.  One functor call handles 4 consecutive columns of one output row, in three parts so that
// the MFMA kernel can keep memory latency off the critical path:
//   col_init(col)            per-lane column constants (bias ...): a lane's column is the same for every
//                            chunk it handles, so this is loaded ONCE per tile
//   pre(row, col)            the functor's own global loads (residual, gelu', row maps), returned RAW so
//                            that a whole pass worth of them is in flight before the first use
//   apply(row, col, v, c, p) the arithmetic and the stores
// ------------------------------------------------------------------------------------------
struct NoCtx {};
struct Bias4 { float b[4]; };
__device__ __forceinline__ Bias4 load_bias4(const float* bias, int col) {
    Bias4 r;
    if (bias) { r.b[0] = bias[col]; r.b[1] = bias[col + 1]; r.b[2] = bias[col + 2]; r.b[3] = bias[col + 3]; }
    else { r.b[0] = r.b[1] = r.b[2] = r.b[3] = 0.f; }
    return r;
}
template <class T> struct Raw4;   // 4 consecutive activations as loaded (conversion deferred to the use)
template <> struct Raw4<float> {
    float4 v;
    __device__ __forceinline__ void get(float (&o)[4]) const { o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w; }
};
template <> struct Raw4<bf16> {
    bf16x4 v;
    __device__ __forceinline__ void get(float (&o)[4]) const {
        o[0] = (float)v[0]; o[1] = (float)v[1]; o[2] = (float)v[2]; o[3] = (float)v[3];
    }
};
__device__ __forceinline__ Raw4<float> load_raw4(const float* p) { return {*reinterpret_cast<const float4*>(p)}; }
__device__ __forceinline__ Raw4<bf16> load_raw4(const bf16* p) { return {*reinterpret_cast<const bf16x4*>(p)}; }
// streaming store: the value is not read again soon (gelu' is consumed by the backward pass) -- keeps the
// write burst out of the L2 lines the main loops of the other workgroups are hitting
__device__ __forceinline__ void store4_nt(float* p, float a, float b, float c, float d) {
    f32x4 v = {a, b, c, d};
    DYT_NT_STORE(v, reinterpret_cast<f32x4*>(p));
}
__device__ __forceinline__ void store4_nt(bf16* p, float a, float b, float c, float d) {
    bf16x4 v = {(bf16)a, (bf16)b, (bf16)c, (bf16)d};
    DYT_NT_STORE(v, reinterpret_cast<bf16x4*>(p));
}
struct EpiBiasF32 {
    const float* bias; float* out; int ld;
    typedef Bias4 Col; typedef NoCtx Pre;
    __device__ __forceinline__ Col col_init(int col) const { return load_bias4(bias, col); }
    __device__ __forceinline__ Pre pre(int, int) const { return {}; }
    __device__ __forceinline__ void apply(int row, int col, const float (&a)[4], const Col& c, const Pre&) const {
        store4(out + (size_t)row * ld + col, a[0] + c.b[0], a[1] + c.b[1], a[2] + c.b[2], a[3] + c.b[3]);
    }
};

template <class AT>
struct EpiQKV {
    const float* bias; AT* q; AT* k; AT* v;
    struct Col { Bias4 b; AT* base; float s; };
    typedef NoCtx Pre;
    __device__ __forceinline__ Col col_init(int col) const {
        const int which = col / D;
        const int c = col - which * D;
        const int h = c >> 6, d = c & 63;
        Col r;
        r.b = load_bias4(bias, col);
        r.s = which == 0 ? 0.125f : 1.0f;  // head_dim ** -0.5, exact in every dtype
        r.base = (which == 0 ? q : (which == 1 ? k : v)) + (((size_t)h * NT) << 6) + d;
        return r;
    }
    __device__ __forceinline__ Pre pre(int, int) const { return {}; }
    __device__ __forceinline__ void apply(int row, int, const float (&a)[4], const Col& c, const Pre&) const {
        const int b = row / NT, n = row - b * NT;
        AT* dst = c.base + (((size_t)b * NH * NT + n) << 6);
        store4(dst, (a[0] + c.b.b[0]) * c.s, (a[1] + c.b.b[1]) * c.s, (a[2] + c.b.b[2]) * c.s, (a[3] + c.b.b[3]) * c.s);
    }
};

// q / k / v of the split forms as two 16-bit planes each (hi = rn16(x), lo = rn16(x - hi), layout [B*12][197][64] like the fp32 tensors they
// replace, the same bytes): the split attention kernel stages them without conversion work and the hi planes ARE the 16-bit q / k / v a
// 16-bit backward pass reads (dyt_ctx::bwd16)
struct EpiQKVPlanes {
    const float* bias; bf16 *qh, *kh, *vh, *ql, *kl, *vl;
    struct Col { Bias4 b; bf16* bh; bf16* bl; float s; };
    typedef NoCtx Pre;
    __device__ __forceinline__ Col col_init(int col) const {
        const int which = col / D;
        const int c = col - which * D;
        const int h = c >> 6, d = c & 63;
        Col r;
        r.b = load_bias4(bias, col);
        r.s = which == 0 ? 0.125f : 1.0f;
        const size_t off = (((size_t)h * NT) << 6) + d;
        r.bh = (which == 0 ? qh : (which == 1 ? kh : vh)) + off;
        r.bl = (which == 0 ? ql : (which == 1 ? kl : vl)) + off;
        return r;
    }
    __device__ __forceinline__ Pre pre(int, int) const { return {}; }
    __device__ __forceinline__ void apply(int row, int, const float (&a)[4], const Col& c, const Pre&) const {
        const int b = row / NT, n = row - b * NT;
        const size_t o = ((size_t)b * NH * NT + n) << 6;
        const Split2 s0 = split2((a[0] + c.b.b[0]) * c.s), s1 = split2((a[1] + c.b.b[1]) * c.s), s2 = split2((a[2] + c.b.b[2]) * c.s),
                     s3 = split2((a[3] + c.b.b[3]) * c.s);
        *reinterpret_cast<bf16x4*>(c.bh + o) = bf16x4{s0.hi, s1.hi, s2.hi, s3.hi};
        *reinterpret_cast<bf16x4*>(c.bl + o) = bf16x4{s0.lo, s1.lo, s2.lo, s3.lo};
    }
};

// OT: type of the optional operand copy (the 16-bit type in the fp32 split form whose backward runs on 16-bit operands: GemmArgs::save16)
// STATS: LayerNorm statistics of the row just produced, for the GEMM that consumes LN(row) in the folded form (GemmArgs::ln_part).  The
// epilogue sweep gives 16 consecutive lanes 64 consecutive columns of one row (ch = tid % (BN / 4), BN / 4 a multiple of 16), so a
// group's (sum, sum of squares about its own mean) is two 4-step DPP reductions inside the lane row -- no LDS, no atomics, fixed order
template <class AT, class OT = AT, bool STATS = false>
struct EpiBiasResid {
    const float* bias; const float* resid; float* out; OT* out_at; int ld;
    float2* part = nullptr;
    const float* rs = nullptr;   // stochastic depth (GemmArgs::row_scale): the branch (acc + bias) of image row / 197 is multiplied by rs[image]
    typedef Bias4 Col; typedef Raw4<float> Pre;
    __device__ __forceinline__ Col col_init(int col) const { return load_bias4(bias, col); }
    __device__ __forceinline__ Pre pre(int row, int col) const { return load_raw4(resid + (size_t)row * ld + col); }
    __device__ __forceinline__ void apply(int row, int col, const float (&a)[4], const Col& c, const Pre& p) const {
        const size_t o = (size_t)row * ld + col;
        float r[4];
        p.get(r);
        float v0 = a[0] + c.b[0] + r[0], v1 = a[1] + c.b[1] + r[1];
        float v2 = a[2] + c.b[2] + r[2], v3 = a[3] + c.b[3] + r[3];
        if (rs) {   // (uniform branch; off the default path)
            const float sc = rs[row / NT];
            v0 = fmaf(sc, a[0] + c.b[0], r[0]); v1 = fmaf(sc, a[1] + c.b[1], r[1]);
            v2 = fmaf(sc, a[2] + c.b[2], r[2]); v3 = fmaf(sc, a[3] + c.b[3], r[3]);
        }
        store4(out + o, v0, v1, v2, v3);
        if (out_at) store4(out_at + o, v0, v1, v2, v3);
        if constexpr (STATS) {
            const float sum = row16_sum((v0 + v1) + (v2 + v3));
            const float m = sum * (1.0f / 64.0f);
            const float d0 = v0 - m, d1 = v1 - m, d2 = v2 - m, d3 = v3 - m;
            const float m2 = row16_sum(fmaf(d0, d0, d1 * d1) + fmaf(d2, d2, d3 * d3));
            if ((col & 63) == 0) part[(size_t)row * LN_PARTS + (col >> 6)] = make_float2(sum, m2);
        }
    }
};

// FAST (fp32 functor of the split forms): Phi by Abramowitz-Stegun 26.2.17 (the 16-bit functor's: |h err| 4e-7, |gelu' err| 3e-7 absolute,
// one v_exp + one v_rcp per element, packed fp32) instead of erff + expf -- below the split GEMMs' own 1e-6 and a tenth of the VALU work
// LNF: LayerNorm folded in (GemmArgs::ln_st): the accumulator is u16 . (gamma W)^T of the un-normalised row; z = rstd (acc - mean cs) + bias'
template <class AT, bool HAS_GP, class GT = AT, bool FAST = false, bool LNF = false>   // GT: type gelu'(z) is saved in (GemmArgs::save16: 16 bits under fp32 arithmetic)
struct EpiFc1 {
    const float* bias; AT* h; GT* gp; int ld;   // gp: gelu'(z), kept for the backward pass (training only)
    bf16* h3;   // split fp32 form: h goes out as the 16-bit hi / hi / lo operand of the fc2 GEMM ([rows, 3 ld]) instead of as fp32
    int f8 = 0; // ... in the hi16 / fp8 form (store4_split_f8)
    // LNF: column sums of W'; (mean, rstd) per LOGICAL row from ln_st (tile shapes without a statistics prologue: a pre-pass filled it), or --
    // RowStats kernels (gemm_bpre.h) -- merged from the producer's partials ln_part in the kernel prologue, which also leaves them in st_out
    const float* ln_cs = nullptr; const float2* ln_st = nullptr; const float2* ln_part = nullptr; float2* st_out = nullptr;
    struct ColF { float b[4]; float cs[4]; };
    typedef typename std::conditional<LNF, ColF, Bias4>::type Col;
    typedef typename std::conditional<LNF, float2, NoCtx>::type Pre;
    __device__ __forceinline__ Col col_init(int col) const {
        if constexpr (LNF) {
            ColF c;
            const Bias4 b4 = load_bias4(bias, col), c4 = load_bias4(ln_cs, col);
#pragma unroll
            for (int i = 0; i < 4; ++i) { c.b[i] = b4.b[i]; c.cs[i] = c4.b[i]; }
            return c;
        } else {
            return load_bias4(bias, col);
        }
    }
    __device__ __forceinline__ Pre pre(int row, int) const {
        if constexpr (LNF) return ln_st[row];   // (RowStats kernels do not call this)
        else return {};
    }
    __device__ __forceinline__ void apply(int row, int col, const float (&a)[4], const Col& c, const Pre& p) const {
        const size_t o = (size_t)row * ld + col;
        float hv[4], gv[4], z[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if constexpr (LNF) z[i] = fmaf(p.y, fmaf(-p.x, c.cs[i], a[i]), c.b[i]);
            else z[i] = a[i] + c.b[i];
        }
        if (HAS_GP) {
            if constexpr (sizeof(AT) == 2 || FAST) {   // two elements per packed-fp32 issue slot
#pragma unroll
                for (int i = 0; i < 4; i += 2) {
                    f32x2 h2, g2;
                    gelu_both_x2(f32x2{z[i], z[i + 1]}, h2, g2);
                    hv[i] = h2[0]; hv[i + 1] = h2[1]; gv[i] = g2[0]; gv[i + 1] = g2[1];
                }
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) gelu_both<AT>(z[i], hv[i], gv[i]);
            }
            store4_nt(gp + o, gv[0], gv[1], gv[2], gv[3]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) hv[i] = FAST ? gelu_fwd<bf16>(z[i]) : gelu_fwd<AT>(z[i]);
        }
        if constexpr (sizeof(AT) == 4) {
            if (h3) {
                if (f8) store4_split_f8(h3 + (size_t)row * SPLIT_A * ld, ld, col, hv[0], hv[1], hv[2], hv[3]);
                else store4_split3(h3 + (size_t)row * SPLIT_A * ld + col, ld, hv[0], hv[1], hv[2], hv[3]);
                return;
            }
        }
        store4(h + o, hv[0], hv[1], hv[2], hv[3]);
    }
};

// functors whose Pre is a per-row float2 that a kernel with a statistics prologue provides from LDS instead of calling pre()
template <class E> struct RowStats : std::false_type {};
template <class AT, bool G, class GT, bool F> struct RowStats<EpiFc1<AT, G, GT, F, true>> : std::true_type {};

// PLAIN = no row map and no row mask (teacher pass / dense rows): the per-chunk context is then just the 16 B of the residual,
// small enough for the kernels to issue a whole pass of residual loads ahead of the staging barriers (PRE_ALL); with the
// 32-byte {dst, mask, residual} context of the general form the loads sit right in front of their use.
// `resid` is the residual the row is added to (x itself for the in-place form; the block's `u` when the adapter's
// up-projection rides along as an extra k-tile of the contraction (CatArgs): x = u + (h W2^T + b2) + (d_act (s Wup)^T + s b_up)
// is then ONE read of u and ONE write of x instead of two fp32 read-modify-write passes over [M,768]).
template <class AT, bool PLAIN, class HT = AT>   // HT: type the MLP output is saved in for the gate gradient (GemmArgs::save16)
struct EpiFc2 {
    const float* bias; float* x; const int* row_map; const float* row_mask; HT* h_out;
    const float* resid; const float* bias2; float scale2;
    const float* rs = nullptr;   // stochastic depth (GemmArgs::row_scale): the MLP branch of token row t is multiplied by rs[t / 197] (h_out keeps the unscaled value)
    // b: what is added to the accumulator for x (fc2 bias + s * up-projection bias); hb: the same for the saved MLP output h_out
    // (fc2 bias only: with the up-projection riding on the contraction h_out = mlp(x) + s up_nobias(d_act), and tok_bwd takes
    // <g, s up_nobias(d_act)> back out of the gate gradient -- without the bias term it needs no 768-wide dot for that)
    struct ColH { float b[4]; float hb[4]; };
    typedef typename std::conditional<PLAIN, Bias4, ColH>::type Col;
    struct PreG { int dst; float m; Raw4<float> r; };
    typedef typename std::conditional<PLAIN, Raw4<float>, PreG>::type Pre;
    __device__ __forceinline__ Col col_init(int col) const {
        Col c;
        const Bias4 c1 = load_bias4(bias, col);
#pragma unroll
        for (int i = 0; i < 4; ++i) c.b[i] = c1.b[i];
        if constexpr (!PLAIN) {
#pragma unroll
            for (int i = 0; i < 4; ++i) c.hb[i] = c1.b[i];
        }
        if (bias2) {
            const Bias4 c2 = load_bias4(bias2, col);
#pragma unroll
            for (int i = 0; i < 4; ++i) c.b[i] = fmaf(scale2, c2.b[i], c.b[i]);
        }
        return c;
    }
    __device__ __forceinline__ Pre pre(int row, int col) const {
        if constexpr (PLAIN) {
            return load_raw4(resid + (size_t)row * D + col);
        } else {
            Pre p;
            p.dst = row_map ? row_map[row] : row;
            p.m = row_mask ? row_mask[p.dst] : 1.0f;
            p.r = load_raw4(resid + (size_t)p.dst * D + col);   // in place when resid == x: this chunk is the only writer of these 4 values
            return p;
        }
    }
    __device__ __forceinline__ void apply(int row, int col, const float (&a)[4], const Col& c, const Pre& p) const {
        const float h0 = a[0] + c.b[0], h1 = a[1] + c.b[1], h2 = a[2] + c.b[2], h3 = a[3] + c.b[3];
        float r[4];
        if constexpr (PLAIN) {
            if (h_out) store4_nt(h_out + (size_t)row * D + col, h0, h1, h2, h3);   // read again only by the backward pass
            p.get(r);
            const float sc = rs ? rs[row / NT] : 1.0f;
            store4(x + (size_t)row * D + col, fmaf(sc, h0, r[0]), fmaf(sc, h1, r[1]), fmaf(sc, h2, r[2]), fmaf(sc, h3, r[3]));
        } else {
            if (h_out) store4_nt(h_out + (size_t)row * D + col, a[0] + c.hb[0], a[1] + c.hb[1], a[2] + c.hb[2], a[3] + c.hb[3]);
            p.r.get(r);
            const float m = rs ? p.m * rs[p.dst / NT] : p.m;
            store4(x + (size_t)p.dst * D + col, r[0] + m * h0, r[1] + m * h1, r[2] + m * h2, r[3] + m * h3);
        }
    }
};

// MAPPED: gp is indexed by TOKEN row (dense "masked" forward) while this GEMM runs on compact rows.  A separate
// instantiation: the extra index load in front of every gelu' load costs the unmapped kernel 37 % (142 -> 195 us at B=128)
template <class AT, bool MAPPED>
struct EpiGeluBwd {
    const AT* gp; AT* out; int ld;   // gp = gelu'(z) saved by the fc1 epilogue
    const int* row_map;
    bf16* out3; float s3;   // split fp32 form: dZ * s3 goes out as the split operand of the fc1 dgrad GEMM instead of as fp32
    bool hi_only;           // ... its hi half alone (that GEMM contracts one part)
    typedef NoCtx Col; typedef Raw4<AT> Pre;
    __device__ __forceinline__ Col col_init(int) const { return {}; }
    __device__ __forceinline__ Pre pre(int row, int col) const {   // gelu'(z) is read exactly once: streaming load
        const size_t src = (size_t)(MAPPED ? row_map[row] : row) * ld + col;
        if constexpr (sizeof(AT) == 2) {
            Pre p;
            p.v = DYT_NT_LOAD(reinterpret_cast<const bf16x4*>(gp + src));
            return p;
        } else {
            return load_raw4(gp + src);
        }
    }
    __device__ __forceinline__ void apply(int row, int col, const float (&a)[4], const Col&, const Pre& p) const {
        float g[4];
        p.get(g);
        if constexpr (sizeof(AT) == 4) {
            if (out3) { store4_split3(out3 + (size_t)row * SPLIT_A * ld + col, ld, a[0] * g[0] * s3, a[1] * g[1] * s3, a[2] * g[2] * s3, a[3] * g[3] * s3, hi_only); return; }
        }
        store4(out + (size_t)row * ld + col, a[0] * g[0], a[1] * g[1], a[2] * g[2], a[3] * g[3]);
    }
};

struct EpiStoreF32 {
    float* out; int ld; int accumulate; float alpha;   // out (+)= alpha * acc
    const float* dscale = nullptr;                     // device word alpha is multiplied by (GemmArgs::out_dscale)
    typedef NoCtx Col; typedef Raw4<float> Pre;
    __device__ __forceinline__ Col col_init(int) const { return {}; }
    __device__ __forceinline__ Pre pre(int row, int col) const {
        if (accumulate) return load_raw4(out + (size_t)row * ld + col);
        return {make_float4(0.f, 0.f, 0.f, 0.f)};
    }
    __device__ __forceinline__ void apply(int row, int col, const float (&a)[4], const Col&, const Pre& p) const {
        float r[4];
        p.get(r);
        const float al = dscale ? alpha * *dscale : alpha;
        store4(out + (size_t)row * ld + col, r[0] + al * a[0], r[1] + al * a[1], r[2] + al * a[2], r[3] + al * a[3]);
    }
};

template <class AT>
struct EpiStoreAT {
    AT* out; int ld;
    const float* dscale = nullptr;   // device word the result is multiplied by (GemmArgs::out_dscale)
    typedef NoCtx Col; typedef NoCtx Pre;
    __device__ __forceinline__ Col col_init(int) const { return {}; }
    __device__ __forceinline__ Pre pre(int, int) const { return {}; }
    __device__ __forceinline__ void apply(int row, int col, const float (&a)[4], const Col&, const Pre&) const {
        if (dscale) {   // (uniform branch)
            const float f = *dscale;
            store4(out + (size_t)row * ld + col, a[0] * f, a[1] * f, a[2] * f, a[3] * f);
            return;
        }
        store4(out + (size_t)row * ld + col, a[0], a[1], a[2], a[3]);
    }
};

template <class AT>
struct EpiBiasAT {
    const float* bias; AT* out; int ld;
    typedef Bias4 Col; typedef NoCtx Pre;
    __device__ __forceinline__ Col col_init(int col) const { return load_bias4(bias, col); }
    __device__ __forceinline__ Pre pre(int, int) const { return {}; }
    __device__ __forceinline__ void apply(int row, int col, const float (&a)[4], const Col& c, const Pre&) const {
        store4(out + (size_t)row * ld + col, a[0] + c.b[0], a[1] + c.b[1], a[2] + c.b[2], a[3] + c.b[3]);
    }
};

template <class AT, class ST = AT>   // ST: type of the second copy (GemmArgs::save16: the 16-bit d_act the 16-bit backward reads)
struct EpiAdDown {
    const float* bias;  // padded to RP
    AT* out;            // [M, RP]
    const uint8_t* keep; int r; float inv_keep; float drop_p; uint64_t seed, subseq;
    const int* row_map;  // token row of compact row `row` (mask / RNG are indexed by token), or null
    const uint64_t* seed_dev;   // overrides `seed` when set (captured graphs draw fresh noise per replay)
    ST* out_s; float s_out;     // optional second copy s_out * result: the A2 operand of the fc2 + up-projection contraction (the adapter
                                // scale goes on the O(1) activations, not on the possibly tiny up-projection weights: fp16 subnormals)
    bf16* out3 = nullptr; float s3 = 1.f;   // split fp32 forms: s3 * result as a [rows][hi 64 | lo 64] image -- the up-projection's three-part operand
    typedef Bias4 Col;
    struct Pre { int trow; };
    __device__ __forceinline__ Col col_init(int col) const { return load_bias4(bias, col); }
    __device__ __forceinline__ Pre pre(int row, int) const { return {row_map ? row_map[row] : row}; }
    __device__ __forceinline__ void apply(int row, int col, const float (&a)[4], const Col& c, const Pre& p) const {
        const int trow = p.trow;
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = fmaxf(a[i] + c.b[i], 0.0f);
        if (drop_p > 0.f) {
            if (keep) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    v[i] = (col + i < r && keep[(size_t)trow * r + col + i]) ? v[i] * inv_keep : 0.0f;
            } else {
                Philox ph(seed_dev ? *seed_dev : seed, subseq, (uint64_t)trow * (RP / 4) + (col >> 2));
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = ph.u01(i) >= drop_p ? v[i] * inv_keep : 0.0f;
            }
        }
        store4(out + (size_t)row * RP + col, v[0], v[1], v[2], v[3]);
        if (out_s) store4(out_s + (size_t)row * RP + col, v[0] * s_out, v[1] * s_out, v[2] * s_out, v[3] * s_out);
        if constexpr (sizeof(AT) == 4) {
            if (out3) store4_split3(out3 + (size_t)row * (SPLIT_A * RP) + col, RP, v[0] * s3, v[1] * s3, v[2] * s3, v[3] * s3);
        }
    }
};

template <bool MAPPED>   // MAPPED: rows go through row_map (cls-only tail of the last block); see EpiFc2 for why two forms
struct EpiAdUp {
    const float* bias; const float* u; float* out; float scale; const int* row_map;
    const float* skip_mask;   // rows with skip_mask[row] != 0 are left alone (kept tokens: their fc2 launch adds the adapter itself)
    const float* rs = nullptr;   // MAPPED (cls-row proj of a complete_model pass's last block): stochastic-depth scale of image dst / 197
    float bscale = -1.f;         // >= 0: out = u + scale * acc + bscale * bias (GemmArgs::bias_scale: the A operand already carries the adapter scale)
    typedef Bias4 Col;
    struct PreG { int dst; Raw4<float> r; };
    typedef typename std::conditional<MAPPED, PreG, Raw4<float>>::type Pre;
    __device__ __forceinline__ Col col_init(int col) const { return load_bias4(bias, col); }
    __device__ __forceinline__ Pre pre(int row, int col) const {
        if constexpr (MAPPED) {
            Pre p;
            p.dst = row_map[row];
            p.r = load_raw4(u + (size_t)p.dst * D + col);
            return p;
        } else {
            if (skip_mask && skip_mask[row] != 0.f) return {make_float4(0.f, 0.f, 0.f, 0.f)};
            return load_raw4(u + (size_t)row * D + col);
        }
    }
    __device__ __forceinline__ void apply(int row, int col, const float (&a)[4], const Col& c, const Pre& p) const {
        float r[4];
        size_t dst = row;
        if constexpr (MAPPED) { p.r.get(r); dst = p.dst; } else { if (skip_mask && skip_mask[row] != 0.f) return; p.get(r); }
        float sc = scale;
        if constexpr (MAPPED) { if (rs) sc *= rs[dst / NT]; }
        if (bscale >= 0.f) {   // (uniform branch)
            store4(out + dst * D + col, r[0] + fmaf(bscale, c.b[0], sc * a[0]), r[1] + fmaf(bscale, c.b[1], sc * a[1]),
                   r[2] + fmaf(bscale, c.b[2], sc * a[2]), r[3] + fmaf(bscale, c.b[3], sc * a[3]));
            return;
        }
        store4(out + dst * D + col, r[0] + sc * (a[0] + c.b[0]), r[1] + sc * (a[1] + c.b[1]),
               r[2] + sc * (a[2] + c.b[2]), r[3] + sc * (a[3] + c.b[3]));
    }
};

template <class AT>
struct EpiAdDgradUp {
    const AT* dact; AT* out; float scale; float inv_keep;
    typedef NoCtx Col; typedef Raw4<AT> Pre;
    __device__ __forceinline__ Col col_init(int) const { return {}; }
    __device__ __forceinline__ Pre pre(int row, int col) const { return load_raw4(dact + (size_t)row * RP + col); }
    __device__ __forceinline__ void apply(int row, int col, const float (&a)[4], const Col&, const Pre& p) const {
        float d[4];
        p.get(d);
        const float s = scale * inv_keep;
        store4(out + (size_t)row * RP + col, d[0] != 0.f ? a[0] * s : 0.f, d[1] != 0.f ? a[1] * s : 0.f,
               d[2] != 0.f ? a[2] * s : 0.f, d[3] != 0.f ? a[3] * s : 0.f);
    }
};

struct EpiEmbed {
    const float* bias; const float* pos; float* x0;
    typedef Bias4 Col; typedef Raw4<float> Pre;
    __device__ __forceinline__ Col col_init(int col) const { return load_bias4(bias, col); }
    __device__ __forceinline__ Pre pre(int row, int col) const {
        const int p = row % NP;
        return load_raw4(pos + (size_t)(1 + p) * D + col);
    }
    __device__ __forceinline__ void apply(int row, int col, const float (&a)[4], const Col& c, const Pre& pr) const {
        const int b = row / NP, p = row - b * NP;
        const size_t o = ((size_t)b * NT + 1 + p) * D + col;
        float ps[4];
        pr.get(ps);
        store4(x0 + o, a[0] + c.b[0] + ps[0], a[1] + c.b[1] + ps[1], a[2] + c.b[2] + ps[2], a[3] + c.b[3] + ps[3]);
    }
};
}  // namespace dyt
