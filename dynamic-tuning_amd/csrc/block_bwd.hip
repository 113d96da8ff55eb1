// Per-block row kernels of the backward pass (gfx950): bwd_prep, the per-token tail tok_bwd, and stochastic depth -- with
// ln_bwd (ln.hip) what tests/test_gpu_row_bwd.py covers.  One 64-lane wave owns one 768-channel token row.
#include "kernels.h"
#include "rowhelp.h"

namespace dyt {

// A/B switches of the probes (tools/probes/README.md): which of the full drains of tok_bwd are compiled in
#if defined(DYT_NOPIN_TOK) || defined(DYT_NOPIN_ROWS)
#define TK_ROWPIN(x)
#else
#define TK_ROWPIN(x) (x).landed()
#endif
#if defined(DYT_NOPIN_TOK) || defined(DYT_NOPIN_SCALARS)
#define TK_SCALPIN3(a, b, c)
#define TK_SCALPIN4(a, b, c, d)
#else
#define TK_SCALPIN3(a, b, c) DYT_PIN3(a, b, c)
#define TK_SCALPIN4(a, b, c, d) DYT_PIN4(a, b, c, d)
#endif

// ------------------------------------------------------------------------------------------
// backward prep of a block: AT copy of g, gathered MLP gradient rows, <g, h> per token
// ------------------------------------------------------------------------------------------
template <class AT>
__global__ __launch_bounds__(256) void bwd_prep_kernel(const float* __restrict__ g, const AT* __restrict__ h,
                                                       const int* __restrict__ dst_of, const float* __restrict__ row_mask,
                                                       AT* __restrict__ g_at, AT* __restrict__ dH,
                                                       float* __restrict__ dmask, int M, float gs) {
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= M) return;
    Row12 gr;
    gr.load(g + (size_t)t * D, lane);
    int r = dst_of ? dst_of[t] : t;
    float mk = row_mask ? row_mask[t] : 1.0f;
    gr.landed(); DYT_PIN2(r, mk);
    if (g_at) {
        Row12 gsc;
#pragma unroll
        for (int i = 0; i < 12; ++i) gsc.v[i] = gr.v[i] * gs;
        gsc.store(g_at + (size_t)t * D, lane);
    }
    float dm = 0.f;
    if (r >= 0) {
        if (h) {
            Row12 hr;
            hr.load_at(h + (size_t)r * D, lane);
            hr.landed();
            dm = dot12(gr, hr);
        }
        if (dH) {
            if (row_mask) {
#pragma unroll
                for (int i = 0; i < 12; ++i) gr.v[i] *= mk;
            }
#pragma unroll
            for (int i = 0; i < 12; ++i) gr.v[i] *= gs;
            gr.store(dH + (size_t)r * D, lane);
        }
    }
    if (dmask && lane == 0) dmask[t] = dm;
}
int launch_bwd_prep(int precision, const BwdPrepArgs& a, hipStream_t s) {
    const int grid = (a.M + 3) / 4;
    if (precision == 0)
        hipLaunchKernelGGL(bwd_prep_kernel<float>, dim3(grid), dim3(256), 0, s, a.g, (const float*)a.h, a.dst_of, a.row_mask,
                           (float*)a.g_at, (float*)a.dH, a.dmask, a.M, 1.0f);
    else
        hipLaunchKernelGGL(bwd_prep_kernel<bf16>, dim3(grid), dim3(256), 0, s, a.g, (const bf16*)a.h, a.dst_of, a.row_mask,
                           (bf16*)a.g_at, (bf16*)a.dH, a.dmask, a.M, a.gs);
    LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------
// per-token tail of a block's backward
// ------------------------------------------------------------------------------------------
constexpr int TOK_PER_BLOCK = 32;

template <class AT>
__global__ __launch_bounds__(256) void tok_bwd_kernel(TokBwdArgs a) {
    __shared__ float red[4][D + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    Row12 wg, ln2w, dwg;
    float dbg = 0.f;
#pragma unroll
    for (int i = 0; i < 12; ++i) dwg.v[i] = 0.f;
    if (a.gate_w) { wg.load(a.gate_w, lane); TK_ROWPIN(wg); }
    if (a.dA2) { ln2w.load(a.ln2_w, lane); TK_ROWPIN(ln2w); }
    const int t0 = blockIdx.x * TOK_PER_BLOCK;
    // compact rows of this wave's tokens, one per lane, loaded up front: the dA2 row of a token then goes out WITH its other rows instead of
    // behind the drain that delivers its index (round 6: one memory latency per token instead of two)
    int rv = -1;
    if (a.dA2 && a.write_du) {
        const int tt = t0 + wave + 4 * lane;
        if (lane < TOK_PER_BLOCK / 4 && tt < a.M) {
            if (a.g_cls) { const int bb = tt / NT; rv = (tt - bb * NT == 0) ? bb : -1; }
            else rv = a.dst_of ? a.dst_of[tt] : tt;
        }
    }
    for (int k = wave; k < TOK_PER_BLOCK; k += 4) {
        const int t = t0 + k;
        if (t >= a.M) break;
        const int b = t / NT, n = t - b * NT;
        // all loads of the token first, then ONE full drain that names every one of them (DYT_PIN*, dyt_common.h): the previous
        // iteration's stores, the row loads (misses) and the per-token scalars share the counter
        Row12 du, ur, e, dy;
        const bool need_u = (a.dA2 && (!a.g_cls || n == 0)) || a.gate_w;   // cls-only tail without a gate: only the cls rows have an LN2 backward
        const bool gate = a.gate_w && n >= 1;
        const bool cat = gate && a.cat_dact && a.dmask;      // the saved MLP output includes the adapter's weight term (see TokBwdArgs)
        if (need_u) ur.load_nt(a.u + (size_t)t * D, lane);   // saved u of the forward pass: last use
        const bool du16 = a.du_in_at && a.write_du && !a.g_cls;   // the incoming gradient as the 16-bit gs-scaled copy (TokBwdArgs::du_in_at)
        if (du16) du.load_at(reinterpret_cast<const AT*>(a.du_in_at) + (size_t)t * D, lane);
        else if (a.write_du && !a.g_cls) du.load(a.du + (size_t)t * D, lane);
        else if (a.write_du && n == 0) du.load(a.g_cls + (size_t)b * D, lane);
        else {
#pragma unroll
            for (int i = 0; i < 12; ++i) du.v[i] = 0.f;
        }
        if (a.dad) e.load_at(reinterpret_cast<const AT*>(a.dad) + (size_t)t * D, lane);
        const int r = __builtin_amdgcn_readlane(rv, k >> 2);   // (k >> 2 is wave-uniform: k = wave + 4 j)
        if (r >= 0) dy.load_at(reinterpret_cast<const AT*>(a.dA2) + (size_t)r * D, lane);
        float2 st2 = make_float2(0.f, 1.f);
        if (a.dA2 && a.write_du) st2 = a.stats2[t];
        float ext = 0.f, sf = 0.f, dmk = 0.f, dlg = 0.f;
        float cd = 0.f, cz = 0.f;   // this lane's column of the token's d_act / ddz rows (saved h includes the adapter, see TokBwdArgs)
        if (gate) {
            const size_t oi = (size_t)b * a.out_stride + n - 1;
            if (a.dtoken_select) ext = a.dtoken_select[oi];
            else if (a.dtok) ext = a.dtok[0] + (a.maskf[t] != 0.f ? a.dtok[2] : a.dtok[1]);
            sf = a.soft[t];
            if (a.dmask) dmk = a.dmask[t];
            if (a.dtoken_logits) dlg = a.dtoken_logits[oi];
            if (cat) {
                cd = to_f32(reinterpret_cast<const AT*>(a.cat_dact)[(size_t)t * RP + lane]);
                cz = to_f32(reinterpret_cast<const AT*>(a.cat_ddz)[(size_t)t * RP + lane]);
            }
        }
        if (need_u) TK_ROWPIN(ur);
        TK_ROWPIN(du);
        if (a.dad) TK_ROWPIN(e);
        if (r >= 0) TK_ROWPIN(dy);
        TK_SCALPIN3(st2.x, st2.y, ext);
        TK_SCALPIN3(sf, dmk, dlg);
        if (cat) {
            DYT_PIN2(cd, cz);
            const float czs = a.cat_ddz_dscale ? a.cat_ddz_scale * *a.cat_ddz_dscale : a.cat_ddz_scale;
            if (a.maskf[t] != 0.f) dmk -= wave_sum(cd * cz) * czs;   // dropped tokens have dmask = 0 and no saved h
        }
        const float bs = a.branch_scale ? a.branch_scale[b] : 1.0f;   // stochastic depth on the MLP branch (uniform per image)
        dmk *= bs;
        if (du16) {
#pragma unroll
            for (int i = 0; i < 12; ++i) du.v[i] *= a.inv_gs;
        }
        if (a.dad) {
#pragma unroll
            for (int i = 0; i < 12; ++i) du.v[i] += e.v[i] * a.inv_gs;
        }
        if (a.dA2 && a.write_du) {
            if (r >= 0) {
                ln_bwd_row(dy, ur, ln2w, st2);
                const float ds = a.inv_gs * bs;
#pragma unroll
                for (int i = 0; i < 12; ++i) du.v[i] += dy.v[i] * ds;
            }
        }
        if (gate) {
            float dlogit = (dmk + ext) * sf * (1.0f - sf);
            if (a.training) dlogit /= a.tau;
            dlogit += dlg;
#pragma unroll
            for (int i = 0; i < 12; ++i) {
                du.v[i] = fmaf(dlogit, wg.v[i], du.v[i]);
                dwg.v[i] = fmaf(dlogit, ur.v[i], dwg.v[i]);
            }
            dbg += dlogit;
        }
        if (a.write_du) {
            if (a.du) du.store(a.du + (size_t)t * D, lane);
            if (a.du3) du.store_split3(reinterpret_cast<bf16*>(a.du3) + (size_t)t * SPLIT_A * D, lane, a.du3_scale, a.du3_hi_only);   // proj dgrad operand (fp32 split form)
            if (a.du_at) {
                Row12 dsc;
#pragma unroll
                for (int i = 0; i < 12; ++i) dsc.v[i] = du.v[i] * a.gs;
                dsc.store(reinterpret_cast<AT*>(a.du_at) + (size_t)t * D, lane);
            }
        }
    }
    if (a.gate_w) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) red[wave][i * 256 + lane * 4 + e] = dwg.v[4 * i + e];
        if (lane == 0) red[wave][D] = dbg;  // dbg is lane-uniform
        __syncthreads();
        for (int c = tid; c < D + 1; c += 256)
            a.partial[(size_t)blockIdx.x * (D + 1) + c] = red[0][c] + red[1][c] + red[2][c] + red[3][c];
    }
}
int launch_tok_bwd(int precision, const TokBwdArgs& a, int* nblocks_out, hipStream_t s) {
    const int grid = (a.M + TOK_PER_BLOCK - 1) / TOK_PER_BLOCK;
    if (nblocks_out) *nblocks_out = grid;
    if (dbg_skip(8)) return 0;
    if (precision == 0) hipLaunchKernelGGL(tok_bwd_kernel<float>, dim3(grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(tok_bwd_kernel<bf16>, dim3(grid), dim3(256), 0, s, a);
    LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------
// stochastic depth (timm DropPath; reference models/vision_transformer_IN21K.py:121,131,148,159 with dpr = linspace(0, rate, depth), :285)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void drop_path_draw_kernel(float* __restrict__ scales, int depth, int batch, float rate, uint64_t seed,
                                                             const uint64_t* __restrict__ seed_dev, uint64_t subseq_base) {
    const int i = blockIdx.x * 256 + threadIdx.x;   // (branch, l, b)
    if (i >= 2 * depth * batch) return;
    const int b = i % batch, l = (i / batch) % depth, branch = i / (batch * depth);
    const float drop = depth > 1 ? rate * (float)l / (float)(depth - 1) : 0.f;
    float v = 1.0f;
    if (drop > 0.f) {
        const float keep = 1.0f - drop;
        Philox ph(seed_dev ? *seed_dev : seed, subseq_base + (uint64_t)(2 * l + branch), (uint64_t)b);
        v = ph.u01(0) < keep ? 1.0f / keep : 0.0f;
    }
    scales[i] = v;
}
int launch_drop_path_draw(float* scales, int depth, int batch, float rate, uint64_t seed, const uint64_t* seed_dev, uint64_t subseq_base, hipStream_t s) {
    hipLaunchKernelGGL(drop_path_draw_kernel, dim3((2 * depth * batch + 255) / 256), dim3(256), 0, s, scales, depth, batch, rate, seed, seed_dev, subseq_base);
    LAUNCH_CHECK();
    return 0;
}
template <class AT>
__global__ __launch_bounds__(256) void scale_rows_kernel(AT* __restrict__ x, const float* __restrict__ scale, int M, int ld) {
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;   // 4 consecutive elements of a row (ld % 4 == 0)
    if (i >= (size_t)M * ld) return;
    const float sc = scale[(int)(i / ld) / NT];
    float v[4];
    load4(x + i, v);
    store4(x + i, v[0] * sc, v[1] * sc, v[2] * sc, v[3] * sc);
}
int launch_scale_rows(int precision, void* x, const float* scale, int M, int ld, hipStream_t s) {
    const unsigned grid = (unsigned)(((size_t)M * ld / 4 + 255) / 256);
    if (precision == 0) hipLaunchKernelGGL(scale_rows_kernel<float>, dim3(grid), dim3(256), 0, s, (float*)x, scale, M, ld);
    else hipLaunchKernelGGL(scale_rows_kernel<bf16>, dim3(grid), dim3(256), 0, s, (bf16*)x, scale, M, ld);
    LAUNCH_CHECK();
    return 0;
}

}  // namespace dyt
