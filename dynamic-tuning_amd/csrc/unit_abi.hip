// Unit-test ABI: single-kernel and sub-module entry points.  They allocate scratch and synchronise.
#include "ctx.h"
#include "image_items.h"

namespace dyt {

template <class AT>
__global__ void qkv_split_kernel(const float* __restrict__ qkv, AT* __restrict__ q, AT* __restrict__ k, AT* __restrict__ v,
                                 int batch) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)batch * NT * 3 * D) return;
    const int col = (int)(idx % (3 * D));
    const size_t row = idx / (3 * D);
    const int b = (int)(row / NT), n = (int)(row % NT);
    const int which = col / D, c = col % D, h = c >> 6, d = c & 63;
    const float val = qkv[idx] * (which == 0 ? 0.125f : 1.0f);
    AT* dst = which == 0 ? q : (which == 1 ? k : v);
    dst[(((size_t)b * NH + h) * NT + n) * HD + d] = from_f32<AT>(val);
}
template <class AT>
__global__ void to_f32_kernel(const AT* __restrict__ src, float* __restrict__ dst, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = to_f32(src[i]);
}

}  // namespace dyt

// Saved adapter bottleneck relu(down(u)) (times the dropout scale) of one block of a saved pass, as fp32 [rows, 64]; *rows_out = B*197,
// or B for the last block in the cls-only tail form.  Test accessor (tests/parity_rules.py checks which side of the ReLU a unit is on).
extern "C" int dyt_debug_dact(dyt_ctx* c, int slot, int layer, float* out, int* rows_out, void* stream) {
    if (!c || !out || slot < 0 || slot >= c->cfg.slots || layer < 0 || layer >= c->cfg.depth) { set_error("bad slot / layer"); return DYT_ERR_ARG; }
    { int rc = refuse_inference(c, "dyt_debug_dact (per-block tensors of a saved pass)"); if (rc) return rc; }
    const Slot& S = c->slots[slot];
    if (S.batch < 1) { set_error("slot %d holds no pass", slot); return DYT_ERR_STATE; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool tail = c->cls_tail && layer == c->cfg.depth - 1;
    const size_t rows = tail ? (size_t)S.batch : (size_t)S.batch * NT, n = rows * RP;
    const LayerS& L = S.L[layer];
    if (rows_out) *rows_out = (int)rows;
    if (S.saved16 && L.dact16) hipLaunchKernelGGL(to_f32_kernel<bf16>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const bf16*)L.dact16, out, n);
    else if (c->prec == DYT_PREC_FP32) DYT_HIP_CHECK(hipMemcpyAsync(out, L.d_act, n * 4, hipMemcpyDeviceToDevice, s));
    else hipLaunchKernelGGL(to_f32_kernel<bf16>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const bf16*)L.d_act, out, n);
    DYT_HIP_CHECK(hipGetLastError());
    return DYT_OK;
}

// ------------------------------------------------------------------------------------------
// single-kernel entry points (unit tests).  These allocate scratch and synchronise: test-only.
// ------------------------------------------------------------------------------------------
extern "C" int dyt_gemm_bf16_raw(const void* a, const void* w, void* cmat, int M, int N, int K, int variant, void* stream) {
    if (!a || !w || !cmat) { set_error("null argument"); return DYT_ERR_ARG; }
    return launch_gemm_raw(a, w, cmat, M, N, K, variant, static_cast<hipStream_t>(stream));
}

// adapter weight-gradient kernel alone (unit tests / probes): out_w[c*r + j] += sum_m X[m][c] Y[m][j], out_xsum[c] += sum_m X[m][c],
// out_ysum[j] += sum_m Y[m][j]; X [M,768], Y [M,64] in the precision's operand type; partial = scratch of dyt_wgrad_scratch_floats(M)
extern "C" int64_t dyt_wgrad_scratch_floats(int M) { return (int64_t)((M + 511) / 512) * (D + 8) * 80; }
extern "C" int dyt_wgrad_raw(const void* X, const void* Y, int M, int r, int precision, float* partial, float* out_w, float* out_xsum,
                             float* out_ysum, void* stream) {
    if (!X || !Y || !partial || !out_w || M < 1 || r < 1 || r > RP) { set_error("bad argument"); return DYT_ERR_ARG; }
    WgradArgs a; a.X = X; a.Y = Y; a.M = M; a.r = r; a.partial = partial;
    a.out_w = out_w; a.sc = r; a.sj = 1; a.alpha = 1.0f; a.out_xsum = out_xsum; a.alpha_x = 1.0f; a.out_ysum = out_ysum; a.alpha_y = 1.0f;
    return launch_wgrad(precision, a, static_cast<hipStream_t>(stream));
}

extern "C" int dyt_gemm_f32_raw(const float* a, const float* w, float* cmat, int M, int N, int K, int variant, void* stream) {
    if (!a || !w || !cmat) { set_error("null argument"); return DYT_ERR_ARG; }
    return launch_gemm_f32_raw(a, w, cmat, M, N, K, variant, static_cast<hipStream_t>(stream));
}

extern "C" int dyt_debug_counters(uint64_t* out4, int reset) {
    if (!out4) { set_error("null argument"); return DYT_ERR_ARG; }
    return gemm_debug_counters(reinterpret_cast<unsigned long long*>(out4), reset);
}

extern "C" int dyt_layernorm(const float* x, const float* w, const float* b, float* out, int rows, void* stream) {
    if (!x || !w || !b || !out || rows < 1) { set_error("bad argument"); return DYT_ERR_ARG; }
    return launch_ln_fwd_f32out(x, w, b, out, rows, static_cast<hipStream_t>(stream));
}

struct Scratch {
    std::vector<void*> ptrs;
    ~Scratch() { for (void* p : ptrs) hipFree(p); }
    void* get(size_t bytes) {
        void* p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
        ptrs.push_back(p);
        return p;
    }
};

extern "C" int dyt_linear(const float* a, const float* w, const float* bias, float* cmat, int M, int N, int K, int precision,
                          void* stream) {
    if (!a || !w || !cmat || M < 1) { set_error("bad argument"); return DYT_ERR_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    GemmArgs g; g.M = M; g.N = N; g.K = K; g.bias = bias; g.out_f32 = cmat;
    Scratch sc;
    if (precision == 0) { g.A = a; g.W = w; }
    else {
        void* a2 = sc.get((size_t)M * K * 2); void* w2 = sc.get((size_t)N * K * 2);
        if (!a2 || !w2) { set_error("scratch alloc failed"); return DYT_ERR_HIP; }
        int rc = launch_convert(1, a, a2, (int64_t)M * K, s); if (rc) return rc;
        rc = launch_convert(1, w, w2, (int64_t)N * K, s); if (rc) return rc;
        g.A = a2; g.W = w2;
    }
    int rc = launch_gemm(precision, EPI_BIAS_F32, g, s);
    if (rc) return rc;
    DYT_HIP_CHECK(hipStreamSynchronize(s));
    return DYT_OK;
}

// One nn.Linear through the split forms of the fp32 mode (unit tests / probes): form 3 = three IEEE-half products, 8 = hi * hi in f16 +
// fp8 correction products.  a [M,K], w [N,K], bias [N] or NULL, cmat [M,N] fp32.  Allocates scratch and synchronises: test-only.
extern "C" int dyt_linear_split(const float* a, const float* w, const float* bias, float* cmat, int M, int N, int K, int form, void* stream) {
    if (!a || !w || !cmat || M < 1 || (form != 3 && form != 8)) { set_error("bad argument"); return DYT_ERR_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scratch sc;
    void* a3 = sc.get((size_t)((M + 255) / 256 * 256) * SPLIT_A * K * 2); void* w3 = sc.get((size_t)N * SPLIT_A * K * 2);
    int* ew = (int*)sc.get(16); unsigned* scr = (unsigned*)sc.get(16);
    if (!a3 || !w3 || !ew || !scr) { set_error("scratch alloc failed"); return DYT_ERR_HIP; }
    int rc = form == 8 ? launch_split_w_f8(w, w3, N, K, ew, scr, s) : launch_split3_w(w, w3, N, K, s);
    if (rc) return rc;
    GemmArgs g; g.A = a; g.W = w; g.M = M; g.N = N; g.K = K; g.bias = bias; g.out_f32 = cmat; g.W3 = w3; g.a3 = a3;
    if (form == 8) { g.f8 = true; g.w_exp = ew; }
    rc = launch_gemm(0, EPI_BIAS_F32, g, s);
    if (rc) return rc;
    DYT_HIP_CHECK(hipStreamSynchronize(s));
    return DYT_OK;
}

template <class AT>
static int attention_test(const float* qkv, float* out, const float* dout, float* dqkv, int B, int P, hipStream_t s) {
    Scratch sc;
    const size_t M = (size_t)B * NT;
    AT* q = (AT*)sc.get(M * D * sizeof(AT)); AT* k = (AT*)sc.get(M * D * sizeof(AT)); AT* v = (AT*)sc.get(M * D * sizeof(AT));
    AT* o = (AT*)sc.get(M * D * sizeof(AT));
    float* lse = (float*)sc.get((size_t)B * NH * NT * 4);
    if (!q || !k || !v || !o || !lse) { set_error("scratch alloc failed"); return DYT_ERR_HIP; }
    const size_t n3 = M * 3 * D;
    hipLaunchKernelGGL(qkv_split_kernel<AT>, dim3((unsigned)((n3 + 255) / 256)), dim3(256), 0, s, qkv, q, k, v, B);
    AttnFwdArgs f; f.batch = B; f.q = q; f.k = k; f.v = v; f.out = o; f.lse = lse;
    int rc = launch_attn_fwd(P, f, s);
    if (rc) return rc;
    hipLaunchKernelGGL(to_f32_kernel<AT>, dim3((unsigned)((M * D + 255) / 256)), dim3(256), 0, s, (const AT*)o, out, M * D);
    if (dout && dqkv) {
        AT* d_o = (AT*)sc.get(M * D * sizeof(AT)); AT* dq = (AT*)sc.get(n3 * sizeof(AT));
        float* delta = (float*)sc.get((size_t)B * NH * NT * 4);
        if (!d_o || !dq || !delta) { set_error("scratch alloc failed"); return DYT_ERR_HIP; }
        rc = launch_convert(P, dout, d_o, (int64_t)(M * D), s); if (rc) return rc;
        AttnBwdArgs b; b.batch = B; b.q = q; b.k = k; b.v = v; b.out = o; b.dout = d_o; b.lse = lse; b.delta = delta; b.dqkv = dq;
        rc = launch_attn_bwd(P, b, s); if (rc) return rc;
        hipLaunchKernelGGL(to_f32_kernel<AT>, dim3((unsigned)((n3 + 255) / 256)), dim3(256), 0, s, (const AT*)dq, dqkv, n3);
    }
    DYT_HIP_CHECK(hipGetLastError());
    DYT_HIP_CHECK(hipStreamSynchronize(s));
    return DYT_OK;
}

extern "C" int dyt_attention(const float* qkv, float* out, const float* dout, float* dqkv, int batch, int precision,
                             void* stream) {
    if (!qkv || !out || batch < 1) { set_error("bad argument"); return DYT_ERR_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    return precision == 0 ? attention_test<float>(qkv, out, dout, dqkv, batch, 0, s)
                          : attention_test<bf16>(qkv, out, dout, dqkv, batch, 1, s);
}

// ---- sub-module unit entries: the adapter and the gathered MLP alone, through the product's own kernels ----
namespace dyt {
// per image: kept-token list (ascending) and count from a {0,1} mask -- what gate_select_kernel leaves behind
__global__ __launch_bounds__(256) void mask_to_keep_kernel(const float* __restrict__ maskf, int* __restrict__ keep_local,
                                                           int* __restrict__ counts) {
    __shared__ int wave_cnt[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool keep = tid < NT && maskf[(size_t)b * NT + tid] != 0.f;
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) wave_cnt[wave] = __popcll(bal);
    __syncthreads();
    int off = 0;
    for (int w = 0; w < wave; ++w) off += wave_cnt[w];
    if (keep) keep_local[(size_t)b * NT + off + __popcll(bal & ((1ull << lane) - 1ull))] = tid;
    if (tid == 0) counts[b] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}
// dyt_adapter_bwd's lifts: *out = max |x| over n floats (as the bit pattern of a non-negative float, which orders like the value;
// *out zeroed by the caller), and dst = f src
__global__ __launch_bounds__(256) void absmax_kernel(const float* __restrict__ x, int64_t n, unsigned* __restrict__ out) {
    __shared__ float red[256];
    float m = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) m = fmaxf(m, fabsf(x[i]));
    red[threadIdx.x] = m;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicMax(out, __float_as_uint(red[0]));
}
__global__ void scale_copy_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t n, float f) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[i] * f;
}
}  // namespace dyt

struct AdapterOps {   // AT copies of one adapter's weights in the layouts the GEMMs want (see prep_adapters_kernel)
    void *x_at, *down_w, *down_wT, *up_w, *up_wT, *d_act;
    float* down_b;
};
static int adapter_prepare(Scratch& sc, int P, const float* x, const float* down_w, const float* down_b, const float* up_w, int M, int r,
                           AdapterOps* o, hipStream_t s) {
    const size_t at = at_size(P);
    o->x_at = P == 0 ? (void*)x : sc.get((size_t)M * D * at);
    o->down_w = sc.get((size_t)RP * D * at); o->down_wT = sc.get((size_t)RP * D * at);
    o->up_w = sc.get((size_t)RP * D * at); o->up_wT = sc.get((size_t)RP * D * at);
    o->d_act = sc.get((size_t)M * RP * at);
    o->down_b = (float*)sc.get(RP * sizeof(float));
    if (!o->x_at || !o->down_w || !o->down_wT || !o->up_w || !o->up_wT || !o->d_act || !o->down_b) { set_error("scratch alloc failed"); return DYT_ERR_HIP; }
    int rc = 0;
    if (P != 0) rc = launch_convert(P, x, o->x_at, (int64_t)M * D, s);
    if (!rc) rc = launch_pad_convert(P, down_w, o->down_w, r, D, RP, D, s);              // [RP,768], rows >= r zero
    if (!rc) rc = launch_transpose_convert(P, down_w, o->down_wT, r, D, D, RP, s);       // [768,RP]
    if (!rc) rc = launch_pad_convert(P, up_w, o->up_w, D, r, D, RP, s);                  // [768,RP], cols >= r zero
    if (!rc) rc = launch_transpose_convert(P, up_w, o->up_wT, D, r, RP, D, s);           // [RP,768]
    if (rc) return rc;
    DYT_HIP_CHECK(hipMemsetAsync(o->down_b, 0, RP * sizeof(float), s));
    DYT_HIP_CHECK(hipMemcpyAsync(o->down_b, down_b, (size_t)r * sizeof(float), hipMemcpyDeviceToDevice, s));
    return 0;
}
static int adapter_down(int P, const AdapterOps& o, int M, int r, float drop_p, const uint8_t* keep, uint64_t seed, hipStream_t s) {
    GemmArgs a; a.A = o.x_at; a.W = o.down_w; a.M = M; a.N = RP; a.K = D; a.bias = o.down_b; a.out_at = o.d_act; a.r = r;
    a.drop_p = drop_p; a.inv_keep = drop_p > 0.f ? 1.0f / (1.0f - drop_p) : 1.0f; a.keep = keep; a.seed = seed; a.subseq = 1;
    return launch_gemm(P, EPI_AD_DOWN, a, s);
}

// Adapter.forward (reference models/dynamic_adapter.py:120-140): out = [residual +] scale * up(dropout_p(relu(down(x))))
extern "C" int dyt_adapter_fwd(const float* x, const float* down_w, const float* down_b, const float* up_w, const float* up_b,
                               const float* residual, float* out, int M, int r, float scale, float drop_p, const uint8_t* keep_mask,
                               uint64_t seed, int precision, void* stream) {
    if (!x || !down_w || !down_b || !up_w || !up_b || !out || M < 1 || r < 1 || r > RP || (precision != 0 && precision != 1)) {
        set_error("bad argument");
        return DYT_ERR_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scratch sc;
    AdapterOps o;
    int rc = adapter_prepare(sc, precision, x, down_w, down_b, up_w, M, r, &o, s);
    if (rc) return rc;
    float* zero = nullptr;
    if (!residual) {
        zero = (float*)sc.get((size_t)M * D * sizeof(float));
        if (!zero) { set_error("scratch alloc failed"); return DYT_ERR_HIP; }
        DYT_HIP_CHECK(hipMemsetAsync(zero, 0, (size_t)M * D * sizeof(float), s));
    }
    rc = adapter_down(precision, o, M, r, drop_p, keep_mask, seed, s);
    if (rc) return rc;
    GemmArgs a; a.A = o.d_act; a.W = o.up_w; a.M = M; a.N = D; a.K = RP; a.bias = up_b; a.resid = residual ? residual : zero;
    a.out_f32 = out; a.scale = scale;
    rc = launch_gemm(precision, EPI_AD_UP, a, s);
    if (rc) return rc;
    DYT_HIP_CHECK(hipStreamSynchronize(s));
    return DYT_OK;
}

// Its backward for an upstream gradient dout [M,768] (the same draws): dx [M,768] (may be NULL) and the four parameter gradients,
// ACCUMULATED into d_down_w [r,768], d_down_b [r], d_up_w [768,r], d_up_b [768].
extern "C" int dyt_adapter_bwd(const float* x, const float* down_w, const float* down_b, const float* up_w, const float* dout, float* dx,
                               float* d_down_w, float* d_down_b, float* d_up_w, float* d_up_b, int M, int r, float scale, float drop_p,
                               const uint8_t* keep_mask, uint64_t seed, int precision, void* stream) {
    if (!x || !down_w || !down_b || !up_w || !dout || !d_down_w || !d_down_b || !d_up_w || !d_up_b || M < 1 || r < 1 || r > RP ||
        (precision != 0 && precision != 1)) {
        set_error("bad argument");
        return DYT_ERR_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int P = precision;
    const size_t at = at_size(P);
    Scratch sc;
    // 16-bit operands: up_w and dout are lifted by powers of two 2^ew, 2^ed (adapter_lift_exp of their absmax) before they are converted --
    // a zero-initialised up_proj and gradient-sized dout sit below IEEE half's normal range -- and ddz carries 2^(ed + ew) out to its consumers
    int ew = 0, ed = 0;
    if (P != 0) {
        unsigned* am = (unsigned*)sc.get(2 * sizeof(unsigned));
        if (!am) { set_error("scratch alloc failed"); return DYT_ERR_HIP; }
        DYT_HIP_CHECK(hipMemsetAsync(am, 0, 2 * sizeof(unsigned), s));
        hipLaunchKernelGGL(absmax_kernel, dim3(64), dim3(256), 0, s, up_w, (int64_t)D * r, am);
        hipLaunchKernelGGL(absmax_kernel, dim3(256), dim3(256), 0, s, dout, (int64_t)M * D, am + 1);
        unsigned h[2];
        DYT_HIP_CHECK(hipMemcpyAsync(h, am, sizeof(h), hipMemcpyDeviceToHost, s));
        DYT_HIP_CHECK(hipStreamSynchronize(s));
        float fa[2];
        memcpy(fa, h, sizeof(fa));
        ew = adapter_lift_exp(fa[0]);
        ed = adapter_lift_exp(fa[1]);
        if (ew > 0) {
            float* uw = (float*)sc.get((size_t)D * r * sizeof(float));
            if (!uw) { set_error("scratch alloc failed"); return DYT_ERR_HIP; }
            hipLaunchKernelGGL(scale_copy_kernel, dim3((D * r + 255) / 256), dim3(256), 0, s, up_w, uw, (int64_t)D * r, ldexpf(1.0f, ew));
            up_w = uw;   // (only its transpose up_wT is read below)
        }
        if (ed > 0) {
            float* dl = (float*)sc.get((size_t)M * D * sizeof(float));
            if (!dl) { set_error("scratch alloc failed"); return DYT_ERR_HIP; }
            hipLaunchKernelGGL(scale_copy_kernel, dim3((unsigned)(((int64_t)M * D + 255) / 256)), dim3(256), 0, s, dout, dl, (int64_t)M * D, ldexpf(1.0f, ed));
            dout = dl;
        }
        DYT_HIP_CHECK(hipGetLastError());
    }
    const float inv_d = ldexpf(1.0f, -ed), inv_dw = ldexpf(1.0f, -(ed + ew));   // 1 at precision 0
    AdapterOps o;
    int rc = adapter_prepare(sc, P, x, down_w, down_b, up_w, M, r, &o, s);
    if (rc) return rc;
    rc = adapter_down(P, o, M, r, drop_p, keep_mask, seed, s);   // recompute the bottleneck activations (relu / dropout pattern)
    if (rc) return rc;
    void* g_at = P == 0 ? (void*)dout : sc.get((size_t)M * D * at);
    void* ddz = sc.get((size_t)M * RP * at);
    float* p1 = (float*)sc.get((size_t)dyt_wgrad_scratch_floats(M) * sizeof(float));
    float* p2 = (float*)sc.get((size_t)dyt_wgrad_scratch_floats(M) * sizeof(float));
    if (!g_at || !ddz || !p1 || !p2) { set_error("scratch alloc failed"); return DYT_ERR_HIP; }
    if (P != 0) { rc = launch_convert(P, dout, g_at, (int64_t)M * D, s); if (rc) return rc; }
    const float inv_keep = drop_p > 0.f ? 1.0f / (1.0f - drop_p) : 1.0f;
    {
        GemmArgs a; a.A = g_at; a.W = o.up_wT; a.M = M; a.N = RP; a.K = D; a.aux_at = o.d_act; a.out_at = ddz; a.scale = scale; a.inv_keep = inv_keep;
        rc = launch_gemm(P, EPI_AD_DGRAD_UP, a, s); if (rc) return rc;
    }
    WgradArgs w[2];
    w[0].X = g_at; w[0].Y = o.d_act; w[0].M = M; w[0].r = r; w[0].partial = p1; w[0].out_w = d_up_w; w[0].sc = r; w[0].sj = 1;
    w[0].alpha = scale * inv_d; w[0].out_xsum = d_up_b; w[0].alpha_x = scale * inv_d;   // X = g_at carries 2^ed
    w[1].X = o.x_at; w[1].Y = ddz; w[1].M = M; w[1].r = r; w[1].partial = p2; w[1].out_w = d_down_w; w[1].sc = 1; w[1].sj = D;
    w[1].alpha = inv_dw; w[1].out_xsum = nullptr; w[1].alpha_x = 0.f; w[1].out_ysum = d_down_b; w[1].alpha_y = inv_dw;   // Y = ddz: 2^(ed + ew)
    rc = launch_wgrad(P, w, 2, s); if (rc) return rc;
    if (dx) {
        GemmArgs a; a.A = ddz; a.W = o.down_wT; a.M = M; a.N = D; a.K = RP; a.out_f32 = dx; a.accumulate = 0; a.scale = inv_dw;
        rc = launch_gemm(P, EPI_STORE_F32, a, s); if (rc) return rc;
    }
    DYT_HIP_CHECK(hipStreamSynchronize(s));
    return DYT_OK;
}

// The wide head alone (head_wide.hip): the launches of forward_impl / backward_impl under DYT_CREATE_WIDE_HEAD, on caller-supplied rows.
extern "C" int dyt_head_wide(const float* cls_x, const float* norm_w, const float* norm_b, const float* head_w, const float* head_b,
                             float* logits, const float* dlogits, float* dx, float* d_head_w, float* d_head_b, int batch, int C, void* stream) {
    if (!cls_x || !norm_w || !norm_b || !head_w || !head_b || !logits || batch < 1 || C < 1 || C > 65536) { set_error("dyt_head_wide: bad argument (batch %d, C %d: 1..65536)", batch, C); return DYT_ERR_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scratch sc;
    float* cls_n = (float*)sc.get((size_t)batch * D * 4);
    float2* stats = (float2*)sc.get((size_t)batch * sizeof(float2));
    float* part = dlogits && dx ? (float*)sc.get(head_wide_scratch_floats(batch, C) * 4) : nullptr;
    if (!cls_n || !stats || (dlogits && dx && !part)) { set_error("scratch alloc failed"); return DYT_ERR_HIP; }
    int rc = launch_head_wide_fwd(cls_x, (size_t)D, norm_w, norm_b, head_w, head_b, cls_n, stats, logits, batch, C, s);
    if (rc) return rc;
    if (dlogits) {
        rc = launch_head_wide_bwd(dlogits, cls_x, (size_t)D, cls_n, stats, norm_w, head_w, dx, d_head_w, d_head_b, batch, C, 1, part, s);
        if (rc) return rc;
    }
    DYT_HIP_CHECK(hipStreamSynchronize(s));
    return DYT_OK;
}

// The pooled head alone (pool_avg.hip + the head kernels): the launches of forward_impl / backward_impl under DYT_CREATE_AVG_POOL /
// DYT_CREATE_FC_NORM (row-kernel or wide head), on caller-supplied tokens.
extern "C" int dyt_pool_head(const float* x_tokens, const float* fc_norm_w, const float* fc_norm_b, const float* head_w, const float* head_b,
                             float* logits, const float* dlogits, float* dx_tokens, float* d_fc_norm_w, float* d_fc_norm_b,
                             float* d_head_w, float* d_head_b, int batch, int C, uint32_t create_flags, void* stream) {
    const bool wide = (create_flags & DYT_CREATE_WIDE_HEAD) != 0, avg = (create_flags & DYT_CREATE_AVG_POOL) != 0;
    if ((create_flags & ~(DYT_CREATE_WIDE_HEAD | DYT_CREATE_AVG_POOL | DYT_CREATE_FC_NORM)) || !(create_flags & DYT_CREATE_FC_NORM)) {
        set_error("dyt_pool_head: create_flags 0x%x (DYT_CREATE_FC_NORM, optionally with DYT_CREATE_AVG_POOL and DYT_CREATE_WIDE_HEAD)", create_flags);
        return DYT_ERR_ARG;
    }
    if (!x_tokens || !fc_norm_w || !fc_norm_b || !head_w || !head_b || !logits || (dlogits && !dx_tokens) || batch < 1 || C < 1 || C > (wide ? 65536 : 1024)) {
        set_error("dyt_pool_head: bad argument (batch %d, C %d: 1..%d)", batch, C, wide ? 65536 : 1024);
        return DYT_ERR_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scratch sc;
    float* cls_n = (float*)sc.get((size_t)batch * D * 4);
    float2* stats = (float2*)sc.get((size_t)batch * sizeof(float2));
    float* pooled = avg ? (float*)sc.get((size_t)batch * D * 4) : nullptr;
    float* dy = dlogits ? (float*)sc.get((size_t)batch * D * 4) : nullptr;
    float* dpooled = dlogits && avg ? (float*)sc.get((size_t)batch * D * 4) : nullptr;
    float* part = dlogits && wide ? (float*)sc.get(head_wide_scratch_floats(batch, C) * 4) : nullptr;
    if (!cls_n || !stats || (avg && !pooled) || (dlogits && !dy) || (dlogits && avg && !dpooled) || (dlogits && wide && !part)) { set_error("scratch alloc failed"); return DYT_ERR_HIP; }
    const float* hx = x_tokens; size_t hx_stride = (size_t)NT * D;
    int rc = 0;
    if (avg) { rc = launch_avg_pool_fwd(x_tokens, pooled, batch, s); if (rc) return rc; hx = pooled; hx_stride = D; }
    rc = wide ? launch_head_wide_fwd(hx, hx_stride, fc_norm_w, fc_norm_b, head_w, head_b, cls_n, stats, logits, batch, C, s)
              : launch_head_fwd(hx, fc_norm_w, fc_norm_b, head_w, head_b, cls_n, stats, logits, batch, C, s, hx_stride);
    if (rc) return rc;
    if (dlogits) {
        float* g = avg ? dpooled : dx_tokens;
        const int compact = avg ? 1 : 0;
        rc = wide ? launch_head_wide_bwd(dlogits, hx, hx_stride, cls_n, stats, fc_norm_w, head_w, g, d_head_w, d_head_b, batch, C, compact, part, s, dy)
                  : launch_head_bwd(dlogits, hx, cls_n, stats, fc_norm_w, head_w, g, d_head_w, d_head_b, batch, C, compact, s, hx_stride, dy);
        if (rc) return rc;
        rc = launch_fc_norm_param_grad(dy, hx, hx_stride, stats, d_fc_norm_w, d_fc_norm_b, batch, s);
        if (rc) return rc;
        if (avg) { rc = launch_avg_pool_bwd(dpooled, dx_tokens, batch, s); if (rc) return rc; }
    }
    DYT_HIP_CHECK(hipStreamSynchronize(s));
    return DYT_OK;
}

// The token-gathered MLP of block `layer` with the context's frozen weights (reference models/model_speed_test.py:297-305):
// x [B*197,768] += scatter(fc2(gelu(fc1(LN2(gather(u, mask)))))) for the tokens whose mask is non-zero; u, x fp32, mask [B*197].
extern "C" int dyt_mlp_gathered_fwd(dyt_ctx* c, int layer, const float* u, const float* mask, float* x, int batch, int32_t* total_out,
                                    void* stream) {
    if (!c || !u || !mask || !x || layer < 0 || layer >= c->cfg.depth || batch < 1 || batch > c->cfg.max_batch) { set_error("bad argument"); return DYT_ERR_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int P = c->prec, M = batch * NT;
    const LayerW& W = c->W[layer];
    Scratch sc;
    int* keep_local = (int*)sc.get((size_t)M * 4); int* counts = (int*)sc.get((size_t)batch * 4); int* total = (int*)sc.get(16);
    int* row_src = (int*)sc.get((size_t)M * 4); int* dst_of = (int*)sc.get((size_t)M * 4);
    float2* st = (float2*)sc.get((size_t)M * sizeof(float2));
    void* xn = sc.get((size_t)M * D * c->at); void* h1 = sc.get((size_t)M * DM * c->at);
    if (!keep_local || !counts || !total || !row_src || !dst_of || !st || !xn || !h1) { set_error("scratch alloc failed"); return DYT_ERR_HIP; }
    hipLaunchKernelGGL(mask_to_keep_kernel, dim3(batch), dim3(256), 0, s, mask, keep_local, counts);
    DYT_HIP_CHECK(hipGetLastError());
    int rc = launch_ln_gather(P, u, W.ln2_w, W.ln2_b, keep_local, counts, total, mask, xn, st, row_src, dst_of, batch, s);
    if (rc) return rc;
    {
        GemmArgs a; a.A = xn; a.W = W.fc1_w; a.Wp = W.fc1_wp; a.M = M; a.N = DM; a.K = D; a.m_dev = total; a.bias = W.fc1_b; a.out_at = h1;
        rc = launch_gemm(P, EPI_FC1, a, s); if (rc) return rc;
    }
    {
        GemmArgs a; a.A = h1; a.W = W.fc2_w; a.M = M; a.N = D; a.K = DM; a.m_dev = total; a.bias = W.fc2_b; a.out_f32 = x; a.row_map = row_src;
        rc = launch_gemm(P, EPI_FC2, a, s); if (rc) return rc;
    }
    if (total_out) DYT_HIP_CHECK(hipMemcpyAsync(total_out, total, 4, hipMemcpyDeviceToDevice, s));
    DYT_HIP_CHECK(hipStreamSynchronize(s));
    return DYT_OK;
}

// Its backward for an upstream gradient dy [B*197,768] (the gradient w.r.t. x of dyt_mlp_gathered_fwd): du [B*197,768] += the gradient that
// reaches u THROUGH the gathered MLP (LN2 backward of fc1^T (gelu'(z) * (fc2^T dy)) for the kept tokens, nothing for the dropped ones;
// the residual path du += dy is the caller's).  Recomputes the forward up to gelu'(z); frozen weights: no weight gradients.
extern "C" int dyt_mlp_gathered_bwd(dyt_ctx* c, int layer, const float* u, const float* mask, const float* dy, float* du, int batch,
                                    void* stream) {
    if (!c || !u || !mask || !dy || !du || layer < 0 || layer >= c->cfg.depth || batch < 1 || batch > c->cfg.max_batch) { set_error("bad argument"); return DYT_ERR_ARG; }
    { int rc = refuse_inference(c, "dyt_mlp_gathered_bwd"); if (rc) return rc; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int P = c->prec, M = batch * NT;
    const float gs = P == 0 ? 1.0f : c->gs;
    const LayerW& W = c->W[layer];
    Scratch sc;
    int* keep_local = (int*)sc.get((size_t)M * 4); int* counts = (int*)sc.get((size_t)batch * 4); int* total = (int*)sc.get(16);
    int* row_src = (int*)sc.get((size_t)M * 4); int* dst_of = (int*)sc.get((size_t)M * 4);
    float2* st = (float2*)sc.get((size_t)M * sizeof(float2));
    void* xn = sc.get((size_t)M * D * c->at); void* h1 = sc.get((size_t)M * DM * c->at); void* gp = sc.get((size_t)M * DM * c->at);
    void* g_at = P == 0 ? nullptr : sc.get((size_t)M * D * c->at);
    void* dZ = sc.get((size_t)M * DM * c->at); void* dA2 = sc.get((size_t)M * D * c->at);
    float* partial = (float*)sc.get((size_t)((M + 31) / 32) * (D + 1) * sizeof(float));
    if (!keep_local || !counts || !total || !row_src || !dst_of || !st || !xn || !h1 || !gp || (P != 0 && !g_at) || !dZ || !dA2 || !partial) {
        set_error("scratch alloc failed");
        return DYT_ERR_HIP;
    }
    hipLaunchKernelGGL(mask_to_keep_kernel, dim3(batch), dim3(256), 0, s, mask, keep_local, counts);
    DYT_HIP_CHECK(hipGetLastError());
    int rc = launch_ln_gather(P, u, W.ln2_w, W.ln2_b, keep_local, counts, total, mask, xn, st, row_src, dst_of, batch, s);
    if (rc) return rc;
    {
        GemmArgs a; a.A = xn; a.W = W.fc1_w; a.Wp = W.fc1_wp; a.M = M; a.N = DM; a.K = D; a.m_dev = total; a.bias = W.fc1_b; a.out_at = h1; a.out_at2 = gp;
        rc = launch_gemm(P, EPI_FC1, a, s); if (rc) return rc;
    }
    if (P != 0) {
        BwdPrepArgs a; a.g = dy; a.h = nullptr; a.dst_of = nullptr; a.row_mask = nullptr; a.g_at = g_at; a.dH = nullptr; a.dmask = nullptr; a.M = M; a.gs = gs;
        rc = launch_bwd_prep(P, a, s); if (rc) return rc;
    }
    {
        GemmArgs a; a.A = P == 0 ? (const void*)dy : (const void*)g_at; a.W = W.fc2_wT; a.Wp = W.fc2_wTp; a.M = M; a.N = DM; a.K = D; a.m_dev = total;
        a.aux_at = gp; a.a_map = row_src; a.out_at = dZ;
        rc = launch_gemm(P, EPI_GELU_BWD, a, s); if (rc) return rc;
    }
    {
        GemmArgs a; a.A = dZ; a.W = W.fc1_wT; a.Wp = W.fc1_wTp; a.M = M; a.N = D; a.K = DM; a.m_dev = total; a.out_at = dA2;
        rc = launch_gemm(P, EPI_STORE_AT, a, s); if (rc) return rc;
    }
    {
        TokBwdArgs a;
        a.du = du; a.dA2 = dA2; a.dst_of = dst_of; a.u = u; a.stats2 = st; a.ln2_w = W.ln2_w; a.gate_w = nullptr; a.soft = nullptr; a.maskf = mask;
        a.dmask = nullptr; a.dtoken_select = nullptr; a.dtoken_logits = nullptr; a.dtok = nullptr; a.out_stride = 0; a.training = 0; a.tau = 1.0f;
        a.du_at = nullptr; a.partial = partial; a.M = M; a.write_du = 1; a.gs = gs; a.inv_gs = 1.0f / gs;
        int nblk = 0;
        rc = launch_tok_bwd(P, a, &nblk, s); if (rc) return rc;
    }
    DYT_HIP_CHECK(hipStreamSynchronize(s));
    return DYT_OK;
}

extern "C" int dyt_gate_compact(const float* u, const float* w, const float* b, const float* g1, const float* g2, int batch,
                                int training, float tau, float threshold, float* mask, float* logits, int32_t* keep_idx,
                                int32_t* counts, int32_t* total, void* stream) {
    if (!u || !w || !b || !mask || !logits || !keep_idx || !counts || !total || batch < 1) { set_error("bad argument"); return DYT_ERR_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scratch sc;
    const size_t M = (size_t)batch * NT;
    float* soft = (float*)sc.get(M * 4); float* maskf = (float*)sc.get(M * 4);
    int* keep_local = (int*)sc.get(M * 4); int* dst_of = (int*)sc.get(M * 4);
    float* xn = (float*)sc.get(M * D * 4); float2* st = (float2*)sc.get(M * sizeof(float2)); float* ones = (float*)sc.get(2 * D * 4);
    if (!soft || !maskf || !keep_local || !dst_of || !xn || !st || !ones) { set_error("scratch alloc failed"); return DYT_ERR_HIP; }
    GateArgs ga;
    ga.u = u; ga.w = w; ga.b = b; ga.g1 = g1; ga.g2 = g2; ga.batch = batch; ga.training = training; ga.tau = tau;
    ga.threshold = threshold; ga.seed = 0; ga.subseq = 0; ga.soft = soft; ga.maskf = maskf; ga.out_select = mask;
    ga.out_logits = logits; ga.out_stride = NP; ga.keep_local = keep_local; ga.counts = counts;
    int rc = launch_gate(ga, s); if (rc) return rc;
    // flat ascending list of kept rows (= nonzero() of model_speed_test.py:300) built on the DEVICE by the product's own
    // gather kernel: its row_src output is that list, its device-side total the length (the LayerNorm it also computes is discarded)
    DYT_HIP_CHECK(hipMemsetAsync(keep_idx, 0xff, M * 4, s));
    DYT_HIP_CHECK(hipMemsetAsync(ones, 0, 2 * D * 4, s));
    rc = launch_ln_gather(0, u, ones, ones + D, keep_local, counts, total, maskf, xn, st, keep_idx, dst_of, batch, s);
    if (rc) return rc;
    DYT_HIP_CHECK(hipStreamSynchronize(s));
    return DYT_OK;
}

// ---- the backward row kernels alone (block_bwd.hip, ln.hip: bwd_prep, ln_bwd, ln_param_grad / ln_param_reduce, tok_bwd + the deferred gate-gradient
// ---- reduction): argument checks, the product's own launch_* function, synchronise.  Test-only (tests/test_gpu_row_bwd.py). ----
static int unit_precision_ok(const char* who, int precision) {
    if (precision == 0 || precision == 1) return 0;
    set_error("%s: precision %d (0 = fp32, 1 = the library's 16-bit operand type)", who, precision);
    return DYT_ERR_ARG;
}

extern "C" int dyt_unit_bwd_prep(const float* g, const void* h, const int32_t* dst_of, const float* row_mask, void* g_at, void* dH,
                                 float* dmask, int M, float gs, int precision, void* stream) {
    { int rc = unit_precision_ok("dyt_unit_bwd_prep", precision); if (rc) return rc; }
    if (!g || M < 1) { set_error("dyt_unit_bwd_prep: g is NULL or M = %d < 1", M); return DYT_ERR_ARG; }
    if (!g_at && !dH && !dmask) { set_error("dyt_unit_bwd_prep: no output (g_at, dH and dmask are all NULL)"); return DYT_ERR_ARG; }
    if (!(gs > 0.f)) { set_error("dyt_unit_bwd_prep: gs = %g (> 0)", gs); return DYT_ERR_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    BwdPrepArgs a; a.g = g; a.h = h; a.dst_of = dst_of; a.row_mask = row_mask; a.g_at = g_at; a.dH = dH; a.dmask = dmask; a.M = M; a.gs = gs;
    int rc = launch_bwd_prep(precision, a, s);
    if (rc) return rc;
    DYT_HIP_CHECK(hipStreamSynchronize(s));
    return DYT_OK;
}

extern "C" int dyt_unit_ln_bwd(const void* dy, const float* x, const float* stats, const float* w, const float* base, const void* base_at,
                               float* dx, int rows, void* g_at, const void* h_next, const int32_t* dst_of_next, float* dmask_next, float gs,
                               void* out3, float s3, int out3_hi_only, int precision, void* stream) {
    { int rc = unit_precision_ok("dyt_unit_ln_bwd", precision); if (rc) return rc; }
    if (!dy || !x || !stats || !w || rows < 1) { set_error("dyt_unit_ln_bwd: dy / x / stats / w is NULL or rows = %d < 1", rows); return DYT_ERR_ARG; }
    if (!dx && !g_at && !out3) { set_error("dyt_unit_ln_bwd: no output row (dx, g_at and out3 are all NULL)"); return DYT_ERR_ARG; }
    if (out3 && precision != 0) { set_error("dyt_unit_ln_bwd: out3 (the split operand) exists at precision 0 only"); return DYT_ERR_ARG; }
    if (base_at && precision == 0) { set_error("dyt_unit_ln_bwd: base_at (the 16-bit stream) exists at precision 1 only"); return DYT_ERR_ARG; }
    if (base && base_at) { set_error("dyt_unit_ln_bwd: base and base_at are alternatives"); return DYT_ERR_ARG; }
    if (!(gs > 0.f)) { set_error("dyt_unit_ln_bwd: gs = %g (> 0)", gs); return DYT_ERR_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = launch_ln_bwd(precision, dy, x, reinterpret_cast<const float2*>(stats), w, base, dx, rows, g_at, h_next, dst_of_next, dmask_next, gs, s,
                           out3, s3, out3_hi_only, base_at);
    if (rc) return rc;
    DYT_HIP_CHECK(hipStreamSynchronize(s));
    return DYT_OK;
}

extern "C" int dyt_unit_ln_bwd_tap(const void* dy, const float* x, const float* stats, const float* w, const float* base, const void* base_at,
                                   float* dx, int rows, void* g_at, const void* h_next, const int32_t* dst_of_next, float* dmask_next, float gs,
                                   void* out3, float s3, int out3_hi_only, const float* tap, int precision, void* stream) {
    { int rc = unit_precision_ok("dyt_unit_ln_bwd_tap", precision); if (rc) return rc; }
    if (!dy || !x || !stats || !w || !tap || rows < 1) { set_error("dyt_unit_ln_bwd_tap: dy / x / stats / w / tap is NULL or rows = %d < 1", rows); return DYT_ERR_ARG; }
    if (!dx && !g_at && !out3) { set_error("dyt_unit_ln_bwd_tap: no output row (dx, g_at and out3 are all NULL)"); return DYT_ERR_ARG; }
    if (out3 && precision != 0) { set_error("dyt_unit_ln_bwd_tap: out3 (the split operand) exists at precision 0 only"); return DYT_ERR_ARG; }
    if (base_at && precision == 0) { set_error("dyt_unit_ln_bwd_tap: base_at (the 16-bit stream) exists at precision 1 only"); return DYT_ERR_ARG; }
    if (base && base_at) { set_error("dyt_unit_ln_bwd_tap: base and base_at are alternatives"); return DYT_ERR_ARG; }
    if (!(gs > 0.f)) { set_error("dyt_unit_ln_bwd_tap: gs = %g (> 0)", gs); return DYT_ERR_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = launch_ln_bwd(precision, dy, x, reinterpret_cast<const float2*>(stats), w, base, dx, rows, g_at, h_next, dst_of_next, dmask_next, gs, s,
                           out3, s3, out3_hi_only, base_at, tap);
    if (rc) return rc;
    DYT_HIP_CHECK(hipStreamSynchronize(s));
    return DYT_OK;
}

extern "C" int dyt_unit_ln_param_grad(const void* dy, const float* x, const float* stats, float* out, int rows, float gs, int precision,
                                      void* stream) {
    { int rc = unit_precision_ok("dyt_unit_ln_param_grad", precision); if (rc) return rc; }
    if (!dy || !x || !stats || !out || rows < 1) { set_error("dyt_unit_ln_param_grad: dy / x / stats / out is NULL or rows = %d < 1", rows); return DYT_ERR_ARG; }
    if (!(gs > 0.f)) { set_error("dyt_unit_ln_param_grad: gs = %g (> 0)", gs); return DYT_ERR_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scratch sc;
    float* partial = (float*)sc.get((size_t)ln_param_grad_scratch_floats(rows) * sizeof(float));
    if (!partial) { set_error("scratch alloc failed"); return DYT_ERR_HIP; }
    int rc = launch_ln_param_grad(precision, dy, x, reinterpret_cast<const float2*>(stats), partial, out, rows, gs, s);
    if (rc) return rc;
    DYT_HIP_CHECK(hipStreamSynchronize(s));
    return DYT_OK;
}

extern "C" int dyt_unit_tok_bwd(const dyt_unit_tok_bwd_args* p, float* d_gate, int precision, void* stream) {
    { int rc = unit_precision_ok("dyt_unit_tok_bwd", precision); if (rc) return rc; }
    if (!p) { set_error("dyt_unit_tok_bwd: args is NULL"); return DYT_ERR_ARG; }
    if (p->M < NT || p->M % NT != 0) { set_error("dyt_unit_tok_bwd: M = %d is not a positive multiple of %d (the kernel takes image = token / %d)", p->M, NT, NT); return DYT_ERR_ARG; }
    const bool wr = p->write_du != 0, lnpart = p->dA2 && wr;
    if (wr && !p->du && !p->du_at) { set_error("dyt_unit_tok_bwd: write_du without du or du_at"); return DYT_ERR_ARG; }
    if (wr && !p->g_cls && !p->du && !p->du_in_at) { set_error("dyt_unit_tok_bwd: write_du without an incoming gradient (du, du_in_at or g_cls)"); return DYT_ERR_ARG; }
    if (p->du3 && precision != 0) { set_error("dyt_unit_tok_bwd: du3 (the split operand) exists at precision 0 only"); return DYT_ERR_ARG; }
    if (p->du_in_at && precision == 0) { set_error("dyt_unit_tok_bwd: du_in_at (the 16-bit stream) exists at precision 1 only"); return DYT_ERR_ARG; }
    if (precision == 0 && p->gs != 1.0f) { set_error("dyt_unit_tok_bwd: gs = %g at precision 0 (fp32 operands carry no factor)", p->gs); return DYT_ERR_ARG; }
    if (!(p->gs > 0.f)) { set_error("dyt_unit_tok_bwd: gs = %g (> 0)", p->gs); return DYT_ERR_ARG; }
    if ((p->dA2 || p->gate_w) && !p->u) { set_error("dyt_unit_tok_bwd: u is NULL (read for the LN2 backward and the gate gradient)"); return DYT_ERR_ARG; }
    if (lnpart && (!p->stats2 || !p->ln2_w)) { set_error("dyt_unit_tok_bwd: dA2 without stats2 / ln2_w"); return DYT_ERR_ARG; }
    if (p->gate_w) {
        if (!p->soft || !d_gate) { set_error("dyt_unit_tok_bwd: gate_w without soft / d_gate"); return DYT_ERR_ARG; }
        if (p->training && !(p->tau > 0.f)) { set_error("dyt_unit_tok_bwd: tau = %g (> 0)", p->tau); return DYT_ERR_ARG; }
        if (((p->dtok && !p->dtoken_select) || p->cat_dact) && !p->maskf) { set_error("dyt_unit_tok_bwd: dtok / cat_dact without maskf"); return DYT_ERR_ARG; }
        if ((p->dtoken_select || p->dtoken_logits) && p->out_stride < NP) { set_error("dyt_unit_tok_bwd: out_stride = %d < %d", p->out_stride, NP); return DYT_ERR_ARG; }
        if ((p->cat_dact != nullptr) != (p->cat_ddz != nullptr)) { set_error("dyt_unit_tok_bwd: cat_dact and cat_ddz come together"); return DYT_ERR_ARG; }
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scratch sc;
    const int nblk_max = (p->M + 31) / 32;
    float* partial = (float*)sc.get((size_t)nblk_max * (D + 1) * sizeof(float));
    if (!partial) { set_error("scratch alloc failed"); return DYT_ERR_HIP; }
    TokBwdArgs a;
    a.du = p->du; a.dA2 = p->dA2; a.dst_of = p->dst_of; a.u = p->u; a.stats2 = reinterpret_cast<const float2*>(p->stats2); a.ln2_w = p->ln2_w;
    a.gate_w = p->gate_w; a.soft = p->soft; a.maskf = p->maskf; a.dmask = p->dmask;
    a.dtoken_select = p->dtoken_select; a.dtoken_logits = p->dtoken_logits; a.dtok = p->dtok; a.out_stride = p->out_stride;
    a.training = p->training; a.tau = p->tau; a.du_at = p->du_at; a.partial = partial; a.M = p->M; a.write_du = wr ? 1 : 0;
    a.gs = p->gs; a.inv_gs = 1.0f / p->gs; a.dad = p->dad; a.g_cls = p->g_cls;
    a.cat_dact = p->cat_dact; a.cat_ddz = p->cat_ddz; a.cat_scale = p->cat_scale; a.cat_ddz_scale = p->cat_ddz_scale; a.cat_ddz_dscale = p->cat_ddz_dscale;
    a.du3 = p->du3; a.du3_scale = p->du3_scale; a.du3_hi_only = p->du3_hi_only != 0;
    a.branch_scale = p->branch_scale; a.du_in_at = p->du_in_at;
    int nblk = 0;
    int rc = launch_tok_bwd(precision, a, &nblk, s);
    if (rc) return rc;
    if (nblk > nblk_max) { set_error("dyt_unit_tok_bwd: %d workgroups for %d partial rows", nblk, nblk_max); return DYT_ERR_STATE; }
    if (p->gate_w) {   // the production path of the gate gradient: queued, then flushed (reduce_partials_batch_kernel)
        ReduceQueue rq;
        rc = queue_tok_reduce(rq, partial, nblk, d_gate); if (rc) return rc;
        rc = flush_reductions(rq, s); if (rc) return rc;
    }
    DYT_HIP_CHECK(hipStreamSynchronize(s));
    return DYT_OK;
}

// ---- the forward row kernels alone (dispatch.hip, ln.hip, embed.hip: the token dispatcher, the LayerNorm family around it, the folded form's
// ---- weight side and the embedding prologue): argument checks, the product's own launch_* function, synchronise.  Test-only
// ---- (tests/test_gpu_row_fwd.py).  No arithmetic here. ----
extern "C" int dyt_unit_gate(const dyt_unit_gate_args* p, void* stream) {
    if (!p) { set_error("dyt_unit_gate: args is NULL"); return DYT_ERR_ARG; }
    if (!p->u || !p->w || !p->b || !p->soft || !p->maskf || !p->keep_local || !p->counts) { set_error("dyt_unit_gate: u / w / b / soft / maskf / keep_local / counts is NULL"); return DYT_ERR_ARG; }
    if (p->batch < 1) { set_error("dyt_unit_gate: batch = %d < 1", p->batch); return DYT_ERR_ARG; }
    if ((p->g1 != nullptr) != (p->g2 != nullptr)) { set_error("dyt_unit_gate: g1 and g2 come together"); return DYT_ERR_ARG; }
    if (p->training && !(p->tau > 0.f)) { set_error("dyt_unit_gate: tau = %g (> 0)", p->tau); return DYT_ERR_ARG; }
    if ((p->out_select || p->out_logits) && p->out_stride < NP) { set_error("dyt_unit_gate: out_stride = %d < %d", p->out_stride, NP); return DYT_ERR_ARG; }
    if (p->force_first < 0 || p->force_first > NT) { set_error("dyt_unit_gate: force_first = %d (0..%d)", p->force_first, NT); return DYT_ERR_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    GateArgs a;
    a.u = p->u; a.w = p->w; a.b = p->b; a.g1 = p->g1; a.g2 = p->g2; a.batch = p->batch; a.training = p->training; a.tau = p->tau;
    a.threshold = p->threshold; a.seed = p->seed; a.subseq = p->subseq; a.seed_dev = p->seed_dev; a.soft = p->soft; a.maskf = p->maskf;
    a.out_select = p->out_select; a.out_logits = p->out_logits; a.out_stride = p->out_stride; a.force_first = p->force_first;
    a.keep_local = p->keep_local; a.counts = p->counts;
    int rc = launch_gate(a, s);
    if (rc) return rc;
    DYT_HIP_CHECK(hipStreamSynchronize(s));
    return DYT_OK;
}

extern "C" int dyt_unit_gather_index(const int32_t* keep_local, const int32_t* counts, int32_t* total, const float* maskf, int32_t* row_src,
                                     int32_t* dst_of, int batch, int32_t* drop_src, void* stream) {
    if (!keep_local || !counts || !total || !maskf || !row_src || !dst_of) { set_error("dyt_unit_gather_index: keep_local / counts / total / maskf / row_src / dst_of is NULL"); return DYT_ERR_ARG; }
    if (batch < 1) { set_error("dyt_unit_gather_index: batch = %d < 1", batch); return DYT_ERR_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = launch_gather_index(keep_local, counts, total, maskf, row_src, dst_of, batch, s, drop_src);
    if (rc) return rc;
    DYT_HIP_CHECK(hipStreamSynchronize(s));
    return DYT_OK;
}

extern "C" int dyt_unit_ln_gather(const float* u, const float* w, const float* b, const int32_t* keep_local, const int32_t* counts, int32_t* total,
                                  const float* maskf, void* out, float* stats, int32_t* row_src, int32_t* dst_of, int batch, void* out3,
                                  int out3_f8, int32_t* drop_src, int precision, void* stream) {
    { int rc = unit_precision_ok("dyt_unit_ln_gather", precision); if (rc) return rc; }
    if (!u || !w || !b || !keep_local || !counts || !total || !maskf || !stats || !row_src || !dst_of) { set_error("dyt_unit_ln_gather: u / w / b / keep_local / counts / total / maskf / stats / row_src / dst_of is NULL"); return DYT_ERR_ARG; }
    if (batch < 1) { set_error("dyt_unit_ln_gather: batch = %d < 1", batch); return DYT_ERR_ARG; }
    if (out3 && precision != 0) { set_error("dyt_unit_ln_gather: out3 (the split operand) exists at precision 0 only"); return DYT_ERR_ARG; }
    if (!out && !out3) { set_error("dyt_unit_ln_gather: no output row (out and out3 are both NULL)"); return DYT_ERR_ARG; }
    if (out3_f8 && !out3) { set_error("dyt_unit_ln_gather: out3_f8 without out3"); return DYT_ERR_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = launch_ln_gather(precision, u, w, b, keep_local, counts, total, maskf, out, reinterpret_cast<float2*>(stats), row_src, dst_of, batch, s,
                              out3, out3_f8 ? 1 : 0, drop_src);
    if (rc) return rc;
    DYT_HIP_CHECK(hipStreamSynchronize(s));
    return DYT_OK;
}

extern "C" int dyt_unit_ln_fwd(const float* x, const float* w, const float* b, void* out, float* stats, int rows, void* out3, int out3_f8,
                               int precision, void* stream) {
    { int rc = unit_precision_ok("dyt_unit_ln_fwd", precision); if (rc) return rc; }
    if (!x || !w || !b || rows < 1) { set_error("dyt_unit_ln_fwd: x / w / b is NULL or rows = %d < 1", rows); return DYT_ERR_ARG; }
    if (out3 && precision != 0) { set_error("dyt_unit_ln_fwd: out3 (the split operand) exists at precision 0 only"); return DYT_ERR_ARG; }
    if (!out && !out3) { set_error("dyt_unit_ln_fwd: no output row (out and out3 are both NULL)"); return DYT_ERR_ARG; }
    if (out3_f8 && !out3) { set_error("dyt_unit_ln_fwd: out3_f8 without out3"); return DYT_ERR_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = launch_ln_fwd(precision, x, w, b, out, reinterpret_cast<float2*>(stats), rows, s, out3, out3_f8 ? 1 : 0);
    if (rc) return rc;
    DYT_HIP_CHECK(hipStreamSynchronize(s));
    return DYT_OK;
}

extern "C" int dyt_unit_adapter_ln_fwd(const float* x, const float* w, const float* b, void* out, float* stats, const float* resid, int rows,
                                       int out_at_precision, void* stream) {
    { int rc = unit_precision_ok("dyt_unit_adapter_ln_fwd", out_at_precision); if (rc) return rc; }
    if (!x || !w || !b || !out || rows < 1) { set_error("dyt_unit_adapter_ln_fwd: x / w / b / out is NULL or rows = %d < 1", rows); return DYT_ERR_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = launch_adapter_ln_fwd(out_at_precision, x, w, b, out, reinterpret_cast<float2*>(stats), resid, rows, s);
    if (rc) return rc;
    DYT_HIP_CHECK(hipStreamSynchronize(s));
    return DYT_OK;
}

extern "C" int dyt_unit_ln_cls(const float* u, const float* w, const float* b, void* out, float* stats, void* u_cls, int batch, int precision,
                               void* stream) {
    { int rc = unit_precision_ok("dyt_unit_ln_cls", precision); if (rc) return rc; }
    if (!u || !w || !b || !out || !stats || batch < 1) { set_error("dyt_unit_ln_cls: u / w / b / out / stats is NULL or batch = %d < 1", batch); return DYT_ERR_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = launch_ln_cls(precision, u, w, b, out, reinterpret_cast<float2*>(stats), u_cls, batch, s);
    if (rc) return rc;
    DYT_HIP_CHECK(hipStreamSynchronize(s));
    return DYT_OK;
}

extern "C" int dyt_unit_ln_fold_w(const float* W, const float* gamma, const float* beta, const float* bias, void* Wf, float* cs, float* bf, int N,
                                  int precision, void* stream) {
    { int rc = unit_precision_ok("dyt_unit_ln_fold_w", precision); if (rc) return rc; }
    if (!W || !gamma || !beta || !bias || !Wf || !cs || !bf || N < 1) { set_error("dyt_unit_ln_fold_w: W / gamma / beta / bias / Wf / cs / bf is NULL or N = %d < 1", N); return DYT_ERR_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = launch_ln_fold_w(precision, W, gamma, beta, bias, Wf, nullptr, cs, bf, N, s);   // (refuses precision 0 itself)
    if (rc) return rc;
    DYT_HIP_CHECK(hipStreamSynchronize(s));
    return DYT_OK;
}

extern "C" int dyt_unit_embed(const float* images, void* patches, const float* cls, const float* pos, float* x0, int batch, int precision,
                              void* stream) {
    { int rc = unit_precision_ok("dyt_unit_embed", precision); if (rc) return rc; }
    if (batch < 1) { set_error("dyt_unit_embed: batch = %d < 1", batch); return DYT_ERR_ARG; }
    if ((images != nullptr) != (patches != nullptr)) { set_error("dyt_unit_embed: images and patches come together"); return DYT_ERR_ARG; }
    const int ncls = (cls != nullptr) + (pos != nullptr) + (x0 != nullptr);
    if (ncls != 0 && ncls != 3) { set_error("dyt_unit_embed: cls, pos and x0 come together"); return DYT_ERR_ARG; }
    if (!images && !ncls) { set_error("dyt_unit_embed: nothing to do (images and cls are both NULL)"); return DYT_ERR_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = 0;
    if (images) {
        ImageLoadArgs a;
        a.src = images; a.src_kind = IMAGE_SRC_F32;
        a.dst = patches; a.dst_kind = precision == 0 ? IMAGE_DST_OPERAND_F32 : IMAGE_DST_OPERAND_16;
        a.batch = batch;
        rc = launch_image_load(a, s);
        if (rc) return rc;
    }
    if (ncls) { rc = launch_cls_rows(cls, pos, x0, batch, s); if (rc) return rc; }
    DYT_HIP_CHECK(hipStreamSynchronize(s));
    return DYT_OK;
}

extern "C" int dyt_unit_pad_convert(const float* src, void* dst, int rows, int cols, int dst_rows, int dst_cols, int transpose, int precision,
                                    void* stream) {
    { int rc = unit_precision_ok("dyt_unit_pad_convert", precision); if (rc) return rc; }
    if (!src || !dst) { set_error("dyt_unit_pad_convert: src / dst is NULL"); return DYT_ERR_ARG; }
    if (rows < 1 || cols < 1 || dst_rows < 1 || dst_cols < 1) { set_error("dyt_unit_pad_convert: shape %d x %d -> %d x %d (all >= 1)", rows, cols, dst_rows, dst_cols); return DYT_ERR_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = transpose ? launch_transpose_convert(precision, src, dst, rows, cols, dst_rows, dst_cols, s)
                       : launch_pad_convert(precision, src, dst, rows, cols, dst_rows, dst_cols, s);
    if (rc) return rc;
    DYT_HIP_CHECK(hipStreamSynchronize(s));
    return DYT_OK;
}

// ---- the attention kernels alone (attention.hip and its family units attention_{16,exact,split,v2}.hip): the structs are AttnFwdArgs / AttnBwdArgs of kernels.h field for field, the
// ---- kernel is whatever attn_fwd_route() / attn_bwd_route() pick from them and the three process-wide switches.  The launcher's own checks
// ---- refuse a bad call; no arithmetic, no kernels, no layout conversion here.  Test-only (tests/test_gpu_unit_attention.py). ----
extern "C" int dyt_unit_attn_fwd(const dyt_unit_attn_fwd_args* p, int precision, void* stream) {
    { int rc = unit_precision_ok("dyt_unit_attn_fwd", precision); if (rc) return rc; }
    if (!p) { set_error("dyt_unit_attn_fwd: args is NULL"); return DYT_ERR_ARG; }
    if (p->batch < 1) { set_error("dyt_unit_attn_fwd: batch = %d < 1", p->batch); return DYT_ERR_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    AttnFwdArgs a;
    a.q = p->q; a.k = p->k; a.v = p->v; a.planar = p->planar != 0;
    a.q_hi = p->q_hi; a.k_hi = p->k_hi; a.v_hi = p->v_hi; a.q_lo = p->q_lo; a.k_lo = p->k_lo; a.v_lo = p->v_lo;
    a.out = p->out; a.out3 = p->out3; a.out3_f8 = p->out3_f8 != 0;
    a.q16 = p->q16; a.k16 = p->k16; a.v16 = p->v16; a.o16 = p->o16;
    a.lse = p->lse; a.lse_optional = p->lse_optional != 0; a.split16 = p->split16 != 0; a.parts = p->parts; a.batch = p->batch;
    int rc = launch_attn_fwd(precision, a, s);
    if (rc) return rc;
    DYT_HIP_CHECK(hipStreamSynchronize(s));
    return DYT_OK;
}

extern "C" int dyt_unit_attn_bwd(const dyt_unit_attn_bwd_args* p, int precision, void* stream) {
    { int rc = unit_precision_ok("dyt_unit_attn_bwd", precision); if (rc) return rc; }
    if (!p) { set_error("dyt_unit_attn_bwd: args is NULL"); return DYT_ERR_ARG; }
    if (p->batch < 1) { set_error("dyt_unit_attn_bwd: batch = %d < 1", p->batch); return DYT_ERR_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    AttnBwdArgs a;
    a.q = p->q; a.k = p->k; a.v = p->v; a.out = p->out; a.out_ld = p->out_ld; a.dout = p->dout; a.lse = p->lse; a.delta = p->delta;
    a.dqkv = p->dqkv; a.dqkv3 = p->dqkv3; a.s3 = p->s3; a.out_hi_only = p->out_hi_only != 0; a.split16 = p->split16 != 0;
    a.grad_parts = p->grad_parts; a.q_tiles = p->q_tiles; a.batch = p->batch;
    int rc = launch_attn_bwd(precision, a, s);
    if (rc) return rc;
    DYT_HIP_CHECK(hipStreamSynchronize(s));
    return DYT_OK;
}

// ---- the weight-gradient and partial-reduction kernels alone (wgrad.hip): the struct is WgradArgs of kernels.h field for field, the caller owns
// ---- every buffer.  Argument checks, launch_wgrad / queue_tok_reduce / flush_reductions / launch_reduce_partials as backward.hip and step.hip
// ---- call them, synchronise.  No arithmetic, no kernels here.  Test-only (tests/test_gpu_unit_wgrad.py). ----
extern "C" int dyt_unit_wgrad(const dyt_unit_wgrad_args* prods, int n_prod, int pair, int defer, const dyt_unit_tok_reduce_args* toks, int n_tok,
                              int precision, void* stream) {
    { int rc = unit_precision_ok("dyt_unit_wgrad", precision); if (rc) return rc; }
    if (!prods) { set_error("dyt_unit_wgrad: prods is NULL"); return DYT_ERR_ARG; }
    if (n_prod < 1 || n_prod > ReduceQueue::MAX_WG) { set_error("dyt_unit_wgrad: n_prod = %d (1..%d)", n_prod, ReduceQueue::MAX_WG); return DYT_ERR_ARG; }
    if (n_tok < 0 || n_tok > ReduceQueue::MAX_TOK) { set_error("dyt_unit_wgrad: n_tok = %d (0..%d)", n_tok, ReduceQueue::MAX_TOK); return DYT_ERR_ARG; }
    if (n_tok > 0 && !defer) { set_error("dyt_unit_wgrad: n_tok = %d without defer (token reductions exist in the queue only)", n_tok); return DYT_ERR_ARG; }
    if (n_tok > 0 && !toks) { set_error("dyt_unit_wgrad: toks is NULL with n_tok = %d", n_tok); return DYT_ERR_ARG; }
    if (pair && (n_prod & 1)) { set_error("dyt_unit_wgrad: odd n_prod = %d with pair", n_prod); return DYT_ERR_ARG; }
    for (int i = 0; i < n_prod; ++i) {
        const dyt_unit_wgrad_args& p = prods[i];
        if (!p.X || !p.Y || !p.partial || !p.out_w) { set_error("dyt_unit_wgrad: product %d: X / Y / partial / out_w is NULL", i); return DYT_ERR_ARG; }
        if (p.r < 1 || p.r > RP) { set_error("dyt_unit_wgrad: product %d: r = %d (1..%d)", i, p.r, RP); return DYT_ERR_ARG; }
        if (p.M < 1) { set_error("dyt_unit_wgrad: product %d: M = %d < 1", i, p.M); return DYT_ERR_ARG; }
        if (p.half_products && precision != 0) { set_error("dyt_unit_wgrad: product %d: half_products exists at precision 0 only", i); return DYT_ERR_ARG; }
        if (!(p.x_scale > 0.f) || !(p.y_scale > 0.f)) { set_error("dyt_unit_wgrad: product %d: x_scale = %g, y_scale = %g (> 0)", i, p.x_scale, p.y_scale); return DYT_ERR_ARG; }
    }
    for (int i = 0; i < n_tok; ++i)
        if (!toks[i].partial || !toks[i].out || toks[i].nparts < 1) { set_error("dyt_unit_wgrad: token reduction %d: partial / out is NULL or nparts = %d < 1", i, toks[i].nparts); return DYT_ERR_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    ReduceQueue rq;
    ReduceQueue* q = defer ? &rq : nullptr;
    const int per = pair ? 2 : 1;
    int rc = 0;
    for (int i = 0; i < n_prod && !rc; i += per) {
        WgradArgs w[2];
        for (int k = 0; k < per; ++k) {
            const dyt_unit_wgrad_args& p = prods[i + k];
            WgradArgs& a = w[k];
            a.X = p.X; a.Y = p.Y; a.M = p.M; a.r = p.r; a.partial = p.partial;
            a.out_w = p.out_w; a.sc = p.sc; a.sj = p.sj; a.alpha = p.alpha;
            a.out_xsum = p.out_xsum; a.alpha_x = p.alpha_x; a.out_ysum = p.out_ysum; a.alpha_y = p.alpha_y;
            a.half_products = p.half_products != 0; a.x_scale = p.x_scale; a.y_scale = p.y_scale; a.alpha_dev = p.alpha_dev;
        }
        rc = launch_wgrad(precision, w, per, s, q);
    }
    for (int i = 0; i < n_tok && !rc; ++i) rc = queue_tok_reduce(rq, toks[i].partial, toks[i].nparts, toks[i].out);
    if (!rc && defer) rc = flush_reductions(rq, s);
    if (rc) { hipStreamSynchronize(s); return rc; }   // (what was accepted before the refusal has finished; the error text is the launcher's)
    DYT_HIP_CHECK(hipStreamSynchronize(s));
    return DYT_OK;
}

extern "C" int dyt_unit_reduce_partials(const float* partial, int nparts, int stride, float* out, int n, float alpha, void* stream) {
    if (!partial || !out) { set_error("dyt_unit_reduce_partials: partial / out is NULL"); return DYT_ERR_ARG; }
    if (nparts < 1 || n < 1 || stride < 0) { set_error("dyt_unit_reduce_partials: nparts = %d, n = %d (>= 1), stride = %d (>= 0)", nparts, n, stride); return DYT_ERR_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = launch_reduce_partials(partial, nparts, stride, out, n, alpha, s);
    if (rc) return rc;
    DYT_HIP_CHECK(hipStreamSynchronize(s));
    return DYT_OK;
}
