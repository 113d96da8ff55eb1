// The round-4 attention kernels for the 16-bit modes (bf16 / fp16 operands, v_mfma_f32_32x32x16): routes AF_16, AB_16_TWO,
// AB_16_FUSED and AB_16_FUSED_AHEAD of attn_route.h.  They run only with DYT_OPT_ATTN_V2 bits cleared (the default is
// attention_v2.hip) and are the fallback and A/B reference the round-5 kernels are measured against.
//
// N = 197 is small: K and V of one (image, head) are 25 KB in bf16 and live in LDS for the
// whole workgroup; a wave keeps the complete 32 x 224 score block of its query tile in
// registers, so no online-softmax rescaling is needed (197 is padded to 224 = 7 x 32 and the
// pad keys are masked to -inf).  Layout tricks, all addressing-only:
//   * scores are computed TRANSPOSED, S^T = K Q^T, so each lane owns one query column: the row
//     max / row sum are in-lane reductions plus a single cross-half shuffle;
//   * the MFMA C/D layout of that tile (lane <-> query, registers <-> keys) is already the
//     B-operand layout of the next MFMA (O^T = V^T P^T) up to a fixed permutation of the k
//     index; the A operand (V^T from an LDS-transposed copy) is fetched with the SAME
//     permutation, so P never moves between lanes;
//   * the same holds for every product of the backward pass (two phases: dQ per query tile,
//     dK/dV per key tile -- no atomics, deterministic).
#include "attn_common.h"

namespace dyt {

// ------------------------------------------------------------------------------------------
// forward, bf16
// ------------------------------------------------------------------------------------------
// Persistent: workgroup w walks the (image, head) pairs w, w + gridDim.x, ...; while it computes on one head the K, V and
// Q rows of the next are already in flight into registers (the staging's HBM/L2 latency was 1/3 of the kernel).
__global__ __launch_bounds__(448) void attn_fwd_bf16_kernel(const bf16* __restrict__ q, const bf16* __restrict__ k,
                                                            const bf16* __restrict__ v, bf16* __restrict__ out,
                                                            float* __restrict__ lse, int nheads) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16* Ks = reinterpret_cast<bf16*>(smem);
    bf16* Vt = reinterpret_cast<bf16*>(smem + ROW_IMG);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int qrow = wave * 32 + l31, qr = min(qrow, NT - 1);   // one 32-row query tile per wave (7 waves)
    StageRegs kr, vr;
    bf16x8 qn[4];
    auto prefetch = [&](int bh) {
        stage_load(kr, k + (size_t)bh * NT * HD, HD, tid);
        stage_load(vr, v + (size_t)bh * NT * HD, HD, tid);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
            qn[ks] = *reinterpret_cast<const bf16x8*>(q + ((size_t)bh * NT + qr) * HD + ks * 16 + hi * 8);
    };
    int bh = blockIdx.x;
    if (bh < nheads) prefetch(bh);
    for (; bh < nheads; bh += gridDim.x) {
        const int b = bh / NH, h = bh - b * NH;
        stage_store(kr, Ks, nullptr, tid);
        stage_store(vr, nullptr, Vt, tid);
        bf16x8 qf[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[ks] = qn[ks];
        __syncthreads();
        if (bh + gridDim.x < nheads) prefetch(bh + gridDim.x);   // lands while this head is computed
        f32x16 st[7];
#pragma unroll
        for (int kt = 0; kt < 7; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) st[kt][r] = 0.f;
        // S^T = K Q^T: the seven key tiles are independent accumulators -- walk them inside each k step so that consecutive
        // MFMAs never depend on each other, and read a whole k step's fragments ahead of its MFMAs
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            bf16x8 a[7];
#pragma unroll
            for (int kt = 0; kt < 7; ++kt) a[kt] = *reinterpret_cast<const bf16x8*>(Ks + (kt * 32 + l31) * RLD + ks * 16 + hi * 8);
#pragma unroll
            for (int kt = 0; kt < 7; ++kt) st[kt] = MFMA32(a[kt], qf[ks], st[kt]);
        }
        // st[kt][r] = S^T[key = kt*32 + (r&3) + 8*(r>>2) + 4*hi][q = l31]; mask the pad keys
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = 192 + (r & 3) + 8 * (r >> 2) + 4 * hi;
            if (key >= NT) st[6][r] = -INFINITY;
        }
        float mp[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};   // independent chains: the reductions are latency-, not issue-bound
#pragma unroll
        for (int kt = 0; kt < 7; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) mp[r & 3] = fmaxf(mp[r & 3], st[kt][r]);
        float m = fmaxf(fmaxf(mp[0], mp[1]), fmaxf(mp[2], mp[3]));
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        // exp, row sum and O^T = V^T P^T per key tile in one loop: the 4 MFMAs of tile kt execute while the VALU works on the
        // exponentials of tile kt+1 (as two separate loops the matrix pipe idled through the whole softmax and vice versa)
        float sp[4] = {0.f, 0.f, 0.f, 0.f};
        f32x16 o[2];
#pragma unroll
        for (int r = 0; r < 16; ++r) { o[0][r] = 0.f; o[1][r] = 0.f; }
#pragma unroll
        for (int kt = 0; kt < 7; ++kt) {
            bf16x8 vf[2][2];
#pragma unroll
            for (int half = 0; half < 2; ++half)
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) vf[half][dt] = join44(Vt + (dt * 32 + l31) * TLD + kt * 32 + half * 16 + 4 * hi);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = __expf(st[kt][r] - m);
                st[kt][r] = p;
                sp[r & 3] += p;
            }
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const bf16x8 pf = pack8(st[kt], half * 8);
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) o[dt] = MFMA32(vf[half][dt], pf, o[dt]);
            }
        }
        float sum = (sp[0] + sp[1]) + (sp[2] + sp[3]);
        sum += __shfl_xor(sum, 32, 64);
        if (hi == 0 && qrow < NT) lse[(size_t)bh * NT + qrow] = m + __logf(sum);
        if (qrow < NT) {
            const float inv = 1.0f / sum;
            bf16* op = out + ((size_t)b * NT + qrow) * D + h * HD;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    store4(op + dt * 32 + 8 * g + 4 * hi, o[dt][4 * g] * inv, o[dt][4 * g + 1] * inv,
                           o[dt][4 * g + 2] * inv, o[dt][4 * g + 3] * inv);
        }
        __syncthreads();   // every wave is done with this head's K / V images before they are overwritten
    }
}

// ------------------------------------------------------------------------------------------
// backward, bf16: the two phases, each ONE body for the stand-alone kernel and for both instances of the fused kernel (whose
// results are bit-identical to the two-kernel form's: tested).  What differs between the kernels -- where the row fragments and
// delta come from, prefetching, barriers -- stays in the kernels.
// ------------------------------------------------------------------------------------------
// dK/dV phase: the wave's key tile (lane's key `key`, its k / v rows kf / vf in registers) against the first nq query tiles of the
// Q / dO row images (Qs, dOs) and transposed images (Qt, dOt), lse / delta of the query rows read from LDS; stores dK and dV
__device__ __forceinline__ void bwd16_dkv_phase(const bf16* Qs, const bf16* dOs, const bf16* Qt, const bf16* dOt, const float* lse_s,
                                                const float* del_s, const bf16x8 (&kf)[4], const bf16x8 (&vf)[4], int nq, int key,
                                                int l31, int hi, bf16* dqkv, int b, int h) {
    f32x16 aK[2], aV[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { aK[0][r] = 0.f; aK[1][r] = 0.f; aV[0][r] = 0.f; aV[1][r] = 0.f; }

#pragma unroll 1
    for (int qt = 0; qt < nq; ++qt) {
        f32x16 s, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const bf16x8 qa = *reinterpret_cast<const bf16x8*>(Qs + (qt * 32 + l31) * RLD + ks * 16 + hi * 8);
            const bf16x8 da = *reinterpret_cast<const bf16x8*>(dOs + (qt * 32 + l31) * RLD + ks * 16 + hi * 8);
            s = MFMA32(qa, kf[ks], s);     // S[q][key]   (rows q in registers, column key = lane)
            dp = MFMA32(da, vf[ks], dp);   // dP[q][key]
        }
        f32x16 p;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int q0 = qt * 32 + 8 * g + 4 * hi;
            const float4 L4 = *reinterpret_cast<const float4*>(lse_s + q0);
            const float4 D4 = *reinterpret_cast<const float4*>(del_s + q0);
            const float Ls[4] = {L4.x, L4.y, L4.z, L4.w};
            const float Ds[4] = {D4.x, D4.y, D4.z, D4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = 4 * g + e;
                const bool ok = (q0 + e < NT) && (key < NT);
                const float pv = ok ? __expf(s[r] - Ls[e]) : 0.f;
                p[r] = pv;
                s[r] = pv * (dp[r] - Ds[e]);  // dS
            }
        }
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const bf16x8 pf = pack8(p, half * 8);
            const bf16x8 dsf = pack8(s, half * 8);
            const int qbase = qt * 32 + half * 16 + 4 * hi;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                const bf16x8 dot = join44(dOt + (dt * 32 + l31) * TLD + qbase);
                const bf16x8 qtf = join44(Qt + (dt * 32 + l31) * TLD + qbase);
                aV[dt] = MFMA32(dot, pf, aV[dt]);   // dV^T[d][key] += dO^T[d][q] P[q][key]
                aK[dt] = MFMA32(qtf, dsf, aK[dt]);  // dK^T[d][key] += Q^T[d][q] dS[q][key]
            }
        }
    }
    if (key < NT) {
        bf16* op = dqkv + ((size_t)b * NT + key) * (3 * D) + h * HD;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int d = dt * 32 + 8 * g + 4 * hi;
                store4(op + D + d, aK[dt][4 * g], aK[dt][4 * g + 1], aK[dt][4 * g + 2], aK[dt][4 * g + 3]);
                store4(op + 2 * D + d, aV[dt][4 * g], aV[dt][4 * g + 1], aV[dt][4 * g + 2], aV[dt][4 * g + 3]);
            }
    }
}

// dQ phase: the wave's query rows (lane's row `qrow`; its q / dO rows qf / dof in registers, their lse L and delta dl) against the
// seven key tiles of the K / V row images (Ks, Vs) and K^T (Kt); stores dQ x 0.125.  A wave that is not `active` (the fused kernel:
// its query tile carries no dO) walks no key tile and stores its zero rows
__device__ __forceinline__ void bwd16_dq_phase(const bf16* Ks, const bf16* Vs, const bf16* Kt, const bf16x8 (&qf)[4],
                                               const bf16x8 (&dof)[4], float L, float dl, bool active, int qrow, int l31, int hi,
                                               bf16* dqkv, int b, int h) {
    f32x16 dq[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { dq[0][r] = 0.f; dq[1][r] = 0.f; }
    auto scores = [&](int kt, f32x16& s_, f32x16& dp_) {   // S^T[key][q], dP^T[key][q] of key tile kt
#pragma unroll
        for (int r = 0; r < 16; ++r) { s_[r] = 0.f; dp_[r] = 0.f; }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const bf16x8 ka = *reinterpret_cast<const bf16x8*>(Ks + (kt * 32 + l31) * RLD + ks * 16 + hi * 8);
            const bf16x8 va = *reinterpret_cast<const bf16x8*>(Vs + (kt * 32 + l31) * RLD + ks * 16 + hi * 8);
            s_ = MFMA32(ka, qf[ks], s_);
            dp_ = MFMA32(va, dof[ks], dp_);
        }
    };
#pragma unroll 1
    for (int kt = 0; kt < (active ? 7 : 0); ++kt) {
        f32x16 s_, dp_;
        scores(kt, s_, dp_);
        bf16x8 ktf[2][2];
#pragma unroll
        for (int half = 0; half < 2; ++half)
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) ktf[half][dt] = join44(Kt + (dt * 32 + l31) * TLD + kt * 32 + half * 16 + 4 * hi);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
            const float p = key < NT ? __expf(s_[r] - L) : 0.f;
            s_[r] = p * (dp_[r] - dl);        // dS^T
        }
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const bf16x8 dsf = pack8(s_, half * 8);
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) dq[dt] = MFMA32(ktf[half][dt], dsf, dq[dt]);  // dQ^T[d][q] += K^T[d][key] dS^T[key][q]
        }
    }
    if (qrow < NT) {
        bf16* op = dqkv + ((size_t)b * NT + qrow) * (3 * D) + h * HD;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                store4(op + dt * 32 + 8 * g + 4 * hi, dq[dt][4 * g] * 0.125f, dq[dt][4 * g + 1] * 0.125f,
                       dq[dt][4 * g + 2] * 0.125f, dq[dt][4 * g + 3] * 0.125f);
    }
}

// ------------------------------------------------------------------------------------------
// backward, bf16: dQ (+ delta = rowsum(dO * O)) per query tile
// ------------------------------------------------------------------------------------------
// Persistent over heads like the forward kernel (next head's K, V and this wave's q / dO / O rows in flight during the
// current one).
__global__ __launch_bounds__(448) void attn_bwd_dq_bf16_kernel(const bf16* __restrict__ q, const bf16* __restrict__ k,
                                                               const bf16* __restrict__ v, const bf16* __restrict__ o,
                                                               const bf16* __restrict__ dout,
                                                               const float* __restrict__ lse, float* __restrict__ delta,
                                                               bf16* __restrict__ dqkv, int nheads, int o_ld) {
    // o_ld: row stride of `o` in elements (768; 1536 when o is the hi plane of a [M][hi | ...] split operand image)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16* Ks = reinterpret_cast<bf16*>(smem);
    bf16* Vs = reinterpret_cast<bf16*>(smem + ROW_IMG);
    bf16* Kt = reinterpret_cast<bf16*>(smem + 2 * ROW_IMG);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int qrow = wave * 32 + l31, qr = min(qrow, NT - 1);   // one 32-row query tile per wave (7 waves)
    StageRegs kr, vr;
    bf16x8 qn[4], don[4], on[4];
    float Ln = 0.f;
    auto prefetch = [&](int bh) {
        const int b = bh / NH, h = bh - b * NH;
        stage_load(kr, k + (size_t)bh * NT * HD, HD, tid);
        stage_load(vr, v + (size_t)bh * NT * HD, HD, tid);
        const size_t trow = ((size_t)b * NT + qr) * D + h * HD;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            qn[ks] = *reinterpret_cast<const bf16x8*>(q + ((size_t)bh * NT + qr) * HD + ks * 16 + hi * 8);
            don[ks] = *reinterpret_cast<const bf16x8*>(dout + trow + ks * 16 + hi * 8);
            on[ks] = *reinterpret_cast<const bf16x8*>(o + ((size_t)b * NT + qr) * o_ld + h * HD + ks * 16 + hi * 8);
        }
        Ln = lse[(size_t)bh * NT + qr];
    };
    int bh = blockIdx.x;
    if (bh < nheads) prefetch(bh);
    for (; bh < nheads; bh += gridDim.x) {
        const int b = bh / NH, h = bh - b * NH;
        stage_store(kr, Ks, Kt, tid);
        stage_store(vr, Vs, nullptr, tid);
        bf16x8 qf[4], dof[4];
        float dl = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            qf[ks] = qn[ks]; dof[ks] = don[ks];
#pragma unroll
            for (int i = 0; i < 8; ++i) dl += (float)don[ks][i] * (float)on[ks][i];
        }
        const float L = Ln;
        dl += __shfl_xor(dl, 32, 64);
        if (hi == 0 && qrow < NT) delta[(size_t)bh * NT + qrow] = dl;
        __syncthreads();
        if (bh + gridDim.x < nheads) prefetch(bh + gridDim.x);
        bwd16_dq_phase(Ks, Vs, Kt, qf, dof, L, dl, true, qrow, l31, hi, dqkv, b, h);
        __syncthreads();   // every wave is done with this head's images before they are overwritten
    }
}

// ------------------------------------------------------------------------------------------
// backward, bf16: dK, dV per key tile
// ------------------------------------------------------------------------------------------
// 7 waves, one 32-key tile each; persistent over heads with the next head's Q / dO rows (and lse, delta) in flight.
__global__ __launch_bounds__(448) void attn_bwd_dkv_bf16_kernel(const bf16* __restrict__ q, const bf16* __restrict__ k,
                                                                const bf16* __restrict__ v,
                                                                const bf16* __restrict__ dout,
                                                                const float* __restrict__ lse,
                                                                const float* __restrict__ delta,
                                                                bf16* __restrict__ dqkv, int nheads) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16* Qs = reinterpret_cast<bf16*>(smem);
    bf16* dOs = reinterpret_cast<bf16*>(smem + ROW_IMG);
    bf16* Qt = reinterpret_cast<bf16*>(smem + 2 * ROW_IMG);
    bf16* dOt = reinterpret_cast<bf16*>(smem + 2 * ROW_IMG + TR_IMG);
    float* lse_s = reinterpret_cast<float*>(smem + 2 * ROW_IMG + 2 * TR_IMG);
    float* del_s = lse_s + NPAD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int key = wave * 32 + l31, kr_ = min(key, NT - 1);
    StageRegs qr, dr;
    float ln = 0.f, dn = 0.f;
    auto prefetch = [&](int bh) {
        const int b = bh / NH, h = bh - b * NH;
        stage_load(qr, q + (size_t)bh * NT * HD, HD, tid);
        stage_load(dr, dout + (size_t)b * NT * D + h * HD, D, tid);
        if (tid < NPAD) {
            ln = tid < NT ? lse[(size_t)bh * NT + tid] : 0.f;
            dn = tid < NT ? delta[(size_t)bh * NT + tid] : 0.f;
        }
    };
    int bh = blockIdx.x;
    if (bh < nheads) prefetch(bh);
    for (; bh < nheads; bh += gridDim.x) {
        const int b = bh / NH, h = bh - b * NH;
        const bf16* kb = k + ((size_t)bh * NT + kr_) * HD;
        const bf16* vb = v + ((size_t)bh * NT + kr_) * HD;
        bf16x8 kf[4], vf[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {   // this head's key / value rows of the wave's tile: land during the staging stores
            kf[ks] = *reinterpret_cast<const bf16x8*>(kb + ks * 16 + hi * 8);
            vf[ks] = *reinterpret_cast<const bf16x8*>(vb + ks * 16 + hi * 8);
        }
        stage_store(qr, Qs, Qt, tid);
        stage_store(dr, dOs, dOt, tid);
        if (tid < NPAD) { lse_s[tid] = ln; del_s[tid] = dn; }
        __syncthreads();
        if (bh + gridDim.x < nheads) prefetch(bh + gridDim.x);
        bwd16_dkv_phase(Qs, dOs, Qt, dOt, lse_s, del_s, kf, vf, 7, key, l31, hi, dqkv, b, h);
        __syncthreads();   // every wave is done with this head's images before they are overwritten
    }
}

// ------------------------------------------------------------------------------------------
// backward, bf16: dQ and dK / dV of one (image, head) in ONE workgroup pass
// ------------------------------------------------------------------------------------------
// The two kernels above each stream q, k, v, dO (and o) of every head from memory: 12 passes over a [M,768] operand per
// backward (464 MB at B=128) at ~3 TB/s -- the attention backward is bound by that traffic and by per-head latencies, not by
// the matrix pipe.  Here a persistent workgroup runs the dK/dV phase and the dQ phase of a head back to back on the same LDS:
//   phase B  Q, dO staged once (row + transposed images); the wave's k / v rows in registers; delta = rowsum(dO * o) goes
//            from registers to LDS (no trip through memory) -> dK, dV   (bwd16_dkv_phase, as attn_bwd_dkv_bf16_kernel)
//   switch   every wave takes the q / dO rows of ITS query tile from the row images (phase A's B operands), then the K / V
//            images (row + K^T) replace Q / dO: their cooperative loads were issued before phase B and landed under it
//   phase A  dQ   (bwd16_dq_phase, as attn_bwd_dq_bf16_kernel)
// Q, dO and o are read once, k / v twice by the same workgroup within one head (second read from L2): 8 operand passes
// instead of 12, one launch instead of two.  The heavy phase (B: four accumulators) runs with 64 prefetch registers in
// flight, the light one (A) with the next head's 112 -- in the opposite order the kernel spills.  Both phases are the
// bodies the two kernels above call, so the results are bit-identical to theirs (tested).
template <bool ROWPF>
__global__ __launch_bounds__(448) void attn_bwd_fused_bf16_kernel(const bf16* __restrict__ q, const bf16* __restrict__ k,
                                                                  const bf16* __restrict__ v, const bf16* __restrict__ o,
                                                                  const bf16* __restrict__ dout,
                                                                  const float* __restrict__ lse, float* __restrict__ delta,
                                                                  bf16* __restrict__ dqkv, int nheads, int nq, int o_ld) {
    // nq: query tiles (of 32 rows) that can carry a non-zero dO -- 7, or 1 when only the cls rows have an upstream gradient
    // (last block, cls-only tail): rows with dO = 0 have dP = delta = 0, hence dS = 0 and no contribution to dK / dV / dQ, so
    // phase B walks nq query tiles and only the first nq waves run phase A (the others store their zero dQ rows)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // phase B images
    bf16* Qs = reinterpret_cast<bf16*>(smem);
    bf16* dOs = reinterpret_cast<bf16*>(smem + ROW_IMG);
    bf16* Qt = reinterpret_cast<bf16*>(smem + 2 * ROW_IMG);
    bf16* dOt = reinterpret_cast<bf16*>(smem + 2 * ROW_IMG + TR_IMG);
    float* lse_s = reinterpret_cast<float*>(smem + 2 * ROW_IMG + 2 * TR_IMG);
    float* del_s = lse_s + NPAD;
    // phase A images (same bytes)
    bf16* Ks = reinterpret_cast<bf16*>(smem);
    bf16* Vs = reinterpret_cast<bf16*>(smem + ROW_IMG);
    bf16* Kt = reinterpret_cast<bf16*>(smem + 2 * ROW_IMG);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int qrow = wave * 32 + l31, qr = min(qrow, NT - 1);   // the wave's key tile (phase B) = its query tile (phase A)
    StageRegs qs_, ds_;            // next head's Q / dO (cooperative): in flight during phase A
    bf16x8 kfr[4], vfr[4], on[4];  // k / v / o rows of this wave's tile
    float Ln = 0.f;
    auto load_rows = [&](int bh) {
        const int b = bh / NH, h = bh - b * NH;
        const size_t hrow = ((size_t)bh * NT + qr) * HD;
        const size_t trow = ((size_t)b * NT + qr) * D + h * HD;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            kfr[ks] = *reinterpret_cast<const bf16x8*>(k + hrow + ks * 16 + hi * 8);
            vfr[ks] = *reinterpret_cast<const bf16x8*>(v + hrow + ks * 16 + hi * 8);
            on[ks] = *reinterpret_cast<const bf16x8*>(o + ((size_t)b * NT + qr) * o_ld + h * HD + ks * 16 + hi * 8);
        }
        Ln = lse[(size_t)bh * NT + qr];
    };
    auto prefetch = [&](int bh) {
        const int b = bh / NH, h = bh - b * NH;
        stage_load(qs_, q + (size_t)bh * NT * HD, HD, tid);
        stage_load(ds_, dout + (size_t)b * NT * D + h * HD, D, tid);
        if (ROWPF) load_rows(bh);   // else: issued at the head's start, first used after the image stores and two barriers
    };
    int bh = blockIdx.x;
    if (bh < nheads) prefetch(bh);
    for (; bh < nheads; bh += gridDim.x) {
        const int b = bh / NH, h = bh - b * NH;
        if (!ROWPF) load_rows(bh);
        stage_store(qs_, Qs, Qt, tid);
        stage_store(ds_, dOs, dOt, tid);
        const float L = Ln;
        bf16x8 kf[4], vf[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) { kf[ks] = kfr[ks]; vf[ks] = vfr[ks]; }
        __syncthreads();
        // delta of this wave's query rows: dO rows from the image just written (the operand order of the dQ kernel's sum)
        float dl = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const bf16x8 dv = *reinterpret_cast<const bf16x8*>(dOs + qrow * RLD + ks * 16 + hi * 8);
#pragma unroll
            for (int i = 0; i < 8; ++i) dl += (float)dv[i] * (float)on[ks][i];
        }
        dl += __shfl_xor(dl, 32, 64);
        if (hi == 0) {
            lse_s[qrow] = qrow < NT ? L : 0.f;
            del_s[qrow] = qrow < NT ? dl : 0.f;
            if (qrow < NT) delta[(size_t)bh * NT + qrow] = dl;
        }
        __syncthreads();
        StageRegs kr, vr;   // this head's K / V for the phase-A images: in flight during phase B
        stage_load(kr, k + (size_t)bh * NT * HD, HD, tid);
        stage_load(vr, v + (size_t)bh * NT * HD, HD, tid);
        // ---------------- phase B: dK, dV ----------------
        bwd16_dkv_phase(Qs, dOs, Qt, dOt, lse_s, del_s, kf, vf, nq, qrow, l31, hi, dqkv, b, h);
        // ---------------- switch ----------------
        bf16x8 qf[4], dof[4];   // q / dO rows of this wave's query tile (pad rows are zero in the images; their columns are never stored)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            qf[ks] = *reinterpret_cast<const bf16x8*>(Qs + qrow * RLD + ks * 16 + hi * 8);
            dof[ks] = *reinterpret_cast<const bf16x8*>(dOs + qrow * RLD + ks * 16 + hi * 8);
        }
        __syncthreads();   // every wave is done with the Q / dO images
        stage_store(kr, Ks, Kt, tid);
        stage_store(vr, Vs, nullptr, tid);
        __syncthreads();
        if (bh + gridDim.x < nheads) prefetch(bh + gridDim.x);   // lands under phase A
        // ---------------- phase A: dQ ----------------
        bwd16_dq_phase(Ks, Vs, Kt, qf, dof, L, dl, wave < nq, qrow, l31, hi, dqkv, b, h);
        __syncthreads();   // every wave is done with this head's images before they are overwritten
    }
}

template <bool ROWPF>
static int launch_bwd_fused(const AttnBwdArgs& a, int out_ld, hipStream_t s) {
    constexpr auto kern = attn_bwd_fused_bf16_kernel<ROWPF>;
    const int grid = a.batch * NH;
    const size_t lds = 2 * ROW_IMG + 2 * TR_IMG + 2 * NPAD * sizeof(float);
    if (int rc = ensure_dyn_lds<kern>(lds)) return rc;
    hipLaunchKernelGGL(kern, dim3(min(grid, 256)), dim3(448), lds, s, (const bf16*)a.q, (const bf16*)a.k, (const bf16*)a.v, (const bf16*)a.out,
                       (const bf16*)a.dout, a.lse, a.delta, (bf16*)a.dqkv, grid, a.q_tiles, out_ld);
    DYT_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_attn_fwd_16(const AttnFwdArgs& a, hipStream_t s) {
    const int grid = a.batch * NH;
    hipLaunchKernelGGL(attn_fwd_bf16_kernel, dim3(min(grid, 256)), dim3(448), ROW_IMG + TR_IMG, s, (const bf16*)a.q, (const bf16*)a.k, (const bf16*)a.v,
                       (bf16*)a.out, a.lse, grid);
    DYT_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_attn_bwd_16(const AttnBwdArgs& a, const AttnBwdRoute& r, int out_ld, hipStream_t s) {
    if (r.kernel == AB_16_FUSED) return launch_bwd_fused<false>(a, out_ld, s);
    if (r.kernel == AB_16_FUSED_AHEAD) return launch_bwd_fused<true>(a, out_ld, s);
    // AB_16_TWO
    const int grid = a.batch * NH;
    const size_t lds1 = 2 * ROW_IMG + TR_IMG, lds2 = 2 * ROW_IMG + 2 * TR_IMG + 2 * NPAD * sizeof(float);
    if (int rc = ensure_dyn_lds<attn_bwd_dq_bf16_kernel>(lds1)) return rc;
    if (int rc = ensure_dyn_lds<attn_bwd_dkv_bf16_kernel>(lds2)) return rc;
    hipLaunchKernelGGL(attn_bwd_dq_bf16_kernel, dim3(min(grid, 256)), dim3(448), lds1, s, (const bf16*)a.q, (const bf16*)a.k, (const bf16*)a.v,
                       (const bf16*)a.out, (const bf16*)a.dout, a.lse, a.delta, (bf16*)a.dqkv, grid, out_ld);
    hipLaunchKernelGGL(attn_bwd_dkv_bf16_kernel, dim3(min(grid, 256)), dim3(448), lds2, s, (const bf16*)a.q, (const bf16*)a.k, (const bf16*)a.v,
                       (const bf16*)a.dout, a.lse, a.delta, (bf16*)a.dqkv, grid);
    DYT_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace dyt
