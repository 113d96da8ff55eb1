// CPU walk of the wide head's index arithmetic (dynamic-tuning_amd/csrc/head_wide_idx.h) -- run BEFORE the kernels see a GPU.
//
// For every test shape it plays the three MFMA kernels of head_wide.hip lane by lane on the host, with the kernels' own index
// functions and exactly-sized heap buffers:
//   * every global index is asserted to lie in its tensor ([0,B) x [0,C), [0,C) x [0,768), [0,B) x [0,768)) and every 16-byte
//     access to be 16-byte aligned; every LDS index to lie in its image, and a stage's writes to cover the image exactly once;
//   * every output element is asserted to be written exactly once;
//   * the lane -> operand -> result mapping of v_mfma_f32_32x32x2_f32 is emulated, and the results are compared with a plain
//     triple loop in double, so a wrong k pairing or a transposed tile shows here and not on the device.
// It checks indices and the tile mapping, not the summation structure: a class slice of dx is summed here as one chain, where the kernel
// restarts its accumulator every 256 classes (DX_CHAIN_STAGES).
// Build and run (host only; the sanitizers catch what the asserts do not):
//   c++ -std=c++17 -O2 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I dynamic-tuning_amd/csrc \
//       tools/head_wide_index_check.cpp -o /tmp/head_wide_index_check && /tmp/head_wide_index_check
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "head_wide_idx.h"

using namespace dyt::hw;

#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed (B=%d C=%d)\n", __FILE__, __LINE__, #cond, gB, gC); abort(); } \
    } while (0)
static int gB, gC;

static float rnd() { return (float)((rand() % 2001) - 1000) * 1e-3f; }

// one v_mfma_f32_32x32x2_f32 of a wave: a = first operand (row of the 32 x 2 matrix on the lane), b = second (column of the 2 x 32)
static void mfma(const float a[64], const float b[64], float acc[64][16]) {
    for (int l = 0; l < 64; ++l)
        for (int r = 0; r < 16; ++r) {
            const int i = 8 * (r >> 2) + 4 * (l >> 5) + (r & 3), j = l & 31;
            float c = acc[l][r];
            for (int k = 0; k < 2; ++k) c = fmaf(a[i + 32 * k], b[j + 32 * k], c);
            acc[l][r] = c;
        }
}

struct Lds {
    std::vector<float> v; std::vector<int> w;
    explicit Lds(int n) : v(n), w(n) {}
    void begin() { std::fill(w.begin(), w.end(), 0); }
    void put(int off, float x, int lo, int hi) { CHECK(off >= lo && off < hi); v[off] = x; ++w[off]; }
    float get(int off, int lo, int hi) const { CHECK(off >= lo && off < hi); return v[off]; }
};

static void close_enough(double got, double want, double scale) { CHECK(std::fabs(got - want) <= 1e-4 * scale + 1e-6); }

static void check_logits(int B, int C) {
    std::vector<float> A((size_t)B * HD768), W((size_t)C * HD768), bias(C), out((size_t)B * C, 0.f);
    std::vector<int> writes((size_t)B * C, 0);
    for (auto& x : A) x = rnd();
    for (auto& x : W) x = rnd();
    for (auto& x : bias) x = rnd();
    Lds lds(LG_LDS_FLOATS);
    for (int by = 0; by < ceil_div(B, BM); ++by)
        for (int bx = 0; bx < ceil_div(C, BN); ++bx) {
            const int m0 = by * BM, n0 = bx * BN;
            static float acc[4][2][64][16];
            for (auto& w : acc) for (auto& i : w) for (auto& l : i) for (auto& r : l) r = 0.f;
            for (int kt = 0; kt < HD768 / BK; ++kt) {
                lds.begin();
                for (int tid = 0; tid < THREADS; ++tid) {
                    for (int t = 0; t < LG_A_PER_THREAD; ++t) {
                        const Src s = lg_stage(tid, t, kt, m0, B, 0);
                        CHECK(s.off >= 0 && s.off + 3 < (long long)B * HD768 && s.off % 4 == 0 && s.lds % 4 == 0);
                        for (int e = 0; e < 4; ++e) lds.put(s.lds + e, A.data()[s.off + e], 0, LG_A_FLOATS);
                    }
                    for (int t = 0; t < LG_W_PER_THREAD; ++t) {
                        const Src s = lg_stage(tid, t, kt, n0, C, LG_A_FLOATS);
                        CHECK(s.off >= 0 && s.off + 3 < (long long)C * HD768 && s.off % 4 == 0 && s.lds % 4 == 0);
                        for (int e = 0; e < 4; ++e) lds.put(s.lds + e, W.data()[s.off + e], LG_A_FLOATS, LG_LDS_FLOATS);
                    }
                }
                for (int x : lds.w) CHECK(x == 1);
                for (int wave = 0; wave < 4; ++wave)
                    for (int j = 0; j < 4; ++j) {
                        float w[4][64], a0[4][64], a1[4][64];
                        for (int lane = 0; lane < 64; ++lane) {
                            const int ow = lg_frag(LG_A_FLOATS, wave * 32 + (lane & 31), lane, j);
                            const int o0 = lg_frag(0, lane & 31, lane, j), o1 = lg_frag(0, 32 + (lane & 31), lane, j);
                            CHECK(ow % 4 == 0 && o0 % 4 == 0 && o1 % 4 == 0);
                            for (int t = 0; t < 4; ++t) {
                                w[t][lane] = lds.get(ow + t, LG_A_FLOATS, LG_LDS_FLOATS);
                                a0[t][lane] = lds.get(o0 + t, 0, LG_A_FLOATS);
                                a1[t][lane] = lds.get(o1 + t, 0, LG_A_FLOATS);
                            }
                        }
                        for (int t = 0; t < 4; ++t) { mfma(w[t], a0[t], acc[wave][0]); mfma(w[t], a1[t], acc[wave][1]); }
                    }
            }
            for (int wave = 0; wave < 4; ++wave)
                for (int lane = 0; lane < 64; ++lane)
                    for (int i = 0; i < 2; ++i)
                        for (int g = 0; g < 4; ++g) {
                            const Out o = lg_out(m0, n0, wave, lane, i, g, B, C);
                            const int n = n0 + acc_col(wave, lane, g);
                            CHECK(o.nvalid >= 0 && o.nvalid <= 4);
                            if (o.vec) CHECK(o.nvalid == 4 && o.off % 4 == 0 && n % 4 == 0);
                            for (int e = 0; e < o.nvalid; ++e) {
                                CHECK(o.off + e >= 0 && o.off + e < (long long)B * C && n + e < C);
                                out.data()[o.off + e] = acc[wave][i][lane][4 * g + e] + bias.data()[n + e];
                                ++writes[o.off + e];
                            }
                        }
        }
    for (int x : writes) CHECK(x == 1);
    for (int b = 0; b < B; ++b)
        for (int c = 0; c < C; c += (C > 300 ? 37 : 1)) {
            double r = bias[c];
            for (int k = 0; k < HD768; ++k) r += (double)A[(size_t)b * HD768 + k] * W[(size_t)c * HD768 + k];
            close_enough(out[(size_t)b * C + c], r, 30.0);
        }
}

static void check_dx(int B, int C) {
    const int ns = n_slices(C);
    std::vector<float> dl((size_t)B * C), W((size_t)C * HD768), part((size_t)ns * B * HD768, 0.f);
    std::vector<int> writes(part.size(), 0);
    for (auto& x : dl) x = rnd();
    for (auto& x : W) x = rnd();
    Lds lds(DX_LDS_FLOATS);
    for (int s = 0; s < ns; ++s) {
        CHECK(slice_end(s, C) > slice_begin(s) && slice_end(s, C) - slice_begin(s) <= SLICE && slice_end(s, C) <= C);
        for (int by = 0; by < ceil_div(B, BM); ++by)
            for (int bx = 0; bx < HD768 / BN; ++bx) {
                const int m0 = by * BM, n0 = bx * BN;
                static float acc[4][2][64][16];
                for (auto& w : acc) for (auto& i : w) for (auto& l : i) for (auto& r : l) r = 0.f;
                for (int kt = 0; kt < slice_stages(s, C); ++kt) {
                    lds.begin();
                    for (int tid = 0; tid < THREADS; ++tid) {
                        for (int t = 0; t < DX_A_PER_THREAD; ++t) {
                            const Src r = dx_stage_a(tid, t, kt, m0, s, B, C);
                            if (r.valid) CHECK(r.off >= 0 && r.off < (long long)B * C);
                            lds.put(r.lds, r.valid ? dl.data()[r.off] : 0.f, 0, DX_A_FLOATS);
                        }
                        for (int t = 0; t < DX_W_PER_THREAD; ++t) {
                            const Src r = dx_stage_w(tid, t, kt, n0, s, C);
                            if (r.valid) CHECK(r.off >= 0 && r.off + 3 < (long long)C * HD768 && r.off % 4 == 0);
                            CHECK(r.lds % 4 == 0);
                            for (int e = 0; e < 4; ++e) lds.put(r.lds + e, r.valid ? W.data()[r.off + e] : 0.f, DX_A_FLOATS, DX_LDS_FLOATS);
                        }
                    }
                    for (int off = 0; off < DX_LDS_FLOATS; ++off) {   // the A image's pad column (row stride 33) and the W image's 32 pad floats stay unwritten
                        const bool used = off < DX_A_FLOATS ? (off % DX_A_LD) < BK : ((off - DX_A_FLOATS) % DX_W_LD) < BN;
                        CHECK(lds.w[off] == (used ? 1 : 0));
                    }
                    for (int wave = 0; wave < 4; ++wave)
                        for (int kp = 0; kp < BK / 2; ++kp) {
                            float w[64], a0[64], a1[64];
                            for (int lane = 0; lane < 64; ++lane) {
                                const int ow = dx_frag_w(wave, lane, kp), o0 = dx_frag_a(0, lane, kp), o1 = dx_frag_a(1, lane, kp);
                                CHECK(lds.w[ow] == 1 && lds.w[o0] == 1 && lds.w[o1] == 1);
                                w[lane] = lds.get(ow, DX_A_FLOATS, DX_LDS_FLOATS);
                                a0[lane] = lds.get(o0, 0, DX_A_FLOATS);
                                a1[lane] = lds.get(o1, 0, DX_A_FLOATS);
                            }
                            mfma(w, a0, acc[wave][0]);
                            mfma(w, a1, acc[wave][1]);
                        }
                }
                for (int wave = 0; wave < 4; ++wave)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int i = 0; i < 2; ++i)
                            for (int g = 0; g < 4; ++g) {
                                const Out o = dx_out(m0, n0, s, wave, lane, i, g, B);
                                if (o.nvalid == 0) continue;
                                CHECK(o.vec && o.nvalid == 4 && o.off % 4 == 0 && o.off >= 0 && o.off + 3 < (long long)part.size());
                                for (int e = 0; e < 4; ++e) { part.data()[o.off + e] = acc[wave][i][lane][4 * g + e]; ++writes[o.off + e]; }
                            }
            }
    }
    for (int x : writes) CHECK(x == 1);
    for (int b = 0; b < B; ++b)
        for (int ch = 0; ch < HD768; ch += 7) {
            double r = 0, got = 0;
            for (int c = 0; c < C; ++c) r += (double)dl[(size_t)b * C + c] * W[(size_t)c * HD768 + ch];
            for (int s = 0; s < ns; ++s) got += part[((size_t)s * B + b) * HD768 + ch];
            close_enough(got, r, std::sqrt((double)C) + 1.0);
        }
}

static void check_dw(int B, int C) {
    std::vector<float> dl((size_t)B * C), X((size_t)B * HD768), dW((size_t)C * HD768), db(C), dW0, db0;
    std::vector<int> writes(dW.size(), 0), bwrites(C, 0);
    for (auto& x : dl) x = rnd();
    for (auto& x : X) x = rnd();
    for (auto& x : dW) x = rnd();
    for (auto& x : db) x = rnd();
    dW0 = dW; db0 = db;
    Lds lds(DW_LDS_FLOATS);
    for (int by = 0; by < ceil_div(C, BM); ++by)
        for (int bx = 0; bx < HD768 / BN; ++bx) {
            const int c0 = by * BM, n0 = bx * BN;
            static float acc[4][2][64][16];
            for (auto& w : acc) for (auto& i : w) for (auto& l : i) for (auto& r : l) r = 0.f;
            float sb[BM] = {0};
            for (int kt = 0; kt < dw_stages(B); ++kt) {
                lds.begin();
                for (int tid = 0; tid < THREADS; ++tid) {
                    for (int t = 0; t < DW_A_PER_THREAD; ++t) {
                        const Src r = dw_stage_a(tid, t, kt, c0, B, C);
                        if (r.valid) CHECK(r.off >= 0 && r.off < (long long)B * C);
                        lds.put(r.lds, r.valid ? dl.data()[r.off] : 0.f, 0, DW_A_FLOATS);
                    }
                    for (int t = 0; t < DW_X_PER_THREAD; ++t) {
                        const Src r = dw_stage_x(tid, t, kt, n0, B);
                        if (r.valid) CHECK(r.off >= 0 && r.off + 3 < (long long)B * HD768 && r.off % 4 == 0);
                        CHECK(r.lds % 4 == 0);
                        for (int e = 0; e < 4; ++e) lds.put(r.lds + e, r.valid ? X.data()[r.off + e] : 0.f, DW_A_FLOATS, DW_LDS_FLOATS);
                    }
                }
                for (int off = 0; off < DW_LDS_FLOATS; ++off) {
                    const bool used = off < DW_A_FLOATS ? (off % DW_A_LD) < BM : ((off - DW_A_FLOATS) % DW_X_LD) < BN;
                    CHECK(lds.w[off] == (used ? 1 : 0));
                }
                for (int wave = 0; wave < 4; ++wave)
                    for (int kp = 0; kp < BK / 2; ++kp) {
                        float w[64], a0[64], a1[64];
                        for (int lane = 0; lane < 64; ++lane) {
                            const int ow = dw_frag_x(wave, lane, kp), o0 = dw_frag_a(0, lane, kp), o1 = dw_frag_a(1, lane, kp);
                            CHECK(lds.w[ow] == 1 && lds.w[o0] == 1 && lds.w[o1] == 1);
                            w[lane] = lds.get(ow, DW_A_FLOATS, DW_LDS_FLOATS);
                            a0[lane] = lds.get(o0, 0, DW_A_FLOATS);
                            a1[lane] = lds.get(o1, 0, DW_A_FLOATS);
                        }
                        mfma(w, a0, acc[wave][0]);
                        mfma(w, a1, acc[wave][1]);
                    }
                if (bx == 0)
                    for (int tid = 0; tid < BM; ++tid)
                        for (int k = 0; k < BK; ++k) { const int o = dw_db_lds(tid, k); CHECK(lds.w[o] == 1); sb[tid] += lds.get(o, 0, DW_A_FLOATS); }
            }
            for (int wave = 0; wave < 4; ++wave)
                for (int lane = 0; lane < 64; ++lane)
                    for (int i = 0; i < 2; ++i)
                        for (int g = 0; g < 4; ++g) {
                            const Out o = dw_out(c0, n0, wave, lane, i, g, C);
                            if (o.nvalid == 0) continue;
                            CHECK(o.vec && o.off % 4 == 0 && o.off >= 0 && o.off + 3 < (long long)dW.size());
                            for (int e = 0; e < 4; ++e) { dW.data()[o.off + e] += acc[wave][i][lane][4 * g + e]; ++writes[o.off + e]; }
                        }
            if (bx == 0)
                for (int tid = 0; tid < BM; ++tid)
                    if (c0 + tid < C) { db.data()[c0 + tid] += sb[tid]; ++bwrites[c0 + tid]; }
        }
    for (int x : writes) CHECK(x == 1);
    for (int x : bwrites) CHECK(x == 1);
    for (int c = 0; c < C; c += (C > 300 ? 41 : 1)) {
        double rb = db0[c];
        for (int b = 0; b < B; ++b) rb += dl[(size_t)b * C + c];
        close_enough(db[c], rb, std::sqrt((double)B) + 1.0);
        for (int ch = 0; ch < HD768; ch += 5) {
            double r = dW0[(size_t)c * HD768 + ch];
            for (int b = 0; b < B; ++b) r += (double)dl[(size_t)b * C + c] * X[(size_t)b * HD768 + ch];
            close_enough(dW[(size_t)c * HD768 + ch], r, std::sqrt((double)B) + 1.0);
        }
    }
}

int main() {
    // the shapes of tests/test_gpu_wide_head.py (unit entry and context path) and the measured B = 128 forms
    static const int Cs[] = {1, 63, 64, 65, 129, 1023, 1024, 1025, 2049, 4099}, Bs[] = {1, 3, 31, 33, 129};
    std::vector<std::pair<int, int>> shapes;
    for (int C : Cs) { shapes.push_back({1, C}); shapes.push_back({33, C}); }
    for (int B : Bs) for (int C : {65, 1025, 2049}) shapes.push_back({B, C});
    for (auto bc : {std::pair<int, int>{2, 21843}, {3, 5}, {17, 5}, {3, 1000}, {17, 1000}, {2, 1100}, {3, 1100}, {4, 1100}, {5, 1100},
                    {128, 1000}, {64, 127}, {65, 128}})
        shapes.push_back(bc);
    for (auto bc : shapes) {
        gB = bc.first; gC = bc.second;
        check_logits(gB, gC);
        check_dx(gB, gC);
        check_dw(gB, gC);
        printf("B=%-4d C=%-6d ok (%d slices)\n", gB, gC, n_slices(gC));
        fflush(stdout);
    }
    printf("head_wide index check: %zu shapes ok\n", shapes.size());
    return 0;
}
