// CPU walk of the GEMM tile routing (dynamic-tuning_amd/csrc/gemm_route.h) -- which kernel family and which rows a GEMM gets, checked
// without a GPU.
//
// No arguments:
//   * the hand-derived routes and workgroup counts of the shapes at the routing's thresholds (256 CUs; M = 2048, the 192-workgroup partial
//     round of 256x256 tiles, a one-row tail, with and without a pre-shuffled weight, store and residual epilogues);
//   * for every M in 1..26000, N in {768, 2304, 3072}, K in {64, 768, 2304, 3072}, over the operand forms: the 256x256 body and the
//     128x128 tail together cover every row exactly once, the body is a multiple of 256, and a device-side row count never changes the route.
// `--table`: reads one GEMM per line from stdin -- family M N K cat lead wp store_epi a_map a_ld a_fold m_dev a2 w2 splitk_fits f8_begin --
// and prints "kernel body" for each: tests/test_gemm_route_host.py feeds it tests/golden/gemm_routes.json.
// Build and run (host only):
//   c++ -std=c++17 -O2 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I dynamic-tuning_amd/csrc
//     tools/gemm_route_check.cpp -o /tmp/gemm_route_check && /tmp/gemm_route_check
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "gemm_route.h"

using namespace dyt;

static GemmShape gS;
#define CHECK(cond)                                                                                                          \
    do {                                                                                                                     \
        if (!(cond)) {                                                                                                       \
            fprintf(stderr, "%s:%d: CHECK(%s) failed (family=%d M=%d N=%d K=%d cat=%d lead=%d wp=%d store=%d a_map=%d a_ld=%d m_dev=%d)\n", __FILE__, __LINE__, \
                    #cond, (int)gS.family, gS.M, gS.N, gS.K, gS.cat, gS.lead, gS.wp, gS.store_epi, gS.a_map, gS.a_ld, gS.m_dev);     \
            abort();                                                                                                         \
        }                                                                                                                    \
    } while (0)

static const char* const NAMES[] = {"error", "splitk", "bpre", "256x256", "128x128", "128x64", "f32_128x128", "f32_128x64"};

// workgroups of the launch on rows [0, body) and of the 128x128 tail launch on rows [body, M)
struct Grids { int head, tail; };
static Grids grids(const GemmShape& g, const GemmRoute& r) {
    switch (r.kernel) {
        case GK_BPRE: return {tile_grid(0, r.body, g.N, 128, 256), 0};
        case GK_256: return {tile_grid(0, r.body, g.N, 256, 256), tile_grid(r.body, g.M, g.N, 128, 128)};
        case GK_128: case GK_F32_128: return {tile_grid(0, r.body, g.N, 128, 128), 0};
        case GK_128x64: case GK_F32_128x64: return {tile_grid(0, r.body, g.N, 128, 64), 0};
        default: return {0, 0};
    }
}

static GemmShape shape(int M, int N, int K, bool wp = false, bool store_epi = false) {
    GemmShape g;
    g.M = M; g.N = N; g.K = K; g.wp = wp; g.store_epi = store_epi;
    return g;
}

static void expect(const GemmShape& g, GemmKernel kernel, int body, int head, int tail) {
    gS = g;
    const GemmRoute r = gemm_route(g);
    const Grids w = grids(g, r);
    CHECK(r.kernel == kernel);
    CHECK(r.body == body);
    CHECK(w.head == head && w.tail == tail);
    CHECK((r.kernel == GK_ERROR) == (r.error != nullptr));
}

static void hand_derived() {
    // B = 128: M = 128 x 197 = 25216.  t256 = ceil(M / 256) x (N / 256) tiles of 256x256, a round = 256 of them
    expect(shape(25216, 2304, 768, true), GK_BPRE, 25216, 197 * 9, 0);            // qkv forward
    expect(shape(25216, 768, 768, true, true), GK_BPRE, 25216, 197 * 3, 0);       // proj dgrad: plain store, K <= 3072
    expect(shape(25216, 768, 768, true, false), GK_128, 25216, 1182, 0);          // proj forward: residual epilogue, K <= 768
    expect(shape(25216, 768, 3072), GK_256, 21760, 255, 162);                     // 297 tiles = 1 round + 41: body 85 x 256 rows, tail 27 x 6
    expect(shape(16129, 768, 3072), GK_256, 16129, 192, 0);                       // 64 x 3 = 192 = 3/4 of a round: one launch
    expect(shape(16128, 768, 3072), GK_128, 16128, 756, 0);                       // 63 x 3 = 189 < 192: no 256x256 tiles
    expect(shape(21761, 768, 3072), GK_256, 21760, 255, 6);                       // 86 x 3 = 258 = 1 round + 2: a one-row tail
    expect(shape(2047, 2304, 768, true), GK_128, 2047, 288, 0);                   // M < 2048, 72 tiles < 192
    expect(shape(2048, 2304, 768, true), GK_BPRE, 2048, 16 * 9, 0);
    expect(shape(2048, 2304, 768, false), GK_256, 2048, 8 * 9, 0);
    expect(shape(25216, 192, 768), GK_128x64, 25216, 197 * 3, 0);
    expect(shape(25216, 100, 768), GK_ERROR, 0, 0, 0);
}

static void structural() {
    static const int Ns[] = {768, 2304, 3072}, Ks[] = {64, 768, 2304, 3072};
    long long n = 0;
    for (int form = 0; form < 7; ++form)
        for (int N : Ns)
            for (int K : Ks)
                for (int M = 1; M <= 26000; ++M) {
                    GemmShape g = shape(M, N, K, form == 1 || form == 2, form == 2);
                    if (form == 3) { g.cat = true; g.a2 = g.w2 = true; }
                    if (form == 4) { g.lead = true; g.a2 = g.w2 = true; g.a_fold = g.a_ld = true; }
                    if (form == 5) { g.a_ld = true; }   // a one-part split operand
                    if (form == 6) { g.family = GF_F8; g.K = 2 * K; g.f8_begin = K / 64; if (K % 128 != 0) continue; }
                    gS = g;
                    const GemmRoute r = gemm_route(g);
                    CHECK(r.kernel != GK_ERROR && r.kernel != GK_SPLITK && r.error == nullptr);
                    CHECK(r.body >= 0 && r.body <= M);
                    if (r.kernel == GK_256) CHECK(r.body == M || r.body % 256 == 0);
                    else CHECK(r.body == M);
                    // rows [0, body) in BM-row tiles of the head launch, rows [body, M) in 128-row tiles of the tail: the tiles' row ranges follow
                    // one another without gap or overlap from row 0 to row M
                    const int BM = r.kernel == GK_256 ? 256 : 128;
                    const Grids w = grids(g, r);
                    const int cols = N / (r.kernel == GK_128 ? 128 : 256);
                    CHECK(w.head % cols == 0 && w.tail % (N / 128) == 0);
                    int next = 0;
                    for (int t = 0; t < w.head / cols; ++t) { CHECK(t * BM == next && next < r.body); next = next + BM < r.body ? next + BM : r.body; }
                    CHECK(next == r.body);
                    for (int t = 0; t < w.tail / (N / 128); ++t) { CHECK(r.body + t * 128 == next && next < M); next = next + 128 < M ? next + 128 : M; }
                    CHECK(next == M);
                    GemmShape d = g; d.m_dev = true;   // a compacted launch: same route, the workgroups beyond the count exit early
                    const GemmRoute rd = gemm_route(d);
                    CHECK(rd.kernel == r.kernel && rd.body == r.body);
                    ++n;
                }
    printf("gemm route check: %lld shapes, every row covered once\n", n);
}

static int table() {
    int family, cat, lead, wp, store, a_map, a_ld, a_fold, m_dev, a2, w2, sk;
    GemmShape g;
    while (scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", &family, &g.M, &g.N, &g.K, &cat, &lead, &wp, &store, &a_map, &a_ld, &a_fold, &m_dev, &a2, &w2, &sk,
                 &g.f8_begin) == 16) {
        if (family < 0 || family > 2) return 2;
        g.family = (GemmFamily)family; g.cat = cat; g.lead = lead; g.wp = wp; g.store_epi = store; g.a_map = a_map; g.a_ld = a_ld; g.a_fold = a_fold;
        g.m_dev = m_dev; g.a2 = a2; g.w2 = w2; g.splitk_fits = sk;
        const GemmRoute r = gemm_route(g);
        printf("%s %d\n", NAMES[r.kernel], r.body);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "--table")) return table();
    hand_derived();
    printf("gemm route check: hand-derived routes ok\n");
    structural();
    return 0;
}
