// Measurement hooks of the backward pass (checksums, stream isolation, poison: CK / ISO / POISON of ctx.h) and the dyt_debug_*
// accessors of a saved pass.
#include "ctx.h"

// Measurement hook (tools/probes/determinism_trace.py): DYT_DBG_CKSUM=1 -> after every backward launch an order-independent
// integer checksum of its output buffer is taken on the same stream into a per-pass log; two runs of the same step are then
// compared launch by launch: the first differing entry names the kernel whose output is not reproducible.
__global__ void dbg_checksum_kernel(const uint32_t* __restrict__ p, size_t nwords, unsigned long long* __restrict__ out) {
    unsigned long long acc = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nwords; i += (size_t)gridDim.x * 256)
        acc += (unsigned long long)p[i] * (unsigned long long)((i & 0xffff) + 1);
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(out, acc);
}
struct DbgCk { unsigned long long* dev = nullptr; int n[2] = {0, 0}; int on = -1; std::vector<std::string> label[2];
               void* dump = nullptr; size_t dump_bytes = 0, dump_len = 0; };
static DbgCk g_ck;
constexpr int DBG_CK_MAX = 1024;
bool dyt::dbg_ck_on() {
    if (g_ck.on < 0) { const char* e = getenv("DYT_DBG_CKSUM"); g_ck.on = e && atoi(e) ? 1 : 0; }
    return g_ck.on == 1;
}
int dyt::dbg_ck_reset(hipStream_t s) {
    if (!dbg_ck_on()) return 0;
    if (!g_ck.dev) DYT_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&g_ck.dev), 2 * DBG_CK_MAX * sizeof(unsigned long long)));
    DYT_HIP_CHECK(hipMemsetAsync(g_ck.dev, 0, 2 * DBG_CK_MAX * sizeof(unsigned long long), s));
    for (int i = 0; i < 2; ++i) { g_ck.n[i] = 0; g_ck.label[i].clear(); }
    return 0;
}
int dyt::dbg_ck(int slot, hipStream_t s, const char* what, int layer, const void* p, size_t bytes) {
    if (!dbg_ck_on() || !p || slot > 1 || g_ck.n[slot] >= DBG_CK_MAX) return 0;
    char buf[64];
    snprintf(buf, sizeof(buf), "L%d %s", layer, what);
    static const char* only = getenv("DYT_DBG_CKSUM_ONLY");   // comma-separated substrings: trace only the matching launches
    if (only && only[0]) {
        bool hit = false;
        std::string pats(only);
        for (size_t a = 0; a <= pats.size();) {
            const size_t e = pats.find(',', a) == std::string::npos ? pats.size() : pats.find(',', a);
            if (e > a && strstr(buf, pats.substr(a, e - a).c_str())) hit = true;
            a = e + 1;
        }
        if (!hit) return 0;
    }
    g_ck.label[slot].push_back(buf);
    static const char* dump = getenv("DYT_DBG_DUMP");   // "<slot>:<label>": keep a copy of that launch's output buffer
    if (dump && dump[0] && dump[1] == ':' && dump[0] - '0' == slot && !strcmp(dump + 2, buf)) {
        if (g_ck.dump_bytes < bytes) {
            if (g_ck.dump) (void)hipFree(g_ck.dump);
            DYT_HIP_CHECK(hipMalloc(&g_ck.dump, bytes));
            g_ck.dump_bytes = bytes;
        }
        DYT_HIP_CHECK(hipMemcpyAsync(g_ck.dump, p, bytes, hipMemcpyDeviceToDevice, s));
        g_ck.dump_len = bytes;
    }
    hipLaunchKernelGGL(dbg_checksum_kernel, dim3(128), dim3(256), 0, s, static_cast<const uint32_t*>(p), bytes / 4,
                       g_ck.dev + slot * DBG_CK_MAX + g_ck.n[slot]++);
    DYT_HIP_CHECK(hipGetLastError());
    return 0;
}
extern "C" int dyt_debug_checksums(int slot, uint64_t* out, int max_n, int* n_out) {
    if (!out || !n_out || slot < 0 || slot > 1) { set_error("bad argument"); return DYT_ERR_ARG; }
    *n_out = 0;
    if (!g_ck.dev) return DYT_OK;
    DYT_HIP_CHECK(hipDeviceSynchronize());
    const int n = g_ck.n[slot] < max_n ? g_ck.n[slot] : max_n;
    DYT_HIP_CHECK(hipMemcpy(out, g_ck.dev + slot * DBG_CK_MAX, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    *n_out = n;
    return DYT_OK;
}
extern "C" int64_t dyt_debug_dump_read(void* dst_device, int64_t max_bytes) {   // -> bytes copied (device to device)
    if (!g_ck.dump || !dst_device) return 0;
    const size_t n = g_ck.dump_len < (size_t)max_bytes ? g_ck.dump_len : (size_t)max_bytes;
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(dst_device, g_ck.dump, n, hipMemcpyDeviceToDevice) != hipSuccess) return -1;
    return (int64_t)n;
}
extern "C" const char* dyt_debug_checksum_label(int slot, int i) {
    if (slot < 0 || slot > 1 || i < 0 || i >= (int)g_ck.label[slot].size()) return "";
    return g_ck.label[slot][i].c_str();
}

// Measurement hook (tools/probes/determinism_cumask.py, PMASK=iso): DYT_DBG_ISO = bit mask of backward kernel classes that are
// launched on a per-pass stream pinned to ONE shader engine of every XCD (mask bits 24..31 of each word), fork/joined with
// events around every launch; the probe pins the two pass streams to the other three engines.  Finds which kernel class
// must share CUs with the other pass for the run-to-run differences of DESIGN.md 7b to appear.
//   1 attention bwd   2 tok_bwd (+ its reduce)   4 ln_bwd   8 frozen-weight dgrad GEMMs   16 adapter dgrad GEMMs   32 wgrad   64 prep / head
struct DbgIso { hipStream_t st[4] = {}; hipEvent_t a[4] = {}, b[4] = {}; int mask = -1; };
static DbgIso g_iso;
static int dbg_iso_mask() {
    if (g_iso.mask < 0) { const char* e = getenv("DYT_DBG_ISO"); g_iso.mask = e ? atoi(e) : 0; }
    return g_iso.mask;
}
int dyt::dbg_iso_enter(int slot, int cls, hipStream_t* s, hipStream_t* keep) {
    *keep = *s;
    if (!(dbg_iso_mask() & cls)) return 0;
    if (!g_iso.st[slot]) {
        uint32_t words[8];
        for (int i = 0; i < 8; ++i) words[i] = 0xFF000000u;
        DYT_HIP_CHECK(hipExtStreamCreateWithCUMask(&g_iso.st[slot], 8, words));
        DYT_HIP_CHECK(hipEventCreateWithFlags(&g_iso.a[slot], hipEventDisableTiming));
        DYT_HIP_CHECK(hipEventCreateWithFlags(&g_iso.b[slot], hipEventDisableTiming));
    }
    DYT_HIP_CHECK(hipEventRecord(g_iso.a[slot], *s));
    DYT_HIP_CHECK(hipStreamWaitEvent(g_iso.st[slot], g_iso.a[slot], 0));
    *s = g_iso.st[slot];
    return 0;
}
int dyt::dbg_iso_leave(int slot, hipStream_t* s, hipStream_t keep) {
    if (*s == keep) return 0;
    DYT_HIP_CHECK(hipEventRecord(g_iso.b[slot], *s));
    *s = keep;
    DYT_HIP_CHECK(hipStreamWaitEvent(*s, g_iso.b[slot], 0));
    return 0;
}

// Measurement hook: DYT_DBG_POISON = bit mask of backward transients that are filled with NaN bit patterns (0xFF bytes) on the
// stream right before the kernel that produces them.  A consumer that reads a row before its producer's store is visible then
// turns the final gradient into NaN instead of a 1e-6 difference.   1 dxn  2 dA2  4 dad  8 du_at  16 dO  32 dqkv  64 ddz  128 dZ  256 g_at
int dyt::dbg_poison(int bit, void* p, size_t bytes, hipStream_t s) {
#ifndef DYT_DEBUG_HOOKS
    (void)bit; (void)p; (void)bytes; (void)s;
    return 0;   // measurement builds only (-DDYT_DEBUG_HOOKS)
#endif
    static int mask = -1;
    if (mask < 0) { const char* e = getenv("DYT_DBG_POISON"); mask = e ? atoi(e) : 0; }
    if (!(mask & bit) || !p) return 0;
    DYT_HIP_CHECK(hipMemsetAsync(p, 0xFF, bytes, s));
    return 0;
}

extern "C" int dyt_debug_dispatch(dyt_ctx* c, int slot, int layer, int32_t* row_src, int32_t* dst_of, int32_t* counts,
                                  int32_t* total, void* stream) {
    if (!c || slot < 0 || slot >= c->cfg.slots || layer < 0 || layer >= c->cfg.depth) { set_error("bad slot / layer"); return DYT_ERR_ARG; }
    { int rc = refuse_inference(c, "dyt_debug_dispatch (per-block index arrays of a pass)"); if (rc) return rc; }
    const Slot& S = c->slots[slot];
    if (S.batch < 1) { set_error("slot %d holds no pass", slot); return DYT_ERR_STATE; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t M = (size_t)S.batch * NT;
    const LayerS& L = S.L[layer];
    if (row_src) DYT_HIP_CHECK(hipMemcpyAsync(row_src, L.row_src, M * 4, hipMemcpyDeviceToDevice, s));
    if (dst_of) DYT_HIP_CHECK(hipMemcpyAsync(dst_of, L.dst_of, M * 4, hipMemcpyDeviceToDevice, s));
    if (counts) DYT_HIP_CHECK(hipMemcpyAsync(counts, S.counts + (size_t)layer * S.batch, (size_t)S.batch * 4, hipMemcpyDeviceToDevice, s));
    if (total) DYT_HIP_CHECK(hipMemcpyAsync(total, L.total, 4, hipMemcpyDeviceToDevice, s));
    return DYT_OK;
}

extern "C" int dyt_debug_drop_path(dyt_ctx* c, int slot, float* out, void* stream) {
    if (!c || !out || slot < 0 || slot >= c->cfg.slots) { set_error("bad slot"); return DYT_ERR_ARG; }
    { int rc = refuse_inference(c, "dyt_debug_drop_path"); if (rc) return rc; }
    const Slot& S = c->slots[slot];
    if (S.batch < 1 || !S.dp) { set_error("slot %d: the last pass ran without stochastic depth", slot); return DYT_ERR_STATE; }
    DYT_HIP_CHECK(hipMemcpyAsync(out, S.dp, (size_t)2 * c->cfg.depth * S.batch * sizeof(float), hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
    return DYT_OK;
}
