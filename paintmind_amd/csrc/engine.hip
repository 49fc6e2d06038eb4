// Model-level orchestration: VQModel encode/decode (reference stage1/vqmodel.py:21-41), the
// stage-2 CondTransformer forward (stage2/transformer.py:80-93) and the MaskGIT sample/generate
// loop (generate.py:159-198), expressed as sequences of the operator-level launches of this
// library on one HIP stream.  No host synchronisation happens inside a forward pass.
#include <stdarg.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>

#include "common.h"

// ------------------------------------------------------------------------------------------------
// error + timing plumbing
// ------------------------------------------------------------------------------------------------
static thread_local std::string g_err;

void pm_set_error(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
}

extern "C" const char* pmhip_last_error(void) { return g_err.c_str(); }
extern "C" int pmhip_abi_version(void) { return PMHIP_ABI_VERSION; }

extern "C" int pmhip_device_info(int device, int* cu_count, int* lds_bytes, char* arch, int arch_len) {
    hipDeviceProp_t prop;
    PM_HIP(hipGetDeviceProperties(&prop, device));
    if (cu_count) *cu_count = prop.multiProcessorCount;
    if (lds_bytes) *lds_bytes = (int)prop.sharedMemPerBlock;
    if (arch && arch_len > 0) snprintf(arch, arch_len, "%s", prop.gcnArchName);
    return PMHIP_OK;
}

// Timing is a process-wide diagnostic that concurrent lanes (one host thread each, generate.py) may run into: the switch is
// atomic and the per-family accumulators are guarded by one mutex (taken only while timing is on).
std::atomic<bool> g_pm_timing_on{false};
namespace {
std::mutex g_fam_mu;
struct FamStat {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    int launches = 0;
    double ms = 0.0;
};
FamStat g_fam[FAM_COUNT];
const char* kFamNames[FAM_COUNT] = {"gemm_plain", "attention", "layernorm", "sample", "vq", "rowops", "gemm_heads", "gemm_swiglu", "gemm_resid",
                                    "gemm_resid2b"};
const int kGemmFams[5] = {FAM_GEMM, FAM_GEMM_HEADS, FAM_GEMM_SWIGLU, FAM_GEMM_RESID, FAM_GEMM_RESID2B};

void drain(FamStat& f) {
    for (auto& pr : f.pending) {
        float ms = 0.f;
        if (hipEventSynchronize(pr.second) == hipSuccess && hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) {
            f.ms += ms;
            f.launches += 1;
        }
        (void)hipEventDestroy(pr.first);
        (void)hipEventDestroy(pr.second);
    }
    f.pending.clear();
}
}  // namespace

PmTimer::PmTimer(int fam, hipStream_t s) : family(fam), stream(s), e0(nullptr), on(g_pm_timing_on.load(std::memory_order_relaxed)) {
    if (on) {
        if (hipEventCreate(&e0) != hipSuccess) { on = false; return; }
        (void)hipEventRecord(e0, stream);
    }
}
PmTimer::~PmTimer() {
    if (!on) return;
    hipEvent_t e1;
    if (hipEventCreate(&e1) != hipSuccess) return;
    (void)hipEventRecord(e1, stream);
    std::lock_guard<std::mutex> lk(g_fam_mu);
    g_fam[family].pending.emplace_back(e0, e1);
}

extern "C" int pmhip_timing_enable(int on) { g_pm_timing_on.store(on != 0); return PMHIP_OK; }
extern "C" int pmhip_timing_reset(void) {
    std::lock_guard<std::mutex> lk(g_fam_mu);
    for (auto& f : g_fam) { drain(f); f.launches = 0; f.ms = 0.0; }
    return PMHIP_OK;
}
extern "C" int pmhip_timing_get(const char* family, int* launches, double* total_ms) {
    if (family && std::string(family) == "gemm") {           // the whole GEMM family
        std::lock_guard<std::mutex> lk(g_fam_mu);
        int n = 0; double ms = 0.0;
        for (int i : kGemmFams) { drain(g_fam[i]); n += g_fam[i].launches; ms += g_fam[i].ms; }
        if (launches) *launches = n;
        if (total_ms) *total_ms = ms;
        return PMHIP_OK;
    }
    for (int i = 0; i < FAM_COUNT; ++i)
        if (family && std::string(family) == kFamNames[i]) {
            std::lock_guard<std::mutex> lk(g_fam_mu);
            drain(g_fam[i]);
            if (launches) *launches = g_fam[i].launches;
            if (total_ms) *total_ms = g_fam[i].ms;
            return PMHIP_OK;
        }
    pm_set_error("timing_get: unknown family '%s'", family ? family : "(null)");
    return PMHIP_EINVAL;
}

// ------------------------------------------------------------------------------------------------
// workspace: named device buffers that only ever grow (the library's only allocations)
// ------------------------------------------------------------------------------------------------
namespace {

struct Workspace {
    std::map<std::string, std::pair<void*, size_t>> bufs;
    bool frozen = false;   // set while a graph capture is in flight: growing would be a bug
    uint64_t gen = 0;      // bumped by every (re)allocation: a captured graph holds raw buffer pointers and is only
                           // valid for the generation it was captured at
    ~Workspace() {
        for (auto& kv : bufs)
            if (kv.second.first) (void)hipFree(kv.second.first);
    }
    int get(const char* name, size_t bytes, void** out, hipStream_t s) {
        auto& e = bufs[name];
        if (e.second < bytes) {
            if (frozen) { pm_set_error("workspace '%s' would grow during graph capture", name); return PMHIP_ESTATE; }
            if (e.first) {
                PM_HIP(hipStreamSynchronize(s));
                PM_HIP(hipFree(e.first));
                e.first = nullptr; e.second = 0;
            }
            const size_t want = (bytes + 255) & ~(size_t)255;
            hipError_t rc = hipMalloc(&e.first, want);
            if (rc != hipSuccess) {
                pm_set_error("hipMalloc(%zu bytes) for workspace '%s' failed: %s", want, name, hipGetErrorString(rc));
                e.first = nullptr;
                return PMHIP_ENOMEM;
            }
            e.second = want;
            ++gen;
        }
        *out = e.first;
        return PMHIP_OK;
    }
};

#define WS(ws, name, bytes, ptr) PM_TRY((ws).get(name, (size_t)(bytes), (void**)&(ptr), s))

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// Stream-ordered copy by a KERNEL (device memory, or pinned host memory through its device alias): the graph-replayed decode loop
// refreshes its per-call parameter block and ids with it, so that the refresh is a queue packet like the graph's own kernels.
// Measured (profiles/r05_c_host_polling.txt, tools/hwtests/graph_dispatch_mode.hip): this did NOT cure the mis-ordered replays
// seen under AMD_DIRECT_DISPATCH=0 -- graph replay itself is broken in that runtime mode on ROCm 7.2, which is why the loop runs
// eagerly there (generate_loop) -- it is kept because it costs nothing and keeps the replay path free of hipMemcpyAsync nodes.
// 16-byte words when size and both pointers allow it, 8-byte words otherwise (ids are int64: any B * tokens is a multiple of 8),
// hipMemcpyAsync for anything else.
template <typename W>
__global__ void copy_words_kernel(W* __restrict__ dst, const W* __restrict__ src, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
}
template <typename W>
int copy_words_async(void* dst, const void* src, size_t n, hipStream_t s) {
    const int blocks = (int)std::min<size_t>((n + 255) / 256, 1024);
    hipLaunchKernelGGL(copy_words_kernel<W>, dim3(blocks > 0 ? blocks : 1), dim3(256), 0, s, (W*)dst, (const W*)src, n);
    PM_HIP(hipGetLastError());
    return PMHIP_OK;
}
int copy16_async(void* dst, const void* src, size_t bytes, hipStream_t s) {
    if (bytes == 0) return PMHIP_OK;
    const uintptr_t bits = (uintptr_t)dst | (uintptr_t)src | (uintptr_t)bytes;
    if (bits % 16 == 0) return copy_words_async<uint4>(dst, src, bytes / 16, s);
    if (bits % 8 == 0) return copy_words_async<unsigned long long>(dst, src, bytes / 8, s);
    PM_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, s));
    return PMHIP_OK;
}
// ids[0 .. n) = value, stream-ordered (the all-mask start of a decode loop)
__global__ void fill_ids_kernel(int64_t* __restrict__ ids, int64_t value, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) ids[i] = value;
}
int fill_ids_async(int64_t* ids, int64_t value, size_t n, hipStream_t s) {
    const int blocks = (int)std::min<size_t>((n + 255) / 256, 1024);
    hipLaunchKernelGGL(fill_ids_kernel, dim3(blocks > 0 ? blocks : 1), dim3(256), 0, s, ids, value, n);
    PM_HIP(hipGetLastError());
    return PMHIP_OK;
}
constexpr float kLog2e = 1.4426950408889634f;

struct CrossKV {            // cached cross-attention K / V^T of a static context, per layer
    const void* k = nullptr;
    const void* vt = nullptr;
    int L = 0, Lp = 0;
    const int32_t* lens = nullptr;   // device [B]: per-image key counts of THIS call (NULL: every image attends to all L rows)
    // regional prompts, THIS call's or NULL: device uint8 [B, L], the segment of every context row (255 = padding),
    // and device uint32 [B, tokens], the segments every token attends to.  Never beside `lens`, except with `pick`.
    const uint8_t* key_seg = nullptr;
    const uint32_t* query_mask = nullptr;
    // a slots step with slots of several kinds side by side, THIS call's or NULL: device uint8 [B], the kind of
    // every image -- 0 = it runs under its length, 1 = under its key sets, 2 = under its key sets and its biases.  Only then `lens`
    // and the segments stand side by side: two picked launches, and a third when `key_bias` is there as well.
    const uint8_t* pick = nullptr;
    // prompt weights, THIS call's or NULL: device f32 [B, L], log(weight) of every context row in the score unit of
    // the handle's dtype (-inf = excluded).  Always beside key_seg / query_mask (the caller's or the neutral ones).  Beside `pick` (a
    // slots step with a weighted slot) the set carries lens, the segments, pick AND key_bias together, and only the
    // images of kind 2 read their rows of it.
    const float* key_bias = nullptr;
    // the maps tap (pmhip_s2_forward_maps only), THIS call's or NULL: device f32 [B, tokens, L].  A layer whose set carries
    // it issues one pmhip_attention_maps directly behind its cross-attention launch, with this scale, writing or accumulating.
    float* maps = nullptr;
    float maps_scale = 1.f;
    bool maps_accumulate = false;
    // cross-attention control (pmhip_s2_forward_control only), THIS call's or NULL: device int32 / f32 / f32 [B / 2, L].
    // The batch is B / 2 pairs, the source images in front; a layer whose set carries the arrays runs the ordinary launch on the
    // source half and pmhip_attention_control on the edited half.  ctl_self: the edited half's first self-attention of this layer
    // takes the source half's Q and K.
    const int32_t* ctl_map = nullptr;
    const float* ctl_blend = nullptr;
    const float* ctl_gain = nullptr;
    bool ctl_self = false;
    // the phrase-score tap (pmhip_s2_forward_control_scores only), THIS call's or NULL: the phrase's row weights of the
    // two halves, device f32 [B / 2, L] each, and the two halves of the score buffer, device f32 [B / 2, tokens] each.  A layer whose
    // set carries them issues one pmhip_attention_phrase_score directly behind its cross-attention launch -- under the layer's control
    // arrays where it has them --, with this scale, writing or accumulating.
    const float* phr_w_src = nullptr;
    const float* phr_w_edit = nullptr;
    float* phr_src = nullptr;
    float* phr_edit = nullptr;
    float phr_scale = 1.f;
    bool phr_accumulate = false;
};

// The bf16 hi/lo residual stream + folded LayerNorm is the DEFAULT of bf16 mode (PMHIP_HILO=0, read when a handle is created, restores
// the fp32 stream + LayerNorm kernel of rounds 1-2): 1.3 % faster on the default workload (same box: 476.5 vs 470.6 images/s),
// as accurate.  It was opt-in while 3-11 of 1800 generate() calls under concurrent lanes were not
// bit-identical; that was a gfx950 packed-FP32 operand-select hazard in the folded epilogue, fixed in
// gemm_common.h and gated by tests/test_isa_hazards.py.
// The PMHIP_* switches are read ONCE, when a handle is created (a handle's graphs, workspace and fold decisions all depend on
// them; a getenv on the hot path is also a data race with a caller that edits the environment from another thread).
struct Switches {
    int overlap_rows = 65536;   // PMHIP_DECODE_OVERLAP_MAX_ROWS: largest B * tokens whose decode loop defers each step's ViT decode
                                // to a side stream beside the next step's tower (0 = never)
    bool hilo = true;       // PMHIP_HILO=0: the fp32 stream + LayerNorm kernel of rounds 1-2
    bool fold = true;       // PMHIP_LN_UNFOLD=1: the hi/lo pair, but the separate LayerNorm kernel
    int fold_rows_cap = 0;  // PMHIP_FOLD_MAX_ROWS (development / tests): cap on the rows one folded launch takes, see fold_rows()
    bool center = true;     // PMHIP_HILO_CENTER=0: the residual producers do not centre the hi plane (A/B, tests)
    bool logits_stats = true;     // PMHIP_LOGITS_STATS=0 (development builds, profiles/r06_d): the logits GEMM leaves no block statistics, the sampling kernel derives
                                  // them from the rows it then has to read in full (same ids and scores, bit for bit)
    bool blocking_wait = false;   // PMHIP_BLOCKING_WAIT=1: host waits between decode-loop segments sleep instead of spinning
    static Switches from_env() {
        Switches w;
        const char* e = getenv("PMHIP_HILO");
        w.hilo = !(e && atoi(e) == 0);
        e = getenv("PMHIP_LN_UNFOLD");
        w.fold = !(e && atoi(e) != 0);
        e = getenv("PMHIP_FOLD_MAX_ROWS");
        w.fold_rows_cap = e ? atoi(e) : 0;
        e = getenv("PMHIP_HILO_CENTER");
        w.center = !(e && atoi(e) == 0);
        e = getenv("PMHIP_BLOCKING_WAIT");
        w.blocking_wait = e && atoi(e) != 0;
        e = getenv("PMHIP_DECODE_OVERLAP_MAX_ROWS");
        if (e) w.overlap_rows = atoi(e);
        w.logits_stats = pm_dev_knob("PMHIP_LOGITS_STATS", 1) != 0;
        return w;
    }
    // bit 2 (the producers leave row statistics for the fold) is constant: the switch that cleared it is gone, the bit keeps its place
    int key() const { return (hilo ? 2 : 0) + (fold ? 1 : 0) + 4 + (center ? 8 : 0); }
};

// LayerNorm fold: where the per-row coefficients (TowerBufs::coef) of the CURRENT hi plane stand.  Every transition is written here:
//   produced()  a residual GEMM wrote a new hi plane (and, with_parts, left its partial row statistics behind)  -> kStale
//   requested() a folded LayerNorm is about to consume the plane: true = nobody can derive the coefficients from parts, the caller
//               runs the pass over the plane now (-> kWritten); false = left to the first folded consumer (-> kDeferred)
//   consumed()  a folded consumer is being launched: it writes the coefficients from parts or finds them written  -> kWritten
// A reader of coef -- the centred producer, residual_gemm -- takes them unless kStale and refuses to run on kDeferred (round-5
// advisor: the invariant was implicit).
struct FoldState {
    enum { kStale, kDeferred, kWritten } coef = kStale;
    bool parts = false;     // TowerBufs::parts describe the current hi plane
    void produced(bool with_parts) { coef = kStale; parts = with_parts; }
    bool requested() { coef = parts ? kDeferred : kWritten; return !parts; }
    void consumed() { coef = kWritten; }
};

struct TowerBufs {
    float* x = nullptr;     // residual stream, fp32 [M, dim]                      (fp32-verify mode)
    void* xh = nullptr;     // residual stream as a bf16 pair: x = hi + lo, [M, dim] each   (bf16-perf mode).  The hi plane IS
    void* xl = nullptr;     //   bf16(x): the operand of every GEMM that consumes LN(x) with the LayerNorm folded in
    void* y = nullptr;      // normed activations, T [M, dim] (unfolded LayerNorm output)
    void* q = nullptr; void* k = nullptr; void* vt = nullptr;
    void* attn = nullptr;   // T [M, inner]
    void* hid = nullptr;    // T [M, hidden_pad]
    float* split = nullptr; // dim_head != 64 only: f32 scratch of the plain head-split path [M, 3*inner]
    float* coef = nullptr;  // LayerNorm fold: per-row (rstd, -rstd * mean) of the hi plane
    float* parts = nullptr; // ... and the partial row statistics the last residual GEMM left behind, [M, dim/64, 2]
    FoldState st;           // where coef and parts stand
    float* shift = nullptr;     // per-row running sum of the subtracted means: only where the absolute x is needed again (ViT encoder)
    const Switches* sw = nullptr;   // the handle's
    bool hilo = false;      // bf16 mode
    bool fold = false;      // hilo and folding not disabled (PMHIP_LN_UNFOLD=1 forces the separate LayerNorm kernel: A/B tests)
    // centred hi plane (gemm_common.h, GemmParams::center_coef): the producers subtract the row mean the last LayerNorm saw
    // (fold on and not PMHIP_HILO_CENTER=0)
    bool center() const { return fold && sw->center; }
};

// where a residual GEMM takes its addend from: fp32 rows (verify mode), or a pair of bf16 planes (bf16 mode)
struct ResSrc {
    const float* f32 = nullptr;
    const void* hi = nullptr; const void* lo = nullptr;
    int ld = 0, rows = 0;      // row stride; rows > 0: the addend row is m % rows (position embedding)
};

// bf16 mode: the LayerNorm that precedes every projection (stage1/layers.py:54-58, stage2/transformer.py:44-49) is folded into
// that projection wherever the 256x256 kernel serves the shape: the consumer multiplies the hi plane by gamma-scaled weights
// and normalises in its epilogue with the row's (rstd, -rstd * mean) from pmhip_ln_coef.  Elsewhere (small batches, the
// decoder's 192-wide projection) pmhip_layernorm_hilo writes LN(x) and the plain GEMM runs.
inline int dh_of(const pmhip_tower_cfg& tc) { return tc.dim_head > 0 ? tc.dim_head : 64; }

int check_dim_head(const char* who, const pmhip_tower_cfg& tc) {
    const int dh = dh_of(tc);
    PM_REQUIRE(tc.heads > 0 && dh >= 16 && dh <= 128 && dh % 16 == 0 && (tc.heads * dh) % 64 == 0,
               "%s: heads=%d dim_head=%d: dim_head must be a multiple of 16 in [16,128] and heads*dim_head a multiple of 64", who, tc.heads, dh);
    return PMHIP_OK;
}

// widest residual stream the hi/lo row operators (pmhip_split_hilo, pmhip_layernorm_hilo, pmhip_layernorm_to_hilo, pmhip_ln_coef,
// pmhip_join_hilo: one wave per row, the row in registers) serve; wider bf16 towers keep the fp32 stream + pmhip_layernorm
constexpr int kHiloMaxDim = 1024;

int alloc_tower(Workspace& ws, const Switches& sw, const char* tag, int dtype, const pmhip_tower_cfg& tc, int B, int tokens, TowerBufs& b,
                hipStream_t s) {
    const size_t es = dtype_size(dtype);
    const size_t M = (size_t)B * tokens;
    const int dh = dh_of(tc), inner = tc.heads * dh, Np = round_up(tokens, 64);
    std::string t(tag);
    b.hilo = dtype == PMHIP_BF16 && sw.hilo && tc.dim <= kHiloMaxDim;
    if (b.hilo) {
        WS(ws, (t + ".xh").c_str(), M * tc.dim * 2, b.xh);
        WS(ws, (t + ".xl").c_str(), M * tc.dim * 2, b.xl);
    } else {
        WS(ws, (t + ".x").c_str(), M * tc.dim * 4, b.x);
    }
    WS(ws, (t + ".y").c_str(), M * tc.dim * es, b.y);
    WS(ws, (t + ".q").c_str(), (size_t)B * tc.heads * tokens * dh * es, b.q);
    WS(ws, (t + ".k").c_str(), (size_t)B * tc.heads * Np * dh * es, b.k);
    WS(ws, (t + ".vt").c_str(), (size_t)B * tc.heads * Np * dh * es, b.vt);
    WS(ws, (t + ".attn").c_str(), M * inner * es, b.attn);
    WS(ws, (t + ".hid").c_str(), M * tc.hidden_pad * es, b.hid);
    WS(ws, (t + ".coef").c_str(), M * 2 * 4, b.coef);
    WS(ws, (t + ".parts").c_str(), M * (size_t)round_up(tc.dim, 64) / 64 * 2 * 4, b.parts);
    b.split = nullptr;
    if (dh != 64) WS(ws, (t + ".split").c_str(), M * 3 * inner * 4, b.split);
    b.sw = &sw;
    b.fold = b.hilo && dh == 64 && sw.fold;
    b.st = FoldState{};
    b.shift = nullptr;
    return PMHIP_OK;
}

// the residual stream itself as the addend (x += ...)
ResSrc res_self(const TowerBufs& b, int dim) {
    ResSrc r;
    r.f32 = b.x; r.hi = b.xh; r.lo = b.xl; r.ld = dim; r.rows = 0;
    return r;
}

// residual GEMM x = A . W^T + bias + addend, written to the tower's residual stream (in place when the addend is the stream)
int residual_gemm(int dtype, TowerBufs& b, const void* A, int lda, const void* W, int ldw, const float* bias, const ResSrc& r,
                  int M, int N, int K, hipStream_t s, float bias_mean = 0.f) {
    if (b.hilo) {
        const bool self = r.hi == b.xh && r.rows == 0;                 // x += ... (not the GEMM that opens the stream)
        const float* cc = (b.center() && self && b.st.coef != FoldState::kStale) ? b.coef : nullptr;
        PM_REQUIRE(!cc || b.st.coef != FoldState::kDeferred,
                   "residual_gemm: the fold coefficients of this LayerNorm were left to a folded consumer that never ran");
        const int shift_mode = !b.shift ? 0 : (self ? (cc ? 2 : 0) : 1);
        // with the LayerNorm folded into the consumers the producer's epilogue also leaves the row statistics of the new hi plane
        // (16 bytes per 64 columns): the coefficient pass over the plane (pmhip_ln_coef, 14 us per launch at the bench shape)
        // becomes a combination of 8-16 partials per row.
        b.st.produced(b.fold && N % 64 == 0 && N <= 1024);             // pmhip_ln_coef_parts combines <= 16 parts
        return pmhip_gemm_hilo_center(A, lda, W, ldw, bias, r.hi, r.lo, r.ld, r.rows, b.xh, b.xl, N, M, N, K, b.st.parts ? b.parts : nullptr,
                                      cc, bias_mean, b.shift, shift_mode, s);
    }
    return pmhip_gemm(dtype, A, lda, W, ldw, bias, r.f32, r.ld, r.rows, b.x, N, PMHIP_F32, M, N, K, s);
}

// LN(x) of the tower's residual stream into b.y (the unfolded path)
int tower_layernorm(int dtype, TowerBufs& b, const float* g, const float* be, int M, int dim, hipStream_t s) {
    if (b.hilo) return pmhip_layernorm_hilo(b.xh, b.xl, g, be, 1e-5f, b.y, dtype, M, dim, s);
    return pmhip_layernorm(b.x, g, be, 1e-5f, b.y, dtype, M, dim, s);
}

// Folded or not must not depend on the BATCH (the two routes differ in rounding, and an image's result may not depend on
// how many images run with it -- lanes, ranks and batch sizes all give bit-identical images): the decision looks at the
// per-image row count and the weight shape only, and the 256x256 kernel then takes the shape whatever its tile count.
// The 256x256 kernel addresses its operands with 32-bit byte offsets (set_lnfold in gemm.hip refuses M * lda * 2 >= 2^31): the
// weight and ONE image's rows must fit -- a larger batch is cut into launches of whole images by fold_rows(), so the decision
// stays a function of the shape and the result stays bit-identical for every batch size.
bool fold_shape_ok(int tokens, int n_out, int dim) { return pm_lnfold_shape_ok(tokens, n_out, dim, dim, dim); }

// rows one folded launch may take: whole images, below the 32-bit byte-offset limit
int fold_rows(const TowerBufs& b, int M, int tokens, int dim) {
    long long rows = ((1ll << 31) - 1) / ((long long)dim * 2);
    if (b.sw->fold_rows_cap > 0 && b.sw->fold_rows_cap < rows) rows = b.sw->fold_rows_cap;
    long long imgs = rows / tokens;
    if (imgs < 1) imgs = 1;
    return (int)std::min<long long>(M, imgs * tokens);
}

// A folded consumer of LN(x) over the whole tower (c, d: its fold vectors), in launches of whole images: launch(m0, rows, a, ln) runs
// the GEMM of the rows [m0, m0 + rows), a = those rows of the hi plane.  The (rstd, -rstd * mean) of the rows go to b.coef: where the
// last residual GEMM left partial row statistics behind, the consumer itself produces them (pmhip_lnfold::parts: in its own prologue
// for a small launch, by pmhip_ln_coef_parts in front of it otherwise) and nothing is launched for them here; else the pass over
// the plane.  The ONLY place a fold descriptor is built: a consumer handed a descriptor without `parts` would read coefficients
// nobody wrote.
template <typename Launch>
int folded_consumer(TowerBufs& b, int M, int tokens, int dim, const float* c, const float* d, hipStream_t s, Launch&& launch) {
    if (b.st.requested()) PM_TRY(pmhip_ln_coef(b.xh, 1e-5f, b.coef, M, dim, s));
    const int step = fold_rows(b, M, tokens, dim);
    for (int m0 = 0; m0 < M; m0 += step) {
        pmhip_lnfold ln{};
        ln.coef = b.coef + (size_t)m0 * 2; ln.c = c; ln.d = d;
        if (b.st.parts) { ln.parts = b.parts + (size_t)m0 * (dim / 64) * 2; ln.nparts = dim / 64; ln.eps = 1e-5f; }
        b.st.consumed();
        PM_TRY(launch(m0, std::min(step, M - m0), reinterpret_cast<const unsigned char*>(b.xh) + (size_t)m0 * dim * 2, &ln));
    }
    return PMHIP_OK;
}

// LN(x) -> head-split projection: folded when the shape is served, else LayerNorm + GEMM
int ln_heads(int dtype, TowerBufs& b, const float* g, const float* be, const void* W, const void* Wf, const float* fc, const float* fd,
             int M, int dim, int heads, int dh, int tokens, int Np, int nparts, const int* kinds, void* const* outs, float q_scale,
             hipStream_t s) {
    if (b.fold && Wf && fold_shape_ok(tokens, nparts * heads * 64, dim))
        return folded_consumer(b, M, tokens, dim, fc, fd, s, [&](int m0, int rows, const void* a, const pmhip_lnfold* ln) {
            const size_t b0 = (size_t)(m0 / tokens);
            void* o[3] = {nullptr, nullptr, nullptr};
            for (int i = 0; i < nparts; ++i)
                o[i] = reinterpret_cast<unsigned char*>(outs[i]) + b0 * heads * (kinds[i] == PMHIP_PART_Q ? tokens : Np) * 64 * dtype_size(dtype);
            return pmhip_gemm_heads_ln(dtype, a, dim, Wf, dim, rows, dim, heads, tokens, Np, nparts, kinds, o, q_scale, ln, s);
        });
    PM_TRY(tower_layernorm(dtype, b, g, be, M, dim, s));
    return pmhip_gemm_heads_dh(dtype, b.y, dim, W, dim, M, dim, heads, dh, tokens, Np, nparts, kinds, outs, q_scale, b.split, s);
}

// A controlled layer sees B / 2 pairs: images [0, B / 2) the source passes, [B / 2, B) the edited ones.  of(): where the
// edited half of a per-image array starts.
struct PairHalf {
    int half; size_t es;
    PairHalf(int dtype, int B) : half(B / 2), es(dtype_size(dtype)) {}
    unsigned char* of(const void* base, size_t per_image) const {
        return const_cast<unsigned char*>(reinterpret_cast<const unsigned char*>(base)) + (size_t)half * per_image * es;
    }
};

// one pre-LN transformer block (stage1/layers.py:54-58; stage2/transformer.py:44-49)
int layer_forward(int dtype, const pmhip_layer_weights& L, const pmhip_tower_cfg& tc, TowerBufs& b, int B, int tokens,
                  bool stage2, const CrossKV* cross, hipStream_t s) {
    const int dh = dh_of(tc);
    const int M = B * tokens, dim = tc.dim, inner = tc.heads * dh, Np = round_up(tokens, 64);
    const bool fast = dtype == PMHIP_BF16;
    const float q_scale = (dh == 64 ? 0.125f : 1.0f / sqrtf((float)dh)) * (fast ? kLog2e : 1.0f);   // dim_head^-0.5, attention.py:31,52
    const int kinds_qkv[3] = {PMHIP_PART_Q, PMHIP_PART_K, PMHIP_PART_V};
    const ResSrc self = res_self(b, dim);

    // x = attn1(norm1(x)) + x
    {
        void* outs[3] = {b.q, b.k, b.vt};
        PM_TRY(ln_heads(dtype, b, L.ln1_g, L.ln1_b, L.wqkv, L.wqkv_f, L.qkv_c, L.qkv_d, M, dim, tc.heads, dh, tokens, Np, 3, kinds_qkv, outs,
                        q_scale, s));
    }
    if (cross && cross->ctl_self) {
        // self-attention injection: the edited half attends with the source half's Q and K and its own V^T -- pointers only
        const PairHalf e(dtype, B);
        PM_TRY(pmhip_attention_dh(dtype, b.q, b.k, b.vt, b.attn, inner, e.half, tc.heads, dh, tokens, tokens, Np, fast, s));
        PM_TRY(pmhip_attention_dh(dtype, b.q, b.k, e.of(b.vt, (size_t)tc.heads * dh * Np), e.of(b.attn, (size_t)tokens * inner), inner, e.half,
                                  tc.heads, dh, tokens, tokens, Np, fast, s));
    } else {
        PM_TRY(pmhip_attention_dh(dtype, b.q, b.k, b.vt, b.attn, inner, B, tc.heads, dh, tokens, tokens, Np, fast, s));
    }
    PM_TRY(residual_gemm(dtype, b, b.attn, inner, L.wo, inner, L.bo, self, M, dim, inner, s, L.bo_mean));

    if (stage2) {
        // x = attn2(norm2(x), context) + x ; context None -> a second self-attention (attention.py:47)
        if (cross && cross->k) {
            const int kind_q[1] = {PMHIP_PART_Q};
            void* outs[1] = {b.q};
            PM_TRY(ln_heads(dtype, b, L.lnx_g, L.lnx_b, L.wqkv2, L.wqkv2_f, L.qkv2_c, L.qkv2_d, M, dim, tc.heads, dh, tokens, Np, 1, kind_q,
                            outs, q_scale, s));
            // the one launch that sees per-image context lengths (self-attention and the unconditional pass never do): the set's
            // arrays go into one record, which selects the form; key sets subsume the lengths (padding is segment 255)
            PmAttnArgs a{b.q, cross->k, cross->vt, b.attn, inner, B, tc.heads, tokens, cross->L, cross->Lp, fast};
            a.key_seg = cross->key_seg; a.query_mask = cross->query_mask; a.key_bias = cross->key_bias;
            a.lens = a.key_seg ? nullptr : cross->lens;
            a.stream = s;
            if (cross->ctl_map) {
                // the source half as ever, on its own; the edited half blends the source half's probabilities into its own
                const PairHalf e(dtype, B);
                a.B = e.half;
                PM_TRY(attention_any("attention", dtype, dh, a));
                PM_TRY(pmhip_attention_control(dtype, b.q, cross->k, e.of(b.q, (size_t)tc.heads * tokens * dh),
                                               e.of(cross->k, (size_t)tc.heads * cross->Lp * dh), e.of(cross->vt, (size_t)tc.heads * dh * cross->Lp),
                                               e.of(b.attn, (size_t)tokens * inner), inner, e.half, tc.heads, dh, tokens, cross->L, cross->Lp, cross->L,
                                               cross->Lp, fast, cross->ctl_map, cross->ctl_blend, cross->ctl_gain, cross->lens,
                                               cross->lens ? cross->lens + e.half : nullptr, s));
            } else if (!cross->pick) {
                PM_TRY(attention_any("attention", dtype, dh, a));
            } else {
                // one launch per kind into one buffer, each leaving the other kinds' rows as they are: the plain
                // images under their lengths, the regional ones under their key sets and, in a step with a weighted slot, the
                // weighted ones under their key sets and biases
                PmAttnArgs kind = a;
                kind.pick = cross->pick;
                kind.lens = cross->lens; kind.key_seg = nullptr; kind.query_mask = nullptr; kind.key_bias = nullptr; kind.want = 0;
                PM_TRY(attention_any("attention_pick", dtype, dh, kind));
                kind.lens = nullptr; kind.key_seg = a.key_seg; kind.query_mask = a.query_mask; kind.want = 1;
                PM_TRY(attention_any("attention_pick", dtype, dh, kind));
                if (a.key_bias) {
                    kind.key_bias = a.key_bias; kind.want = 2;
                    PM_TRY(attention_any("attention_pick_weighted", dtype, dh, kind));
                }
            }
            // the maps tap: the head-mean probabilities of the launch above, from the same Q, K, lengths, sets and biases
            if (cross->maps)
                PM_TRY(pmhip_attention_maps(dtype, a.Q, a.K, cross->maps, cross->L, B, tc.heads, dh, tokens, cross->L, cross->Lp, fast, a.lens,
                                            a.key_seg, a.query_mask, a.key_bias, cross->maps_scale, cross->maps_accumulate, s));
            // the phrase-score tap: where the pair looks at the phrase, from the same Q, K, lengths and control arrays
            if (cross->phr_src) {
                const PairHalf e(dtype, B);
                PM_TRY(pmhip_attention_phrase_score(dtype, b.q, cross->k, e.of(b.q, (size_t)tc.heads * tokens * dh),
                                                    e.of(cross->k, (size_t)tc.heads * cross->Lp * dh), e.half, tc.heads, dh, tokens, cross->L,
                                                    cross->Lp, cross->L, cross->Lp, fast, cross->ctl_map, cross->ctl_blend, cross->ctl_gain,
                                                    cross->lens, cross->lens ? cross->lens + e.half : nullptr, cross->phr_w_src,
                                                    cross->phr_w_edit, cross->phr_src, cross->phr_edit, cross->phr_scale, cross->phr_accumulate,
                                                    s));
            }
        } else {
            void* outs[3] = {b.q, b.k, b.vt};
            PM_TRY(ln_heads(dtype, b, L.lnx_g, L.lnx_b, L.wqkv2, L.wqkv2_f, L.qkv2_c, L.qkv2_d, M, dim, tc.heads, dh, tokens, Np, 3, kinds_qkv,
                            outs, q_scale, s));
            PM_TRY(pmhip_attention_dh(dtype, b.q, b.k, b.vt, b.attn, inner, B, tc.heads, dh, tokens, tokens, Np, fast, s));
        }
        PM_TRY(residual_gemm(dtype, b, b.attn, inner, L.wo2, inner, L.bo2, self, M, dim, inner, s, L.bo2_mean));
    }

    // x = ffnet(norm(x)) + x
    if (b.fold && L.w12p_f && fold_shape_ok(tokens, 2 * tc.hidden_pad, dim)) {
        PM_TRY(folded_consumer(b, M, tokens, dim, L.w12_c, L.w12_d, s, [&](int m0, int rows, const void* a, const pmhip_lnfold* ln) {
            return pmhip_gemm_swiglu_ln(dtype, a, dim, L.w12p_f, L.b12p,
                                        reinterpret_cast<unsigned char*>(b.hid) + (size_t)m0 * tc.hidden_pad * dtype_size(dtype), tc.hidden_pad,
                                        rows, tc.hidden_pad, dim, ln, s);
        }));
    } else {
        PM_TRY(tower_layernorm(dtype, b, L.ln2_g, L.ln2_b, M, dim, s));
        PM_TRY(pmhip_gemm_swiglu(dtype, b.y, dim, L.w12p, L.b12p, b.hid, tc.hidden_pad, M, tc.hidden_pad, dim, s));
    }
    return residual_gemm(dtype, b, b.hid, tc.hidden_pad, L.w3p, tc.hidden_pad, L.b3, self, M, dim, tc.hidden_pad, s, L.b3_mean);
}

// a position embedding as the addend of the GEMM that opens a residual stream: the fp32 table in verify mode, its hi / lo
// planes (split once per handle, kept in the workspace) in bf16 mode
int pos_source(Workspace& ws, const char* tag, bool hilo, const float* pos, int rows, int dim, bool& done, ResSrc& r, hipStream_t s) {
    r = ResSrc{};
    r.ld = dim; r.rows = rows;
    if (!hilo) { r.f32 = pos; return PMHIP_OK; }
    void* hi; void* lo;
    std::string t(tag);
    WS(ws, (t + ".hi").c_str(), (size_t)rows * dim * 2, hi);
    WS(ws, (t + ".lo").c_str(), (size_t)rows * dim * 2, lo);
    if (!done) {
        PM_TRY(pmhip_split_hilo(pos, hi, lo, rows, dim, s));
        done = true;
    }
    r.hi = hi; r.lo = lo;
    return PMHIP_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// VQModel
// ------------------------------------------------------------------------------------------------
static std::atomic<uint64_t> g_next_vq_uid{1};   // handles are created from lane threads too (Pipeline._lanes clones)
struct pmhip_vqgan {
    uint64_t uid = g_next_vq_uid.fetch_add(1, std::memory_order_relaxed);   // graph keys name the handle by this, never by its (reusable) heap address
    int device = 0, dtype = 0;
    pmhip_vqgan_cfg cfg{};
    pmhip_vqgan_weights w{};
    std::vector<pmhip_layer_weights> enc_layers, dec_layers;
    int grid = 0, tokens = 0, patch_k = 0;
    Workspace ws;
    Switches sw = Switches::from_env();
    bool dec_pos_split = false;     // bf16 mode: the decoder position embedding has been split into hi / lo planes (ws "decpos.*")
};

extern "C" int pmhip_vqgan_create(pmhip_vqgan** out, int device, int dtype, const pmhip_vqgan_cfg* cfg,
                                  const pmhip_vqgan_weights* w) {
    PM_REQUIRE(out && cfg && w, "vqgan_create: null argument");
    PM_REQUIRE(dtype == PMHIP_F32 || dtype == PMHIP_BF16, "vqgan_create: bad dtype");
    PM_REQUIRE(cfg->patch_size > 0 && cfg->image_size % cfg->patch_size == 0, "vqgan_create: image/patch mismatch");
    PM_REQUIRE(cfg->patch_size % 8 == 0, "vqgan_create: patch_size must be a multiple of 8");
    PM_REQUIRE((cfg->channels * cfg->patch_size * cfg->patch_size) % 64 == 0, "vqgan_create: C*P*P must be a multiple of 64");
    PM_REQUIRE(cfg->enc.dim % 64 == 0 && cfg->dec.dim % 64 == 0, "vqgan_create: dim must be a multiple of 64");
    PM_REQUIRE(cfg->enc.hidden_pad % 64 == 0 && cfg->dec.hidden_pad % 64 == 0, "vqgan_create: hidden_pad must be a multiple of 64");
    PM_REQUIRE(cfg->embed_dim <= 64 && cfg->embed_dim % 4 == 0, "vqgan_create: embed_dim must be <= 64 and a multiple of 4");
    PM_TRY(check_dim_head("vqgan_create(enc)", cfg->enc));
    PM_TRY(check_dim_head("vqgan_create(dec)", cfg->dec));
    auto h = std::make_unique<pmhip_vqgan>();
    h->device = device; h->dtype = dtype; h->cfg = *cfg; h->w = *w;
    h->enc_layers.assign(w->enc_layers, w->enc_layers + cfg->enc.depth);
    h->dec_layers.assign(w->dec_layers, w->dec_layers + cfg->dec.depth);
    h->w.enc_layers = h->enc_layers.data();
    h->w.dec_layers = h->dec_layers.data();
    h->grid = cfg->image_size / cfg->patch_size;
    h->tokens = h->grid * h->grid;
    h->patch_k = cfg->channels * cfg->patch_size * cfg->patch_size;
    *out = h.release();
    return PMHIP_OK;
}

extern "C" void pmhip_vqgan_destroy(pmhip_vqgan* h) {
    if (!h) return;
    (void)hipDeviceSynchronize();
    delete h;
}

namespace {

// Encoder.forward (stage1/layers.py:106-112): returns the residual stream in tb.x
int vq_encoder(pmhip_vqgan* h, const float* img, int B, TowerBufs& tb, hipStream_t s) {
    const auto& c = h->cfg;
    const int M = B * h->tokens, dim = c.enc.dim;
    PM_TRY(alloc_tower(h->ws, h->sw, "enc", h->dtype, c.enc, B, h->tokens, tb, s));
    void* pa; float* x0;
    WS(h->ws, "enc.patches", (size_t)M * h->patch_k * dtype_size(h->dtype), pa);
    WS(h->ws, "enc.x0", (size_t)M * dim * 4, x0);
    PM_TRY(pmhip_patchify(img, pa, h->dtype, B, c.channels, c.image_size, c.image_size, c.patch_size, s));
    // conv-as-GEMM (no bias) + position embedding, then norm_pre
    PM_TRY(pmhip_gemm(h->dtype, pa, h->patch_k, h->w.patch_w, h->patch_k, nullptr, h->w.enc_pos, dim, h->tokens, x0, dim,
                      PMHIP_F32, M, dim, h->patch_k, s));
    if (tb.hilo) PM_TRY(pmhip_layernorm_to_hilo(x0, h->w.pre_g, h->w.pre_b, 1e-5f, tb.xh, tb.xl, M, dim, s));
    else PM_TRY(pmhip_layernorm(x0, h->w.pre_g, h->w.pre_b, 1e-5f, tb.x, PMHIP_F32, M, dim, s));
    if (tb.center()) {
        // prev_quant (vqmodel.py:23) consumes the ABSOLUTE residual stream, so this tower keeps the running shift of its centred
        // hi plane and folds it back in at the end (the decoder and the stage-2 tower end in a LayerNorm, which never sees it)
        WS(h->ws, "enc.shift", (size_t)M * 4, tb.shift);
        PM_HIP(hipMemsetAsync(tb.shift, 0, (size_t)M * 4, s));
    }
    for (int l = 0; l < c.enc.depth; ++l)
        PM_TRY(layer_forward(h->dtype, h->enc_layers[l], c.enc, tb, B, h->tokens, false, nullptr, s));
    if (tb.shift) PM_TRY(pmhip_unshift_hilo(tb.xh, tb.xl, tb.shift, M, dim, s));
    return PMHIP_OK;
}

// transformer + norm + proj + un-patchify of Decoder.forward (stage1/layers.py:147-150); tb.x holds
// x + position_embedding on entry
int vq_decoder_tower(pmhip_vqgan* h, TowerBufs& tb, int B, float* img_out, bool clamp, hipStream_t s) {
    const auto& c = h->cfg;
    const int M = B * h->tokens, dim = c.dec.dim;
    for (int l = 0; l < c.dec.depth; ++l)
        PM_TRY(layer_forward(h->dtype, h->dec_layers[l], c.dec, tb, B, h->tokens, false, nullptr, s));
    float* yo;
    WS(h->ws, "dec.pixels", (size_t)M * h->patch_k * 4, yo);
    PM_TRY(tower_layernorm(h->dtype, tb, h->w.dn_g, h->w.dn_b, M, dim, s));
    PM_TRY(pmhip_gemm(h->dtype, tb.y, dim, h->w.proj_w, dim, h->w.proj_b, nullptr, 0, 0, yo, h->patch_k, PMHIP_F32, M,
                      h->patch_k, dim, s));
    const float lim = clamp ? 1.0f : INFINITY;
    return pmhip_unpatchify_clamp(yo, img_out, B, c.channels, c.image_size, c.image_size, c.patch_size, -lim, lim, s);
}

// VQModel.decode from zp = T [M,64] latent rows (vqmodel.py:27-30)
int vq_decode_latent(pmhip_vqgan* h, const void* zp, int B, float* img_out, hipStream_t s) {
    const auto& c = h->cfg;
    const int M = B * h->tokens, dim = c.dec.dim;
    TowerBufs tb;
    PM_TRY(alloc_tower(h->ws, h->sw, "dec", h->dtype, c.dec, B, h->tokens, tb, s));
    // post_quant + position embedding fused (vqmodel.py:28, layers.py:146)
    ResSrc pos;
    PM_TRY(pos_source(h->ws, "decpos", tb.hilo, h->w.dec_pos, h->tokens, dim, h->dec_pos_split, pos, s));
    PM_TRY(residual_gemm(h->dtype, tb, zp, 64, h->w.postq_w, 64, h->w.postq_b, pos, M, dim, 64, s));
    return vq_decoder_tower(h, tb, B, img_out, true, s);
}

int vq_decode_indices(pmhip_vqgan* h, const int64_t* idx, int B, float* img_out, hipStream_t s) {
    const int M = B * h->tokens;
    void* zp;
    WS(h->ws, "dec.zp", (size_t)M * 64 * dtype_size(h->dtype), zp);
    // l2norm(embedding(idx)) == a row of the pre-normalised codebook (quantize.py:40-44)
    PM_TRY(pmhip_embed_rows(h->w.codebook_n, idx, zp, h->dtype, 64, M, h->cfg.n_embed, h->cfg.embed_dim, s));
    return vq_decode_latent(h, zp, B, img_out, s);
}

}  // namespace

extern "C" int pmhip_vqgan_encoder_forward(pmhip_vqgan* h, const float* img, int B, float* x_out, pmhip_stream stream) {
    PM_REQUIRE(h && img && x_out && B > 0, "encoder_forward: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    TowerBufs tb;
    PM_TRY(vq_encoder(h, img, B, tb, s));
    if (tb.hilo) return pmhip_join_hilo(tb.xh, tb.xl, x_out, B * h->tokens, h->cfg.enc.dim, s);
    PM_HIP(hipMemcpyAsync(x_out, tb.x, (size_t)B * h->tokens * h->cfg.enc.dim * 4, hipMemcpyDeviceToDevice, s));
    return PMHIP_OK;
}

extern "C" int pmhip_vqgan_encode(pmhip_vqgan* h, const float* img, int B, float* z_out, int64_t* idx_out,
                                  float* loss_out, pmhip_stream stream) {
    PM_REQUIRE(h && img && idx_out && B > 0, "vqgan_encode: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    const auto& c = h->cfg;
    const int M = B * h->tokens, dim = c.enc.dim, E = c.embed_dim;
    TowerBufs tb;
    PM_TRY(vq_encoder(h, img, B, tb, s));
    // prev_quant acts on the raw residual stream (vqmodel.py:23): cast it to T when T != f32 (with the hi/lo stream the
    // operand bf16(x) is the hi plane itself)
    const void* xin = tb.hilo ? tb.xh : (const void*)tb.x;
    if (!tb.hilo && h->dtype != PMHIP_F32) {
        PM_TRY(pmhip_convert_pad(tb.x, dim, tb.y, h->dtype, dim, M, s));
        xin = tb.y;
    }
    float* ze; void* scratch;
    WS(h->ws, "enc.ze", (size_t)M * E * 4, ze);
    WS(h->ws, "enc.vq", pmhip_vq_scratch_bytes(M, c.n_embed), scratch);
    PM_TRY(pmhip_gemm(h->dtype, xin, dim, h->w.prevq_w, dim, h->w.prevq_b, nullptr, 0, 0, ze, E, PMHIP_F32, M, E, dim, s));
    return pmhip_vq_quantize(ze, h->w.codebook_n, h->w.codebook_sq, c.beta, z_out, idx_out, loss_out, scratch, M, c.n_embed,
                             E, s);
}

extern "C" int pmhip_vqgan_decode(pmhip_vqgan* h, const float* z, int B, float* img_out, pmhip_stream stream) {
    PM_REQUIRE(h && z && img_out && B > 0, "vqgan_decode: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    const int M = B * h->tokens;
    void* zp;
    WS(h->ws, "dec.zp", (size_t)M * 64 * dtype_size(h->dtype), zp);
    PM_TRY(pmhip_convert_pad(z, h->cfg.embed_dim, zp, h->dtype, 64, M, s));
    return vq_decode_latent(h, zp, B, img_out, s);
}

extern "C" int pmhip_vqgan_decode_indices(pmhip_vqgan* h, const int64_t* idx, int B, float* img_out,
                                          pmhip_stream stream) {
    PM_REQUIRE(h && idx && img_out && B > 0, "vqgan_decode_indices: bad arguments");
    return vq_decode_indices(h, idx, B, img_out, (hipStream_t)stream);
}

extern "C" int pmhip_vqgan_decoder_forward(pmhip_vqgan* h, const float* x, int B, float* img_out, pmhip_stream stream) {
    PM_REQUIRE(h && x && img_out && B > 0, "decoder_forward: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    const int M = B * h->tokens;
    TowerBufs tb;
    PM_TRY(alloc_tower(h->ws, h->sw, "dec", h->dtype, h->cfg.dec, B, h->tokens, tb, s));
    if (tb.hilo) {
        float* x0;
        WS(h->ws, "dec.x0", (size_t)M * h->cfg.dec.dim * 4, x0);
        PM_TRY(pmhip_add_rows(x, h->w.dec_pos, h->tokens, x0, M, h->cfg.dec.dim, s));
        PM_TRY(pmhip_split_hilo(x0, tb.xh, tb.xl, M, h->cfg.dec.dim, s));
    } else {
        PM_TRY(pmhip_add_rows(x, h->w.dec_pos, h->tokens, tb.x, M, h->cfg.dec.dim, s));
    }
    return vq_decoder_tower(h, tb, B, img_out, false, s);
}

// ------------------------------------------------------------------------------------------------
// stage 2: CondTransformer + MaskGIT loop
// ------------------------------------------------------------------------------------------------
namespace {

// A HIP event or stream that is created at most once, on first use, and destroyed with its owner.
template <typename H, hipError_t (*Create)(H*, unsigned), hipError_t (*Destroy)(H)>
struct HipOwned {
    H h = nullptr;
    HipOwned() = default;
    HipOwned(HipOwned&& o) noexcept : h(o.h) { o.h = nullptr; }
    HipOwned(const HipOwned&) = delete;
    HipOwned& operator=(const HipOwned&) = delete;
    ~HipOwned() { if (h) (void)Destroy(h); }
    int get(unsigned flags, H& out) {           // the flags of the FIRST call are the handle's
        if (!h) PM_HIP(Create(&h, flags));
        out = h;
        return PMHIP_OK;
    }
};
using OwnedEvent = HipOwned<hipEvent_t, hipEventCreateWithFlags, hipEventDestroy>;
using OwnedStream = HipOwned<hipStream_t, hipStreamCreateWithFlags, hipStreamDestroy>;

// Per-call host records travel through PINNED host memory (a pageable source makes hipMemcpyAsync stage synchronously): a ring of
// kParamSlots entries, each reused only after the last copy that read it has completed.  Per call: acquire(), stage() once per
// destination, commit().
struct PinnedRing {
    static constexpr int kParamSlots = 4;
    unsigned char* host = nullptr;
    size_t entry_bytes = 0;
    OwnedEvent done[kParamSlots];
    int cur = kParamSlots - 1;                                // the entry of the last acquire()
    ~PinnedRing() { if (host) (void)hipHostFree(host); }
    // at least `bytes` per entry (kept a multiple of 16: copy16_async takes its widest path from every entry)
    int reserve(size_t bytes) {
        if (bytes <= entry_bytes) return PMHIP_OK;
        for (auto& e : done)
            if (e.h) PM_HIP(hipEventSynchronize(e.h));        // copies still reading the old ring
        if (host) { PM_HIP(hipHostFree(host)); host = nullptr; entry_bytes = 0; }
        const size_t want = (bytes + 15) & ~(size_t)15;
        PM_HIP(hipHostMalloc(&host, want * kParamSlots));
        entry_bytes = want;
        return PMHIP_OK;
    }
    int acquire() {
        cur = (cur + 1) % kParamSlots;
        hipEvent_t e;
        PM_TRY(done[cur].get(hipEventDisableTiming, e));
        PM_HIP(hipEventSynchronize(e));                       // the copy that last read this entry (no-op when never recorded)
        return PMHIP_OK;
    }
    // src[0 .. bytes) -> the entry at `offset` -> dst, by a kernel on `s` that reads the entry through its device alias
    int stage(void* dst, size_t offset, const void* src, size_t bytes, hipStream_t s) {
        unsigned char* at = host + (size_t)cur * entry_bytes + offset;
        memcpy(at, src, bytes);
        void* alias = nullptr;
        PM_HIP(hipHostGetDevicePointer(&alias, at, 0));
        return copy16_async(dst, alias, bytes, s);
    }
    int commit(hipStream_t s) {                               // after the last stage() of the entry
        PM_HIP(hipEventRecord(done[cur].h, s));
        return PMHIP_OK;
    }
};

struct GraphEntry {
    bool warmed = false;            // one eager pass has sized every workspace buffer
    std::vector<hipGraphExec_t> segs;   // one executable graph per segment (a segment ends with a decoded step)
    uint64_t s2_gen = 0, vq_gen = 0;   // workspace generations the graphs' baked-in pointers belong to
    GraphEntry() = default;
    GraphEntry(const GraphEntry&) = delete;
    GraphEntry& operator=(const GraphEntry&) = delete;
    ~GraphEntry() { destroy(); }
    void destroy() {
        for (auto e : segs)
            if (e) (void)hipGraphExecDestroy(e);
        segs.clear();
    }
};

}  // namespace

struct pmhip_s2 {
    int device = 0, dtype = 0;
    pmhip_s2_cfg cfg{};
    pmhip_s2_weights w{};
    std::vector<pmhip_layer_weights> layers;
    std::vector<CrossKV> cross;     // per layer, valid after prepare_context
    std::vector<CrossKV> cross_neg; // per layer: the NEGATIVE context's set (pmhip_pipeline_*_negative), empty K/V when the last call brought none
    Workspace ws;
    Switches sw = Switches::from_env();
    bool pos_split = false;         // bf16 mode: position embedding split into hi / lo planes (ws "pos.*")
    std::map<std::string, GraphEntry> graphs;   // captured decode loops, keyed by shape / schedule structure
    OwnedStream capture_stream;                 // capture_graph
    // small batches: the ViT decode of step t runs on a side stream BESIDE the tower of step t + 1 (fork / join by events, inside
    // the captured graphs too)
    OwnedStream side_stream;
    OwnedEvent ev_fork, ev_join;
    PinnedRing params_ring;         // pipeline_generate: one PmGenParams per call
    // per-image decode state (pmhip_pipeline_step_slots): an entry of the ring holds B pmhip_slot records and, behind them, the B
    // pmhip_slot_guide records of a call with guidance (they travel under the entry's one event); the handle remembers which
    // context the last slots call prepared (slots_ctx_L: 0 = prepared without a context, -1 = nothing a slots call may reuse);
    // slots_one_pass / slots_two_pass / slots_three_pass count the steps by tower passes.  The negative set a slots call prepared
    // (pmhip_pipeline_step_slots_negative) is remembered the same way: slots_neg_Ln = -1: none a slots call may reuse
    PinnedRing slots_ring;
    PinnedRing lens_ring;           // per-image context lengths of a call (ctx_lens_host): B int32 -> workspace "ctx.lens"
    PinnedRing neg_lens_ring;       // ... and of its negative context (neg_lens_host): B int32 -> workspace "neg.lens"
    PinnedRing w_ring;              // prompt weights: B * L f32 -> workspace "ctx.w", from where pmhip_key_bias fills "ctx.bias"
    PinnedRing seg_ring;            // regional prompts: B * tokens uint32 token masks, then B * L uint8 row segments -> workspace "ctx.seg"
    PinnedRing ctl_ring;            // cross-attention control: row_map | blend | gain, each B * L 4-byte values -> workspace "ctl.arrays"
    PinnedRing counts_ring;         // the edit loop's re-masking counts (nmask_img_host): T * B int32 -> workspace "gen.counts"
    int slots_one_pass = 0, slots_two_pass = 0, slots_three_pass = 0;
    int slots_filter_tiles = 0, slots_filter_chain = 0;   // steps of pmhip_pipeline_step_slots_filter by the form of their sampling tail
    int slots_region_steps = 0;                           // steps of pmhip_pipeline_step_slots_regions that ran the two-launch cross-attention
    int slots_weight_steps = 0;                           // steps of pmhip_pipeline_step_slots_weights that ran the three-launch cross-attention
    int slots_edit_steps = 0;                             // steps of pmhip_pipeline_step_slots_edit that re-masked by a count per slot
    int slots_ctx_B = 0, slots_ctx_L = -1;
    int slots_neg_B = 0, slots_neg_Ln = -1;
    // device image d complete -> copy stream (one event per image of a call: an event is never re-recorded while a wait on
    // its previous record may still be queued); last D2H complete -> next call
    std::vector<OwnedEvent> img_ready;
    OwnedEvent host_copied;
    bool host_copy_pending = false;
    // the shared step 0 of unconditional loops that start from the all-mask state (PMHIP_GENERATE_FROM_MASK): the logits and block
    // statistics of ONE all-mask image (workspace "s0.logits" / "s0.lstats", fixed size) are a function of the weights alone,
    // which this handle never changes; filled by the first such loop, sampled from by every later one at any B
    bool s0_valid = false;
    int s0_fills = 0, s0_hits = 0;
    hipStream_t s0_stream = nullptr;            // the stream that filled the buffers: a loop on another stream waits for s0_ready
    OwnedEvent s0_ready;
};

extern "C" int pmhip_s2_create(pmhip_s2** out, int device, int dtype, const pmhip_s2_cfg* cfg, const pmhip_s2_weights* w) {
    PM_REQUIRE(out && cfg && w, "s2_create: null argument");
    PM_REQUIRE(dtype == PMHIP_F32 || dtype == PMHIP_BF16, "s2_create: bad dtype");
    PM_REQUIRE(cfg->tower.dim % 64 == 0 && cfg->tower.hidden_pad % 64 == 0, "s2_create: dim/hidden_pad must be multiples of 64");
    PM_REQUIRE(cfg->embed_dim <= 64 && cfg->embed_dim % 4 == 0, "s2_create: embed_dim must be <= 64 and a multiple of 4");
    PM_TRY(check_dim_head("s2_create", cfg->tower));
    PM_REQUIRE(cfg->context_dim_pad % 64 == 0 && cfg->context_dim_pad >= cfg->context_dim, "s2_create: bad context_dim_pad");
    PM_REQUIRE(w->ctxproj_w || cfg->context_dim == cfg->tower.dim, "s2_create: Identity context_proj needs context_dim == dim");
    PM_REQUIRE(cfg->n_embed % 4 == 0, "s2_create: n_embed must be a multiple of 4");
    auto h = std::make_unique<pmhip_s2>();
    h->device = device; h->dtype = dtype; h->cfg = *cfg; h->w = *w;
    h->layers.assign(w->layers, w->layers + cfg->tower.depth);
    h->w.layers = h->layers.data();
    h->cross.resize(cfg->tower.depth);
    h->cross_neg.resize(cfg->tower.depth);
    *out = h.release();
    return PMHIP_OK;
}

extern "C" void pmhip_s2_destroy(pmhip_s2* h) {
    if (!h) return;
    (void)hipDeviceSynchronize();
    delete h;
}

namespace {

// Which cross K/V a tower's attn2 layers attend to: none (the unconditional branch: a second self-attention), the context's, or
// the negative context's.  The two sets are the same thing twice -- workspace buffers, a device length array and ring staging of
// their own -- so s2_prepare_context and s2_set_ctx_lens are written once and act on the set they are told.
enum CrossSet { kCrossNone = 0, kCrossContext, kCrossNegative };
struct CrossSetRef {
    std::vector<CrossKV>& kv;
    PinnedRing& ring;
    const char *in, *proj, *kvbuf, *split, *lens;           // workspace names
};
CrossSetRef cross_set(pmhip_s2* h, CrossSet set) {
    if (set == kCrossNegative) return {h->cross_neg, h->neg_lens_ring, "neg.in", "neg.proj", "neg.kv", "neg.split", "neg.lens"};
    return {h->cross, h->lens_ring, "ctx.in", "ctx.proj", "ctx.kv", "ctx.split", "ctx.lens"};
}

// context_proj (transformer.py:84-85) and every layer's attn2 to_k / to_v of the projected context
// (attention.py:48-49).  The context is static over a decode loop, so this runs once per loop.
// Every model-level entry prepares (or drops) the context's set first; that drops the negative set too, so a call that brings no
// negative context can never run against a stale one.  An entry with a negative context prepares that set right behind.
int s2_prepare_context(pmhip_s2* h, const float* context, int L, int B, hipStream_t s, CrossSet set = kCrossContext) {
    const auto& c = h->cfg;
    const int dim = c.tower.dim, heads = c.tower.heads, dh = dh_of(c.tower), inner = heads * dh;
    const size_t es = dtype_size(h->dtype);
    const CrossSetRef cs = cross_set(h, set);
    h->slots_ctx_L = -1;                                      // whatever a slots call prepared is about to be replaced
    h->slots_neg_Ln = -1;                                     // (a slots call sets both again behind its own preparation)
    if (set == kCrossContext)
        for (auto& ck : h->cross_neg) ck = CrossKV{};
    if (!context) {
        for (auto& ck : cs.kv) ck = CrossKV{};
        return PMHIP_OK;
    }
    PM_REQUIRE(L > 0, "s2: context given with L=%d", L);
    const int Mc = B * L, Lp = round_up(L, 64);
    void* cT; void* cp = nullptr;
    WS(h->ws, cs.in, (size_t)Mc * c.context_dim_pad * es, cT);
    PM_TRY(pmhip_convert_pad(context, c.context_dim, cT, h->dtype, c.context_dim_pad, Mc, s));
    if (h->w.ctxproj_w) {
        WS(h->ws, cs.proj, (size_t)Mc * dim * es, cp);
        PM_TRY(pmhip_gemm(h->dtype, cT, c.context_dim_pad, h->w.ctxproj_w, c.context_dim_pad, nullptr, nullptr, 0, 0, cp, dim,
                          h->dtype, Mc, dim, c.context_dim_pad, s));
    } else {
        cp = cT;
    }
    const size_t per = (size_t)B * heads * Lp * dh * es;
    unsigned char* kv;
    WS(h->ws, cs.kvbuf, per * 2 * c.tower.depth, kv);
    float* split = nullptr;
    if (dh != 64) WS(h->ws, cs.split, (size_t)Mc * 2 * inner * 4, split);
    const int kinds[2] = {PMHIP_PART_K, PMHIP_PART_V};
    for (int l = 0; l < c.tower.depth; ++l) {
        void* outs[2] = {kv + per * (2 * l), kv + per * (2 * l + 1)};
        const unsigned char* wkv = reinterpret_cast<const unsigned char*>(h->layers[l].wqkv2) + (size_t)inner * dim * es;
        PM_TRY(pmhip_gemm_heads_dh(h->dtype, cp, dim, wkv, dim, Mc, dim, heads, dh, L, Lp, 2, kinds, outs, 1.0f, split, s));
        cs.kv[l].k = outs[0]; cs.kv[l].vt = outs[1]; cs.kv[l].L = L; cs.kv[l].Lp = Lp; cs.kv[l].lens = nullptr;
        cs.kv[l].key_seg = nullptr; cs.kv[l].query_mask = nullptr; cs.kv[l].pick = nullptr; cs.kv[l].key_bias = nullptr;
    }
    return PMHIP_OK;
}

// Per-image context lengths (ctx_lens_host of the *_lens entries), checked BEFORE anything is launched: 1 <= len <= L.  They need
// a context: without one attn2 is a second self-attention, which never sees lengths.
int check_ctx_lens(const char* who, const int32_t* lens_host, bool have_context, int L, int B) {
    if (!lens_host) return PMHIP_OK;
    PM_REQUIRE(have_context && L > 0, "%s: ctx_lens_host given without a context", who);
    for (int b = 0; b < B; ++b)
        PM_REQUIRE(lens_host[b] >= 1 && lens_host[b] <= L, "%s: image %d: context length %d must be in [1, L=%d]", who, b, (int)lens_host[b], L);
    return PMHIP_OK;
}

// The checked lengths travel like the slot records and PmGenParams: pinned ring entry -> copy kernel -> the handle's device array
// -> every layer's CrossKV, from where the cross-attention launch of layer_forward hands them to pmhip_attention_lens.  Called by
// every model-level entry AFTER the context is prepared or kept (lens_host NULL: the lengths of an earlier call are dropped), and
// always outside a graph: a captured graph bakes in the device array, never a length.
int s2_set_ctx_lens(pmhip_s2* h, const int32_t* lens_host, int L, int B, hipStream_t s, CrossSet set = kCrossContext) {
    const CrossSetRef cs = cross_set(h, set);
    int32_t* dlens = nullptr;
    if (lens_host) {
        const int Bp = round_up(B, 4);                        // 16-byte multiples: the copy kernel's widest path
        WS(h->ws, cs.lens, (size_t)Bp * 4, dlens);
        std::vector<int32_t> padded((size_t)Bp, L);
        std::copy(lens_host, lens_host + B, padded.begin());
        PM_TRY(cs.ring.reserve((size_t)Bp * 4));
        PM_TRY(cs.ring.acquire());
        PM_TRY(cs.ring.stage(dlens, 0, padded.data(), (size_t)Bp * 4, s));
        PM_TRY(cs.ring.commit(s));
    }
    for (auto& ck : cs.kv) {
        ck.lens = ck.k ? dlens : nullptr;
        ck.key_seg = nullptr; ck.query_mask = nullptr;        // the segments of an earlier call are dropped with its lengths
        ck.pick = nullptr;
        ck.key_bias = nullptr;                                // ... and so are its weights
    }
    return PMHIP_OK;
}

// One image's rows of the two arrays: every id in 0..31 or 255, every token allowing a segment that is present.  `noun` is what the
// messages call b: "image" in the *_segments entries, "slot" in a slots step (pmhip_pipeline_step_slots_regions).
int check_segments_of(const char* who, const char* noun, int b, const uint8_t* ctx_seg_host, const uint32_t* tok_seg_host, int L, int tokens) {
    uint32_t present = 0;
    for (int k = 0; k < L; ++k) {
        const int sg = ctx_seg_host[(size_t)b * L + k];
        PM_REQUIRE(sg < 32 || sg == 255, "%s: %s %d: context row %d: segment %d must be in 0..31, or 255 for padding", who, noun, b, k, sg);
        if (sg < 32) present |= 1u << sg;
    }
    for (int t = 0; t < tokens; ++t)
        PM_REQUIRE(tok_seg_host[(size_t)b * tokens + t] & present,
                   "%s: %s %d: token %d allows no segment that is present in its context (mask 0x%08x, present 0x%08x)", who, noun, b, t,
                   (unsigned)tok_seg_host[(size_t)b * tokens + t], (unsigned)present);
    return PMHIP_OK;
}

// Regional prompts (the *_segments entries), checked BEFORE anything is launched.  ctx_seg_host uint8 [B, L]: the segment 0..31 of
// every context row, 255 = padding; tok_seg_host uint32 [B, tokens]: bit s = the token attends to segment s.  Both or neither; they
// need a context (without one attn2 is a second self-attention, which never sees segments) and exclude ctx_lens_host, which the
// padding value subsumes.  Every token must allow a segment that is PRESENT in its image: an empty softmax has no value.
int check_segments(const char* who, const uint8_t* ctx_seg_host, const uint32_t* tok_seg_host, const int32_t* ctx_lens_host, bool have_context,
                   int L, int B, const pmhip_s2* h) {
    PM_REQUIRE(!ctx_seg_host == !tok_seg_host, "%s: ctx_seg_host and tok_seg_host come together (one of them is NULL)", who);
    if (!ctx_seg_host) return PMHIP_OK;
    PM_REQUIRE(have_context && L > 0, "%s: segments given without a context", who);
    PM_REQUIRE(!ctx_lens_host, "%s: segments and ctx_lens_host exclude each other (mark padding rows with segment 255)", who);
    const int tokens = h->cfg.tokens;                         // (the handle is read only once the arrays are known to be there)
    for (int b = 0; b < B; ++b) PM_TRY(check_segments_of(who, "image", b, ctx_seg_host, tok_seg_host, L, tokens));
    return PMHIP_OK;
}

// The checked segments travel like the lengths: one pinned ring entry (token masks, then row segments, each padded to 16 bytes) ->
// copy kernel -> the handle's device array "ctx.seg" -> every layer's CrossKV of the context's set, from where the cross-attention
// launch of layer_forward hands them to pmhip_attention_segments.  Called right behind s2_set_ctx_lens (which drops the segments of
// an earlier call), always outside a graph: a captured graph bakes in the device array, never a layout of regions.
// region_host (a slots step of pmhip_pipeline_step_slots_regions / _weights; NULL otherwise): the B kinds ride in the same ring entry,
// behind the row segments, into a device array of their own ("ctx.pick"), and the CrossKV keep the lengths s2_set_ctx_lens has just set.
int s2_set_segments(pmhip_s2* h, const uint8_t* ctx_seg_host, const uint32_t* tok_seg_host, int L, int B, hipStream_t s,
                    const uint8_t* region_host = nullptr) {
    if (!ctx_seg_host) return PMHIP_OK;
    const size_t qbytes = ((size_t)B * h->cfg.tokens * 4 + 15) & ~(size_t)15, kbytes = ((size_t)B * L + 15) & ~(size_t)15;
    const size_t pbytes = region_host ? ((size_t)B + 15) & ~(size_t)15 : 0;
    unsigned char* dseg;
    unsigned char* dpick = nullptr;
    WS(h->ws, "ctx.seg", qbytes + kbytes, dseg);
    if (region_host) WS(h->ws, "ctx.pick", pbytes, dpick);
    std::vector<unsigned char> packed(qbytes + kbytes, 255);
    memcpy(packed.data(), tok_seg_host, (size_t)B * h->cfg.tokens * 4);
    memcpy(packed.data() + qbytes, ctx_seg_host, (size_t)B * L);
    PM_TRY(h->seg_ring.reserve(qbytes + kbytes + pbytes));
    PM_TRY(h->seg_ring.acquire());
    PM_TRY(h->seg_ring.stage(dseg, 0, packed.data(), qbytes + kbytes, s));
    if (region_host) {
        std::vector<unsigned char> flags(pbytes, 0);
        memcpy(flags.data(), region_host, (size_t)B);
        PM_TRY(h->seg_ring.stage(dpick, qbytes + kbytes, flags.data(), pbytes, s));
    }
    PM_TRY(h->seg_ring.commit(s));
    for (auto& ck : h->cross)
        if (ck.k) { ck.query_mask = reinterpret_cast<const uint32_t*>(dseg); ck.key_seg = dseg + qbytes; ck.pick = dpick; }
    return PMHIP_OK;
}

// Prompt weights (the *_weights entries), checked BEFORE anything is launched, behind check_ctx_lens and check_segments.
// ctx_w_host f32 [B, L]: the weight of every context row, 0 or in [2^-20, 2^20].  They need a context; they stand beside the pair of
// segment arrays, beside ctx_lens_host, or alone -- without segment arrays the engine stages NEUTRAL ones: segment 0 for the rows
// below the image's length, 255 behind, every token mask all ones.  Every token must allow a row with w > 0.
struct CtxWeights {
    const float* w = nullptr;                                 // the caller's array, or NULL: no weights, everything below is the caller's
    std::vector<uint8_t> kseg;                                // the neutral arrays, when the caller gave none
    std::vector<uint32_t> tseg;
    const uint8_t* seg = nullptr;                             // what s2_set_segments stages
    const uint32_t* tok = nullptr;
    const int32_t* lens = nullptr;                            // what s2_set_ctx_lens stages: the caller's lengths, or NULL under weights
};
int check_weights(const char* who, const float* ctx_w_host, const uint8_t* ctx_seg_host, const uint32_t* tok_seg_host, const int32_t* ctx_lens_host,
                  bool have_context, int L, int B, const pmhip_s2* h, CtxWeights& out) {
    out.w = ctx_w_host; out.seg = ctx_seg_host; out.tok = tok_seg_host; out.lens = ctx_lens_host;
    if (!ctx_w_host) return PMHIP_OK;
    PM_REQUIRE(have_context && L > 0, "%s: weights given without a context", who);
    const int tokens = h->cfg.tokens;
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < L; ++k) {
            const float w = ctx_w_host[(size_t)b * L + k];
            PM_REQUIRE(std::isfinite(w) && (w == 0.f || (w >= 0x1p-20f && w <= 0x1p20f)),
                       "%s: image %d: context row %d: weight %g must be 0 or in [2^-20, 2^20]", who, b, k, (double)w);
        }
    if (!ctx_seg_host) {                                      // (check_segments has seen to it that both are NULL then)
        out.kseg.assign((size_t)B * L, 0);
        out.tseg.assign((size_t)B * tokens, 0xffffffffu);
        for (int b = 0; ctx_lens_host && b < B; ++b)
            for (int k = ctx_lens_host[b]; k < L; ++k) out.kseg[(size_t)b * L + k] = 255;
        out.seg = out.kseg.data(); out.tok = out.tseg.data();
    }
    out.lens = nullptr;                                       // the padding value subsumes the length
    for (int b = 0; b < B; ++b) {
        uint32_t present = 0;                                 // segments with a row of weight > 0
        for (int k = 0; k < L; ++k) {
            const int sg = out.seg[(size_t)b * L + k];
            if (sg < 32 && ctx_w_host[(size_t)b * L + k] > 0.f) present |= 1u << sg;
        }
        for (int t = 0; t < tokens; ++t)
            PM_REQUIRE(out.tok[(size_t)b * tokens + t] & present,
                       "%s: image %d: token %d allows no context row with a weight above 0 (mask 0x%08x, segments with such a row 0x%08x)", who, b,
                       t, (unsigned)out.tok[(size_t)b * tokens + t], (unsigned)present);
    }
    return PMHIP_OK;
}

// The checked weights travel like the segments: pinned ring entry -> copy kernel -> the handle's device array "ctx.w" -> the conversion
// kernel (pmhip_key_bias, in the score unit of the handle's dtype) -> the handle's device array "ctx.bias" -> every layer's CrossKV of
// the context's set, from where the cross-attention launch of layer_forward hands it to pmhip_attention_weighted.  Called right behind
// s2_set_segments, always outside a graph: a captured graph bakes in the bias array, never a weight.  In a slots step with a weighted
// slot (pmhip_pipeline_step_slots_weights) the set then carries lens, the segments, pick AND key_bias together, and the
// third picked launch of layer_forward (pmhip_attention_pick_weighted, want = 2) is the one that reads the bias.
int s2_set_weights(pmhip_s2* h, const float* ctx_w_host, int L, int B, hipStream_t s) {
    if (!ctx_w_host) return PMHIP_OK;
    const size_t n = (size_t)B * L, bytes = (n * 4 + 15) & ~(size_t)15;
    float* dw;
    float* dbias;
    WS(h->ws, "ctx.w", bytes, dw);
    WS(h->ws, "ctx.bias", bytes, dbias);
    std::vector<float> padded(bytes / 4, 0.f);
    std::copy(ctx_w_host, ctx_w_host + n, padded.begin());
    PM_TRY(h->w_ring.reserve(bytes));
    PM_TRY(h->w_ring.acquire());
    PM_TRY(h->w_ring.stage(dw, 0, padded.data(), bytes, s));
    PM_TRY(h->w_ring.commit(s));
    PM_TRY(pmhip_key_bias(dw, dbias, (int)n, h->dtype == PMHIP_BF16, s));
    for (auto& ck : h->cross)
        if (ck.k) ck.key_bias = dbias;
    return PMHIP_OK;
}

// One weighted slot's row of ctx_w_host (pmhip_pipeline_step_slots_weights), behind check_segments_of: the rules of
// check_weights for that slot alone -- every weight 0 or in [2^-20, 2^20], every token allowing a segment with a row of weight > 0.
int check_slot_weights(const char* who, int b, const float* ctx_w_host, const uint8_t* ctx_seg_host, const uint32_t* tok_seg_host, int L,
                       int tokens) {
    uint32_t present = 0;                                     // segments with a row of weight > 0
    for (int k = 0; k < L; ++k) {
        const float w = ctx_w_host[(size_t)b * L + k];
        PM_REQUIRE(std::isfinite(w) && (w == 0.f || (w >= 0x1p-20f && w <= 0x1p20f)),
                   "%s: slot %d: context row %d: weight %g must be 0 or in [2^-20, 2^20]", who, b, k, (double)w);
        const int sg = ctx_seg_host[(size_t)b * L + k];
        if (sg < 32 && w > 0.f) present |= 1u << sg;
    }
    for (int t = 0; t < tokens; ++t)
        PM_REQUIRE(tok_seg_host[(size_t)b * tokens + t] & present,
                   "%s: slot %d: token %d allows no context row with a weight above 0 (mask 0x%08x, segments with such a row 0x%08x)", who, b, t,
                   (unsigned)tok_seg_host[(size_t)b * tokens + t], (unsigned)present);
    return PMHIP_OK;
}

// The two records every decode family's call carries (the native twins of ops.Keys and of its negative set).  Absent features sit
// at their neutral values; an entry assigns the fields its own signature has.
struct CtxKeys {                                              // what says which context rows a token attends to
    const float* context = nullptr; int L = 0;                // [B, L, context_dim], or NULL: the unconditional branch
    const int32_t* lens = nullptr;                            // host [B] (the *_lens entries)
    const uint8_t* seg = nullptr; const uint32_t* tok = nullptr;   // host uint8 [B, L] and uint32 [B, tokens] (the *_segments entries)
    const float* w = nullptr;                                 // host f32 [B, L] (the *_weights entries)
    CtxKeys(const float* context_, int L_) : context(context_), L(L_) {}
};
struct NegSet {                                               // the negative context (the *_negative entries) with its host lengths [B]
    const float* context = nullptr; int Ln = 0; const int32_t* lens = nullptr;
};

// The negative context of the *_negative entries, checked BEFORE anything is launched (who: the entry family).  It and a guidance
// schedule need guidance and a context; Ln >= 1; 1 <= neg_len_b <= Ln; lengths need the negative context they are about.
int check_negative(const char* who, const NegSet& neg, bool schedule, bool guided, bool have_context, int B) {
    PM_REQUIRE(neg.context || !neg.lens, "%s: neg_lens_host given without a negative context", who);
    if (!neg.context && !schedule) return PMHIP_OK;
    PM_REQUIRE(guided && have_context, "%s: a negative context or a guidance schedule needs guidance (guided != 0) and a context", who);
    if (!neg.context) return PMHIP_OK;
    PM_REQUIRE(neg.Ln >= 1, "%s: negative context given with Ln=%d", who, neg.Ln);
    for (int b = 0; neg.lens && b < B; ++b)
        PM_REQUIRE(neg.lens[b] >= 1 && neg.lens[b] <= neg.Ln, "%s: image %d: negative context length %d must be in [1, Ln=%d]", who, b,
                   (int)neg.lens[b], neg.Ln);
    return PMHIP_OK;
}

// The context sequence of every model-level entry but the slots step (which keeps contexts and stages neutral rows: slots_context),
// in its two halves.  check_context: the three host checks of the key set, BEFORE anything is launched, yielding what is staged.
// (The negative set's own check, check_negative, stands earlier in the sample and generate families' order and carries a name of
// its own, so it stays a call of theirs.)
int check_context(const char* who, const CtxKeys& k, int B, const pmhip_s2* h, CtxWeights& cw) {
    PM_TRY(check_ctx_lens(who, k.lens, k.context != nullptr, k.L, B));
    PM_TRY(check_segments(who, k.seg, k.tok, k.lens, k.context != nullptr, k.L, B, h));
    return check_weights(who, k.w, k.seg, k.tok, k.lens, k.context != nullptr, k.L, B, h, cw);
}

// stage_context: the context's set prepared (or dropped, which drops the negative set of an earlier call too), its lengths, segments
// and weights staged -- the context's set only: the other passes never see segments or weights -- and behind it the negative set of
// a call that brings one.  Eager, outside any graph: once per call or loop.
int stage_context(pmhip_s2* h, const CtxKeys& k, const CtxWeights& cw, const NegSet& neg, int B, hipStream_t s) {
    PM_TRY(s2_prepare_context(h, k.context, k.L, B, s));
    PM_TRY(s2_set_ctx_lens(h, cw.lens, k.L, B, s));
    PM_TRY(s2_set_segments(h, cw.seg, cw.tok, k.L, B, s));
    PM_TRY(s2_set_weights(h, cw.w, k.L, B, s));
    if (neg.context) {
        PM_TRY(s2_prepare_context(h, neg.context, neg.Ln, B, s, kCrossNegative));
        PM_TRY(s2_set_ctx_lens(h, neg.lens, neg.Ln, B, s, kCrossNegative));
    }
    return PMHIP_OK;
}

// The name a call's messages carry, written once: the first arm whose feature is present names the call, widest feature first,
// otherwise the fallback (the caller's narrow name) -- the shape of S2Engine._call in engine.py.
struct NameArm { bool present; const char* name; };
const char* call_name(std::initializer_list<NameArm> arms, const char* fallback) {
    for (const NameArm& a : arms)
        if (a.present) return a.name;
    return fallback;
}

// token rows (T [M,64]) -> logits fp32 [M,V]  (transformer.py:81-82,87-91)
// set = kCrossNone: the unconditional branch (context None: every attn2 is a second self-attention, attention.py:47) although a
// context has been prepared -- the second forward of a guided step; kCrossNegative: that forward against the negative context
// block_stats (optional, n_embed % 64 == 0): the softmax statistics of the logits' 64-column blocks, [M][n_embed/64][2], written by
// the logits GEMM's epilogue for the sampling kernel (gemm_common.h GemmParams::block_stats)
int s2_tower(pmhip_s2* h, const void* tp, int B, float* logits, hipStream_t s, CrossSet set = kCrossContext, float* block_stats = nullptr) {
    const std::vector<CrossKV>* cross = set == kCrossNone ? nullptr : set == kCrossNegative ? &h->cross_neg : &h->cross;
    const auto& c = h->cfg;
    const int M = B * c.tokens, dim = c.tower.dim;
    TowerBufs tb;
    PM_TRY(alloc_tower(h->ws, h->sw, "s2", h->dtype, c.tower, B, c.tokens, tb, s));
    ResSrc pos;
    PM_TRY(pos_source(h->ws, "pos", tb.hilo, h->w.pos, c.tokens, dim, h->pos_split, pos, s));
    PM_TRY(residual_gemm(h->dtype, tb, tp, 64, h->w.tokproj_w, 64, h->w.tokproj_b, pos, M, dim, 64, s));
    for (int l = 0; l < c.tower.depth; ++l)
        PM_TRY(layer_forward(h->dtype, h->layers[l], c.tower, tb, B, c.tokens, true, cross ? &(*cross)[l] : nullptr, s));
    if (tb.fold && h->w.logits_wf && fold_shape_ok(c.tokens, c.n_embed, dim))   // the final norm folded into to_logits
        return folded_consumer(tb, M, c.tokens, dim, h->w.logits_c, h->w.logits_d, s, [&](int m0, int rows, const void* a, const pmhip_lnfold* ln) {
            float* out = logits + (size_t)m0 * c.n_embed;
            if (block_stats)
                return pmhip_gemm_softmax_stats(h->dtype, a, dim, h->w.logits_wf, dim, h->w.logits_b, out, c.n_embed, rows, c.n_embed, dim, ln,
                                                block_stats + (size_t)m0 * (c.n_embed / 64) * 2, s);
            return pmhip_gemm_ln(h->dtype, a, dim, h->w.logits_wf, dim, h->w.logits_b, out, c.n_embed, PMHIP_F32, rows, c.n_embed, dim, ln, s);
        });
    PM_TRY(tower_layernorm(h->dtype, tb, h->w.norm_g, h->w.norm_b, M, dim, s));
    if (block_stats)
        return pmhip_gemm_softmax_stats(h->dtype, tb.y, dim, h->w.logits_w, dim, h->w.logits_b, logits, c.n_embed, M, c.n_embed, dim, nullptr,
                                        block_stats, s);
    return pmhip_gemm(h->dtype, tb.y, dim, h->w.logits_w, dim, h->w.logits_b, nullptr, 0, 0, logits, c.n_embed, PMHIP_F32, M,
                      c.n_embed, dim, s);
}

// Pipeline.sample after the context is prepared (generate.py:161-179)
// Step::guidance != nullptr: the step's logits are uncond + *guidance * (cond - uncond), uncond = the same tower without the context
// (the branch the reference trains by dropping the text, utils/trainer.py:379,387-388); everything after the logits is unchanged
// The step in two halves, so that a caller can put something between the tower and the sampling (the small-batch loop joins the
// previous step's decode there).  step_tower: ids2tokens + the tower(s) -> logits.  step_tail: sampling, the optional decode,
// the optional copies, re-masking.
// the buffers the two halves share: the logits, the softmax statistics of their 64-column blocks for the sampling kernel (NULL:
// it derives them), and the predictions and scores the sampling leaves for the decode, the copies and the re-masking
struct StepBufs {
    float* logits = nullptr; float* lstats = nullptr;
    int64_t* pred = nullptr; float* score = nullptr;
};

int pred_bufs(pmhip_s2* s2, size_t M, StepBufs& b, hipStream_t s) {
    WS(s2->ws, "s2.pred", M * 8, b.pred);
    WS(s2->ws, "s2.score", M * 4, b.score);
    return PMHIP_OK;
}

// shared0: the logits and statistics are those of ONE image, kept: the shared step 0 (pmhip_s2::s0_valid)
int step_bufs(pmhip_s2* s2, int M, bool shared0, StepBufs& b, hipStream_t s) {
    const auto& c = s2->cfg;
    const size_t rows = shared0 ? c.tokens : M;
    WS(s2->ws, shared0 ? "s0.logits" : "s2.logits", rows * c.n_embed * 4, b.logits);
    b.lstats = nullptr;
    if (c.n_embed % 64 == 0 && s2->sw.logits_stats) WS(s2->ws, shared0 ? "s0.lstats" : "s2.lstats", rows * (c.n_embed / 64) * 8, b.lstats);
    return pred_bufs(s2, (size_t)M, b, s);
}

// the tower's input rows, T [M,64]
int tok_buf(pmhip_s2* s2, int M, void*& tp, hipStream_t s) {
    WS(s2->ws, "s2.tok", (size_t)M * 64 * dtype_size(s2->dtype), tp);
    return PMHIP_OK;
}

// ids2tokens: lookup in cat(raw codebook, mask_token) (generate.py:148-157)
int step_tokens(pmhip_s2* s2, const int64_t* ids, int M, void*& tp, hipStream_t s) {
    PM_TRY(tok_buf(s2, M, tp, s));
    return pmhip_embed_rows(s2->w.tok_table, ids, tp, s2->dtype, 64, M, s2->cfg.n_embed + 1, s2->cfg.embed_dim, s);
}

// the optional copies of a step's predictions and scores
int copy_aux(const StepBufs& b, size_t M, int64_t* pred_out, float* score_out, hipStream_t s) {
    if (pred_out) PM_HIP(hipMemcpyAsync(pred_out, b.pred, M * 8, hipMemcpyDeviceToDevice, s));
    if (score_out) PM_HIP(hipMemcpyAsync(score_out, b.score, M * 4, hipMemcpyDeviceToDevice, s));
    return PMHIP_OK;
}

// ONE description of a step, taken by both halves: where the values it samples, re-masks and guides by come from.  Exactly one
// of (the three sources of common.h PmStepSource, which source() maps them onto)
//   the batch scalars: one set of values for the batch;
//   gp: temperature, mask count, seed and row base from the device parameter block of a replayed loop (top-k and step stay);
//   slots: every per-image value from the device records slots [B], with guides [B] where an active slot is guided.
// shared0: every image samples from the one all-mask image's kept rows (step0_tower_once); guidance: the batch's scale (above).
struct Step {
    int topk = 0; float temperature = 0.f; int num_mask = 0;
    const float* noise = nullptr;
    uint64_t seed = 0; uint32_t step = 0; uint64_t image_base = 0;
    const PmGenParams* gp = nullptr;
    bool shared0 = false;
    const float* guidance = nullptr;
    const pmhip_slot* slots = nullptr; const pmhip_slot_guide* guides = nullptr;
    // guidance_dev: the batch's scale in DEVICE memory (a scheduled loop: &gp->gscales[step]) instead of *guidance; negative: the
    // second tower of a batch-guided step attends to the negative context's set instead of running without one
    const float* guidance_dev = nullptr; bool negative = false;
    // a slots step with guide records whose `on` names a kind (pmhip_pipeline_step_slots_negative): slots_neg: an active slot is
    // guided against the negative context (on == 2), slots_uncond: one against the pass without a context (on == 1) beside it
    bool slots_uncond = false, slots_neg = false;
    // the re-masking step's choice temperature, by the same three sources: the scalar choice_t (with optional
    // given uniforms choice_noise [B,N]); choice_params: gp->ctemps[step]; choice_dev: a device float [B] beside the slot records.
    // None of them set: the plain re-masking launch.
    float choice_t = 0.f; const float* choice_noise = nullptr; bool choice_params = false; const float* choice_dev = nullptr;
    // the token draw's nucleus mass: the batch's value, with the scalars and with gp alike (a kernel argument
    // of a captured step, like top-k); a slots step has none.  1: no filter.
    float top_p = 1.f;
    // the sampler filters per slot (pmhip_pipeline_step_slots_filter): the sampling tail of a slots step is
    // the launch per class, every slot's nucleus mass from the device array top_p_dev [B].  Off: the one block-statistics launch.
    bool filters = false; const float* top_p_dev = nullptr;
    // the edit loop: counts = the step's re-masking counts, a device int32 [B] beside the scalars or gp (NULL:
    // one count for the batch); decode_merged: the step's image -- inline or deferred -- is decoded from the MERGED ids
    const int32_t* counts = nullptr; bool decode_merged = false;
    PmStepSource source(int tokens) const { return source_of(tokens).with_counts(counts); }
    PmStepSource source_of(int tokens) const {
        if (slots) {
            const PmStepSource p = PmStepSource::per_image(slots, tokens), q = (choice_dev ? p.with_choice_dev(choice_dev) : p).with_top_p(top_p);
            return filters ? q.with_filters(top_p_dev) : q;
        }
        if (gp) { const PmStepSource p = PmStepSource::params(gp, topk, step); return (choice_params ? p.with_choice_params() : p).with_top_p(top_p); }
        return PmStepSource::batch(topk, temperature, num_mask, seed, step, image_base * (uint64_t)tokens).with_choice(choice_t, choice_noise).with_top_p(top_p);
    }
};

// guides: per-image guidance (pmhip_pipeline_step_slots_guided).  BOTH towers for the whole batch, the first one with the logits
// GEMM's block statistics (the same logits as without them, bit for bit: tests/test_gpu_abi_memory.py), then the combination in
// place on the rows of the guided images only -- an unguided image keeps the first tower's logits and statistics, i.e. exactly
// what the one-pass step leaves for it
int step_tower(pmhip_s2* s2, const int64_t* ids, int B, const Step& st, hipStream_t s) {
    const auto& c = s2->cfg;
    const int M = B * c.tokens;
    void* tp; StepBufs b;
    PM_TRY(step_tokens(s2, ids, M, tp, s));
    PM_TRY(step_bufs(s2, M, false, b, s));
    // the statistics come from the logits GEMM, or -- one scale for the batch -- from the combination, which produces the logits
    // that are sampled
    const bool batch_guided = st.guidance || st.guidance_dev;
    PM_TRY(s2_tower(s2, tp, B, b.logits, s, kCrossContext, batch_guided ? nullptr : b.lstats));
    if (!batch_guided && !st.guides) return PMHIP_OK;
    float* uncond;
    WS(s2->ws, "s2.logits_u", (size_t)M * c.n_embed * 4, uncond);
    if (st.guides && st.slots_neg) {
        // up to two more passes, one after the other into the same plane; each combine touches the images of its kind only, so
        // the two write disjoint rows and an unguided image keeps the first tower's
        if (st.slots_uncond) {
            PM_TRY(s2_tower(s2, tp, B, uncond, s, kCrossNone));
            PM_TRY(pmhip_guidance_combine_slots_which(b.logits, uncond, st.guides, st.slots, 1, c.tokens, b.logits, b.lstats, M, c.n_embed, s));
        }
        PM_TRY(s2_tower(s2, tp, B, uncond, s, kCrossNegative));
        return pmhip_guidance_combine_slots_which(b.logits, uncond, st.guides, st.slots, 2, c.tokens, b.logits, b.lstats, M, c.n_embed, s);
    }
    PM_TRY(s2_tower(s2, tp, B, uncond, s, st.negative ? kCrossNegative : kCrossNone));
    if (st.guidance_dev) return pmhip_guidance_combine_dev(b.logits, uncond, st.guidance_dev, b.logits, (size_t)M * c.n_embed, b.lstats, s);
    if (st.guides) return pmhip_guidance_combine_slots(b.logits, uncond, st.guides, st.slots, c.tokens, b.logits, b.lstats, M, c.n_embed, s);
    if (b.lstats) return pmhip_guidance_combine_stats(b.logits, uncond, *st.guidance, b.logits, (size_t)M * c.n_embed, b.lstats, s);
    return pmhip_guidance_combine(b.logits, uncond, *st.guidance, b.logits, (size_t)M * c.n_embed, s);
}

// the image of the predictions the last step_tail left in the handle's `s2.pred` (decoded from pred at ALL positions, generate.py:165)
int decode_pred(pmhip_s2* s2, pmhip_vqgan* vq, int B, float* img_out, hipStream_t s) {
    PM_REQUIRE(vq, "pipeline_sample: img_out requested without a vqgan handle");
    StepBufs b;
    PM_TRY(pred_bufs(s2, (size_t)B * s2->cfg.tokens, b, s));
    return vq_decode_indices(vq, b.pred, B, img_out, s);
}

// sampling, the optional decode, the optional copies, re-masking
int step_tail(pmhip_s2* s2, pmhip_vqgan* vq, int64_t* ids, int B, const Step& st, float* img_out, int64_t* pred_out, float* score_out,
              hipStream_t s) {
    const auto& c = s2->cfg;
    const int M = B * c.tokens;
    const PmStepSource src = st.source(c.tokens);
    StepBufs b;
    PM_TRY(step_bufs(s2, M, st.shared0, b, s));               // step_tower (or the shared step 0) filled the logits
    PM_TRY(pm_sample_rows(b.logits, c.n_embed, b.lstats, st.shared0 ? c.tokens : 0, ids, (int64_t)c.n_embed, st.noise, b.pred, ids, b.score,
                          M, c.n_embed, src, s));
    // the edit loop: the buffer the decode reads takes the merged ids (the sampler wrote them as ids_out) before the re-masking
    // launch below touches them -- the decode itself may run here or, deferred, beside the next step's tower
    if (st.decode_merged) PM_TRY(copy16_async(b.pred, ids, (size_t)M * 8, s));
    if (img_out) PM_TRY(decode_pred(s2, vq, B, img_out, s));
    PM_TRY(copy_aux(b, (size_t)M, pred_out, score_out, s));
    return pm_remask(ids, b.score, (int64_t)c.n_embed, B, c.tokens, src, s);
}

int sample_step(pmhip_s2* s2, pmhip_vqgan* vq, int64_t* ids, int B, const Step& st, float* img_out, int64_t* pred_out, float* score_out,
                hipStream_t s) {
    PM_TRY(step_tower(s2, ids, B, st, s));
    return step_tail(s2, vq, ids, B, st, img_out, pred_out, score_out, s);
}

// The tower half of step 0 of an unconditional loop from the all-mask state (ids: B all-mask images).  Its input is the same for
// every image and every call -- tok_table[mask] -> token_proj + pos -> the layers -> to_logits, no context -- rows of different
// images never mix, and the kernels are batch-invariant bit for bit, so image 0's logits ARE every image's, at any B.  The first
// such loop on a handle runs the ordinary tower and keeps image 0's rows; every later one runs nothing here, and step_tail
// (shared0) samples all B images from the kept rows.
int step0_tower_once(pmhip_s2* s2, const int64_t* ids, int B, hipStream_t s) {
    if (s2->s0_valid) return PMHIP_OK;
    PM_REQUIRE(!s2->ws.frozen, "pipeline_generate: the shared step-0 logits are missing during a graph capture");
    const auto& c = s2->cfg;
    StepBufs kept, b;
    PM_TRY(step_bufs(s2, B * c.tokens, true, kept, s));
    PM_TRY(step_tower(s2, ids, B, Step{}, s));
    PM_TRY(step_bufs(s2, B * c.tokens, false, b, s));
    PM_TRY(copy16_async(kept.logits, b.logits, (size_t)c.tokens * c.n_embed * 4, s));
    if (kept.lstats) PM_TRY(copy16_async(kept.lstats, b.lstats, (size_t)c.tokens * (c.n_embed / 64) * 8, s));
    hipEvent_t ready;
    PM_TRY(s2->s0_ready.get(hipEventDisableTiming, ready));
    PM_HIP(hipEventRecord(ready, s));
    s2->s0_stream = s;
    s2->s0_valid = true;
    ++s2->s0_fills;
    return PMHIP_OK;
}

// One executable graph of what record(stream) launches, captured on the handle's own stream (never the caller's: it may be the
// NULL stream) with both workspaces frozen; a library error from the recorded launches takes precedence over the HIP error.
template <typename Record>
int capture_graph(pmhip_s2* s2, pmhip_vqgan* vq, hipGraphExec_t* exec, Record&& record) {
    hipStream_t cap;
    PM_TRY(s2->capture_stream.get(hipStreamNonBlocking, cap));
    hipGraph_t g = nullptr;
    hipError_t rc;
    int unit_rc = PMHIP_OK;
    {
        struct Freeze {                                       // growing a workspace during the capture would be a bug
            Workspace& a; Workspace* b;
            Freeze(Workspace& a_, Workspace* b_) : a(a_), b(b_) { a.frozen = true; if (b) b->frozen = true; }
            ~Freeze() { a.frozen = false; if (b) b->frozen = false; }
        } freeze(s2->ws, vq ? &vq->ws : nullptr);
        rc = hipStreamBeginCapture(cap, hipStreamCaptureModeThreadLocal);
        if (rc == hipSuccess) {
            unit_rc = record(cap);                            // records only: nothing executes during capture
            rc = hipStreamEndCapture(cap, &g);
        }
    }
    if (unit_rc == PMHIP_OK && rc == hipSuccess) rc = hipGraphInstantiate(exec, g, nullptr, nullptr, 0);
    if (g) (void)hipGraphDestroy(g);
    PM_TRY(unit_rc);
    PM_HIP(rc);
    return PMHIP_OK;
}

// The graphs of one captured loop (ge: its entry in s2->graphs): n_units executable graphs, unit i = what run_unit(stream, i)
// launches.  The first call for an entry runs the units eagerly, which sizes every workspace buffer; the second captures them;
// every later one replays.  after(i) runs behind unit i, however it was run.  vq: the vqgan handle whose buffers the units use
// (NULL: none).
template <typename RunUnit, typename After>
int run_graphs(pmhip_s2* s2, pmhip_vqgan* vq, GraphEntry& ge, size_t n_units, hipStream_t s, RunUnit&& run_unit, After&& after) {
    if (!ge.warmed) {
        for (size_t i = 0; i < n_units; ++i) {                // eager once: sizes every workspace buffer
            PM_TRY(run_unit(s, i));
            PM_TRY(after(i));
        }
        ge.warmed = true;
        return PMHIP_OK;
    }
    // a workspace buffer of either handle was reallocated since the capture (a later call with a larger batch, a
    // longer context, a direct encode/decode on the shared vqgan handle ...): the graphs' pointers are stale
    if (!ge.segs.empty() && (ge.s2_gen != s2->ws.gen || (vq && ge.vq_gen != vq->ws.gen))) {
        PM_HIP(hipStreamSynchronize(s));                      // an earlier replay may still be running
        ge.destroy();
    }
    if (ge.segs.empty()) {
        for (size_t i = 0; i < n_units; ++i) {
            hipGraphExec_t exec = nullptr;
            const int rc = capture_graph(s2, vq, &exec, [&](hipStream_t cap) { return run_unit(cap, i); });
            if (rc != PMHIP_OK) { ge.destroy(); return rc; }
            ge.segs.push_back(exec);
        }
        ge.s2_gen = s2->ws.gen;
        ge.vq_gen = vq ? vq->ws.gen : 0;
    }
    for (size_t i = 0; i < n_units; ++i) {
        PM_HIP(hipGraphLaunch(ge.segs[i], s));
        PM_TRY(after(i));
    }
    return PMHIP_OK;
}

}  // namespace

namespace {
// One eager forward: the record the pmhip_s2_forward_* entries fill.  `who` is the entry's narrow name; maps_out / layer_bits are the
// maps tap of pmhip_s2_forward_maps.
struct ForwardCall {
    const char* who; pmhip_s2* h; const float* tokens; CtxKeys keys; int B; float* logits_out; pmhip_stream stream;
    uint64_t layer_bits = 0; float* maps_out = nullptr;
    ForwardCall(const char* who_, pmhip_s2* h_, const float* tokens_, const float* context, int L, int B_, float* logits_out_, pmhip_stream stream_)
        : who(who_), h(h_), tokens(tokens_), keys(context, L), B(B_), logits_out(logits_out_), stream(stream_) {}
};
}  // namespace

static int s2_forward_impl(const ForwardCall& c) {
    pmhip_s2* h = c.h;
    const int B = c.B;
    float* const maps_out = c.maps_out;
    const uint64_t layer_bits = c.layer_bits;
    const char* who = c.who;
    PM_REQUIRE(h && c.tokens && c.logits_out && B > 0, "%s: bad arguments", who);
    if (maps_out) {                                           // pmhip_s2_forward_maps: three checks of its own, before anything is launched
        const int depth = h->cfg.tower.depth;
        PM_REQUIRE(c.keys.context && c.keys.L > 0, "%s: the maps are those of the cross-attention: a context is required", who);
        PM_REQUIRE(layer_bits != 0, "%s: layer_bits selects no layer", who);
        PM_REQUIRE(depth >= 64 || (layer_bits >> depth) == 0, "%s: layer_bits 0x%llx selects a layer at or above depth=%d", who,
                   (unsigned long long)layer_bits, depth);
    }
    CtxWeights cw;
    PM_TRY(check_context(who, c.keys, B, h, cw));
    hipStream_t s = (hipStream_t)c.stream;
    const int M = B * h->cfg.tokens;
    PM_TRY(stage_context(h, c.keys, cw, NegSet{}, B, s));
    const float* tokens = c.tokens;
    float* logits_out = c.logits_out;
    void* tp;
    PM_TRY(tok_buf(h, M, tp, s));
    PM_TRY(pmhip_convert_pad(tokens, h->cfg.embed_dim, tp, h->dtype, 64, M, s));
    if (!maps_out) return s2_tower(h, tp, B, logits_out, s);
    // the maps tap: the chosen layers' sets carry the pointer for this one eager tower, the first one writing, the
    // later ones accumulating, each with scale 1 / n; cleared on every way out
    struct Tap {
        std::vector<CrossKV>& kv;
        ~Tap() { for (auto& ck : kv) { ck.maps = nullptr; ck.maps_scale = 1.f; ck.maps_accumulate = false; } }
    } tap{h->cross};
    int n = 0;
    for (size_t l = 0; l < h->cross.size() && l < 64; ++l) n += (int)((layer_bits >> l) & 1);
    bool first = true;
    for (size_t l = 0; l < h->cross.size() && l < 64; ++l)
        if ((layer_bits >> l) & 1) {
            h->cross[l].maps = maps_out; h->cross[l].maps_scale = 1.0f / (float)n; h->cross[l].maps_accumulate = !first;
            first = false;
        }
    return s2_tower(h, tp, B, logits_out, s);
}

extern "C" int pmhip_s2_forward(pmhip_s2* h, const float* tokens, const float* context, int L, int B, float* logits_out,
                                pmhip_stream stream) {
    return s2_forward_impl(ForwardCall("s2_forward", h, tokens, context, L, B, logits_out, stream));
}

extern "C" int pmhip_s2_forward_lens(pmhip_s2* h, const float* tokens, const float* context, int L, int B,
                                     const int32_t* ctx_lens_host, float* logits_out, pmhip_stream stream) {
    ForwardCall c("s2_forward_lens", h, tokens, context, L, B, logits_out, stream);
    c.keys.lens = ctx_lens_host;
    return s2_forward_impl(c);
}

// the handle's graph cache: keys it holds, and how many of them hold captured graphs (the first call under a key runs eagerly)
extern "C" int pmhip_s2_graph_count(const pmhip_s2* h, int* entries, int* captured) {
    PM_REQUIRE(h, "s2_graph_count: NULL handle");
    int n = 0;
    for (const auto& kv : h->graphs) n += kv.second.segs.empty() ? 0 : 1;
    if (entries) *entries = (int)h->graphs.size();
    if (captured) *captured = n;
    return PMHIP_OK;
}

// the two entries above pmhip_s2_forward that take no lengths report under the widest key array that came, otherwise as s2_forward
static const char* s2_forward_name(const CtxKeys& k) {
    return call_name({{k.w != nullptr, "s2_forward_weights"}, {k.seg || k.tok, "s2_forward_segments"}}, "s2_forward");
}

// ctx_seg_host == NULL and tok_seg_host == NULL: exactly pmhip_s2_forward
extern "C" int pmhip_s2_forward_segments(pmhip_s2* h, const float* tokens, const float* context, int L, int B, const uint8_t* ctx_seg_host,
                                         const uint32_t* tok_seg_host, float* logits_out, pmhip_stream stream) {
    ForwardCall c("s2_forward", h, tokens, context, L, B, logits_out, stream);
    c.keys.seg = ctx_seg_host; c.keys.tok = tok_seg_host;
    c.who = s2_forward_name(c.keys);
    return s2_forward_impl(c);
}

// ctx_w_host == NULL: exactly pmhip_s2_forward_segments
extern "C" int pmhip_s2_forward_weights(pmhip_s2* h, const float* tokens, const float* context, int L, int B, const uint8_t* ctx_seg_host,
                                        const uint32_t* tok_seg_host, const float* ctx_w_host, float* logits_out, pmhip_stream stream) {
    ForwardCall c("s2_forward", h, tokens, context, L, B, logits_out, stream);
    c.keys.seg = ctx_seg_host; c.keys.tok = tok_seg_host; c.keys.w = ctx_w_host;
    c.who = s2_forward_name(c.keys);
    return s2_forward_impl(c);
}

// the logits of pmhip_s2_forward_weights / _lens on the same arguments, and the chosen layers' cross-attention maps beside them
// (its messages carry its own name whatever key arrays came)
extern "C" int pmhip_s2_forward_maps(pmhip_s2* h, const float* tokens, const float* context, int L, int B, const int32_t* ctx_lens_host,
                                     const uint8_t* ctx_seg_host, const uint32_t* tok_seg_host, const float* ctx_w_host, uint64_t layer_bits,
                                     float* logits_out, float* maps_out, pmhip_stream stream) {
    PM_REQUIRE(maps_out, "s2_forward_maps: maps_out is NULL (pmhip_s2_forward_weights is the entry without maps)");
    ForwardCall c("s2_forward_maps", h, tokens, context, L, B, logits_out, stream);
    c.keys.lens = ctx_lens_host; c.keys.seg = ctx_seg_host; c.keys.tok = tok_seg_host; c.keys.w = ctx_w_host;
    c.layer_bits = layer_bits; c.maps_out = maps_out;
    return s2_forward_impl(c);
}

// One eager forward over B pairs: images [0, B) carry the source prompts, [B, 2B) the edited ones.  The layers of
// cross_bits run the edited half's cross-attention under control, the layers of self_bits its first self-attention on the source
// half's Q and K.  Everything is checked before anything is launched; the layers' sets carry the control for this one tower only.
static int s2_forward_control_impl(const char* who, pmhip_s2* h, const float* tokens, const float* context, int L, int B,
                                   const int32_t* ctx_lens_host, uint64_t cross_bits, uint64_t self_bits, const int32_t* row_map_host,
                                   const float* blend_host, const float* gain_host, float* logits_out, pmhip_stream stream,
                                   bool with_scores = false, uint64_t score_bits = 0, const float* w_src_host = nullptr,
                                   const float* w_edit_host = nullptr, float* scores = nullptr, int accumulate = 0) {
    PM_REQUIRE(h && tokens && logits_out && B > 0 && B <= (1 << 20), "%s: bad arguments", who);
    const int depth = h->cfg.tower.depth, B2 = 2 * B;
    PM_REQUIRE(context && L > 0, "%s: the control is that of the cross-attention: a context is required", who);
    if (with_scores)
        PM_REQUIRE(score_bits != 0 && w_src_host && w_edit_host && scores,
                   "%s: score_bits selects no layer, or w_src_host / w_edit_host / scores is NULL (pmhip_s2_forward_control is the entry without scores)", who);
    else
        PM_REQUIRE((cross_bits | self_bits) != 0, "%s: cross_bits and self_bits select no layer", who);
    PM_REQUIRE(depth >= 64 || ((cross_bits | self_bits) >> depth) == 0, "%s: cross_bits 0x%llx / self_bits 0x%llx select a layer at or above depth=%d",
               who, (unsigned long long)cross_bits, (unsigned long long)self_bits, depth);
    PM_REQUIRE(depth >= 64 || (score_bits >> depth) == 0, "%s: score_bits 0x%llx selects a layer at or above depth=%d", who,
               (unsigned long long)score_bits, depth);
    const int given = (row_map_host != nullptr) + (blend_host != nullptr) + (gain_host != nullptr);
    PM_REQUIRE(given == (cross_bits ? 3 : 0), "%s: row_map_host, blend_host and gain_host are required with cross_bits and refused without", who);
    PM_TRY(check_ctx_lens(who, ctx_lens_host, true, L, B2));
    const size_t n = (size_t)B * L;
    for (size_t i = 0; cross_bits && i < n; ++i) {
        const int b = (int)(i / L), j = (int)(i % L);
        PM_REQUIRE(row_map_host[i] < L, "%s: pair %d: row %d: source row %d must be below L=%d (negative: none)", who, b, j, (int)row_map_host[i], L);
        PM_REQUIRE(blend_host[i] >= 0.f && blend_host[i] <= 1.f, "%s: pair %d: row %d: blend %g must be in [0, 1]", who, b, j, (double)blend_host[i]);
        PM_REQUIRE(std::isfinite(gain_host[i]) && gain_host[i] >= 0.f, "%s: pair %d: row %d: gain %g must be finite and >= 0", who, b, j,
                   (double)gain_host[i]);
    }
    for (int b = 0; with_scores && b < B; ++b) {              // the phrase's rows: finite, >= 0, and something to look at in one half
        bool any = false;
        for (int half = 0; half < 2; ++half) {
            const float* w = (half ? w_edit_host : w_src_host) + (size_t)b * L;
            const int len = ctx_lens_host ? ctx_lens_host[half * B + b] : L;
            for (int j = 0; j < L; ++j) {
                PM_REQUIRE(std::isfinite(w[j]) && w[j] >= 0.f, "%s: pair %d: %s row %d: weight %g must be finite and >= 0", who, b,
                           half ? "edited" : "source", j, (double)w[j]);
                any |= j < len && w[j] > 0.f;
            }
        }
        PM_REQUIRE(any, "%s: pair %d: no row of the phrase has a positive weight below its length in either half", who, b);
    }
    hipStream_t s = (hipStream_t)stream;
    const int M = B2 * h->cfg.tokens;
    PM_TRY(s2_prepare_context(h, context, L, B2, s));
    PM_TRY(s2_set_ctx_lens(h, ctx_lens_host, L, B2, s));
    unsigned char* dctl = nullptr;
    unsigned char* dw = nullptr;
    const size_t part = (n * 4 + 15) & ~(size_t)15;
    if (cross_bits || with_scores) {                          // one trip through the control ring: row_map | blend | gain, then w_src | w_edit
        const size_t ctl_bytes = cross_bits ? 3 * part : 0, w_bytes = with_scores ? 2 * part : 0;
        if (cross_bits) WS(h->ws, "ctl.arrays", ctl_bytes, dctl);
        if (with_scores) WS(h->ws, "ctl.weights", w_bytes, dw);
        std::vector<unsigned char> packed(ctl_bytes + w_bytes, 0);
        if (cross_bits) {
            memcpy(packed.data(), row_map_host, n * 4);
            memcpy(packed.data() + part, blend_host, n * 4);
            memcpy(packed.data() + 2 * part, gain_host, n * 4);
        }
        if (with_scores) {
            memcpy(packed.data() + ctl_bytes, w_src_host, n * 4);
            memcpy(packed.data() + ctl_bytes + part, w_edit_host, n * 4);
        }
        PM_TRY(h->ctl_ring.reserve(ctl_bytes + w_bytes));
        PM_TRY(h->ctl_ring.acquire());
        if (cross_bits) PM_TRY(h->ctl_ring.stage(dctl, 0, packed.data(), ctl_bytes, s));
        if (with_scores) PM_TRY(h->ctl_ring.stage(dw, ctl_bytes, packed.data() + ctl_bytes, w_bytes, s));
        PM_TRY(h->ctl_ring.commit(s));
    }
    void* tp;
    PM_TRY(tok_buf(h, M, tp, s));
    PM_TRY(pmhip_convert_pad(tokens, h->cfg.embed_dim, tp, h->dtype, 64, M, s));
    struct Control {                                          // cleared on every way out
        std::vector<CrossKV>& kv;
        ~Control() {
            for (auto& ck : kv) {
                ck.ctl_map = nullptr; ck.ctl_blend = nullptr; ck.ctl_gain = nullptr; ck.ctl_self = false;
                ck.phr_w_src = nullptr; ck.phr_w_edit = nullptr; ck.phr_src = nullptr; ck.phr_edit = nullptr;
                ck.phr_scale = 1.f; ck.phr_accumulate = false;
            }
        }
    } control{h->cross};
    int tapped = 0;
    for (size_t l = 0; l < h->cross.size() && l < 64; ++l) tapped += (int)((score_bits >> l) & 1);
    bool first = true;
    for (size_t l = 0; l < h->cross.size() && l < 64; ++l) {
        CrossKV& ck = h->cross[l];
        if ((cross_bits >> l) & 1) {
            ck.ctl_map = reinterpret_cast<const int32_t*>(dctl);
            ck.ctl_blend = reinterpret_cast<const float*>(dctl + part);
            ck.ctl_gain = reinterpret_cast<const float*>(dctl + 2 * part);
        }
        ck.ctl_self = ((self_bits >> l) & 1) != 0;
        if (with_scores && ((score_bits >> l) & 1)) {
            ck.phr_w_src = reinterpret_cast<const float*>(dw);
            ck.phr_w_edit = reinterpret_cast<const float*>(dw + part);
            ck.phr_src = scores; ck.phr_edit = scores + (size_t)B * h->cfg.tokens;
            ck.phr_scale = 1.0f / (float)tapped; ck.phr_accumulate = !first || accumulate != 0;
            first = false;
        }
    }
    return s2_tower(h, tp, B2, logits_out, s);
}

extern "C" int pmhip_s2_forward_control(pmhip_s2* h, const float* tokens, const float* context, int L, int B, const int32_t* ctx_lens_host,
                                        uint64_t cross_bits, uint64_t self_bits, const int32_t* row_map_host, const float* blend_host,
                                        const float* gain_host, float* logits_out, pmhip_stream stream) {
    return s2_forward_control_impl("s2_forward_control", h, tokens, context, L, B, ctx_lens_host, cross_bits, self_bits, row_map_host, blend_host,
                                   gain_host, logits_out, stream);
}

// pmhip_s2_forward_control with the phrase-score tap: the layers of score_bits leave where the pair looks at the
// phrase in `scores` [2B, tokens], the source half in front.  cross_bits | self_bits == 0 is allowed here: the logits are then those
// of pmhip_s2_forward_lens.
extern "C" int pmhip_s2_forward_control_scores(pmhip_s2* h, const float* tokens, const float* context, int L, int B,
                                               const int32_t* ctx_lens_host, uint64_t cross_bits, uint64_t self_bits,
                                               const int32_t* row_map_host, const float* blend_host, const float* gain_host,
                                               uint64_t score_bits, const float* w_src_host, const float* w_edit_host, float* logits_out,
                                               float* scores, int accumulate, pmhip_stream stream) {
    return s2_forward_control_impl("s2_forward_control_scores", h, tokens, context, L, B, ctx_lens_host, cross_bits, self_bits, row_map_host,
                                   blend_host, gain_host, logits_out, stream, true, score_bits, w_src_host, w_edit_host, scores, accumulate);
}

namespace {
// The sample family's call record: the common head of its eight entries by the constructor, every optional feature at its neutral
// value (include/pmhip.h) until an entry assigns it.  `narrow` is the name the entry's messages carry when no wider feature is
// present: its own, or the *_lens entry's for the entries above that one.
struct SampleCall {
    const char* narrow; pmhip_s2* s2; pmhip_vqgan* vq; int64_t* ids; CtxKeys keys; int B;
    int topk; float temperature; int num_mask; const float* noise; uint64_t seed; uint32_t step; uint64_t image_base;
    float* img_out; int64_t* pred_out; float* score_out; pmhip_stream stream;
    int guided = 0; float guidance_scale = 0.f;
    float choice_t = 0.f; const float* choice_noise = nullptr;
    float top_p = 1.f;
    NegSet neg;
    SampleCall(const char* narrow_, pmhip_s2* s2_, pmhip_vqgan* vq_, int64_t* ids_, const float* context, int L, int B_, int topk_,
               float temperature_, int num_mask_, const float* noise_, uint64_t seed_, uint32_t step_, uint64_t image_base_, float* img_out_,
               int64_t* pred_out_, float* score_out_, pmhip_stream stream_)
        : narrow(narrow_), s2(s2_), vq(vq_), ids(ids_), keys(context, L), B(B_), topk(topk_), temperature(temperature_), num_mask(num_mask_),
          noise(noise_), seed(seed_), step(step_), image_base(image_base_), img_out(img_out_), pred_out(pred_out_), score_out(score_out_),
          stream(stream_) {}
};
}  // namespace

// The sample family's one builder: the record -> the checks, the context, the Step.
static int pipeline_sample_call(const SampleCall& c) {
    // (pm_check_top_p always reports under the nucleus entry's name)
    PM_TRY(pm_check_top_p("pipeline_sample_nucleus", c.top_p));
    // (the choice temperature's check: the nucleus entry's name when a mass came, the choice entry's otherwise)
    PM_TRY(pm_check_choice_t(call_name({{c.top_p != 1.f, "pipeline_sample_nucleus"}}, "pipeline_sample_choice"), c.choice_t));
    // (check_negative always reports under the negative entry's name)
    const bool schedule = false;                              // (a single step has no guidance schedule)
    PM_TRY(check_negative("pipeline_sample_negative", c.neg, schedule, c.guided != 0, c.keys.context && c.keys.L > 0, c.B));
    // (the entries above *_lens pass that entry's name as `narrow`: they report as *_lens when no wider feature is present)
    const char* who = call_name({{c.keys.w != nullptr, "pipeline_sample_weights"},
                                 {c.keys.seg || c.keys.tok, "pipeline_sample_segments"},
                                 {c.neg.context != nullptr, "pipeline_sample_negative"},
                                 {c.top_p != 1.f, "pipeline_sample_nucleus"},
                                 {c.choice_t != 0.f, "pipeline_sample_choice"}}, c.narrow);
    Step st;
    st.topk = c.topk; st.temperature = c.temperature; st.num_mask = c.num_mask; st.noise = c.noise;
    st.seed = c.seed; st.step = c.step; st.image_base = c.image_base;
    st.guidance = c.guided ? &c.guidance_scale : nullptr;
    if (c.choice_t != 0.f) { st.choice_t = c.choice_t; st.choice_noise = c.choice_noise; }     // 0: no given uniforms to ignore
    st.top_p = c.top_p;
    st.negative = c.neg.context != nullptr;
    PM_REQUIRE(c.s2 && c.ids && c.B > 0, "%s: bad arguments", who);
    PM_REQUIRE(!st.guidance || (c.keys.context && c.keys.L > 0), "%s: guidance needs a context (context NULL IS the unconditional branch)", who);
    CtxWeights cw;
    PM_TRY(check_context(who, c.keys, c.B, c.s2, cw));
    hipStream_t s = (hipStream_t)c.stream;
    PM_TRY(stage_context(c.s2, c.keys, cw, c.neg, c.B, s));
    return sample_step(c.s2, c.vq, c.ids, c.B, st, c.img_out, c.pred_out, c.score_out, s);
}

extern "C" int pmhip_pipeline_sample(pmhip_s2* s2, pmhip_vqgan* vq, int64_t* ids, const float* context, int L, int B,
                                     int topk, float temperature, int num_mask, const float* noise, uint64_t seed,
                                     uint32_t step, uint64_t image_base, float* img_out, int64_t* pred_out,
                                     float* score_out, pmhip_stream stream) {
    SampleCall c("pipeline_sample", s2, vq, ids, context, L, B, topk, temperature, num_mask, noise, seed, step, image_base, img_out, pred_out,
                 score_out, stream);
    return pipeline_sample_call(c);
}

extern "C" int pmhip_pipeline_sample_guided(pmhip_s2* s2, pmhip_vqgan* vq, int64_t* ids, const float* context, int L, int B,
                                            int topk, float temperature, int num_mask, const float* noise, uint64_t seed,
                                            uint32_t step, uint64_t image_base, float* img_out, int64_t* pred_out,
                                            float* score_out, float guidance_scale, pmhip_stream stream) {
    SampleCall c("pipeline_sample_guided", s2, vq, ids, context, L, B, topk, temperature, num_mask, noise, seed, step, image_base, img_out, pred_out,
                 score_out, stream);
    c.guided = 1; c.guidance_scale = guidance_scale;
    return pipeline_sample_call(c);
}

extern "C" int pmhip_pipeline_sample_lens(pmhip_s2* s2, pmhip_vqgan* vq, int64_t* ids, const float* context, int L, int B,
                                          const int32_t* ctx_lens_host, int topk, float temperature, int num_mask, const float* noise,
                                          uint64_t seed, uint32_t step, uint64_t image_base, float* img_out, int64_t* pred_out,
                                          float* score_out, int guided, float guidance_scale, pmhip_stream stream) {
    SampleCall c("pipeline_sample_lens", s2, vq, ids, context, L, B, topk, temperature, num_mask, noise, seed, step, image_base, img_out, pred_out,
                 score_out, stream);
    c.keys.lens = ctx_lens_host;
    c.guided = guided; c.guidance_scale = guidance_scale;
    return pipeline_sample_call(c);
}

// choice_t == 0: exactly pmhip_pipeline_sample_lens
extern "C" int pmhip_pipeline_sample_choice(pmhip_s2* s2, pmhip_vqgan* vq, int64_t* ids, const float* context, int L, int B,
                                            const int32_t* ctx_lens_host, int topk, float temperature, int num_mask, const float* noise,
                                            uint64_t seed, uint32_t step, uint64_t image_base, float* img_out, int64_t* pred_out,
                                            float* score_out, int guided, float guidance_scale, float choice_t, const float* choice_noise,
                                            pmhip_stream stream) {
    SampleCall c("pipeline_sample_lens", s2, vq, ids, context, L, B, topk, temperature, num_mask, noise, seed, step, image_base, img_out, pred_out,
                 score_out, stream);
    c.keys.lens = ctx_lens_host;
    c.guided = guided; c.guidance_scale = guidance_scale;
    c.choice_t = choice_t; c.choice_noise = choice_noise;
    return pipeline_sample_call(c);
}

// top_p == 1: exactly pmhip_pipeline_sample_choice
extern "C" int pmhip_pipeline_sample_nucleus(pmhip_s2* s2, pmhip_vqgan* vq, int64_t* ids, const float* context, int L, int B,
                                             const int32_t* ctx_lens_host, int topk, float temperature, int num_mask, const float* noise,
                                             uint64_t seed, uint32_t step, uint64_t image_base, float* img_out, int64_t* pred_out,
                                             float* score_out, int guided, float guidance_scale, float choice_t, const float* choice_noise,
                                             float top_p, pmhip_stream stream) {
    SampleCall c("pipeline_sample_lens", s2, vq, ids, context, L, B, topk, temperature, num_mask, noise, seed, step, image_base, img_out, pred_out,
                 score_out, stream);
    c.keys.lens = ctx_lens_host;
    c.guided = guided; c.guidance_scale = guidance_scale;
    c.choice_t = choice_t; c.choice_noise = choice_noise;
    c.top_p = top_p;
    return pipeline_sample_call(c);
}

// neg_context == NULL: exactly pmhip_pipeline_sample_nucleus
extern "C" int pmhip_pipeline_sample_negative(pmhip_s2* s2, pmhip_vqgan* vq, int64_t* ids, const float* context, int L, int B,
                                              const int32_t* ctx_lens_host, int topk, float temperature, int num_mask, const float* noise,
                                              uint64_t seed, uint32_t step, uint64_t image_base, float* img_out, int64_t* pred_out,
                                              float* score_out, int guided, float guidance_scale, float choice_t, const float* choice_noise,
                                              float top_p, const float* neg_context, int Ln, const int32_t* neg_lens_host,
                                              pmhip_stream stream) {
    SampleCall c("pipeline_sample_lens", s2, vq, ids, context, L, B, topk, temperature, num_mask, noise, seed, step, image_base, img_out, pred_out,
                 score_out, stream);
    c.keys.lens = ctx_lens_host;
    c.guided = guided; c.guidance_scale = guidance_scale;
    c.choice_t = choice_t; c.choice_noise = choice_noise;
    c.top_p = top_p;
    c.neg.context = neg_context; c.neg.Ln = Ln; c.neg.lens = neg_lens_host;
    return pipeline_sample_call(c);
}

// ctx_seg_host == NULL and tok_seg_host == NULL: exactly pmhip_pipeline_sample_negative
extern "C" int pmhip_pipeline_sample_segments(pmhip_s2* s2, pmhip_vqgan* vq, int64_t* ids, const float* context, int L, int B,
                                              const int32_t* ctx_lens_host, int topk, float temperature, int num_mask, const float* noise,
                                              uint64_t seed, uint32_t step, uint64_t image_base, float* img_out, int64_t* pred_out,
                                              float* score_out, int guided, float guidance_scale, float choice_t, const float* choice_noise,
                                              float top_p, const float* neg_context, int Ln, const int32_t* neg_lens_host,
                                              const uint8_t* ctx_seg_host, const uint32_t* tok_seg_host, pmhip_stream stream) {
    SampleCall c("pipeline_sample_lens", s2, vq, ids, context, L, B, topk, temperature, num_mask, noise, seed, step, image_base, img_out, pred_out,
                 score_out, stream);
    c.keys.lens = ctx_lens_host; c.keys.seg = ctx_seg_host; c.keys.tok = tok_seg_host;
    c.guided = guided; c.guidance_scale = guidance_scale;
    c.choice_t = choice_t; c.choice_noise = choice_noise;
    c.top_p = top_p;
    c.neg.context = neg_context; c.neg.Ln = Ln; c.neg.lens = neg_lens_host;
    return pipeline_sample_call(c);
}

// ctx_w_host == NULL: exactly pmhip_pipeline_sample_segments
extern "C" int pmhip_pipeline_sample_weights(pmhip_s2* s2, pmhip_vqgan* vq, int64_t* ids, const float* context, int L, int B,
                                             const int32_t* ctx_lens_host, int topk, float temperature, int num_mask, const float* noise,
                                             uint64_t seed, uint32_t step, uint64_t image_base, float* img_out, int64_t* pred_out,
                                             float* score_out, int guided, float guidance_scale, float choice_t, const float* choice_noise,
                                             float top_p, const float* neg_context, int Ln, const int32_t* neg_lens_host,
                                             const uint8_t* ctx_seg_host, const uint32_t* tok_seg_host, const float* ctx_w_host,
                                             pmhip_stream stream) {
    SampleCall c("pipeline_sample_lens", s2, vq, ids, context, L, B, topk, temperature, num_mask, noise, seed, step, image_base, img_out, pred_out,
                 score_out, stream);
    c.keys.lens = ctx_lens_host; c.keys.seg = ctx_seg_host; c.keys.tok = tok_seg_host; c.keys.w = ctx_w_host;
    c.guided = guided; c.guidance_scale = guidance_scale;
    c.choice_t = choice_t; c.choice_noise = choice_noise;
    c.top_p = top_p;
    c.neg.context = neg_context; c.neg.Ln = Ln; c.neg.lens = neg_lens_host;
    return pipeline_sample_call(c);
}

// process-wide: the runtime reads AMD_DIRECT_DISPATCH once when it starts, so does this
static bool direct_dispatch_off() {
    static const bool off = [] { const char* e = getenv("AMD_DIRECT_DISPATCH"); return e && atoi(e) == 0; }();
    return off;
}

namespace {

// The generate family's call record: the common head of its nine entries by the constructor, every optional feature at its
// neutral value (include/pmhip.h) until an entry assigns it.  `narrow` is the name the entry's messages carry when no wider feature
// is present: its own, or the *_lens entry's for the entries above that one.
struct GenCall {
    const char* narrow; pmhip_s2* s2; pmhip_vqgan* vq; int64_t* ids; CtxKeys keys; int B, T;
    const float* temps_host; const int* nmask_host; const unsigned char* decode_host;
    int topk; uint64_t seed, image_base; float* imgs_out; int use_graph; pmhip_stream stream;
    float* imgs_host; size_t host_stride; pmhip_stream copy_stream;
    int guided = 0; float guidance_scale = 0.f;   // one scale for the loop (ignored under a schedule)
    const float* ctemps = nullptr;          // host [T] or NULL: the steps' choice temperatures (pmhip_pipeline_generate_choice)
    float top_p = 1.f;                      // every step's nucleus mass (pmhip_pipeline_generate_nucleus); 1: no filter
    // pmhip_pipeline_generate_negative: the negative context [B, Ln, context_dim] with its host lengths [B] (or NULL), and the
    // steps' guidance scales, host [T] (then the scalar is ignored)
    NegSet neg;
    const float* gscales = nullptr;
    // pmhip_pipeline_generate_edit: the re-masking counts per step and image, host [T][B], instead of nmask_host (then NULL); a
    // decoded step of such a loop decodes the merged ids
    const int32_t* nmask_img = nullptr;
    GenCall(const char* narrow_, pmhip_s2* s2_, pmhip_vqgan* vq_, int64_t* ids_, const float* context, int L, int B_, int T_,
            const float* temps_host_, const int* nmask_host_, const unsigned char* decode_host_, int topk_, uint64_t seed_, uint64_t image_base_,
            float* imgs_out_, int use_graph_, pmhip_stream stream_, float* imgs_host_, size_t host_stride_, pmhip_stream copy_stream_)
        : narrow(narrow_), s2(s2_), vq(vq_), ids(ids_), keys(context, L), B(B_), T(T_), temps_host(temps_host_), nmask_host(nmask_host_),
          decode_host(decode_host_), topk(topk_), seed(seed_), image_base(image_base_), imgs_out(imgs_out_), use_graph(use_graph_),
          stream(stream_), imgs_host(imgs_host_), host_stride(host_stride_), copy_stream(copy_stream_) {}
    const float* guidance() const { return guided && !gscales ? &guidance_scale : nullptr; }   // the loop's one scale, or NULL
    bool any_guidance() const { return guidance() || gscales; }
    bool decodes(int t) const { return decode_host && decode_host[t]; }
};

// A unit = one executable graph.  Normally a unit is a SEGMENT [t0, t1) (t1 - 1 is a decoded step, or the end of the loop) whose
// last step decodes in place and whose image is complete when the unit is.  Small batches (B * tokens <= overlap_rows: every
// kernel is a few dozen workgroups on 256 CUs and the loop is one long dependent chain) DEFER the decode instead: the ViT decode
// of a segment's last step opens the NEXT unit on a side stream, beside that unit's first tower pass (which only needs the ids),
// and is joined before the first sampling kernel overwrites the predictions it reads; a last unit without steps decodes the
// final image.  Same kernels, same inputs: bit-identical images, one unit later.
struct Unit { int t0, t1, decode_first, delivers; bool decode_inline; };

std::vector<Unit> plan_units(const GenCall& c, bool overlap) {
    std::vector<Unit> units;
    int d = 0, pend = -1;
    for (int t = 0, t0 = 0; t < c.T; ++t) {
        const bool dec = c.decodes(t);
        if (!dec && t != c.T - 1) continue;
        if (overlap) { units.push_back({t0, t + 1, pend, pend, false}); pend = dec ? d++ : -1; }
        else units.push_back({t0, t + 1, -1, dec ? d++ : -1, true});
        t0 = t + 1;
    }
    if (pend >= 0) units.push_back({c.T, c.T, pend, pend, false});
    return units;
}

// Image d is complete on `s` after the step that decodes it.  Device destination: a copy on `s`.  Host destination: the
// copy must run on the copy stream UNDER the following steps, but it is not made to wait there by a cross-stream event:
// a barrier packet parked at the head of the copy queue until a whole segment has run starves the other lane's queue
// on this part (measured: two lanes with such waits run one after the other, 164 vs 138 ms per call).  Instead the HOST
// paces the loop, like the reference's blocking `img.cpu()` per saved step (generate.py:195-196): once the next
// segment is queued it waits for image d's event and enqueues a copy that can start at once.  The caller runs
// concurrent lanes from one thread each (the ctypes call drops the GIL).
// Per unit or step, in this order: run it, flush(), deliver().
struct HostDelivery {
    const GenCall& c;
    hipStream_t s, cs;
    size_t img_elems;
    int n_dec;
    bool handle_buffer;                                       // the images are produced into the handle's "gen.imgs"
    int pending = -1;                                         // decoded image whose host copy has not been enqueued yet
    const float* pending_src = nullptr;
    int flush() {
        if (pending < 0) return PMHIP_OK;
        if (cs != s) PM_HIP(hipEventSynchronize(c.s2->img_ready[pending].h));
        PM_HIP(hipMemcpyAsync(c.imgs_host + (size_t)pending * c.host_stride, pending_src, img_elems * 4, hipMemcpyDeviceToHost, cs));
        if (pending == n_dec - 1 && handle_buffer) {
            PM_HIP(hipEventRecord(c.s2->host_copied.h, cs));
            c.s2->host_copy_pending = cs != s;
        }
        pending = -1;
        return PMHIP_OK;
    }
    int deliver(int d, const float* src) {
        if (c.imgs_out && src != c.imgs_out + (size_t)d * img_elems)
            PM_HIP(hipMemcpyAsync(c.imgs_out + (size_t)d * img_elems, src, img_elems * 4, hipMemcpyDeviceToDevice, s));
        if (c.imgs_host) {
            if (cs != s) PM_HIP(hipEventRecord(c.s2->img_ready[d].h, s));
            pending = d;
            pending_src = src;
        }
        return PMHIP_OK;
    }
};

// A call of the generate family beyond its record: the name its messages carry, the forms its checks found, and what the
// preparation left in the workspace.  pipeline_generate fills it phase by phase: gen_checks, gen_prepare, then one of the two loops.
struct GenLoop {
    const GenCall& c;
    const char* who;
    const bool edit, sched, neg;
    bool choice = false;                                      // a step has a choice temperature other than 0
    CtxWeights cw;
    hipStream_t s = nullptr, cs = nullptr;
    bool graph = false, from_mask = false, share0 = false;
    size_t img_elems = 0, n_ids = 0;
    int n_dec = 0;
    float* gimgs = nullptr;                                   // the handle-owned image buffer "gen.imgs", or NULL
    PmGenParams* gparams = nullptr;                           // "gen.params" (stage_gen_params)
    int32_t* gcounts = nullptr;                               // "gen.counts" (stage_gen_counts)
    // the name: the widest feature present, otherwise the entry's narrow name
    // (the edit entry's calls carry its own name wherever the negative entry's would stand)
    // (the entries above *_lens pass that entry's name as `narrow`: they report as *_lens when no wider feature is present)
    explicit GenLoop(const GenCall& c_)
        : c(c_),
          who(call_name({{c_.keys.w != nullptr, "pipeline_generate_weights"},
                         {c_.keys.seg || c_.keys.tok, "pipeline_generate_segments"},
                         {c_.nmask_img != nullptr, c_.narrow},
                         {c_.neg.context || c_.gscales, "pipeline_generate_negative"},
                         {c_.top_p != 1.f, "pipeline_generate_nucleus"},
                         {c_.ctemps != nullptr, "pipeline_generate_choice"}}, c_.narrow)),
          edit(c_.nmask_img != nullptr), sched(c_.gscales != nullptr), neg(c_.neg.context != nullptr) {}
};

// checks: every host check of the loop, in order, before anything is launched
int gen_checks(GenLoop& g) {
    const GenCall& c = g.c;
    pmhip_s2* s2 = c.s2;
    const int B = c.B, T = c.T;
    // (pm_check_top_p always reports under the nucleus entry's name)
    PM_TRY(pm_check_top_p("pipeline_generate_nucleus", c.top_p));
    // (check_negative and the schedule's checks report under the negative entry's name, except under the edit entry, which uses its own)
    const char* neg_who = call_name({{g.edit, c.narrow}}, "pipeline_generate_negative");
    PM_TRY(check_negative(neg_who, c.neg, g.sched, c.guided != 0, c.keys.context && c.keys.L > 0, B));
    if (g.sched) {
        PM_REQUIRE(T <= PM_MAX_STEPS, "%s: a guidance schedule serves at most %d steps, T=%d", neg_who, PM_MAX_STEPS, T);
        for (int t = 0; t < T; ++t) PM_REQUIRE(std::isfinite(c.gscales[t]), "%s: step %d: the guidance scale must be finite", neg_who, t);
    }
    // (the loop's first check of its arguments says pipeline_generate, whichever entry was called)
    PM_REQUIRE(s2 && c.ids && B > 0 && T > 0 && c.temps_host && (c.nmask_host || g.edit), "pipeline_generate: bad arguments");
    if (g.edit) {
        PM_REQUIRE(!(c.use_graph & PMHIP_GENERATE_FROM_MASK), "%s: an edit starts from the caller's ids, the from-mask flag is refused", g.who);
        for (int t = 0; t < T; ++t)
            for (int b = 0; b < B; ++b)
                PM_REQUIRE(c.nmask_img[(size_t)t * B + b] >= 0 && c.nmask_img[(size_t)t * B + b] <= s2->cfg.tokens,
                           "%s: step %d, image %d: the re-masking count %d must be in [0, %d]", g.who, t, b, c.nmask_img[(size_t)t * B + b],
                           s2->cfg.tokens);
    }
    // (the guidance-needs-a-context message always says pipeline_generate_guided)
    PM_REQUIRE(!c.any_guidance() || (c.keys.context && c.keys.L > 0),
               "pipeline_generate_guided: guidance needs a context (context NULL IS the unconditional branch)");
    PM_TRY(check_context(g.who, c.keys, B, s2, g.cw));
    // the choice temperatures; all zero IS the loop without them (same kernels, same graphs)
    for (int t = 0; c.ctemps && t < T; ++t) {
        PM_TRY(pm_check_choice_t(g.who, c.ctemps[t]));
        g.choice = g.choice || c.ctemps[t] != 0.f;
    }
    return PMHIP_OK;
}

// preparation: the contexts (once per loop, eager: the device memory the -- captured -- cross-attention launches read), the decode
// plan, the loop's form, the events of a host delivery and the handle-owned image buffer
int gen_prepare(GenLoop& g) {
    const GenCall& c = g.c;
    pmhip_s2* s2 = c.s2; pmhip_vqgan* vq = c.vq;
    const int B = c.B, T = c.T;
    hipStream_t s = g.s = (hipStream_t)c.stream;
    g.cs = c.copy_stream ? (hipStream_t)c.copy_stream : s;
    PM_TRY(stage_context(s2, c.keys, g.cw, c.neg, B, s));
    if (vq) g.img_elems = (size_t)B * vq->cfg.channels * vq->cfg.image_size * vq->cfg.image_size;
    for (int t = 0; t < T; ++t) g.n_dec += c.decodes(t) ? 1 : 0;
    PM_REQUIRE(g.n_dec == 0 || (vq && (c.imgs_out || c.imgs_host)), "pipeline_generate: decode requested without vqgan / an image destination");
    PM_REQUIRE(!c.imgs_host || c.host_stride >= g.img_elems, "pipeline_generate: host_stride smaller than one image batch");
    // AMD_DIRECT_DISPATCH=0 (the runtime mode without the busy-polling helper thread): hipGraph replay is broken there on ROCm 7.2
    // -- tools/hwtests/graph_dispatch_mode.hip, 39 of 40 replays of a chain of dependent kernels wrong with none of this library's
    // code involved -- so the loop stays eager in that mode whatever the caller asked for (same results, bit for bit)
    // pmhip_s2_switches reports the downgrade (bit 5) so that a caller can tell which mode ran
    g.graph = (c.use_graph & PMHIP_GENERATE_GRAPH) && !g_pm_timing_on.load() && T <= PM_MAX_STEPS && !direct_dispatch_off();
    // PMHIP_GENERATE_FROM_MASK: the loop starts from the all-mask state -- the library writes that state itself, so the claim
    // cannot be false -- and, without a context, step 0 samples from the handle's shared step-0 logits instead of running the tower
    // (step0_tower_once).  Not while per-kernel timing is on: the timed pass accounts for the work of all T tower passes.
    g.from_mask = (c.use_graph & PMHIP_GENERATE_FROM_MASK) != 0;
    g.share0 = g.from_mask && !c.keys.context && !c.guidance() && !g_pm_timing_on.load();
    g.n_ids = (size_t)B * s2->cfg.tokens;
    if (g.share0 && s2->s0_valid) {
        ++s2->s0_hits;
        if (s != s2->s0_stream) PM_HIP(hipStreamWaitEvent(s, s2->s0_ready.h, 0));
    }
    if (c.imgs_host) {
        // PMHIP_BLOCKING_WAIT=1 (read when the handle is created): the lane's host thread SLEEPS in hipEventSynchronize while its
        // segment runs instead of spinning -- frees a core per lane on a host that is short of them, at 0.6 ms of wake-up latency
        // per saved image (measured: the drop-in generate() 151 vs 141 ms per call), hence off by default
        const unsigned evflags = hipEventDisableTiming | (s2->sw.blocking_wait ? hipEventBlockingSync : 0u);
        hipEvent_t e;
        PM_TRY(s2->host_copied.get(evflags, e));
        if ((int)s2->img_ready.size() < g.n_dec) s2->img_ready.resize(g.n_dec);
        for (int d = 0; d < g.n_dec; ++d) PM_TRY(s2->img_ready[d].get(evflags, e));
    }
    // images are produced into a handle-owned buffer when a graph bakes the pointer in or when the caller only wants the
    // host copy; that buffer must not be overwritten while the previous call's last device-to-host copy still reads it
    if (g.n_dec && (g.graph || !c.imgs_out)) {
        WS(s2->ws, "gen.imgs", (size_t)g.n_dec * g.img_elems * 4 + 16, g.gimgs);
        if (s2->host_copy_pending) { PM_HIP(hipStreamWaitEvent(s, s2->host_copied.h, 0)); s2->host_copy_pending = false; }
    }
    return PMHIP_OK;
}

// staging: the device parameter block -- what the kernels of a replayed loop read their per-call values from, and, eager or
// replayed, where the combine launches of a loop with a guidance schedule read their scales (one kernel form for eager, capture and
// replay)
int stage_gen_params(GenLoop& g) {
    const GenCall& c = g.c;
    pmhip_s2* s2 = c.s2;
    hipStream_t s = g.s;
    WS(s2->ws, "gen.params", sizeof(PmGenParams), g.gparams);
    PmGenParams hp;
    hp.seed = c.seed;
    hp.row_base = c.image_base * (uint64_t)s2->cfg.tokens;
    for (int t = 0; t < c.T; ++t) {
        hp.temps[t] = c.temps_host[t]; hp.nmask[t] = g.edit ? 0 : c.nmask_host[t]; hp.ctemps[t] = g.choice ? c.ctemps[t] : 0.f;
        hp.gscales[t] = g.sched ? c.gscales[t] : 0.f;
    }
    // a loop stages what it always staged: without choice temperatures the block up to ctemps, without a guidance schedule the
    // block up to gscales -- none of its kernels reads what lies behind
    const size_t hp_bytes = g.sched ? sizeof hp : g.choice ? offsetof(PmGenParams, gscales) : offsetof(PmGenParams, ctemps);
    PM_TRY(s2->params_ring.reserve(sizeof hp));
    PM_TRY(s2->params_ring.acquire());
    PM_TRY(s2->params_ring.stage(g.gparams, 0, &hp, hp_bytes, s));
    return s2->params_ring.commit(s);
}

// ... and the edit loop's count table, T * B int32 at a fixed address: step t's re-masking launch -- eager, captured or replayed --
// reads its B counts at gcounts + t * B, so a graph bakes in the address and never the counts.  Refreshed per call like the block above.
int stage_gen_counts(GenLoop& g) {
    const GenCall& c = g.c;
    pmhip_s2* s2 = c.s2;
    hipStream_t s = g.s;
    const size_t bytes = ((size_t)c.T * c.B * 4 + 15) & ~(size_t)15;
    WS(s2->ws, "gen.counts", bytes, g.gcounts);
    std::vector<int32_t> padded(bytes / 4, 0);
    std::copy(c.nmask_img, c.nmask_img + (size_t)c.T * c.B, padded.begin());
    PM_TRY(s2->counts_ring.reserve(bytes));
    PM_TRY(s2->counts_ring.acquire());
    PM_TRY(s2->counts_ring.stage(g.gcounts, 0, padded.data(), bytes, s));
    return s2->counts_ring.commit(s);
}

// The Step of loop step t, for both loops.  from_params: the per-call scalars (temperature, mask count, seed, row base, choice
// temperature) come from the device parameter block -- the graph loop, whose graphs serve every call -- instead of from the call.
Step gen_step(const GenLoop& g, int t, bool from_params) {
    const GenCall& c = g.c;
    Step st;
    st.topk = c.topk;
    st.step = (uint32_t)t;
    st.shared0 = g.share0 && t == 0;
    st.guidance = c.guidance();
    if (from_params) {
        st.gp = g.gparams;
        st.choice_params = g.choice;
    } else {
        st.temperature = c.temps_host[t]; st.num_mask = g.edit ? 0 : c.nmask_host[t];
        st.seed = c.seed; st.image_base = c.image_base;
        if (g.choice) st.choice_t = c.ctemps[t];              // 0 (the last step of an annealed loop): the plain launch, the same keys
    }
    st.top_p = c.top_p;
    st.negative = g.neg;
    if (g.sched) st.guidance_dev = &g.gparams->gscales[t];
    if (g.edit) { st.counts = g.gcounts + (size_t)t * c.B; st.decode_merged = c.decodes(t); }
    return st;
}

// the tower half of a step
int gen_tower(const GenLoop& g, const int64_t* from, const Step& st, hipStream_t on) {
    return st.shared0 ? step0_tower_once(g.c.s2, from, g.c.B, on) : step_tower(g.c.s2, from, g.c.B, st, on);
}

// the eager loop: every step on the caller's ids, its scalars from the call
int gen_eager_loop(GenLoop& g) {
    const GenCall& c = g.c;
    pmhip_s2* s2 = c.s2;
    hipStream_t s = g.s;
    HostDelivery out{c, s, g.cs, g.img_elems, g.n_dec, g.gimgs != nullptr};
    int d = 0;
    if (g.sched) PM_TRY(stage_gen_params(g));
    if (g.edit) PM_TRY(stage_gen_counts(g));
    if (g.from_mask) PM_TRY(fill_ids_async(c.ids, (int64_t)s2->cfg.n_embed, g.n_ids, s));
    for (int t = 0; t < c.T; ++t) {
        const bool dec = c.decodes(t);
        float* img = !dec ? nullptr : (g.gimgs ? g.gimgs : c.imgs_out) + (size_t)d * g.img_elems;
        const Step st = gen_step(g, t, false);
        PM_TRY(gen_tower(g, c.ids, st, s));
        PM_TRY(step_tail(s2, c.vq, c.ids, c.B, st, img, nullptr, nullptr, s));
        PM_TRY(out.flush());                                   // the previous image, now that one more step is queued behind it
        if (dec) PM_TRY(out.deliver(d++, img));
    }
    return out.flush();
}

// The graph cache key of a loop: everything that shapes its launches, nothing a launch reads from device memory.
std::string gen_key(const GenLoop& g, bool overlap) {
    const GenCall& c = g.c;
    std::string key = "B" + std::to_string(c.B) + "T" + std::to_string(c.T) + "k" + std::to_string(c.topk) + "L" +
                      std::to_string(c.keys.context ? c.keys.L : 0) + "v" + std::to_string(c.vq ? c.vq->uid : 0) + "f" +
                      std::to_string(c.s2->sw.key() * 16 + (c.vq ? c.vq->sw.key() : 0));
    if (c.guidance()) {                                       // the scale is a kernel argument of the captured combine: one graph per value
        unsigned bits;
        memcpy(&bits, c.guidance(), 4);
        key += "g" + std::to_string(bits);
    } else if (g.sched) {                                     // the combine reads &gparams->gscales[t]: an address, so one graph serves every schedule
        key += "gs";
    }
    // the second tower attends to the negative set: Ln shapes its cross-attention launches, lengths pick their per-image form
    if (g.neg) key += "N" + std::to_string(c.neg.Ln) + (c.neg.lens ? "l" : "");
    key += "d";
    for (int t = 0; t < c.T; ++t) key += c.decodes(t) ? '1' : '0';
    key += overlap ? "o1" : "o0";
    if (g.from_mask) key += "m";                              // step 0 is captured without its tower: never shared with an unflagged loop
    if (c.keys.lens && !c.keys.w) key += "n";                 // the per-image form of the cross-attention kernel; the lengths are not in the key
    if (c.keys.seg) key += "s";                               // the per-query form of the cross-attention kernel; the layout of regions is not in the key
    if (c.keys.w) key += "w";                                 // the weighted form of the cross-attention kernel; neither the weights nor the layout are in the key
    if (g.edit) key += "e";                                   // the counts form of the re-masking kernel and the merged decode; the counts are not in the key
    if (g.choice) key += "c";                                 // the choice form of the re-masking kernel; the temperatures are not in the key
    if (c.top_p < 1.f) {                                      // the nucleus kernel, the mass its argument in the captured graph: one graph per value
        unsigned bits;
        memcpy(&bits, &c.top_p, 4);
        key += "p" + std::to_string(bits);
    }
    return key;
}

// The hipGraph loop.  The T-step loop is a chain of graphs, one per SEGMENT (the steps up to and including a decoded
// one), whose kernels read the per-call scalars (temperatures, mask counts, seed, row base) from a device parameter
// block and whose ids / image pointers are handle-owned buffers, so the same executable graphs serve every call with
// this structure; between two segments the finished image starts its way to the host.
int gen_graph_loop(GenLoop& g) {
    const GenCall& c = g.c;
    pmhip_s2* s2 = c.s2; pmhip_vqgan* vq = c.vq;
    const int B = c.B;
    hipStream_t s = g.s;
    HostDelivery out{c, s, g.cs, g.img_elems, g.n_dec, g.gimgs != nullptr};
    const size_t ids_bytes = g.n_ids * 8;
    int64_t* gids;
    WS(s2->ws, "gen.ids", ids_bytes, gids);
    PM_TRY(stage_gen_params(g));
    if (g.edit) PM_TRY(stage_gen_counts(g));
    if (g.from_mask) PM_TRY(fill_ids_async(gids, (int64_t)s2->cfg.n_embed, g.n_ids, s));
    else PM_TRY(copy16_async(gids, c.ids, ids_bytes, s));

    // (no deferred decode when the caller runs other lanes beside this one -- PMHIP_GENERATE_CONCURRENT_LANES: the chip is full
    // then, and a third and fourth stream of kernels costs 5-17 % at 15-16 images per lane, profiles/r05_g_*)
    const bool overlap = vq && g.n_dec > 0 && s2->sw.overlap_rows > 0 && (long long)B * s2->cfg.tokens <= s2->sw.overlap_rows &&
                         !(c.use_graph & PMHIP_GENERATE_CONCURRENT_LANES);
    const std::vector<Unit> units = plan_units(c, overlap);
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    if (overlap) {
        PM_TRY(s2->side_stream.get(hipStreamNonBlocking, side));
        PM_TRY(s2->ev_fork.get(hipEventDisableTiming, ev_fork));
        PM_TRY(s2->ev_join.get(hipEventDisableTiming, ev_join));
    }
    float* const gimgs = g.gimgs;
    const size_t img_elems = g.img_elems;

    auto run_unit = [&](hipStream_t on, size_t i) -> int {
        const Unit& u = units[i];
        bool need_join = false;
        if (u.decode_first >= 0) {
            float* img = gimgs + (size_t)u.decode_first * img_elems;
            if (u.t1 > u.t0) {                                // fork: the pending decode runs beside this unit's first tower pass
                PM_HIP(hipEventRecord(ev_fork, on));
                PM_HIP(hipStreamWaitEvent(side, ev_fork, 0));
                PM_TRY(decode_pred(s2, vq, B, img, side));
                PM_HIP(hipEventRecord(ev_join, side));
                need_join = true;
            } else {
                PM_TRY(decode_pred(s2, vq, B, img, on));
            }
        }
        for (int t = u.t0; t < u.t1; ++t) {
            const Step st = gen_step(g, t, true);
            PM_TRY(gen_tower(g, gids, st, on));
            if (need_join) { PM_HIP(hipStreamWaitEvent(on, ev_join, 0)); need_join = false; }   // before `s2.pred` is overwritten
            float* img = (u.decode_inline && c.decodes(t)) ? gimgs + (size_t)u.delivers * img_elems : nullptr;
            PM_TRY(step_tail(s2, vq, gids, B, st, img, nullptr, nullptr, on));
        }
        return PMHIP_OK;
    };
    PM_TRY(run_graphs(s2, vq, s2->graphs[gen_key(g, overlap)], units.size(), s, run_unit, [&](size_t i) -> int {
        PM_TRY(out.flush());
        if (units[i].delivers >= 0) PM_TRY(out.deliver(units[i].delivers, gimgs + (size_t)units[i].delivers * img_elems));
        return PMHIP_OK;
    }));
    PM_TRY(copy16_async(c.ids, gids, ids_bytes, s));
    return out.flush();
}

// The generate family's one builder: the record -> the checks, the preparation, one of the two loops.
int pipeline_generate(const GenCall& c) {
    GenLoop g(c);
    PM_TRY(gen_checks(g));
    PM_TRY(gen_prepare(g));
    return g.graph ? gen_graph_loop(g) : gen_eager_loop(g);
}

}  // namespace

extern "C" int pmhip_pipeline_generate(pmhip_s2* s2, pmhip_vqgan* vq, int64_t* ids, const float* context, int L, int B,
                                       int T, const float* temps_host, const int* nmask_host,
                                       const unsigned char* decode_host, int topk, uint64_t seed, uint64_t image_base,
                                       float* imgs_out, int use_graph, pmhip_stream stream, float* imgs_host,
                                       size_t host_stride, pmhip_stream copy_stream) {
    GenCall c("pipeline_generate", s2, vq, ids, context, L, B, T, temps_host, nmask_host, decode_host, topk, seed, image_base,
              imgs_out, use_graph, stream, imgs_host, host_stride, copy_stream);
    return pipeline_generate(c);
}

extern "C" int pmhip_pipeline_generate_guided(pmhip_s2* s2, pmhip_vqgan* vq, int64_t* ids, const float* context, int L, int B,
                                              int T, const float* temps_host, const int* nmask_host,
                                              const unsigned char* decode_host, int topk, uint64_t seed, uint64_t image_base,
                                              float* imgs_out, int use_graph, pmhip_stream stream, float* imgs_host,
                                              size_t host_stride, pmhip_stream copy_stream, float guidance_scale) {
    GenCall c("pipeline_generate", s2, vq, ids, context, L, B, T, temps_host, nmask_host, decode_host, topk, seed, image_base,
              imgs_out, use_graph, stream, imgs_host, host_stride, copy_stream);
    c.guided = 1; c.guidance_scale = guidance_scale;
    return pipeline_generate(c);
}

extern "C" int pmhip_pipeline_generate_lens(pmhip_s2* s2, pmhip_vqgan* vq, int64_t* ids, const float* context, int L, int B,
                                            const int32_t* ctx_lens_host, int T, const float* temps_host, const int* nmask_host,
                                            const unsigned char* decode_host, int topk, uint64_t seed, uint64_t image_base,
                                            float* imgs_out, int use_graph, pmhip_stream stream, float* imgs_host, size_t host_stride,
                                            pmhip_stream copy_stream, int guided, float guidance_scale) {
    GenCall c("pipeline_generate_lens", s2, vq, ids, context, L, B, T, temps_host, nmask_host, decode_host, topk, seed, image_base,
              imgs_out, use_graph, stream, imgs_host, host_stride, copy_stream);
    c.keys.lens = ctx_lens_host;
    c.guided = guided; c.guidance_scale = guidance_scale;
    return pipeline_generate(c);
}

extern "C" int pmhip_pipeline_generate_choice(pmhip_s2* s2, pmhip_vqgan* vq, int64_t* ids, const float* context, int L, int B,
                                              const int32_t* ctx_lens_host, int T, const float* temps_host, const int* nmask_host,
                                              const unsigned char* decode_host, int topk, uint64_t seed, uint64_t image_base,
                                              float* imgs_out, int use_graph, pmhip_stream stream, float* imgs_host, size_t host_stride,
                                              pmhip_stream copy_stream, int guided, float guidance_scale, const float* ctemps_host) {
    GenCall c("pipeline_generate_lens", s2, vq, ids, context, L, B, T, temps_host, nmask_host, decode_host, topk, seed, image_base,
              imgs_out, use_graph, stream, imgs_host, host_stride, copy_stream);
    c.keys.lens = ctx_lens_host;
    c.guided = guided; c.guidance_scale = guidance_scale;
    c.ctemps = ctemps_host;
    return pipeline_generate(c);
}

// top_p == 1: exactly pmhip_pipeline_generate_choice
extern "C" int pmhip_pipeline_generate_nucleus(pmhip_s2* s2, pmhip_vqgan* vq, int64_t* ids, const float* context, int L, int B,
                                               const int32_t* ctx_lens_host, int T, const float* temps_host, const int* nmask_host,
                                               const unsigned char* decode_host, int topk, uint64_t seed, uint64_t image_base,
                                               float* imgs_out, int use_graph, pmhip_stream stream, float* imgs_host, size_t host_stride,
                                               pmhip_stream copy_stream, int guided, float guidance_scale, const float* ctemps_host,
                                               float top_p) {
    GenCall c("pipeline_generate_lens", s2, vq, ids, context, L, B, T, temps_host, nmask_host, decode_host, topk, seed, image_base,
              imgs_out, use_graph, stream, imgs_host, host_stride, copy_stream);
    c.keys.lens = ctx_lens_host;
    c.guided = guided; c.guidance_scale = guidance_scale;
    c.ctemps = ctemps_host;
    c.top_p = top_p;
    return pipeline_generate(c);
}

// neg_context == NULL and gscales_host == NULL: exactly pmhip_pipeline_generate_nucleus
extern "C" int pmhip_pipeline_generate_negative(pmhip_s2* s2, pmhip_vqgan* vq, int64_t* ids, const float* context, int L, int B,
                                                const int32_t* ctx_lens_host, int T, const float* temps_host, const int* nmask_host,
                                                const unsigned char* decode_host, int topk, uint64_t seed, uint64_t image_base,
                                                float* imgs_out, int use_graph, pmhip_stream stream, float* imgs_host, size_t host_stride,
                                                pmhip_stream copy_stream, int guided, float guidance_scale, const float* ctemps_host,
                                                float top_p, const float* neg_context, int Ln, const int32_t* neg_lens_host,
                                                const float* gscales_host) {
    GenCall c("pipeline_generate_lens", s2, vq, ids, context, L, B, T, temps_host, nmask_host, decode_host, topk, seed, image_base,
              imgs_out, use_graph, stream, imgs_host, host_stride, copy_stream);
    c.keys.lens = ctx_lens_host;
    c.guided = guided; c.guidance_scale = guidance_scale;
    c.ctemps = ctemps_host;
    c.top_p = top_p;
    c.neg.context = neg_context; c.neg.Ln = Ln; c.neg.lens = neg_lens_host;
    c.gscales = gscales_host;
    return pipeline_generate(c);
}

// ctx_seg_host == NULL and tok_seg_host == NULL: exactly pmhip_pipeline_generate_negative
extern "C" int pmhip_pipeline_generate_segments(pmhip_s2* s2, pmhip_vqgan* vq, int64_t* ids, const float* context, int L, int B,
                                                const int32_t* ctx_lens_host, int T, const float* temps_host, const int* nmask_host,
                                                const unsigned char* decode_host, int topk, uint64_t seed, uint64_t image_base,
                                                float* imgs_out, int use_graph, pmhip_stream stream, float* imgs_host, size_t host_stride,
                                                pmhip_stream copy_stream, int guided, float guidance_scale, const float* ctemps_host,
                                                float top_p, const float* neg_context, int Ln, const int32_t* neg_lens_host,
                                                const float* gscales_host, const uint8_t* ctx_seg_host, const uint32_t* tok_seg_host) {
    GenCall c("pipeline_generate_lens", s2, vq, ids, context, L, B, T, temps_host, nmask_host, decode_host, topk, seed, image_base,
              imgs_out, use_graph, stream, imgs_host, host_stride, copy_stream);
    c.keys.lens = ctx_lens_host; c.keys.seg = ctx_seg_host; c.keys.tok = tok_seg_host;
    c.guided = guided; c.guidance_scale = guidance_scale;
    c.ctemps = ctemps_host;
    c.top_p = top_p;
    c.neg.context = neg_context; c.neg.Ln = Ln; c.neg.lens = neg_lens_host;
    c.gscales = gscales_host;
    return pipeline_generate(c);
}

// ctx_w_host == NULL: exactly pmhip_pipeline_generate_segments
extern "C" int pmhip_pipeline_generate_weights(pmhip_s2* s2, pmhip_vqgan* vq, int64_t* ids, const float* context, int L, int B,
                                               const int32_t* ctx_lens_host, int T, const float* temps_host, const int* nmask_host,
                                               const unsigned char* decode_host, int topk, uint64_t seed, uint64_t image_base,
                                               float* imgs_out, int use_graph, pmhip_stream stream, float* imgs_host, size_t host_stride,
                                               pmhip_stream copy_stream, int guided, float guidance_scale, const float* ctemps_host,
                                               float top_p, const float* neg_context, int Ln, const int32_t* neg_lens_host,
                                               const float* gscales_host, const uint8_t* ctx_seg_host, const uint32_t* tok_seg_host,
                                               const float* ctx_w_host) {
    GenCall c("pipeline_generate_lens", s2, vq, ids, context, L, B, T, temps_host, nmask_host, decode_host, topk, seed, image_base,
              imgs_out, use_graph, stream, imgs_host, host_stride, copy_stream);
    c.keys.lens = ctx_lens_host; c.keys.seg = ctx_seg_host; c.keys.tok = tok_seg_host; c.keys.w = ctx_w_host;
    c.guided = guided; c.guidance_scale = guidance_scale;
    c.ctemps = ctemps_host;
    c.top_p = top_p;
    c.neg.context = neg_context; c.neg.Ln = Ln; c.neg.lens = neg_lens_host;
    c.gscales = gscales_host;
    return pipeline_generate(c);
}

// One MaskGIT step in which every image carries its own decode state (include/pmhip.h).  The host records are validated, staged
// through the pinned ring into the workspace, and read from there by the sampling and re-masking kernels; with the graph flag the
// step -- tower, sampling, re-masking: one linear chain -- is captured once per (B, context length) on handle-owned ids and
// replayed, whatever the records say.
// The host decides the step's FORM from the records of the active slots (SlotsPlan below): the tower passes, the form of the
// cross-attention, of the sampling tail and of the re-masking launch.  Each form has a graph of its own, and a step in which no
// active slot uses a feature is the step of the entry without it: its launches, its graph key and its graph.
namespace {

// The slots family's call record: the common head of its nine entries by the constructor, every optional feature at its neutral
// value until an entry assigns it.  `narrow` is the name the entry's messages carry when no wider feature is present: its own, or
// the *_lens entry's for the entries above that one.
struct SlotsCall {
    const char* narrow; pmhip_s2* s2; int64_t* ids;
    // keys.lens (… _lens): staged by EVERY call -- also under PMHIP_SLOTS_KEEP_CONTEXT, where the kept cross K/V serve whatever
    // lengths this call brings.  keys.seg / keys.tok with `region` (… _regions) and keys.w (… _weights; 4x):
    // region names the kind of every slot -- 0 under its length, 1 under its key sets, 2 (with keys.w only) under its key sets and
    // its weights.  An active slot of kind 1: two picked cross-attention launches per layer; of kind 2: the weights staged too, three.
    CtxKeys keys; const uint8_t* region = nullptr;
    int B; const pmhip_slot* slots; int flags;
    int64_t* pred_out; float* score_out; pmhip_stream stream;
    // per-image guidance (… _guided): two tower passes exactly when an active slot is guided; which rows the combination touches is
    // decided on the device, from the staged records
    const pmhip_slot_guide* guides = nullptr;
    const float* choice = nullptr;                            // host [B]: choice temperatures (… _choice)
    // (… _negative) kinds: guides[b].on names what slot b is guided against -- 1 the pass without a context, 2 the negative
    // context's K/V -- and PMHIP_SLOTS_KEEP_NEGATIVE counts.  The passes per step: the conditional tower, the tower without a
    // context iff an active slot has on == 1, the tower against the negative set iff one has on == 2, each of the two followed by
    // the combine of its kind.  The negative set is prepared eagerly like the context's, or kept from the previous slots call.
    bool kinds = false; NegSet neg;
    // (… _filter) an active slot may carry top-k up to n_embed and a nucleus mass, host [B].  The sampling tail
    // is the one block-statistics launch unless an active slot is of another class (common.h pm_sample_class): then the launch per class
    bool filters = false; const float* top_p = nullptr;
    // (… _edit) a re-masking count per slot, host [B], -1 = the record's num_mask; with an active slot at >= 0
    // the re-masking launch is the form with a count per slot
    const int32_t* counts = nullptr;
    SlotsCall(const char* narrow_, pmhip_s2* s2_, int64_t* ids_, const float* context, int L, int B_, const pmhip_slot* slots_, int flags_,
              int64_t* pred_out_, float* score_out_, pmhip_stream stream_)
        : narrow(narrow_), s2(s2_), ids(ids_), keys(context, L), B(B_), slots(slots_), flags(flags_), pred_out(pred_out_), score_out(score_out_),
          stream(stream_) {}
    bool idle(int b) const { return (slots[b].step & PM_SLOT_IDLE) != 0; }
};

// What the host decides about a step from its records: the name its messages carry, which sets it has, and the step's form.
struct SlotsPlan {
    const char* who = nullptr;
    bool keep_neg = false, neg_set = false;                   // the negative set is kept / this call has one, given or kept
    bool regions = false;                                     // an active slot is of kind 1 or 2: the picked cross-attention
    bool weighted = false;                                    // an active slot is of kind 2: its third launch
    bool two_pass = false;                                    // an active slot is guided
    bool pass_neg = false, pass_uncond = false;               // ... against the negative set / against no context
    bool choice = false;                                      // an active slot has a choice temperature other than 0 (else: the step without)
    bool chain = false;                                       // filters: an active slot is of another class than the block-statistics kernel's
    bool edit = false;                                        // counts: an active slot brings a count of its own (>= 0)
};

bool slot_regional(const SlotsCall& c, const SlotsPlan& p, int b) { return p.regions && !c.idle(b) && c.region[b] >= 1; }
bool slot_weighted(const SlotsCall& c, const SlotsPlan& p, int b) { return slot_regional(c, p, b) && c.region[b] == 2; }

// plan: every check of the host records and the step's form, pure host code
int slots_plan(const SlotsCall& c, SlotsPlan& p) {
    pmhip_s2* s2 = c.s2;
    const CtxKeys& k = c.keys;
    const int B = c.B, L = k.L, Ln = c.neg.Ln;
    p.keep_neg = c.kinds && (c.flags & PMHIP_SLOTS_KEEP_NEGATIVE) != 0;
    p.neg_set = c.neg.context || p.keep_neg;
    // (the entries above *_lens pass that entry's name as `narrow`: they report as *_lens when no wider feature is present)
    const char* who = p.who = call_name({{k.w != nullptr, "pipeline_step_slots_weights"},
                                         {k.seg || k.tok || c.region, "pipeline_step_slots_regions"},
                                         {c.counts != nullptr, "pipeline_step_slots_edit"},
                                         {c.filters, "pipeline_step_slots_filter"},
                                         {p.neg_set || c.neg.lens, "pipeline_step_slots_negative"},
                                         {c.choice != nullptr, "pipeline_step_slots_choice"}}, c.narrow);
    PM_REQUIRE(s2 && c.ids && c.slots && B > 0, "%s: bad arguments (null handle, ids or slots, or B <= 0)", who);
    const bool have_context = k.context || ((c.flags & PMHIP_SLOTS_KEEP_CONTEXT) && L > 0);
    // regional slots (pmhip_pipeline_step_slots_regions): the three arrays together or none, the rules of
    // check_segments for the ACTIVE slots that are flagged, the length check for every other slot
    // weighted slots (pmhip_pipeline_step_slots_weights): region is a KIND per slot -- 0 under its length,
    // 1 under its key sets, 2 under its key sets and its weights --, kind 2 only where the weights came; a kind-2 slot follows the
    // rules of a regional one and the weight rules of check_weights
    PM_REQUIRE((!k.seg == !k.tok) && (!k.seg == !c.region), "%s: ctx_seg_host, tok_seg_host and region_host come together (one of them is NULL)",
               who);
    if (c.region) {
        for (int b = 0; b < B; ++b) {
            if (c.idle(b)) continue;
            if (k.w) PM_REQUIRE(c.region[b] <= 2, "%s: slot %d: region_host=%d must be 0, 1 or 2", who, b, (int)c.region[b]);
            else PM_REQUIRE(c.region[b] <= 1, "%s: slot %d: region_host=%d must be 0 or 1 (2 needs ctx_w_host)", who, b, (int)c.region[b]);
            p.regions = p.regions || c.region[b] >= 1;
            p.weighted = p.weighted || c.region[b] == 2;
        }
    } else {
        PM_REQUIRE(!k.w, "%s: ctx_w_host given without ctx_seg_host, tok_seg_host and region_host", who);
    }
    if (!p.regions) {
        PM_TRY(check_ctx_lens(who, k.lens, have_context, L, B));
    } else {
        PM_REQUIRE(have_context && L > 0, "%s: regional slots given without a context", who);
        for (int b = 0; b < B; ++b) {
            if (slot_regional(c, p, b)) {
                PM_TRY(check_segments_of(who, "slot", b, k.seg, k.tok, L, s2->cfg.tokens));
                if (slot_weighted(c, p, b)) PM_TRY(check_slot_weights(who, b, k.w, k.seg, k.tok, L, s2->cfg.tokens));
            } else
                PM_REQUIRE(!k.lens || (k.lens[b] >= 1 && k.lens[b] <= L), "%s: image %d: context length %d must be in [1, L=%d]", who, b,
                           (int)k.lens[b], L);
        }
    }
    const auto& cfg = s2->cfg;
    PM_REQUIRE(cfg.n_embed % 64 == 0, "%s: n_embed=%d must be a multiple of 64", who, cfg.n_embed);
    PM_REQUIRE(p.neg_set || !c.neg.lens, "%s: neg_lens_host given without a negative context", who);
    PM_REQUIRE(!p.neg_set || Ln >= 1, "%s: negative context given with Ln=%d", who, Ln);
    for (int b = 0; c.neg.lens && b < B; ++b)
        PM_REQUIRE(c.neg.lens[b] >= 1 && c.neg.lens[b] <= Ln, "%s: slot %d: negative context length %d must be in [1, Ln=%d]", who, b,
                   (int)c.neg.lens[b], Ln);
    for (int b = 0; b < B; ++b) {
        const pmhip_slot& sl = c.slots[b];
        if (c.idle(b)) continue;
        if (c.choice) {
            PM_TRY(pm_check_choice_t(who, c.choice[b]));
            p.choice = p.choice || c.choice[b] != 0.f;
        }
        if (c.filters) {
            PM_REQUIRE(sl.topk >= 1 && sl.topk <= cfg.n_embed, "%s: slot %d: topk=%d must be in [1, n_embed=%d]", who, b, sl.topk, cfg.n_embed);
            const float mass = c.top_p ? c.top_p[b] : 1.f;
            PM_TRY(pm_check_top_p((std::string(who) + ": slot " + std::to_string(b)).c_str(), mass));
            p.chain = p.chain || pm_sample_class(sl.topk, mass < 1.f) != PM_CLASS_TILES;
        } else {
            PM_REQUIRE(sl.topk >= 1 && sl.topk <= 8, "%s: slot %d: topk=%d must be in [1, 8]", who, b, sl.topk);
        }
        if (c.counts) {
            PM_REQUIRE(c.counts[b] >= -1 && c.counts[b] <= cfg.tokens, "%s: slot %d: count %d must be in [-1, tokens=%d]", who, b,
                       (int)c.counts[b], cfg.tokens);
            p.edit = p.edit || c.counts[b] >= 0;
        }
        // (a slot with a count of its own never reads the record's)
        PM_REQUIRE(sl.num_mask >= 1 || (c.counts && c.counts[b] >= 0), "%s: slot %d: num_mask=%d must be >= 1", who, b, sl.num_mask);
        if (c.guides && c.guides[b].on) {
            PM_REQUIRE(!c.kinds || c.guides[b].on <= 2, "%s: slot %d: on=%u must be 0, 1 or 2", who, b, c.guides[b].on);
            PM_REQUIRE(std::isfinite(c.guides[b].scale), "%s: slot %d: the guidance scale must be finite", who, b);
            PM_REQUIRE(L > 0 && (k.context || (c.flags & PMHIP_SLOTS_KEEP_CONTEXT)),
                       "%s: slot %d: guidance needs a context (context NULL IS the unconditional branch)", who, b);
            const bool against_neg = c.kinds && c.guides[b].on == 2;
            PM_REQUIRE(!against_neg || p.neg_set, "%s: slot %d: on=2 needs a negative context, given or kept", who, b);
            (against_neg ? p.pass_neg : p.pass_uncond) = true;
            p.two_pass = true;
        }
    }
    return PMHIP_OK;
}

// context: both sets prepared (eager, outside any graph) or kept, the key arrays staged -- the slots step's own variant of
// stage_context: a kept set is refused unless a slots call prepared it at this shape, and under regional slots the rows of the other
// slots are staged neutral.  Lc: the length the context's set was prepared at (0: without a context).
int slots_context(const SlotsCall& c, const SlotsPlan& p, hipStream_t s, int& Lc) {
    pmhip_s2* s2 = c.s2;
    const CtxKeys& k = c.keys;
    const int B = c.B, L = k.L, Ln = c.neg.Ln, tokens = s2->cfg.tokens;
    const char* who = p.who;
    if (p.keep_neg && (s2->slots_neg_Ln < 0 || s2->slots_neg_B != B || s2->slots_neg_Ln != Ln)) {
        pm_set_error("%s: keep-negative asked for B=%d Ln=%d, but %s", who, B, Ln,
                     s2->slots_neg_Ln < 0 ? "no slots call has prepared a negative context on this handle (or another entry point replaced it)"
                                          : "the prepared negative context has another B or Ln");
        return PMHIP_ESTATE;
    }
    // a kept negative set outlives the preparation of a new context (which drops the handle's negative set: s2_prepare_context);
    // its K/V live in workspace buffers of their own, which only a negative preparation touches
    std::vector<CrossKV> kept_neg;
    if (p.keep_neg) kept_neg = s2->cross_neg;
    if (c.flags & PMHIP_SLOTS_KEEP_CONTEXT) {
        if (s2->slots_ctx_L < 0 || s2->slots_ctx_B != B || s2->slots_ctx_L != L) {
            pm_set_error("%s: keep-context asked for B=%d L=%d, but %s", who, B, L,
                         s2->slots_ctx_L < 0 ? "no slots call has prepared a context on this handle (or another entry point replaced it)"
                                             : "the prepared context has another B or L");
            return PMHIP_ESTATE;
        }
    } else {
        PM_TRY(s2_prepare_context(s2, k.context, L, B, s));
        s2->slots_ctx_B = B;
        s2->slots_ctx_L = k.context ? L : 0;
    }
    Lc = s2->slots_ctx_L;
    PM_REQUIRE(!k.lens || Lc > 0, "%s: ctx_lens_host given, but the kept context was prepared without one", who);
    PM_REQUIRE(!p.regions || Lc > 0, "%s: regional slots given, but the kept context was prepared without one", who);
    if (!p.regions) {
        PM_TRY(s2_set_ctx_lens(s2, k.lens, L, B, s));
    } else {
        // The lengths the want = 0 launch reads (L where none came; a regional or idle slot's is never read by a workgroup that
        // goes on), then the arrays with the rows of the slots that are not regional made neutral: they are not looked at here
        // and by no kernel -- one segment, every token attending to it.
        std::vector<int32_t> lens((size_t)B, L);
        std::vector<uint8_t> kseg((size_t)B * L, 0), flag((size_t)B, 0);
        std::vector<float> wts(p.weighted ? (size_t)B * L : 0, 1.f);   // a slot of kind 0 or 1 is staged as 1; no kernel reads its rows
        std::vector<uint32_t> tseg((size_t)B * tokens, 1u);
        for (int b = 0; b < B; ++b) {
            if (!slot_regional(c, p, b)) {
                if (k.lens) lens[b] = k.lens[b];
                continue;
            }
            flag[b] = c.region[b];
            if (slot_weighted(c, p, b)) std::copy(k.w + (size_t)b * L, k.w + (size_t)(b + 1) * L, wts.begin() + (size_t)b * L);
            memcpy(kseg.data() + (size_t)b * L, k.seg + (size_t)b * L, (size_t)L);
            memcpy(tseg.data() + (size_t)b * tokens, k.tok + (size_t)b * tokens, (size_t)tokens * 4);
        }
        PM_TRY(s2_set_ctx_lens(s2, lens.data(), L, B, s));
        PM_TRY(s2_set_segments(s2, kseg.data(), tseg.data(), L, B, s, flag.data()));
        if (p.weighted) PM_TRY(s2_set_weights(s2, wts.data(), L, B, s));
    }
    // the negative set: prepared, kept, or -- a call that neither brings nor keeps one -- dropped
    if (p.keep_neg) {
        s2->cross_neg = kept_neg;                             // (neg.context is ignored, like the context under PMHIP_SLOTS_KEEP_CONTEXT)
    } else if (c.neg.context) {
        const int ctx_B = s2->slots_ctx_B, ctx_L = s2->slots_ctx_L;
        PM_TRY(s2_prepare_context(s2, c.neg.context, Ln, B, s, kCrossNegative));
        s2->slots_ctx_B = ctx_B; s2->slots_ctx_L = ctx_L;     // (the preparation of either set forgets what slots calls prepared)
    } else {
        for (auto& ck : s2->cross_neg) ck = CrossKV{};
    }
    s2->slots_neg_B = B;
    s2->slots_neg_Ln = p.neg_set ? Ln : -1;
    if (p.neg_set) PM_TRY(s2_set_ctx_lens(s2, c.neg.lens, Ln, B, s, kCrossNegative));   // every call brings its own lengths (or NULL)
    return PMHIP_OK;
}

uint32_t word_of(float v) { uint32_t w; memcpy(&w, &v, 4); return w; }

// records: one pinned ring entry -> the workspace, in five sections, each on a 16-byte boundary behind the one before it.  A section
// has its place in the entry whether or not this step stages it (the layout is a contract with captured graphs).  The first two are
// the caller's records as they came; the other three are 4-byte values per slot, padded to whole 16-byte words, an idle slot's (and
// the padding) at the section's idle value.  The Step takes the device pointers; an unstaged section's is NULL.
int slots_records(const SlotsCall& c, const SlotsPlan& p, hipStream_t s, Step& st) {
    pmhip_s2* s2 = c.s2;
    const size_t B = (size_t)c.B, words = (size_t)round_up(c.B, 4) * 4;
    static_assert(sizeof(pmhip_slot) % 16 == 0, "the guide records sit right behind the slot records");
    pmhip_slot* dslots = nullptr;
    pmhip_slot_guide* dguides = nullptr;
    float *dchoice = nullptr, *dtop_p = nullptr;
    int32_t* dcounts = nullptr;
    struct Section { const char* ws; size_t bytes; bool staged; const void* host; bool padded; uint32_t idle; void** dev; size_t at; };
    Section sections[5] = {
        {"slots.dev", sizeof(pmhip_slot) * B, true, c.slots, false, 0, (void**)&dslots, 0},                  // the slot records
        {"slots.guides", sizeof(pmhip_slot_guide) * B, p.two_pass, c.guides, false, 0, (void**)&dguides, 0},  // the guide records
        {"slots.choice", words, p.choice, c.choice, true, word_of(0.f), (void**)&dchoice, 0},                 // choice temperatures; idle: 0
        // the nucleus masses of a step whose tail is the launch per class; idle, or no masses given: 1
        {"slots.top_p", words, p.chain, c.top_p, true, word_of(1.f), (void**)&dtop_p, 0},
        // the re-masking counts of a step in which an active slot brings its own; idle: 0
        {"slots.counts", words, p.edit, c.counts, true, 0, (void**)&dcounts, 0},
    };
    size_t end = 0;
    for (Section& x : sections) {
        x.at = (end + 15) & ~(size_t)15;
        end = x.at + x.bytes;
        if (x.staged) PM_TRY(s2->ws.get(x.ws, x.bytes, x.dev, s));
    }
    PM_TRY(s2->slots_ring.reserve(end));                      // the whole layout, whatever this step stages
    PM_TRY(s2->slots_ring.acquire());
    std::vector<uint32_t> padded;
    for (const Section& x : sections) {
        if (!x.staged) continue;
        const void* src = x.host;
        if (x.padded) {
            padded.assign(x.bytes / 4, x.idle);
            for (size_t b = 0; x.host && b < B; ++b)
                if (!c.idle((int)b)) memcpy(&padded[b], static_cast<const unsigned char*>(x.host) + 4 * b, 4);
            src = padded.data();
        }
        PM_TRY(s2->slots_ring.stage(*x.dev, x.at, src, x.bytes, s));
    }
    PM_TRY(s2->slots_ring.commit(s));
    st.slots = dslots;
    st.guides = dguides;
    st.slots_neg = p.pass_neg;
    st.slots_uncond = p.pass_uncond;
    st.choice_dev = dchoice;
    st.filters = p.chain;                                     // every active slot of class T: the step of the entries without filters
    st.top_p_dev = dtop_p;
    st.counts = dcounts;                                      // NULL: the re-masking launch of the entries without counts
    return PMHIP_OK;
}

// counters: a step is counted once it is staged, by each of its forms; a refused call counts nothing
void slots_count(const SlotsCall& c, const SlotsPlan& p) {
    pmhip_s2* s2 = c.s2;
    if (p.regions) ++(p.weighted ? s2->slots_weight_steps : s2->slots_region_steps);
    if (p.edit) ++s2->slots_edit_steps;
    if (c.filters) ++(p.chain ? s2->slots_filter_chain : s2->slots_filter_tiles);
    ++(p.pass_neg && p.pass_uncond ? s2->slots_three_pass : p.two_pass ? s2->slots_two_pass : s2->slots_one_pass);
}

// key: the graph cache key of a step.  It names the pass set; a step without a pass against the negative set keeps the key it had
// before there was one, and one with it adds Ln and whether negative lengths came (the kernel form of that tower's cross-attention).
// Behind it the form of the cross-attention (W three picked launches, R two, n per-image lengths), c the choice form of the
// re-masking launch, F the sampling launch per class, E the re-masking launch with a count per slot.
std::string slots_key(const SlotsCall& c, const SlotsPlan& p, int Lc) {
    const char* passes = p.pass_neg ? (p.pass_uncond ? "slotsthreeB" : "slotsnegB") : p.two_pass ? "slotsguidedB" : "slotsB";
    const std::string neg_key = p.pass_neg ? "N" + std::to_string(c.neg.Ln) + (c.neg.lens ? "n" : "") : "";
    return passes + std::to_string(c.B) + "L" + std::to_string(Lc) + "f" + std::to_string(c.s2->sw.key()) +
           (p.weighted ? "W" : p.regions ? "R" : c.keys.lens ? "n" : "") + (p.choice ? "c" : "") + neg_key + (p.chain ? "F" : "") +
           (p.edit ? "E" : "");
}

// run: the step on the caller's ids, or -- with the graph flag -- captured once per key on handle-owned ids and replayed
int slots_run(const SlotsCall& c, const SlotsPlan& p, const Step& st, int Lc, hipStream_t s) {
    pmhip_s2* s2 = c.s2;
    const int B = c.B;
    // ignored exactly when pipeline_generate ignores its graph request (same bits either way)
    const bool graph = (c.flags & PMHIP_SLOTS_GRAPH) && !g_pm_timing_on.load() && !direct_dispatch_off();
    if (!graph) return sample_step(s2, nullptr, c.ids, B, st, nullptr, c.pred_out, c.score_out, s);

    const size_t rows = (size_t)B * s2->cfg.tokens, ids_bytes = rows * 8;
    int64_t* gids;
    WS(s2->ws, "slots.ids", ids_bytes, gids);
    PM_TRY(copy16_async(gids, c.ids, ids_bytes, s));
    PM_TRY(run_graphs(s2, nullptr, s2->graphs[slots_key(c, p, Lc)], 1, s,
                      [&](hipStream_t on, size_t) { return sample_step(s2, nullptr, gids, B, st, nullptr, nullptr, nullptr, on); },
                      [](size_t) { return PMHIP_OK; }));
    PM_TRY(copy16_async(c.ids, gids, ids_bytes, s));
    StepBufs b;
    PM_TRY(pred_bufs(s2, rows, b, s));
    return copy_aux(b, rows, c.pred_out, c.score_out, s);
}

}  // namespace

// The slots family's one builder: the record -> the step, phase by phase.
static int step_slots_call(const SlotsCall& c) {
    SlotsPlan p;
    PM_TRY(slots_plan(c, p));
    hipStream_t s = (hipStream_t)c.stream;
    int Lc = 0;
    PM_TRY(slots_context(c, p, s, Lc));
    Step st;
    PM_TRY(slots_records(c, p, s, st));
    slots_count(c, p);
    return slots_run(c, p, st, Lc, s);
}

extern "C" int pmhip_pipeline_step_slots(pmhip_s2* s2, int64_t* ids, const float* context, int L, int B, const pmhip_slot* slots_host,
                                         int flags, int64_t* pred_out, float* score_out, pmhip_stream stream) {
    SlotsCall c("pipeline_step_slots", s2, ids, context, L, B, slots_host, flags, pred_out, score_out, stream);
    return step_slots_call(c);
}

extern "C" int pmhip_pipeline_step_slots_guided(pmhip_s2* s2, int64_t* ids, const float* context, int L, int B, const pmhip_slot* slots_host,
                                                const pmhip_slot_guide* guides_host, int flags, int64_t* pred_out, float* score_out,
                                                pmhip_stream stream) {
    SlotsCall c("pipeline_step_slots_guided", s2, ids, context, L, B, slots_host, flags, pred_out, score_out, stream);
    c.guides = guides_host;
    return step_slots_call(c);
}

extern "C" int pmhip_pipeline_step_slots_lens(pmhip_s2* s2, int64_t* ids, const float* context, int L, int B, const int32_t* ctx_lens_host,
                                              const pmhip_slot* slots_host, const pmhip_slot_guide* guides_host, int flags,
                                              int64_t* pred_out, float* score_out, pmhip_stream stream) {
    SlotsCall c("pipeline_step_slots_lens", s2, ids, context, L, B, slots_host, flags, pred_out, score_out, stream);
    c.keys.lens = ctx_lens_host;
    c.guides = guides_host;
    return step_slots_call(c);
}

// choice_host NULL, or 0 for every active slot: exactly pmhip_pipeline_step_slots_lens
extern "C" int pmhip_pipeline_step_slots_choice(pmhip_s2* s2, int64_t* ids, const float* context, int L, int B, const int32_t* ctx_lens_host,
                                                const pmhip_slot* slots_host, const pmhip_slot_guide* guides_host, const float* choice_host,
                                                int flags, int64_t* pred_out, float* score_out, pmhip_stream stream) {
    SlotsCall c("pipeline_step_slots_lens", s2, ids, context, L, B, slots_host, flags, pred_out, score_out, stream);
    c.keys.lens = ctx_lens_host;
    c.guides = guides_host;
    c.choice = choice_host;
    return step_slots_call(c);
}

// neg_context NULL, PMHIP_SLOTS_KEEP_NEGATIVE clear and no active slot with on == 2: exactly pmhip_pipeline_step_slots_choice
extern "C" int pmhip_pipeline_step_slots_negative(pmhip_s2* s2, int64_t* ids, const float* context, int L, int B, const int32_t* ctx_lens_host,
                                                  const pmhip_slot* slots_host, const pmhip_slot_guide* guides_host, const float* choice_host,
                                                  const float* neg_context, int Ln, const int32_t* neg_lens_host, int flags,
                                                  int64_t* pred_out, float* score_out, pmhip_stream stream) {
    SlotsCall c("pipeline_step_slots_lens", s2, ids, context, L, B, slots_host, flags, pred_out, score_out, stream);
    c.keys.lens = ctx_lens_host;
    c.guides = guides_host;
    c.choice = choice_host;
    c.kinds = true; c.neg.context = neg_context; c.neg.Ln = Ln; c.neg.lens = neg_lens_host;
    return step_slots_call(c);
}

// top_p_host NULL and every active slot at topk <= 8: exactly pmhip_pipeline_step_slots_negative
extern "C" int pmhip_pipeline_step_slots_filter(pmhip_s2* s2, int64_t* ids, const float* context, int L, int B, const int32_t* ctx_lens_host,
                                                const pmhip_slot* slots_host, const pmhip_slot_guide* guides_host, const float* choice_host,
                                                const float* neg_context, int Ln, const int32_t* neg_lens_host, const float* top_p_host,
                                                int flags, int64_t* pred_out, float* score_out, pmhip_stream stream) {
    SlotsCall c("pipeline_step_slots_lens", s2, ids, context, L, B, slots_host, flags, pred_out, score_out, stream);
    c.keys.lens = ctx_lens_host;
    c.guides = guides_host;
    c.choice = choice_host;
    c.kinds = true; c.neg.context = neg_context; c.neg.Ln = Ln; c.neg.lens = neg_lens_host;
    c.filters = true; c.top_p = top_p_host;
    return step_slots_call(c);
}

// every active slot at -1 (or counts_host NULL): exactly pmhip_pipeline_step_slots_filter
extern "C" int pmhip_pipeline_step_slots_edit(pmhip_s2* s2, int64_t* ids, const float* context, int L, int B, const int32_t* ctx_lens_host,
                                              const pmhip_slot* slots_host, const pmhip_slot_guide* guides_host, const float* choice_host,
                                              const float* neg_context, int Ln, const int32_t* neg_lens_host, const float* top_p_host,
                                              const int32_t* counts_host, int flags, int64_t* pred_out, float* score_out, pmhip_stream stream) {
    SlotsCall c("pipeline_step_slots_lens", s2, ids, context, L, B, slots_host, flags, pred_out, score_out, stream);
    c.keys.lens = ctx_lens_host;
    c.guides = guides_host;
    c.choice = choice_host;
    c.kinds = true; c.neg.context = neg_context; c.neg.Ln = Ln; c.neg.lens = neg_lens_host;
    c.filters = true; c.top_p = top_p_host;
    c.counts = counts_host;
    return step_slots_call(c);
}

// no active slot with region_host == 1 (or the three arrays NULL): exactly pmhip_pipeline_step_slots_edit
extern "C" int pmhip_pipeline_step_slots_regions(pmhip_s2* s2, int64_t* ids, const float* context, int L, int B, const int32_t* ctx_lens_host,
                                                 const pmhip_slot* slots_host, const pmhip_slot_guide* guides_host, const float* choice_host,
                                                 const float* neg_context, int Ln, const int32_t* neg_lens_host, const float* top_p_host,
                                                 const int32_t* counts_host, const uint8_t* ctx_seg_host, const uint32_t* tok_seg_host,
                                                 const uint8_t* region_host, int flags, int64_t* pred_out, float* score_out,
                                                 pmhip_stream stream) {
    SlotsCall c("pipeline_step_slots_lens", s2, ids, context, L, B, slots_host, flags, pred_out, score_out, stream);
    c.keys.lens = ctx_lens_host;
    c.guides = guides_host;
    c.choice = choice_host;
    c.kinds = true; c.neg.context = neg_context; c.neg.Ln = Ln; c.neg.lens = neg_lens_host;
    c.filters = true; c.top_p = top_p_host;
    c.counts = counts_host;
    c.keys.seg = ctx_seg_host; c.keys.tok = tok_seg_host; c.region = region_host;
    return step_slots_call(c);
}

// steps of that entry that ran the two-launch cross-attention (an active slot was regional)
extern "C" int pmhip_s2_slots_region_steps(const pmhip_s2* h, int* steps) {
    PM_REQUIRE(h, "s2_slots_region_steps: null handle");
    if (steps) *steps = h->slots_region_steps;
    return PMHIP_OK;
}

// ctx_w_host NULL, or no active slot of kind 2: exactly pmhip_pipeline_step_slots_regions
extern "C" int pmhip_pipeline_step_slots_weights(pmhip_s2* s2, int64_t* ids, const float* context, int L, int B, const int32_t* ctx_lens_host,
                                                 const pmhip_slot* slots_host, const pmhip_slot_guide* guides_host, const float* choice_host,
                                                 const float* neg_context, int Ln, const int32_t* neg_lens_host, const float* top_p_host,
                                                 const int32_t* counts_host, const uint8_t* ctx_seg_host, const uint32_t* tok_seg_host,
                                                 const uint8_t* region_host, const float* ctx_w_host, int flags, int64_t* pred_out,
                                                 float* score_out, pmhip_stream stream) {
    SlotsCall c("pipeline_step_slots_lens", s2, ids, context, L, B, slots_host, flags, pred_out, score_out, stream);
    c.keys.lens = ctx_lens_host;
    c.guides = guides_host;
    c.choice = choice_host;
    c.kinds = true; c.neg.context = neg_context; c.neg.Ln = Ln; c.neg.lens = neg_lens_host;
    c.filters = true; c.top_p = top_p_host;
    c.counts = counts_host;
    c.keys.seg = ctx_seg_host; c.keys.tok = tok_seg_host; c.region = region_host;
    c.keys.w = ctx_w_host;
    return step_slots_call(c);
}

// steps of that entry that ran the three-launch cross-attention (an active slot was weighted)
extern "C" int pmhip_s2_slots_weight_steps(const pmhip_s2* h, int* steps) {
    PM_REQUIRE(h, "s2_slots_weight_steps: null handle");
    if (steps) *steps = h->slots_weight_steps;
    return PMHIP_OK;
}

// steps of that entry whose re-masking launch was the form with a count per slot
extern "C" int pmhip_s2_slots_edit_steps(const pmhip_s2* h, int* steps) {
    PM_REQUIRE(h, "s2_slots_edit_steps: null handle");
    if (steps) *steps = h->slots_edit_steps;
    return PMHIP_OK;
}

// steps of pmhip_pipeline_step_slots_filter (and of the edit entry, which is that entry with counts) by the form of their sampling tail
extern "C" int pmhip_s2_slots_filter_steps(const pmhip_s2* h, int* tiles_only, int* chain) {
    PM_REQUIRE(h, "s2_slots_filter_steps: null handle");
    if (tiles_only) *tiles_only = h->slots_filter_tiles;
    if (chain) *chain = h->slots_filter_chain;
    return PMHIP_OK;
}

// slots steps by tower passes: one (no active slot guided) / exactly two
extern "C" int pmhip_s2_slots_steps(const pmhip_s2* h, int* one_pass, int* two_pass) {
    PM_REQUIRE(h, "s2_slots_steps: null handle");
    if (one_pass) *one_pass = h->slots_one_pass;
    if (two_pass) *two_pass = h->slots_two_pass;
    return PMHIP_OK;
}

// ... and three: active slots guided against no context and against the negative set in one step
extern "C" int pmhip_s2_slots_passes(const pmhip_s2* h, int* one_pass, int* two_pass, int* three_pass) {
    PM_REQUIRE(h, "s2_slots_passes: null handle");
    if (one_pass) *one_pass = h->slots_one_pass;
    if (two_pass) *two_pass = h->slots_two_pass;
    if (three_pass) *three_pass = h->slots_three_pass;
    return PMHIP_OK;
}

// how often the shared step 0 was computed (0 or 1 per handle) and how many loops sampled from it without running a tower
extern "C" int pmhip_s2_step0_shared(const pmhip_s2* h, int* fills, int* hits) {
    PM_REQUIRE(h, "s2_step0_shared: null handle");
    if (fills) *fills = h->s0_fills;
    if (hits) *hits = h->s0_hits;
    return PMHIP_OK;
}

// the PMHIP_* switches a handle latched when it was created (bit 0 fold, 1 hilo, 2 stats, 3 center, 4 blocking_wait)
extern "C" int pmhip_s2_switches(const pmhip_s2* h) {
    return h ? h->sw.key() + (h->sw.blocking_wait ? 16 : 0) + (direct_dispatch_off() ? 32 : 0) : -1;
}
extern "C" int pmhip_vqgan_switches(const pmhip_vqgan* h) { return h ? h->sw.key() + (h->sw.blocking_wait ? 16 : 0) : -1; }

// the edit loop (include/pmhip.h): pmhip_pipeline_generate_negative with a re-masking count per step and image, a decode of the
// merged ids, and the caller's ids as the start
extern "C" int pmhip_pipeline_generate_edit(pmhip_s2* s2, pmhip_vqgan* vq, int64_t* ids, const float* context, int L, int B,
                                            const int32_t* ctx_lens_host, int T, const float* temps_host, const int32_t* nmask_img_host,
                                            const unsigned char* decode_host, int topk, uint64_t seed, uint64_t image_base,
                                            float* imgs_out, int use_graph, pmhip_stream stream, float* imgs_host, size_t host_stride,
                                            pmhip_stream copy_stream, int guided, float guidance_scale, const float* ctemps_host,
                                            float top_p, const float* neg_context, int Ln, const int32_t* neg_lens_host,
                                            const float* gscales_host) {
    PM_REQUIRE(nmask_img_host, "pipeline_generate_edit: null count table");
    GenCall c("pipeline_generate_edit", s2, vq, ids, context, L, B, T, temps_host, nullptr, decode_host, topk, seed, image_base,
              imgs_out, use_graph, stream, imgs_host, host_stride, copy_stream);
    c.keys.lens = ctx_lens_host;
    c.guided = guided; c.guidance_scale = guidance_scale;
    c.ctemps = ctemps_host;
    c.top_p = top_p;
    c.neg.context = neg_context; c.neg.Ln = Ln; c.neg.lens = neg_lens_host;
    c.gscales = gscales_host;
    c.nmask_img = nmask_img_host;
    return pipeline_generate(c);
}
