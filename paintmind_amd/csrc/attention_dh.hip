// Attention for dim_head != 64 (reference modules/attention.py:27-33 takes any dim_head; every shipped config uses 64,
// which the tuned kernels in attention.hip / the head-split GEMM epilogue are built for).  This file is the plain path
// behind pmhip_gemm_heads_dh / pmhip_attention_dh: correct for dim_head = 16, 32, ..., 128, not tuned.
//
//   head split : the projection is an ordinary GEMM into an f32 scratch [M, nparts*heads*dh]; one thread per element
//                moves it into Q [B,H,t,dh] (scaled), K [B,H,tp,dh] or V^T [B,H,dh,tp] and rounds to the compute type once.
//   attention  : flash-style online softmax on the vector ALU.  4 lanes share one query row, each owning dh/4 contiguous
//                dims of q and of the output; the score is a quad reduction (two DPP steps).  All lanes of a workgroup
//                walk the keys in the same order, so K / V^T addresses are wave-uniform per quad position and come out of
//                L1/L2 as broadcasts.  The score matrix is never materialised.
//
// The attention entry points of the C ABI (pmhip_attention, pmhip_attention_dh, pmhip_attention_lens, pmhip_attention_segments, pmhip_attention_weighted, pmhip_attention_pick, pmhip_attention_pick_weighted) are at the end of this file:
// one argument check for the family, then the launcher of attention.hip, attention_bf16.hip or this file.
#include "common.h"

namespace {

struct SplitParams {
    const float* src;
    void* outs[3];
    int kinds[3];
    int M, nparts, heads, dh, tokens, tokens_pad;
    float q_scale;
};

template <typename T>
__global__ __launch_bounds__(256) void head_split_kernel(SplitParams p) {
    const int inner = p.heads * p.dh, N = p.nparts * inner;
    const long long total = (long long)p.M * N;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int m = (int)(idx / N), col = (int)(idx % N);
        const int part = col / inner, hc = col % inner, h = hc / p.dh, d = hc % p.dh;
        const int b = m / p.tokens, t = m % p.tokens;
        const float v = p.src[idx];
        T* o = reinterpret_cast<T*>(p.outs[part]);
        const size_t bh = (size_t)b * p.heads + h;
        if (p.kinds[part] == PMHIP_PART_Q)
            o[(bh * p.tokens + t) * p.dh + d] = from_f32<T>(v * p.q_scale);
        else if (p.kinds[part] == PMHIP_PART_K)
            o[(bh * p.tokens_pad + t) * p.dh + d] = from_f32<T>(v);
        else
            o[(bh * p.dh + d) * p.tokens_pad + t] = from_f32<T>(v);
    }
}

// DPL = dims per lane = dh / 4
#define PM_ATTN_BODY "attention_dh_body.h"
#define PM_ATTN_NAME(sfx) attention_dh##sfx##kernel
#define PM_ATTN_INSTANTIATE
#include "attention_forms.h"

// weights -> key_bias: 0 -> -inf (excluded), 1 -> exactly 0, otherwise log2(w), times ln 2 when the scores are nats
__global__ __launch_bounds__(256) void key_bias_kernel(const float* __restrict__ w, float* __restrict__ bias, int n, int use_exp2) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float x = w[i];
    float r;
    if (x == 0.f) r = -INFINITY;
    else if (x == 1.f) r = 0.f;
    else r = use_exp2 ? log2f(x) : log2f(x) * 0.693147180559945309f;
    bias[i] = r;
}

template <typename T, int DPL>
void launch_dh(const PmAttnArgs& a) {
    const dim3 grid((a.Nq + 63) / 64, a.B * a.heads), block(256);
#define PM_ATTN_LAUNCH(form, sfx, ...)                                                                                                    \
    case PM_FORM_##form: {                                                                                                                \
        auto k = a.use_exp2 ? PM_ATTN_NAME(sfx)<T, DPL, true> : PM_ATTN_NAME(sfx)<T, DPL, false>;                                          \
        hipLaunchKernelGGL(k, grid, block, 0, a.stream, (const T*)a.Q, (const T*)a.K, (const T*)a.Vt, (T*)a.out, a.ldo, a.heads, a.Nq, a.Nkv, \
                           a.Nkv_pad, ##__VA_ARGS__);                                                                                     \
    } break;
    switch (pm_attn_form(a)) { PM_ATTN_FORMS(PM_ATTN_LAUNCH) }
#undef PM_ATTN_LAUNCH
}
#undef PM_ATTN_BODY
#undef PM_ATTN_NAME

// the launcher of this file's kernels: dim_head != 64, already passed through check_dh
template <typename T>
int pm_attention_dh(int dh, const PmAttnArgs& a) {
    return pm_dh_dispatch("attention_dh", dh, [&](auto dpl) { launch_dh<T, decltype(dpl)::value>(a); });
}

int check_dh(const char* who, int heads, int dim_head) {
    PM_REQUIRE(dim_head >= 16 && dim_head <= 128 && dim_head % 16 == 0, "%s: dim_head=%d must be a multiple of 16 in [16,128]", who, dim_head);
    PM_REQUIRE(heads > 0 && (heads * dim_head) % 64 == 0, "%s: heads*dim_head=%d must be a multiple of 64", who, heads * dim_head);
    return PMHIP_OK;
}

}  // namespace

extern "C" int pmhip_gemm_heads_dh(int dtype, const void* A, int lda, const void* W, int ldw, int M, int K, int heads, int dim_head,
                                   int tokens, int tokens_pad, int nparts, const int* part_kinds_host, void* const* part_outs_host,
                                   float q_scale, float* scratch, pmhip_stream stream) {
    if (dim_head == 64)
        return pmhip_gemm_heads(dtype, A, lda, W, ldw, M, K, heads, tokens, tokens_pad, nparts, part_kinds_host, part_outs_host, q_scale,
                                stream);
    PM_TRY(check_dh("gemm_heads_dh", heads, dim_head));
    PM_REQUIRE(dtype == PMHIP_F32 || dtype == PMHIP_BF16, "gemm_heads_dh: bad dtype %d", dtype);
    PM_REQUIRE(nparts >= 1 && nparts <= 3 && part_kinds_host && part_outs_host, "gemm_heads_dh: nparts=%d", nparts);
    PM_REQUIRE(tokens > 0 && tokens_pad >= tokens && M > 0 && M % tokens == 0, "gemm_heads_dh: bad token geometry M=%d tokens=%d", M, tokens);
    PM_REQUIRE(scratch, "gemm_heads_dh: dim_head=%d needs the f32 scratch [M, nparts*heads*dim_head]", dim_head);
    SplitParams p{};
    p.src = scratch; p.M = M; p.nparts = nparts; p.heads = heads; p.dh = dim_head; p.tokens = tokens; p.tokens_pad = tokens_pad;
    p.q_scale = q_scale;
    for (int i = 0; i < nparts; ++i) {
        PM_REQUIRE(part_outs_host[i] && part_kinds_host[i] >= 0 && part_kinds_host[i] <= 2, "gemm_heads_dh: bad part %d", i);
        p.outs[i] = part_outs_host[i]; p.kinds[i] = part_kinds_host[i];
    }
    const int N = nparts * heads * dim_head;
    PM_TRY(pmhip_gemm(dtype, A, lda, W, ldw, nullptr, nullptr, 0, 0, scratch, N, PMHIP_F32, M, N, K, stream));
    hipStream_t s = (hipStream_t)stream;
    PmTimer tm(FAM_ROWOPS, s);
    const long long total = (long long)M * N;
    const int blocks = (int)((total + 255) / 256 < 65536 ? (total + 255) / 256 : 65536);
    if (dtype == PMHIP_F32) hipLaunchKernelGGL(head_split_kernel<float>, dim3(blocks), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(head_split_kernel<bf16_t>, dim3(blocks), dim3(256), 0, s, p);
    PM_HIP(hipGetLastError());
    return PMHIP_OK;
}

int pm_attn_check(const char* who, const PmAttnArgs& a) {
    PM_REQUIRE(!a.key_seg == !a.query_mask, "%s: key_seg and query_mask go together", who);
    if (a.pick) PM_REQUIRE(!a.lens != !a.key_seg, "%s: exactly one of kv_lens and the pair key_seg + query_mask selects the form", who);
    PM_REQUIRE(!(a.lens && a.key_seg), "%s: kv_lens and the pair key_seg + query_mask exclude each other (padding is segment 255)", who);
    PM_REQUIRE(!a.key_bias || a.key_seg, "%s: key_bias needs key_seg and query_mask beside it", who);
    if (a.pick) PM_REQUIRE(a.want >= 0 && a.want <= 255, "%s: want=%d is no value of a uint8 pick", who, a.want);
    return PMHIP_OK;
}

int pm_probs_check(const char* who, int dtype, int dim_head, int heads, std::initializer_list<PmContext> contexts) {
    PM_REQUIRE(dtype == PMHIP_F32 || dtype == PMHIP_BF16, "%s: bad dtype %d", who, dtype);
    PM_REQUIRE(dim_head >= 16 && dim_head <= 128 && dim_head % 16 == 0, "%s: dim_head=%d must be a multiple of 16 in [16,128]", who, dim_head);
    PM_REQUIRE(heads <= 64, "%s: heads=%d exceeds 64", who, heads);
    for (const PmContext& c : contexts) PM_REQUIRE(c.pad >= c.len, "%s: %s_pad=%d must be >= %s=%d", who, c.name, c.pad, c.name, c.len);
    return PMHIP_OK;
}

int attention_any(const char* who, int dtype, int dim_head, const PmAttnArgs& a) {
    const bool tuned = dim_head == 64;               // the MFMA kernels; otherwise this file's plain path
    PM_TRY(pm_attn_check(who, a));
    if (!tuned) PM_TRY(check_dh(who, a.heads, dim_head));
    PM_REQUIRE(dtype == PMHIP_F32 || dtype == PMHIP_BF16, "%s: bad dtype %d", who, dtype);
    PM_REQUIRE(a.Q && a.K && a.Vt && a.out, "%s: null pointer", who);
    PM_REQUIRE(a.B > 0 && a.heads > 0 && a.Nq > 0 && a.Nkv > 0, "%s: empty problem", who);
    if (tuned) {
        PM_REQUIRE(a.Nkv_pad % 64 == 0 && a.Nkv_pad >= a.Nkv, "%s: Nkv_pad=%d must be a multiple of 64 >= Nkv=%d", who, a.Nkv_pad, a.Nkv);
        PM_REQUIRE(a.ldo % 4 == 0 && (dtype == PMHIP_F32 || a.ldo % 8 == 0), "%s: ldo must be a multiple of 4 (f32) / 8 (bf16: 16-byte row stores)", who);
    } else {
        PM_REQUIRE(a.Nkv_pad >= a.Nkv, "%s: Nkv_pad=%d must be >= Nkv=%d", who, a.Nkv_pad, a.Nkv);
    }
    PM_REQUIRE(a.ldo >= a.heads * dim_head, "%s: ldo=%d is smaller than heads*dim_head=%d (rows of out would overlap)", who, a.ldo, a.heads * dim_head);
    if (!tuned) PM_REQUIRE((long long)a.B * a.heads <= 65535, "%s: B*heads=%lld exceeds the grid's y range", who, (long long)a.B * a.heads);
    PmTimer tm(FAM_ATTENTION, a.stream);
    if (!tuned) PM_TRY(dtype == PMHIP_F32 ? pm_attention_dh<float>(dim_head, a) : pm_attention_dh<bf16_t>(dim_head, a));
    else if (dtype == PMHIP_F32) pm_attention_f32(a);
    else pm_attention_bf16(a);
    PM_HIP(hipGetLastError());
    return PMHIP_OK;
}

// The C entry points: each checks the pointers that make it THIS entry, fills the record and calls attention_any.
static PmAttnArgs attn_record(const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads, int Nq, int Nkv, int Nkv_pad,
                              int use_exp2, pmhip_stream stream) {
    PmAttnArgs a{Q, K, Vt, out, ldo, B, heads, Nq, Nkv, Nkv_pad, use_exp2};
    a.stream = (hipStream_t)stream;
    return a;
}

extern "C" int pmhip_attention(int dtype, const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads, int Nq,
                               int Nkv, int Nkv_pad, int use_exp2, pmhip_stream stream) {
    PmAttnArgs a = attn_record(Q, K, Vt, out, ldo, B, heads, Nq, Nkv, Nkv_pad, use_exp2, stream);
   
    return attention_any("attention", dtype, 64, a);
}

extern "C" int pmhip_attention_dh(int dtype, const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads,
                                  int dim_head, int Nq, int Nkv, int Nkv_pad, int use_exp2, pmhip_stream stream) {
    PmAttnArgs a = attn_record(Q, K, Vt, out, ldo, B, heads, Nq, Nkv, Nkv_pad, use_exp2, stream);
   
    return attention_any(dim_head == 64 ? "attention" : "attention_dh", dtype, dim_head, a);
}

extern "C" int pmhip_attention_lens(int dtype, const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads,
                                    int dim_head, int Nq, int Nkv, int Nkv_pad, int use_exp2, const int32_t* kv_lens,
                                    pmhip_stream stream) {
    PM_REQUIRE(kv_lens, "attention_lens: kv_lens is NULL (pmhip_attention_dh is the entry without per-image key counts)");
    PmAttnArgs a = attn_record(Q, K, Vt, out, ldo, B, heads, Nq, Nkv, Nkv_pad, use_exp2, stream);
    a.lens = kv_lens;
    return attention_any("attention_lens", dtype, dim_head, a);
}

extern "C" int pmhip_attention_segments(int dtype, const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads,
                                        int dim_head, int Nq, int Nkv, int Nkv_pad, int use_exp2, const uint8_t* key_seg,
                                        const uint32_t* query_mask, pmhip_stream stream) {
    PM_REQUIRE(key_seg && query_mask, "attention_segments: key_seg / query_mask is NULL (pmhip_attention_dh is the entry without key sets)");
    PmAttnArgs a = attn_record(Q, K, Vt, out, ldo, B, heads, Nq, Nkv, Nkv_pad, use_exp2, stream);
    a.key_seg = key_seg; a.query_mask = query_mask;
    return attention_any("attention_segments", dtype, dim_head, a);
}

extern "C" int pmhip_attention_weighted(int dtype, const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads,
                                        int dim_head, int Nq, int Nkv, int Nkv_pad, int use_exp2, const uint8_t* key_seg,
                                        const uint32_t* query_mask, const float* key_bias, pmhip_stream stream) {
    PM_REQUIRE(key_seg && query_mask && key_bias,
               "attention_weighted: key_seg / query_mask / key_bias is NULL (pmhip_attention_segments is the entry without weights)");
    PmAttnArgs a = attn_record(Q, K, Vt, out, ldo, B, heads, Nq, Nkv, Nkv_pad, use_exp2, stream);
    a.key_seg = key_seg; a.query_mask = query_mask; a.key_bias = key_bias;
    return attention_any("attention_weighted", dtype, dim_head, a);
}

extern "C" int pmhip_key_bias(const float* weights, float* bias, int n, int use_exp2, pmhip_stream stream) {
    PM_REQUIRE(weights && bias, "key_bias: null pointer");
    PM_REQUIRE(n > 0, "key_bias: n=%d must be positive", n);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(key_bias_kernel, dim3((n + 255) / 256), dim3(256), 0, s, weights, bias, n, use_exp2);
    PM_HIP(hipGetLastError());
    return PMHIP_OK;
}

extern "C" int pmhip_attention_pick(int dtype, const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads,
                                    int dim_head, int Nq, int Nkv, int Nkv_pad, int use_exp2, const int32_t* kv_lens,
                                    const uint8_t* key_seg, const uint32_t* query_mask, const uint8_t* pick, int want,
                                    pmhip_stream stream) {
    PM_REQUIRE(pick, "attention_pick: pick is NULL (pmhip_attention_lens / pmhip_attention_segments are the entries that serve every image)");
    PmAttnArgs a = attn_record(Q, K, Vt, out, ldo, B, heads, Nq, Nkv, Nkv_pad, use_exp2, stream);
    a.lens = kv_lens; a.key_seg = key_seg; a.query_mask = query_mask; a.pick = pick; a.want = want;
    return attention_any("attention_pick", dtype, dim_head, a);
}

extern "C" int pmhip_attention_pick_weighted(int dtype, const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads,
                                             int dim_head, int Nq, int Nkv, int Nkv_pad, int use_exp2, const uint8_t* key_seg,
                                             const uint32_t* query_mask, const float* key_bias, const uint8_t* pick, int want,
                                             pmhip_stream stream) {
    PM_REQUIRE(pick, "attention_pick_weighted: pick is NULL (pmhip_attention_weighted is the entry that serves every image)");
    PM_REQUIRE(key_seg && query_mask && key_bias,
               "attention_pick_weighted: key_seg / query_mask / key_bias is NULL (pmhip_attention_pick is the entry without weights)");
    PmAttnArgs a = attn_record(Q, K, Vt, out, ldo, B, heads, Nq, Nkv, Nkv_pad, use_exp2, stream);
    a.key_seg = key_seg; a.query_mask = query_mask; a.key_bias = key_bias; a.pick = pick; a.want = want;
    return attention_any("attention_pick_weighted", dtype, dim_head, a);
}
