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

__device__ __forceinline__ float quad_sum(float v) {
    v += dpp_mov<0xB1>(v);      // quad_perm [1,0,3,2]
    v += dpp_mov<0x4E>(v);      // quad_perm [2,3,0,1]
    return v;
}

// DPL = dims per lane = dh / 4.  The kernel, in its two forms (attention_dh_body.h)
#define PM_ATTN_KERNEL attention_dh_kernel
#define PM_ATTN_LENS_PARAM
#include "attention_dh_body.h"
#undef PM_ATTN_KERNEL
#undef PM_ATTN_LENS_PARAM
// the per-image form: Nkv_b = clamp(lens[b], 1, Nkv)
#define PM_ATTN_KERNEL attention_dh_lens_kernel
#define PM_ATTN_LENS_PARAM , const int* __restrict__ lens
#define PM_ATTN_LENS 1
#include "attention_dh_body.h"
#undef PM_ATTN_KERNEL
#undef PM_ATTN_LENS_PARAM
#undef PM_ATTN_LENS
// the per-query form: key k takes part in query q's softmax iff key_seg[b,k] < 32 and bit key_seg[b,k] of query_mask[b,q] is set
#define PM_ATTN_KERNEL attention_dh_seg_kernel
#define PM_ATTN_LENS_PARAM , const unsigned char* __restrict__ key_seg, const unsigned* __restrict__ query_mask
#define PM_ATTN_SEG 1
#include "attention_dh_body.h"
#undef PM_ATTN_KERNEL
#undef PM_ATTN_LENS_PARAM
#undef PM_ATTN_SEG
// the picked forms: the per-image and the per-query form again, each with `pick` (device uint8 [B]) and `want` --
// a workgroup whose image has pick[b] != want returns at once, every other one runs its twin's text
#define PM_ATTN_KERNEL attention_dh_lens_pick_kernel
#define PM_ATTN_LENS_PARAM , const int* __restrict__ lens, const unsigned char* __restrict__ pick, int want
#define PM_ATTN_LENS 1
#define PM_ATTN_PICK 1
#include "attention_dh_body.h"
#undef PM_ATTN_KERNEL
#undef PM_ATTN_LENS_PARAM
#undef PM_ATTN_LENS
#define PM_ATTN_KERNEL attention_dh_seg_pick_kernel
#define PM_ATTN_LENS_PARAM , const unsigned char* __restrict__ key_seg, const unsigned* __restrict__ query_mask, const unsigned char* __restrict__ pick, int want
#define PM_ATTN_SEG 1
#include "attention_dh_body.h"
#undef PM_ATTN_KERNEL
#undef PM_ATTN_LENS_PARAM
#undef PM_ATTN_SEG
#undef PM_ATTN_PICK
// the weighted form: the per-query form plus key_bias (device f32 [B, Nkv]), log(weight) of every key in the
// kernel's score unit; -inf = the key is skipped like padding
#define PM_ATTN_KERNEL attention_dh_seg_bias_kernel
#define PM_ATTN_LENS_PARAM , const unsigned char* __restrict__ key_seg, const unsigned* __restrict__ query_mask, const float* __restrict__ key_bias
#define PM_ATTN_SEG 1
#define PM_ATTN_BIAS 1
#include "attention_dh_body.h"
#undef PM_ATTN_KERNEL
#undef PM_ATTN_LENS_PARAM
#undef PM_ATTN_SEG
#undef PM_ATTN_BIAS
// the picked weighted form: the weighted form again with `pick` and `want` -- a workgroup whose image has
// pick[b] != want returns at once, every other one runs attention_dh_seg_bias_kernel's text
#define PM_ATTN_KERNEL attention_dh_seg_bias_pick_kernel
#define PM_ATTN_LENS_PARAM , const unsigned char* __restrict__ key_seg, const unsigned* __restrict__ query_mask, const float* __restrict__ key_bias, const unsigned char* __restrict__ pick, int want
#define PM_ATTN_SEG 1
#define PM_ATTN_BIAS 1
#define PM_ATTN_PICK 1
#include "attention_dh_body.h"
#undef PM_ATTN_KERNEL
#undef PM_ATTN_LENS_PARAM
#undef PM_ATTN_SEG
#undef PM_ATTN_BIAS
#undef PM_ATTN_PICK

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
void launch_dh(const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads, int Nq, int Nkv, int Nkp,
               int use_exp2, const int* lens, const PmAttnSeg* seg, const PmAttnPick* pk, const float* bias, hipStream_t s) {
    if (bias && pk) {                                  // the picked weighted form: the geometry of the weighted twin
        auto k = use_exp2 ? attention_dh_seg_bias_pick_kernel<T, DPL, true> : attention_dh_seg_bias_pick_kernel<T, DPL, false>;
        hipLaunchKernelGGL(k, dim3((Nq + 63) / 64, B * heads), dim3(256), 0, s, (const T*)Q, (const T*)K, (const T*)Vt, (T*)out, ldo, heads, Nq,
                           Nkv, Nkp, seg->key_seg, seg->query_mask, bias, pk->pick, pk->want);
        return;
    }
    if (bias) {                                        // the weighted form: seg beside it
        auto k = use_exp2 ? attention_dh_seg_bias_kernel<T, DPL, true> : attention_dh_seg_bias_kernel<T, DPL, false>;
        hipLaunchKernelGGL(k, dim3((Nq + 63) / 64, B * heads), dim3(256), 0, s, (const T*)Q, (const T*)K, (const T*)Vt, (T*)out, ldo, heads, Nq,
                           Nkv, Nkp, seg->key_seg, seg->query_mask, bias);
        return;
    }
    if (pk) {                                          // the picked forms: exactly one of lens / seg, the geometry of the twin
        const dim3 grid((Nq + 63) / 64, B * heads);
        if (seg) {
            auto k = use_exp2 ? attention_dh_seg_pick_kernel<T, DPL, true> : attention_dh_seg_pick_kernel<T, DPL, false>;
            hipLaunchKernelGGL(k, grid, dim3(256), 0, s, (const T*)Q, (const T*)K, (const T*)Vt, (T*)out, ldo, heads, Nq, Nkv, Nkp, seg->key_seg,
                               seg->query_mask, pk->pick, pk->want);
        } else {
            auto k = use_exp2 ? attention_dh_lens_pick_kernel<T, DPL, true> : attention_dh_lens_pick_kernel<T, DPL, false>;
            hipLaunchKernelGGL(k, grid, dim3(256), 0, s, (const T*)Q, (const T*)K, (const T*)Vt, (T*)out, ldo, heads, Nq, Nkv, Nkp, lens, pk->pick,
                               pk->want);
        }
        return;
    }
    if (seg) {
        auto k = use_exp2 ? attention_dh_seg_kernel<T, DPL, true> : attention_dh_seg_kernel<T, DPL, false>;
        hipLaunchKernelGGL(k, dim3((Nq + 63) / 64, B * heads), dim3(256), 0, s, (const T*)Q, (const T*)K, (const T*)Vt, (T*)out, ldo, heads, Nq,
                           Nkv, Nkp, seg->key_seg, seg->query_mask);
        return;
    }
    auto launch = [&](auto plain, auto per_image) {
        pm_launch_lens(plain, per_image, dim3((Nq + 63) / 64, B * heads), dim3(256), s, lens, (const T*)Q, (const T*)K, (const T*)Vt, (T*)out,
                       ldo, heads, Nq, Nkv, Nkp);
    };
    if (use_exp2) launch(attention_dh_kernel<T, DPL, true>, attention_dh_lens_kernel<T, DPL, true>);
    else launch(attention_dh_kernel<T, DPL, false>, attention_dh_lens_kernel<T, DPL, false>);
}

// the launcher of this file's kernels: dim_head != 64, already passed through check_dh
template <typename T>
int pm_attention_dh(int dh, const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads, int Nq, int Nkv, int Nkp,
                    int use_exp2, const int* lens, const PmAttnSeg* seg, const PmAttnPick* pk, const float* bias, hipStream_t s) {
    switch (dh / 4) {
#define PM_DH_CASE(n) case n: launch_dh<T, n>(Q, K, Vt, out, ldo, B, heads, Nq, Nkv, Nkp, use_exp2, lens, seg, pk, bias, s); break;
        PM_DH_CASE(4) PM_DH_CASE(8) PM_DH_CASE(12) PM_DH_CASE(16) PM_DH_CASE(20) PM_DH_CASE(24) PM_DH_CASE(28) PM_DH_CASE(32)
#undef PM_DH_CASE
        default: PM_REQUIRE(false, "attention_dh: dim_head=%d not served", dh);
    }
    return PMHIP_OK;
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

// the dim_head = 64 launchers (attention.hip, attention_bf16.hip)
void pm_attention_f32(const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads, int Nq, int Nkv,
                      int Nkv_pad, int use_exp2, const int* lens, const PmAttnSeg* seg, hipStream_t s);
void pm_attention_bf16(const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads, int Nq, int Nkv,
                       int Nkv_pad, int use_exp2, const int* lens, hipStream_t s);
void pm_attention_bf16_seg(const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads, int Nq, int Nkv,
                           int Nkv_pad, int use_exp2, const PmAttnSeg& seg, hipStream_t s);
void pm_attention_f32_pick(const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads, int Nq, int Nkv,
                           int Nkv_pad, int use_exp2, const int* lens, const PmAttnSeg* seg, const PmAttnPick& pk, hipStream_t s);
void pm_attention_f32_seg_bias(const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads, int Nq, int Nkv,
                               int Nkv_pad, int use_exp2, const PmAttnSeg& seg, const float* key_bias, hipStream_t s);
void pm_attention_bf16_seg_bias(const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads, int Nq, int Nkv,
                                int Nkv_pad, int use_exp2, const PmAttnSeg& seg, const float* key_bias, hipStream_t s);
void pm_attention_bf16_pick(const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads, int Nq, int Nkv,
                            int Nkv_pad, int use_exp2, const int* lens, const PmAttnSeg* seg, const PmAttnPick& pk, hipStream_t s);
void pm_attention_f32_seg_bias_pick(const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads, int Nq, int Nkv,
                                    int Nkv_pad, int use_exp2, const PmAttnSeg& seg, const float* key_bias, const PmAttnPick& pk,
                                    hipStream_t s);
void pm_attention_bf16_seg_bias_pick(const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads, int Nq, int Nkv,
                                     int Nkv_pad, int use_exp2, const PmAttnSeg& seg, const float* key_bias, const PmAttnPick& pk,
                                     hipStream_t s);

// Every attention entry point ends here: the arguments are checked once, then one launcher per kernel file.  lens = device
// int32 [B], the per-image key counts, or NULL (one key count for the launch); seg = the per-query key sets (device arrays), or NULL;
// pk = the picked forms (exactly one of lens / seg beside it), or NULL; bias = the weighted form (seg beside it), or NULL; bias
// and pk together = the picked weighted form.
static int attention_any(const char* who, int dtype, const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads,
                         int dim_head, int Nq, int Nkv, int Nkv_pad, int use_exp2, const int* lens, hipStream_t s,
                         const PmAttnSeg* seg = nullptr, const PmAttnPick* pk = nullptr, const float* bias = nullptr) {
    const bool tuned = dim_head == 64;               // the MFMA kernels; otherwise this file's plain path
    if (!tuned) PM_TRY(check_dh(who, heads, dim_head));
    PM_REQUIRE(dtype == PMHIP_F32 || dtype == PMHIP_BF16, "%s: bad dtype %d", who, dtype);
    PM_REQUIRE(Q && K && Vt && out, "%s: null pointer", who);
    PM_REQUIRE(B > 0 && heads > 0 && Nq > 0 && Nkv > 0, "%s: empty problem", who);
    if (tuned) {
        PM_REQUIRE(Nkv_pad % 64 == 0 && Nkv_pad >= Nkv, "%s: Nkv_pad=%d must be a multiple of 64 >= Nkv=%d", who, Nkv_pad, Nkv);
        PM_REQUIRE(ldo % 4 == 0 && (dtype == PMHIP_F32 || ldo % 8 == 0), "%s: ldo must be a multiple of 4 (f32) / 8 (bf16: 16-byte row stores)", who);
    } else {
        PM_REQUIRE(Nkv_pad >= Nkv, "%s: Nkv_pad=%d must be >= Nkv=%d", who, Nkv_pad, Nkv);
    }
    PM_REQUIRE(ldo >= heads * dim_head, "%s: ldo=%d is smaller than heads*dim_head=%d (rows of out would overlap)", who, ldo, heads * dim_head);
    if (!tuned) PM_REQUIRE((long long)B * heads <= 65535, "%s: B*heads=%lld exceeds the grid's y range", who, (long long)B * heads);
    PmTimer tm(FAM_ATTENTION, s);
    if (!tuned) {
        if (dtype == PMHIP_F32) PM_TRY(pm_attention_dh<float>(dim_head, Q, K, Vt, out, ldo, B, heads, Nq, Nkv, Nkv_pad, use_exp2, lens, seg, pk, bias, s));
        else PM_TRY(pm_attention_dh<bf16_t>(dim_head, Q, K, Vt, out, ldo, B, heads, Nq, Nkv, Nkv_pad, use_exp2, lens, seg, pk, bias, s));
    } else if (bias && pk) {
        if (dtype == PMHIP_F32) pm_attention_f32_seg_bias_pick(Q, K, Vt, out, ldo, B, heads, Nq, Nkv, Nkv_pad, use_exp2, *seg, bias, *pk, s);
        else pm_attention_bf16_seg_bias_pick(Q, K, Vt, out, ldo, B, heads, Nq, Nkv, Nkv_pad, use_exp2, *seg, bias, *pk, s);
    } else if (bias) {
        if (dtype == PMHIP_F32) pm_attention_f32_seg_bias(Q, K, Vt, out, ldo, B, heads, Nq, Nkv, Nkv_pad, use_exp2, *seg, bias, s);
        else pm_attention_bf16_seg_bias(Q, K, Vt, out, ldo, B, heads, Nq, Nkv, Nkv_pad, use_exp2, *seg, bias, s);
    } else if (pk) {
        if (dtype == PMHIP_F32) pm_attention_f32_pick(Q, K, Vt, out, ldo, B, heads, Nq, Nkv, Nkv_pad, use_exp2, lens, seg, *pk, s);
        else pm_attention_bf16_pick(Q, K, Vt, out, ldo, B, heads, Nq, Nkv, Nkv_pad, use_exp2, lens, seg, *pk, s);
    } else if (dtype == PMHIP_F32) {
        pm_attention_f32(Q, K, Vt, out, ldo, B, heads, Nq, Nkv, Nkv_pad, use_exp2, lens, seg, s);
    } else {
        if (seg) pm_attention_bf16_seg(Q, K, Vt, out, ldo, B, heads, Nq, Nkv, Nkv_pad, use_exp2, *seg, s);
        else pm_attention_bf16(Q, K, Vt, out, ldo, B, heads, Nq, Nkv, Nkv_pad, use_exp2, lens, s);
    }
    PM_HIP(hipGetLastError());
    return PMHIP_OK;
}

extern "C" int pmhip_attention(int dtype, const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads, int Nq,
                               int Nkv, int Nkv_pad, int use_exp2, pmhip_stream stream) {
    return attention_any("attention", dtype, Q, K, Vt, out, ldo, B, heads, 64, Nq, Nkv, Nkv_pad, use_exp2, nullptr, (hipStream_t)stream);
}

extern "C" int pmhip_attention_dh(int dtype, const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads,
                                  int dim_head, int Nq, int Nkv, int Nkv_pad, int use_exp2, pmhip_stream stream) {
    return attention_any(dim_head == 64 ? "attention" : "attention_dh", dtype, Q, K, Vt, out, ldo, B, heads, dim_head, Nq, Nkv, Nkv_pad,
                         use_exp2, nullptr, (hipStream_t)stream);
}

extern "C" int pmhip_attention_lens(int dtype, const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads,
                                    int dim_head, int Nq, int Nkv, int Nkv_pad, int use_exp2, const int32_t* kv_lens,
                                    pmhip_stream stream) {
    PM_REQUIRE(kv_lens, "attention_lens: kv_lens is NULL (pmhip_attention_dh is the entry without per-image key counts)");
    return attention_any("attention_lens", dtype, Q, K, Vt, out, ldo, B, heads, dim_head, Nq, Nkv, Nkv_pad, use_exp2, kv_lens,
                         (hipStream_t)stream);
}

extern "C" int pmhip_attention_segments(int dtype, const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads,
                                        int dim_head, int Nq, int Nkv, int Nkv_pad, int use_exp2, const uint8_t* key_seg,
                                        const uint32_t* query_mask, pmhip_stream stream) {
    PM_REQUIRE(key_seg && query_mask, "attention_segments: key_seg / query_mask is NULL (pmhip_attention_dh is the entry without key sets)");
    const PmAttnSeg seg{key_seg, query_mask};
    return attention_any("attention_segments", dtype, Q, K, Vt, out, ldo, B, heads, dim_head, Nq, Nkv, Nkv_pad, use_exp2, nullptr,
                         (hipStream_t)stream, &seg);
}

extern "C" int pmhip_attention_weighted(int dtype, const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads,
                                        int dim_head, int Nq, int Nkv, int Nkv_pad, int use_exp2, const uint8_t* key_seg,
                                        const uint32_t* query_mask, const float* key_bias, pmhip_stream stream) {
    PM_REQUIRE(key_seg && query_mask && key_bias,
               "attention_weighted: key_seg / query_mask / key_bias is NULL (pmhip_attention_segments is the entry without weights)");
    const PmAttnSeg seg{key_seg, query_mask};
    return attention_any("attention_weighted", dtype, Q, K, Vt, out, ldo, B, heads, dim_head, Nq, Nkv, Nkv_pad, use_exp2, nullptr,
                         (hipStream_t)stream, &seg, nullptr, key_bias);
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
    PM_REQUIRE(!key_seg == !query_mask, "attention_pick: key_seg and query_mask go together");
    PM_REQUIRE(!kv_lens != !key_seg, "attention_pick: exactly one of kv_lens and the pair key_seg + query_mask selects the form");
    PM_REQUIRE(want >= 0 && want <= 255, "attention_pick: want=%d is no value of a uint8 pick", want);
    const PmAttnSeg seg{key_seg, query_mask};
    const PmAttnPick pk{pick, want};
    return attention_any("attention_pick", dtype, Q, K, Vt, out, ldo, B, heads, dim_head, Nq, Nkv, Nkv_pad, use_exp2, kv_lens,
                         (hipStream_t)stream, key_seg ? &seg : nullptr, &pk);
}

extern "C" int pmhip_attention_pick_weighted(int dtype, const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads,
                                             int dim_head, int Nq, int Nkv, int Nkv_pad, int use_exp2, const uint8_t* key_seg,
                                             const uint32_t* query_mask, const float* key_bias, const uint8_t* pick, int want,
                                             pmhip_stream stream) {
    PM_REQUIRE(pick, "attention_pick_weighted: pick is NULL (pmhip_attention_weighted is the entry that serves every image)");
    PM_REQUIRE(key_seg && query_mask && key_bias,
               "attention_pick_weighted: key_seg / query_mask / key_bias is NULL (pmhip_attention_pick is the entry without weights)");
    PM_REQUIRE(want >= 0 && want <= 255, "attention_pick_weighted: want=%d is no value of a uint8 pick", want);
    const PmAttnSeg seg{key_seg, query_mask};
    const PmAttnPick pk{pick, want};
    return attention_any("attention_pick_weighted", dtype, Q, K, Vt, out, ldo, B, heads, dim_head, Nq, Nkv, Nkv_pad, use_exp2, nullptr,
                         (hipStream_t)stream, &seg, &pk, key_bias);
}
