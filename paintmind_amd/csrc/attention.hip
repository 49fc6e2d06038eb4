// Fused softmax(Q K^T) V in fp32 for dim_head = 64, no mask, no dropout (gfx950): the fp32-verify kernel, the reference the
// bf16 kernel (attention_bf16.hip) is tested against.
// Replaces the reference's materialised-score attention (modules/attention.py:51-58: q@k^T ->
// softmax -> @v, a (B*H, N, N) fp32 tensor per layer) and its xformers alternative (:100).
//
// Work split: one workgroup = 128 queries of one (batch, head): 4 waves x 2 tiles of 16 queries, so every K / V^T fragment
// read from LDS feeds 2 MFMAs.  K / V^T stream through a 3-stage LDS ring in tiles of 64 keys, written by DMA (glds16):
// on entering tile t a wave waits for its own DMA (vmcnt(0)), a barrier publishes the tile, and the DMA of tile t+1 goes
// out into the stage that tile t-2 has left.  In exp2 mode the running max is only raised (and O rescaled) when it
// grows by more than 2^8 (deferred rescale; P stays <= 256, l and O accumulate in fp32).
//
// MFMA formulation (16x16 tiles; operand chunk = 16 B = 4 floats per lane, see common.h Mma<float>):
//   S^T[key, query]  = K . Q^T     -> each lane holds ONE query column (lane&15) and 4 keys per tile,
//                                     so row max / row sum are in-lane plus two cross-lane steps.  The accumulators
//                                     start from -m (the column's running max), so the MFMA delivers s - m
//   O^T[d, query]   += V^T . P^T   -> P^T is consumed straight from the S^T accumulators: the lane's
//                                     keys are exactly the k-slice the column operand needs
// V arrives pre-transposed ([B,H,64,Nkv_pad], written by the projection GEMM's epilogue).
#include <type_traits>

#include "common.h"

namespace {

constexpr int KT = 64;        // keys per tile
constexpr int DH = 64;
constexpr int THREADS = 256;
constexpr int ROWB = 256;     // bytes per K row / per 64-key V^T row of a tile
constexpr int SLOTS = 16;     // 16-B chunks per row
constexpr int NCH = 4;        // MFMA k-steps over dim_head (16 floats each)

__device__ __forceinline__ uint4 lds_chunk(const unsigned char* tile, int row, int slot) {
    return *reinterpret_cast<const uint4*>(tile + row * ROWB + ((slot ^ (row & (SLOTS - 1))) << 4));
}

// zero the elements of a 16-B V^T chunk whose key index is >= nkv (first key of the chunk = k0)
__device__ __forceinline__ uint4 mask_keys(uint4 v, int k0, int nkv) {
    if (k0 + 0 >= nkv) v.x = 0u;
    if (k0 + 1 >= nkv) v.y = 0u;
    if (k0 + 2 >= nkv) v.z = 0u;
    if (k0 + 3 >= nkv) v.w = 0u;
    return v;
}

// One K tile + one V^T tile (64 rows x ROWB bytes each) go global -> LDS by DMA, 1 KiB per wave-instruction.
// The LDS image is lane-linear, so the bank swizzle (slot ^ row) is applied to the SOURCE address here and
// again in lds_chunk() on the read side.
__device__ __forceinline__ void stage_tiles(unsigned char* stage, const unsigned char* __restrict__ Kbh,
                                            const unsigned char* __restrict__ Vbh, size_t v_row_bytes, int t, int wave,
                                            int lane) {
    constexpr int RPC = 1024 / ROWB;                     // rows per 1 KiB chunk
    constexpr int CHUNKS = KT / RPC;                     // chunks per tile
    constexpr int PER_WAVE = CHUNKS / 4;
    const int kv0 = t * KT;
#pragma unroll
    for (int i = 0; i < PER_WAVE; ++i) {
        const int chunk = wave * PER_WAVE + i;
        const int row = chunk * RPC + lane / SLOTS;
        const int lslot = (lane % SLOTS) ^ (row & (SLOTS - 1));
        glds16(Kbh + (size_t)(kv0 + row) * ROWB + lslot * 16, stage + chunk * 1024);
        glds16(Vbh + (size_t)row * v_row_bytes + (size_t)kv0 * sizeof(float) + lslot * 16, stage + KT * ROWB + chunk * 1024);
    }
}

// ragged last tile: zero the V^T columns of keys >= Nkv (K needs nothing: those scores are masked to -inf)
__device__ __forceinline__ void zero_ragged_v(unsigned char* Vl, int kv0, int Nkv, int tid) {
    for (int idx = tid; idx < KT * SLOTS; idx += THREADS) {
        const int row = idx / SLOTS, lslot = idx % SLOTS;
        uint4* p = reinterpret_cast<uint4*>(Vl + row * ROWB + ((lslot ^ (row & (SLOTS - 1))) << 4));
        *p = mask_keys(*p, kv0 + lslot * 4, Nkv);
    }
}

// QF = 16-query tiles per wave (2: 32 queries per wave, 128 per workgroup).
// the kernel, in its two forms (attention_body.h)
#define PM_ATTN_KERNEL attention_kernel
#define PM_ATTN_LENS_PARAM
#include "attention_body.h"
#undef PM_ATTN_KERNEL
#undef PM_ATTN_LENS_PARAM
// the per-image form: Nkv_b = clamp(lens[b], 1, Nkv)
#define PM_ATTN_KERNEL attention_lens_kernel
#define PM_ATTN_LENS_PARAM , const int* __restrict__ lens
#define PM_ATTN_LENS 1
#include "attention_body.h"
#undef PM_ATTN_KERNEL
#undef PM_ATTN_LENS_PARAM
#undef PM_ATTN_LENS
// the per-query form: key k takes part in query q's softmax iff key_seg[b,k] < 32 and bit key_seg[b,k] of query_mask[b,q] is set
#define PM_ATTN_KERNEL attention_seg_kernel
#define PM_ATTN_LENS_PARAM , const unsigned char* __restrict__ key_seg, const unsigned* __restrict__ query_mask
#define PM_ATTN_SEG 1
#include "attention_body.h"
#undef PM_ATTN_KERNEL
#undef PM_ATTN_LENS_PARAM
#undef PM_ATTN_SEG
// the picked forms: the per-image and the per-query form again, each with `pick` (device uint8 [B]) and `want` --
// a workgroup whose image has pick[b] != want returns at once, every other one runs its twin's text
#define PM_ATTN_KERNEL attention_lens_pick_kernel
#define PM_ATTN_LENS_PARAM , const int* __restrict__ lens, const unsigned char* __restrict__ pick, int want
#define PM_ATTN_LENS 1
#define PM_ATTN_PICK 1
#include "attention_body.h"
#undef PM_ATTN_KERNEL
#undef PM_ATTN_LENS_PARAM
#undef PM_ATTN_LENS
#define PM_ATTN_KERNEL attention_seg_pick_kernel
#define PM_ATTN_LENS_PARAM , const unsigned char* __restrict__ key_seg, const unsigned* __restrict__ query_mask, const unsigned char* __restrict__ pick, int want
#define PM_ATTN_SEG 1
#include "attention_body.h"
#undef PM_ATTN_KERNEL
#undef PM_ATTN_LENS_PARAM
#undef PM_ATTN_SEG
#undef PM_ATTN_PICK
// the weighted form: the per-query form plus key_bias (device f32 [B, Nkv]), log(weight) of every key in the
// kernel's score unit; -inf = the key is padding
#define PM_ATTN_KERNEL attention_seg_bias_kernel
#define PM_ATTN_LENS_PARAM , const unsigned char* __restrict__ key_seg, const unsigned* __restrict__ query_mask, const float* __restrict__ key_bias
#define PM_ATTN_SEG 1
#define PM_ATTN_BIAS 1
#include "attention_body.h"
#undef PM_ATTN_KERNEL
#undef PM_ATTN_LENS_PARAM
#undef PM_ATTN_SEG
#undef PM_ATTN_BIAS
// the picked weighted form: the weighted form again with `pick` and `want` -- a workgroup whose image has
// pick[b] != want returns at once, every other one runs attention_seg_bias_kernel's text
#define PM_ATTN_KERNEL attention_seg_bias_pick_kernel
#define PM_ATTN_LENS_PARAM , const unsigned char* __restrict__ key_seg, const unsigned* __restrict__ query_mask, const float* __restrict__ key_bias, const unsigned char* __restrict__ pick, int want
#define PM_ATTN_SEG 1
#define PM_ATTN_BIAS 1
#define PM_ATTN_PICK 1
#include "attention_body.h"
#undef PM_ATTN_KERNEL
#undef PM_ATTN_LENS_PARAM
#undef PM_ATTN_SEG
#undef PM_ATTN_BIAS
#undef PM_ATTN_PICK

}  // namespace

// fp32, dim_head = 64 leg of the attention entry points (attention_dh.hip): arguments already validated there;
// lens = device int32 [B], the per-image key counts, or NULL; seg = the per-query key sets, or NULL (never both)
void pm_attention_f32(const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads, int Nq, int Nkv,
                      int Nkv_pad, int use_exp2, const int* lens, const PmAttnSeg* seg, hipStream_t s) {
    constexpr int QF = 2;
    const int nqb = ceil_div(Nq, 4 * QF * 16);
    if (seg) {
        auto k = use_exp2 ? attention_seg_kernel<true, QF> : attention_seg_kernel<false, QF>;
        hipLaunchKernelGGL(k, dim3(nqb * B * heads), dim3(THREADS), 0, s, (const float*)Q, (const float*)K, (const float*)Vt, (float*)out, ldo, heads,
                           Nq, Nkv, Nkv_pad, nqb, seg->key_seg, seg->query_mask);
        return;
    }
    auto launch = [&](auto plain, auto per_image) {
        pm_launch_lens(plain, per_image, dim3(nqb * B * heads), dim3(THREADS), s, lens, (const float*)Q, (const float*)K, (const float*)Vt,
                       (float*)out, ldo, heads, Nq, Nkv, Nkv_pad, nqb);
    };
    if (use_exp2) launch(attention_kernel<true, QF>, attention_lens_kernel<true, QF>);
    else launch(attention_kernel<false, QF>, attention_lens_kernel<false, QF>);
}

// The weighted form, a launcher of its own so that the one above keeps its text: the grid and the workgroup of the
// segmented twin.
void pm_attention_f32_seg_bias(const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads, int Nq, int Nkv,
                               int Nkv_pad, int use_exp2, const PmAttnSeg& seg, const float* key_bias, hipStream_t s) {
    constexpr int QF = 2;
    const int nqb = ceil_div(Nq, 4 * QF * 16);
    auto k = use_exp2 ? attention_seg_bias_kernel<true, QF> : attention_seg_bias_kernel<false, QF>;
    hipLaunchKernelGGL(k, dim3(nqb * B * heads), dim3(THREADS), 0, s, (const float*)Q, (const float*)K, (const float*)Vt, (float*)out, ldo, heads,
                       Nq, Nkv, Nkv_pad, nqb, seg.key_seg, seg.query_mask, key_bias);
}

// The picked forms, a launcher of their own so that the one above keeps its text: exactly one of lens / seg is given,
// the grid and the workgroup are those of the twin.
void pm_attention_f32_pick(const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads, int Nq, int Nkv,
                           int Nkv_pad, int use_exp2, const int* lens, const PmAttnSeg* seg, const PmAttnPick& pk, hipStream_t s) {
    constexpr int QF = 2;
    const int nqb = ceil_div(Nq, 4 * QF * 16);
    if (seg) {
        auto k = use_exp2 ? attention_seg_pick_kernel<true, QF> : attention_seg_pick_kernel<false, QF>;
        hipLaunchKernelGGL(k, dim3(nqb * B * heads), dim3(THREADS), 0, s, (const float*)Q, (const float*)K, (const float*)Vt, (float*)out, ldo, heads,
                           Nq, Nkv, Nkv_pad, nqb, seg->key_seg, seg->query_mask, pk.pick, pk.want);
        return;
    }
    auto k = use_exp2 ? attention_lens_pick_kernel<true, QF> : attention_lens_pick_kernel<false, QF>;
    hipLaunchKernelGGL(k, dim3(nqb * B * heads), dim3(THREADS), 0, s, (const float*)Q, (const float*)K, (const float*)Vt, (float*)out, ldo, heads,
                       Nq, Nkv, Nkv_pad, nqb, lens, pk.pick, pk.want);
}

// The picked weighted form, a launcher of its own again: the grid and the workgroup of the weighted twin.
void pm_attention_f32_seg_bias_pick(const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads, int Nq, int Nkv,
                                    int Nkv_pad, int use_exp2, const PmAttnSeg& seg, const float* key_bias, const PmAttnPick& pk,
                                    hipStream_t s) {
    constexpr int QF = 2;
    const int nqb = ceil_div(Nq, 4 * QF * 16);
    auto k = use_exp2 ? attention_seg_bias_pick_kernel<true, QF> : attention_seg_bias_pick_kernel<false, QF>;
    hipLaunchKernelGGL(k, dim3(nqb * B * heads), dim3(THREADS), 0, s, (const float*)Q, (const float*)K, (const float*)Vt, (float*)out, ldo, heads,
                       Nq, Nkv, Nkv_pad, nqb, seg.key_seg, seg.query_mask, key_bias, pk.pick, pk.want);
}
