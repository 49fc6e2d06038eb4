// Fused softmax(Q K^T) V in bf16 for dim_head = 64 (gfx950), fourth generation (the third-generation notes are kept below
// because the fourth builds on them).
// Replaces the reference's materialised-score attention (modules/attention.py:51-58: q@k^T -> softmax -> @v, a
// (B*H, N, N) fp32 tensor per layer) and its xformers alternative (:100).  Same data layout and work split as the
// f32 kernel in attention.hip (which stays the fp32-verify path): Q [B,H,Nq,64] pre-scaled, K [B,H,Np,64],
// V^T [B,H,64,Np]; one workgroup = 64*QF queries of one (batch, head), 4 waves x 16*QF queries (QF = 4, or 2 / 1 when the
// launch would otherwise leave CUs idle: bit-identical forms); K / V^T tiles of 64 keys by DMA into a 4-stage LDS ring with
// counted vmcnt waits, one bare s_barrier per tile; swapped QK^T (a lane owns 8 consecutive keys of ONE query per
// 32-key half-tile, so P feeds the P.V product straight from the S^T accumulators).
//
// What changed against the second generation (round 2: 0.40 MFMA busy, 4.5 VALU per MFMA):
//  * the row sums l = sum_k P[k, q] are computed by the MATRIX pipe: one extra MFMA per 16-query tile with an all-ones
//    row operand accumulates sum_k bf16(P) into an f32 accumulator whose 16 rows are all l (32 adds per half-tile ->
//    4 MFMAs; no cross-lane reduction at the end either).  l is therefore the sum of the ROUNDED probabilities, the
//    same values that multiply V.
//  * S^T accumulators start from -m by naming the running-max quad as the MFMA's C operand (D != C): no copies.
//  * growth of the running max is detected from ONE in-lane maximum over the lane's 32 scores (16 v_max3 instead of 20
//    + compares); the per-tile maxima are only computed inside the rare rescale branch.
//  * per half-tile the instruction stream is two blocks that each carry matrix work AND vector work:
//      A: 16 MFMAs of S^T(h+1)          with the 32 exponentials + 16 bf16 packs of S^T(h)
//      B: 20 MFMAs of P.V(h) + l(h)     with the 16 v_max3 of S^T(h+1)
//    V^T fragments of h are requested before block A, K fragments of h+2 before block B, so no LDS latency is exposed.
//
// Fourth generation (round 5): the steady loop has NO running-max bookkeeping at all.
//  * The reference max of a query is fixed after the first 32-key half-tile; every later probability is 2^(s - m_ref),
//    whatever its size.  bf16 P and the f32 accumulators have the exponent range of f32, so nothing is lost until a
//    probability overflows -- which the epilogue detects POST HOC (l not below 2^64, NaN included) and answers by running the
//    whole workgroup again through the exact path (running max raised at every half-tile: the rare-path code that ragged and
//    short contexts use anyway).  Round 4 counted the old growth branch on real data: 0 executions in 134 M steps, while
//    its detector was 16 of the 69 vector instructions of a half-tile.
//  * S^T is single-buffered and the half-tile is walked QUERY-TILE-major: group g issues the 4 QK^T MFMAs of S^T(h+1, g)
//    (overwriting S^T(h, g), whose exponentials were issued one group earlier), the 4 P.V MFMAs + the row-sum MFMA of
//    (h, g), and the 8 exponentials + 4 packs of (h, g+1).  Every group is 9 MFMAs beside 12 vector instructions: the
//    vector work is spread evenly under ALL matrix instructions (third generation: 3 per MFMA in block A, none in B).
#include <stdlib.h>

#include <type_traits>

#include "common.h"

#ifndef ABL
#define ABL 0                 // ablation bit mask (tools/hwtests/attn_abl.hip); 0 in the library
#endif

// workgroups whose fast path overflowed and that were run again through the exact path (pmhip_attention_fallbacks)
__device__ unsigned long long g_attn_fallbacks;
#ifndef PM_ATTN_NO_ABI           // tools/hwtests/attn_ab.hip compiles this file several times in one program
extern "C" int pmhip_attention_fallbacks(unsigned long long* count, int reset) {
    PM_REQUIRE(count != nullptr, "pmhip_attention_fallbacks: count is NULL");
    PM_HIP(hipDeviceSynchronize());
    PM_HIP(hipMemcpyFromSymbol(count, HIP_SYMBOL(g_attn_fallbacks), sizeof(unsigned long long)));
    if (reset) {
        const unsigned long long z = 0;
        PM_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_attn_fallbacks), &z, sizeof(z)));
    }
    return PMHIP_OK;
}
#endif

#ifdef PM_ATTN_COUNT
// DEBUG BUILD ONLY (tools/attn_rescale_count.sh): how often the steady loop leaves its fast path on real data.
// [1] fast half-tile steps (per wave), [2] exact steps
__device__ unsigned long long g_attn_counters[4];
extern "C" int pmhip_debug_attention_counters(unsigned long long* out4, int reset) {
    if (out4 && hipMemcpyFromSymbol(out4, HIP_SYMBOL(g_attn_counters), 32) != hipSuccess) return 1;
    if (reset) { unsigned long long z[4] = {0, 0, 0, 0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_attn_counters), z, 32) != hipSuccess) return 1; }
    return 0;
}
#endif

namespace {

constexpr int KT = 64;        // keys per tile
constexpr int DH = 64;
constexpr int THREADS = 256;
constexpr int TILE_BYTES = KT * 128;
constexpr int STAGE_BYTES = 2 * TILE_BYTES;              // K tile + V^T tile
#ifndef PM_ATTN_KSWZ
#define PM_ATTN_KSWZ 1        // 0: the K tile swizzle of rounds 3-4 (2-way bank conflicts on the K fragment reads); A/B only
#endif
#ifndef PM_ATTN_RING
#define PM_ATTN_RING 4
#endif
constexpr int RING = PM_ATTN_RING;       // ring stages: a tile is requested RING - 2 tiles before it is entered (round 5: 4;
                                         // with 3 the DMA had ONE tile period, about 1 us, to come back from HBM)
constexpr int AHEAD = RING - 2;

typedef __amdgpu_buffer_rsrc_t rsrc_t;
typedef unsigned v4u_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4_t mma(const v4u_t& rows, const v4u_t& cols, const f32x4_t& c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, rows), __builtin_bit_cast(bf16x8_t, cols), c, 0, 0, 0);
}

#if ABL & 2
#define DSRX(dst, addr, off) asm volatile("; no read %0 %1 %2" : "=v"(dst) : "v"(addr), "n"(off))
#else
#define DSRX(dst, addr, off) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off))
#endif
// one counted wait that names four fragments as in/out operands: every MFMA that consumes one is ordered behind it
#define LGKM4(n, a, b, c, d) asm volatile("s_waitcnt lgkmcnt(" #n ")" : "+v"(a), "+v"(b), "+v"(c), "+v"(d))
#define LGKM2(n, a, b) asm volatile("s_waitcnt lgkmcnt(" #n ")" : "+v"(a), "+v"(b))

// QF = 16-query tiles per wave: 4 (256 queries per workgroup) wherever that fills the chip; 2 and 1 (128 / 64 queries per
// workgroup) for small batches, where a grid of 256-query workgroups leaves most CUs idle (B = 1, H = 8, N = 1024: 32
// workgroups of 41 us each).  The arithmetic of a 16-query tile does not depend on QF or on its neighbours in the workgroup
// (same MFMA chains, same half-tile order, the fallback below decided per tile), so an image's result does not depend on the
// batch it runs in.
// (Measured and not adopted, round 5: ONE workgroup of 8 waves / 512 queries per CU sharing the ring -- half the DMA pieces per
// wave and per CU -- needs 13 % MORE cycles, 2.45e6 against 2.16e6 per launch, MFMA busy 0.49 against 0.55: the 8-wave barrier
// per tile costs more than the DMA saves; two independent 4-wave workgroups cover each other's barrier waits.  The patch is
// tools/ab_variants/attn_wv8.patch, the numbers profiles/r05_a_attention_gen4_ab.txt (5).)
// the kernel, in its two forms (attention_bf16_body.h)
#define PM_ATTN_KERNEL attention_bf16_kernel
#define PM_ATTN_LENS_PARAM
#include "attention_bf16_body.h"
#undef PM_ATTN_KERNEL
#undef PM_ATTN_LENS_PARAM
// the per-image form: Nkv_b = clamp(lens[b], 1, Nkv)
#define PM_ATTN_KERNEL attention_bf16_lens_kernel
#define PM_ATTN_LENS_PARAM , const int* __restrict__ lens
#define PM_ATTN_LENS 1
#include "attention_bf16_body.h"
#undef PM_ATTN_KERNEL
#undef PM_ATTN_LENS_PARAM
#undef PM_ATTN_LENS
// the per-query form: key k takes part in query q's softmax iff key_seg[b,k] < 32 and bit key_seg[b,k] of query_mask[b,q] is set
#define PM_ATTN_KERNEL attention_bf16_seg_kernel
#define PM_ATTN_LENS_PARAM , const unsigned char* __restrict__ key_seg, const unsigned* __restrict__ query_mask
#define PM_ATTN_SEG 1
#include "attention_bf16_body.h"
#undef PM_ATTN_KERNEL
#undef PM_ATTN_LENS_PARAM
#undef PM_ATTN_SEG
// the picked forms: the per-image and the per-query form again, each with `pick` (device uint8 [B]) and `want` --
// a workgroup whose image has pick[b] != want returns at once, every other one runs its twin's text
#define PM_ATTN_KERNEL attention_bf16_lens_pick_kernel
#define PM_ATTN_LENS_PARAM , const int* __restrict__ lens, const unsigned char* __restrict__ pick, int want
#define PM_ATTN_LENS 1
#define PM_ATTN_PICK 1
#include "attention_bf16_body.h"
#undef PM_ATTN_KERNEL
#undef PM_ATTN_LENS_PARAM
#undef PM_ATTN_LENS
#define PM_ATTN_KERNEL attention_bf16_seg_pick_kernel
#define PM_ATTN_LENS_PARAM , const unsigned char* __restrict__ key_seg, const unsigned* __restrict__ query_mask, const unsigned char* __restrict__ pick, int want
#define PM_ATTN_SEG 1
#include "attention_bf16_body.h"
#undef PM_ATTN_KERNEL
#undef PM_ATTN_LENS_PARAM
#undef PM_ATTN_SEG
#undef PM_ATTN_PICK
// the weighted form: the per-query form plus key_bias (device f32 [B, Nkv]), log(weight) of every key in the
// kernel's score unit, added to an allowed key's score before the maximum is taken; -inf = the key is padding
#define PM_ATTN_KERNEL attention_bf16_seg_bias_kernel
#define PM_ATTN_LENS_PARAM , const unsigned char* __restrict__ key_seg, const unsigned* __restrict__ query_mask, const float* __restrict__ key_bias
#define PM_ATTN_SEG 1
#define PM_ATTN_BIAS 1
#include "attention_bf16_body.h"
#undef PM_ATTN_KERNEL
#undef PM_ATTN_LENS_PARAM
#undef PM_ATTN_SEG
#undef PM_ATTN_BIAS
// the picked weighted form: the weighted form again with `pick` and `want` -- a workgroup whose image has
// pick[b] != want returns at once, every other one runs attention_bf16_seg_bias_kernel's text
#define PM_ATTN_KERNEL attention_bf16_seg_bias_pick_kernel
#define PM_ATTN_LENS_PARAM , const unsigned char* __restrict__ key_seg, const unsigned* __restrict__ query_mask, const float* __restrict__ key_bias, const unsigned char* __restrict__ pick, int want
#define PM_ATTN_SEG 1
#define PM_ATTN_BIAS 1
#define PM_ATTN_PICK 1
#include "attention_bf16_body.h"
#undef PM_ATTN_KERNEL
#undef PM_ATTN_LENS_PARAM
#undef PM_ATTN_SEG
#undef PM_ATTN_BIAS
#undef PM_ATTN_PICK

#undef DSRX
#undef LGKM4
#undef LGKM2

template <int QF>
static void launch_qf(const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads, int Nq, int Nkv, int Nkv_pad,
                      int use_exp2, const int* lens, hipStream_t s) {
    const int nqb = ceil_div(Nq, 4 * QF * 16);
    auto launch = [&](auto plain, auto per_image) {
        pm_launch_lens(plain, per_image, dim3(nqb * B * heads), dim3(THREADS), s, lens, (const bf16_t*)Q, (const bf16_t*)K, (const bf16_t*)Vt,
                       (bf16_t*)out, ldo, heads, Nq, Nkv, Nkv_pad, nqb);
    };
    if (use_exp2) launch(attention_bf16_kernel<true, QF>, attention_bf16_lens_kernel<true, QF>);
    else launch(attention_bf16_kernel<false, QF>, attention_bf16_lens_kernel<false, QF>);
}

template <int QF>
static void launch_seg_qf(const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads, int Nq, int Nkv, int Nkv_pad,
                          int use_exp2, const PmAttnSeg& seg, hipStream_t s) {
    const int nqb = ceil_div(Nq, 4 * QF * 16);
    auto k = use_exp2 ? attention_bf16_seg_kernel<true, QF> : attention_bf16_seg_kernel<false, QF>;
    hipLaunchKernelGGL(k, dim3(nqb * B * heads), dim3(THREADS), 0, s, (const bf16_t*)Q, (const bf16_t*)K, (const bf16_t*)Vt, (bf16_t*)out, ldo, heads,
                       Nq, Nkv, Nkv_pad, nqb, seg.key_seg, seg.query_mask);
}

// the weighted form: the geometry of the segmented twin
template <int QF>
static void launch_seg_bias_qf(const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads, int Nq, int Nkv, int Nkv_pad,
                               int use_exp2, const PmAttnSeg& seg, const float* key_bias, hipStream_t s) {
    const int nqb = ceil_div(Nq, 4 * QF * 16);
    auto k = use_exp2 ? attention_bf16_seg_bias_kernel<true, QF> : attention_bf16_seg_bias_kernel<false, QF>;
    hipLaunchKernelGGL(k, dim3(nqb * B * heads), dim3(THREADS), 0, s, (const bf16_t*)Q, (const bf16_t*)K, (const bf16_t*)Vt, (bf16_t*)out, ldo, heads,
                       Nq, Nkv, Nkv_pad, nqb, seg.key_seg, seg.query_mask, key_bias);
}

// the picked weighted form: the geometry of the weighted twin
template <int QF>
static void launch_seg_bias_pick_qf(const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads, int Nq, int Nkv,
                                    int Nkv_pad, int use_exp2, const PmAttnSeg& seg, const float* key_bias, const PmAttnPick& pk, hipStream_t s) {
    const int nqb = ceil_div(Nq, 4 * QF * 16);
    auto k = use_exp2 ? attention_bf16_seg_bias_pick_kernel<true, QF> : attention_bf16_seg_bias_pick_kernel<false, QF>;
    hipLaunchKernelGGL(k, dim3(nqb * B * heads), dim3(THREADS), 0, s, (const bf16_t*)Q, (const bf16_t*)K, (const bf16_t*)Vt, (bf16_t*)out, ldo, heads,
                       Nq, Nkv, Nkv_pad, nqb, seg.key_seg, seg.query_mask, key_bias, pk.pick, pk.want);
}

// the picked forms: exactly one of lens / seg, the geometry of the twin
template <int QF>
static void launch_pick_qf(const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads, int Nq, int Nkv, int Nkv_pad,
                           int use_exp2, const int* lens, const PmAttnSeg* seg, const PmAttnPick& pk, hipStream_t s) {
    const int nqb = ceil_div(Nq, 4 * QF * 16);
    if constexpr (QF <= 2) {
        if (seg) {
            auto k = use_exp2 ? attention_bf16_seg_pick_kernel<true, QF> : attention_bf16_seg_pick_kernel<false, QF>;
            hipLaunchKernelGGL(k, dim3(nqb * B * heads), dim3(THREADS), 0, s, (const bf16_t*)Q, (const bf16_t*)K, (const bf16_t*)Vt, (bf16_t*)out, ldo,
                               heads, Nq, Nkv, Nkv_pad, nqb, seg->key_seg, seg->query_mask, pk.pick, pk.want);
            return;
        }
    }
    auto k = use_exp2 ? attention_bf16_lens_pick_kernel<true, QF> : attention_bf16_lens_pick_kernel<false, QF>;
    hipLaunchKernelGGL(k, dim3(nqb * B * heads), dim3(THREADS), 0, s, (const bf16_t*)Q, (const bf16_t*)K, (const bf16_t*)Vt, (bf16_t*)out, ldo, heads,
                       Nq, Nkv, Nkv_pad, nqb, lens, pk.pick, pk.want);
}

}  // namespace

// bf16, dim_head = 64 leg of the attention entry points (attention_dh.hip): arguments already validated there; lens = device
// int32 [B], the per-image key counts, or NULL.  The largest workgroup that still gives the chip two workgroups per CU (256 CUs on
// this part: 512) is taken; the result of an image does not depend on the choice, and the choice looks at B, heads and Nq only --
// never at `lens`.
void pm_attention_bf16(const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads, int Nq, int Nkv,
                       int Nkv_pad, int use_exp2, const int* lens, hipStream_t s) {
#ifdef PM_ATTN_FORCE_QF
    constexpr int kFill = 0;
    const int force = PM_ATTN_FORCE_QF;
#else
    constexpr int kFill = 512;
    const int force = 0;
#endif
    const long long bh = (long long)B * heads;
    if (force == 4 || (!force && bh * ceil_div(Nq, 256) >= kFill)) launch_qf<4>(Q, K, Vt, out, ldo, B, heads, Nq, Nkv, Nkv_pad, use_exp2, lens, s);
    else if (force == 2 || (!force && bh * ceil_div(Nq, 128) >= kFill)) launch_qf<2>(Q, K, Vt, out, ldo, B, heads, Nq, Nkv, Nkv_pad, use_exp2, lens, s);
    else launch_qf<1>(Q, K, Vt, out, ldo, B, heads, Nq, Nkv, Nkv_pad, use_exp2, lens, s);
}

// The per-query form, a launcher of its own so that the one above keeps its signature (tools/hwtests build this file
// under several names and call it through one function-pointer type).  128 or 64 queries per workgroup only: the 256-query form
// with the masks does not fit in 256 VGPRs without more scratch than its twins, so it is not built.  Same rule otherwise -- B,
// heads and Nq decide, never the masks -- and the forms are bit-identical per 16-query tile.
void pm_attention_bf16_seg(const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads, int Nq, int Nkv,
                           int Nkv_pad, int use_exp2, const PmAttnSeg& seg, hipStream_t s) {
    if ((long long)B * heads * ceil_div(Nq, 128) >= 512) launch_seg_qf<2>(Q, K, Vt, out, ldo, B, heads, Nq, Nkv, Nkv_pad, use_exp2, seg, s);
    else launch_seg_qf<1>(Q, K, Vt, out, ldo, B, heads, Nq, Nkv, Nkv_pad, use_exp2, seg, s);
}

// The weighted form: the rule of pm_attention_bf16_seg, word for word -- B, heads and Nq decide between 128 and 64
// queries per workgroup, never the arrays --, and the forms are bit-identical per 16-query tile.
void pm_attention_bf16_seg_bias(const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads, int Nq, int Nkv,
                                int Nkv_pad, int use_exp2, const PmAttnSeg& seg, const float* key_bias, hipStream_t s) {
    if ((long long)B * heads * ceil_div(Nq, 128) >= 512)
        launch_seg_bias_qf<2>(Q, K, Vt, out, ldo, B, heads, Nq, Nkv, Nkv_pad, use_exp2, seg, key_bias, s);
    else launch_seg_bias_qf<1>(Q, K, Vt, out, ldo, B, heads, Nq, Nkv, Nkv_pad, use_exp2, seg, key_bias, s);
}

// The picked forms: the rule of the twin, from B, heads and Nq only -- never from `pick` --, so an image's bits do not
// depend on which images a launch serves.  lens: 256 / 128 / 64 queries per workgroup as pm_attention_bf16 (PM_ATTN_FORCE_QF builds
// do not reach this launcher); seg: 128 / 64 as pm_attention_bf16_seg.
void pm_attention_bf16_pick(const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads, int Nq, int Nkv,
                            int Nkv_pad, int use_exp2, const int* lens, const PmAttnSeg* seg, const PmAttnPick& pk, hipStream_t s) {
    const long long bh = (long long)B * heads;
    if (!seg && bh * ceil_div(Nq, 256) >= 512) launch_pick_qf<4>(Q, K, Vt, out, ldo, B, heads, Nq, Nkv, Nkv_pad, use_exp2, lens, seg, pk, s);
    else if (bh * ceil_div(Nq, 128) >= 512) launch_pick_qf<2>(Q, K, Vt, out, ldo, B, heads, Nq, Nkv, Nkv_pad, use_exp2, lens, seg, pk, s);
    else launch_pick_qf<1>(Q, K, Vt, out, ldo, B, heads, Nq, Nkv, Nkv_pad, use_exp2, lens, seg, pk, s);
}

// The picked weighted form: the rule of pm_attention_bf16_seg_bias, word for word -- B, heads and Nq decide between
// 128 and 64 queries per workgroup, never `pick` or the arrays --, so a served image's bits are those of the weighted launch.
void pm_attention_bf16_seg_bias_pick(const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads, int Nq, int Nkv,
                                     int Nkv_pad, int use_exp2, const PmAttnSeg& seg, const float* key_bias, const PmAttnPick& pk,
                                     hipStream_t s) {
    if ((long long)B * heads * ceil_div(Nq, 128) >= 512)
        launch_seg_bias_pick_qf<2>(Q, K, Vt, out, ldo, B, heads, Nq, Nkv, Nkv_pad, use_exp2, seg, key_bias, pk, s);
    else launch_seg_bias_pick_qf<1>(Q, K, Vt, out, ldo, B, heads, Nq, Nkv, Nkv_pad, use_exp2, seg, key_bias, pk, s);
}
