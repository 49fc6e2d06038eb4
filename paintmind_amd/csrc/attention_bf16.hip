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
#define PM_ATTN_BODY "attention_bf16_body.h"
#define PM_ATTN_NAME(sfx) attention_bf16##sfx##kernel
#define PM_ATTN_INSTANTIATE
#include "attention_forms.h"

#undef DSRX
#undef LGKM4
#undef LGKM2

// The forms with a key set per query exist with 128 or 64 queries per workgroup only (QF <= 2): the 256-query form with the masks
// does not fit in 256 VGPRs without more scratch than its twins, so it is not built.
template <int QF>
static void launch_qf(const PmAttnArgs& a) {
    const int nqb = ceil_div(a.Nq, 4 * QF * 16);
    const dim3 grid(nqb * a.B * a.heads), block(THREADS);
#define PM_ATTN_LAUNCH(form, sfx, ...)                                                                                                     \
    case PM_FORM_##form: {                                                                                                                 \
        auto k = a.use_exp2 ? PM_ATTN_NAME(sfx)<true, QF> : PM_ATTN_NAME(sfx)<false, QF>;                                                   \
        hipLaunchKernelGGL(k, grid, block, 0, a.stream, (const bf16_t*)a.Q, (const bf16_t*)a.K, (const bf16_t*)a.Vt, (bf16_t*)a.out, a.ldo, \
                           a.heads, a.Nq, a.Nkv, a.Nkv_pad, nqb, ##__VA_ARGS__);                                                           \
    } break;
    const PmAttnForm f = pm_attn_form(a);
    if (!a.key_seg) switch (f) { PM_ATTN_FORMS_IMAGE(PM_ATTN_LAUNCH) default: break; }
    else if constexpr (QF <= 2) switch (f) { PM_ATTN_FORMS_QUERY(PM_ATTN_LAUNCH) default: break; }
#undef PM_ATTN_LAUNCH
}

// The largest workgroup (64 * QF queries, QF <= max_qf) that still gives the chip two workgroups per CU (256 CUs on this part).  B,
// heads and Nq decide, never lens, the key sets, the biases or pick: the forms are bit-identical per 16-query tile, so an image's
// result depends neither on the choice nor on which images a launch serves.
static int queries_qf(int B, int heads, int Nq, int max_qf) {
#ifdef PM_ATTN_FORCE_QF              // tools/hwtests: one workgroup size for every launch (they launch the plain form only)
    return PM_ATTN_FORCE_QF < max_qf ? PM_ATTN_FORCE_QF : max_qf;
#else
    constexpr int kFill = 512;
    for (int qf = max_qf; qf > 1; qf /= 2)
        if ((long long)B * heads * ceil_div(Nq, 64 * qf) >= kFill) return qf;
    return 1;
#endif
}

}  // namespace

// bf16, dim_head = 64 leg of attention_any (attention_dh.hip): arguments already validated there
void pm_attention_bf16(const PmAttnArgs& a) {
    switch (queries_qf(a.B, a.heads, a.Nq, a.key_seg ? 2 : 4)) {
        case 4: launch_qf<4>(a); break;
        case 2: launch_qf<2>(a); break;
        default: launch_qf<1>(a);
    }
}
#undef PM_ATTN_BODY
#undef PM_ATTN_NAME
