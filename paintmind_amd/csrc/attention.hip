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
#define PM_ATTN_BODY "attention_body.h"
#define PM_ATTN_NAME(sfx) attention##sfx##kernel
#define PM_ATTN_INSTANTIATE
#include "attention_forms.h"

}  // namespace

// fp32, dim_head = 64 leg of attention_any (attention_dh.hip): arguments already validated there
void pm_attention_f32(const PmAttnArgs& a) {
    constexpr int QF = 2;
    const int nqb = ceil_div(a.Nq, 4 * QF * 16);
    const dim3 grid(nqb * a.B * a.heads), block(THREADS);
#define PM_ATTN_LAUNCH(form, sfx, ...)                                                                                                  \
    case PM_FORM_##form: {                                                                                                              \
        auto k = a.use_exp2 ? PM_ATTN_NAME(sfx)<true, QF> : PM_ATTN_NAME(sfx)<false, QF>;                                                \
        hipLaunchKernelGGL(k, grid, block, 0, a.stream, (const float*)a.Q, (const float*)a.K, (const float*)a.Vt, (float*)a.out, a.ldo, \
                           a.heads, a.Nq, a.Nkv, a.Nkv_pad, nqb, ##__VA_ARGS__);                                                        \
    } break;
    switch (pm_attn_form(a)) { PM_ATTN_FORMS(PM_ATTN_LAUNCH) }
#undef PM_ATTN_LAUNCH
}
#undef PM_ATTN_BODY
#undef PM_ATTN_NAME
