// Fused softmax(Q K^T) V for dim_head = 64, no mask, no dropout (gfx950): the fp32-verify kernel (bf16: attention_bf16.hip).
// Replaces the reference's materialised-score attention (modules/attention.py:51-58: q@k^T ->
// softmax -> @v, a (B*H, N, N) fp32 tensor per layer) and its xformers alternative (:100).
//
// Work split: one workgroup = 256 queries (bf16; 128 in f32) of one (batch, head); 4 waves x 64 queries, so
// every K / V^T fragment read from LDS feeds 4 MFMAs.  K/V stream through a 2-stage LDS ring in tiles of
// 64 keys: tile t+1 is written (from registers loaded one iteration earlier) while tile t is being
// multiplied, one barrier per tile.  In exp2 mode the running max is only raised (and O rescaled) when it
// grows by more than 2^8 (deferred rescale; P stays <= 256, l and O accumulate in fp32).
//
// MFMA formulation (16x16 tiles; operand chunk = 16 B per lane, see common.h Mma<T>):
//   S^T[key, query]  = K . Q^T     -> each lane holds ONE query column (lane&15) and 4 keys per tile,
//                                     so row max / row sum are in-lane plus two cross-lane steps
//   O^T[d, query]   += V^T . P^T   -> P^T is consumed straight from the S^T accumulators: the lane's
//                                     keys are exactly the k-slice the column operand needs
// For bf16 the K rows of a tile are read in a permuted order so that the 8 keys a lane owns across
// two S^T tiles are CONTIGUOUS, which makes the matching V^T operand one ds_read_b128.
// V arrives pre-transposed ([B,H,64,Nkv_pad], written by the projection GEMM's epilogue).
#include <stdlib.h>

#include <type_traits>

#include "common.h"

namespace {

constexpr int KT = 64;        // keys per tile
constexpr int DH = 64;
constexpr int THREADS = 256;

template <typename T> struct AttnCfg;
// (the bf16 instantiation of this kernel -- the round-2 bf16 path behind PMHIP_ATTN_OLD -- left the library in round 6: bf16 is
// served by attention_bf16.hip; this file is the fp32-verify kernel)
template <> struct AttnCfg<float> {
    static constexpr int ROWB = 256;
    static constexpr int SLOTS = 16;
    static constexpr int NCH = 4;
};

// tile row (key within the 64-key tile) that S^T tile kf presents as its row i (i = 0..15)
template <typename T> __device__ __forceinline__ int key_of_row(int kf, int i);
template <> __device__ __forceinline__ int key_of_row<bf16_t>(int kf, int i) {
    return 32 * (kf >> 1) + 8 * (i >> 2) + 4 * (kf & 1) + (i & 3);
}
template <> __device__ __forceinline__ int key_of_row<float>(int kf, int i) { return 16 * kf + i; }

template <typename T>
__device__ __forceinline__ uint4 lds_chunk(const unsigned char* tile, int row, int slot) {
    using C = AttnCfg<T>;
    return *reinterpret_cast<const uint4*>(tile + row * C::ROWB + ((slot ^ (row & (C::SLOTS - 1))) << 4));
}

// zero the elements of a 16-B V^T chunk whose key index is >= nkv (first key of the chunk = k0)
template <typename T> __device__ __forceinline__ uint4 mask_keys(uint4 v, int k0, int nkv);
template <> __device__ __forceinline__ uint4 mask_keys<bf16_t>(uint4 v, int k0, int nkv) {
    const int n = nkv - k0;                      // number of valid keys in this 8-key chunk (may be <= 0)
    v.x = n <= 0 ? 0u : (n == 1 ? (v.x & 0xffffu) : v.x);
    v.y = n <= 2 ? 0u : (n == 3 ? (v.y & 0xffffu) : v.y);
    v.z = n <= 4 ? 0u : (n == 5 ? (v.z & 0xffffu) : v.z);
    v.w = n <= 6 ? 0u : (n == 7 ? (v.w & 0xffffu) : v.w);
    return v;
}
template <> __device__ __forceinline__ uint4 mask_keys<float>(uint4 v, int k0, int nkv) {
    if (k0 + 0 >= nkv) v.x = 0u;
    if (k0 + 1 >= nkv) v.y = 0u;
    if (k0 + 2 >= nkv) v.z = 0u;
    if (k0 + 3 >= nkv) v.w = 0u;
    return v;
}

template <typename T> __device__ __forceinline__ uint4 pack_p(const f32x4_t& lo, const f32x4_t& hi);
template <> __device__ __forceinline__ uint4 pack_p<bf16_t>(const f32x4_t& lo, const f32x4_t& hi) {
    return make_uint4(pack_bf16x2(lo[0], lo[1]), pack_bf16x2(lo[2], lo[3]), pack_bf16x2(hi[0], hi[1]),
                      pack_bf16x2(hi[2], hi[3]));
}

// One K tile + one V^T tile (64 rows x ROWB bytes each) go global -> LDS by DMA, 1 KiB per wave-instruction.
// The LDS image is lane-linear, so the bank swizzle (slot ^ row) is applied to the SOURCE address here and
// again in lds_chunk() on the read side.
template <typename T>
__device__ __forceinline__ void stage_tiles(unsigned char* stage, const unsigned char* __restrict__ Kbh,
                                            const unsigned char* __restrict__ Vbh, size_t v_row_bytes, int t, int wave,
                                            int lane) {
    using C = AttnCfg<T>;
    constexpr int RPC = 1024 / C::ROWB;                  // rows per 1 KiB chunk
    constexpr int CHUNKS = KT / RPC;                     // chunks per tile
    constexpr int PER_WAVE = CHUNKS / 4;
    const int kv0 = t * KT;
#pragma unroll
    for (int i = 0; i < PER_WAVE; ++i) {
        const int chunk = wave * PER_WAVE + i;
        const int row = chunk * RPC + lane / C::SLOTS;
        const int lslot = (lane % C::SLOTS) ^ (row & (C::SLOTS - 1));
        glds16(Kbh + (size_t)(kv0 + row) * C::ROWB + lslot * 16, stage + chunk * 1024);
        glds16(Vbh + (size_t)row * v_row_bytes + (size_t)kv0 * sizeof(T) + lslot * 16, stage + KT * C::ROWB + chunk * 1024);
    }
}

// bf16 form of stage_tiles on `buffer_load_dwordx4 ... lds`: descriptors based at the (batch, head)'s K / V^T, ONE per-lane
// vector offset each (row-in-chunk and swizzled slot do not depend on the chunk: chunks start at multiples of 8 rows), the
// chunk / tile position in the scalar offset -- no VALU address arithmetic per instruction.
typedef __amdgpu_buffer_rsrc_t rsrc_t;
__device__ __forceinline__ void stage_tiles_bf16(unsigned char* stage, rsrc_t Kr, rsrc_t Vr, unsigned kvoff, unsigned vvoff,
                                                 unsigned v_row_bytes, int t, int wave) {
    constexpr int PER_WAVE = 2;                          // 8 chunks of 8 rows per tile, 4 waves
    const unsigned kv0 = (unsigned)t * KT;
#pragma unroll
    for (int i = 0; i < PER_WAVE; ++i) {
        const unsigned chunk = (unsigned)wave * PER_WAVE + i;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(Kr, (__attribute__((address_space(3))) void*)(stage + chunk * 1024), 16, kvoff,
                                                 (kv0 + chunk * 8) * 128u, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(Vr, (__attribute__((address_space(3))) void*)(stage + KT * 128 + chunk * 1024), 16, vvoff,
                                                 chunk * 8 * v_row_bytes + kv0 * 2u, 0, 0);
    }
}

// ragged last tile: zero the V^T columns of keys >= Nkv (K needs nothing: those scores are masked to -inf)
template <typename T>
__device__ __forceinline__ void zero_ragged_v(unsigned char* Vl, int kv0, int Nkv, int tid) {
    using C = AttnCfg<T>;
    for (int idx = tid; idx < KT * C::SLOTS; idx += THREADS) {
        const int row = idx / C::SLOTS, lslot = idx % C::SLOTS;
        uint4* p = reinterpret_cast<uint4*>(Vl + row * C::ROWB + ((lslot ^ (row & (C::SLOTS - 1))) << 4));
        *p = mask_keys<T>(*p, kv0 + lslot * (16 / (int)sizeof(T)), Nkv);
    }
}

// QF = 16-query tiles per wave (bf16: 4 -> 64 queries per wave, 256 per workgroup; f32: 2).
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

}  // namespace

int pm_attention_bf16(const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads, int Nq, int Nkv,
                      int Nkv_pad, int use_exp2, hipStream_t s);
int pm_attention_bf16_lens(const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads, int Nq, int Nkv,
                           int Nkv_pad, int use_exp2, const int* lens, hipStream_t s);

// pmhip_attention, and the dim_head = 64 leg of pmhip_attention_lens (attention_dh.hip): lens = device int32 [B] or NULL
int pm_attention64(const char* who, int dtype, const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads,
                   int Nq, int Nkv, int Nkv_pad, int use_exp2, const int* lens, hipStream_t s) {
    PM_REQUIRE(dtype == PMHIP_F32 || dtype == PMHIP_BF16, "%s: bad dtype %d", who, dtype);
    PM_REQUIRE(Q && K && Vt && out, "%s: null pointer", who);
    PM_REQUIRE(B > 0 && heads > 0 && Nq > 0 && Nkv > 0, "%s: empty problem", who);
    PM_REQUIRE(Nkv_pad % KT == 0 && Nkv_pad >= Nkv, "%s: Nkv_pad=%d must be a multiple of 64 >= Nkv=%d", who, Nkv_pad, Nkv);
    PM_REQUIRE(ldo % 4 == 0 && (dtype == PMHIP_F32 || ldo % 8 == 0), "%s: ldo must be a multiple of 4 (f32) / 8 (bf16: 16-byte row stores)", who);
    PM_REQUIRE(ldo >= heads * DH, "%s: ldo=%d is smaller than heads*64=%d (rows of out would overlap)", who, ldo, heads * DH);
    dim3 block(THREADS);
    PmTimer tm(FAM_ATTENTION, s);
    if (dtype == PMHIP_F32) {
        const int nqb = ceil_div(Nq, 4 * 2 * 16);
        dim3 grid(nqb * B * heads);
        if (lens) {
            if (use_exp2)
                hipLaunchKernelGGL((attention_lens_kernel<float, true, 2>), grid, block, 0, s, (const float*)Q, (const float*)K,
                                   (const float*)Vt, (float*)out, ldo, heads, Nq, Nkv, Nkv_pad, nqb, lens);
            else
                hipLaunchKernelGGL((attention_lens_kernel<float, false, 2>), grid, block, 0, s, (const float*)Q, (const float*)K,
                                   (const float*)Vt, (float*)out, ldo, heads, Nq, Nkv, Nkv_pad, nqb, lens);
        } else if (use_exp2)
            hipLaunchKernelGGL((attention_kernel<float, true, 2>), grid, block, 0, s, (const float*)Q, (const float*)K,
                               (const float*)Vt, (float*)out, ldo, heads, Nq, Nkv, Nkv_pad, nqb);
        else
            hipLaunchKernelGGL((attention_kernel<float, false, 2>), grid, block, 0, s, (const float*)Q, (const float*)K,
                               (const float*)Vt, (float*)out, ldo, heads, Nq, Nkv, Nkv_pad, nqb);
    } else {
        if (lens) PM_TRY(pm_attention_bf16_lens(Q, K, Vt, out, ldo, B, heads, Nq, Nkv, Nkv_pad, use_exp2, lens, s));
        else PM_TRY(pm_attention_bf16(Q, K, Vt, out, ldo, B, heads, Nq, Nkv, Nkv_pad, use_exp2, s));
    }
    PM_HIP(hipGetLastError());
    return PMHIP_OK;
}

extern "C" int pmhip_attention(int dtype, const void* Q, const void* K, const void* Vt, void* out, int ldo,
                               int B, int heads, int Nq, int Nkv, int Nkv_pad, int use_exp2,
                               pmhip_stream stream) {
    return pm_attention64("attention", dtype, Q, K, Vt, out, ldo, B, heads, Nq, Nkv, Nkv_pad, use_exp2, nullptr, (hipStream_t)stream);
}
