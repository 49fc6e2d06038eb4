// Operand helpers of the attention kernels that give one wave 16 queries of one (image, head) and keep P in registers as its own MFMA
// operand (attention_relbias_kernel in t5ops.hip, attention_causal_kernel in clipops.hip).  Fragment maps (common.h, Mma): the score
// tile is computed TRANSPOSED, S^T = K . Q^T, so a lane holds S[key 4g + r, query c] (g = lane >> 4, c = lane & 15) in acc[r], and
// the probabilities a lane holds ARE its 16-byte operand chunk of P for O^T = V^T . P^T: chunk element e <-> key 16 (e / 4) + 4 g +
// e % 4 of the block.  load_vt reads the V^T operand from memory in the same order.
#pragma once

#include "common.h"

template <typename T> __device__ __forceinline__ uint4 pack_probs(const f32x4_t (&p)[Mma<T>::kElemsPerChunk / 4]);
template <> __device__ __forceinline__ uint4 pack_probs<bf16_t>(const f32x4_t (&p)[2]) {
    return make_uint4(pack_bf16x2(p[0][0], p[0][1]), pack_bf16x2(p[0][2], p[0][3]), pack_bf16x2(p[1][0], p[1][1]), pack_bf16x2(p[1][2], p[1][3]));
}
template <> __device__ __forceinline__ uint4 pack_probs<float>(const f32x4_t (&p)[1]) {
    return make_uint4(__float_as_uint(p[0][0]), __float_as_uint(p[0][1]), __float_as_uint(p[0][2]), __float_as_uint(p[0][3]));
}
// the V^T operand chunk of dim row `vrow` for the block at k0: NT groups of 4 consecutive keys; keys >= n are replaced by 0 and not read
__device__ __forceinline__ uint4 load_vt(const bf16_t* vrow, int k0, int g, int n, bool full) {
    uint32_t w[4];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int key = k0 + 16 * t + 4 * g;
        if (full) {
            const uint2 x = *reinterpret_cast<const uint2*>(vrow + key);
            w[2 * t] = x.x, w[2 * t + 1] = x.y;
        } else {
            uint32_t e[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) e[r] = key + r < n ? (uint32_t)vrow[key + r] : 0u;
            w[2 * t] = e[0] | (e[1] << 16), w[2 * t + 1] = e[2] | (e[3] << 16);
        }
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}
__device__ __forceinline__ uint4 load_vt(const float* vrow, int k0, int g, int n, bool full) {
    const int key = k0 + 4 * g;
    if (full) return *reinterpret_cast<const uint4*>(vrow + key);
    uint32_t e[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) e[r] = key + r < n ? __float_as_uint(vrow[key + r]) : 0u;
    return make_uint4(e[0], e[1], e[2], e[3]);
}
