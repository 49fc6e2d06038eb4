// Device helpers of the kernels that recompute softmax probabilities the flash kernels never hold: attention_maps.hip,
// attention_control.hip and attention_phrase.hip.  ONE definition of each piece; in particular the pair-control arithmetic below IS the
// P of prompt-to-prompt, for the kernel that attends with it and for the kernel that scores a phrase under it.
// Plain force-inlined functions: these kernels' instruction streams were compared per symbol before and after the move and did not
// change (profiles/attention_probs_refactor_isa.txt).  The flash kernels stay variants by text (attention_forms.h says why).
#pragma once
#include "common.h"

#include <cmath>

template <bool EXP2> __device__ __forceinline__ float prob_exp(float x) { return EXP2 ? exp2f(x) : expf(x); }

// one more key of an online softmax: (m, l) <- (max(m, s), l exp(m - max) + exp(s - max))
template <bool EXP2> __device__ __forceinline__ void prob_online(float& m, float& l, float s) {
    const float mn = fmaxf(m, s);
    l = fmaf(l, prob_exp<EXP2>(m - mn), prob_exp<EXP2>(s - mn));
    m = mn;
}

// workgroup-uniform: image b's key count of at most L (lens NULL: L), with the clamp of pmhip_attention_lens
__device__ __forceinline__ int prob_len(const int* lens, int b, int L) {
    if (!lens) return L;
    const int n = __builtin_amdgcn_readfirstlane(lens[b]);
    return n < 1 ? 1 : (n > L ? L : n);
}

// ---------------------------------------------------------------------------------------------------- the pair control
// Per pair b, over the target keys j < nt, with ps / pt the softmaxes of the source / edited pass over ns / nt keys:
//   m = row_map[b, j];  has = 0 <= m < ns and blend[b, j] != 0
//   P[q, j] = gain[b, j] * (has ? (1 - blend[b, j]) * pt[q, j] + blend[b, j] * ps[q, m] : pt[q, j])
struct PairControl {
    const int* row_map;                 // [B, Lt]
    const float* blend;                 // [B, Lt]
    const float* gain;                  // [B, Lt]
};
// target key j < nt of pair b: its gain, and whether (and from which source row, with which blend) the source takes part
struct PairKey {
    float gain, blend;
    int row;
    bool has;
};
__device__ __forceinline__ PairKey pair_key(const PairControl& c, int Lt, int b, int j, int ns) {
    const size_t at = (size_t)b * Lt + j;
    PairKey k;
    k.gain = c.gain[at]; k.blend = c.blend[at]; k.row = c.row_map[at];
    k.has = (k.row >= 0) & (k.row < ns) & (k.blend != 0.f);
    return k;
}
__device__ __forceinline__ float pair_mix(const PairKey& k, float pt, float ps) {
    const float mixed = fmaf(k.blend, ps, (1.f - k.blend) * pt);
    return k.gain * (k.has ? mixed : pt);
}

// ------------------------------------------------------------------------------- S^T = K Q^T by v_mfma_f32_16x16x32_bf16, dim_head 64
// Operands straight from global memory in fragment layout.  With col = lane & 15 and g = lane >> 4, a lane holds 8 dims per MFMA of
// its query col -- (f0, f1) = [8 g, 8 g + 8) and [32 + 8 g, 32 + 8 g + 8) -- and kb = the head's K + 8 g; it then holds the scores of
// ONE query and of keys 4 g + r of a 16-key tile.

// acc[r] = s[key row of lane (4 g + r)][query col]: `row` is the K row THIS lane feeds, as key (lane & 15) of the tile
__device__ __forceinline__ f32x4_t kq_scores(const bf16_t* kb, int row, const uint4& f0, const uint4& f1) {
    const uint4* kp = reinterpret_cast<const uint4*>(kb + (size_t)row * 64);
    const uint4 k0 = kp[0], k1 = kp[4];
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    Mma<bf16_t>::run(acc, k0, f0);
    Mma<bf16_t>::run(acc, k1, f1);
    return acc;
}
// pass 1: (m, 1 / l) of this lane's query over n keys; the four lanes of a query hold the key residues 4 g + r of every tile
template <bool EXP2>
__device__ __forceinline__ void kq_stats(const bf16_t* kb, int n, const uint4& f0, const uint4& f1, int col, int g, float& mx, float& inv) {
    float m = -INFINITY, l = 0.f;
    for (int k0 = 0; k0 < n; k0 += 16) {
        const int kr = k0 + col < n ? k0 + col : n - 1;         // no row at or behind n is read
        const f32x4_t s = kq_scores(kb, kr, f0, f1);
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (k0 + 4 * g + r < n) prob_online<EXP2>(m, l, s[r]);
    }
    mx = group4_max(m);
    const float ll = group4_sum(m == -INFINITY ? 0.f : l * prob_exp<EXP2>(m - mx));
    inv = 1.f / ll;                                             // n >= 1: key 0 takes part in every query
}
// The source scores of a tile's 16 target keys, the Ks ROWS gathered through row_map, into the tile `ss` the caller has zeroed: this
// lane feeds the row of key kj = tile + col.  Where `has` is false (or kj is at or behind nt) it feeds row 0 of the pair's own Ks --
// any lane must feed the matrix core something -- and the caller drops that score by a select; a tile without any source row stays
// 0 and costs no MFMA.  By TEXT, the one piece here that is: written out in the control and the phrase kernel, these lines compile
// to the two initialisations of (feed, srow) in opposite orders, and a function gives one order to both.
#define PM_KQ_GATHER(ss, c, Lt, b, kj, nt, ns, ksb, f0, f1)                                                           \
    do {                                                                                                              \
        bool feed = false; int srow = 0;                                                                              \
        if ((kj) < (nt)) {                                                                                            \
            const PairKey k = pair_key(c, Lt, b, kj, ns);                                                             \
            feed = k.has; srow = k.has ? k.row : 0;                                                                   \
        }                                                                                                             \
        if (__builtin_amdgcn_ballot_w64(feed) != 0) ss = kq_scores(ksb, srow, f0, f1);      /* (wave-uniform) */     \
    } while (0)

// --------------------------------------------------------------------------------------- the vector ALU, in the manner of attention_dh.hip
// 4 lanes share a query, each owning DPL = dim_head / 4 dims of q: lane `part` the dims from part * DPL (kb = the head's K + part * DPL).
// Pass 1 is `for (k < n) prob_online(m, l, quad_score(kb, k, q))` in the kernel itself: the loop inside a helper comes out with its
// back branch inverted.

// q . k over the quad, kp = this lane's DPL dims of the K row; every lane of the quad returns the score
template <typename T, int DPL> __device__ __forceinline__ float quad_score(const T* kp, const float (&q)[DPL]) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < DPL; ++i) s = fmaf(q[i], to_f32<T>(kp[i]), s);
    return quad_sum(s);
}
template <typename T, int DPL> __device__ __forceinline__ float quad_score(const T* kb, int row, const float (&q)[DPL]) {
    return quad_score<T, DPL>(kb + (size_t)row * (DPL * 4), q);
}
