// Cross-attention maps: the head-mean softmax probabilities of one attention launch, materialised.
//
//   maps[b, q, k] (+)= scale / heads * sum_h p_h[q, k]        p_h = the softmax the matching attention entry defines
//
// The flash kernels never hold a row of P; this file recomputes it from the same Q and K under the same lengths, key sets and key
// biases.  Two kernels, one structure -- a workgroup owns one image and 64 queries and walks the context twice:
//   pass 1, per head : the maximum m and the sum l of every query row over the keys that take part; (m, 1 / l) per (head, query)
//                      goes to LDS (heads * 64 pairs)
//   pass 2, per chunk of keys : loop over the heads h = 0 .. heads-1, recompute the chunk's scores, add exp(s - m_h) / l_h in
//                      registers, store the chunk ONCE
// so registers and LDS do not depend on Nkv, the sum over the heads has a fixed order inside one thread, every element of `maps` is
// written by exactly one thread once per launch, and there are no atomics.  P stays f32 in both dtypes.
//   attention_maps_mfma_kernel  bf16, dim_head 64: S = Q K^T by v_mfma_f32_16x16x32_bf16, both operands straight from global memory
//                               in fragment layout (a lane holds 8 contiguous bf16 of one Q row / one K row); a wave owns 16 queries,
//                               the result has the key on lane & 15 and the query on (lane >> 4) * 4 + reg; chunks of 64 keys
//   attention_maps_valu_kernel  everything else (fp32, dim_head != 64), in the manner of attention_dh.hip: 4 lanes share a query,
//                               each owning dh / 4 dims, the score is a quad reduction; chunks of 16 keys, 4 per lane of the quad
// A key that takes part in no softmax of a query (behind the image's length, a denied segment, segment 255, bias -inf) contributes
// through a select, never through arithmetic: NaN in its K row reaches nothing, and its element is written as 0.0f (left alone
// under `accumulate`).  K rows are read below Nkv only (tile tails re-read row Nkv - 1 and are masked).
#include "attention_probs.h"

namespace {

struct MapParams {
    float* maps;
    int ldm, heads, Nq, Nkv, Nkp;
    const int* lens;                    // the per-image form, or NULL
    const unsigned char* key_seg;       // the per-query forms, or NULL (query_mask beside it)
    const unsigned* query_mask;
    const float* key_bias;              // the weighted form, or NULL
    float factor;                       // scale / heads
    int accumulate;
};

// this image's view of the forms: after it, a key takes part in query q's softmax iff seg(key) < 32 and bit seg(key) of mask(q) is set
struct MapKeys {
    const unsigned char* segb;
    const float* biasb;
    int nb;                             // keys at or behind nb take part in nothing
    __device__ __forceinline__ MapKeys(const MapParams& p, int b) {
        segb = p.key_seg ? p.key_seg + (size_t)b * p.Nkv : nullptr;
        biasb = p.key_bias ? p.key_bias + (size_t)b * p.Nkv : nullptr;
        nb = prob_len(p.lens, b, p.Nkv);
    }
    // segment of `key` (255: excluded for every query) and its bias (0 without weights)
    __device__ __forceinline__ void of(int key, unsigned& sg, float& kb) const {
        sg = 255u; kb = 0.f;
        if (key < nb) {
            sg = segb ? (unsigned)segb[key] : 0u;
            if (biasb) {
                kb = biasb[key];
                if (kb == -INFINITY) { sg = 255u; kb = 0.f; }
            }
        }
    }
};
__device__ __forceinline__ unsigned map_query_mask(const MapParams& p, int b, int q) {
    return p.query_mask ? p.query_mask[(size_t)b * p.Nq + q] : 1u;
}
__device__ __forceinline__ bool map_allowed(unsigned sg, unsigned qm) { return (sg < 32u) & ((qm >> (sg & 31u)) & 1u); }

__device__ __forceinline__ void map_store(const MapParams& p, int b, int q, int key, bool ok, float sum) {
    float* o = p.maps + ((size_t)b * p.Nq + q) * p.ldm + key;
    const float v = sum * p.factor;
    if (p.accumulate) {
        if (ok) *o += v;
    } else {
        *o = ok ? v : 0.f;
    }
}

// reductions over the 16 lanes of a DPP row
__device__ __forceinline__ float row16_max(float v) {
    v = fmaxf(v, dpp_mov<0xB1>(v));
    v = fmaxf(v, dpp_mov<0x4E>(v));
    v = fmaxf(v, dpp_mov<0x141>(v));
    return fmaxf(v, dpp_mov<0x140>(v));
}
__device__ __forceinline__ float row16_sum(float v) {
    v += dpp_mov<0xB1>(v);
    v += dpp_mov<0x4E>(v);
    v += dpp_mov<0x141>(v);
    return v + dpp_mov<0x140>(v);
}

template <bool EXP2>
__global__ __launch_bounds__(256) void attention_maps_mfma_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K, MapParams p) {
    extern __shared__ float2 map_stat[];                        // [heads][64]: (m, 1 / l) of the workgroup's queries
    const int b = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, col = lane & 15, g = lane >> 4;
    const int Nq = p.Nq, Nkv = p.Nkv, heads = p.heads;
    const MapKeys keys(p, b);
    const int q0 = blockIdx.x * 64 + wave * 16;
    const int qa = q0 + col < Nq ? q0 + col : Nq - 1;           // the Q row this lane loads (rows past the end: a copy, never stored)
    unsigned qm[4];                                             // the queries this lane holds results of: q0 + 4 g + r
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int q = q0 + 4 * g + r;
        qm[r] = map_query_mask(p, b, q < Nq ? q : Nq - 1);
    }
    // 8 dims per lane and MFMA: [8 g, 8 g + 8) and [32 + 8 g, 32 + 8 g + 8), the same for both operands
    auto q_frag = [&](int h, uint4& f0, uint4& f1) {
        const uint4* qp = reinterpret_cast<const uint4*>(Q + (((size_t)b * heads + h) * Nq + qa) * 64 + g * 8);
        f0 = qp[0]; f1 = qp[4];
    };
    auto scores = [&](int h, int key, const uint4& f0, const uint4& f1) -> f32x4_t {
        const int kr = key < Nkv ? key : Nkv - 1;               // no row at or behind Nkv is read
        const uint4* kp = reinterpret_cast<const uint4*>(K + (((size_t)b * heads + h) * p.Nkp + kr) * 64 + g * 8);
        const uint4 k0 = kp[0], k1 = kp[4];
        f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
        Mma<bf16_t>::run(acc, f0, k0);
        Mma<bf16_t>::run(acc, f1, k1);
        return acc;                                             // acc[r] = s[query 4 g + r][key]
    };

    for (int h = 0; h < heads; ++h) {
        uint4 f0, f1;
        q_frag(h, f0, f1);
        float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY}, l[4] = {0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < keys.nb; k0 += 16) {
            unsigned sg; float kb;
            keys.of(k0 + col, sg, kb);
            const f32x4_t s = scores(h, k0 + col, f0, f1);
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (map_allowed(sg, qm[r])) prob_online<EXP2>(m[r], l[r], s[r] + kb);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {                           // the 16 lanes of a row hold the 16 key residues of one query
            const float mm = row16_max(m[r]);
            const float ll = row16_sum(m[r] == -INFINITY ? 0.f : l[r] * prob_exp<EXP2>(m[r] - mm));
            if (col == 0) map_stat[h * 64 + wave * 16 + 4 * g + r] = make_float2(mm, ll > 0.f ? 1.f / ll : 0.f);
        }
    }
    __syncthreads();

    for (int c0 = 0; c0 < Nkv; c0 += 64) {
        float sum[4][4];
        unsigned sg[4]; float kb[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            keys.of(c0 + 16 * t + col, sg[t], kb[t]);
#pragma unroll
            for (int r = 0; r < 4; ++r) sum[t][r] = 0.f;
        }
        for (int h = 0; h < heads; ++h) {
            uint4 f0, f1;
            q_frag(h, f0, f1);
            float2 st[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) st[r] = map_stat[h * 64 + wave * 16 + 4 * g + r];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (c0 + 16 * t >= keys.nb) break;              // (workgroup-uniform) nothing behind takes part
                const f32x4_t s = scores(h, c0 + 16 * t + col, f0, f1);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float pr = prob_exp<EXP2>(s[r] + kb[t] - st[r].x) * st[r].y;
                    sum[t][r] += map_allowed(sg[t], qm[r]) ? pr : 0.f;
                }
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int key = c0 + 16 * t + col;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = q0 + 4 * g + r;
                if (key < Nkv && q < Nq) map_store(p, b, q, key, map_allowed(sg[t], qm[r]), sum[t][r]);
            }
        }
    }
}

// DPL = dims per lane = dh / 4
template <typename T, int DPL, bool EXP2>
__global__ __launch_bounds__(256) void attention_maps_valu_kernel(const T* __restrict__ Q, const T* __restrict__ K, MapParams p) {
    extern __shared__ float2 map_stat[];                        // [heads][64]: (m, 1 / l) of the workgroup's queries
    constexpr int DH = DPL * 4;
    const int b = blockIdx.y, ql = threadIdx.x >> 2, part = threadIdx.x & 3;
    const int Nq = p.Nq, Nkv = p.Nkv, heads = p.heads;
    const MapKeys keys(p, b);
    const int qi = blockIdx.x * 64 + ql;
    const int qr = qi < Nq ? qi : Nq - 1;                       // rows past the end compute a copy and do not store
    const unsigned qm = map_query_mask(p, b, qr);
    float q[DPL];
    auto q_load = [&](int h) {
        const T* qp = Q + (((size_t)b * heads + h) * Nq + qr) * DH + part * DPL;
#pragma unroll
        for (int i = 0; i < DPL; ++i) q[i] = to_f32<T>(qp[i]);
    };
    auto score = [&](int h, int j) -> float {                   // j < Nkv
        return quad_score<T, DPL>(K + (((size_t)b * heads + h) * p.Nkp + j) * DH + part * DPL, q);
    };

    for (int h = 0; h < heads; ++h) {
        q_load(h);
        float m = -INFINITY, l = 0.f;
        for (int j = 0; j < keys.nb; ++j) {
            const float s = score(h, j);
            unsigned sg; float kb;
            keys.of(j, sg, kb);                                 // (wave-uniform address; the four lanes of a query agree)
            if (map_allowed(sg, qm)) prob_online<EXP2>(m, l, s + kb);
        }
        if (part == 0) map_stat[h * 64 + ql] = make_float2(m, l > 0.f ? 1.f / l : 0.f);
    }
    __syncthreads();

    for (int c0 = 0; c0 < Nkv; c0 += 16) {
        float sum[4] = {0.f, 0.f, 0.f, 0.f};                    // keys c0 + 4 part + i
        for (int h = 0; h < heads; ++h) {
            q_load(h);
            const float2 st = map_stat[h * 64 + ql];
#pragma unroll
            for (int jj = 0; jj < 16; ++jj) {
                const int j = c0 + jj;
                if (j >= keys.nb) break;                        // (workgroup-uniform) nothing behind takes part
                const float s = score(h, j);
                unsigned sg; float kb;
                keys.of(j, sg, kb);
                const float pr = prob_exp<EXP2>(s + kb - st.x) * st.y;
                sum[jj & 3] += ((jj >> 2) == part && map_allowed(sg, qm)) ? pr : 0.f;
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int key = c0 + 4 * part + i;
            if (key < Nkv && qi < Nq) {
                unsigned sg; float kb;
                keys.of(key, sg, kb);
                map_store(p, b, qi, key, map_allowed(sg, qm), sum[i]);
            }
        }
    }
}

template <typename T>
int maps_valu(int dh, const void* Q, const void* K, const MapParams& p, int B, int use_exp2, hipStream_t s) {
    return pm_dh_dispatch("attention_maps", dh, [&](auto dpl) {
        constexpr int DPL = decltype(dpl)::value;
        auto k = use_exp2 ? attention_maps_valu_kernel<T, DPL, true> : attention_maps_valu_kernel<T, DPL, false>;
        hipLaunchKernelGGL(k, dim3((p.Nq + 63) / 64, B), dim3(256), (size_t)p.heads * 64 * sizeof(float2), s, (const T*)Q, (const T*)K, p);
    });
}

}  // namespace

extern "C" int pmhip_attention_maps(int dtype, const void* Q, const void* K, float* maps, int ldm, int B, int heads, int dim_head, int Nq,
                                    int Nkv, int Nkv_pad, int use_exp2, const int32_t* kv_lens, const uint8_t* key_seg,
                                    const uint32_t* query_mask, const float* key_bias, float scale, int accumulate, pmhip_stream stream) {
    PM_TRY(pm_probs_check("attention_maps", dtype, dim_head, heads, {{"Nkv", Nkv, Nkv_pad}}));    // (heads: the row statistics live in LDS)
    PM_REQUIRE(Q && K && maps, "attention_maps: null pointer");
    PM_REQUIRE(B > 0 && heads > 0 && Nq > 0 && Nkv > 0, "attention_maps: empty problem");
    PM_REQUIRE(ldm >= Nkv, "attention_maps: ldm=%d is smaller than Nkv=%d (rows of maps would overlap)", ldm, Nkv);
    PM_REQUIRE(B <= 65535, "attention_maps: B=%d exceeds the grid's y range", B);
    PmAttnArgs a{};                                             // the optional arrays only: the rule of every attention entry
    a.lens = kv_lens; a.key_seg = key_seg; a.query_mask = query_mask; a.key_bias = key_bias;
    PM_TRY(pm_attn_check("attention_maps", a));
    PM_REQUIRE(std::isfinite(scale), "attention_maps: scale must be finite");
    hipStream_t s = (hipStream_t)stream;
    MapParams p{};
    p.maps = maps; p.ldm = ldm; p.heads = heads; p.Nq = Nq; p.Nkv = Nkv; p.Nkp = Nkv_pad;
    p.lens = kv_lens; p.key_seg = key_seg; p.query_mask = query_mask; p.key_bias = key_bias;
    p.factor = scale * (1.0f / (float)heads); p.accumulate = accumulate != 0;
    PmTimer tm(FAM_ATTENTION, s);
    if (dtype == PMHIP_BF16 && dim_head == 64) {
        PM_REQUIRE(pm_aligned(16, {Q, K}), "attention_maps: Q and K must be 16-byte aligned");
        auto k = use_exp2 ? attention_maps_mfma_kernel<true> : attention_maps_mfma_kernel<false>;
        hipLaunchKernelGGL(k, dim3((Nq + 63) / 64, B), dim3(256), (size_t)heads * 64 * sizeof(float2), s, (const bf16_t*)Q, (const bf16_t*)K, p);
    } else if (dtype == PMHIP_F32) {
        PM_TRY(maps_valu<float>(dim_head, Q, K, p, B, use_exp2, s));
    } else {
        PM_TRY(maps_valu<bf16_t>(dim_head, Q, K, p, B, use_exp2, s));
    }
    PM_HIP(hipGetLastError());
    return PMHIP_OK;
}
