// Local blend of a prompt-to-prompt pair: where the pair looks at a phrase, the region that follows from it, and the
// token blend under that region.
//
// pmhip_attention_phrase_score.  Per pair b and query q, over the heads h, with ps, pt, has and P those of the pair control
// (attention_probs.h; P = pt when the control arrays are NULL):
//
//   score_s[b, q] (+)= scale / heads * sum_h sum_{k < ns} w_s[b, k] * ps_h[q, k]
//   score_t[b, q] (+)= scale / heads * sum_h sum_{j < nt} w_t[b, j] * P_h[q, j]
//
// pmhip_attention_maps would materialise [B, Nq, L] floats for what is [B, Nq] here, and knows nothing of the controlled P;
// pmhip_attention_control owns one head per workgroup.  This file recomputes both softmaxes in the two-pass structure of
// attention_maps.hip -- a workgroup owns one pair and 64 queries and walks both contexts twice PER HEAD:
//   pass 1 : the maximum m and the sum l of every query row of both softmaxes, (m, 1 / l) kept in registers
//   pass 2 : walk the source keys (w_s . ps) and the target keys (w_t . P; the Ks rows gathered through row_map by the control
//            kernel's own PM_KQ_GATHER), adding into two registers that live across the loop over the heads h = 0 .. heads-1
// so registers do not depend on the contexts, there is no LDS, the sum over heads and keys has a fixed order, every element of the
// two outputs is written by exactly one thread once, and there are no atomics.  P stays f32 in both dtypes.
//   attention_phrase_mfma_kernel  bf16, dim_head 64.  S^T = K Q^T by v_mfma_f32_16x16x32_bf16, operands straight from global memory in
//                                 fragment layout: a lane holds the scores of ONE query (lane & 15) and of keys 4 g + r of a 16-key tile;
//                                 the four lanes of a query are joined once, behind the loop over the heads
//   attention_phrase_valu_kernel  everything else (fp32, dim_head != 64): 4 lanes share a query, each owning dh / 4 dims
// A tile (MFMA) or key (vector ALU) whose weights are all 0 is skipped in pass 2: p is finite, so 0 * p adds nothing, and the skip
// changes no bit.  Every key still takes part in pass 1, the softmax.
// Select, never arithmetic: a key at or behind the pair's length is not read and its weight is not read; a map entry at or behind ns
// is `none`; where `has` is false the gathered row is row 0 of the pair's own Ks in the MFMA kernel (any lane must feed the matrix
// core something) and its score is dropped by a select.
//
// pmhip_phrase_region: the rule of Pipeline.phrase_mask on both halves, joined, then dilated; one workgroup per pair, the grid in LDS.
// pmhip_blend_tokens: outside the region the edited half's (pred, merged, score) become the source half's.
#include "attention_probs.h"

namespace {

struct PhrParams {
    float* score_s;                     // [B, Nq]
    float* score_t;                     // [B, Nq]
    int heads, Nq, Ls, Lsp, Lt, Ltp;
    PairControl ctl;                    // or all three NULL: no control
    const int* lens_s;                  // [B] or NULL
    const int* lens_t;                  // [B] or NULL
    const float* w_s;                   // [B, Ls]
    const float* w_t;                   // [B, Lt]
    float factor;                       // scale / heads
    int accumulate;
};

__device__ __forceinline__ void phr_store(const PhrParams& p, int b, int q, float ss, float st) {
    const size_t at = (size_t)b * p.Nq + q;
    const float vs = ss * p.factor, vt = st * p.factor;
    if (p.accumulate) {
        p.score_s[at] += vs; p.score_t[at] += vt;
    } else {
        p.score_s[at] = vs; p.score_t[at] = vt;
    }
}

template <bool EXP2>
__global__ __launch_bounds__(256) void attention_phrase_mfma_kernel(const bf16_t* __restrict__ Qs, const bf16_t* __restrict__ Ks,
                                                                    const bf16_t* __restrict__ Qt, const bf16_t* __restrict__ Kt, PhrParams p) {
    const int b = blockIdx.y;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, col = lane & 15, g = lane >> 4;
    const int Nq = p.Nq, heads = p.heads;
    const int ns = prob_len(p.lens_s, b, p.Ls), nt = prob_len(p.lens_t, b, p.Lt);
    const bool ctl = p.ctl.row_map != nullptr;                      // (uniform over the launch)
    const int qi = blockIdx.x * 64 + wave * 16 + col;           // this lane's query: every score it holds
    const int qa = qi < Nq ? qi : Nq - 1;                       // (rows past the end: a copy, never stored)
    const float* wsb = p.w_s + (size_t)b * p.Ls;
    const float* wtb = p.w_t + (size_t)b * p.Lt;
    // the weights of this lane's four keys of the tile at k0 (0 by a select at or behind n) and whether any lane of the wave has one
    auto tile_weights = [&](const float* wb, int k0, int n, float (&w)[4]) -> bool {
        bool any = false;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = k0 + 4 * g + r;
            w[r] = k < n ? wb[k] : 0.f;
            any |= w[r] != 0.f;
        }
        return __builtin_amdgcn_ballot_w64(any) != 0;           // (wave-uniform)
    };

    float acc_s = 0.f, acc_t = 0.f;                             // this lane's part of the two sums, over the heads in order
    for (int h = 0; h < heads; ++h) {
        const size_t bh = (size_t)b * heads + h;
        // 8 dims per lane and MFMA: [8 g, 8 g + 8) and [32 + 8 g, 32 + 8 g + 8), the same for both operands
        uint4 qs0, qs1, qt0, qt1;
        {
            const uint4* a = reinterpret_cast<const uint4*>(Qs + (bh * Nq + qa) * 64 + g * 8);
            const uint4* c = reinterpret_cast<const uint4*>(Qt + (bh * Nq + qa) * 64 + g * 8);
            qs0 = a[0]; qs1 = a[4]; qt0 = c[0]; qt1 = c[4];
        }
        const bf16_t* ksb = Ks + bh * p.Lsp * 64 + g * 8;
        const bf16_t* ktb = Kt + bh * p.Ltp * 64 + g * 8;
        float ms, is, mt, it;
        kq_stats<EXP2>(ksb, ns, qs0, qs1, col, g, ms, is);
        kq_stats<EXP2>(ktb, nt, qt0, qt1, col, g, mt, it);

        for (int k0 = 0; k0 < ns; k0 += 16) {                   // w_s . ps
            float w[4];
            if (!tile_weights(wsb, k0, ns, w)) continue;
            const f32x4_t s = kq_scores(ksb, k0 + col < ns ? k0 + col : ns - 1, qs0, qs1);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float pr = prob_exp<EXP2>(s[r] - ms) * is;
                acc_s += (k0 + 4 * g + r < ns) ? w[r] * pr : 0.f;
            }
        }
        for (int j0 = 0; j0 < nt; j0 += 16) {                   // w_t . P
            float w[4];
            if (!tile_weights(wtb, j0, nt, w)) continue;
            const int kj = j0 + col;
            const f32x4_t st = kq_scores(ktb, kj < nt ? kj : nt - 1, qt0, qt1);
            f32x4_t ss = {0.f, 0.f, 0.f, 0.f};
            if (ctl) PM_KQ_GATHER(ss, p.ctl, p.Lt, b, kj, nt, ns, ksb, qs0, qs1);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = j0 + 4 * g + r;
                if (j < nt) {
                    float pj = prob_exp<EXP2>(st[r] - mt) * it;
                    if (ctl) {
                        const PairKey k = pair_key(p.ctl, p.Lt, b, j, ns);
                        const float ps = k.has ? prob_exp<EXP2>(ss[r] - ms) * is : 0.f;
                        pj = pair_mix(k, pj, ps);
                    }
                    acc_t += w[r] * pj;
                }
            }
        }
    }
    acc_s = group4_sum(acc_s);
    acc_t = group4_sum(acc_t);
    if (g == 0 && qi < Nq) phr_store(p, b, qi, acc_s, acc_t);
}

// DPL = dims per lane = dh / 4
template <typename T, int DPL, bool EXP2>
__global__ __launch_bounds__(256) void attention_phrase_valu_kernel(const T* __restrict__ Qs, const T* __restrict__ Ks,
                                                                    const T* __restrict__ Qt, const T* __restrict__ Kt, PhrParams p) {
    constexpr int DH = DPL * 4;
    const int b = blockIdx.y;
    const int Nq = p.Nq, heads = p.heads;
    const int ns = prob_len(p.lens_s, b, p.Ls), nt = prob_len(p.lens_t, b, p.Lt);
    const bool ctl = p.ctl.row_map != nullptr;
    const int qi = blockIdx.x * 64 + (threadIdx.x >> 2), part = threadIdx.x & 3;
    const int qr = qi < Nq ? qi : Nq - 1;                       // rows past the end compute a copy and do not store
    const float* wsb = p.w_s + (size_t)b * p.Ls;
    const float* wtb = p.w_t + (size_t)b * p.Lt;
    float acc_s = 0.f, acc_t = 0.f;                             // (the four lanes of a query hold the same sums)
    for (int h = 0; h < heads; ++h) {
        const size_t bh = (size_t)b * heads + h;
        float qs[DPL], qt[DPL];
        {
            const T* a = Qs + (bh * Nq + qr) * DH + part * DPL;
            const T* c = Qt + (bh * Nq + qr) * DH + part * DPL;
#pragma unroll
            for (int i = 0; i < DPL; ++i) { qs[i] = to_f32<T>(a[i]); qt[i] = to_f32<T>(c[i]); }
        }
        const T* ksb = Ks + bh * p.Lsp * DH + part * DPL;
        const T* ktb = Kt + bh * p.Ltp * DH + part * DPL;
        float ms = -INFINITY, ls = 0.f, mt = -INFINITY, lt = 0.f;                   // pass 1
        for (int k = 0; k < ns; ++k) prob_online<EXP2>(ms, ls, quad_score<T, DPL>(ksb, k, qs));
        for (int j = 0; j < nt; ++j) prob_online<EXP2>(mt, lt, quad_score<T, DPL>(ktb, j, qt));
        const float is = 1.f / ls, it = 1.f / lt;

        for (int k = 0; k < ns; ++k) {                          // w_s . ps
            const float w = wsb[k];                             // (workgroup-uniform: the quads stay whole)
            if (w == 0.f) continue;
            acc_s += w * (prob_exp<EXP2>(quad_score<T, DPL>(ksb, k, qs) - ms) * is);
        }
        for (int j = 0; j < nt; ++j) {                          // w_t . P
            const float w = wtb[j];
            if (w == 0.f) continue;
            float pj = prob_exp<EXP2>(quad_score<T, DPL>(ktb, j, qt) - mt) * it;
            if (ctl) {
                const PairKey k = pair_key(p.ctl, p.Lt, b, j, ns);
                float ps = 0.f;
                if (k.has) ps = prob_exp<EXP2>(quad_score<T, DPL>(ksb, k.row, qs) - ms) * is;
                pj = pair_mix(k, pj, ps);
            }
            acc_t += w * pj;
        }
    }
    if (part == 0 && qi < Nq) phr_store(p, b, qi, acc_s, acc_t);
}

template <typename T>
int phrase_valu(int dh, const void* Qs, const void* Ks, const void* Qt, const void* Kt, const PhrParams& p, int B, int use_exp2,
                hipStream_t s) {
    return pm_dh_dispatch("attention_phrase_score", dh, [&](auto dpl) {
        constexpr int DPL = decltype(dpl)::value;
        auto k = use_exp2 ? attention_phrase_valu_kernel<T, DPL, true> : attention_phrase_valu_kernel<T, DPL, false>;
        hipLaunchKernelGGL(k, dim3((p.Nq + 63) / 64, B), dim3(256), 0, s, (const T*)Qs, (const T*)Ks, (const T*)Qt, (const T*)Kt, p);
    });
}

// ------------------------------------------------------------------------------------------------------------- region and blend

constexpr int REGION_MAX_G = 64;

// one workgroup per pair: the two maxima, the two thresholds, the union, `grow` dilations between two grids in LDS
__global__ __launch_bounds__(256) void phrase_region_kernel(const float* __restrict__ score_s, const float* __restrict__ score_t,
                                                            unsigned char* __restrict__ mask_out, int g, float threshold, int grow) {
    __shared__ unsigned char grid[2][REGION_MAX_G * REGION_MAX_G];
    __shared__ float red[2][4];
    const int b = blockIdx.x, N = g * g, tid = threadIdx.x;
    const float* ss = score_s + (size_t)b * N;
    const float* st = score_t + (size_t)b * N;
    float ms = -INFINITY, mt = -INFINITY;
    for (int t = tid; t < N; t += 256) { ms = fmaxf(ms, ss[t]); mt = fmaxf(mt, st[t]); }
    ms = wave_max(ms); mt = wave_max(mt);
    if ((tid & 63) == 0) { red[0][tid >> 6] = ms; red[1][tid >> 6] = mt; }
    __syncthreads();
    ms = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
    mt = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
    const float cut_s = __fmul_rn(threshold, ms), cut_t = __fmul_rn(threshold, mt);                  // one f32 product each
    for (int t = tid; t < N; t += 256) grid[0][t] = (ss[t] >= cut_s) | (st[t] >= cut_t);
    __syncthreads();
    int cur = 0;
    const int rounds = grow < g ? grow : g;                     // g dilations already cover the grid from any non-empty mask
    for (int it = 0; it < rounds; ++it) {
        for (int t = tid; t < N; t += 256) {
            const int y = t / g, x = t - y * g;
            unsigned char v = 0;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int yy = y + dy, xx = x + dx;
                    if (yy >= 0 && yy < g && xx >= 0 && xx < g) v |= grid[cur][yy * g + xx];
                }
            grid[cur ^ 1][t] = v;
        }
        __syncthreads();
        cur ^= 1;
    }
    for (int t = tid; t < N; t += 256) mask_out[(size_t)b * N + t] = grid[cur][t];
}

__global__ __launch_bounds__(256) void blend_tokens_kernel(const unsigned char* __restrict__ mask, const long long* __restrict__ pred_s,
                                                           const long long* __restrict__ merged_s, const float* __restrict__ score_s,
                                                           long long* __restrict__ pred_t, long long* __restrict__ merged_t,
                                                           float* __restrict__ score_t, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n && mask[i] == 0) {
        pred_t[i] = pred_s[i]; merged_t[i] = merged_s[i]; score_t[i] = score_s[i];
    }
}

}  // namespace

extern "C" int pmhip_attention_phrase_score(int dtype, const void* Qs, const void* Ks, const void* Qt, const void* Kt, int B, int heads,
                                            int dim_head, int Nq, int Ls, int Ls_pad, int Lt, int Lt_pad, int use_exp2,
                                            const int32_t* row_map, const float* blend, const float* gain, const int32_t* lens_s,
                                            const int32_t* lens_t, const float* w_s, const float* w_t, float* score_s, float* score_t,
                                            float scale, int accumulate, pmhip_stream stream) {
    PM_TRY(pm_probs_check("attention_phrase_score", dtype, dim_head, heads, {{"Ls", Ls, Ls_pad}, {"Lt", Lt, Lt_pad}}));
    PM_REQUIRE(Qs && Ks && Qt && Kt, "attention_phrase_score: null pointer");
    PM_REQUIRE(w_s && w_t && score_s && score_t, "attention_phrase_score: w_s / w_t / score_s / score_t is NULL");
    PM_REQUIRE((row_map != nullptr) == (blend != nullptr) && (blend != nullptr) == (gain != nullptr),
               "attention_phrase_score: row_map, blend and gain come together (all NULL: no control)");
    PM_REQUIRE(B > 0 && heads > 0 && Nq > 0 && Ls > 0 && Lt > 0, "attention_phrase_score: empty problem");
    PM_REQUIRE((long long)B * heads <= 65535, "attention_phrase_score: B*heads=%lld exceeds the range of pmhip_attention_control", (long long)B * heads);
    PM_REQUIRE(std::isfinite(scale), "attention_phrase_score: scale must be finite");
    hipStream_t s = (hipStream_t)stream;
    PhrParams p{};
    p.score_s = score_s; p.score_t = score_t; p.heads = heads; p.Nq = Nq; p.Ls = Ls; p.Lsp = Ls_pad; p.Lt = Lt; p.Ltp = Lt_pad;
    p.ctl = {row_map, blend, gain}; p.lens_s = lens_s; p.lens_t = lens_t; p.w_s = w_s; p.w_t = w_t;
    p.factor = scale * (1.0f / (float)heads); p.accumulate = accumulate != 0;
    const bool mfma = dtype == PMHIP_BF16 && dim_head == 64;
    if (mfma)
        PM_REQUIRE(pm_aligned(16, {Qs, Ks, Qt, Kt}), "attention_phrase_score: Q and K must be 16-byte aligned");
    PmTimer tm(FAM_ATTENTION, s);
    if (mfma) {
        auto k = use_exp2 ? attention_phrase_mfma_kernel<true> : attention_phrase_mfma_kernel<false>;
        hipLaunchKernelGGL(k, dim3((Nq + 63) / 64, B), dim3(256), 0, s, (const bf16_t*)Qs, (const bf16_t*)Ks, (const bf16_t*)Qt,
                           (const bf16_t*)Kt, p);
    } else if (dtype == PMHIP_F32) {
        PM_TRY(phrase_valu<float>(dim_head, Qs, Ks, Qt, Kt, p, B, use_exp2, s));
    } else {
        PM_TRY(phrase_valu<bf16_t>(dim_head, Qs, Ks, Qt, Kt, p, B, use_exp2, s));
    }
    PM_HIP(hipGetLastError());
    return PMHIP_OK;
}

extern "C" int pmhip_phrase_region(const float* score_s, const float* score_t, uint8_t* mask_out, int B, int g, float threshold, int grow,
                                   pmhip_stream stream) {
    PM_REQUIRE(score_s && score_t && mask_out, "phrase_region: null pointer");
    PM_REQUIRE(B > 0, "phrase_region: empty problem");
    PM_REQUIRE(g >= 1 && g <= REGION_MAX_G, "phrase_region: g=%d must be in [1, %d] (the grid lives in LDS)", g, REGION_MAX_G);
    PM_REQUIRE(threshold > 0.f && threshold <= 1.f, "phrase_region: threshold=%g must be in (0, 1]", (double)threshold);
    PM_REQUIRE(grow >= 0, "phrase_region: grow=%d must be >= 0", grow);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(phrase_region_kernel, dim3(B), dim3(256), 0, s, score_s, score_t, mask_out, g, threshold, grow);
    PM_HIP(hipGetLastError());
    return PMHIP_OK;
}

extern "C" int pmhip_blend_tokens(const uint8_t* mask, const int64_t* pred_s, const int64_t* merged_s, const float* score_s, int64_t* pred_t,
                                  int64_t* merged_t, float* score_t, int B, int N, pmhip_stream stream) {
    PM_REQUIRE(mask && pred_s && merged_s && score_s && pred_t && merged_t && score_t, "blend_tokens: null pointer");
    PM_REQUIRE(B > 0 && N > 0, "blend_tokens: empty problem");
    const long long n = (long long)B * N;
    PM_REQUIRE(n <= 0x7fffffffLL * 256, "blend_tokens: B*N=%lld exceeds the grid", n);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(blend_tokens_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, mask, (const long long*)pred_s,
                       (const long long*)merged_s, score_s, (long long*)pred_t, (long long*)merged_t, score_t, n);
    PM_HIP(hipGetLastError());
    return PMHIP_OK;
}
