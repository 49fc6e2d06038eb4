// Per-row model likelihood of a GIVEN token (pmhip_token_logprob): for every scored row r with target t, over
// x = a_r, or the guided row x_i = b_i + scale (a_i - b_i) formed at load,
//     lp  = log softmax(x)_t                                   <= 0
//     ent = -sum_i p_i log p_i = log s + sum_i p_i (m - x_i)    >= 0
//     rk  = #{ i : x_i > x_t, or x_i == x_t and i < t }         the target's place in the samplers' order (value down, column up)
// An HBM-bound row kernel of the family of masked_ce (loss.hip), sample_rows_forced (sample.hip) and logit_divergence
// (divergence.hip): every logits element is requested from memory ONCE (the target's own logit a second time, one broadcast load)
// and both passes -- the maximum, then the sum, the entropy term and the rank -- run from registers.
//
// RESIDENCY.  A row belongs to WAVES waves; lane l of wave w holds the float4 groups g = 0 .. G - 1 at columns
// ((g * WAVES + w) * 64 + l) * 4 .. + 3.  The classes of divergence.hip, by V:
//     V <= 256    G = 1, one wave per row,    four rows per workgroup        V <= 8192    G = 8, four waves per row,  one row per workgroup
//     V <= 1024   G = 4, one wave per row,    four rows per workgroup        V <= 16384   G = 8, eight waves per row, one row per workgroup
// so no lane holds more than 32 registers of logits (half of what the divergence kernel's pair takes).  The compiler reports 20-44
// registers for the two narrow classes (eight waves a SIMD) and 74-78 for the two wide ones, whose eight loads in flight and second
// pass take the rest: 80 allocated, six waves a SIMD, i.e. six rows of 8192 resident per CU with 128 bytes a lane in flight.
// With b given the combination happens at load: the second operand's float4 lives until its fused multiply-add and ONE row stays
// resident.
// The waves of a row exchange four words each through LDS: the maximum, then (one barrier) the sum, the entropy term and the count.
// Where a workgroup meets a barrier it serves ONE row, so the early return of an unscored row is uniform over every thread that
// would meet it; the classes with four rows per workgroup have no barrier at all (one wave reduces by DPP alone).
//
// AN UNSCORED ROW (ids given and ids[r] != mask_id, or target[r] outside [0, V)) returns in front of its loads: the range test sits
// in front of any use of the target as an index, the row's logits are never requested, and a NaN there reaches nothing.
//
// EVALUATION ORDER (explicitly rounded operations, no contraction except the ONE fused multiply-add of the combination, no
// re-association):
//     x_i = a_i                                     or   x_i = fma(scale, rn(a_i - b_i), b_i): pmhip_guidance_combine's expression
//     m   = max_i x_i                               d_i = rn(x_i - m) <= 0                       e_i = exp2(rn(d_i log2 e))
//     s   = sum_i e_i                               T   = sum_i (e_i == 0 ? 0 : rn(e_i (-d_i)))  c   = sum_i [x_i > x_t or (x_i == x_t and i < t)]
// the sums per lane over its groups in order, each group as (x + y) + (z + w), then the wave butterfly, then the waves in order
// (c is counted in integers per lane and summed as floats: at most 16384, exact).  Then
//     L   = rn(log2(s) ln 2)                        lp  = rn(rn(x_t - m) - L)                    ent = rn(L + rn(T / s))
// x_t is loaded by every lane from the target's own address and combined by the expression above: the bits of the resident copy.
// What follows, and is part of the contract:
//   * the maximum's own term is exp2(0) = 1 exactly and every other term is >= 0, so s >= 1 (a sum of non-negative numbers is
//     monotone under rounding), log2(s) >= 0, L >= 0; rn(x_t - m) <= 0 because m >= x_t exactly: lp <= 0 exactly;
//   * every e_i (-d_i) is >= 0, so T >= 0 and ent >= 0; a row with one finite column has s = 1, L = 0, T = 1 * 0 = 0: ent = 0 exactly;
//   * a -inf column has e_i = 0 and -d_i = inf: the select keeps its 0 * inf out of T; a target on it gives lp = -inf;
//   * the rank compares stored (or combined) values as they are: it is exact.
// Columns [V, G * WAVES * 256) are initialised to -inf: they take part in no maximum, sum or count (their index is >= V > t).
// A NaN in a scored row reaches s through its e_i: lp and ent are NaN; the count of such a row is unspecified.
//
// One writer per row (lane 0 of the row's first wave), no atomics: two launches give the same bits.
#include <cmath>

#include "common.h"

// The order above is the contract (divergence.hip has the reasons): the arithmetic of this file is written with the operators below,
// under a pragma that forbids contraction.  The combination's fmaf is a call, not a contraction: it stays one fused operation.
#pragma clang fp contract(off)

namespace {

constexpr float PM_LN2 = 0.6931471805599453f;

__device__ __forceinline__ float add_rn(float x, float y) { return x + y; }
__device__ __forceinline__ float sub_rn(float x, float y) { return x - y; }
__device__ __forceinline__ float mul_rn(float x, float y) { return x * y; }
__device__ __forceinline__ float combine(float c, float u, float scale) { return fmaf(scale, sub_rn(c, u), u); }      // guidance_body's
__device__ __forceinline__ float4 combine4(const float4& c, const float4& u, float scale) {
    return make_float4(combine(c.x, u.x, scale), combine(c.y, u.y, scale), combine(c.z, u.z, scale), combine(c.w, u.w, scale));
}
__device__ __forceinline__ float max4(const float4& v) { return fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)); }

// one column: e -> its term of s, t -> its term of T, returns whether it is ordered in front of the target
__device__ __forceinline__ bool column(float x, float m, float xt, int col, int64_t t, float& e, float& term) {
    const float d = sub_rn(x, m);
    e = __builtin_amdgcn_exp2f(mul_rn(d, PM_LOG2E));
    term = e == 0.f ? 0.f : mul_rn(e, -d);
    return x > xt || (x == xt && (int64_t)col < t);
}

// one word per wave of a row, combined in wave order (no barrier inside: the caller has placed one behind the stores)
template <int WAVES, bool MAX>
__device__ __forceinline__ float in_wave_order(const float* slot) {
    float r = slot[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) r = MAX ? fmaxf(r, slot[w]) : add_rn(r, slot[w]);
    return r;
}

template <int G, int WAVES, int ROWS, bool GUIDED>
__global__ __launch_bounds__(64 * WAVES * ROWS) void token_logprob_kernel(const float* __restrict__ a, const float* __restrict__ b, float scale,
                                                                         int ldl, const int64_t* __restrict__ ids, int64_t mask_id,
                                                                         const int64_t* __restrict__ target, float* __restrict__ logp,
                                                                         float* __restrict__ entropy, int32_t* __restrict__ rank,
                                                                         int32_t* __restrict__ count, int accumulate, int M, int V) {
    static_assert(WAVES == 1 || ROWS == 1, "a workgroup that meets a barrier serves one row");
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wave = WAVES == 1 ? 0 : wid;
    const int row = WAVES == 1 ? blockIdx.x * ROWS + wid : blockIdx.x;
    if (row >= M) return;                                      // (WAVES > 1: the grid has M workgroups, never taken)
    const int64_t t = target[row];
    const bool scored = (ids == nullptr || ids[row] == mask_id) && t >= 0 && t < (int64_t)V;
    if (!scored) {                                             // uniform over the row's waves: in front of every load and barrier
        if (!accumulate && wave == 0 && lane == 0) {
            logp[row] = 0.f;
            if (entropy != nullptr) entropy[row] = 0.f;
            if (rank != nullptr) rank[row] = 0;
            if (count != nullptr) count[row] = 0;
        }
        return;
    }
    const float* ar = a + (size_t)row * ldl;
    const float* br = GUIDED ? b + (size_t)row * ldl : nullptr;
    float4 x[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int col = ((g * WAVES + wave) * 64 + lane) * 4;
        x[g] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        if (col < V) {
            x[g] = *reinterpret_cast<const float4*>(ar + col);
            if (GUIDED) x[g] = combine4(x[g], *reinterpret_cast<const float4*>(br + col), scale);
        }
    }
    float xt = ar[t];                                          // 0 <= t < V: tested above.  One address for the whole row: a broadcast
    if (GUIDED) xt = combine(xt, br[t], scale);
    __shared__ float lds[WAVES == 1 ? 1 : 4 * WAVES];          // two exchanges, a set of words each: nothing is reused
    float m = -INFINITY;
#pragma unroll
    for (int g = 0; g < G; ++g) m = fmaxf(m, max4(x[g]));
    m = wave_max(m);
    if (WAVES > 1) {
        if (lane == 0) lds[wave] = m;
        __syncthreads();
        m = in_wave_order<WAVES, true>(lds);
    }
    float s = 0.f, T = 0.f;
    int c = 0;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int col = ((g * WAVES + wave) * 64 + lane) * 4;
        float e0, e1, e2, e3, t0, t1, t2, t3;
        c += column(x[g].x, m, xt, col, t, e0, t0);
        c += column(x[g].y, m, xt, col + 1, t, e1, t1);
        c += column(x[g].z, m, xt, col + 2, t, e2, t2);
        c += column(x[g].w, m, xt, col + 3, t, e3, t3);
        s = add_rn(s, add_rn(add_rn(e0, e1), add_rn(e2, e3)));
        T = add_rn(T, add_rn(add_rn(t0, t1), add_rn(t2, t3)));
    }
    s = wave_sum(s);
    T = wave_sum(T);
    float cf = wave_sum((float)c);                             // integers up to 16384: every partial sum is exact
    if (WAVES > 1) {
        if (lane == 0) {
            lds[WAVES + wave] = s;
            lds[2 * WAVES + wave] = T;
            lds[3 * WAVES + wave] = cf;
        }
        __syncthreads();
        s = in_wave_order<WAVES, false>(lds + WAVES);
        T = in_wave_order<WAVES, false>(lds + 2 * WAVES);
        cf = in_wave_order<WAVES, false>(lds + 3 * WAVES);
    }
    if (wave == 0 && lane == 0) {
        const float L = mul_rn(__builtin_amdgcn_logf(s), PM_LN2);      // v_log_f32 is log2; s >= 1: no subnormal operand
        const float lp = sub_rn(sub_rn(xt, m), L);
        const float ent = add_rn(L, T / s);
        const int32_t rk = (int32_t)cf;
        if (accumulate) {
            logp[row] = add_rn(logp[row], lp);
            if (entropy != nullptr) entropy[row] = add_rn(entropy[row], ent);
            if (rank != nullptr) rank[row] += rk;
            if (count != nullptr) count[row] += 1;
        } else {
            logp[row] = lp;
            if (entropy != nullptr) entropy[row] = ent;
            if (rank != nullptr) rank[row] = rk;
            if (count != nullptr) count[row] = 1;
        }
    }
}

template <int G, int WAVES, int ROWS>
void launch(const float* a, const float* b, float scale, int ldl, const int64_t* ids, int64_t mask_id, const int64_t* target, float* logp,
            float* entropy, int32_t* rank, int32_t* count, int accumulate, int M, int V, hipStream_t s) {
    const dim3 grid(ceil_div(M, ROWS)), block(64 * WAVES * ROWS);
    if (b != nullptr)
        hipLaunchKernelGGL((token_logprob_kernel<G, WAVES, ROWS, true>), grid, block, 0, s, a, b, scale, ldl, ids, mask_id, target, logp, entropy,
                           rank, count, accumulate, M, V);
    else
        hipLaunchKernelGGL((token_logprob_kernel<G, WAVES, ROWS, false>), grid, block, 0, s, a, b, scale, ldl, ids, mask_id, target, logp, entropy,
                           rank, count, accumulate, M, V);
}

}  // namespace

extern "C" int pmhip_token_logprob(const float* a, const float* b, float scale, int ldl, const int64_t* ids, int64_t mask_id,
                                   const int64_t* target, float* logp, float* entropy, int32_t* rank, int32_t* count, int accumulate, int M,
                                   int V, pmhip_stream stream) {
    PM_REQUIRE(a, "token_logprob: a is NULL");
    PM_REQUIRE(target, "token_logprob: target is NULL");
    PM_REQUIRE(logp, "token_logprob: logp is NULL");
    PM_REQUIRE(pm_aligned(16, {a, b}), "token_logprob: a and b must be 16-byte aligned (float4 loads)");
    PM_REQUIRE(M > 0, "token_logprob: M=%d must be positive", M);
    PM_REQUIRE(V > 0 && V % 4 == 0 && V <= 16384, "token_logprob: V=%d must be a multiple of 4 in (0, 16384]", V);
    PM_REQUIRE(ldl % 4 == 0 && ldl >= V, "token_logprob: ldl=%d must be a multiple of 4 and at least V=%d", ldl, V);
    PM_REQUIRE(b == nullptr || std::isfinite(scale), "token_logprob: scale=%f must be finite (b is given)", (double)scale);
    hipStream_t s = (hipStream_t)stream;
    PmTimer tm(FAM_SAMPLE, s);
#define PM_LOGPROB(G, WAVES, ROWS) launch<G, WAVES, ROWS>(a, b, scale, ldl, ids, mask_id, target, logp, entropy, rank, count, accumulate, M, V, s)
    if (V <= 256) PM_LOGPROB(1, 1, 4);
    else if (V <= 1024) PM_LOGPROB(4, 1, 4);
    else if (V <= 8192) PM_LOGPROB(8, 4, 1);
    else PM_LOGPROB(8, 8, 1);
#undef PM_LOGPROB
    PM_HIP(hipGetLastError());
    return PMHIP_OK;
}
