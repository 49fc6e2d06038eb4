// Per-row divergence between two logits tensors (pmhip_logit_divergence): for every scored row r, with
// p = softmax(a_r) and q = softmax(b_r), each over its own row,
//     kind 0 (tv)        d = 1/2 sum_i |p_i - q_i|
//     kind 1 (jeffreys)  d = sum_i (p_i - q_i) (log p_i - log q_i)            = KL(p || q) + KL(q || p)
// An HBM-bound row kernel of the family of masked_ce (loss.hip) and sample_rows_forced (sample.hip): every logits element is
// requested from memory ONCE and both passes -- the maxima and normalisers, then the sum over the columns -- run from registers.
//
// RESIDENCY.  A row pair belongs to WAVES waves; lane l of wave w holds, of BOTH rows, the float4 groups g = 0 .. G - 1 at columns
// ((g * WAVES + w) * 64 + l) * 4 .. + 3.  Four classes, by V:
//     V <= 256    G = 1, one wave per pair,    four pairs per workgroup       V <= 8192    G = 8, four waves per pair,  one pair per workgroup
//     V <= 1024   G = 4, one wave per pair,    four pairs per workgroup       V <= 16384   G = 8, eight waves per pair, one pair per workgroup
// so no lane holds more than 64 registers of logits (one wave cannot hold two rows of 8192: one such row is masked_ce's 128).  Jeffreys
// keeps a third value per column pair, rn(rn(a_i - ma) - rn(b_i - mb)), because the e_i replace the logits in place: its two wide
// classes are G = 4 with eight and sixteen waves per pair, 48 registers a lane.
// The waves of a pair exchange five words each through LDS: the two maxima, the two sums, the partial result.  Where a workgroup
// meets a barrier it serves ONE pair, so the early return of an unscored row is uniform over every thread that would meet it; the
// classes with four pairs per workgroup have no barrier at all (one wave reduces by DPP alone).
//
// AN UNSCORED ROW (ids given and ids[r] != mask_id) returns in front of its loads: its logits are never requested, a NaN there
// reaches nothing, and the launch costs the scored rows' bytes.
//
// EVALUATION ORDER.  Both rows run through the SAME explicitly rounded operations (no contraction, no re-association):
//     m = max over the row's own columns                      e_i = exp2(rn(rn(x_i - m) log2 e))            s = sum e_i
//     r = rn(1 / s)                                           p_i = rn(e_i r)
// the sums per lane over its groups in order, each group as (x + y) + (z + w), then the wave butterfly, then the waves in order.
//     tv        t_i = |rn(p_i - q_i)|
//     jeffreys  t_i = rn( rn(p_i - q_i) * rn( rn(rn(a_i - ma) - rn(b_i - mb)) - rn(log sa - log sb) ) )
// and d = the same ordered sum of t_i (times 1/2 for tv, exact).  Two things follow, and both are part of the contract:
//   * a == b row-wise gives exactly 0: p_i and q_i are the same bits, every difference is +0, every t_i is +0;
//   * swapping a and b gives the same bits: rn(x - y) = -rn(y - x) exactly, so every difference changes its sign and nothing else,
//     |.| and the product of two negated factors are unchanged, and the order of the sums does not depend on the operands.
// A column that is -inf in both rows has t_i = 0 by a select (its difference of shifted logits is inf - inf, both e_i exactly 0); a
// column that is -inf in exactly one row makes jeffreys +inf by a select (the mathematics; p_i - q_i may have underflowed to 0
// there) and is an ordinary column under tv.  Columns [V, G * WAVES * 256) are initialised to -inf in both rows: they take part in
// neither maximum nor sum.
// A NaN in a scored row reaches its sum of e_i and with it every p_i: the row's result is NaN.
//
// One writer per row (lane 0 of the pair's first wave), no atomics: two launches give the same bits.
#include "common.h"

// The order above is the contract: no product may be fused into the subtraction or addition behind it (rn(e_a r_a) - rn(e_b r_b) as
// fma(e_a, r_a, -rn(e_b r_b)) leaves the rounding error of one product where a == b must give 0, and is not symmetric in a and b).
// The arithmetic of this file is therefore written with the operators below, under a pragma that forbids contraction (the
// __f*_rn functions of the HIP headers are plain operators compiled where contraction is allowed: the compiler fuses through them).
#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ float add_rn(float x, float y) { return x + y; }
__device__ __forceinline__ float sub_rn(float x, float y) { return x - y; }
__device__ __forceinline__ float mul_rn(float x, float y) { return x * y; }
__device__ __forceinline__ float exp_below(float x, float m) { return __builtin_amdgcn_exp2f(mul_rn(sub_rn(x, m), PM_LOG2E)); }     // softmax_exp_below's

constexpr int KIND_TV = 0, KIND_JEFFREYS = 1;
// jeffreys holds three registers per column pair where tv holds two: its wide classes halve the groups and double the waves
#define KIND_JEFFREYS_G(G) ((G) == 8 ? 4 : (G))
#define KIND_JEFFREYS_WAVES(G, WAVES) ((G) == 8 ? 2 * (WAVES) : (WAVES))

__device__ __forceinline__ float max4(const float4& v) { return fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)); }

// the row's e_i in place of its logits (x <- e) -> this lane's sum
template <int G>
__device__ __forceinline__ float exp_below_row(float4 (&x)[G], float m) {
    float s = 0.f;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        x[g] = make_float4(exp_below(x[g].x, m), exp_below(x[g].y, m), exp_below(x[g].z, m), exp_below(x[g].w, m));
        s = add_rn(s, add_rn(add_rn(x[g].x, x[g].y), add_rn(x[g].z, x[g].w)));
    }
    return s;
}

__device__ __forceinline__ float tv_term(float ea, float ra, float eb, float rb) {
    return fabsf(sub_rn(mul_rn(ea, ra), mul_rn(eb, rb)));
}
// dd = rn(rn(a_i - ma) - rn(b_i - mb)): +-inf where exactly one logit is -inf, NaN (with both e exactly 0) where both are;
// dl = rn(log sa - log sb)
__device__ __forceinline__ float jeffreys_term(float ea, float ra, float eb, float rb, float dd, float dl) {
    const float t = mul_rn(sub_rn(mul_rn(ea, ra), mul_rn(eb, rb)), sub_rn(dd, dl));
    return fabsf(dd) == INFINITY ? INFINITY : (dd != dd && ea == 0.f && eb == 0.f) ? 0.f : t;
}
__device__ __forceinline__ float sub_below(float xa, float ma, float xb, float mb) { return sub_rn(sub_rn(xa, ma), sub_rn(xb, mb)); }

// combine one word per wave of a pair, in wave order; every thread of the workgroup calls it (a barrier inside)
template <int WAVES, bool MAX>
__device__ __forceinline__ float across_waves(float v, float* slot, int wave, int lane) {
    if (lane == 0) slot[wave] = v;
    __syncthreads();
    float r = slot[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) r = MAX ? fmaxf(r, slot[w]) : add_rn(r, slot[w]);
    return r;
}

template <int G, int WAVES, int PAIRS, int KIND>
__global__ __launch_bounds__(64 * WAVES * PAIRS) void logit_divergence_kernel(const float* __restrict__ a, const float* __restrict__ b, int ldl,
                                                                             const int64_t* __restrict__ ids, int64_t mask_id,
                                                                             float* __restrict__ acc, int32_t* __restrict__ count,
                                                                             int accumulate, int M, int V) {
    static_assert(WAVES == 1 || PAIRS == 1, "a workgroup that meets a barrier serves one pair");
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wave = WAVES == 1 ? 0 : wid;
    const int row = WAVES == 1 ? blockIdx.x * PAIRS + wid : blockIdx.x;
    if (row >= M) return;                                      // (WAVES > 1: the grid has M workgroups, never taken)
    if (ids != nullptr && ids[row] != mask_id) {               // uniform over the pair's waves: in front of every load and barrier
        if (!accumulate && wave == 0 && lane == 0) {
            acc[row] = 0.f;
            if (count != nullptr) count[row] = 0;
        }
        return;
    }
    const float* ar = a + (size_t)row * ldl;
    const float* br = b + (size_t)row * ldl;
    float4 xa[G], xb[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int col = ((g * WAVES + wave) * 64 + lane) * 4;
        xa[g] = xb[g] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        if (col < V) {
            xa[g] = *reinterpret_cast<const float4*>(ar + col);
            xb[g] = *reinterpret_cast<const float4*>(br + col);
        }
    }
    __shared__ float lds[WAVES == 1 ? 1 : 5 * WAVES];          // five exchanges, a set of words each: nothing is reused
    float ma = -INFINITY, mb = -INFINITY;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        ma = fmaxf(ma, max4(xa[g]));
        mb = fmaxf(mb, max4(xb[g]));
    }
    ma = wave_max(ma);
    mb = wave_max(mb);
    if (WAVES > 1) {
        ma = across_waves<WAVES, true>(ma, lds, wave, lane);
        mb = across_waves<WAVES, true>(mb, lds + WAVES, wave, lane);
    }
    constexpr bool KEEP = KIND == KIND_JEFFREYS;                 // jeffreys keeps the difference of the two shifted logits beside the e_i
    float4 dd[KEEP ? G : 1];
#pragma unroll
    for (int g = 0; g < (KEEP ? G : 0); ++g)
        dd[g] = make_float4(sub_below(xa[g].x, ma, xb[g].x, mb), sub_below(xa[g].y, ma, xb[g].y, mb), sub_below(xa[g].z, ma, xb[g].z, mb),
                            sub_below(xa[g].w, ma, xb[g].w, mb));
    float sa = wave_sum(exp_below_row<G>(xa, ma));
    float sb = wave_sum(exp_below_row<G>(xb, mb));
    if (WAVES > 1) {
        sa = across_waves<WAVES, false>(sa, lds + 2 * WAVES, wave, lane);
        sb = across_waves<WAVES, false>(sb, lds + 3 * WAVES, wave, lane);
    }
    const float ra = 1.f / sa, rb = 1.f / sb;
    float d = 0.f;
    if (KIND == KIND_TV) {
#pragma unroll
        for (int g = 0; g < G; ++g)
            d = add_rn(d, add_rn(add_rn(tv_term(xa[g].x, ra, xb[g].x, rb), tv_term(xa[g].y, ra, xb[g].y, rb)),
                                       add_rn(tv_term(xa[g].z, ra, xb[g].z, rb), tv_term(xa[g].w, ra, xb[g].w, rb))));
    } else {
        const float dl = sub_rn(logf(sa), logf(sb));
#pragma unroll
        for (int g = 0; g < (KEEP ? G : 0); ++g)
            d = add_rn(d, add_rn(add_rn(jeffreys_term(xa[g].x, ra, xb[g].x, rb, dd[g].x, dl), jeffreys_term(xa[g].y, ra, xb[g].y, rb, dd[g].y, dl)),
                                       add_rn(jeffreys_term(xa[g].z, ra, xb[g].z, rb, dd[g].z, dl), jeffreys_term(xa[g].w, ra, xb[g].w, rb, dd[g].w, dl))));
    }
    d = wave_sum(d);
    if (WAVES > 1) d = across_waves<WAVES, false>(d, lds + 4 * WAVES, wave, lane);
    if (KIND == KIND_TV) d = mul_rn(0.5f, d);
    if (wave == 0 && lane == 0) {
        if (accumulate) {
            acc[row] = add_rn(acc[row], d);
            if (count != nullptr) count[row] += 1;
        } else {
            acc[row] = d;
            if (count != nullptr) count[row] = 1;
        }
    }
}

template <int G, int WAVES, int PAIRS, int KIND>
void launch(const float* a, const float* b, int ldl, const int64_t* ids, int64_t mask_id, float* acc, int32_t* count, int accumulate, int M, int V,
            hipStream_t s) {
    hipLaunchKernelGGL((logit_divergence_kernel<G, WAVES, PAIRS, KIND>), dim3(ceil_div(M, PAIRS)), dim3(64 * WAVES * PAIRS), 0, s, a, b, ldl, ids,
                       mask_id, acc, count, accumulate, M, V);
}

}  // namespace

extern "C" int pmhip_logit_divergence(const float* a, const float* b, int ldl, const int64_t* ids, int64_t mask_id, int kind, float* acc,
                                      int32_t* count, int accumulate, int M, int V, pmhip_stream stream) {
    PM_REQUIRE(a, "logit_divergence: a is NULL");
    PM_REQUIRE(b, "logit_divergence: b is NULL");
    PM_REQUIRE(acc, "logit_divergence: acc is NULL");
    PM_REQUIRE(pm_aligned(16, {a, b}), "logit_divergence: a and b must be 16-byte aligned (float4 loads)");
    PM_REQUIRE(M > 0, "logit_divergence: M=%d must be positive", M);
    PM_REQUIRE(V > 0 && V % 4 == 0 && V <= 16384, "logit_divergence: V=%d must be a multiple of 4 in (0, 16384]", V);
    PM_REQUIRE(ldl % 4 == 0 && ldl >= V, "logit_divergence: ldl=%d must be a multiple of 4 and at least V=%d", ldl, V);
    PM_REQUIRE(kind == KIND_TV || kind == KIND_JEFFREYS, "logit_divergence: kind=%d is neither 0 (tv) nor 1 (jeffreys)", kind);
    hipStream_t s = (hipStream_t)stream;
    PmTimer tm(FAM_SAMPLE, s);
#define PM_DIV(G, WAVES, PAIRS)                                                                                        \
    (kind == KIND_TV ? launch<G, WAVES, PAIRS, KIND_TV>(a, b, ldl, ids, mask_id, acc, count, accumulate, M, V, s) \
                     : launch<KIND_JEFFREYS_G(G), KIND_JEFFREYS_WAVES(G, WAVES), PAIRS, KIND_JEFFREYS>(a, b, ldl, ids, mask_id, acc, count, accumulate, M, V, s))
    if (V <= 256) PM_DIV(1, 1, 4);
    else if (V <= 1024) PM_DIV(4, 1, 4);
    else if (V <= 8192) PM_DIV(8, 4, 1);
    else PM_DIV(8, 8, 1);
#undef PM_DIV
    PM_HIP(hipGetLastError());
    return PMHIP_OK;
}
