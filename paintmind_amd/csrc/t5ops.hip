// The three operators a Flan-T5 encoder needs beside the generic GEMMs: T5's RMS norm, its gated GELU, and
// self-attention with the relative-position bias.  The row kernels are one pass with 16-byte accesses; the attention kernel is one
// wave per 16 query rows of one (image, head), no LDS and no barrier.
#include <math.h>

#include "attn_wave16.h"
#include "common.h"

namespace {

constexpr int THREADS = 256;

// ------------------------------------------------------------------------------------------------
// T5LayerNorm: out = weight * (x * rsqrt(mean(x^2) + eps)); no mean subtraction, no bias.  One wave per row, the row (D <= 256 * NV4
// floats) in registers: read once.  The sum of squares is a chain per lane over its NV4 chunks (pairwise inside a chunk), then the
// wave butterfly.
// ------------------------------------------------------------------------------------------------
template <typename OutT, int NV4>
__global__ __launch_bounds__(THREADS) void rmsnorm_kernel(const float* __restrict__ x, const float* __restrict__ weight, float eps,
                                                          OutT* __restrict__ out, int M, int D) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* xr = x + (size_t)row * D;
    OutT* orow = out + (size_t)row * D;
    float4 v[NV4];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV4; ++i) {
        const int c0 = (i * 64 + lane) * 4;
        v[i] = c0 < D ? *reinterpret_cast<const float4*>(xr + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
        s += (v[i].x * v[i].x + v[i].y * v[i].y) + (v[i].z * v[i].z + v[i].w * v[i].w);
    }
    const float r = 1.0f / sqrtf(wave_sum(s) / (float)D + eps);
#pragma unroll
    for (int i = 0; i < NV4; ++i) {
        const int c0 = (i * 64 + lane) * 4;
        if (c0 < D) {
            const float4 w = *reinterpret_cast<const float4*>(weight + c0);
            store4(orow + c0, w.x * (v[i].x * r), w.y * (v[i].y * r), w.z * (v[i].z * r), w.w * (v[i].w * r));
        }
    }
}

template <typename OutT>
int launch_rmsnorm(const float* x, const float* w, float eps, void* out, int M, int D, hipStream_t s) {
    dim3 grid(ceil_div(M, THREADS / 64)), block(THREADS);
    OutT* o = reinterpret_cast<OutT*>(out);
    PmTimer tm(FAM_LAYERNORM, s);
    if (D <= 1024) hipLaunchKernelGGL((rmsnorm_kernel<OutT, 4>), grid, block, 0, s, x, w, eps, o, M, D);
    else if (D <= 2048) hipLaunchKernelGGL((rmsnorm_kernel<OutT, 8>), grid, block, 0, s, x, w, eps, o, M, D);
    else hipLaunchKernelGGL((rmsnorm_kernel<OutT, 16>), grid, block, 0, s, x, w, eps, o, M, D);
    PM_HIP(hipGetLastError());
    return PMHIP_OK;
}

// ------------------------------------------------------------------------------------------------
// Gated GELU: out[m,j] = gelu_new(u[m,j]) * u[m,F+j].  gelu_new(x) = 0.5 x (1 + tanh(z)), z = sqrt(2/pi) (x + 0.044715 x^3), is
// evaluated as x / (1 + e^(-2z)) -- the same function (1 + tanh z = 2 / (1 + e^(-2z))) without the cancellation of 1 + tanh(z)
// at negative z, and with no NaN where x^3 overflows: z = +-inf gives e^(-2z) = 0 or inf and the quotient x or -0.
// One thread = 4 consecutive columns.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float gelu_new(float x) {
    const float z = 0.7978845608028654f * (x + 0.044715f * (x * x * x));
    return x / (1.0f + expf(-2.0f * z));
}

template <typename OutT>
__global__ __launch_bounds__(THREADS) void geglu_kernel(const float* __restrict__ u, int ldu, OutT* __restrict__ out, int ldo, int M, int F) {
    const int f4 = F / 4;
    const size_t idx = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (idx >= (size_t)M * f4) return;
    const size_t m = idx / f4;
    const int j = (int)(idx % f4) * 4;
    const float4 a = *reinterpret_cast<const float4*>(u + m * ldu + j);
    const float4 g = *reinterpret_cast<const float4*>(u + m * ldu + F + j);
    store4(out + m * ldo + j, gelu_new(a.x) * g.x, gelu_new(a.y) * g.y, gelu_new(a.z) * g.z, gelu_new(a.w) * g.w);
}

// ------------------------------------------------------------------------------------------------
// Self-attention with T5's relative-position bias.  One wave serves 16 queries of one (image, head) and walks the keys in blocks of
// KB = 32 (bf16) / 16 (f32), flash style with an exact running maximum.  Fragment maps (common.h, Mma): the score tile is computed
// TRANSPOSED, S^T = K . Q^T, so a lane holds S[key 4g + r, query c] (g = lane >> 4, c = lane & 15) in acc[r] -- the query is the
// lane's column through the whole kernel: the row maximum and sum are a reduction over r and over the four lanes {c, c+16, c+32,
// c+48}, and the probabilities the lane holds ARE its 16-byte operand chunk of P for O^T = V^T . P^T (chunk element e <-> key
// 16 (e / 4) + 4 g + e % 4 of the block; the V^T operand is read from memory in the same order).  Nothing is transposed through LDS.
//   O^T tile dt: acc[r] = O[query c, dim 16 dt + 4 g + r] -> one 4-element store per tile.
// Keys >= n (the image's count) get the score -inf; their K rows are never read (the row index is clamped to n - 1) and their V^T
// elements are replaced by 0 on load (0 * NaN is NaN).  Queries >= L of the last tile repeat row L - 1 and are not stored.
// pack_probs and load_vt live in attn_wave16.h: the causal kernel of clipops.hip uses them too.
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(64) void attention_relbias_kernel(const T* __restrict__ Q, const T* __restrict__ K, const T* __restrict__ Vt,
                                                               T* __restrict__ out, int ldo, int heads, int L, int L_pad,
                                                               const float* __restrict__ rel_bias, const int* __restrict__ kv_lens) {
    constexpr int E = Mma<T>::kElemsPerChunk;       // elements of a 16-byte chunk: 8 (bf16) / 4 (f32)
    constexpr int NT = E / 4;                       // 16-key tiles of a block
    constexpr int KB = 16 * NT;                     // keys of a block
    constexpr int DS = 64 / (4 * E);                // chunks of a 64-wide Q / K row per lane
    const int lane = threadIdx.x, g = lane >> 4, c = lane & 15;
    const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * 16;
    const int n = kv_lens ? min(max(kv_lens[b], 1), L) : L;
    const size_t bh = (size_t)b * heads + h;
    const T* Qp = Q + bh * L * 64;
    const T* Kp = K + bh * L_pad * 64;
    const T* Vp = Vt + bh * 64 * L_pad;
    const float* bias = rel_bias + (size_t)h * (2 * L - 1) + (L - 1);
    const int qc = min(q0 + c, L - 1);

    uint4 qf[DS];
#pragma unroll
    for (int s = 0; s < DS; ++s) qf[s] = *reinterpret_cast<const uint4*>(Qp + (size_t)qc * 64 + s * 4 * E + g * E);

    f32x4_t o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;

    for (int k0 = 0; k0 < n; k0 += KB) {
        f32x4_t sc[NT];
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int kr = min(k0 + 16 * t + c, n - 1);
            f32x4_t acc = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < DS; ++s) {
                const uint4 kf = *reinterpret_cast<const uint4*>(Kp + (size_t)kr * 64 + s * 4 * E + g * E);
                Mma<T>::run(acc, kf, qf[s]);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = k0 + 16 * t + 4 * g + r;
                const float sv = key < n ? acc[r] + bias[min(key, n - 1) - qc] : -INFINITY;
                sc[t][r] = sv;
                mx = fmaxf(mx, sv);
            }
        }
        mx = group4_max(mx);
        const float m_new = fmaxf(m, mx);           // finite from the first block on: key 0 is always allowed
        const float alpha = softmax_exp_below(m, m_new);
        float ps = 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                sc[t][r] = softmax_exp_below(sc[t][r], m_new);
                ps += sc[t][r];
            }
        l = l * alpha + group4_sum(ps);
        m = m_new;
        const uint4 pf = pack_probs<T>(sc);
        const bool full = k0 + KB <= n;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            const uint4 vf = load_vt(Vp + (size_t)(16 * dt + c) * L_pad, k0, g, n, full);
#pragma unroll
            for (int r = 0; r < 4; ++r) o[dt][r] *= alpha;
            Mma<T>::run(o[dt], vf, pf);
        }
    }
    if (q0 + c < L) {
        const float inv = 1.0f / l;
        T* orow = out + ((size_t)b * L + q0 + c) * ldo + h * 64 + 4 * g;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) store4(orow + 16 * dt, o[dt][0] * inv, o[dt][1] * inv, o[dt][2] * inv, o[dt][3] * inv);
    }
}

template <typename T>
int launch_relbias(const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads, int L, int L_pad, const float* rel_bias,
                   const int* kv_lens, hipStream_t s) {
    dim3 grid(ceil_div(L, 16), heads, B), block(64);
    PmTimer tm(FAM_ATTENTION, s);
    hipLaunchKernelGGL((attention_relbias_kernel<T>), grid, block, 0, s, reinterpret_cast<const T*>(Q), reinterpret_cast<const T*>(K),
                       reinterpret_cast<const T*>(Vt), reinterpret_cast<T*>(out), ldo, heads, L, L_pad, rel_bias, kv_lens);
    PM_HIP(hipGetLastError());
    return PMHIP_OK;
}

}  // namespace

extern "C" int pmhip_rmsnorm(const float* x, const float* weight, float eps, void* out, int out_dtype, int M, int D, pmhip_stream stream) {
    PM_REQUIRE(x && weight && out, "rmsnorm: null pointer");
    PM_REQUIRE(M > 0, "rmsnorm: M=%d must be positive", M);
    PM_REQUIRE(D >= 4 && D <= 4096 && D % 4 == 0, "rmsnorm: D=%d must be a multiple of 4 in [4, 4096]", D);
    PM_REQUIRE(eps >= 0.f, "rmsnorm: eps=%g must not be negative", (double)eps);
    hipStream_t s = (hipStream_t)stream;
    if (out_dtype == PMHIP_F32) return launch_rmsnorm<float>(x, weight, eps, out, M, D, s);
    if (out_dtype == PMHIP_BF16) return launch_rmsnorm<bf16_t>(x, weight, eps, out, M, D, s);
    pm_set_error("rmsnorm: bad out_dtype %d", out_dtype);
    return PMHIP_EINVAL;
}

extern "C" int pmhip_geglu(const float* u, int ldu, void* out, int ldo, int out_dtype, int M, int F, pmhip_stream stream) {
    PM_REQUIRE(u && out, "geglu: null pointer");
    PM_REQUIRE(out_dtype == PMHIP_F32 || out_dtype == PMHIP_BF16, "geglu: bad out_dtype %d", out_dtype);
    PM_REQUIRE(M > 0 && F > 0 && F % 4 == 0, "geglu: bad shape M=%d F=%d (F must be a multiple of 4)", M, F);
    PM_REQUIRE(ldu >= 2 * F && ldu % 4 == 0, "geglu: ldu=%d must be a multiple of 4 >= 2F=%d", ldu, 2 * F);
    PM_REQUIRE(ldo >= F && ldo % 4 == 0, "geglu: ldo=%d must be a multiple of 4 >= F=%d", ldo, F);
    PM_REQUIRE(pm_aligned(16, {u}) && pm_aligned(out_dtype == PMHIP_F32 ? 16 : 8, {out}), "geglu: u / out must be 16-byte / 4-element aligned");
    hipStream_t s = (hipStream_t)stream;
    const size_t total = (size_t)M * (F / 4);
    PM_REQUIRE(total <= 0x7fffffffull * THREADS, "geglu: M*F too large");
    dim3 grid((unsigned)((total + THREADS - 1) / THREADS)), block(THREADS);
    PmTimer tm(FAM_ROWOPS, s);
    if (out_dtype == PMHIP_F32) hipLaunchKernelGGL((geglu_kernel<float>), grid, block, 0, s, u, ldu, reinterpret_cast<float*>(out), ldo, M, F);
    else hipLaunchKernelGGL((geglu_kernel<bf16_t>), grid, block, 0, s, u, ldu, reinterpret_cast<bf16_t*>(out), ldo, M, F);
    PM_HIP(hipGetLastError());
    return PMHIP_OK;
}

extern "C" int pmhip_attention_relbias(int dtype, const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads, int L,
                                       int L_pad, const float* rel_bias, const int32_t* kv_lens, pmhip_stream stream) {
    PM_REQUIRE(dtype == PMHIP_F32 || dtype == PMHIP_BF16, "attention_relbias: bad dtype %d", dtype);
    PM_REQUIRE(Q && K && Vt && out, "attention_relbias: null pointer (Q, K, Vt or out)");
    PM_REQUIRE(rel_bias, "attention_relbias: rel_bias is NULL (the [heads][2L-1] table; pmhip_attention_dh is the entry without a bias)");
    PM_REQUIRE(B > 0 && B <= 65535 && heads > 0 && heads <= 65535, "attention_relbias: B=%d and heads=%d must be in [1, 65535]", B, heads);
    PM_REQUIRE(L >= 1 && L <= (1 << 20), "attention_relbias: L=%d must be in [1, 2^20]", L);
    PM_REQUIRE(L_pad >= L && L_pad % 4 == 0, "attention_relbias: L_pad=%d must be a multiple of 4 >= L=%d", L_pad, L);
    PM_REQUIRE(ldo >= heads * 64 && ldo % 4 == 0, "attention_relbias: ldo=%d must be a multiple of 4 >= heads*64=%d", ldo, heads * 64);
    PM_REQUIRE(pm_aligned(16, {Q, K, Vt}) && pm_aligned(dtype == PMHIP_F32 ? 16 : 8, {out}),
               "attention_relbias: Q, K, Vt must be 16-byte aligned and out 4-element aligned");
    hipStream_t s = (hipStream_t)stream;
    if (dtype == PMHIP_F32) return launch_relbias<float>(Q, K, Vt, out, ldo, B, heads, L, L_pad, rel_bias, kv_lens, s);
    return launch_relbias<bf16_t>(Q, K, Vt, out, ldo, B, heads, L, L_pad, rel_bias, kv_lens, s);
}
